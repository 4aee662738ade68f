"""RGB-D front end: a sensor's 16-bit depth image and 8-bit colour image become landmarks on the device (include/icp_amd.h: icp_rgbd_t,
icp_set_rgbd, icp_write_rgbd, icp_kernel_rgbd, icp_track_submit_rgbd, icp_track_next_rgbd).

The functions work on an ICP / ICPStep object; the classes themselves keep the surface they have.

    python -m icp_amd.rgbd DEPTH.raw RGB.raw OUT.bin [--radius R --range S ...]

turns a raw little-endian u16 / u8 image pair (640 x 480) into the reference's pc8d file (io.save_pc8d), which icp_amd.register reads."""
import argparse
import ctypes as C
import sys

import numpy as np

import icp_amd
from icp_amd import io


class icp_rgbd_t(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("depth_scale", C.c_float),
                ("d_min", C.c_uint32), ("d_max", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("step_x", C.c_uint32), ("step_y", C.c_uint32),
                ("radius", C.c_uint32), ("range", C.c_uint32)]


class RGBDConfig:
    """icp_rgbd_t: the image size, the pinhole model, the valid counts, the landmark lattice and the depth filter.  The defaults are the
    header's table: the reference's unfiltered writer followed by getLMs on a 640 x 480 Kinect frame."""
    FIELDS = tuple(name for name, _ in icp_rgbd_t._fields_)

    def __init__(self, width=640, height=480, fx=595.0, fy=595.0, cx=319.5, cy=239.5, depth_scale=1.0, d_min=1, d_max=65535,
                 x0=65, y0=49, step_x=4, step_y=3, radius=0, range=30):
        self.width, self.height = width, height
        self.fx, self.fy, self.cx, self.cy = fx, fy, cx, cy
        self.depth_scale = depth_scale
        self.d_min, self.d_max = d_min, d_max
        self.x0, self.y0, self.step_x, self.step_y = x0, y0, step_x, step_y
        self.radius, self.range = radius, range

    @classmethod
    def kinect(cls):
        return cls()

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, RGBDConfig) and self._c_bytes() == other._c_bytes()

    def __repr__(self):
        return "RGBDConfig(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())

    def _c(self):
        return icp_rgbd_t(*[getattr(self, f) for f in self.FIELDS])

    def _c_bytes(self):
        return bytes(self._c())

    @classmethod
    def _from_c(cls, c):
        return cls(**{f: getattr(c, f) for f in cls.FIELDS})


_declared = None


def _lib():
    """The engine's library with the front end's entry points declared."""
    global _declared
    L = icp_amd.lib()
    if _declared is not L:
        vp, i32, u32p, i32p, cfg = C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(icp_rgbd_t)
        for name, args in (("icp_set_rgbd", (vp, cfg)), ("icp_get_rgbd", (vp, cfg)),
                           ("icp_write_rgbd", (vp, i32, vp, vp, i32, i32)),
                           ("icp_kernel_rgbd", (i32, cfg, vp, vp, vp, vp)),
                           ("icp_time_rgbd", (vp, i32, i32, vp, vp, C.c_uint32, C.POINTER(C.c_float))),
                           ("icp_track_submit_rgbd", (vp, vp, vp, i32)),
                           ("icp_track_next_rgbd", (vp, vp, vp, i32, u32p, i32p))):
            f = getattr(L, name)
            f.restype, f.argtypes = i32, list(args)
        _declared = L
    return L


def _images(depth, rgb, width, height):
    """The two images as contiguous arrays of the configured size (rgb may be None); shape and dtype are checked, nothing is converted."""
    depth = np.asarray(depth)
    if depth.dtype != np.uint16 or depth.size != width * height:
        raise ValueError("expected a %d x %d uint16 depth image" % (width, height))
    depth = np.ascontiguousarray(depth)
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.size != width * height * 3:
            raise ValueError("expected a %d x %d x 3 uint8 colour image" % (width, height))
        rgb = np.ascontiguousarray(rgb)
    return depth, rgb


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _handle(icp, what):
    if isinstance(icp, icp_amd._PyramidLevel):
        icp._refuse(what)
    return icp


def to_cloud(depth, rgb=None, cfg=None, normals=False, device=0):
    """The dense form (icp_kernel_rgbd): every pixel's float8 point, (height * width, 8) float32 — and, with normals, the
    (height * width, 4) normals of the vertex map as the second element of a pair.  The lattice fields of cfg are ignored."""
    cfg = cfg or RGBDConfig()
    depth, rgb = _images(depth, rgb, cfg.width, cfg.height)
    L = _lib()
    n = cfg.width * cfg.height
    cloud = np.empty((n, 8), np.float32)
    nrm = np.empty((n, 4), np.float32) if normals else None
    c = cfg._c()
    rc = L.icp_kernel_rgbd(device, C.byref(c), _ptr(depth), _ptr(rgb), _ptr(cloud), _ptr(nrm))
    if rc:
        raise icp_amd.ICPError(rc, L.icp_kernel_last_error().decode())
    return (cloud, nrm) if normals else cloud


def set_config(icp, cfg=None):
    """icp_set_rgbd: the handle's configuration (None: the defaults); it survives init as the other settings do."""
    c = (cfg or RGBDConfig())._c()
    icp._chk(_lib().icp_set_rgbd(icp._h, C.byref(c)))


def get_config(icp):
    c = icp_rgbd_t()
    icp._chk(_lib().icp_get_rgbd(icp._h, C.byref(c)))
    return RGBDConfig._from_c(c)


def write(icp, which, depth, rgb=None, normals=False):
    """icp_write_rgbd: the landmarks of an image pair into F or M (which = Memory.F / Memory.M), with normals also into NORMALS_F / NORMALS_M."""
    _handle(icp, "write of images into a level")
    cfg = get_config(icp)
    depth, rgb = _images(depth, rgb, cfg.width, cfg.height)
    icp._chk(_lib().icp_write_rgbd(icp._h, which, _ptr(depth), _ptr(rgb), int(bool(normals)), 1))


def track_submit(icp, depth, rgb=None, warm_start=False):
    """icp_track_submit_rgbd: enqueues a frame given as images; track_collect of the object collects it, as it does a float8 frame."""
    _handle(icp, "tracking on a level")
    cfg = get_config(icp)
    depth, rgb = _images(depth, rgb, cfg.width, cfg.height)
    icp._chk(_lib().icp_track_submit_rgbd(icp._h, _ptr(depth), _ptr(rgb), int(warm_start)))


def track_next(icp, depth, rgb=None, warm_start=False):
    """icp_track_next_rgbd: submit + collect (blocking); k once there is a previous frame to register against, else None."""
    _handle(icp, "tracking on a level")
    cfg = get_config(icp)
    depth, rgb = _images(depth, rgb, cfg.width, cfg.height)
    k, registered = C.c_uint32(), C.c_int()
    icp._chk(_lib().icp_track_next_rgbd(icp._h, _ptr(depth), _ptr(rgb), int(warm_start), C.byref(k), C.byref(registered)))
    return k.value if registered.value else None


def time_kernel(icp, dense, depth, rgb=None, normals=False, reps=20):
    """icp_time_rgbd (diagnostic): microseconds per launch of the dense (every pixel) or the lattice form alone, device events around `reps`
    launches; the handle's F, M and normals stay as they are."""
    cfg = get_config(icp)
    depth, rgb = _images(depth, rgb, cfg.width, cfg.height)
    us = C.c_float()
    icp._chk(_lib().icp_time_rgbd(icp._h, int(bool(dense)), int(bool(normals)), _ptr(depth), _ptr(rgb), reps, C.byref(us)))
    return us.value


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m icp_amd.rgbd",
                                 description="A raw 640 x 480 u16 depth / u8 RGB image pair -> the reference's pc8d cloud file.")
    ap.add_argument("depth", metavar="DEPTH.raw")
    ap.add_argument("rgb", metavar="RGB.raw", help="'-': no colour image")
    ap.add_argument("out", metavar="OUT.bin")
    for name, kind, text in (("fx", float, "focal length"), ("fy", float, "focal length"), ("cx", float, "principal point"),
                             ("cy", float, "principal point"), ("depth-scale", float, "engine units per count"),
                             ("d-min", int, "smallest valid count"), ("d-max", int, "largest valid count"),
                             ("radius", int, "filter radius, 0 .. 6 (0: no filter)"), ("range", int, "range cut-off in counts, 1 .. 4095")):
        ap.add_argument("--" + name, type=kind, default=None, help=text)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    cfg = RGBDConfig()
    for f in ("fx", "fy", "cx", "cy", "depth_scale", "d_min", "d_max", "radius", "range"):
        if getattr(a, f) is not None:
            setattr(cfg, f, getattr(a, f))
    depth = np.fromfile(a.depth, dtype="<u2")
    rgb = None if a.rgb == "-" else np.fromfile(a.rgb, dtype=np.uint8)
    try:
        cloud = to_cloud(depth, rgb, cfg, device=a.device)
    except (ValueError, icp_amd.ICPError) as e:
        print("icp_amd.rgbd: %s" % e, file=sys.stderr)
        return 1
    io.save_pc8d(a.out, cloud)
    return 0


if __name__ == "__main__":
    sys.exit(main())
