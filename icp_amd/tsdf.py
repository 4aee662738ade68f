"""Frame-to-model: a TSDF volume fused and ray-cast on the device (include/icp_amd.h: icp_tsdf_t, icp_tsdf_integrate, icp_tsdf_raycast,
icp_tsdf_raycast_to, icp_tsdf_compose_pose), and its surface as a point cloud (icp_tsdf_extract_surface) or a triangle mesh
(icp_tsdf_extract_mesh), and a cloud registered against the volume itself (icp_tsdf_register, icp_tsdf_register_from, track_to_volume),
and the moving volume: the window shifted by whole voxels on the device (icp_tsdf_shift), the surface that leaves it
(icp_tsdf_extract_surface_region, kept_box) and the rule that decides when to shift (follow).

    vol = TSDFVolume(TSDFConfig(256, 256, 256, voxel=8.0, origin=(-1024, -1024, 0), mu=24.0))
    for pose, k, scale in track_to_model(icp, vol, frames, pose0, 300.0, 4000.0):
        ...
    cloud, normals = vol.extract_surface()
    icp_amd.io.save_ply("model.ply", cloud, normals)
    cloud, normals, triangles = vol.extract_mesh()
    icp_amd.io.save_ply("mesh.ply", cloud, normals, triangles)

A pose is 12 floats, row-major [R | t], camera -> world.  A camera is an icp_amd.rgbd.RGBDConfig."""
import ctypes as C

import numpy as np

import icp_amd
from icp_amd import rgbd
from icp_amd.rgbd import _images, _ptr


class icp_tsdf_t(C.Structure):
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32), ("voxel", C.c_float), ("origin", C.c_float * 3),
                ("mu", C.c_float), ("w_max", C.c_float), ("colour", C.c_uint32)]


class icp_tsdf_surface_t(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("normals", C.c_uint32)]


class icp_tsdf_region_t(C.Structure):
    _fields_ = [("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("mode", C.c_uint32)]


REGION_INSIDE, REGION_OUTSIDE = 0, 1


class icp_tsdf_register_t(C.Structure):
    _fields_ = [("max_iterations", C.c_uint32), ("angle_threshold", C.c_double), ("translation_threshold", C.c_double)]


class icp_tsdf_registration_t(C.Structure):
    _fields_ = [("pose12", C.c_float * 12), ("iterations", C.c_uint32), ("converged", C.c_uint32), ("singular", C.c_uint32),
                ("members", C.c_uint32), ("rmse", C.c_double), ("sys", C.c_double * 27)]


class Registration:
    """icp_tsdf_registration_t: pose (12 float32), iterations, converged, singular, and of the last iteration evaluated members, rmse and
    sys (27 float64: the information matrix's upper triangle, then J^T r)."""

    def __init__(self, c):
        self.pose = np.array(c.pose12, np.float32)
        self.iterations, self.converged, self.singular, self.members = c.iterations, bool(c.converged), bool(c.singular), c.members
        self.rmse, self.sys = c.rmse, np.array(c.sys, np.float64)

    def __repr__(self):
        return "Registration(iterations=%d, converged=%s, singular=%s, members=%d, rmse=%r)" % (self.iterations, self.converged, self.singular, self.members, self.rmse)


ANGLE_THRESHOLD, TRANSLATION_THRESHOLD = 0.001, 0.01          # icp_tsdf_register's defaults: those of ICP.init


def _register_options(max_iterations, angle_threshold, translation_threshold):
    return icp_tsdf_register_t(max_iterations, ANGLE_THRESHOLD if angle_threshold is None else angle_threshold,
                               TRANSLATION_THRESHOLD if translation_threshold is None else translation_threshold)


class TSDFConfig:
    """icp_tsdf_t: nx x ny x nz voxels of edge `voxel`, voxel (0, 0, 0) centred at `origin`, truncation distance mu, weight cap w_max,
    and whether the volume keeps colour."""
    FIELDS = ("nx", "ny", "nz", "voxel", "origin", "mu", "w_max", "colour")

    def __init__(self, nx, ny, nz, voxel, origin, mu, w_max=64.0, colour=False):
        self.nx, self.ny, self.nz = nx, ny, nz
        self.voxel, self.origin, self.mu, self.w_max, self.colour = voxel, tuple(origin), mu, w_max, int(colour)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "TSDFConfig(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())

    def _c(self):
        return icp_tsdf_t(self.nx, self.ny, self.nz, self.voxel, (C.c_float * 3)(*self.origin), self.mu, self.w_max, self.colour)

    @classmethod
    def _from_c(cls, c):
        return cls(c.nx, c.ny, c.nz, c.voxel, tuple(c.origin), c.mu, c.w_max, c.colour)


_declared = None


def _lib():
    """The engine's library with the volume's entry points declared."""
    global _declared
    L = icp_amd.lib()
    if _declared is not L:
        vp, i32, u32, f32, cfg, cam = C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.POINTER(icp_tsdf_t), C.POINTER(rgbd.icp_rgbd_t)
        for name, args in (("icp_tsdf_create", (C.POINTER(vp), i32, cfg)), ("icp_tsdf_destroy", (vp,)), ("icp_tsdf_reset", (vp,)),
                           ("icp_tsdf_get_config", (vp, cfg)),
                           ("icp_tsdf_integrate", (vp, cam, vp, vp, vp)),
                           ("icp_tsdf_raycast", (vp, cam, vp, f32, f32, u32, vp, vp)),
                           ("icp_tsdf_raycast_to", (vp, vp, i32, cam, vp, f32, f32, i32)),
                           ("icp_tsdf_read", (vp, vp, vp)), ("icp_tsdf_write", (vp, vp, vp)),
                           ("icp_tsdf_compose_pose", (vp, vp, vp, C.POINTER(f32))),
                           ("icp_tsdf_extract_surface", (vp, C.POINTER(icp_tsdf_surface_t), u32, vp, vp, C.POINTER(u32))),
                           ("icp_tsdf_extract_mesh", (vp, C.POINTER(icp_tsdf_surface_t), u32, vp, vp, C.POINTER(u32), u32, vp, C.POINTER(u32))),
                           ("icp_tsdf_mesh_case", (u32, C.POINTER(u32), C.POINTER(C.c_uint8))),
                           ("icp_tsdf_register", (vp, C.POINTER(icp_tsdf_register_t), vp, u32, vp, C.POINTER(icp_tsdf_registration_t))),
                           ("icp_tsdf_register_from", (vp, C.POINTER(icp_tsdf_register_t), vp, i32, vp, C.POINTER(icp_tsdf_registration_t))),
                           ("icp_tsdf_shift", (vp, C.POINTER(C.c_int32))), ("icp_tsdf_get_window", (vp, C.POINTER(C.c_int32))),
                           ("icp_tsdf_extract_surface_region", (vp, C.POINTER(icp_tsdf_surface_t), C.POINTER(icp_tsdf_region_t), u32, vp, vp, C.POINTER(u32))),
                           ("icp_tsdf_kept_box", (cfg, C.POINTER(C.c_int32), C.POINTER(icp_tsdf_region_t))),
                           ("icp_tsdf_follow", (cfg, C.POINTER(f32), u32, C.POINTER(C.c_int32))),
                           ("icp_tsdf_time", (vp, i32, cam, vp, vp, vp, f32, f32, u32, u32, C.POINTER(f32)))):
            f = getattr(L, name)
            f.restype, f.argtypes = i32, list(args)
        L.icp_tsdf_last_error.restype, L.icp_tsdf_last_error.argtypes = C.c_char_p, [vp]
        _declared = L
    return L


def _pose(pose12):
    p = np.ascontiguousarray(pose12, np.float32).reshape(-1)
    if p.size != 12:
        raise ValueError("expected a pose of 12 floats, row-major [R | t]")
    return p


def compose_pose(pose12, T8):
    """icp_tsdf_compose_pose: (pose12 o (R (q), t) of the engine's T8 as 12 float32, T8's scale) — computed in double, rounded once."""
    p, T = _pose(pose12), np.ascontiguousarray(T8, np.float32).reshape(-1)
    if T.size != 8:
        raise ValueError("expected a transform of 8 floats [q | t, s]")
    out, s = np.empty(12, np.float32), C.c_float()
    rc = _lib().icp_tsdf_compose_pose(_ptr(p), _ptr(T), _ptr(out), C.byref(s))
    if rc:
        raise icp_amd.ICPError(rc, "icp_tsdf_compose_pose: the quaternion must be finite and non-zero")
    return out, s.value


def mesh_case(case_index):
    """icp_tsdf_mesh_case (host only): the case table's entry as a list of triangles, each a triple of local edge ids 4 a + m."""
    n, edges = C.c_uint32(), (C.c_uint8 * 15)()
    rc = _lib().icp_tsdf_mesh_case(case_index, C.byref(n), edges)
    if rc:
        raise icp_amd.ICPError(rc, "icp_tsdf_mesh_case: the case index must be at most 255")
    return [tuple(edges[3 * t:3 * t + 3]) for t in range(n.value)]


def _shift3(s):
    s = [int(x) for x in s]
    if len(s) != 3 or any(not -2 ** 31 <= x < 2 ** 31 for x in s):
        raise ValueError("expected a shift of three int32")
    return (C.c_int32 * 3)(*s)


def kept_box(cfg, s):
    """icp_tsdf_kept_box (host only): (lo, hi) of the box of voxels a shift by s keeps, lo_a = max (0, s_a), hi_a = max (lo_a, min (n_a,
    n_a + s_a)); the members of extract_surface_region (lo, hi, outside=True) are what the shift drops."""
    c, box = cfg._c(), icp_tsdf_region_t()
    rc = _lib().icp_tsdf_kept_box(C.byref(c), _shift3(s), C.byref(box))
    if rc:
        raise icp_amd.ICPError(rc, "icp_tsdf_kept_box: bad arguments")
    return tuple(box.lo), tuple(box.hi)


def follow(cfg, point, threshold):
    """icp_tsdf_follow (host only): the shift (three ints) that centres the window of cfg on `point` again, or (0, 0, 0) while the point
    is at most `threshold` voxels from the centre on every axis."""
    c, out = cfg._c(), (C.c_int32 * 3)()
    pt = np.ascontiguousarray(point, np.float32).reshape(-1)
    if pt.size != 3:
        raise ValueError("expected a point of 3 floats")
    rc = _lib().icp_tsdf_follow(C.byref(c), pt.ctypes.data_as(C.POINTER(C.c_float)), int(threshold), out)
    if rc:
        raise icp_amd.ICPError(rc, "icp_tsdf_follow: the point must be finite and within int32 voxels of the centre")
    return tuple(out)


class TSDFVolume:
    """A volume on device `device` (icp_tsdf_create).  Every call is blocking."""

    def __init__(self, cfg, device=0):
        self._L = _lib()
        self._t = C.c_void_p()
        c = cfg._c()
        rc = self._L.icp_tsdf_create(C.byref(self._t), device, C.byref(c))
        if rc:
            self._t = None
            raise icp_amd.ICPError(rc, self._L.icp_tsdf_last_error(None).decode())
        self.cfg = cfg
        self.device = device

    def close(self):
        if self._t:
            self._L.icp_tsdf_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc:
            raise icp_amd.ICPError(rc, self._L.icp_tsdf_last_error(self._t).decode())

    @property
    def shape(self):
        return (self.cfg.nz, self.cfg.ny, self.cfg.nx)

    def get_config(self):
        c = icp_tsdf_t()
        self._chk(self._L.icp_tsdf_get_config(self._t, C.byref(c)))
        return TSDFConfig._from_c(c)

    def reset(self):
        self._chk(self._L.icp_tsdf_reset(self._t))

    def integrate(self, cam, pose12, depth, rgb=None):
        """icp_tsdf_integrate: one frame (a uint16 depth image, a uint8 colour image or None) seen from pose12 into the volume."""
        depth, rgb = _images(depth, rgb, cam.width, cam.height)
        c = cam._c()
        self._chk(self._L.icp_tsdf_integrate(self._t, C.byref(c), _ptr(_pose(pose12)), _ptr(depth), _ptr(rgb)))

    def raycast(self, cam, pose12, z_near, z_far, side=0, normals=True):
        """icp_tsdf_raycast: the view from pose12 as (cloud (n, 8), normals (n, 4) or None) — every pixel (side = 0, n = width * height) or
        the side x side landmarks of the camera's lattice."""
        n = side * side if side else cam.width * cam.height
        cloud = np.empty((n, 8), np.float32)
        nrm = np.empty((n, 4), np.float32) if normals else None
        c = cam._c()
        self._chk(self._L.icp_tsdf_raycast(self._t, C.byref(c), _ptr(_pose(pose12)), z_near, z_far, side, _ptr(cloud), _ptr(nrm)))
        return cloud, nrm

    def raycast_to(self, icp, which, pose12, z_near, z_far, cam=None, normals=False):
        """icp_tsdf_raycast_to: the sqrt (m) x sqrt (m) landmarks of the view into F or M of `icp` (which = Memory.F / Memory.M), device to
        device; with normals also into NORMALS_F / NORMALS_M.  cam = None: the handle's RGB-D configuration."""
        rgbd._handle(icp, "a ray cast into a level")
        c = cam._c() if cam is not None else None
        self._chk(self._L.icp_tsdf_raycast_to(self._t, icp._h, which, C.byref(c) if c is not None else None, _ptr(_pose(pose12)),
                                              z_near, z_far, int(bool(normals))))

    def read(self):
        """icp_tsdf_read: (dw (nz, ny, nx, 2), rgb (nz, ny, nx, 3) or None without colour)."""
        dw = np.empty(self.shape + (2,), np.float32)
        col = np.empty(self.shape + (3,), np.float32) if self.cfg.colour else None
        self._chk(self._L.icp_tsdf_read(self._t, _ptr(dw), _ptr(col)))
        return dw, col

    def write(self, dw, rgb=None):
        """icp_tsdf_write: the whole volume from the layout read () returns."""
        dw = np.ascontiguousarray(dw, np.float32)
        if dw.size != 2 * np.prod(self.shape):
            raise ValueError("expected nz x ny x nx x 2 floats")
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.float32)
            if rgb.size != 3 * np.prod(self.shape):
                raise ValueError("expected nz x ny x nx x 3 floats")
        self._chk(self._L.icp_tsdf_write(self._t, _ptr(dw), _ptr(rgb)))

    def extract_surface(self, min_weight=1.0, normals=True, capacity=None):
        """icp_tsdf_extract_surface: the volume's surface as (cloud (n, 8), normals (n, 4) or None), the zero crossings of D on the edges
        between usable voxels in ascending 3 * (linear voxel index) + axis.  capacity = None: a counting call first, then every member.
        With a capacity: (cloud, normals, count) — the first min (count, capacity) members and the number there are."""
        opt, count = icp_tsdf_surface_t(min_weight, int(bool(normals))), C.c_uint32()
        if capacity is None:
            self._chk(self._L.icp_tsdf_extract_surface(self._t, C.byref(opt), 0, None, None, C.byref(count)))
            room = count.value
        else:
            room = int(capacity)
        cloud = np.empty((room, 8), np.float32)
        nrm = np.empty((room, 4), np.float32) if normals else None
        self._chk(self._L.icp_tsdf_extract_surface(self._t, C.byref(opt), room, _ptr(cloud) if room else None, _ptr(nrm) if room else None, C.byref(count)))
        n = min(count.value, room)
        if capacity is None:
            return cloud[:n], (nrm[:n] if normals else None)
        return cloud[:n], (nrm[:n] if normals else None), count.value

    def extract_surface_region(self, lo, hi, outside=False, min_weight=1.0, normals=True, capacity=None):
        """icp_tsdf_extract_surface_region: extract_surface's members with both ends in the box of voxels lo_a <= idx_a < hi_a (or, with
        `outside`, every other member), the same records in the same relative order; the capacity convention is extract_surface's."""
        opt, count = icp_tsdf_surface_t(min_weight, int(bool(normals))), C.c_uint32()
        box = icp_tsdf_region_t((C.c_uint32 * 3)(*lo), (C.c_uint32 * 3)(*hi), REGION_OUTSIDE if outside else REGION_INSIDE)
        if capacity is None:
            self._chk(self._L.icp_tsdf_extract_surface_region(self._t, C.byref(opt), C.byref(box), 0, None, None, C.byref(count)))
            room = count.value
        else:
            room = int(capacity)
        cloud = np.empty((room, 8), np.float32)
        nrm = np.empty((room, 4), np.float32) if normals else None
        self._chk(self._L.icp_tsdf_extract_surface_region(self._t, C.byref(opt), C.byref(box), room, _ptr(cloud) if room else None,
                                                          _ptr(nrm) if room else None, C.byref(count)))
        n = min(count.value, room)
        if capacity is None:
            return cloud[:n], (nrm[:n] if normals else None)
        return cloud[:n], (nrm[:n] if normals else None), count.value

    def window(self):
        """icp_tsdf_get_window: the cumulative shift of the window in voxels, three ints."""
        c = (C.c_int32 * 3)()
        self._chk(self._L.icp_tsdf_get_window(self._t, c))
        return tuple(c)

    def shift(self, s, extract=False, min_weight=1.0, normals=True):
        """icp_tsdf_shift: the window moves by s voxels; the new voxel v holds the old voxel v + s, what enters is empty.  With `extract`
        the surface the shift drops (extract_surface_region outside kept_box) is taken first and returned as (cloud, normals); else None.
        self.cfg follows the window's origin."""
        s3 = _shift3(s)
        leaving = None
        if extract:
            lo, hi = kept_box(self.cfg, s)
            leaving = self.extract_surface_region(lo, hi, True, min_weight, normals)
        self._chk(self._L.icp_tsdf_shift(self._t, s3))
        self.cfg = self.get_config()
        return leaving

    def time_shift(self, what, s, reps=20):
        """icp_tsdf_time (diagnostic), what = 10: microseconds per launch of k_tsdf_shift by +s and -s in turn (the volume stays as it is);
        11: per group of the launches of one extract_surface_region outside kept_box (s)."""
        us = C.c_float()
        self._chk(self._L.icp_tsdf_time(self._t, what, None, None, C.cast(_shift3(s), C.c_void_p), None, 0.0, 0.0, 0, reps, C.byref(us)))
        return us.value

    def extract_mesh(self, min_weight=1.0, normals=True, vertex_capacity=None, triangle_capacity=None):
        """icp_tsdf_extract_mesh: the volume's surface as (cloud (n, 8), normals (n, 4) or None, triangles (m, 3) uint32): the vertices
        are extract_surface's members, a triangle is three member positions, in ascending cell index and table order.  Without capacities:
        one counting call for both counts, then everything.  When a capacity is given: (cloud, normals, triangles, vertex count, triangle
        count), the first min (count, capacity) records of each kind (a capacity left None is 0) and the numbers there are; the indices
        always refer to the full member order."""
        opt, nv, nt = icp_tsdf_surface_t(min_weight, int(bool(normals))), C.c_uint32(), C.c_uint32()
        counting = vertex_capacity is None and triangle_capacity is None
        if counting:
            self._chk(self._L.icp_tsdf_extract_mesh(self._t, C.byref(opt), 0, None, None, C.byref(nv), 0, None, C.byref(nt)))
            vroom, troom = nv.value, nt.value
        else:
            vroom, troom = int(vertex_capacity or 0), int(triangle_capacity or 0)
        cloud = np.empty((vroom, 8), np.float32)
        nrm = np.empty((vroom, 4), np.float32) if normals else None
        tri = np.empty((troom, 3), np.uint32)
        self._chk(self._L.icp_tsdf_extract_mesh(self._t, C.byref(opt), vroom, _ptr(cloud) if vroom else None, _ptr(nrm) if vroom else None, C.byref(nv),
                                                troom, _ptr(tri) if troom else None, C.byref(nt)))
        n, m = min(nv.value, vroom), min(nt.value, troom)
        out = (cloud[:n], (nrm[:n] if normals else None), tri[:m])
        return out if counting else out + (nv.value, nt.value)

    def register(self, cloud, pose12, max_iterations=20, angle_threshold=None, translation_threshold=None):
        """icp_tsdf_register: the cloud (n, 8) of the camera's frame registered against the volume itself from pose12: a Registration."""
        cloud = np.ascontiguousarray(cloud, np.float32)
        if cloud.ndim != 2 or cloud.shape[1] != 8:
            raise ValueError("expected a cloud of n x 8 floats")
        opt, out = _register_options(max_iterations, angle_threshold, translation_threshold), icp_tsdf_registration_t()
        self._chk(self._L.icp_tsdf_register(self._t, C.byref(opt), _ptr(cloud), cloud.shape[0], _ptr(_pose(pose12)), C.byref(out)))
        return Registration(out)

    def register_from(self, icp, which, pose12, max_iterations=20, angle_threshold=None, translation_threshold=None):
        """icp_tsdf_register_from: F or M (which = Memory.F / Memory.M) of registration 0 of `icp`, device to device: a Registration."""
        rgbd._handle(icp, "a registration of a level's landmarks")
        opt, out = _register_options(max_iterations, angle_threshold, translation_threshold), icp_tsdf_registration_t()
        self._chk(self._L.icp_tsdf_register_from(self._t, C.byref(opt), icp._h, which, _ptr(_pose(pose12)), C.byref(out)))
        return Registration(out)

    def time_register(self, what, cloud, pose12, reps=20):
        """icp_tsdf_time (diagnostic), what = 8: microseconds per iteration (both launches) of a registration of `cloud` held at pose12;
        9: of k_tsdf_reg_moments alone."""
        cloud, us = np.ascontiguousarray(cloud, np.float32), C.c_float()
        self._chk(self._L.icp_tsdf_time(self._t, what, None, _ptr(_pose(pose12)), _ptr(cloud), None, 0.0, 0.0, cloud.shape[0], reps, C.byref(us)))
        return us.value

    def time_kernel(self, what, cam=None, pose12=None, depth=None, rgb=None, z_near=0.0, z_far=0.0, side=0, reps=20):
        """icp_tsdf_time (diagnostic): microseconds per launch of k_tsdf_integrate (what = 0; the volume changes) or k_tsdf_raycast (1), or
        per group of the launches of one extract_surface with normals (2; 3: its two scan launches alone, 4: its scatter and points launches alone), or
        per group of the launches of one extract_mesh with normals (5; 6: its cell sweep alone, 7: its triangle pass alone) — for 2 .. 7
        nothing but reps is used."""
        if depth is not None:
            depth, rgb = _images(depth, rgb, cam.width, cam.height)
        c, us = cam._c() if cam is not None else None, C.c_float()
        self._chk(self._L.icp_tsdf_time(self._t, what, C.byref(c) if c is not None else None, _ptr(_pose(pose12)) if pose12 is not None else None,
                                        _ptr(depth), _ptr(rgb), z_near, z_far, side, reps, C.byref(us)))
        return us.value


def _follow_camera(volume, pose, follow_, on_shift):
    """After a frame: hand pose . (0, 0, distance) to follow (); a non-zero shift extracts what leaves, shifts, and calls on_shift."""
    distance, threshold = follow_
    P = np.asarray(pose, np.float64).reshape(3, 4)
    point = (P[:, 2] * float(distance) + P[:, 3]).astype(np.float32)
    s = follow(volume.cfg, point, threshold)
    if any(s):
        cloud, nrm = volume.shift(s, extract=True)
        if on_shift is not None:
            on_shift(s, cloud, nrm)


def track_to_model(icp, volume, frames, pose0, z_near, z_far, normals=False, follow=None, on_shift=None):
    """Frame-to-model tracking as a generator over `frames`, an iterable of (depth, rgb or None) image pairs of the handle's RGB-D
    configuration.  The first frame is integrated at pose0.  Every later frame: the volume's view from the current pose goes into F
    (raycast_to; with `normals` also into NORMALS_F) and buildRBC follows; the front end writes the frame into M; reset_transform and run;
    pose = compose_pose (pose, T); the frame is integrated at the new pose.  Yields (pose, k, scale) per frame, (pose0, None, 1.0) first.
    follow = (distance, threshold): the volume follows the camera — after a frame is integrated the point pose . (0, 0, distance) goes to
    follow (); a non-zero shift s runs volume.shift (s, extract=True) and on_shift (s, cloud, normals) receives the surface that left."""
    cam = rgbd.get_config(icp)
    pose = _pose(pose0).copy()
    first = True
    for depth, colour in frames:
        if first:
            first, k, scale = False, None, 1.0
        else:
            volume.raycast_to(icp, icp_amd.Memory.F, pose, z_near, z_far, normals=normals)
            icp.buildRBC()
            rgbd.write(icp, icp_amd.Memory.M, depth, colour)
            icp.reset_transform()
            k = icp.run()
            pose, scale = compose_pose(pose, icp.read(icp_amd.Memory.T))
        volume.integrate(cam, pose, depth, colour)
        if follow is not None:
            _follow_camera(volume, pose, follow, on_shift)
        yield pose.copy(), k, scale


def track_to_volume(icp, volume, frames, pose0, max_iterations=20, follow=None, on_shift=None):
    """track_to_model without the view, as a generator over `frames`.  The first frame is integrated at pose0.  Every later frame: the front
    end writes it into M (rgbd.write), register_from registers M against the volume starting at the last pose, and the frame is integrated
    at the new pose.  Yields (pose, Registration) per frame, (pose0, None) first.  follow, on_shift: as in track_to_model."""
    cam = rgbd.get_config(icp)
    pose = _pose(pose0).copy()
    first = True
    for depth, colour in frames:
        reg = None
        if first:
            first = False
        else:
            rgbd.write(icp, icp_amd.Memory.M, depth, colour)
            reg = volume.register_from(icp, icp_amd.Memory.M, pose, max_iterations)
            pose = reg.pose.copy()
        volume.integrate(cam, pose, depth, colour)
        if follow is not None:
            _follow_camera(volume, pose, follow, on_shift)
        yield pose.copy(), reg
