"""GPU tests of the TSDF volume (icp_tsdf.hip, icp_amd/tsdf.py) against its numpy restatement (tsdf_ref.py): everything bit for bit.
Every condition on a test's own inputs is asserted on the restatement, so that no comparison is one of empty images."""
import functools
import os
import subprocess

import numpy as np
import pytest

import icp_checks as K
import rgbd_ref as R
import tsdf_ref as T
from icp_checks import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 4
F32 = np.float32
Z_NEAR, Z_FAR = 200.0, 1600.0


def _p12(P):
    return np.ascontiguousarray(P, np.float64).reshape(12).astype(F32)


def _cam(d):
    from icp_amd import rgbd
    return rgbd.RGBDConfig(**d)


def _device_volume(cfg):
    from icp_amd import tsdf
    return tsdf.TSDFVolume(tsdf.TSDFConfig(**cfg))


def _assert_volume(dev, ref, what):
    dw, col = dev.read()
    assert_bits(dw, ref.dw, what + ": {D, W}")
    if ref.rgb is not None:
        assert_bits(col, ref.rgb, what + ": colour")
    else:
        assert col is None


# ---- inputs, computed once ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _corner_frames():
    """The six frames of the corner scene through the CPU test's camera: (camera, [(pose12, depth, rgb)])."""
    cam = T.corner_camera()
    out = []
    for eye in T.EYES:
        P = T.look_at(eye)
        depth, rgb = T.render_corner(P, cam)[:2]
        depth.flags.writeable = rgb.flags.writeable = False
        out.append((_p12(P), depth, rgb))
    return cam, out


@functools.lru_cache(maxsize=None)
def _fused_corner(dims, colour):
    """The restatement's volume of the six frames (read-only), 16 mm voxels."""
    cam, frames = _corner_frames()
    vol = T.Volume(T.corner_volume(dims=dims, colour=colour))
    for pose, depth, rgb in frames:
        T.integrate(vol, cam, pose, depth, rgb if colour else None)
    vol.dw.flags.writeable = False
    if vol.rgb is not None:
        vol.rgb.flags.writeable = False
    return vol


def _fuse_on_device(dims, colour):
    cam, frames = _corner_frames()
    dev = _device_volume(T.corner_volume(dims=dims, colour=colour))
    for pose, depth, rgb in frames:
        dev.integrate(_cam(cam), pose, depth, rgb if colour else None)
    return dev


# The tracking camera: the CPU test's field of view at four times its resolution, with a lattice of 64 x 64 landmarks.  (test_gpu_rgbd.py's
# table has sides 16 and 128 only: its "steps (5, 2)" lattice serves side 16 below.)
TRACK_CAM = dict(width=320, height=240, fx=300.0, cx=159.5, cy=119.5, x0=2, y0=3, step_x=5, step_y=3)


def _track_cam():
    return T.corner_camera(**TRACK_CAM)


# ---- 1. integrate, small ----------------------------------------------------------------------------------------------------------------

SMALL = dict(dims=(24, 20, 12), origin=(-100.0, -80.0, -40.0), mu=32.0, eyes=[(-30, -20, -10), (20, 20, 20), (60, 10, 100)],
             targets=[(284, 240, 152), (250, 240, 60), (250, 200, 20)])


@functools.lru_cache(maxsize=None)
def _small_frames():
    cam = T.corner_camera(width=46, height=31, fx=30.0, cx=22.3, cy=15.1)
    rng = np.random.default_rng(1)
    u, v = np.meshgrid(np.arange(46), np.arange(31))
    out = []
    for i in range(3):
        depth = (120 + u + 2 * v + 10 * i + rng.integers(-3, 4, (31, 46))).astype(np.uint16)
        depth[rng.random((31, 46)) < 0.2] = 0                               # 20 % invalid pixels
        rgb = rng.integers(0, 256, (31, 46, 3)).astype(np.uint8)
        out.append((_p12(T.look_at(SMALL["eyes"][i], SMALL["targets"][i], up=(0.1, 0.2, 1.0))), depth, rgb))
    return cam, out


@pytest.mark.parametrize("colour", [1, 0], ids=["colour", "no colour"])
def test_integrate_small(engine, colour):
    """24 x 20 x 12 voxels, a 46 x 31 image: nothing is a multiple of 8 or 64.  Three oblique frames, the second without a colour image,
    w_max = 2 so that the cap acts; the whole volume after every frame."""
    cam, frames = _small_frames()
    nx, ny, nz = SMALL["dims"]
    cfg = T.volume_config(nx, ny, nz, 16.0, SMALL["origin"], SMALL["mu"], w_max=2.0, colour=colour)
    ref, dev = T.Volume(cfg), _device_volume(cfg)
    _assert_volume(dev, ref, "a fresh volume")
    always = np.ones((nz, ny, nx), bool)
    for f, (pose, depth, rgb) in enumerate(frames):
        image = rgb if f != 1 else None
        before = None if ref.rgb is None else ref.rgb.copy()
        cls = T.integrate(ref, cam, pose, depth, image)
        for name in ("behind", "outside", "occluded", "front", "changed"):
            assert cls[name].mean() >= 0.05, (f, name, cls[name].mean())
        assert 0.15 < (depth == 0).mean() < 0.25
        always &= cls["changed"]
        if colour and f == 1:
            assert np.array_equal(ref.rgb, before)                           # no colour image: C stays
        dev.integrate(_cam(cam), pose, depth, image)
        _assert_volume(dev, ref, "after frame %d" % f)
    assert always.sum() > 50 and ref.dw[..., 1].max() == 2.0                # voxels seen three times: the cap acted
    dev.reset()
    _assert_volume(dev, T.Volume(cfg), "after reset")
    dev.close()


# ---- 2. the corner scene: integrate and the dense ray cast ------------------------------------------------------------------------------

CORNER_DIMS = (64, 56, 48)


@functools.lru_cache(maxsize=None)
def _corner_cast():
    cam, _ = _corner_frames()
    P = T.look_at(T.EYE_CAST)
    return P, T.raycast(_fused_corner(CORNER_DIMS, 1), cam, _p12(P), Z_NEAR, Z_FAR)


def test_corner_scene_volume_and_dense_raycast(engine):
    cam, _ = _corner_frames()
    ref = _fused_corner(CORNER_DIMS, 1)
    P, cast = _corner_cast()
    f = T.corner_figures(ref, cam, P, cast=cast)
    assert f["hits"] >= 0.95 and f["normals"] >= 0.9 and f["err"].max() < 16.0, f       # 0.9806, 0.9533, 11.22: as the CPU test's 64^3
    assert (cast[0][:, 4:7].max(0) > 0.5).all()                                          # the colour is there
    dev = _fuse_on_device(CORNER_DIMS, 1)
    _assert_volume(dev, ref, "the fused corner")
    cloud, nrm = dev.raycast(_cam(cam), _p12(P), Z_NEAR, Z_FAR)
    assert_bits(cloud, cast[0], "cloud")
    assert_bits(nrm, cast[1], "normals")
    only_cloud, none = dev.raycast(_cam(cam), _p12(P), Z_NEAR, Z_FAR, normals=False)
    assert none is None
    assert_bits(only_cloud, cast[0], "cloud without normals")
    # a volume without colour: the same geometry, the colour lanes 0
    plain = _fuse_on_device(CORNER_DIMS, 0)
    _assert_volume(plain, _fused_corner(CORNER_DIMS, 0), "the fused corner without colour")
    cloud0, nrm0 = plain.raycast(_cam(cam), _p12(P), Z_NEAR, Z_FAR)
    want0 = cast[0].copy(); want0[:, 4:7] = 0
    assert_bits(cloud0, want0, "cloud without colour")
    assert_bits(nrm0, cast[1], "normals without colour")
    dev.close(); plain.close()


# ---- 3. ray casts of written volumes ------------------------------------------------------------------------------------------------------

CAST_CAM = dict(width=16, height=12, fx=14.0, cx=7.0, cy=5.0)          # (integral cx, cy: pixel (7, 5) looks along the axis)
CAST_DIMS = (16, 14, 12)
LOOK_UP = np.array([[1, 0, 0, 7.0], [0, 1, 0, 6.0], [0, 0, 1, -3.0]])   # below the volume, looking along +z, integral position


def _plane_volume(z_of, mu=4.0, holes=None, colour=1, dims=CAST_DIMS):
    """D = clip ((z_of (i, j) - k) / mu), W = 1 (0 where `holes`), a colour that varies along every axis; voxels of 1 from the origin."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), mu, colour=colour))
    k, j, i = np.meshgrid(np.arange(nz, dtype=F32), np.arange(ny, dtype=F32), np.arange(nx, dtype=F32), indexing="ij")
    vol.dw[..., 0] = np.clip((z_of(i, j) - k) / F32(mu), -1, 1)
    vol.dw[..., 1] = 1
    if holes is not None:
        vol.dw[..., 1][holes(i, j, k)] = 0
    if colour:
        vol.rgb[..., 0], vol.rgb[..., 1], vol.rgb[..., 2] = i / nx, j / ny, k / nz
    return vol


def _random_holes(seed, share):
    return lambda i, j, k: np.random.default_rng(seed).random(i.shape) < share


def _oblique():
    return T.look_at((4.0, 3.0, -5.0), (9.0, 8.0, 7.0), up=(0.0, 1.0, 0.2))


def _indices(vol, cam, P, z_near, z_far):
    """floor (g_a) of every sample of every ray, (N + 1, rays, 3)."""
    c = vol.cfg
    Rm, t = T._pose(_p12(P))
    u, v = np.meshgrid(np.arange(cam["width"], dtype=F32), np.arange(cam["height"], dtype=F32))
    ax, ay = ((u - F32(cam["cx"])) / F32(cam["fx"])).reshape(-1), ((v - F32(cam["cy"])) / F32(cam["fy"])).reshape(-1)
    out = []
    for n in range(T.march_trips(c["mu"], z_near, z_far) + 1):
        lam = F32(z_near) + F32(n) * (F32(0.5) * F32(c["mu"]))
        w = T._world(Rm, t, [ax * lam, ay * lam, np.full(ax.shape, lam, F32)])
        out.append(np.stack([np.floor((w[a] - F32(c["origin"][a])) / F32(c["voxel"])) for a in range(3)], -1))
    return np.stack(out)


def _case(name):
    """(volume, camera, pose (3, 4), z_near, z_far, the condition on (info, hit mask, normal mask, volume) that makes it the case it
    is called)."""
    vol, P, z_near, z_far, condition = _case_inputs(name)
    fx = 1400.0 if name == "N = 4095" else CAST_CAM["fx"]               # (a volume 1000 away: a narrow camera keeps the rays inside it)
    return vol, T.corner_camera(**dict(CAST_CAM, fx=fx)), P, z_near, z_far, condition


def _case_inputs(name):
    flat = lambda z: (lambda i, j: np.full(i.shape, z, F32))
    tilt = lambda i, j: F32(6.3) + F32(0.11) * i - F32(0.07) * j
    if name == "empty":
        vol = T.Volume(T.volume_config(*CAST_DIMS, 1.0, (0.0, 0.0, 0.0), 4.0, colour=1))
        return vol, LOOK_UP, 1.0, 14.0, lambda I, hit, nz, v: not hit.any() and (I["n_star"] == -1).all()
    if name == "sample exactly 0":
        # D (k) = (6 - k) / 4 and samples at z = -2, 0, .. 6 on the axis: S = 0 exactly at n = 4, so lambda* = lambda_3 + delta = lambda_4
        return (_plane_volume(flat(6.0)), LOOK_UP, 1.0, 14.0,
                lambda I, hit, nz, v: I["lam_exact"].reshape(12, 16)[5, 7] and I["n_star"].reshape(12, 16)[5, 7] == 4 and hit.all())
    if name == "first known sample <= 0":
        # the layers below the surface are unknown: the first sample a ray knows lies behind the surface already
        return (_plane_volume(flat(3.5), holes=lambda i, j, k: k < 5), LOOK_UP, 1.0, 14.0,
                lambda I, hit, nz, v: not hit.any() and ((I["n_star"] >= 1) & ~I["seen_before"]).all())
    if name == "predecessor unknown":
        # known and positive, then one unknown layer just in front of the surface, then known and negative
        return (_plane_volume(flat(6.5), holes=lambda i, j, k: k == 5), LOOK_UP, 1.5, 14.0,
                lambda I, hit, nz, v: not hit.any() and ((I["n_star"] >= 1) & I["seen_before"] & ~I["prev_known"]).all())
    if name == "hit cell unknown":
        return (_plane_volume(tilt, holes=_random_holes(3, 0.03)), _oblique(), 1.0, 24.0,
                lambda I, hit, nz, v: (I["cross"] & ~I["cell_known"]).sum() >= 2 and hit.sum() >= 20)
    if name == "gradient sample unknown":
        return (_plane_volume(tilt, holes=_random_holes(4, 0.03)), _oblique(), 1.0, 24.0,
                lambda I, hit, nz, v: (hit & ~I["grad_known"]).sum() >= 5 and (hit & nz).sum() >= 20 and not (nz & ~I["grad_known"]).any())
    if name == "through the faces":
        def cond(I, hit, nz, v):
            idx = _indices(v, T.corner_camera(**CAST_CAM), _oblique(), 1.0, 24.0)
            n = np.array([v.cfg["nx"], v.cfg["ny"], v.cfg["nz"]], F32)
            print("axes with a sample at -1:", [a for a in range(3) if (idx[..., a] == -1).any()], " at n_a - 1:", [a for a in range(3) if (idx[..., a] == n[a] - 1).any()])
            return sum((idx[..., a] == -1).any() for a in range(3)) >= 2 and sum((idx[..., a] == n[a] - 1).any() for a in range(3)) >= 2 and hit.sum() >= 20
        return _plane_volume(tilt), _oblique(), 1.0, 24.0, cond
    if name == "N = 0":
        return (_plane_volume(flat(6.5)), LOOK_UP, 8.0, 9.5,
                lambda I, hit, nz, v: T.march_trips(4.0, 8.0, 9.5) == 0 and not hit.any() and (I["n_star"] == -1).all())
    if name == "N = 4095":
        # mu = 0.5: 4096 samples a quarter voxel apart up to a volume 1015 away; the surface two thirds into it
        vol = _plane_volume(flat(8.3), mu=0.5)
        vol.cfg["origin"] = (0.0, 0.0, 1012.0)
        return (vol, LOOK_UP, 1.0, 1024.75,
                lambda I, hit, nz, v: T.march_trips(0.5, 1.0, 1024.75) == 4095 and hit.all() and I["n_star"].min() > 4000)
    raise KeyError(name)


CASES = ["empty", "sample exactly 0", "first known sample <= 0", "predecessor unknown", "hit cell unknown", "gradient sample unknown",
         "through the faces", "N = 0", "N = 4095"]


@pytest.mark.parametrize("name", CASES)
def test_raycast_of_written_volumes(engine, name):
    vol, cam, P, z_near, z_far, condition = _case(name)
    info = {}
    cloud, nrm, lam = T.raycast(vol, cam, _p12(P), z_near, z_far, info=info)
    hit, with_normal = ~np.isnan(lam), np.any(nrm[:, :3] != 0, axis=1)
    assert condition(info, hit, with_normal, vol), name
    dev = _device_volume(vol.cfg)
    dev.write(vol.dw, vol.rgb)
    _assert_volume(dev, vol, name + ": write then read")
    got, gotn = dev.raycast(_cam(cam), _p12(P), z_near, z_far)
    assert_bits(got, cloud, name + ": cloud")
    assert_bits(gotn, nrm, name + ": normals")
    dev.close()


# ---- 4. the lattice form is the dense form at the lattice -------------------------------------------------------------------------------

def _lattice_case(side):
    if side == 16:
        # test_gpu_rgbd.py's "steps (5, 2)": 16 x 16 landmarks of an 80 x 40 image, nr = 4
        return T.corner_camera(width=80, height=40, cy=19.5, x0=2, y0=3, step_x=5, step_y=2), 4
    return _track_cam(), 64


@pytest.mark.parametrize("side", [16, 64])
def test_lattice_form_equals_dense_form_at_the_lattice(engine, side):
    from icp_amd import rgbd
    Mem = engine.Memory
    d, nr = _lattice_case(side)
    ref = _fused_corner(CORNER_DIMS, 1)
    P = T.look_at(T.EYE_CAST)
    pose = _p12(P)
    dev = _fuse_on_device(CORNER_DIMS, 1)
    dense, dense_n = dev.raycast(_cam(d), pose, Z_NEAR, Z_FAR)
    at = R.lattice(d, side)
    want, want_n, lam = T.raycast(ref, d, pose, Z_NEAR, Z_FAR, side=side)
    assert (~np.isnan(lam)).mean() >= 0.9 and np.any(want_n[:, :3] != 0, axis=1).mean() >= 0.8
    assert_bits(dense[at], want, "the dense form at the lattice")
    assert_bits(dense_n[at], want_n, "the dense form's normals at the lattice")
    lm, lm_n = dev.raycast(_cam(d), pose, Z_NEAR, Z_FAR, side=side)
    assert_bits(lm, want, "the lattice form")
    assert_bits(lm_n, want_n, "the lattice form's normals")
    # into a handle: F, M and their normals hold exactly those bits
    moved = T.rotate_pose(P, (0.3, 1.0, 0.2), 1.0, (6.0, -5.0, 6.0))
    depth, rgb = T.render_corner(moved, d)[:2]
    g, twin = engine.ICP(0), engine.ICP(0)
    for x in (g, twin):
        x.init(side * side, nr, 2e2, 1e-6)
        rgbd.set_config(x, _cam(d))
    for which, nmem in ((Mem.M, Mem.NORMALS_M), (Mem.F, Mem.NORMALS_F)):
        dev.raycast_to(g, which, pose, Z_NEAR, Z_FAR, normals=True)
        assert_bits(g.read(which), want, "landmarks of memory %d" % which)
        assert_bits(g.read(nmem), want_n, "normals of memory %d" % which)
    kept = g.read(Mem.NORMALS_F).copy()
    dev.raycast_to(g, Mem.F, pose, Z_NEAR, Z_FAR, cam=_cam(d))                # an explicit camera, no normals: they stay
    assert_bits(g.read(Mem.F), want, "landmarks with the camera given")
    assert_bits(g.read(Mem.NORMALS_F), kept, "the normals stay")
    # one step against the new frame equals the twin's, loaded through icp_write
    rgbd.write(g, Mem.M, depth, rgb)
    twin.write(Mem.F, want)
    twin.write(Mem.NORMALS_F, want_n)
    rgbd.write(twin, Mem.M, depth, rgb)
    for x in (g, twin):
        x.buildRBC()
        x.step()
    for mem in (Mem.T, Mem.R, Mem.TK, Mem.NN, Mem.QT):
        assert_bits(g.read(mem), twin.read(mem), "memory %d after one step" % mem)
    assert g.state().k == twin.state().k == 1
    g.close(); twin.close(); dev.close()


# ---- 5. frame-to-model end to end ------------------------------------------------------------------------------------------------------------

def pose_errors(pose12, P_true):
    """(rotation error in degrees, translation error) of a pose against the true (3, 4) one."""
    P = np.asarray(pose12, np.float64).reshape(3, 4)
    c = (np.trace(P[:, :3].T @ P_true[:, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(P[:, 3] - P_true[:, 3]))


MOTION = ((0.3, 1.0, 0.2), 1.0, (6.0, -5.0, 6.0))                     # 1 degree about an oblique axis and 10 mm (|(6, -5, 6)| = 9.85)
P2PL_MU = 0.05                                                         # (the point weight of every point-to-plane test here: icp_checks.make_plane)


def _plane_handle(engine, d):
    """64 x 64 landmarks, 64 representatives, point-to-plane against given normals — the view of a volume is an organised grid with normals,
    and both frames lie on one pixel lattice: point-to-point pairs a landmark with the fixed landmark of its own pixel ray and cannot see a
    motion along the three planes (on the CPU oracle it leaves this scene's 1 degree and 9.85 mm at 0.99 degrees and 10.7 mm)."""
    from icp_amd import rgbd
    g = engine.ICP(0)
    g.init(64 * 64, 64, 2e2, 1e-6)
    rgbd.set_config(g, _cam(d))
    g.set_normals(K.GIVEN, 0)
    g.set_error_metric(K.P2PL, P2PL_MU)
    g.set_rejection(invalid=True)                                      # (a ray that misses leaves the engine's invalid point)
    return g


def frame_to_model_errors(engine, dev):
    """The end-to-end registration of test 5 on a fused device volume: ((k, converged, rotation error, translation error) of the model run,
    the same of the twin, the errors before)."""
    from icp_amd import rgbd, tsdf
    Mem = engine.Memory
    d = _track_cam()
    P_prev = T.look_at(T.EYE_CAST)
    P_new = T.rotate_pose(P_prev, *MOTION)
    prev, new = T.render_corner(P_prev, d)[:2], T.render_corner(P_new, d)[:2]
    out = []
    for model in (True, False):
        g = _plane_handle(engine, d)
        if model:
            dev.raycast_to(g, Mem.F, _p12(P_prev), Z_NEAR, Z_FAR, normals=True)
        else:
            rgbd.write(g, Mem.F, *prev, normals=True)
        g.buildRBC()
        rgbd.write(g, Mem.M, *new)
        g.reset_transform()
        k = g.run()
        pose, _ = tsdf.compose_pose(_p12(P_prev), g.read(Mem.T))
        out.append((k, g.state().converged) + pose_errors(pose, P_new))
        g.close()
    return out[0], out[1], pose_errors(_p12(P_prev), P_new)


def test_frame_to_model_end_to_end(engine):
    """Frame-to-model against frame-to-frame with a perfect previous frame.  The CPU restatements (oracle search, p2pl_ref) predict
    0.180 degrees / 2.00 mm for the model and 0.181 degrees / 1.75 mm for the twin at the point weight 0.05; at the point weight 0 they
    predict 0.030 / 0.73 against 0.036 / 0.34: a translation ratio of 2.1 at a third of the error.  Measured on an MI355X at 0.05:
    0.1800 degrees / 1.998 mm in 8 iterations against 0.1803 degrees / 1.746 mm in 7."""
    dev = _fuse_on_device((64, 64, 64), 1)
    model, twin, start = frame_to_model_errors(engine, dev)
    dev.close()
    print("frame-to-model: k %d rotation %.4f deg translation %.3f;  frame-to-frame twin: k %d rotation %.4f deg translation %.3f;  before: %.4f deg %.3f"
          % (model[0], model[2], model[3], twin[0], twin[2], twin[3], start[0], start[1]))
    assert model[1] and twin[1] and model[0] < 40 and twin[0] < 40, (model, twin)          # both converge
    assert twin[2] < start[0] and twin[3] < start[1], (twin, start)                        # the twin ends closer than it started
    assert model[2] <= 2.0 * twin[2] and model[3] <= 2.0 * twin[3], (model, twin)


# ---- 6. track_to_model ------------------------------------------------------------------------------------------------------------------

def test_track_to_model_is_the_loop_written_out(engine):
    from icp_amd import rgbd, tsdf
    Mem = engine.Memory
    d = _track_cam()
    P = [T.look_at(T.EYE_CAST)]
    for _ in range(3):
        P.append(T.rotate_pose(P[-1], *MOTION))
    frames = [T.render_corner(p, d)[:2] for p in P]
    cfg = T.corner_volume(colour=1)

    g, dev = _plane_handle(engine, d), _device_volume(cfg)
    got = list(tsdf.track_to_model(g, dev, frames, _p12(P[0]), Z_NEAR, Z_FAR, normals=True))
    # by hand
    h, vol = _plane_handle(engine, d), _device_volume(cfg)
    pose = _p12(P[0])
    vol.integrate(_cam(d), pose, *frames[0])
    want = [(pose.copy(), None, 1.0)]
    for depth, rgb in frames[1:]:
        vol.raycast_to(h, Mem.F, pose, Z_NEAR, Z_FAR, normals=True)
        h.buildRBC()
        rgbd.write(h, Mem.M, depth, rgb)
        h.reset_transform()
        k = h.run()
        pose, scale = tsdf.compose_pose(pose, h.read(Mem.T))
        vol.integrate(_cam(d), pose, depth, rgb)
        want.append((pose.copy(), k, scale))
    assert len(got) == len(want) == 4
    ref = T.Volume(cfg)
    for i, ((pg, kg, sg), (pw, kw, sw)) in enumerate(zip(got, want)):
        assert_bits(pg, pw, "pose of frame %d" % i)
        assert kg == kw and sg == sw, (i, kg, kw, sg, sw)
        T.integrate(ref, d, pg, *frames[i])
        if i:
            rot, tra = pose_errors(pg, P[i])
            print("track_to_model frame %d: k %d rotation error %.4f degrees translation error %.3f" % (i, kg, rot, tra))
            assert kg < 40 and rot < 1.0 and tra < 9.84, (i, kg, rot, tra)      # every frame ends closer to the truth than one hop's motion
    _assert_volume(dev, ref, "the volume after four frames")
    g.close(); h.close(); dev.close(); vol.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_volume_and_the_handle_as_they_were(engine):
    from icp_amd import rgbd, tsdf
    Mem = engine.Memory
    good = dict(nx=8, ny=8, nz=8, voxel=16.0, origin=(0.0, 0.0, 0.0), mu=48.0, w_max=64.0, colour=0)
    for field, value in T.BAD_FIELDS:
        with pytest.raises(engine.ICPError) as e:
            tsdf.TSDFVolume(tsdf.TSDFConfig(**dict(good, **{field: value})))
        assert e.value.code == EINVAL, (field, value)
    with pytest.raises(engine.ICPError) as e:
        tsdf.TSDFVolume(tsdf.TSDFConfig(**good), device=99)                  # the wrong device index
    assert e.value.code == EINVAL
    cam, frames = _corner_frames()
    pose, depth, rgb = frames[0]
    cfg = T.corner_volume(dims=(24, 20, 12), colour=1)
    dev, ref = _device_volume(cfg), T.Volume(cfg)
    dev.integrate(_cam(cam), pose, depth, rgb)
    T.integrate(ref, cam, pose, depth, rgb)
    d = T.corner_camera(x0=2, y0=3, step_x=5, step_y=3)                      # 16 x 16 landmarks fit the 80 x 60 image
    g = engine.ICP(0)
    g.init(256, 4, 2e2, 1e-6)
    rgbd.set_config(g, _cam(d))
    dev.raycast_to(g, Mem.F, pose, Z_NEAR, Z_FAR, normals=True)
    F, NF = g.read(Mem.F).copy(), g.read(Mem.NORMALS_F).copy()
    L, t = tsdf._lib(), dev._t
    c = _cam(cam)._c()
    import ctypes as C
    cp, pp, dp = C.byref(c), pose.ctypes.data, depth.ctypes.data
    out = np.empty((80 * 60, 8), F32)
    nan_pose, inf_pose = pose.copy(), pose.copy()
    nan_pose[5], inf_pose[11] = np.nan, np.inf
    bad_cam = _cam(dict(cam, fx=0.0))._c()
    no_fit = _cam(dict(d, x0=10))._c()                                         # 10 + 5 * 15 = 85 >= 80
    other = np.roll(pose, 4)
    far = 200.0 + 24.0 * 4096.0                                                # N = 4096 at mu = 48

    def refused(rc, code=EINVAL):
        assert rc == code, (rc, L.icp_tsdf_last_error(t))
        _assert_volume(dev, ref, "the volume after a refusal")
        assert_bits(g.read(Mem.F), F, "F after a refusal")
        assert_bits(g.read(Mem.NORMALS_F), NF, "NORMALS_F after a refusal")

    # NULL pointers
    refused(L.icp_tsdf_integrate(t, None, pp, dp, None))
    refused(L.icp_tsdf_integrate(t, cp, None, dp, None))
    refused(L.icp_tsdf_integrate(t, cp, pp, None, None))
    refused(L.icp_tsdf_raycast(t, cp, pp, Z_NEAR, Z_FAR, 0, None, None))
    refused(L.icp_tsdf_raycast(t, None, pp, Z_NEAR, Z_FAR, 0, out.ctypes.data, None))
    refused(L.icp_tsdf_raycast_to(t, None, Mem.F, None, pp, Z_NEAR, Z_FAR, 0))
    refused(L.icp_tsdf_raycast_to(t, g._h, Mem.F, None, None, Z_NEAR, Z_FAR, 0))
    refused(L.icp_tsdf_read(t, None, None))
    refused(L.icp_tsdf_read(t, out.ctypes.data, None))                         # a volume with colour needs rgb
    refused(L.icp_tsdf_write(t, out.ctypes.data, None))
    # a non-finite pose, a camera out of range
    for p in (nan_pose, inf_pose):
        refused(L.icp_tsdf_integrate(t, cp, p.ctypes.data, dp, None))
        refused(L.icp_tsdf_raycast(t, cp, p.ctypes.data, Z_NEAR, Z_FAR, 0, out.ctypes.data, None))
        refused(L.icp_tsdf_raycast_to(t, g._h, Mem.F, None, p.ctypes.data, Z_NEAR, Z_FAR, 1))
    refused(L.icp_tsdf_integrate(t, C.byref(bad_cam), pp, dp, None))
    refused(L.icp_tsdf_raycast(t, C.byref(bad_cam), pp, Z_NEAR, Z_FAR, 0, out.ctypes.data, None))
    # z ranges: not 0 < z_near < z_far finite, N > 4095
    for zn, zf in ((0.0, 100.0), (-1.0, 100.0), (300.0, 300.0), (300.0, 200.0), (float("nan"), 100.0), (200.0, float("inf")), (200.0, far)):
        refused(L.icp_tsdf_raycast(t, cp, pp, zn, zf, 0, out.ctypes.data, None))
        refused(L.icp_tsdf_raycast_to(t, g._h, Mem.F, None, other.ctypes.data, zn, zf, 1))
    assert L.icp_tsdf_raycast(t, cp, pp, 200.0, float(np.nextafter(F32(far), F32(0))), 0, out.ctypes.data, None) == 0      # N = 4095 passes
    # a lattice that does not fit; which; a non-square m
    refused(L.icp_tsdf_raycast(t, cp, pp, Z_NEAR, Z_FAR, 64, out.ctypes.data, None))
    refused(L.icp_tsdf_raycast_to(t, g._h, Mem.F, C.byref(no_fit), other.ctypes.data, Z_NEAR, Z_FAR, 1))
    refused(L.icp_tsdf_raycast_to(t, g._h, Mem.T, None, other.ctypes.data, Z_NEAR, Z_FAR, 1))
    # a handle that is not initialised
    fresh = engine.ICP(0)
    refused(L.icp_tsdf_raycast_to(t, fresh._h, Mem.F, cp, pp, Z_NEAR, Z_FAR, 0), ESTATE)
    fresh.close()
    # the facade raises what the library says
    with pytest.raises(engine.ICPError) as e:
        dev.raycast(_cam(cam), pose, 200.0, far)
    assert e.value.code == EINVAL and "4096" in str(e.value)
    with pytest.raises(ValueError):
        dev.integrate(_cam(cam), pose, depth.astype(np.float32))
    with pytest.raises(ValueError):
        dev.write(np.zeros(7, F32))
    g.close(); dev.close()


def test_raycast_to_is_refused_while_tracked_frames_are_in_flight(engine):
    """ICP_ESTATE with a tracked frame submitted and not collected; the landmarks of the frame stay."""
    from icp_amd import rgbd, tsdf
    Mem = engine.Memory
    cam, frames = _corner_frames()
    dev = _fuse_on_device((24, 20, 12), 0)
    g = engine.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    g.track_submit(engine.synth_cloud_vga())
    with pytest.raises(engine.ICPError) as e:
        dev.raycast_to(g, Mem.F, frames[0][0], Z_NEAR, Z_FAR)
    assert e.value.code == ESTATE
    g.track_collect()
    g.close(); dev.close()


# ---- 8. the layers above ------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_program():
    """tests/cpp/tsdf_facade_test.cpp: cl_algo::ICP::TSDFVolume against the C-ABI it wraps and the rule written out on the host."""
    exe = os.path.join(ROOT, "tests", "cpp", "tsdf_facade_test")
    assert os.path.exists(exe), "tests/cpp/tsdf_facade_test is built by build() / make tsdf_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tsdf facade ok" in out.stdout, (out.stdout, out.stderr)


def test_timing_entry_runs_both_kernels(engine):
    """icp_tsdf_time (tools/diag/tsdf_time.py): the ray cast goes into scratch and leaves the volume alone; integrate leaves reps + 1 frames."""
    cam, frames = _corner_frames()
    pose, depth, rgb = frames[0]
    cfg = T.corner_volume(dims=(24, 20, 12), colour=1, w_max=64.0)
    dev, ref = _device_volume(cfg), T.Volume(cfg)
    assert dev.time_kernel(0, _cam(cam), pose, depth, rgb, reps=2) > 0
    for _ in range(3):
        T.integrate(ref, cam, pose, depth, rgb)
    _assert_volume(dev, ref, "after 1 + 2 timed integrations")
    for side in (0, 16):
        assert dev.time_kernel(1, _cam(T.corner_camera(x0=2, y0=3, step_x=5, step_y=3)), pose, z_near=Z_NEAR, z_far=Z_FAR, side=side, reps=2) > 0
    _assert_volume(dev, ref, "after the timed ray casts")
    dev.close()
