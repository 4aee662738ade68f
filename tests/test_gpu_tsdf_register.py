"""GPU tests of the registration against the TSDF volume itself (icp_tsdf_register.hip, icp_amd/tsdf.py) against its numpy restatement
(tsdf_register_ref.py): everything bit for bit.  Every condition on a test's own inputs is asserted on the restatement first."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import rgbd_ref as R
import tsdf_ref as T
import tsdf_register_ref as G
from icp_checks import assert_bits
from tsdf_register_ref import IDENTITY, START, TRUE_1, p12 as _p12, corner, edge_points, edge_volume, frame_cloud, plane_volume, points, pose_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 4
F32 = np.float32
TRACK_CAM = dict(width=320, height=240, fx=300.0, cx=159.5, cy=119.5, x0=2, y0=3, step_x=5, step_y=3)


def _cam(d):
    from icp_amd import rgbd
    return rgbd.RGBDConfig(**d)


def _device(vol):
    from icp_amd import tsdf
    dev = tsdf.TSDFVolume(tsdf.TSDFConfig(**vol.cfg))
    dev.write(vol.dw, vol.rgb)
    return dev


def _assert_record(got, want, what):
    assert_bits(got.pose, want.pose, what + ": pose")
    assert (got.iterations, got.converged, got.singular, got.members) == (want.iterations, want.converged, want.singular, want.members), \
        (what, got, vars(want))
    assert_bits(np.float64(got.rmse), np.float64(want.rmse), what + ": rmse")
    assert_bits(got.sys, want.sys, what + ": the 27 sums")


@functools.lru_cache(maxsize=None)
def small():
    """The small volume of test_gpu_tsdf.py's recipe: 24 x 20 x 12 voxels, three oblique 46 x 31 frames with 20 % invalid pixels; and the
    cloud of its first frame with the frame's pose."""
    cam = T.corner_camera(width=46, height=31, fx=30.0, cx=22.3, cy=15.1)
    eyes, targets = [(-30, -20, -10), (20, 20, 20), (60, 10, 100)], [(284, 240, 152), (250, 240, 60), (250, 200, 20)]
    rng = np.random.default_rng(1)
    u, v = np.meshgrid(np.arange(46), np.arange(31))
    vol = T.Volume(T.volume_config(24, 20, 12, 16.0, (-100.0, -80.0, -40.0), 32.0))
    first = None
    for i in range(3):
        depth = (120 + u + 2 * v + 10 * i + rng.integers(-3, 4, (31, 46))).astype(np.uint16)
        depth[rng.random((31, 46)) < 0.2] = 0
        rng.integers(0, 256, (31, 46, 3))
        pose = _p12(T.look_at(eyes[i], targets[i], up=(0.1, 0.2, 1.0)))
        T.integrate(vol, cam, pose, depth)
        if first is None:
            first = (R.cloud(depth, None, cam), pose)
    vol.dw.flags.writeable = False
    return vol, first[0], first[1]


def _with_edges(cloud, n):
    """n points of the cloud (repeated as needed), one fifth replaced by non-finite, invalid and far points."""
    out = np.ascontiguousarray(np.resize(cloud, (n, 8)))
    rng = np.random.default_rng(n)
    bad = rng.choice(n, n // 5, replace=False) if n >= 5 else []
    specials = [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (0, 0, 0), (-0.0, -0.0, -0.0), (1e30, 0, 5), (3.0, -0.0, 200.0)]
    for j, i in enumerate(bad):
        out[i, :3] = specials[j % len(specials)]
    return out


@pytest.mark.parametrize("scene", ["small", "corner"])
def test_single_iteration(engine, scene):
    if scene == "small":
        vol, cloud, pose = small()
    else:
        vol, cloud, pose = corner()[1], frame_cloud(TRUE_1), _p12(START)
    dev = _device(vol)
    before = dev.read()[0].copy()
    valid = cloud[np.any(cloud[:, :3] != 0, 1)]
    is_member = G.point_terms(vol, valid, *T._pose(pose))[1]
    for n in (1, 255, 256, 257, 4800):
        if n == 1:
            c = np.ascontiguousarray(valid[is_member][:1])
        elif n < 4800:
            c = np.ascontiguousarray(valid[np.linspace(0, len(valid) - 1, n).astype(int)])        # (spread over the image)
        else:
            c = _with_edges(cloud, n)
        want = G.register(vol, c, pose, 1)
        member = G.point_terms(vol, c, *T._pose(pose))[1]
        assert member.any() and want.members == member.sum(), (scene, n, want.members)
        if n == 4800:
            assert not member.all() and not want.singular, (scene, n, want.members)
        got = dev.register(c, pose, 1)
        print(scene, n, "members", want.members, "singular", want.singular)
        _assert_record(got, want, "%s n = %d" % (scene, n))
    assert_bits(dev.read()[0], before, "the volume after the registrations")
    dev.close()


def test_chained_run_and_one_by_one(engine):
    vol, cloud, pose = corner()[1], frame_cloud(TRUE_1), _p12(START)
    dev = _device(vol)
    want = G.register(vol, cloud, pose, 6, 0.0, 0.0)
    assert want.iterations == 6 and want.members > 0.8 * 4800
    got = dev.register(cloud, pose, 6, 0.0, 0.0)
    _assert_record(got, want, "six iterations in one call")
    p = pose
    for i in range(6):
        one = dev.register(cloud, p, 1, 0.0, 0.0)
        p = one.pose
    assert_bits(one.pose, got.pose, "six calls of one iteration")
    assert_bits(one.sys, got.sys, "the sums of the sixth iteration")
    assert one.members == got.members and one.iterations == 1 and not one.converged and not one.singular
    assert_bits(np.float64(one.rmse), np.float64(got.rmse), "the rmse of the sixth iteration")
    dev.close()


@pytest.mark.parametrize("n", [65537, 1 << 20], ids=["a padded tree", "the full tree"])
def test_large_clouds(engine, n):
    """nblk = 257 (a padded finalize tree) and nblk = 4096 (the full one): points drawn uniformly in the 64^3 volume's box plus a margin."""
    vol = corner()[1]
    rng = np.random.default_rng(n)
    cloud = points(rng.uniform(-164.0, 1060.0, (n, 3)).astype(F32))
    want = G.register(vol, cloud, IDENTITY, 1)
    assert 0 < want.members < n and not want.singular
    dev = _device(vol)
    _assert_record(dev.register(cloud, IDENTITY, 1), want, "n = %d" % n)
    dev.close()


def test_singular_and_early_converged(engine):
    vol = plane_volume()
    rng = np.random.default_rng(2)
    cloud = points(np.stack([rng.uniform(3, 12, 200), rng.uniform(3, 12, 200), rng.uniform(5, 9, 200)], 1))
    want = G.register(vol, cloud, IDENTITY, 5)
    assert want.singular and want.iterations == 0 and want.members > 100
    dev = _device(vol)
    _assert_record(dev.register(cloud, IDENTITY, 5), want, "one plane")
    none = points([[100.0, 3.0, 3.0], [3.0, 3.0, 50.0]])
    want = G.register(vol, none, IDENTITY, 3)
    assert want.singular and want.members == 0
    _assert_record(dev.register(none, IDENTITY, 3), want, "no members")
    # the rule's edges as a cloud of their own
    ev, ec = edge_volume(), points([c[1] for c in edge_points()])
    want = G.register(ev, ec, IDENTITY, 1)
    assert 0 < want.members < ec.shape[0]
    dev.write(ev.dw)
    _assert_record(dev.register(ec, IDENTITY, 1), want, "the rule's edges")
    dev.close()
    # early convergence: the remaining launches are without effect
    vol, cloud, pose = corner()[1], frame_cloud(TRUE_1), _p12(START)
    want = G.register(vol, cloud, pose, 20, 5.0, 100.0)
    assert want.converged and want.iterations == 1
    dev = _device(vol)
    _assert_record(dev.register(cloud, pose, 20, 5.0, 100.0), want, "converged after one iteration of twenty")
    dev.close()


def _handle(engine, d):
    from icp_amd import rgbd
    g = engine.ICP(0)
    g.init(64 * 64, 64, 2e2, 1e-6)
    rgbd.set_config(g, _cam(d))
    return g


def test_register_from_a_handle(engine):
    from icp_amd import rgbd
    Mem = engine.Memory
    d = T.corner_camera(**TRACK_CAM)
    vol = corner()[1]
    dev = _device(vol)
    depth, rgb = T.render_corner(TRUE_1, d)[:2]
    g = _handle(engine, d)
    rgbd.write(g, Mem.M, depth, rgb)
    rgbd.write(g, Mem.F, depth, rgb)
    M = g.read(Mem.M).copy()
    kept = {m: g.read(m).copy() for m in (Mem.F, Mem.M, Mem.T)}
    state = bytes(g.state())
    want = G.register(vol, M, _p12(START), 4)
    assert want.members > 0.5 * 4096 and want.iterations >= 1
    _assert_record(dev.register(M, _p12(START), 4), want, "register of M read back")
    _assert_record(dev.register_from(g, Mem.M, _p12(START), 4), want, "register_from M")
    _assert_record(dev.register_from(g, Mem.F, _p12(START), 4), want, "register_from F")
    for m, v in kept.items():
        assert_bits(g.read(m), v, "memory %d of the handle afterwards" % m)
    assert bytes(g.state()) == state, "the handle's state record afterwards"
    assert_bits(dev.read()[0], vol.dw, "the volume afterwards")
    g.close(); dev.close()


def test_refusals(engine):
    from icp_amd import tsdf
    Mem = engine.Memory
    vol = plane_volume()
    dev = _device(vol)
    L, t = tsdf._lib(), dev._t
    cloud, pose = points([[6.5, 6.5, 7.5]] * 4), IDENTITY.copy()
    out = tsdf.icp_tsdf_registration_t()
    op, cp, pp = C.byref(out), cloud.ctypes.data, pose.ctypes.data
    nan_pose = pose.copy(); nan_pose[7] = np.nan
    d = T.corner_camera(**TRACK_CAM)
    g = _handle(engine, d)
    F = g.read(Mem.F).copy()

    def refused(rc, code=EINVAL):
        assert rc == code, (rc, L.icp_tsdf_last_error(t))
        assert L.icp_tsdf_last_error(t)
        assert_bits(dev.read()[0], vol.dw, "the volume after a refusal")
        assert_bits(g.read(Mem.F), F, "F after a refusal")

    def opt(its=20, ang=0.001, tra=0.01):
        return C.byref(tsdf.icp_tsdf_register_t(its, ang, tra))

    refused(L.icp_tsdf_register(t, None, None, 4, pp, op))
    refused(L.icp_tsdf_register(t, None, cp, 4, None, op))
    refused(L.icp_tsdf_register(t, None, cp, 4, pp, None))
    refused(L.icp_tsdf_register(t, None, cp, 0, pp, op))
    refused(L.icp_tsdf_register(t, None, cp, (1 << 20) + 1, pp, op))
    refused(L.icp_tsdf_register(t, None, cp, 4, nan_pose.ctypes.data, op))
    for bad in (opt(0), opt(257), opt(20, -1.0), opt(20, float("nan")), opt(20, 0.001, float("inf")), opt(20, 0.001, -0.5)):
        refused(L.icp_tsdf_register(t, bad, cp, 4, pp, op))
        refused(L.icp_tsdf_register_from(t, bad, g._h, Mem.M, pp, op))
    refused(L.icp_tsdf_register_from(t, None, None, Mem.M, pp, op))
    refused(L.icp_tsdf_register_from(t, None, g._h, Mem.M, None, op))
    refused(L.icp_tsdf_register_from(t, None, g._h, Mem.M, pp, None))
    refused(L.icp_tsdf_register_from(t, None, g._h, Mem.M, nan_pose.ctypes.data, op))
    refused(L.icp_tsdf_register_from(t, None, g._h, Mem.T, pp, op))
    fresh = engine.ICP(0)
    refused(L.icp_tsdf_register_from(t, None, fresh._h, Mem.M, pp, op), ESTATE)
    fresh.close()
    assert L.icp_tsdf_register(t, opt(1, 0.0, 0.0), cp, 4, pp, op) == 0 and out.singular == 1      # one plane
    with pytest.raises(ValueError):
        dev.register(np.zeros((3, 7), F32), pose)
    g.close()
    # tracked frames in flight
    g = engine.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    F = g.read(Mem.F).copy()
    g.track_submit(engine.synth_cloud_vga())
    assert L.icp_tsdf_register_from(t, None, g._h, Mem.M, pp, op) == ESTATE and L.icp_tsdf_last_error(t)
    g.track_collect()
    g.close(); dev.close()


def test_track_to_volume_is_the_loop_written_out(engine):
    from icp_amd import tsdf
    d = T.corner_camera(**TRACK_CAM)
    P = [START]
    for _ in range(3):
        P.append(T.rotate_pose(P[-1], (0.3, 1.0, 0.2), 1.0, (6.0, -5.0, 6.0)))
    frames = [T.render_corner(p, d)[:2] for p in P]
    cfg = T.corner_volume(colour=1)
    ref = T.Volume(cfg)
    want = G.track_to_volume(ref, d, frames, _p12(P[0]), lambda depth, rgb: R.landmarks(depth, rgb, d, 64)[0], 10)
    bounds = []
    for i in range(1, 4):
        rot, tra = pose_errors(want[i][0], P[i])
        print("track_to_volume (restatement) frame %d: k %d members %d rotation error %.4f degrees translation error %.3f" % (i, want[i][1].iterations, want[i][1].members, rot, tra))
        assert want[i][1].members > 0 and not want[i][1].singular
        bounds.append((3 * rot, 3 * tra))
    g, dev = _handle(engine, d), tsdf.TSDFVolume(tsdf.TSDFConfig(**cfg))
    got = list(tsdf.track_to_volume(g, dev, frames, _p12(P[0]), 10))
    assert len(got) == 4 and got[0][1] is None
    for i, ((pg, rg), (pw, rw)) in enumerate(zip(got, want)):
        assert_bits(pg, pw, "pose of frame %d" % i)
        if i:
            _assert_record(rg, rw, "record of frame %d" % i)
            rot, tra = pose_errors(pg, P[i])
            assert rot <= bounds[i - 1][0] and tra <= bounds[i - 1][1], (i, rot, tra, bounds[i - 1])
    dw, col = dev.read()
    assert_bits(dw, ref.dw, "the volume after four frames")
    assert_bits(col, ref.rgb, "its colour")
    g.close(); dev.close()


def test_timing_entry(engine):
    vol, cloud, pose = corner()[1], frame_cloud(TRUE_1), _p12(START)
    dev = _device(vol)
    assert dev.time_register(8, cloud, pose, reps=3) > 0 and dev.time_register(9, cloud, pose, reps=3) > 0
    _assert_record(dev.register(cloud, pose, 2), G.register(vol, cloud, pose, 2), "after the timed launches")
    dev.close()


def test_cpp_facade_program():
    """tests/cpp/tsdf_register_facade_test.cpp: TSDFVolume::registerCloud / registerFrom against the C-ABI they wrap."""
    exe = os.path.join(ROOT, "tests", "cpp", "tsdf_register_facade_test")
    assert os.path.exists(exe), "tests/cpp/tsdf_register_facade_test is built by build() / make tsdf_register_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tsdf register facade ok" in out.stdout, (out.stdout, out.stderr)
