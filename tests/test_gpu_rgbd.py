"""GPU tests of the RGB-D front end (icp_rgbd.hip, icp_amd/rgbd.py) against its numpy restatement (rgbd_ref.py): everything bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import icp_checks as K
import rgbd_ref as R
from icp_checks import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 4
F32 = np.float32


def _cfg(rgbd, d):
    return rgbd.RGBDConfig(**d)


# ---- inputs, computed once ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frame(f):
    """Frame f of the synthetic sequence as a sensor would deliver it: z quantised to counts, the colour to bytes."""
    import icp_amd
    c = icp_amd.synth_cloud_vga(moved=f).reshape(480, 640, 8)
    depth = np.rint(c[..., 2]).astype(np.uint16)
    rgb = np.rint(c[..., 4:7] * 255).astype(np.uint8)
    depth.flags.writeable = rgb.flags.writeable = False
    return depth, rgb


@functools.lru_cache(maxsize=None)
def _holes(kind):
    """Frame 0's counts with 30 % holes: contiguous, scattered, or both (20 % and 12.5 %: 30 % together)."""
    import icp_amd
    c = icp_amd.synth_cloud_vga()
    parts = {"contiguous": [(icp_amd.HOLES_CONTIGUOUS, 0.3)], "scattered": [(icp_amd.HOLES_SCATTERED, 0.3)],
             "both": [(icp_amd.HOLES_CONTIGUOUS, 0.2), (icp_amd.HOLES_SCATTERED, 0.125)]}[kind]
    for i, (pattern, fraction) in enumerate(parts):
        c = icp_amd.punch_holes(c, 640, 480, pattern, fraction, True, seed=77 + i)
    depth = np.rint(c.reshape(480, 640, 8)[..., 2]).astype(np.uint16)
    assert 0.25 < (depth == 0).mean() < 0.35
    depth.flags.writeable = False
    return depth


@functools.lru_cache(maxsize=None)
def _host_cloud(f):
    """The float8 cloud a host makes of frame f with the reference's writer (the restatement at the defaults)."""
    c = R.cloud(*_frame(f), R.config())
    c.flags.writeable = False
    return c


def _images(W, H, S):
    """The depth images of test 1 at one size (name, counts, extra configuration)."""
    rng = np.random.default_rng(W * 1000 + H)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    half = (u >= (W + 1) // 2)
    crop = lambda a: np.ascontiguousarray(a[200:200 + H, 300:300 + W]) if (H, W) != (480, 640) else a
    out = [("constant", np.full((H, W), 1234), {}),
           ("ramp", 800 + 3 * u + 7 * v, {}),
           ("step S", 1000 + S * half + (v % 2), {}),
           ("step S - 1", 1000 + (S - 1) * half + (v % 2), {}),
           ("noise", 2000 + rng.integers(-40, 41, (H, W)), {}),
           ("holes contiguous", crop(_holes("contiguous")), {}),
           ("holes scattered", crop(_holes("scattered")), {}),
           ("all invalid", np.zeros((H, W)), {}),
           ("d_min d_max", np.array([499, 500, 1500, 1501, 1000])[(u + 2 * v) % 5], {"d_min": 500, "d_max": 1500}),
           ("full of 65535", np.full((H, W), 65535), {})]
    return [(n, np.asarray(d).astype(np.uint16), e) for n, d, e in out]


# ---- 1. the dense form ---------------------------------------------------------------------------------------------------------------

def _check_dense(rgbd, depth, rgb, d, normals, what):
    got = rgbd.to_cloud(depth, rgb, _cfg(rgbd, d), normals=normals)
    want = R.cloud(depth, rgb, d)
    if normals:
        assert_bits(got[0], want, what + ": cloud")
        assert_bits(got[1], R.normals(want, d), what + ": normals")
    else:
        assert_bits(got, want, what + ": cloud")


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (37, 29), (64, 16)])
def test_dense_form_equals_the_restatement(engine, W, H):
    """Every (r, S) of {0, 1, 6} x {1, 30, 4095} on every depth image; with and without colour and normals, default and other intrinsics and
    depth_scale taking turns — and all four together on the noise image."""
    from icp_amd import rgbd
    rng = np.random.default_rng(W + H)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    other = dict(fx=525.5, fy=517.25, cx=W / 3.0, cy=H / 2.5, depth_scale=0.001)
    turn = 0
    for r in (0, 1, 6):
        for S in (1, 30, 4095):
            for name, depth, extra in _images(W, H, S):
                variants = [(turn & 1, turn & 2, turn & 4)]
                if name == "noise":
                    variants = [(a, b, c) for a in (0, 1) for b in (0, 2) for c in (0, 4)]
                for colour, normals, intr in variants:
                    d = R.config(width=W, height=H, radius=r, range=S, **extra, **(other if intr else {}))
                    _check_dense(rgbd, depth, rgb if colour else None, d, bool(normals), "%s r=%d S=%d %s" % (name, r, S, (colour, normals, intr)))
                turn += 1


def test_dense_form_at_640_x_480(engine):
    """Once at the sensor's size: 30 % holes of both kinds, r = 6, colour and normals."""
    from icp_amd import rgbd
    d = R.config(radius=6, range=30)
    _check_dense(rgbd, _holes("both"), _frame(0)[1], d, True, "640 x 480")


# ---- 2. the default configuration is today's path -----------------------------------------------------------------------------------------

def test_default_configuration_is_write_cloud(engine):
    from icp_amd import rgbd
    Mem = engine.Memory
    depth, rgb = _frame(0)
    g, o = engine.ICP(0), engine.ICP(0)
    for x in (g, o):
        x.init(16384, 256, 2e2, 1e-6)
    assert rgbd.get_config(g) == rgbd.RGBDConfig.kinect()
    for which in (Mem.M, Mem.F):
        rgbd.write(g, which, depth, rgb)
        o.write_cloud(which, _host_cloud(0))
        assert_bits(g.read(which), o.read(which), "landmarks of memory %d" % which)
        assert np.any(g.read(which)[:, 2] != 0)
    g.close(); o.close()


def test_timing_entry_disturbs_nothing(engine):
    """icp_time_rgbd (tools/diag/rgbd_time.py) runs either form into scratch: F, M and the normals stay as they are."""
    from icp_amd import rgbd
    Mem = engine.Memory
    depth, rgb = _frame(1)
    g = engine.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    rgbd.set_config(g, rgbd.RGBDConfig(radius=2))
    rgbd.write(g, Mem.M, depth, rgb, normals=True)
    M, N = g.read(Mem.M).copy(), g.read(Mem.NORMALS_M).copy()
    for dense in (0, 1):
        assert rgbd.time_kernel(g, dense, _frame(2)[0], None, normals=True, reps=2) > 0
    assert_bits(g.read(Mem.M), M, "M")
    assert_bits(g.read(Mem.NORMALS_M), N, "NORMALS_M")
    g.close()


# ---- 3. the lattice form is the dense form picked at the lattice -------------------------------------------------------------------------

LATTICES = {
    "default": (dict(radius=3, range=30), 128, 256),
    "16 x 16 of 20 x 18": (dict(width=20, height=18, x0=2, y0=1, step_x=1, step_y=1, radius=2, range=30), 16, 4),
    "whole image": (dict(width=16, height=16, x0=0, y0=0, step_x=1, step_y=1, radius=6, range=4095), 16, 4),
    "first to last": (dict(width=46, height=31, x0=0, y0=0, step_x=3, step_y=2, radius=1, range=30), 16, 4),
    "steps (5, 2)": (dict(width=80, height=40, x0=2, y0=3, step_x=5, step_y=2, radius=3, range=50), 16, 4),
}


@pytest.mark.parametrize("name", list(LATTICES))
def test_lattice_form_equals_dense_form_at_the_lattice(engine, name):
    from icp_amd import rgbd
    Mem = engine.Memory
    extra, side, nr = LATTICES[name]
    d = R.config(**extra)
    W, H = d["width"], d["height"]
    if (W, H) == (640, 480):
        depth, rgb = _holes("both"), _frame(0)[1]
    else:
        rng = np.random.default_rng(W)
        depth = (1500 + rng.integers(-25, 26, (H, W))).astype(np.uint16)
        depth[rng.random((H, W)) < 0.2] = 0
        depth[0, 0], depth[H - 1, W - 1] = 1500, 1490                  # (the corners' windows and neighbours clip: keep them valid)
        rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    cloud, nrm = rgbd.to_cloud(depth, rgb, _cfg(rgbd, d), normals=True)
    at = R.lattice(d, side)
    want_lm, want_n = R.landmarks(depth, rgb, d, side, True)
    assert_bits(cloud[at], want_lm, name + ": the dense form itself")
    g = engine.ICP(0)
    g.init(side * side, nr, 2e2, 1e-6)
    rgbd.set_config(g, _cfg(rgbd, d))
    for which, nmem in ((Mem.F, Mem.NORMALS_F), (Mem.M, Mem.NORMALS_M)):
        rgbd.write(g, which, depth, rgb, normals=True)
        assert_bits(g.read(which), cloud[at], name + ": landmarks")
        assert_bits(g.read(nmem), nrm[at], name + ": normals")
    rgbd.write(g, Mem.F, depth, None)                                  # no colour image, no normals: the colour lanes are 0, the normals stay
    noc = cloud[at].copy(); noc[:, 4:7] = 0
    assert_bits(g.read(Mem.F), noc, name + ": landmarks without colour")
    assert_bits(g.read(Mem.NORMALS_F), want_n, name + ": normals stay")
    g.close()


# ---- 4. the normals reach the plane system ---------------------------------------------------------------------------------------------

def test_front_end_normals_feed_point_to_plane(engine):
    from icp_amd import rgbd
    Mem = engine.Memory
    d = R.config(radius=3, range=30)
    (dF, cF), (dM, cM) = _frame(0), _frame(1)
    F, NF = R.landmarks(dF, cF, d, 128, True)
    M, _ = R.landmarks(dM, cM, d, 128)
    a = K.make_plane(engine, 128, 256, normals=K.GIVEN)
    rgbd.set_config(a, _cfg(rgbd, d))
    rgbd.write(a, Mem.F, dF, cF, normals=True)
    rgbd.write(a, Mem.M, dM, cM)
    assert_bits(a.read(Mem.NORMALS_F), NF, "NORMALS_F")
    assert np.count_nonzero(np.any(NF[:, :3] != 0, axis=1)) > 12000
    b = K.make_plane(engine, 128, 256, normals=K.GIVEN)
    K.load(engine, b, F, M)
    b.write(Mem.NORMALS_F, NF)
    for g in (a, b):
        g.buildRBC()
    K.check_step(engine, a, K.restate_p2pl(0.05))
    b.step()
    for mem in (Mem.T, Mem.R, Mem.TK, Mem.PLANE_SYSTEM, Mem.NN, Mem.QT):
        assert_bits(a.read(mem), b.read(mem), "memory %d" % mem)
    assert a.state().k == b.state().k == 1
    a.close(); b.close()


# ---- 5. tracking -----------------------------------------------------------------------------------------------------------------------

ORDER = [0, 1, 2, 3, 4, 2, 0]


def _pipelined(g, submit, n, depth=2):
    out, inflight = [], 0
    for i in range(n):
        if inflight >= depth:
            out.append(g.track_collect()); inflight -= 1
        submit(i); inflight += 1
    while inflight:
        out.append(g.track_collect()); inflight -= 1
    return out


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("form", ["blocking", "pipelined", "alternating"])
def test_tracking_from_images_equals_tracking_from_host_made_clouds(engine, form, warm):
    """r = 0: every hop's k and T8 equal a second handle's, fed the host-made float8 clouds."""
    from icp_amd import rgbd
    Mem = engine.Memory
    g, o = engine.ICP(0), engine.ICP(0)
    for x in (g, o):
        x.init(16384, 256, 2e2, 1e-6)
    n = len(ORDER)
    if form == "blocking":
        for i in ORDER:
            kg, ko = rgbd.track_next(g, *_frame(i), warm_start=warm), o.track_next(_host_cloud(i), warm)
            assert kg == ko, (i, kg, ko)
            assert_bits(g.read(Mem.T), o.read(Mem.T), "T of frame %d" % i)
    else:
        def submit(i):
            if form == "alternating" and i % 2 == 0:
                g.track_submit(_host_cloud(ORDER[i]), warm)
            else:
                rgbd.track_submit(g, *_frame(ORDER[i]), warm_start=warm)
        got = _pipelined(g, submit, n)
        want = o.track_pipelined([_host_cloud(i) for i in ORDER], warm_start=warm, depth=2)
        assert got[0] is None and want[0] is None and len(got) == n
        for i in range(1, n):
            assert got[i][0] == want[i][0], (i, got[i][0], want[i][0])
            assert_bits(got[i][1], want[i][1], "T8 of hop %d" % i)
    assert_bits(g.read(Mem.M), o.read(Mem.M), "the last frame's landmarks")
    assert_bits(g.read(Mem.F), o.read(Mem.F), "the frame before")
    # the sequence continues correctly after a reset
    g.track_reset(); o.track_reset()
    for i in (3, 1, 4):
        kg, ko = rgbd.track_next(g, *_frame(i), warm_start=warm), o.track_next(_host_cloud(i), warm)
        assert kg == ko, (i, kg, ko)
        assert_bits(g.read(Mem.T), o.read(Mem.T), "T of frame %d after the reset" % i)
    g.close(); o.close()


def test_tracked_landmarks_are_the_filtered_ones(engine):
    """r = 3: the landmarks read back after a collect equal the restatement (with two frames in flight; one frame without a colour image)."""
    from icp_amd import rgbd
    Mem = engine.Memory
    d = R.config(radius=3, range=30)
    g = engine.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    rgbd.set_config(g, _cfg(rgbd, d))
    frames = [(_holes("both"), _frame(0)[1]), _frame(1), (_frame(2)[0], None)]
    res = _pipelined(g, lambda i: rgbd.track_submit(g, *frames[i]), 3)
    assert res[0] is None and res[1] is not None and res[2] is not None
    assert_bits(g.read(Mem.M), R.landmarks(*frames[2], d, 128)[0], "frame 2")
    assert_bits(g.read(Mem.F), R.landmarks(*frames[1], d, 128)[0], "frame 1")
    g.track_reset()
    assert rgbd.track_next(g, *frames[0]) is None
    assert_bits(g.read(Mem.M), R.landmarks(*frames[0], d, 128)[0], "frame 0 (holes)")
    g.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_configuration_as_it_was(engine):
    from icp_amd import rgbd
    g = engine.ICP(0)
    kept = rgbd.RGBDConfig(radius=2, range=77, fx=500.0)
    rgbd.set_config(g, kept)                                           # (before init: it survives it)
    g.init(16384, 256, 2e2, 1e-6)
    assert rgbd.get_config(g) == kept
    bad = [dict(radius=7), dict(range=0), dict(range=4096), dict(step_x=0), dict(step_y=0), dict(width=0), dict(width=4097), dict(height=0),
           dict(height=4097), dict(fx=0.0), dict(fx=-1.0), dict(fx=float("nan")), dict(fy=float("inf")), dict(cx=float("nan")),
           dict(depth_scale=0.0), dict(d_min=200, d_max=100), dict(d_max=65536),
           dict(x0=132), dict(y0=99), dict(step_x=5), dict(width=512)]                       # (the lattice leaves the image for m = 16384)
    for b in bad:
        with pytest.raises(engine.ICPError) as e:
            rgbd.set_config(g, rgbd.RGBDConfig(**{**kept.as_dict(), **b}))
        assert e.value.code == EINVAL, b
        assert rgbd.get_config(g) == kept, b
    rgbd.set_config(g, rgbd.RGBDConfig(**{**kept.as_dict(), "d_min": 0, "d_max": 0}))         # (in range: no count is valid)
    rgbd.set_config(g, kept)
    depth, rgb = _frame(0)
    with pytest.raises(engine.ICPError) as e:
        rgbd.write(g, engine.Memory.T, depth, rgb)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        rgbd.write(g, engine.Memory.F, depth.astype(np.float32), rgb)
    # with a frame in flight the configuration cannot change
    g.track_submit(_host_cloud(0))
    with pytest.raises(engine.ICPError) as e:
        rgbd.set_config(g, rgbd.RGBDConfig())
    assert e.value.code == ESTATE and rgbd.get_config(g) == kept
    g.track_collect()
    rgbd.set_config(g, kept)
    assert rgbd._lib().icp_set_rgbd(g._h, None) == 0                   # (cfg == NULL: the defaults)
    assert rgbd.get_config(g) == rgbd.RGBDConfig()
    # a handle whose m the lattice does not fit: the write and the tracked frame are refused
    s = engine.ICP(0)
    s.init(65536, 1024, 2e2, 1e-6)
    with pytest.raises(engine.ICPError) as e:
        rgbd.write(s, engine.Memory.F, depth, rgb)
    assert e.value.code == EINVAL
    s.close(); g.close()
    # the one-call operation checks the same ranges
    with pytest.raises(engine.ICPError) as e:
        rgbd.to_cloud(depth, rgb, rgbd.RGBDConfig(radius=7))
    assert e.value.code == EINVAL


def test_a_pyramid_level_is_refused(engine):
    from icp_amd import rgbd
    p = engine.ICPPyramid(0)
    p.init(16384, [256, 64], 2e2, 1e-6)
    depth, rgb = _frame(0)
    for call in (lambda: rgbd.write(p.level(0), engine.Memory.F, depth, rgb), lambda: rgbd.track_next(p.level(0), depth, rgb),
                 lambda: rgbd.track_submit(p.level(0), depth, rgb)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == ESTATE
    p.close()


# ---- 7. the layers above ---------------------------------------------------------------------------------------------------------------

def test_cpp_facade_program():
    """tests/cpp/rgbd_facade_test.cpp: ICPStep::setRGBD / writeRGBD, ICPTrack::nextRGBD / submitRGBD and RGBDTo8D against the C-ABI they wrap."""
    exe = os.path.join(ROOT, "tests", "cpp", "rgbd_facade_test")
    assert os.path.exists(exe), "tests/cpp/rgbd_facade_test is built by build() / make rgbd_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rgbd facade ok" in out.stdout, (out.stdout, out.stderr)


def test_command_line_writes_the_pc8d_file(engine, tmp_path):
    from icp_amd import io, rgbd
    depth, rgb = _frame(0)
    depth.astype("<u2").tofile(tmp_path / "d.raw")
    rgb.tofile(tmp_path / "c.raw")
    assert rgbd.main([str(tmp_path / "d.raw"), str(tmp_path / "c.raw"), str(tmp_path / "o.bin")]) == 0
    assert_bits(io.load_pc8d(str(tmp_path / "o.bin")), _host_cloud(0), "the default configuration's cloud")
