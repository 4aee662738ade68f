"""CPU tests of coarse-to-fine registration (icp_pyramid_*, include/icp_amd.h): the reduction rule restated in numpy (pyramid_ref) on
hand-made blocks, the convergence basin a pyramid buys on the CPU oracle, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import pyramid_ref as PR

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _pt(x, y, z, r=0.5, g=0.25, b=0.125):
    return [x, y, z, 1.0, r, g, b, 1.0]


def _level_of_one_block(p0, p1, p2, p3):
    """A 2 x 2 level whose only block is (p0, p1, p2, p3) in block order."""
    return np.array([p0, p1, p2, p3], F32)


def test_pick_is_the_strided_grid(engine):
    F, _ = engine.synth_pair(32)
    for side, X in ((32, F), (16, PR.reduce_level(F, 32, 1, PR.PICK))):
        got = PR.reduce_level(X, side, 1, PR.PICK)
        want = X.reshape(side, side, 8)[::2, ::2].reshape(-1, 8)
        assert np.array_equal(_bits(got), _bits(want))
    lv = PR.build(F, 32, 3, PR.PICK)
    assert [a.shape for a in lv] == [(1024, 8), (256, 8), (64, 8)]
    assert np.array_equal(_bits(lv[2]), _bits(F.reshape(32, 32, 8)[::4, ::4].reshape(-1, 8)))


def test_mean_of_four_valid_points_in_block_order():
    a, b, c, d = _pt(1, 2, 1000), _pt(3, 5, 1001, 0.1, 0.2, 0.3), _pt(1e-3, 7, 1002), _pt(2, 2, 1003.5)
    out = PR.reduce_level(_level_of_one_block(a, b, c, d), 2, 1)[0]
    A = np.array([a, b, c, d], F32)
    for col in (0, 1, 2, 4, 5, 6):
        s = A[0, col]
        for i in (1, 2, 3):
            s = F32(s + A[i, col])
        assert out[col] == F32(s / F32(4))
    assert out[3] == 1.0 and out[7] == 1.0


def test_mean_skips_invalid_points_and_keeps_an_all_invalid_block():
    hole = [0, 0, 0, 1.0, 0.3, 0.6, 0.9, 1.0]
    nanp = _pt(np.nan, 1, 1000)
    infp = _pt(1, -np.inf, 1000)
    a, b = _pt(10, 20, 1000, 0.2, 0.4, 0.6), _pt(12, 24, 1010, 0.4, 0.8, 0.2)
    out = PR.reduce_level(_level_of_one_block(hole, a, nanp, b), 2, 1)[0]       # the reference point is the first VALID one
    assert np.array_equal(out, np.array([11, 22, 1005, 1, F32(F32(0.2) + F32(0.4)) / F32(2), F32(F32(0.4) + F32(0.8)) / F32(2),
                                         F32(F32(0.6) + F32(0.2)) / F32(2), 1], F32))
    # none valid: element 0's bits, a NaN payload and w != 1 included
    weird = np.array([nanp, hole, infp, hole], F32)
    weird[0, 3] = 7.0
    weird.view(np.uint32)[0, 0] = 0x7FC12345
    out = PR.reduce_level(weird, 2, 1)
    assert np.array_equal(out.view(np.uint32)[0], weird.view(np.uint32)[0])
    assert not PR.valid(out)[0]


def test_band_excludes_a_far_point_and_doubles_per_level():
    a, b, c, d = _pt(0, 0, 1000), _pt(2, 0, 1024), _pt(0, 2, 1025), _pt(2, 2, 900)
    X = _level_of_one_block(a, b, c, d)
    out = PR.reduce_level(X, 2, 1, PR.MEAN, 24.0)[0]                 # |dz| <= 24: a and b
    assert out[0] == 1.0 and out[1] == 0.0 and out[2] == 1012.0
    out = PR.reduce_level(X, 2, 2, PR.MEAN, 24.0)[0]                 # the same block at the transition to level 2: band 48 takes c too
    assert out[2] == F32(F32(F32(1000) + F32(1024)) + F32(1025)) / F32(3)
    assert PR.band_of(24.0, 1) == 24.0 and PR.band_of(24.0, 2) == 48.0 and PR.band_of(24.0, 4) == 192.0
    cen = PR.block_census(X, 2, 1, 24.0)
    assert cen == dict(blocks=1, none=0, some=1, four=0, with_valid=1, band_cut=1)
    # 0 and +inf: no band test, the same bits
    z = PR.reduce_level(X, 2, 1, PR.MEAN, 0.0)
    i = PR.reduce_level(X, 2, 1, PR.MEAN, np.inf)
    assert np.array_equal(_bits(z), _bits(i))
    assert z[0, 2] == F32(F32(F32(F32(1000) + F32(1024)) + F32(1025)) + F32(900)) / F32(4)


def test_a_single_point_keeps_its_minus_zero():
    hole = [0, 0, 0, 1.0, 0, 0, 0, 1.0]
    p = [-0.0, 5.0, 1000.0, 1.0, -0.0, 0.5, 0.5, 1.0]
    out = PR.reduce_level(_level_of_one_block(hole, hole, p, hole), 2, 1)
    assert np.array_equal(_bits(out)[0], _bits(np.array(p, F32)))
    assert np.signbit(out[0, 0]) and np.signbit(out[0, 4])


def test_levels_are_derived_recursively(engine):
    F, _ = engine.synth_pair(16)
    lv = PR.build(F, 16, 3, PR.MEAN, 8.0)
    assert np.array_equal(_bits(lv[2]), _bits(PR.reduce_level(lv[1], 8, 2, PR.MEAN, 8.0)))


# ---- the convergence basin (ISSUE: "Why this is next"): a 10 degree motion is outside the single-level basin and inside the chain's ----
@pytest.fixture(scope="module")
def basin(engine, oracle):
    return PR.basin_case(engine, oracle)


def test_three_levels_widen_the_convergence_basin(basin):
    """Measured: single level 40 iterations, not converged, 2.75 deg / 247 mm from T_true; the chain 40 / 11 / 22 iterations (coarsest
    first), level 0 converged, 0.152 deg / 9.3 mm."""
    deg1, mm1 = PR.error_to(basin["single"][0]["T"], basin["T_true"])
    degc, mmc = PR.error_to(basin["chain"][0]["T"], basin["T_true"])
    print("single: k %d converged %s %.3f deg %.1f mm" % (basin["single"][0]["k"], basin["single"][0]["converged"], deg1, mm1))
    print("chain:  k %s converged %s %.3f deg %.1f mm" % ([r["k"] for r in basin["chain"]], basin["chain"][0]["converged"], degc, mmc))
    assert deg1 > 1.0
    assert basin["chain"][0]["converged"] and degc < 0.5


# ---- argument checks that need no device ----
def test_entry_points_without_a_device(engine):
    L = engine.lib()
    p = C.c_void_p()
    assert L.icp_pyramid_create(None, 0, 1, 1) == 1
    rc = L.icp_pyramid_create(C.byref(p), 0, 1, 1)
    if rc == 0:                                                      # (a GPU box)
        assert L.icp_pyramid_destroy(p) == 0
    else:
        assert rc == 5 and not p.value                               # ICP_ENODEVICE: no CPU fallback, as icp_create
        assert b"icp_pyramid_create" in L.icp_pyramid_last_error(None)
    nr = (C.c_uint32 * 3)(256, 64, 64)
    u, k, z, h = C.c_uint32(), C.c_int(), C.c_float(), C.c_void_p()
    assert L.icp_pyramid_destroy(None) == 1
    assert L.icp_pyramid_init(None, 3, 16384, nr, 2e2, 1e-6, nr, 0.001, 0.01) == 1
    assert L.icp_pyramid_set_reduction(None, 0, 0.0) == 1
    assert L.icp_pyramid_get_reduction(None, C.byref(k), C.byref(z)) == 1
    assert L.icp_pyramid_levels(None, C.byref(u)) == 1
    assert L.icp_pyramid_level(None, 0, C.byref(h)) == 1
    assert L.icp_pyramid_write(None, 0, None, 0) == 1
    assert L.icp_pyramid_write_cloud(None, 0, None, 0) == 1
    assert L.icp_pyramid_reset_transform(None) == 1
    assert L.icp_pyramid_build_rbc(None) == 1
    assert L.icp_pyramid_run(None, None) == 1
    assert L.icp_pyramid_run_fixed(None, nr) == 1
    assert L.icp_pyramid_sync(None) == 1
    if rc:
        with pytest.raises(engine.ICPError) as e:
            engine.ICPPyramid(0)
        assert e.value.code == 5


# ---- the command lines (argument parsing needs no device) ----
def test_command_lines_have_the_option():
    import inspect
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and "--pyramid" in r.stdout and "LEVELS[:MAXDZ]" in r.stdout, r.stderr
    exe = os.path.join(root, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("0", "6", "3:-1", "3:nan", "x", "3:"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--pyramid", bad], capture_output=True, text=True, cwd=root)
        assert r.returncode == 2 and "--pyramid" in r.stderr, (bad, r.stderr)
        r = subprocess.run([exe, "--pyramid", bad], capture_output=True, text=True, cwd=root)
        assert r.returncode == 2 and "--pyramid: LEVELS[:MAXDZ]" in r.stderr, (bad, r.stderr)
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["pyramid"].default is None
    assert register._pyramid("3") == (3, 0.0) and register._pyramid("2:24") == (2, 24.0)
    assert register.pyramid_nr(3) == [256, 64, 64] and register.pyramid_nr(1) == [256]


# ---- the construction kernel's resources (compiler only) ----
def test_construction_kernel_uses_no_scratch_and_fits_its_block():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_pyramid.hip")
    assert list(res) == ["k_pyramid_build"], list(res)
    r = res["k_pyramid_build"]
    assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False"), r
    assert r["lds"] == (512 + 128) * 16, r                           # the two tile buffers, nothing else
    assert r["vgprs"] <= 128 and r["occupancy"] >= 4, r              # 256-thread blocks: several per CU
