"""GPU tests of coarse-to-fine registration (icp_pyramid_*, include/icp_amd.h): the levels the device builds against the numpy
restatement (pyramid_ref) bit for bit, the chain of runs against the CPU oracle's chain bit for bit, per-level options against a chain
of plain handles made by hand, and the status codes."""
import ctypes as C

import numpy as np
import pytest

import icp_checks as K
import pyramid_ref as PR

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 7
# shape -> (levels, nr per level finest first, max_dz whose band excludes a point in 10 - 90 % of the blocks at every transition:
# picked per shape on the CPU — 24 cuts 42 - 45 % at side 128, 54 - 57 % at 100, 44 - 67 % at 96; 12 cuts 42 - 46 % at 256)
SHAPES = {128: (3, (256, 64, 64), 24.0), 100: (2, (4, 4), 24.0), 96: (5, (4, 4, 4, 4, 4), 24.0), 256: (2, (1024, 256), 12.0)}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %08x != %08x" % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


_PYR = {}


@pytest.fixture(scope="module")
def pyramids(engine):
    """One pyramid object per shape for the construction tests (created on first use, closed with the module)."""
    def get(side):
        if side not in _PYR:
            levels, nr, _ = SHAPES[side]
            p = engine.ICPPyramid(0)
            p.init(side * side, nr, 2e2, 1e-6)
            assert p.levels == levels
            _PYR[side] = p
        return _PYR[side]
    yield get
    for p in _PYR.values():
        p.close()
    _PYR.clear()


_CLOUDS = {}


def _clouds(engine, side, name):
    if (side, name) not in _CLOUDS:
        if name == "clean":
            F, M = engine.synth_pair(side, seed=SEED)
        elif name == "blobs30":
            F, M = K.holes_pair(engine, side, SEED, "blobs30")
        else:
            F, M = K.messy_grid(engine, side, SEED), K.messy_grid(engine, side, SEED + 1)
        _CLOUDS[(side, name)] = (F, M)
    return _CLOUDS[(side, name)]


@pytest.mark.parametrize("kind", ["mean_band", "pick"])
@pytest.mark.parametrize("name", ["clean", "blobs30", "messy"])
@pytest.mark.parametrize("side", sorted(SHAPES))
def test_levels_match_the_restatement(engine, pyramids, side, name, kind):
    levels, nr, max_dz = SHAPES[side]
    F, M = _clouds(engine, side, name)
    k, dz = (PR.MEAN, max_dz) if kind == "mean_band" else (PR.PICK, 0.0)
    want = {engine.Memory.F: PR.build(F, side, levels, k, dz), engine.Memory.M: PR.build(M, side, levels, k, dz)}
    # the rule bites, shown on the expectation alone
    if kind == "mean_band":
        for X in want.values():
            for l in range(1, levels):
                c = PR.block_census(X[l - 1], side >> (l - 1), l, dz)
                assert 0.10 <= c["band_cut"] / c["with_valid"] <= 0.90, (side, name, l, c)
            if name == "blobs30":
                c = PR.block_census(X[0], side, 1, dz)
                assert min(c["none"], c["some"], c["four"]) >= 0.05 * c["blocks"], c
    p = pyramids(side)
    p.set_reduction(k, dz)
    assert p.reduction() == (k, dz)
    for mem, X in want.items():
        p.write(mem, X[0])
    for mem, X in want.items():
        for l in range(levels):
            got = p.level(l).read(mem)
            assert got.shape == ((side >> l) ** 2, 8)
            _same_bits(got, X[l], "side %d %s %s level %d mem %d" % (side, name, kind, l, mem))


def test_mean_without_a_band_and_the_setting_survives_init(engine, pyramids):
    p = pyramids(128)
    F, M = _clouds(engine, 128, "messy")
    p.set_reduction(PR.MEAN, float("inf"))
    p.init(128 * 128, SHAPES[128][1], 2e2, 1e-6)
    assert p.reduction() == (PR.MEAN, float("inf"))
    p.write(engine.Memory.F, F, block=True)
    want = PR.build(F, 128, 3, PR.MEAN, 0.0)
    for l in range(3):
        _same_bits(p.level(l).read(engine.Memory.F), want[l], "level %d" % l)
    p.set_reduction(PR.MEAN, 0.0)


def test_write_cloud_goes_through_get_lms(engine, oracle, pyramids):
    cloud = engine.synth_cloud_vga(seed=SEED, moved=1)
    p = pyramids(128)
    p.set_reduction(PR.MEAN, 24.0)
    want = PR.build(oracle.get_lms(cloud), 128, 3, PR.MEAN, 24.0)
    for mem in (engine.Memory.F, engine.Memory.M):
        p.write_cloud(mem, cloud)
        for l in range(3):
            _same_bits(p.level(l).read(mem), want[l], "mem %d level %d" % (mem, l))
    p.set_reduction(PR.MEAN, 0.0)


# ---- runs ----
MODES = {"fused": dict(power_fast=True, fused=True), "reference_order": dict(power_fast=False, fused=False)}


def _pyramid_for(engine, mode, nr=(256, 64, 64), m=128 * 128, max_iterations=40):
    p = engine.ICPPyramid(0)
    p.init(m, nr, 2e2, 1e-6, max_iterations)
    if mode == "reference_order":
        for l in range(p.levels):
            p.level(l).setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
            p.level(l).setPowerMode(engine.PowerMode.LITERAL)
    return p


@pytest.mark.parametrize("mode", sorted(MODES))
def test_run_fixed_is_the_oracle_chain(engine, oracle, mode):
    F, M = _clouds(engine, 128, "clean")
    Fs, Ms = PR.build(F, 128, 3), PR.build(M, 128, 3)
    want = PR.oracle_chain(oracle, Fs, Ms, (256, 64, 64), fixed=[3, 3, 3], a=2e2, c=1e-6, threads=4, **MODES[mode])
    p = _pyramid_for(engine, mode)
    try:
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M)
        p.buildRBC()
        p.run_fixed([3, 3, 3])
        p.sync()
        assert not p.pending()
        for l in range(3):
            lv = p.level(l)
            _same_bits(lv.read(engine.Memory.T), want[l]["T"], "%s level %d T" % (mode, l))
            _same_bits(lv.R, want[l]["R"], "%s level %d R" % (mode, l))
            assert lv.k == 3 == want[l]["k"]
    finally:
        p.close()


def test_run_fixed_only_enqueues(engine):
    """The call returns with the device still at work — seen by state (an event query), not by a clock.  The pass in flight is
    3 x 300 iterations, milliseconds of device work against the microseconds between the call's return and the query, and the
    collector is off in between: a host that had waited for anything would find the event done."""
    import gc
    F, M = _clouds(engine, 128, "clean")
    p = _pyramid_for(engine, "fused")
    try:
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M)
        p.buildRBC()
        p.run_fixed([300, 300, 300])                                 # (captures the levels' graphs)
        p.sync()
        assert not p.pending()
        gc.disable()
        try:
            p.run_fixed([300, 300, 300])
            waiting = p.pending()
        finally:
            gc.enable()
        p.sync()
        assert waiting and not p.pending()
        assert [p.level(l).k for l in range(3)] == [300, 300, 300]
    finally:
        p.close()


def test_calls_queued_behind_a_fixed_run_need_no_sync(engine, oracle):
    """run_fixed, then — with no sync in between — reset_transform + run_fixed, a written T + run_fixed, and a plain second run_fixed:
    whatever writes a level's T next is ordered behind the hand-over that still reads it, so each pass is the oracle chain from the
    start it was given."""
    F, M = _clouds(engine, 128, "clean")
    Fs, Ms = PR.build(F, 128, 3), PR.build(M, 128, 3)
    kw = dict(a=2e2, c=1e-6, threads=4, **MODES["fused"])
    its = [3, 3, 3]
    T1 = np.array([0.0, 0.01, 0.0, 1.0, 3.0, -2.0, 1.0, 1.0], F32)
    T1[:4] /= np.linalg.norm(T1[:4].astype(np.float64))
    first = PR.oracle_chain(oracle, Fs, Ms, (256, 64, 64), fixed=its, **kw)
    given = PR.oracle_chain(oracle, Fs, Ms, (256, 64, 64), fixed=its, T0=T1, **kw)
    p = _pyramid_for(engine, "fused")
    try:
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M)
        p.buildRBC()
        for _ in range(2):                                           # run, reset, run: nothing but enqueues
            p.run_fixed(its)
            p.reset_transform()
        p.run_fixed(its)
        p.sync()
        for l in range(3):
            _same_bits(p.level(l).read(engine.Memory.T), first[l]["T"], "after reset, level %d" % l)
        p.run_fixed(its)
        p.write(engine.Memory.T, T1)
        p.run_fixed(its)
        p.sync()
        for l in range(3):
            _same_bits(p.level(l).read(engine.Memory.T), given[l]["T"], "after a written T, level %d" % l)
        # a second run in a row goes on from the coarsest level's own state: against the same calls with the host waiting after each
        got = {}
        for wait in (True, False):
            p.write(engine.Memory.T, T1)
            for _ in range(2):
                if wait:
                    p.sync()
                p.run_fixed(its)
            p.sync()
            got[wait] = [p.level(l).read(engine.Memory.T) for l in range(3)]
        for l in range(3):
            _same_bits(got[False][l], got[True][l], "second run in a row, level %d" % l)
            assert not np.array_equal(_bits(got[True][l]), _bits(given[l]["T"]))
    finally:
        p.close()


def test_a_borrowed_level_refuses_what_takes_the_levels_apart(engine):
    p = engine.ICPPyramid(0)
    try:
        p.init(64 * 64, [64, 64], 2e2, 1e-6)
        lv = p.level(1)
        F, _ = engine.synth_pair(32, seed=SEED)
        cloud = np.zeros((480 * 640, 8), F32)
        for call in (lambda: lv.init(1024, 64), lambda: lv.write(engine.Memory.F, F), lambda: lv.write(engine.Memory.M, F),
                     lambda: lv.write_cloud(engine.Memory.F, cloud), lambda: lv.track_next(cloud), lambda: lv.track_submit(cloud),
                     lambda: lv.track_reset()):
            with pytest.raises(engine.ICPError) as e:
                call()
            assert e.value.code == 4 and "levels apart" in str(e.value)
        lv.write(engine.Memory.T, np.array([0, 0, 0, 1, 1, 2, 3, 1], F32), block=True)      # (T, normals and the setters stay open)
        assert np.array_equal(lv.read(engine.Memory.T), np.array([0, 0, 0, 1, 1, 2, 3, 1], F32))
        lv.close()
        assert p.level(0).read(engine.Memory.T).shape == (8,)        # (closing a borrowed level destroys nothing)
    finally:
        p.close()


def test_run_registers_what_a_single_level_does_not(engine, oracle):
    """The 10 degree pair of test_pyramid_cpu: the pyramid's k[] and every level's T are the oracle chain's bits, a plain handle is
    the single-level oracle's — so the device lands within 0.5 degrees where the single level stays more than 1 degree off."""
    b = PR.basin_case(engine, oracle)
    p = _pyramid_for(engine, "fused")
    g = engine.ICP(0)
    try:
        p.write(engine.Memory.F, b["F"])
        p.write(engine.Memory.M, b["M"])
        p.buildRBC()
        k = p.run()
        assert k == [r["k"] for r in b["chain"]], (k, [r["k"] for r in b["chain"]])
        for l in range(3):
            _same_bits(p.level(l).read(engine.Memory.T), b["chain"][l]["T"], "level %d T" % l)
            assert p.level(l).k == k[l]
        assert bool(p.level(0).state().converged) == b["chain"][0]["converged"]
        g.init(128 * 128, 256, 2e2, 1e-6)
        g.write(engine.Memory.F, b["F"])
        g.write(engine.Memory.M, b["M"])
        g.buildRBC()
        assert g.run() == b["single"][0]["k"]
        _same_bits(g.read(engine.Memory.T), b["single"][0]["T"], "single level T")
        assert PR.error_to(g.read(engine.Memory.T), b["T_true"])[0] > 1.0
        assert PR.error_to(p.level(0).read(engine.Memory.T), b["T_true"])[0] < 0.5
    finally:
        g.close()
        p.close()


def _opt_point_to_plane(engine, h, side_l):
    h.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.1)
    h.set_normals(engine.Normals.GRID, side_l)
    h.set_rejection(invalid=True, max_dist=80.0)
    h.set_trimming(0.8)


def _opt_symmetric(engine, h, side_l):
    h.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.1)
    h.set_normals(engine.Normals.GRID, side_l)
    h.set_symmetric(True)


def _opt_projective(engine, h, side_l):
    """Point-to-point behind the projection, r = 1, the level's own intrinsics under the MEAN reduction."""
    from icp_amd import register
    h.set_projective(side_l, *register.level_intrinsics(engine.grid_intrinsics(128), 128 // side_l), radius=1)


@pytest.mark.parametrize("case", ["point_to_plane_rejection_trimming", "symmetric", "projective"])
def test_options_per_level_match_a_chain_made_by_hand(engine, case):
    """Every level's own options (grid widths per level, the projection's intrinsics per level) take part: T, the plane system, the
    moving normals, the pairs and the projection's words of every level equal those of separate plain handles fed pyramid_ref's clouds,
    T handed on through the host.  The moving set is written a second time after buildRBC: with grid normals the levels' moving normals
    must follow the device-side write as they follow icp_write."""
    opt = {"point": _opt_point_to_plane, "symme": _opt_symmetric, "proje": _opt_projective}[case[:5]]
    F, M = _clouds(engine, 128, "blobs30")
    M0 = _clouds(engine, 128, "clean")[1]
    nr, its = (256, 64, 64), [3, 3, 3]
    Fs, Ms, M0s = PR.build(F, 128, 3), PR.build(M, 128, 3), PR.build(M0, 128, 3)
    mems = (engine.Memory.T, engine.Memory.NN_ID, engine.Memory.QT, engine.Memory.PROJECTIVE)
    if case != "projective":
        mems += (engine.Memory.PLANE_SYSTEM, engine.Memory.NORMALS_M)
    want = [None] * 3
    T = np.array([0, 0, 0, 1, 0, 0, 0, 1], F32)
    for l in (2, 1, 0):
        g = engine.ICP(0)
        try:
            opt(engine, g, 128 >> l)
            g.init(Fs[l].shape[0], nr[l], 2e2, 1e-6)
            g.write(engine.Memory.F, Fs[l])
            g.write(engine.Memory.M, M0s[l])
            g.buildRBC()
            g.write(engine.Memory.M, Ms[l])
            g.write(engine.Memory.T, T)
            g.run_fixed(its[l])
            want[l] = {mem: g.read(mem) for mem in mems}
            T = want[l][engine.Memory.T].reshape(-1).copy()
        finally:
            g.close()
    p = engine.ICPPyramid(0)
    try:
        p.init(128 * 128, nr, 2e2, 1e-6)
        for l in range(3):
            opt(engine, p.level(l), 128 >> l)
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M0)
        p.buildRBC()
        p.write(engine.Memory.M, M)
        p.run_fixed(its)
        p.sync()
        for l in range(3):
            for mem in mems:
                got = p.level(l).read(mem)
                assert np.array_equal(got.view(np.uint8), want[l][mem].view(np.uint8)), "%s level %d mem %d" % (case, l, mem)
        if case == "projective":
            for l in range(3):
                n, hits, outside, empty = (int(x) for x in want[l][engine.Memory.PROJECTIVE])
                assert n == hits + outside + empty and 2 * hits >= n and outside > 0 and empty > 0, (l, n, hits, outside, empty)
        else:
            assert np.any(want[0][engine.Memory.PLANE_SYSTEM] != 0)
            assert all(not want[l][engine.Memory.PROJECTIVE].any() for l in range(3))
        if case == "symmetric":
            assert np.any(want[2][engine.Memory.NORMALS_M] != 0)
    finally:
        p.close()


@pytest.mark.parametrize("kind", ["mean", "pick"])
def test_projective_levels_match_the_restatement(engine, oracle, kind):
    """One projective iteration per level (r = 1, a level's intrinsics by include/icp_amd.h: f / 2^l, and (c - (2^l - 1) / 2) / 2^l
    under MEAN, c / 2^l under PICK): every level's pairs, words and pieces against projective_ref.project on pyramid_ref's level
    clouds at the T the level started from — the identity at the coarsest level, the T of the level above at a finer one —, and the T
    it leaves.  projective_ref.pyramid_chain computes all of it on the CPU; tests/test_projective_cpu.py proves that every level has
    hits, outside queries and empty cells and no pixel at a rounding boundary."""
    import projective_ref as ref
    check_step = K.check_projective_step
    k = ref.PYRAMID_MEAN if kind == "mean" else ref.PYRAMID_PICK
    chain = ref.pyramid_chain(k)
    p = engine.ICPPyramid(0)
    try:
        p.init(ref.PYRAMID_SIDE ** 2, ref.PYRAMID_NR, 2e2, 1e-6)
        p.set_reduction(k, 0.0)
        for l, lv in enumerate(chain):
            p.level(l).set_projective(lv.side, *lv.intr, radius=1)
        p.write(engine.Memory.F, chain[0].F)
        p.write(engine.Memory.M, chain[0].M)
        p.buildRBC()
        p.run_fixed([1, 1, 1])
        p.sync()
        for l in (2, 1, 0):
            lv, h = chain[l], p.level(l)
            if l < 2:
                _same_bits(p.level(l + 1).read(engine.Memory.T), lv.T, "the T level %d started from" % l)
            _same_bits(h.read(engine.Memory.F), lv.F, "level %d F" % l)
            _same_bits(h.read(engine.Memory.M), lv.M, "level %d M" % l)
            got = check_step(engine, oracle, h, lv.res, lv.F, lv.M, lv.T, lv.side, True, K.WEIGHTED, K.POWER, True, pieces=lv.pieces)
            assert got[1] > 0 and got[2] > 0 and got[3] > 0, (l, got)
            _same_bits(h.read(engine.Memory.T), lv.T_next, "level %d T" % l)
            assert h.k == 1
    finally:
        p.close()


def test_a_second_run_and_a_rewritten_moving_set_give_the_first_bits(engine):
    F, M = _clouds(engine, 128, "clean")
    p = _pyramid_for(engine, "fused")
    try:
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M)
        p.buildRBC()
        k1 = p.run()
        T1 = [p.level(l).read(engine.Memory.T) for l in range(3)]
        p.reset_transform()
        assert p.run() == k1
        for l in range(3):
            _same_bits(p.level(l).read(engine.Memory.T), T1[l], "second run, level %d" % l)
        p.write(engine.Memory.M, M)
        p.reset_transform()
        assert p.run() == k1
        for l in range(3):
            _same_bits(p.level(l).read(engine.Memory.T), T1[l], "after re-writing M, level %d" % l)
    finally:
        p.close()


def test_status_codes(engine):
    L = engine.lib()
    p = engine.ICPPyramid(0)

    def code_of(fn, *a, **kw):
        with pytest.raises(engine.ICPError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    try:
        assert code_of(p.buildRBC)[0] == 4                           # before init
        assert code_of(p.init, 16384, [])[0] == 1                    # levels 0
        assert code_of(p.init, 16384, [64] * 6)[0] == 1              # levels 6
        assert code_of(p.init, 100 * 100, [4, 4, 4, 4])[0] == 1      # 100 % 8 != 0
        c, msg = code_of(p.init, 100 * 100, [4, 4, 1])               # sides 100, 50, 25: level 2 is odd
        assert c == 1 and "level 2" in msg
        c, msg = code_of(p.init, 16384, [256, 48, 64])
        assert c == 1 and "level 1" in msg
        assert code_of(p.set_reduction, 2, 0.0)[0] == 1
        assert code_of(p.set_reduction, PR.MEAN, -1.0)[0] == 1
        assert code_of(p.set_reduction, PR.MEAN, float("nan"))[0] == 1
        p.init(64 * 64, [64, 64], 2e2, 1e-6)
        assert code_of(p.level, 2)[0] == 1
        u, h = C.c_uint32(), C.c_void_p()
        assert L.icp_pyramid_levels(p._p, None) == 1 and L.icp_pyramid_level(p._p, 0, None) == 1
        assert L.icp_pyramid_get_reduction(p._p, None, None) == 1 and L.icp_pyramid_pending(p._p, None) == 1
        assert L.icp_pyramid_levels(p._p, C.byref(u)) == 0 and u.value == 2
        assert L.icp_pyramid_level(p._p, 1, C.byref(h)) == 0 and h.value
        assert code_of(p.run)[0] == 4                                # before build_rbc
        assert code_of(p.run_fixed, [1, 1])[0] == 4
        assert L.icp_pyramid_write(p._p, engine.Memory.S, None, 0) == 1   # not F, M or T
        cloud = np.zeros((480 * 640, 8), F32)
        assert code_of(p.write_cloud, engine.Memory.F, cloud)[0] == 1   # m != 16384
        F, M = engine.synth_pair(64, seed=SEED)
        p.write(engine.Memory.F, F)
        p.write(engine.Memory.M, M)
        p.buildRBC()
        assert L.icp_pyramid_run_fixed(p._p, None) == 1
        assert L.icp_pyramid_run(p._p, None) == 0                    # k may be NULL
    finally:
        p.close()


# ---- the layers above ----
def test_cpp_facade_program():
    """tests/cpp/pyramid_facade_test.cpp: cl_algo::ICP::ICPPyramid against the C-ABI it wraps (built by build())."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "pyramid_facade_test")
    assert os.path.exists(exe), "tests/cpp/pyramid_facade_test is built by build() / make pyramid_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pyramid facade ok" in out.stdout, (out.stdout, out.stderr)


def test_command_lines_register_coarse_to_fine(engine, oracle, tmp_path):
    """`python -m icp_amd.register --pyramid 3:24` (in process) and `examples/registration --pyramid 3:24` on a pair of 640 x 480
    clouds: both report the oracle chain's counts and transform, the options reach every level with its own grid width."""
    import os
    import re
    import subprocess
    from icp_amd import register
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cloud_f, cloud_m = engine.synth_cloud_vga(moved=False), engine.synth_cloud_vga(moved=True)
    Fs, Ms = PR.build(oracle.get_lms(cloud_f), 128, 3, PR.MEAN, 24.0), PR.build(oracle.get_lms(cloud_m), 128, 3, PR.MEAN, 24.0)
    want = PR.oracle_chain(oracle, Fs, Ms, (256, 64, 64), 40, a=2e2, c=1e-6, threads=4, power_fast=True, fused=True)
    T, k, ms, moved = register.register_clouds(cloud_f, cloud_m, pyramid=(3, 24.0))
    assert k == [r["k"] for r in want]
    _same_bits(T, want[0]["T"], "register_clouds T")
    assert np.array_equal(moved.view(np.uint32), oracle.transform_q(cloud_m, want[0]["T"]).view(np.uint32))
    T2, k2, _, _ = register.register_clouds(cloud_f, cloud_m, pyramid=(2, 0.0), point_to_plane=0.1, reject_boundary=True, trim=0.9)
    assert len(k2) == 2 and np.all(np.isfinite(T2))                  # (a grid width that is not the level's own is ICP_ESTATE at buildRBC)
    pf, pm = tmp_path / "a.bin", tmp_path / "b.bin"
    cloud_f.astype("<f4").tofile(pf)
    cloud_m.astype("<f4").tofile(pm)
    out = subprocess.run([os.path.join(root, "examples", "registration"), str(pf), str(pm), "--pyramid", "3:24"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    num = r"([-+0-9.eE]+|nan|inf)"
    m = re.search(r"q = \(%s, %s, %s, %s\)\s+t = \(%s, %s, %s\)\s+s = %s\s+k = (\d+) (\d+) (\d+)" % ((num,) * 8), out.stdout)
    assert m, out.stdout
    _same_bits(np.array([float(x) for x in m.groups()[:8]], F32), want[0]["T"], "examples/registration T")
    assert [int(x) for x in m.groups()[8:]] == [r["k"] for r in want]
