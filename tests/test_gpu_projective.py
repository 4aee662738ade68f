"""Projective data association (icp_set_projective): every transformed moving point is projected through the fixed frame's pinhole model
onto F read as a grid and paired with the closest valid point of the (2 r + 1)^2 window around its cell; a point that lands outside the
grid or on an empty window is a miss, which is exactly a rejected pair.  The kernel stands where the RBC search stands; every pass and
every tail behind it is the existing one.

The rule is restated by tests/projective_ref.py (the oracle's transform and metric, the pixel in float64); the step's pieces come from
the oracle's piecewise entries fed the rule's pairs (icp_checks.expected_pieces); the other rules and the plane metrics from their
existing numpy restatements fed the engine's own outputs.  Everything is compared bit for bit unless said otherwise.
tests/test_projective_cpu.py proves what these tests rely on without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks                                               # noqa: E402
import projective_ref as ref                                    # noqa: E402
import robust_ref                                               # noqa: E402
from icp_checks import (A, C_, COLORED, IDENTITY, MODES, P2PL, POWER, REGULAR, WEIGHTED, assert_bits, assert_bits_nan,  # noqa: E402
                        assert_words, one_step, step_batch, _t0)

pytestmark = pytest.mark.gpu

F32 = np.float32
EINVAL, ESTATE = 1, 4


make_handle, check_outputs, check_step = icp_checks.projective_handle, icp_checks.check_projective_outputs, icp_checks.check_projective_step


# ---- 1. arguments

def test_arguments_and_getter(engine):
    g = engine.ICP(0)
    L = engine.lib()
    nan, inf = float("nan"), float("inf")
    assert g.projective() is None
    bad = [(2, 16, 1.0, 1.0, 0.0, 0.0, 0), (-1, 16, 1.0, 1.0, 0.0, 0.0, 0), (1, 0, 1.0, 1.0, 0.0, 0.0, 0), (1, 16, 0.0, 1.0, 0.0, 0.0, 0),
           (1, 16, -1.0, 1.0, 0.0, 0.0, 0), (1, 16, nan, 1.0, 0.0, 0.0, 0), (1, 16, inf, 1.0, 0.0, 0.0, 0), (1, 16, 1.0, 0.0, 0.0, 0.0, 0),
           (1, 16, 1.0, nan, 0.0, 0.0, 0), (1, 16, 1.0, inf, 0.0, 0.0, 0), (1, 16, 1.0, 1.0, nan, 0.0, 0), (1, 16, 1.0, 1.0, inf, 0.0, 0),
           (1, 16, 1.0, 1.0, 0.0, nan, 0), (1, 16, 1.0, 1.0, 0.0, -inf, 0), (1, 16, 1.0, 1.0, 0.0, 0.0, 9)]
    for args in bad:
        assert L.icp_set_projective(g._h, *args) == EINVAL, args
    assert g.projective() is None
    intr = engine.grid_intrinsics(16)
    g.set_projective(16, *intr, radius=8)
    want = (16,) + tuple(float(F32(x)) for x in intr) + (8,)
    assert g.projective() == want
    g.init(256, 16, A, C_)                              # the setting survives icp_init
    assert g.projective() == want
    assert np.all(g.read(engine.Memory.PROJECTIVE) == 0)    # (no iteration yet)
    g.set_projective(16, *intr)
    assert g.projective() == want[:5] + (0,)
    g.set_projective(None)
    assert g.projective() is None
    v = [engine.C.c_int32(7), engine.C.c_uint32(7)] + [engine.C.c_float(7.0) for _ in range(4)] + [engine.C.c_uint32(7)]
    assert L.icp_get_projective(g._h, *[engine.C.byref(x) for x in v]) == 0 and [x.value for x in v] == [0, 0, 0.0, 0.0, 0.0, 0.0, 0]
    g.close()


# ---- 2. one step at (128, 256), every mode, clean and with invalid points, r = 0 and 1

@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("zero_fraction", [0.0, 0.1])
@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, fused, weighted, rot, power_fast, zero_fraction, r):
    side, nr = 128, 256
    F, M, T = ref.scene(side, zero_fraction)
    res = ref.reweighted(ref.at(side, zero_fraction, r), weighted)
    g = make_handle(engine, side * side, nr, fused, weighted, rot, power_fast, side, engine.grid_intrinsics(side), r)
    one_step(engine, g, F, M, T)
    got = check_step(engine, oracle, g, res, F, M, T, side, fused, weighted, rot, power_fast)
    assert tuple(got.tolist()) == ref.EXACT[side, zero_fraction, r]
    g.close()


# ---- 3. smallest shapes: windows clipped at all four edges, lanes past m, a window that covers the whole grid

@pytest.mark.parametrize("r", [0, 1, 2, 8])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", ref.SMALL)
def test_small_shapes(engine, oracle, side, nr, fused, r):
    F, M, T = ref.scene(side, 0.0)
    res = ref.at(side, 0.0, r)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), r)
    one_step(engine, g, F, M, T)
    got = check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused)
    assert tuple(got.tolist()) == ref.EXACT[side, 0.0, 0]                                 # (a clean fixed set: the counts of r = 0)
    if side == 6 and r == 8:                             # the window is the grid: the brute-force nearest neighbour
        Q = oracle.transform_q(M, T)
        Q[:, 4:7] = M[:, 4:7]
        brute = oracle.nn_brute(Q, F, A)
        gn = g.read(engine.Memory.NN_ID)
        assert np.array_equal(gn["id"][res.inside], brute["id"][res.inside])
        assert_bits(gn["dist"][res.inside], brute["dist"][res.inside], "distances")
    # F against itself from the identity: every point lands on its own cell, so the windows are clipped at all four edges and corners
    own = ref.at_self(side, r)
    x, y = own.pu[own.inside], own.pv[own.inside]
    assert own.inside.all() and {x.min(), y.min()} == {0.0} and {x.max(), y.max()} == {side - 1.0}
    one_step(engine, g, F, F, IDENTITY)
    got = check_step(engine, oracle, g, own, F, F, IDENTITY, side, fused, WEIGHTED, POWER, fused)
    assert got.tolist() == [side * side, side * side, 0, 0] and np.array_equal(own.nn_id["id"], np.arange(side * side))
    g.close()


# ---- 4. a rectangular reading

@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("fused", [True, False])
def test_a_rectangular_grid(engine, oracle, fused, r):
    """m = 256 read 32 wide and 8 high (icp_init's own reading of the set is 16 x 16: the pieces' tiles follow that one)."""
    F, M, T = ref.rect_scene()
    res = ref.project(oracle, F, M, T, ref.RECT_GW, ref.RECT_INTRINSICS, r, True)
    g = make_handle(engine, 256, 16, fused, WEIGHTED, POWER, fused, ref.RECT_GW, ref.RECT_INTRINSICS, r)
    one_step(engine, g, F, M, T)
    got = check_step(engine, oracle, g, res, F, M, T, 16, fused, WEIGHTED, POWER, fused)
    assert 2 * got[1] >= got[0] and 100 * got[2] >= got[0]
    g.close()


# ---- 5. messy inputs

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", icp_checks.MESSY_SHAPES)
def test_messy_inputs_and_a_scale(engine, oracle, side, nr, fused):
    """NaN / +-inf / origin points in both frames, and a transform with s = 1.25."""
    F, M = ref.messy_pair(side)
    T = ref.scaled_T()
    intr = engine.grid_intrinsics(side)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, intr, 0)
    for r in (0, 1):
        res = ref.project(oracle, F, M, T, side, intr, r, True)
        g.set_projective(side, *intr, radius=r)          # (a new radius while the rule stays on: the device word)
        one_step(engine, g, F, M, T)
        got = check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused)
        assert got[1] > 0 and got[2] > 0 and (r or got[3] > 0), got
    g.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", icp_checks.MESSY_SHAPES)
def test_every_query_outside_is_the_identity_step(engine, oracle, side, nr, fused):
    """A half turn about y puts every transformed point behind the camera: nothing is paired, T stays, a checked run is done at k = 1."""
    F, M = ref.messy_pair(side)
    T = ref.turned_T()
    Mem = engine.Memory
    intr = engine.grid_intrinsics(side)
    res = ref.project(oracle, F, M, T, side, intr, 1, True)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, intr, 1)
    one_step(engine, g, F, M, T)
    got = check_outputs(engine, g, res)
    assert got[1] == 0 and got[2] == got[0] > 0
    assert np.all(g.read(Mem.W).view(np.uint32) == 0) and g.read(Mem.SUM_W)[0] == 0.0
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert_bits(g.read(Mem.T), T, "T")
    g.reset_transform(); g.buildRBC()
    g.write(Mem.T, T, block=True)
    k = g.run()
    st = g.state()
    assert k == 1 and st.k == 1 and st.converged == 1, (k, st.k, st.converged)
    assert_bits(g.read(Mem.T), T, "T behind the run")
    g.close()


# ---- 6. a batch of three different pairs

@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch3(engine, oracle, fused, r):
    side, nr = ref.BATCH_SIDE, 4
    pairs = ref.batch_pairs()
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), r, batch=3)
    step_batch(engine, g, pairs, T)
    seen = set()
    for b, ((F, M), (seed, zf)) in enumerate(zip(pairs, ref.BATCH)):
        got = check_step(engine, oracle, g, ref.at(side, zf, r, seed), F, M, T, side, fused, WEIGHTED, POWER, fused, b=b)
        seen.add(tuple(got.tolist()))
    assert len(seen) == 3, seen
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_a_converged_registration_keeps_its_outputs_and_words(engine, oracle, fused):
    """Registration 0 is F against itself from the identity: every valid point lands on itself at distance 0, ICP::check stops it at
    k = 1; the other two go on.  Its outputs and words are still those of its only iteration when the run returns."""
    side, nr = ref.BATCH_SIDE, 4
    Mem = engine.Memory
    pairs = ref.batch_pairs()
    pairs[0] = (pairs[0][0], pairs[0][0])
    intr = engine.grid_intrinsics(side)
    res0 = ref.project(oracle, pairs[0][0], pairs[0][0], IDENTITY, side, intr, 1, True)
    assert res0.counts.tolist() == [900, 900, 0, 0] and not res0.nn_id["dist"].any()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, intr, 1, batch=3)
    for b, (F, M) in enumerate(pairs):
        g.write(Mem.F, F, batch_index=b); g.write(Mem.M, M, batch_index=b)
    g.buildRBC()
    g.run()
    ks = [g.state(b).k for b in range(3)]
    assert ks[0] == 1 and g.state(0).converged == 1 and min(ks[1:]) > 2, ks
    check_outputs(engine, g, res0, 0)
    assert np.array_equal(g.read(Mem.W, batch_index=0) != 0, ~res0.miss)
    for b in (1, 2):
        w = g.read(Mem.PROJECTIVE, batch_index=b)
        assert w[0] == w[1] + w[2] + w[3] and w[1] > 0 and tuple(w) != (900, 900, 0, 0)
    g.close()


# ---- 7. the plane metrics

def check_plane_last(engine, g, restate, T0, R0, k0):
    """icp_checks.check_last with the ids of the misses clipped in a copy: the restatement indexes the normals with them, and a miss's
    weight is +0."""
    Mem = engine.Memory
    PF, PM, ids = g.read(Mem.NN), g.read(Mem.QT), g.read(Mem.NN_ID)["id"].copy()
    miss = ids == ref.NONE
    assert not PF[miss].any()
    ids[miss] = 0
    system, T, R, Tk, Rk = restate(lambda name: g.read(getattr(Mem, name)), PF, PM, ids, T0, R0)
    assert_bits(g.read(Mem.PLANE_SYSTEM), system, "PLANE_SYSTEM")
    assert_bits(g.read(Mem.T), T, "T")
    assert_bits(g.read(Mem.R).ravel(), R, "R")
    assert_bits(g.read(Mem.TK), Tk, "TK")
    assert_bits(g.read(Mem.RK).ravel(), Rk, "RK")
    assert g.state().k == k0 + 1
    return system


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("metric", [P2PL, COLORED])
@pytest.mark.parametrize("side,nr", [(30, 4), (128, 256)])
def test_with_a_plane_metric(engine, oracle, side, nr, metric, fused):
    zf = 0.1
    seed = ref.BATCH[1][0] if side == 30 else 0x1C9D5EED
    F, M, T = ref.scene(side, zf, seed)
    res = ref.at(side, zf, 0, seed)
    g = icp_checks.make_plane(engine, side, nr, fused=fused, power_fast=fused, metric=metric)
    off = g.launches_per_iteration()
    g.set_projective(side, *engine.grid_intrinsics(side), radius=0)
    assert g.run_form() == 0 and g.launches_per_iteration() == off == 1 + 2
    icp_checks.load(engine, g, F, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    T0, R0, k0 = icp_checks.before(engine, g)
    g.step()
    got = check_outputs(engine, g, res)
    assert got[3] > 0
    assert_bits(g.read(engine.Memory.NN)[:, 3], res.NN[:, 3], "weights")
    restate = icp_checks.restate_p2pl(0.05) if metric == P2PL else icp_checks.restate_colored(0.05, 1e3)
    system = check_plane_last(engine, g, restate, T0, R0, k0)
    assert system[27] == 1.0
    g.close()


# ---- 8. composition with the rules behind the search

RULES = ["rejection", "boundary", "unique", "trimming", "cauchy"]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", [(30, 4), (128, 256)])
def test_composed_with(engine, oracle, side, nr, fused, rule):
    """Each rule behind the search with its existing numpy restatement, fed the engine's own outputs (the ids of the misses clipped in a
    copy); the pairs themselves are the restatement's, whatever the rule behind them."""
    Mem = engine.Memory
    zf = 0.1
    seed = ref.BATCH[1][0] if side == 30 else 0x1C9D5EED
    F, M, T = ref.scene(side, zf, seed)
    res = ref.at(side, zf, 0, seed)
    hits = int(res.counts[1])
    geo = icp_checks.geo_of(res.NN, res.QT)[~res.miss]
    max_dist = float(F32(np.sqrt(np.quantile(geo.astype(np.float64), 0.88))))
    options = {"rejection": dict(rejection=(True, max_dist)), "boundary": dict(boundary=side), "unique": dict(unique=True),
               "trimming": dict(trimming=0.75), "cauchy": dict(robust_loss=(robust_ref.CAUCHY, 12.0))}[rule]
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 0, **options)
    # (the rules bring the apply pass with them: the projection adds no launch; the boundary rule and one-to-one add their own)
    tail = 2 if fused else 4
    assert g.launches_per_iteration() == tail + {"rejection": 1, "boundary": 2, "unique": 3, "trimming": 2, "cauchy": 1}[rule]
    one_step(engine, g, F, M, T)
    check_outputs(engine, g, res)
    gn = g.read(Mem.NN_ID)
    miss = gn["id"] == ref.NONE
    nn = ref.clipped(gn, miss)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    weights = None
    if rule == "rejection":
        zero = icp_checks.rejected_set(M, PF, PM, True, max_dist)
        assert zero[miss].all() and 0.05 * hits < np.count_nonzero(zero & ~miss) < 0.2 * hits
    elif rule == "boundary":
        zero, counts, _, _ = icp_checks.pair_filter_rule_of(engine, g, F, M, None, WEIGHTED, True, side, None, nn_id=nn)
        assert_words(engine, g, "PAIR_FILTER", counts)
        assert counts[0] == hits and 0 < counts[1] < counts[0]
    elif rule == "unique":
        win, zero, counts, _ = icp_checks.unique_rule_of(engine, g, M, WEIGHTED, True, nn_id=nn)
        assert_words(engine, g, "UNIQUE", counts)
        assert counts[0] == hits and 0 < counts[1]
    elif rule == "trimming":
        acc, words = icp_checks.trim_rule(PF, PM, icp_checks.weights_before_trim(nn, M, PF, PM, WEIGHTED, True), 0.75)
        assert_words(engine, g, "TRIM", words)
        assert words[1] == hits and 0 < words[3] < hits
        zero = ~acc
    else:
        weights = icp_checks._robust_weights(engine, g, nn, M, WEIGHTED, True, None, 1.0, robust_ref.CAUCHY, 12.0, 0)
        zero = weights == 0
        assert np.array_equal(zero, miss)
    W, sw, means, S, Tk = icp_checks.expected_pieces(oracle, F, M, T, nn, side, fused, WEIGHTED, POWER, fused, zero | miss, weights)
    gW = g.read(Mem.W)
    assert_bits(gW, W, "weights")
    assert np.count_nonzero(np.ascontiguousarray(gW[zero | miss]).view(np.uint32)) == 0
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits_nan(g.read(Mem.TK), Tk, "Tk")
    g.close()


def test_last_iteration_pairs_are_the_hits(engine, oracle):
    side, nr = 128, 256
    F, M, T = ref.scene(side, 0.1)
    res = ref.at(side, 0.1, 0)
    g = make_handle(engine, side * side, nr, True, WEIGHTED, POWER, True, side, engine.grid_intrinsics(side), 0)
    one_step(engine, g, F, M, T)
    pairs = g.correspondences(engine.Pairs.LAST_ITERATION)
    assert len(pairs) == res.counts[1] and np.array_equal(pairs["moving"], np.flatnonzero(~res.miss))
    assert np.array_equal(pairs["fixed"], res.nn_id["id"][~res.miss])
    g.close()


# ---- 9. runs

def _snapshot(engine, g):
    Mem = engine.Memory
    return [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.PROJECTIVE).copy(), g.read(Mem.NN_ID).copy(), g.read(Mem.NN).copy(),
            g.read(Mem.QT).copy(), np.array([g.state().k])]


def _same(a, b):
    for x, y, what in zip(a, b, ("T", "W", "PROJECTIVE", "NN_ID", "NN", "QT", "k")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what


@pytest.mark.parametrize("every_iteration", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_fixed_run_equals_steps(engine, fused, every_iteration):
    """icp_run_fixed (10) against ten icp_step: T, k and the per-query outputs, under the lazy and the eager output mode."""
    side, nr = 128, 256
    F, M, _ = ref.scene(side, 0.1)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 1)
    g.set_output_mode(every_iteration)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run_fixed(10)
    fixed = _snapshot(engine, g)
    assert fixed[6][0] == 10 and 0 < fixed[2][1] < fixed[2][0]
    g.reset_transform(); g.buildRBC()
    for _ in range(10):
        g.step()
    _same(fixed, _snapshot(engine, g))
    g.close()


# ---- 10. bookkeeping

def test_form_and_launch_count(engine):
    side = 128
    intr = engine.grid_intrinsics(side)
    g = engine.ICP(0)
    g.init(side * side, 256, A, C_)
    g.setReduceMode(engine.ReduceMode.FUSED)
    form0 = g.run_form()
    g.set_projective(side, *intr, radius=1)
    assert g.run_form() == 0
    assert g.launches_per_iteration() == 2 + 1           # (the projection in the search's place, the fused finalize, and the apply pass)
    g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
    assert g.launches_per_iteration() == 4 + 1
    g.set_unique(True)                                   # (the apply pass runs anyway: the rule adds nothing)
    on = g.launches_per_iteration()
    g.set_projective(None)
    assert on == g.launches_per_iteration() == 4 + 3
    g.set_unique(False)
    g.setReduceMode(engine.ReduceMode.FUSED)
    assert g.run_form() == form0
    g.set_normals(1, side)
    g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
    off = g.launches_per_iteration()
    g.set_projective(side, *intr)
    assert g.launches_per_iteration() == off == 3 and g.run_form() == 0
    g.close()


def test_evaluate_ignores_the_rule(engine):
    side, nr = 128, 256
    F, M, T = ref.scene(side, 0.1)
    quality = []
    for on in (False, True):
        g = icp_checks.make_handle(engine, side * side, nr, True, WEIGHTED, POWER, True)
        if on:
            g.set_projective(side, *engine.grid_intrinsics(side), radius=1)
        one_step(engine, g, F, M, T)
        g.write(engine.Memory.T, T, block=True)          # (the step moved T by the pairs it used: the same transform for both)
        quality.append(bytes(g.evaluate(50.0)[0]))
        if on:
            assert len(g.correspondences(engine.Pairs.EVALUATED, 50.0)) > 0
        g.close()
    assert quality[0] == quality[1], "icp_evaluate gives the same bytes with the rule on and off"


# ---- 11. state errors

def test_state_errors(engine):
    side = 16
    intr = engine.grid_intrinsics(side)
    F, M, T = ref.scene(side, 0.0)
    g = engine.ICP(0)
    g.set_projective(7, *intr)                           # (no size yet: accepted; icp_build_rbc finds that 7 does not divide 256)
    g.init(side * side, 16, A, C_)
    icp_checks.load(engine, g, F, M)
    with pytest.raises(engine.ICPError) as e:
        g.buildRBC()
    assert e.value.code == ESTATE
    with pytest.raises(engine.ICPError) as e:            # (an initialised handle: the setter refuses)
        g.set_projective(24, *intr)
    assert e.value.code == ESTATE and g.projective()[0] == 7
    g.set_projective(side, *intr)
    g.buildRBC()
    g.step()
    g.set_reciprocal(True, 5.0)
    for call in (g.step, g.run, lambda: g.run_fixed(2)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == ESTATE
    g.set_reciprocal(False)
    g.step()
    g.close()
    g = engine.ICP(0)
    g.init(128 * 128, 256, A, C_)
    g.set_projective(128, *engine.landmark_intrinsics(), radius=1)
    for call in (g.track_next, g.track_submit):
        with pytest.raises(engine.ICPError) as e:
            call(engine.synth_cloud_vga())
        assert e.value.code == ESTATE
    g.close()


# ---- 12. switching the rule off in the middle of a registration

@pytest.mark.parametrize("fused", [True, False])
def test_off_again_is_the_search(engine, oracle, fused):
    """Two projective steps, the rule off, T written, a step: the RBC search's ids, distances and nearest representatives are the
    oracle's, whatever the projective iterations left in ICP_MEM_RID (they leave it alone; pruning is exact)."""
    side, nr = 128, 256
    F, M, T, _, want = icp_checks.scene(engine, oracle, side, nr, "clean")
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 1)
    one_step(engine, g, F, M, T)
    rid = g.read(engine.Memory.RID).copy()
    g.step()
    assert np.array_equal(g.read(engine.Memory.RID), rid), "a projective iteration leaves RID alone"
    g.set_projective(None)
    assert np.all(g.read(engine.Memory.PROJECTIVE) == 0)
    g.write(engine.Memory.T, T, block=True)
    g.step()
    icp_checks.check_search(engine, g, want)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, np.zeros(side * side, bool), want)
    g.close()


# ---- 13. convergence

def test_converges_like_the_search(engine):
    """synth_pair_scene (128) one degree apart, point-to-point, checked runs: the projective run with r = 2 ends within 1.5 x the RBC
    run's rotation and translation error.  (A float64 simulation gave 0.137 degrees / 9.3 mm against the documented 0.125-degree class
    of the RBC run; the margin also covers the queries that leave the grid at its rim.)  Measured on an MI355X: the RBC run ends
    0.1243 degrees / 8.80 mm from the ground truth after 27 iterations, the projective run 0.1375 degrees / 9.31 mm after 30."""
    F, M, T_true = engine.synth_pair_scene(128, rot_deg=1.0)
    err = []
    for on in (False, True):
        g = engine.ICP(0)
        g.init(128 * 128, 256, A, C_)
        if on:
            g.set_projective(128, *engine.grid_intrinsics(128), radius=2)
        icp_checks.load(engine, g, F, M)
        g.buildRBC()
        k = g.run()
        err.append(icp_checks._errors(g.read(engine.Memory.T), T_true))
        print("projective r = 2" if on else "RBC", "k", k, "rotation error %.4f deg, translation error %.3f mm" % err[-1])
        g.close()
    assert err[1][0] <= 1.5 * err[0][0] and err[1][1] <= 1.5 * err[0][1], err


# ---- 14. icp_batch_*, and a new radius under a captured graph

def test_icp_batch_with_two_registrations_on_one_slot(engine):
    side, nr = ref.BATCH_SIDE, 4
    intr = engine.grid_intrinsics(side)
    pairs = ref.batch_pairs()[:2]
    bt = engine.ICPBatch([0])
    bt.init(2, side * side, nr, A, C_)
    assert bt.projective() is None
    bt.set_projective(side, *intr, radius=1)
    assert bt.projective() == (side,) + tuple(float(F32(x)) for x in intr) + (1,)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(side * side, nr, A, C_)
        g.set_projective(side, *intr, radius=1)
        icp_checks.load(engine, g, F, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        u = bt.read(i, engine.Memory.PROJECTIVE)
        assert np.array_equal(u, g.read(engine.Memory.PROJECTIVE)) and 0 < u[1] < u[0], i
        g.close()
    bt.set_projective(None)
    assert bt.projective() is None
    bt.close()


def test_a_new_radius_reaches_a_captured_graph(engine, oracle):
    """run_fixed's graph is captured with r = 0; a new radius and new intrinsics while the rule stays on are device words it reads."""
    side, nr = 30, 4
    seed, zf = ref.BATCH[1]
    F, M, T = ref.scene(side, zf, seed)
    intr = engine.grid_intrinsics(side)
    g = make_handle(engine, side * side, nr, True, WEIGHTED, POWER, True, side, intr, 0)
    icp_checks.load(engine, g, F, M)
    g.buildRBC()
    for r in (0, 1):
        g.set_projective(side, *intr, radius=r)
        g.reset_transform()
        g.write(engine.Memory.T, T, block=True)
        g.step()
        check_outputs(engine, g, ref.at(side, zf, r, seed))
    for r in (0, 1):
        g.set_projective(side, *intr, radius=r)
        g.write(engine.Memory.T, T, block=True)
        g.run_fixed(3)
        assert g.state().k >= 3
        w = g.read(engine.Memory.PROJECTIVE)
        assert w[0] == w[1] + w[2] + w[3] and (w[3] > 0) == (r == 0), (r, w)
    g.close()
