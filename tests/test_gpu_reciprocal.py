"""Reciprocal correspondences (icp_set_reciprocal): a candidate pair (m_i, f_j) keeps its weight only if f_j's back search into the
moving set finds m_i again (exact), or a moving point within max_gap of it (near); every other candidate gets the weight +0 and is then
a rejected pair.  The forward search is not touched.

The back search is restated by the CPU oracle with F and M swapped and the inverse transform of tests/reciprocal_ref.py; the rule by
numpy from the engine's own NN_ID / NN / QT outputs and the weights before the rule; the reference values come from the oracle's
piecewise entries with the rejected rows zeroed (icp_checks.expected_pieces).  ICP_MEM_RECIPROCAL holds (n, exact, near, accepted) of
the last iteration, ICP_MEM_REVERSE_ID the back search's (dist, id) per fixed point.  Everything is compared bit for bit.

Sections 13 to 15 take every expectation from the oracle's pairs alone (icp_checks.composed_rule with the rule as a stage): the rule in
every search layout, a converged registration beside two running ones, max_gap exactly at a pair's gap, and non-finite rows in the back
search's database.  tests/test_reciprocal_cpu.py proves what they rely on without a device; the rule composed with every other pass is
tests/test_gpu_route_numerics.py's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                 # noqa: E402
import quality_ref                                              # noqa: E402
import reciprocal_ref as ref                                    # noqa: E402
import icp_checks                                               # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, POWER, EIGEN, REGULAR, WEIGHTED, assert_bits, assert_words, check_pieces,  # noqa: E402
                        holes_pair as _holes, one_step, oracle_search, only_invalid, set_modes, step_batch, weights_before_trim, _t0)
from reciprocal_ref import EXACT, NEAR_20, rotation_T           # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
# What the header documents for icp_launches_per_iteration: the inverse transform, the back search, the test, and on point-to-point
# the apply pass.
ADDED_P2P, ADDED_PLANE = 4, 3
ESTATE = 4


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, max_gap=0.0, batch=1, on=True, **options):
    """icp_checks.make_handle, then the rule on the handle."""
    g = icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid), **options)
    if on:
        g.set_reciprocal(True, max_gap)
    return g


@pytest.fixture(scope="module")
def scenes_A(engine, oracle):
    """name -> (F, M, T, invalid flag, the oracle's (nn_id, rid) at T, the oracle's back search (nn_id, rid) at T)."""
    out = {}
    for name, s in icp_checks.scenes_A(engine, oracle).items():
        back, ok = ref.back_search(oracle, s[0], s[1], s[2], 256)
        assert ok
        out[name] = s + (back,)
    return out


def numpy_rule(engine, g, M, weighted, invalid, back, max_gap, ok=True, b=0, W0=None, max_dist=None):
    """(exact, near, rows that weigh nothing, counts, weights before the rule) from the engine's outputs of registration b and the
    restated back search."""
    Mem = engine.Memory
    nn_id = g.read(Mem.NN_ID, batch_index=b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    if W0 is None:
        W0 = weights_before_trim(nn_id, M, PF, PM, weighted, invalid, max_dist)
    exact, near, zero, counts = ref.reciprocal_rule(nn_id["id"], back[0]["id"], PM, W0, max_gap, ok)
    return exact, near, zero, counts, W0


def check_back_search(engine, g, back, b=0):
    got = g.read(engine.Memory.REVERSE_ID, batch_index=b)
    assert np.array_equal(got["id"], back[0]["id"]), "back search ids: %d differ" % np.count_nonzero(got["id"] != back[0]["id"])
    assert_bits(got["dist"], back[0]["dist"], "back search distances")


def check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, back, max_gap, want=None, b=0, max_dist=None):
    """REVERSE_ID against the restated back search, ICP_MEM_RECIPROCAL, `W != 0 equals the rule`, and the pieces.  Returns the counts."""
    check_back_search(engine, g, back, b)
    exact, near, zero, counts, W0 = numpy_rule(engine, g, M, weighted, invalid, back, max_gap, b=b, max_dist=max_dist)
    got = assert_words(engine, g, "RECIPROCAL", counts, b)
    assert got[3] == got[1] + got[2], got
    check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, zero, want, b)
    gW = g.read(engine.Memory.W, batch_index=b)
    assert np.array_equal(gW != 0, ~zero), "W != 0 equals the rule"
    assert_bits(gW[~zero], W0[~zero], "an accepted pair keeps its weight")
    assert_bits(g.read(engine.Memory.NN, batch_index=b)[:, 3], gW, "the NN output's weights")
    return counts


# ---- 1. arguments

def test_arguments_and_getter(engine):
    g = engine.ICP(0)
    L = engine.lib()
    assert g.reciprocal() is None
    for on, gap in ((2, 0.0), (-1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf")), (0, -1.0)):
        assert L.icp_set_reciprocal(g._h, on, gap) == 1, (on, gap)                        # ICP_EINVAL
    assert g.reciprocal() is None
    g.set_reciprocal(True, 12.5)
    assert g.reciprocal() == 12.5
    g.init(256, 16, A, C_)                              # the setting survives icp_init
    assert g.reciprocal() == 12.5
    assert np.all(g.read(engine.Memory.RECIPROCAL) == 0)    # (no iteration yet)
    g.set_reciprocal(True)
    assert g.reciprocal() == 0.0
    g.set_reciprocal(False, 3.0)
    assert g.reciprocal() is None
    on, gap = engine.C.c_int32(7), engine.C.c_float(7.0)
    assert L.icp_get_reciprocal(g._h, engine.C.byref(on), engine.C.byref(gap)) == 0 and (on.value, gap.value) == (0, 0.0)
    g.close()


# ---- 2. one step at the latency layout, every mode, clean and with holes, max_gap 0 and 20

@pytest.mark.parametrize("max_gap", [0.0, 20.0])
@pytest.mark.parametrize("scene", ["clean", "holes"])
@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, scenes_A, fused, weighted, rot, power_fast, scene, max_gap):
    F, M, T, invalid, want, back = scenes_A[scene]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, rot, power_fast, invalid, max_gap)
    one_step(engine, g, F, M, T)
    counts = check_step(engine, oracle, g, F, M, T, 128, fused, weighted, rot, power_fast, invalid, back, max_gap, want)
    assert 0 < counts[3] < counts[0]
    if scene == "clean":
        near = NEAR_20[128, 256] if max_gap else 0
        assert counts.tolist() == [16384, EXACT[128, 256], near, EXACT[128, 256] + near], counts
        if max_gap:
            assert counts.tolist() == [16384, 1367, 2111, 3478]
    g.close()


def test_search_is_untouched(engine, scenes_A):
    """Forward ids, distances, RID, the transformed moving points and the matched fixed points at the same T: the bits of a handle with
    the rule off."""
    F, M, T, invalid, _, _ = scenes_A["holes"]
    out = []
    for on in (False, True):
        g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid, 20.0, on=on)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy(),
                    g.read(engine.Memory.NN)[:, :3].copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")
    assert_bits(out[0][3], out[1][3], "matched fixed points")


# ---- 3. smallest shapes: sides that are no multiple of 8, blocks with lanes past m

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", [(6, 4), (14, 4), (16, 16), (30, 4)])
def test_small_shapes(engine, oracle, side, nr, fused):
    F, M = engine.synth_pair(side)
    T = _t0()
    want = oracle_search(oracle, F, M, T, nr)
    back, ok = ref.back_search(oracle, F, M, T, nr)
    assert ok
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, 0.0)
    one_step(engine, g, F, M, T)
    counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, back, 0.0, want)
    assert counts.tolist() == [side * side, EXACT[side, nr], 0, EXACT[side, nr]], counts
    # max_gap = 20 is below these shapes' smallest non-exact gap: the lower quartile of the restatement's non-exact gaps instead
    gaps = ref.gaps(want[0]["id"], back[0]["id"], oracle.transform_q(M, T), np.ones(side * side, F32))
    max_gap = float(F32(np.quantile(gaps, 0.25)))
    g.set_reciprocal(True, max_gap)                     # (a new max_gap while the rule stays on: the device word)
    g.write(engine.Memory.T, T, block=True)
    g.step()
    counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, back, max_gap, want)
    assert 0 < counts[2] and counts[3] < counts[0], counts
    g.close()


# ---- 4. dense layouts: a batch, and 65536 pairs

@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch3(engine, oracle, fused):
    from icp_amd import workloads as W
    side, nr, B = 128, 256, 3
    pairs = [W.pair(engine, 0), _holes(engine, side, W.BASE_SEED + 3, "blobs30"), _holes(engine, side, W.BASE_SEED + 6, "scattered10")]
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, 20.0, batch=B)
    assert g.search_layout()[0] == 1, "the batch runs the dense search"
    step_batch(engine, g, pairs, T)
    seen = set()
    for b, (F, M) in enumerate(pairs):
        back, ok = ref.back_search(oracle, F, M, T, nr)
        counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, back, 20.0,
                            oracle_search(oracle, F, M, T, nr), b=b)
        assert ok and 0 < counts[2] and counts[3] < counts[0]
        seen.add(tuple(counts.tolist()))
    assert len(seen) == B, seen
    g.close()


@pytest.mark.parametrize("fused,weighted,rot", [(True, WEIGHTED, POWER), (False, REGULAR, EIGEN)])
def test_one_step_65536(engine, oracle, fused, weighted, rot):
    """m = 65536, |R| = 1024: the dense layout, many blocks per registration; the pinned counts of the clean pair."""
    side, nr = 256, 1024
    F, M = engine.synth_pair(side)
    T = _t0()
    back, ok = ref.back_search(oracle, F, M, T, nr)
    g = make_handle(engine, F.shape[0], nr, fused, weighted, rot, fused, False, 20.0)
    assert g.search_layout()[0] == 1
    one_step(engine, g, F, M, T)
    counts = check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, fused, False, back, 20.0, oracle_search(oracle, F, M, T, nr))
    assert ok and counts.tolist() == [65536, EXACT[side, nr], NEAR_20[side, nr], EXACT[side, nr] + NEAR_20[side, nr]] == [65536, 2751, 12812, 15563]
    # a second iteration: the back search seeds its pruning from its own first answer
    T1 = g.read(engine.Memory.T).copy()
    g.step()
    back1, ok1 = ref.back_search(oracle, F, M, T1, nr)
    assert ok1
    check_back_search(engine, g, back1)
    _, _, _, c1, _ = numpy_rule(engine, g, M, weighted, False, back1, 20.0)
    assert_words(engine, g, "RECIPROCAL", c1)
    g.close()


# ---- 5. T with s != 1

@pytest.mark.parametrize("s,axis,t", [(1.02, (0.2, -0.5, 0.8), (25.0, -40.0, 12.5)), (0.97, (1.0, 0.3, -0.4), (-7.0, 3.0, 30.0))])
@pytest.mark.parametrize("fused", [True, False])
def test_a_transform_with_a_scale(engine, oracle, fused, s, axis, t):
    """A 10 degree rotation, a non-trivial t and s != 1: the back ids against the restatement, whose counts are taken at test time."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    T = rotation_T(10.0, axis, t, s)
    back, ok = ref.back_search(oracle, F, M, T, nr)
    assert ok
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, 20.0)
    one_step(engine, g, F, M, T)
    counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, back, 20.0, oracle_search(oracle, F, M, T, nr))
    assert 0 < counts[1] and 0 < counts[3] < counts[0], counts
    g.close()


# ---- 6. the guard

@pytest.mark.parametrize("fused", [True, False])
def test_a_transform_without_an_inverse_rejects_everything(engine, fused):
    side, nr = 32, 64
    F, M = engine.synth_pair(side)
    T = _t0().copy()
    T[7] = 0.0
    Mem = engine.Memory
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, 20.0)
    one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    n = np.count_nonzero(nn_id["id"] < side * side)
    assert n == side * side
    assert g.read(Mem.RECIPROCAL).tolist() == [n, 0, 0, 0]
    assert np.all(g.read(Mem.W).view(np.uint32) == 0) and g.read(Mem.SUM_W)[0] == 0.0
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    got = g.read(Mem.T)
    assert np.isfinite(got).all()
    assert_bits(got, T, "T")
    g.close()


# ---- 7. a plane metric

@pytest.mark.parametrize("fused", [True, False])
def test_with_point_to_plane(engine, oracle, scenes_A, fused):
    """ICP_MEM_PLANE_SYSTEM, T, R, TK against tests/p2pl_ref.py's float64 restatement with the rejected weights zeroed."""
    F, M, T0, invalid, _, back = scenes_A["holes"]
    mu, side = 0.05, 128
    Mem = engine.Memory
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, 256, A, C_)
    set_modes(engine, g, fused, fused)
    g.set_normals(1, side)                               # Normals.GRID
    g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, mu)
    g.set_rejection(True, None)
    g.set_reciprocal(True, 20.0)
    assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + ADDED_PLANE
    R0 = one_step(engine, g, F, M, T0)
    check_back_search(engine, g, back)
    exact, near, zero, counts, W0 = numpy_rule(engine, g, M, True, invalid, back, 20.0)
    assert_words(engine, g, "RECIPROCAL", counts)
    assert 0 < counts[2] and counts[3] < counts[0]
    PF = g.read(Mem.NN).copy()
    assert_bits(PF[:, 3], np.where(zero, F32(0), W0).astype(F32), "weights")
    system, T, R, Tk, Rk = p2pl_ref.step(PF, g.read(Mem.QT), g.read(Mem.NN_ID)["id"], g.read(Mem.NORMALS_F), mu, T0, R0)
    assert system[27] == 1.0
    assert_bits(g.read(Mem.PLANE_SYSTEM), system, "PLANE_SYSTEM")
    assert_bits(g.read(Mem.T), T, "T")
    assert_bits(g.read(Mem.R).ravel(), R, "R")
    assert_bits(g.read(Mem.TK), Tk, "TK")
    g.close()


# ---- 8. the order of the passes

@pytest.mark.parametrize("fused", [True, False])
def test_order_of_the_passes(engine, scenes_A, fused):
    """The pair filter, the rule, one-to-one and trimming all on: each pass's candidates are what the pass in front left."""
    F, M, T, invalid, _, _ = scenes_A["holes"]
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], 256, fused, WEIGHTED, POWER, fused, invalid, 20.0, boundary=128, unique=True, trimming=0.75)
    assert g.launches_per_iteration() == (2 if fused else 4) + 1 + 3 + 2 + 2      # (tail, filter, the rule, claim + resolve, select + apply)
    one_step(engine, g, F, M, T)
    pf, rc, un, tr = g.read(Mem.PAIR_FILTER), g.read(Mem.RECIPROCAL), g.read(Mem.UNIQUE), g.read(Mem.TRIM)
    assert pf[3] == rc[0] and 0 < rc[3] < rc[0] < pf[0], (pf, rc)
    assert un[0] == rc[3] and 0 < un[1] <= un[0], (un, rc)
    assert tr[1] == un[1] and 0 < tr[3] < tr[1], (tr, un)
    assert np.count_nonzero(g.read(Mem.W)) == tr[3]
    g.close()


# ---- 9. runs

def _snapshot(engine, g):
    Mem = engine.Memory
    return [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.RECIPROCAL).copy(), g.read(Mem.NN_ID)["id"].copy(),
            g.read(Mem.REVERSE_ID)["id"].copy()]


def _same(a, b):
    for x, y, what in zip(a, b, ("T", "W", "RECIPROCAL", "ids", "back ids")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_run_equals_steps(engine, scenes_A, fused, weighted):
    """run_fixed (5) as a graph against 5 single steps, and a checked run against stepping until ICP::check says stop."""
    F, M, _, invalid, _, _ = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, POWER, fused, invalid, 20.0)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run_fixed(5)
    fixed = _snapshot(engine, g)
    assert 0 < fixed[2][3] < fixed[2][0]
    g.reset_transform(); g.buildRBC()
    for _ in range(5):
        g.step()
    _same(fixed, _snapshot(engine, g))
    g.reset_transform(); g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    run = _snapshot(engine, g)
    conv = g.state().converged
    assert np.count_nonzero(run[1]) == run[2][3], "the weights read behind a checked run show the rule's zeros"
    g.reset_transform(); g.buildRBC()
    # (a single step runs unchecked: ICP::check, restated on the host by p2pl_ref.check_converged, decides when the stepping stops)
    n, stop = 0, False
    while n < 40 and not stop:
        g.step(); n += 1
        stop = p2pl_ref.check_converged(g.read(engine.Memory.TK), 0.001, 0.01)
    assert n == k and stop == bool(conv), (n, k, stop, conv)
    _same(run, _snapshot(engine, g))
    g.close()


def test_off_again_equals_never_on(engine, scenes_A):
    F, M, _, _, _, _ = scenes_A["holes"]
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        g.set_rejection(True, None)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        form0, n0 = g.run_form(), g.launches_per_iteration()
        if toggled:
            g.set_reciprocal(True, 20.0)
            assert g.run_form() == 0
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(engine.Memory.RECIPROCAL)[3] > 0
            g.set_reciprocal(False)
            assert g.reciprocal() is None
            assert np.all(g.read(engine.Memory.RECIPROCAL) == 0)
            assert g.run_form() == form0 and g.launches_per_iteration() == n0
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy(),
                    g.read(engine.Memory.W).view(np.uint32).copy()))
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


# ---- 10. staleness

@pytest.mark.parametrize("route", ["a new M behind the build", "the rule switched on behind the build"])
def test_a_stale_moving_set_is_rebuilt(engine, scenes_A, route):
    F, M0, T, _, _, _ = scenes_A["clean"]
    M1 = scenes_A["holes"][1]
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, True, 20.0, on=route.startswith("a new M"))
    g.write(Mem.F, F); g.write(Mem.M, M0)
    g.buildRBC()
    g.write(Mem.M, M1)
    if not route.startswith("a new M"):
        g.set_reciprocal(True, 20.0)
    g.write(Mem.T, T, block=True)
    g.step()
    h = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, True, 20.0)
    one_step(engine, h, F, M1, T)
    a, b = g.read(Mem.REVERSE_ID), h.read(Mem.REVERSE_ID)
    assert np.array_equal(a["id"], b["id"])
    assert_bits(a["dist"], b["dist"], "back search distances")
    assert np.array_equal(g.read(Mem.RECIPROCAL), h.read(Mem.RECIPROCAL)) and g.read(Mem.RECIPROCAL)[3] > 0
    assert_bits(g.read(Mem.T), h.read(Mem.T), "T")
    # (and the set did change: the back search over M0 answers differently)
    k = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, True, 20.0)
    one_step(engine, k, F, M0, T)
    assert not np.array_equal(k.read(Mem.REVERSE_ID)["id"], b["id"])
    g.close(); h.close(); k.close()


# ---- 11. surroundings

def test_surroundings(engine, scenes_A):
    F, M, T, invalid, _, _ = scenes_A["holes"]
    Mem = engine.Memory
    quality = []
    for on in (False, True):
        g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid, 20.0, on=on)
        one_step(engine, g, F, M, T)
        if on:
            acc = int(g.read(Mem.RECIPROCAL)[3])
            pairs = g.correspondences(engine.Pairs.LAST_ITERATION)
            assert len(pairs) == acc > 0 and np.array_equal(pairs["moving"], np.flatnonzero(g.read(Mem.W) != 0))
            evaluated = g.correspondences(engine.Pairs.EVALUATED, 50.0)
            assert len(evaluated) > acc, "the evaluated set ignores the rule"
            assert g.run_form() == 0
            with pytest.raises(engine.ICPError) as e:
                g.track_next(engine.synth_cloud_vga())
            assert e.value.code == ESTATE
        g.write(Mem.T, T, block=True)                       # (the step moved T by the pairs it used: the same transform for both)
        quality.append(bytes(g.evaluate(50.0)[0]))
        g.close()
    assert quality[0] == quality[1], "icp_evaluate gives the same bits with the rule on and off"


def test_form_and_launch_count(engine):
    """With the rule on the iteration is the separate form; the launches it adds are the header's."""
    for side in (128, 256):
        g = engine.ICP(0)
        g.init(side * side, 256, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0, tail = g.run_form(), (3 if (side * side // 64 + 127) // 128 > 2 else 2)
        g.set_reciprocal(True, 5.0)
        assert g.run_form() == 0
        assert g.launches_per_iteration() == tail + ADDED_P2P
        g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
        assert g.launches_per_iteration() == 4 + ADDED_P2P
        g.set_unique(True)                                  # (the apply pass runs anyway: the rule adds 3)
        assert g.launches_per_iteration() == 4 + 3 + 3
        g.set_unique(False)
        g.setReduceMode(engine.ReduceMode.FUSED)
        g.set_normals(1, side)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        plane_on = g.launches_per_iteration()
        g.set_reciprocal(False)
        assert plane_on == g.launches_per_iteration() + ADDED_PLANE == 1 + 2 + ADDED_PLANE
        g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT, 0.0)
        assert g.run_form() == form0
        g.close()


def test_profile_run_counts_the_additions_into_the_search_stage(engine, scenes_A):
    F, M, _, invalid, _, _ = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid, 20.0)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    n = 4
    for _ in range(n):
        g.step()
    want = _snapshot(engine, g)
    g.reset_transform(); g.buildRBC()
    table, _ = g.profile_run(n)
    _same(want, _snapshot(engine, g))
    assert table.shape == (n, 4) and np.all(table[:, 0] > 0)
    g.close()


# ---- 12. icp_batch_* and the pyramid

def test_icp_batch_with_two_registrations_on_one_slot(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 2
    m = side * side
    pairs = [_holes(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    assert bt.reciprocal() is None
    bt.set_reciprocal(True, 20.0)
    assert bt.reciprocal() == 20.0
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = make_handle(engine, m, nr, True, WEIGHTED, POWER, True, True, 20.0)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        u = bt.read(i, engine.Memory.RECIPROCAL)
        assert np.array_equal(u, g.read(engine.Memory.RECIPROCAL)) and 0 < u[3] < u[0], i
        assert np.array_equal(bt.read(i, engine.Memory.REVERSE_ID)["id"], g.read(engine.Memory.REVERSE_ID)["id"]), i
        g.close()
    bt.close()


def test_two_level_pyramid(engine):
    """The rule on both level handles: level 0's words are non-zero, and its T is the chain of two plain handles handed over by
    icp_write (ICP_MEM_T)."""
    import pyramid_ref as PR
    F, M = _holes(engine, 128, 7, "blobs30")
    nr, its = (256, 64), [3, 3]
    Fs, Ms = PR.build(F, 128, 2), PR.build(M, 128, 2)
    Mem = engine.Memory
    want = [None] * 2
    T = np.array(IDENTITY, F32)
    for l in (1, 0):
        g = engine.ICP(0)
        g.set_rejection(True, None)
        g.set_reciprocal(True, 20.0)
        g.init(Fs[l].shape[0], nr[l], A, C_)
        g.write(Mem.F, Fs[l]); g.write(Mem.M, Ms[l])
        g.buildRBC()
        g.write(Mem.T, T)
        g.run_fixed(its[l])
        want[l] = (g.read(Mem.T).copy(), g.read(Mem.RECIPROCAL).copy())
        T = want[l][0].reshape(-1).copy()
        g.close()
    p = engine.ICPPyramid(0)
    try:
        p.init(128 * 128, nr, A, C_)
        for l in range(2):
            p.level(l).set_rejection(True, None)
            p.level(l).set_reciprocal(True, 20.0)
        p.write(Mem.F, F)
        p.write(Mem.M, M)
        p.buildRBC()
        p.run_fixed(its)
        p.sync()
        for l in range(2):
            assert_bits(p.level(l).read(Mem.T), want[l][0], "T of level %d" % l)
            assert np.array_equal(p.level(l).read(Mem.RECIPROCAL), want[l][1]), l
        assert np.all(want[0][1][[0, 1, 3]] > 0), want[0][1]
    finally:
        p.close()


# ---- 13. every search layout: the back search's database is M with its holes, its queries every fixed point

@pytest.mark.parametrize("case", icp_checks.LAYOUT_CASES,
                         ids=lambda c: "%d-%d-%d-%s-%s" % (c[0], c[1], c[2], "fused" if c[3] else "reference_order", c[4]))
def test_every_search_layout(engine, oracle, case):
    """icp_checks.layout_scene's pairs with its rejection and trimming, the rule between them at layout_reciprocal's max_gap; one step
    from _t0 ().  Per registration REVERSE_ID for every fixed point — in the scenes with holes thousands of them are invalid points
    whose answer is a tie among M's coincident origin points —, the RECIPROCAL and TRIM words, ICP_MEM_W and the LAST_ITERATION set,
    all against the oracle's pairs alone.  tests/test_reciprocal_cpu.py proves the conditions asserted at the end from the oracle;
    here they are asserted on the device's words and ids."""
    side, nr, batch, fused, zero, layout = case
    m = side * side
    Mem = engine.Memory
    sc, lr = icp_checks.layout_scene(side, nr, batch, zero), icp_checks.layout_reciprocal(side, nr, batch, zero)
    g = icp_checks.make_handle(engine, m, nr, fused, WEIGHTED, POWER, fused, batch, rejection=(True, sc.max_dist), trimming=icp_checks.LAYOUT_KEEP)
    g.set_reciprocal(True, lr.max_gap)
    assert g.search_layout() == layout, g.search_layout()
    if batch == 1:
        one_step(engine, g, sc.pairs[0][0], sc.pairs[0][1], sc.T)
    else:
        step_batch(engine, g, sc.pairs, sc.T)
    words, finals, counted, origin = [], [], [], 0
    for b, ((F, M), want, back, r) in enumerate(zip(sc.pairs, sc.wants, lr.backs, lr.rules)):
        what = "side %d, |R| %d, registration %d of %d" % (side, nr, b, batch)
        icp_checks.check_search(engine, g, want, b)
        icp_checks.check_back_search(engine, g, back, b, what)
        words.append(assert_words(engine, g, "RECIPROCAL", r.words["RECIPROCAL"], b))
        assert_words(engine, g, "TRIM", r.words["TRIM"], b)
        gW = g.read(Mem.W, batch_index=b)
        assert_bits(gW, r.W, "ICP_MEM_W (%s)" % what)
        got = icp_checks.check_route_pairs(engine, g, want[0], sc.PF[b], sc.PM[b], r, False, lr.options, b, what)
        finals.append(len(got))
        counted.append(int(np.count_nonzero(quality_ref.masks(M, sc.PF[b], sc.PM[b], 0.0)[0])))
        origin += int(np.count_nonzero(icp_checks.origin_rows(M)[g.read(Mem.REVERSE_ID, batch_index=b)["id"]]))
    holes = any(icp_checks.origin_rows(M).any() for _, M in sc.pairs)
    print(case[:5], "max_gap", lr.max_gap, [w.tolist() for w in words], finals, counted, origin)
    icp_checks.layout_reciprocal_conditions(words, finals, counted, origin / (batch * m) if holes else None, str(case[:5]))
    g.close()


# ---- 14. a converged registration of a checked run is left alone by every launch the rule adds

@pytest.mark.parametrize("metric,fused", [("p2p", True), ("p2p", False), ("p2pl", None)])
def test_a_converged_registration_is_left_alone(engine, metric, fused):
    """One handle, three registrations, dense by batch, a checked run with the rule on.  Registration 0 registers a frame with itself
    and is done at k = 1 (tests/test_reciprocal_cpu.py); the other two go on for at least two more iterations, every one of which
    launches the state kernel, the back search and the test over all three.  Each registration's k, T, W, words, back search and
    LAST_ITERATION set are those of a handle that runs the same pair alone."""
    Mem = engine.Memory
    pairs = icp_checks.converged_pairs()
    s0 = icp_checks.route_scene("batch0")
    o = icp_checks.route_scene_options(s0, 16)
    read = lambda g, b: (g.state(b).k, g.read(Mem.T, b).copy(), g.read(Mem.W, b).copy(), g.read(Mem.RECIPROCAL, b).copy(),
                         g.read(Mem.REVERSE_ID, b).view(np.uint32).copy(), g.correspondences(engine.Pairs.LAST_ITERATION, batch_index=b).view(np.uint32).copy())
    alone = []
    for F, M in pairs:
        h = icp_checks.route_handle(engine, s0.side, s0.nr, o, metric, fused)
        icp_checks.load(engine, h, F, M)
        h.buildRBC()
        assert h.run() == h.state().k
        alone.append(read(h, 0))
        h.close()
    assert alone[0][0] == 1 and alone[1][0] >= 3 and alone[2][0] >= 3, [a[0] for a in alone]
    assert alone[0][3].tolist() == [14742, 14742, 0, 14742], alone[0][3]
    g = icp_checks.route_handle(engine, s0.side, s0.nr, o, metric, fused, batch=3)
    assert g.search_layout()[0] == 1, g.search_layout()
    for b, (F, M) in enumerate(pairs):
        icp_checks.load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    for b in range(3):
        got = read(g, b)
        assert got[0] == alone[b][0], "k of registration %d: %d, alone %d" % (b, got[0], alone[b][0])
        for x, y, name in zip(got[1:], alone[b][1:], ("T", "W", "RECIPROCAL", "REVERSE_ID", "the LAST_ITERATION set")):
            assert_bits(x, y, "%s of registration %d against the same pair alone" % (name, b))
        assert 0 < got[3][3] and len(got[5]) > 0
    assert g.state(0).k == 1 and g.state(1).k >= 3 and g.state(2).k >= 3
    g.close()


# ---- 15. the rule's edges on the device

def test_max_gap_at_a_pair_s_own_gap(engine, oracle):
    """Scene 30 behind the search's rejection, the rule alone.  g2: a squared gap of a non-exact candidate that some float squares to
    (reciprocal_ref.equality_gap; tests/test_reciprocal_cpu.py).  With that float as max_gap the pair is near — the device's <= against
    (float) ((double) max_gap * max_gap) —, with the next float below it is not: `near` drops by exactly the pairs at g2."""
    s = icp_checks.route_scene("30")
    ids, rev = s.want[0]["id"], s.back[0][0]["id"]
    W0 = weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, s.max_dist)
    g2, gap, below, pairs, (distinct, have) = ref.equality_gap(ids, rev, s.PM, W0)
    assert have > 0 and pairs >= 1 and F32(np.float64(F32(gap)) * np.float64(F32(gap))) == g2
    rows = np.flatnonzero(ref.reciprocal_rule(ids, rev, s.PM, W0, gap)[1] & ~ref.reciprocal_rule(ids, rev, s.PM, W0, below)[1])
    assert len(rows) == pairs
    g = icp_checks.make_handle(engine, s.side * s.side, s.nr, True, WEIGHTED, POWER, True, rejection=(True, s.max_dist))
    near = []
    for k, max_gap in enumerate((gap, below)):
        g.set_reciprocal(True, max_gap)
        if k == 0:
            one_step(engine, g, s.F, s.M, s.T)
        else:
            g.write(engine.Memory.T, s.T, block=True)
            g.step()
        counts = check_step(engine, oracle, g, s.F, s.M, s.T, s.side, True, WEIGHTED, POWER, True, True, s.back[0], max_gap, s.want,
                            max_dist=s.max_dist)
        want = ref.reciprocal_rule(ids, rev, s.PM, W0, max_gap)
        assert counts.tolist() == want[3].tolist(), (counts, want[3])
        assert np.array_equal(g.read(engine.Memory.W)[rows] != 0, np.full(pairs, k == 0)), "the pairs at the gap are near at it and not below it"
        near.append(int(g.read(engine.Memory.RECIPROCAL)[2]))
    assert near[0] - near[1] == pairs and near[1] > 0, near
    g.close()


def _check_messy(engine, g, s, b, what):
    """Registration b holds messy_scene s: the back search for every fixed point, the words and W against the rule, the forward search
    on the finite rows."""
    Mem = engine.Memory
    icp_checks.check_back_search(engine, g, s.back, b, what)
    exact, near, zero, words = s.rule
    got = assert_words(engine, g, "RECIPROCAL", words, b)
    assert_bits(g.read(Mem.W, batch_index=b), np.where(zero, F32(0), s.W0).astype(F32), "ICP_MEM_W (%s)" % what)
    nn = g.read(Mem.NN_ID, batch_index=b)
    assert np.array_equal(nn["id"][s.finite], s.want[0]["id"][s.finite]), "forward ids on the finite rows (%s)" % what
    assert_bits(nn["dist"][s.finite], s.want[0]["dist"][s.finite], "forward distances on the finite rows (%s)" % what)
    icp_checks.messy_conditions(s.finite, s.W0, g.read(Mem.REVERSE_ID, batch_index=b)["id"], got, what)


def test_non_finite_moving_rows_alone(engine, oracle):
    """(50, 4): M — the back search's database — with holes and thirty NaN / +inf / -inf coordinates; rejection by invalid points and a
    max_dist from the clean pair, so a non-finite row is no candidate.  No back answer names such a row."""
    side, nr = icp_checks.MESSY_SHAPES[0]
    s = icp_checks.messy_scene(side, nr)
    g = icp_checks.make_handle(engine, side * side, nr, True, WEIGHTED, POWER, True, rejection=(True, s.max_dist))
    g.set_reciprocal(True, s.max_gap)
    one_step(engine, g, s.F, s.M, s.T)
    _check_messy(engine, g, s, 0, "(%d, %d) alone" % (side, nr))
    g.close()


def test_non_finite_moving_rows_in_a_batch_of_three(engine, oracle):
    """(64, 64) x 3 — three registrations side by side in the latency layout —; only registration 1 is messy.  Its clean neighbours are bit-identical to the same batch with the
    clean M in registration 1."""
    side, nr = icp_checks.MESSY_SHAPES[1]
    s = icp_checks.messy_scene(side, nr)
    Mem = engine.Memory
    neighbours = [engine.synth_pair(side, seed=0x5EED + side + 7 * (b + 1), rot_deg=3.0 + 0.5 * b) for b in range(2)]
    out = []
    for M1 in (s.M, s.clean):
        pairs = [neighbours[0], (s.F, M1), neighbours[1]]
        g = icp_checks.make_handle(engine, side * side, nr, True, WEIGHTED, POWER, True, 3, rejection=(True, s.max_dist))
        g.set_reciprocal(True, s.max_gap)
        step_batch(engine, g, pairs, s.T)
        if M1 is s.M:
            _check_messy(engine, g, s, 1, "(%d, %d), registration 1 of 3" % (side, nr))
        out.append([[g.read(mem, batch_index=b).view(np.uint32).copy() for mem in (Mem.T, Mem.W, Mem.RECIPROCAL, Mem.REVERSE_ID, Mem.NN_ID)]
                    for b in (0, 2)])
        g.close()
    for b, messy, clean in zip((0, 2), out[0], out[1]):
        for x, y, name in zip(messy, clean, ("T", "W", "RECIPROCAL", "REVERSE_ID", "NN_ID")):
            assert_bits(x, y, "%s of registration %d beside a messy registration" % (name, b))
        assert 0 < messy[2][3] < messy[2][0], messy[2]
