"""One-to-one correspondences (icp_set_unique): of the candidate pairs that share a fixed point only the closest keeps its weight (a tie
goes to the lowest query index); every other gets the weight +0 and is then a rejected pair.  The search is not touched.

The winners come from numpy — tests/unique_ref.py: np.minimum.at on the 64-bit keys, from the engine's own NN_ID / NN / QT outputs and
the weights before the rule —, and the reference values from the oracle's piecewise entries with the losers' and rejected rows zeroed
(tests/test_gpu_trimming.py's construction).  ICP_MEM_UNIQUE holds (candidates, winners) of the last iteration.  Everything is
compared bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                 # noqa: E402
import robust_ref                                               # noqa: E402
import unique_ref as ref                                        # noqa: E402
import icp_checks      # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, POWER, EIGEN, REGULAR, WEIGHTED, assert_bits, check_unique_step as check_step,  # noqa: E402
                        expected_pieces, holes_pair as _holes, one_step, oracle_search, only_invalid, set_modes, trim_rule,
                        unique_rule_of as numpy_rule, _partial_overlap, step_batch, _t0)

pytestmark = pytest.mark.gpu

# What the header documents for icp_launches_per_iteration: the rule adds claim + resolve + the apply pass on point-to-point, claim +
# resolve on the plane metrics.
ADDED_P2P, ADDED_PLANE = 3, 2


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, batch=1, unique=True):
    return icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid),
                                  unique=True if unique else None)


@pytest.fixture(scope="module")
def scenes_A(engine, oracle):
    """name -> (F, M, T, invalid flag, the oracle's (nn_id, rid) at T): a clean pair and a blobs30 holes pair."""
    return icp_checks.scenes_A(engine, oracle)


# ---- 0. arguments

def test_arguments_and_getter(engine):
    g = engine.ICP(0)
    L = engine.lib()
    assert g.unique() is False
    assert L.icp_set_unique(g._h, 2) == 1 and L.icp_set_unique(g._h, -1) == 1            # ICP_EINVAL
    assert g.unique() is False
    g.set_unique(True)
    assert g.unique() is True
    g.init(256, 16, A, C_)                              # the setting survives icp_init
    assert g.unique() is True
    assert np.all(g.read(engine.Memory.UNIQUE) == 0)    # (no iteration yet)
    g.set_unique(False)
    assert g.unique() is False
    g.close()


# ---- 1. one step at the latency layout, every mode, clean and with holes

@pytest.mark.parametrize("scene", ["clean", "holes"])
@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, scenes_A, fused, weighted, rot, power_fast, scene):
    F, M, T, invalid, want = scenes_A[scene]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, rot, power_fast, invalid)
    one_step(engine, g, F, M, T)
    win, counts = check_step(engine, oracle, g, F, M, T, 128, fused, weighted, rot, power_fast, invalid, want)
    assert counts[1] == np.count_nonzero(win) < counts[0]
    if scene == "clean":
        # (every pair is a candidate: the winners are the distinct fixed points of the CPU oracle's search — 5589 at the tests' alpha = 200;
        # test_winner_count_of_the_oracle pins the 5587 of alpha = 100)
        assert counts.tolist() == [16384, len(np.unique(want[0]["id"]))] == [16384, 5589], counts
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_winner_count_of_the_oracle(engine, oracle, fused):
    """synth_pair (128), |R| = 256, _t0(): the CPU oracle matches 5587 distinct fixed points among the 16384 pairs, at most 54 queries
    on one — with the oracle's default alpha = 100, which is what that figure was taken with (at the tests' alpha = 200 it is 5589:
    test_one_step_config_A).  Exactly 5587 winners: the search and the rule together; any second claim let through raises it."""
    side, nr, a = 128, 256, 1e2
    F, M = engine.synth_pair(side)
    T = _t0()
    o = oracle.OracleICP(side * side, nr, a, C_, threads=8)
    o.write_f(F); o.write_m(M); o.build_rbc(); o.write_t(T)
    o.step()
    assert len(np.unique(o.nn_id["id"])) == 5587 and np.bincount(o.nn_id["id"]).max() == 54
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, nr, a, C_)
    set_modes(engine, g, fused, fused)
    g.set_unique(True)
    one_step(engine, g, F, M, T)
    gn = g.read(engine.Memory.NN_ID)
    assert np.array_equal(gn["id"], o.nn_id["id"]) and np.array_equal(g.read(engine.Memory.RID), o.rid)
    assert_bits(gn["dist"], o.nn_id["dist"], "correspondence distances")
    assert g.read(engine.Memory.UNIQUE).tolist() == [16384, 5587]
    assert np.count_nonzero(g.read(engine.Memory.W)) == 5587
    win, _, counts, _ = numpy_rule(engine, g, M, True, False)
    assert counts.tolist() == [16384, 5587] and np.array_equal(g.read(engine.Memory.W) != 0, win)
    g.close()


# ---- 2. smallest shapes: sides that are no multiple of 8, blocks with lanes past m

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", [(6, 4), (14, 4), (16, 16), (30, 4)])
def test_small_shapes(engine, oracle, side, nr, fused):
    F, M = engine.synth_pair(side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False)
    one_step(engine, g, F, M, T)
    win, counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, oracle_search(oracle, F, M, T, nr))
    assert counts[0] == side * side and 0 < counts[1] <= counts[0]
    if (side, nr) == (16, 16):
        assert counts.tolist() == [256, 151], counts    # (the CPU oracle's search: 151 distinct fixed points among the 256 pairs)
    g.close()


# ---- 3. dense layouts: a batch, and 65536 pairs

@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch3(engine, oracle, fused):
    from icp_amd import workloads as W
    side, nr, B = 128, 256, 3
    pairs = [W.pair(engine, 0), _holes(engine, side, W.BASE_SEED + 3, "blobs30"), _holes(engine, side, W.BASE_SEED + 6, "scattered10")]
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, batch=B)
    step_batch(engine, g, pairs, T)
    seen = set()
    for b, (F, M) in enumerate(pairs):
        _, counts = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, oracle_search(oracle, F, M, T, nr), b=b)
        seen.add(tuple(counts.tolist()))
    assert len(seen) == B, seen
    g.close()


@pytest.mark.parametrize("fused,weighted,rot", [(True, WEIGHTED, POWER), (False, REGULAR, EIGEN)])
def test_one_step_65536(engine, oracle, fused, weighted, rot):
    """m = 65536, |R| = 1024: the table and both passes span many blocks; the oracle's pieces fed the engine's own correspondences."""
    side, nr = 256, 1024
    F, M = _holes(engine, side, 0x1C9D5EED + 7)
    T = _t0()
    g = make_handle(engine, F.shape[0], nr, fused, weighted, rot, fused, True)
    one_step(engine, g, F, M, T)
    _, counts = check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, fused, True)
    assert 10000 < counts[1] < counts[0]
    g.close()


# ---- 4. ties

@pytest.mark.parametrize("fused", [True, False])
def test_a_tie_goes_to_the_lowest_query_index(engine, oracle, fused):
    """M[2j] = M[2j + 1] = F[2j], the identity, no noise: both queries claim F[2j] with geo = 0, and the even one wins."""
    side, nr = 64, 64
    F, _ = engine.synth_pair(side)
    m = side * side
    M = F.copy()
    M[1::2] = F[0::2]
    T = IDENTITY.copy()
    g = make_handle(engine, m, nr, fused, WEIGHTED, POWER, fused, False)
    one_step(engine, g, F, M, T)
    # numpy first: the construction only counts if the ids show the doubled claims
    nn_id = g.read(engine.Memory.NN_ID)
    PF, PM = g.read(engine.Memory.NN), g.read(engine.Memory.QT)
    assert np.array_equal(nn_id["id"], (np.arange(m) // 2 * 2).astype(np.uint32)), "every pair of queries claims F[2j]"
    assert np.all(ref.geo(PF, PM) == 0)
    win, _, counts, _ = numpy_rule(engine, g, M, True, False)
    assert counts.tolist() == [m, m // 2] and np.array_equal(np.flatnonzero(win), np.arange(0, m, 2))
    check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False)
    gW = g.read(engine.Memory.W)
    assert np.all(gW[0::2] != 0) and np.all(gW[1::2].view(np.uint32) == 0)
    assert g.read(engine.Memory.UNIQUE).tolist() == [m, m // 2]
    g.close()


def test_nothing_left_is_the_identity_step(engine):
    """Every pair rejected before the rule (no candidate, no winner): one identity step, T as it was, ICP_MEM_UNIQUE (0, 0)."""
    side, nr = 32, 64
    F, M = engine.synth_pair(side)
    T0 = _t0()
    for fused in (True, False):
        g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False)
        g.set_rejection(False, 1e-3)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        g.write(engine.Memory.T, T0, block=True)
        assert g.run() == 1
        Mem = engine.Memory
        assert_bits(g.read(Mem.T), T0, "T")
        assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
        assert np.all(g.read(Mem.UNIQUE) == 0)
        assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W) == 0.0)
        g.close()


# ---- 5. the search is untouched

def test_search_is_untouched(engine, scenes_A):
    F, M, T, invalid, _ = scenes_A["holes"]
    out = []
    for on in (False, True):
        g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid, unique=on)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy(),
                    g.read(engine.Memory.NN)[:, :3].copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")
    assert_bits(out[0][3], out[1][3], "matched fixed points")


# ---- 6. combinations

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_with_trimming(engine, oracle, scenes_A, fused, weighted):
    """Trimming's candidates are the winners: ICP_MEM_TRIM's n is the winner count, the accepted set numpy's trim rule on them."""
    F, M, T, invalid, want = scenes_A["holes"]
    keep = 0.8
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], 256, fused, weighted, POWER, fused, invalid)
    g.set_trimming(keep)
    one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    assert np.array_equal(nn_id["id"], want[0]["id"])
    win, _, counts, W0 = numpy_rule(engine, g, M, weighted, invalid)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    acc, trim = trim_rule(PF, PM, np.where(win, W0, np.float32(0)).astype(np.float32), keep)
    assert np.array_equal(g.read(Mem.UNIQUE), counts)
    got = g.read(Mem.TRIM)
    assert np.array_equal(got, trim), ("ICP_MEM_TRIM", got, trim)
    assert got[1] == g.read(Mem.UNIQUE)[1] and got[3] < got[1]
    W, sw, means, S, Tk = expected_pieces(oracle, F, M, T, nn_id, 128, fused, weighted, POWER, fused, ~acc)
    gW = g.read(Mem.W)
    assert_bits(gW, W, "weights")
    assert np.all(np.ascontiguousarray(gW[~acc]).view(np.uint32) == 0)
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits(g.read(Mem.TK), Tk, "Tk")
    assert g.launches_per_iteration() == (2 if fused else 4) + 2 + 2      # (tail, select + apply, claim + resolve)
    g.close()


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_with_a_huber_loss(engine, oracle, scenes_A, fused, weighted):
    """The loss weighs the winners: W' = robust_ref.p2p_weights on the weights behind the rule."""
    F, M, T, invalid, _ = scenes_A["holes"]
    scale = 8.0
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], 256, fused, weighted, POWER, fused, invalid)
    g.set_robust_loss(robust_ref.HUBER, scale)
    one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    win, _, counts, W0 = numpy_rule(engine, g, M, weighted, invalid)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W = robust_ref.p2p_weights(np.where(win, W0, np.float32(0)).astype(np.float32), PF, PM, robust_ref.HUBER, scale)
    assert np.array_equal(g.read(Mem.UNIQUE), counts)
    assert_bits(g.read(Mem.W), W, "W'")
    assert np.count_nonzero(W) == counts[1] and np.count_nonzero((W != 0) & (W != W0)) > 100       # (the loss cuts into the winners)
    zero = W == 0
    NNz, tMz = np.ascontiguousarray(F[nn_id["id"]]), oracle.transform_q(M, T)
    NNz[zero] = 0.0; tMz[zero] = 0.0
    if fused:
        sw, means, S = oracle.moments_fused(NNz, tMz, W, 128, C_)
    else:
        sw = robust_ref.sum_w_reference(W)
        means = oracle.mean_weighted(NNz, tMz, W, sw)
        DF, DM = oracle.devs(NNz, tMz, means)
        S = oracle.sij(DM, DF, W, C_)
    Tk, _ = oracle.power_method(S, means, fast=fused)
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits(g.read(Mem.TK), Tk, "Tk")
    assert g.launches_per_iteration() == (2 if fused else 4) + 1 + 2      # (tail, the loss's apply pass, claim + resolve)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_with_point_to_plane(engine, scenes_A, fused):
    """ICP_MEM_PLANE_SYSTEM, T, R, TK against tests/p2pl_ref.py's float64 restatement fed numpy's winners' weights: bit for bit, as
    tests/test_gpu_point_to_plane.py compares."""
    F, M, _, invalid, _ = scenes_A["holes"]
    mu, side = 0.05, 128
    Mem = engine.Memory
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, 256, A, C_)
    set_modes(engine, g, fused, fused)
    g.set_normals(1, side)                               # Normals.GRID
    g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, mu)
    g.set_rejection(True, None)
    g.set_unique(True)
    assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + ADDED_PLANE
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    for _ in range(3):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        win, zero, counts, W0 = numpy_rule(engine, g, M, True, invalid)
        assert np.array_equal(g.read(Mem.UNIQUE), counts) and counts[1] < counts[0]
        PF = g.read(Mem.NN).copy()
        assert_bits(PF[:, 3], np.where(zero, np.float32(0), W0).astype(np.float32), "weights")
        PF[:, 3] = np.where(zero, np.float32(0), W0)
        system, T, R, Tk, Rk = p2pl_ref.step(PF, g.read(Mem.QT), g.read(Mem.NN_ID)["id"], g.read(Mem.NORMALS_F), mu, T0, R0)
        assert system[27] == 1.0
        assert_bits(g.read(Mem.PLANE_SYSTEM), system, "PLANE_SYSTEM")
        assert_bits(g.read(Mem.T), T, "T")
        assert_bits(g.read(Mem.R).ravel(), R, "R")
        assert_bits(g.read(Mem.TK), Tk, "TK")
    g.close()


@pytest.mark.parametrize("metric", ["colored", "plane_to_plane", "symmetric"])
def test_other_plane_metrics_equal_removal_by_rejection(engine, scenes_A, metric):
    """Colored, plane-to-plane and symmetric: a step with the rule on equals a step with the rule off on a moving set whose losers
    were removed another way — put at the origin, which ICP_REJECT_INVALID rejects — wherever that leaves the search alone: the
    system of the winners is compared through T after the step and ICP_MEM_W."""
    F, M, T, invalid, _ = scenes_A["holes"]
    side = 128
    Mem = engine.Memory

    def handle(unique):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, 256, A, C_)
        g.set_normals(1, side)
        if metric == "colored":
            g.set_color_weight(1000.0)
            g.set_error_metric(engine.ErrorMetric.COLORED, 0.05)
        else:
            if metric == "plane_to_plane":
                g.set_plane_to_plane(0.001)
            else:
                g.set_symmetric(True)
            g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        g.set_rejection(True, None)
        if unique:
            g.set_unique(True)
        return g

    g = handle(True)
    assert g.launches_per_iteration() == 1 + 2 + ADDED_PLANE
    one_step(engine, g, F, M, T)
    win, zero, counts, W0 = numpy_rule(engine, g, M, True, invalid)
    assert np.array_equal(g.read(Mem.UNIQUE), counts)
    assert_bits(g.read(Mem.W), np.where(zero, np.float32(0), W0).astype(np.float32), "weights")
    on = [g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.T).copy()]
    # the same step with the rule off: the losers' weights written as zeros into NN by hand is not possible from outside, so the
    # losers leave through rejection: their moving points at the origin (the moving normals and intensities of the others stay)
    Mz = M.copy()
    Mz[zero] = 0.0
    h = handle(False)
    if metric != "colored":
        h.set_normals(0, 0)                             # Normals.GIVEN: the same normals as the run with the rule on
    h.write(Mem.F, F); h.write(Mem.M, Mz)
    h.buildRBC()
    if metric != "colored":
        h.write(Mem.NORMALS_F, g.read(Mem.NORMALS_F)); h.write(Mem.NORMALS_M, g.read(Mem.NORMALS_M))
    h.write(Mem.T, T, block=True)
    h.step()
    hz = h.read(Mem.W) == 0
    assert np.array_equal(hz, zero), "the same pairs weigh nothing"
    assert np.array_equal(h.read(Mem.NN_ID)["id"][~zero], g.read(Mem.NN_ID)["id"][~zero])
    assert_bits(h.read(Mem.PLANE_SYSTEM), on[0], "PLANE_SYSTEM")
    assert_bits(h.read(Mem.T), on[1], "T")
    g.close(); h.close()


# ---- 7. multi-iteration: run, run_fixed, twice on one handle, icp_batch, tracking

def _snapshot(engine, g):
    Mem = engine.Memory
    return [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.UNIQUE).copy(), g.read(Mem.NN_ID)["id"].copy()]


def _same(a, b):
    for x, y, what in zip(a, b, ("T", "W", "UNIQUE", "ids")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_run_equals_steps(engine, scenes_A, fused, weighted):
    """A checked run and run_fixed against the same iterations as single steps — where a table not cleared between iterations
    shows —, and the same registration twice on one handle."""
    F, M, _, invalid, _ = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, POWER, fused, invalid)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    run = _snapshot(engine, g)
    assert 0 < run[2][1] < run[2][0]
    assert np.count_nonzero(run[1]) == run[2][1], "the lazily read weights show the rule's zeros"
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    _same(run, _snapshot(engine, g))
    g.reset_transform(); g.buildRBC()
    assert g.run() == k
    _same(run, _snapshot(engine, g))                    # twice on one handle
    n = 5
    g.reset_transform(); g.buildRBC()
    g.run_fixed(n)
    fixed = _snapshot(engine, g)
    g.reset_transform(); g.buildRBC()
    for _ in range(n):
        g.step()
    _same(fixed, _snapshot(engine, g))
    g.close()


def test_profile_run_counts_the_passes_into_the_search_stage(engine, scenes_A):
    F, M, _, invalid, _ = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    n = 5
    for _ in range(n):
        g.step()
    want = _snapshot(engine, g)
    g.reset_transform(); g.buildRBC()
    table, _ = g.profile_run(n)
    _same(want, _snapshot(engine, g))
    assert table.shape == (n, 4) and np.all(table[:, 0] > 0)
    g.close()


def test_icp_batch_equals_single_handles(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [_holes(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    assert bt.unique() is False
    bt.set_unique(True)
    assert bt.unique() is True
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = make_handle(engine, m, nr, True, WEIGHTED, POWER, True, True)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        u = bt.read(i, engine.Memory.UNIQUE)
        assert np.array_equal(u, g.read(engine.Memory.UNIQUE)) and 0 < u[1] < u[0], i
        g.close()
    bt.close()


def test_tracking_equals_run_on_the_landmarks(engine, oracle):
    frames = [engine.punch_holes(engine.synth_cloud_vga(moved=f), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=77 + f)
              for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    g, h = (make_handle(engine, 16384, 256, True, WEIGHTED, POWER, True, True) for _ in range(2))
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h.write(engine.Memory.F, lms[i - 1]); h.write(engine.Memory.M, lms[i])
        h.reset_transform(); h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], h.read(engine.Memory.NN_ID)["id"]), i
        u = g.read(engine.Memory.UNIQUE)
        assert np.array_equal(u, h.read(engine.Memory.UNIQUE)) and 0 < u[1] < u[0], i
    g.close(); h.close()


# ---- 8. off again equals never on; the form and the launch counts

def test_off_again_equals_never_on(engine, scenes_A):
    F, M, _, _, _ = scenes_A["holes"]
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        g.set_rejection(True, None)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        form0 = g.run_form()
        if toggled:
            g.set_unique(True)
            assert g.run_form() == 0
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(engine.Memory.UNIQUE)[1] > 0
            g.set_unique(False)
            assert g.unique() is False
            assert np.all(g.read(engine.Memory.UNIQUE) == 0)
            assert g.run_form() == form0
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy(),
                    g.read(engine.Memory.W).view(np.uint32).copy()))
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


def test_form_and_launch_count(engine):
    """With the rule on the iteration is the separate form; the launches it adds are the header's: claim, resolve and the apply pass
    on point-to-point, claim and resolve on point-to-plane."""
    for side in (128, 256):
        g = engine.ICP(0)
        g.init(side * side, 256, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0, tail = g.run_form(), (3 if (side * side // 64 + 127) // 128 > 2 else 2)
        g.set_unique(True)
        assert g.run_form() == 0
        assert g.launches_per_iteration() == tail + ADDED_P2P
        g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
        assert g.launches_per_iteration() == 4 + ADDED_P2P
        g.setReduceMode(engine.ReduceMode.FUSED)
        g.set_normals(1, side)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        plane_on = g.launches_per_iteration()
        g.set_unique(False)
        assert plane_on == g.launches_per_iteration() + ADDED_PLANE == 1 + 2 + ADDED_PLANE
        g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT, 0.0)
        assert g.run_form() == form0
        g.close()


# ---- 9. what it is for: partial overlap, measured

@pytest.mark.parametrize("fused", [True, False])
def test_one_to_one_copes_with_partial_overlap(engine, fused):
    """tests/test_gpu_trimming.py's partial-overlap scene (1 degree, (8, -4, 5) mm, a quarter of M pushed 150 mm off), the rule off, on,
    and on together with trimming 0.7 (and trimming alone, for the record); rotation / translation error against T_true.  Measured on
    an MI355X (both reduce modes alike): off 0.431 deg / 8.27 mm in 30 iterations; on 0.221 deg / 2.29 mm, still moving at the 40th
    iteration (k = 40: fewer, better pairs, smaller steps); on with trimming 0.7: 0.170 deg / 3.01 mm in 25; trimming 0.7 alone 0.157 deg
    / 3.12 mm in 21.  The rule ends clearly closer to T_true than the run without it; the bounds leave room on both sides."""
    from icp_amd import workloads as W
    F, M, T_true = _partial_overlap(engine)
    res = {}
    for name, on, keep in (("off", False, 1.0), ("on", True, 1.0), ("on + trim 0.7", True, 0.7), ("trim 0.7", False, 0.7)):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_unique(on)
        g.set_trimming(keep)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        T = g.read(engine.Memory.T).copy()
        g.close()
        res[name] = (k, W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])))
        print("partial overlap %s, one-to-one %s: k = %d, %.3f deg %.2f mm" % ("fused" if fused else "reference order", name, *res[name]))
    for name in ("on", "on + trim 0.7"):
        assert 1 < res[name][0] <= 40, (name, res)
    assert res["off"][2] > 6.0 and res["off"][1] > 0.3, res
    assert res["on"][2] < 4.0 and res["on"][1] < 0.3, res
    assert res["on + trim 0.7"][2] < 4.5 and res["on + trim 0.7"][1] < 0.25, res
