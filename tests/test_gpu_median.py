"""Median-distance rejection (icp_set_median_rejection): every iteration rejects the candidate pairs farther apart than factor times the
median pair distance of that iteration — geo > thr, thr = (float) (factor^2 t_med), t_med the lower median of the candidates' geo — and
gives them the weight +0; the search is not touched.

The accepted set comes from numpy (tests/median_ref.py: the rule of include/icp_amd.h applied to the engine's own NN / QT outputs), the
reference values from the oracle's piecewise entries with the rejected rows zeroed, bit for bit.  ICP_MEM_MEDIAN holds (t_med bits, n,
thr bits, accepted) of the last iteration.

The shapes: (6, 4) — 36 pairs, most threads of the one workgroup hold no key —, (50, 4) — 2500, no multiple of 256 —, (128, 256) —
exactly 16384, the one-workgroup limit —, (130, 4) — 16900, the smallest multi-workgroup shape: nine workgroups, the last partly filled."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks      # noqa: E402
import unique_ref      # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, P2PL, POWER, REGULAR, WEIGHTED, assert_bits, assert_words, geo_of,  # noqa: E402
                        one_step, only_invalid, set_modes, step_batch, trim_rule, weights_before_trim, _partial_overlap, _t0)
from median_ref import median_rule, pick_factor      # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4
SHAPES = [(6, 4), (50, 4), (128, 256), (130, 4)]
EDGE_SHAPES = [(128, 256), (130, 4)]
ONE_BLOCK_MAX = 16384
INF_BITS = 0x7F800000


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, factor, batch=1, **options):
    g = icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid), **options)
    if factor:
        g.set_median_rejection(factor)
    return g


def oracle_pairs(oracle, F, M, T, want, weighted, invalid):
    """(PF, PM, W0) of the oracle's search at T: what the rule's factor is picked from before a handle exists."""
    nn_id = want[0]
    PF, PM = np.ascontiguousarray(F[nn_id["id"]][:, :4]), np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])
    return PF, PM, weights_before_trim(nn_id, M, PF, PM, weighted, invalid)


@functools.lru_cache(maxsize=None)
def _holes(side, nr):
    """The "holes" pair at _t0 () with the factor at which about 15 % of its candidates lie above the threshold."""
    import icp_amd as engine
    from oracle import oracle
    F, M, T, invalid, want = icp_checks.scene(engine, oracle, side, nr, "holes")
    PF, PM, W0 = oracle_pairs(oracle, F, M, T, want, True, invalid)       # (the candidates are the same in REGULAR mode: W0 != 0)
    geo = geo_of(PF, PM)
    return F, M, T, invalid, want, pick_factor(geo[(W0 != 0) & np.isfinite(geo)], 0.15)


def check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, factor, want=None, b=0):
    """ICP_MEM_MEDIAN against median_rule on the engine's own NN / QT, then the pieces.  Returns (accepted, the words)."""
    Mem = engine.Memory
    nn_id = icp_checks.correspondences(engine, g, want, b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    acc, words = median_rule(PF, PM, weights_before_trim(nn_id, M, PF, PM, weighted, invalid), factor)
    assert_words(engine, g, "MEDIAN", words, b)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, ~acc, want, b)
    return acc, words


# ---- 12. arguments

def test_arguments_and_getter(engine):
    g = engine.ICP(0)
    L = engine.lib()
    assert g.median_rejection() == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.icp_set_median_rejection(g._h, bad) == EINVAL
    assert L.icp_set_median_rejection(None, 2.0) == EINVAL
    assert g.median_rejection() == 0.0
    g.set_median_rejection(2.5)
    assert g.median_rejection() == 2.5
    g.init(256, 16, A, C_)                              # the setting survives icp_init
    assert g.median_rejection() == 2.5
    assert np.all(g.read(engine.Memory.MEDIAN) == 0)    # (no iteration yet)
    g.set_median_rejection(0.25)                        # (below 1 is allowed)
    assert g.median_rejection() == 0.25
    g.set_median_rejection(0.0)
    assert g.median_rejection() == 0.0
    g.close()


# ---- 1. one step at every shape, every mode

@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_one_step(engine, oracle, side, nr, fused, weighted, rot, power_fast):
    F, M, T, invalid, want, factor = _holes(side, nr)
    g = make_handle(engine, side * side, nr, fused, weighted, rot, power_fast, invalid, factor)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, factor, want)
    assert 0 < words[3] < words[1], words
    g.close()


# ---- 2. the search is untouched

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_search_is_untouched(engine, side, nr):
    """At the same T the correspondences, distances and nearest representatives are those of a run with the rule off, bit for bit."""
    F, M, T, invalid, _, factor = _holes(side, nr)
    out = []
    for f in (0.0, factor):
        g = make_handle(engine, F.shape[0], nr, True, WEIGHTED, POWER, True, invalid, f)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")


# ---- 3. edges

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_ties_at_the_median_are_kept(engine, oracle, side, nr):
    """Integer coordinates moved by an integer translation (the scene of trimming's test_ties_at_t_are_kept): geo is an integer, many
    pairs share the median's value — at factor 1 all of them are kept."""
    j, i = np.mgrid[0:side, 0:side]
    F = np.zeros((side * side, 8), np.float32)
    F[:, 0] = (10 * i).reshape(-1) - 640
    F[:, 1] = (10 * j).reshape(-1) - 640
    F[:, 2] = 1000 + ((i * j) % 5).reshape(-1)
    F[:, 3] = 1.0
    F[:, 4:7] = 0.5
    M = F.copy()
    M[:, 0] -= 3.0
    M[:, 1] += 4.0
    T = IDENTITY.copy()
    for fused in (True, False):
        g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, 1.0)
        one_step(engine, g, F, M, T)
        acc, words = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, 1.0)
        assert words[0] == words[2], words                               # (factor 1: thr is t_med)
        t = np.uint32(words[0]).view(np.float32)
        ties = geo_of(g.read(engine.Memory.NN), g.read(engine.Memory.QT)) == t
        K = (int(words[1]) + 1) // 2
        assert np.count_nonzero(ties) > 1000 and words[3] > K, (words, K)
        assert np.all(g.read(engine.Memory.W)[ties] != 0.0), "every tie at the median is kept"
        g.close()


@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_a_median_of_zero(engine, oracle, side, nr):
    """M = F at the identity with the last quarter of M's rows moved 150 mm: t_med == 0, thr == 0, exactly the unmoved rows accepted."""
    m = side * side
    F, _ = engine.synth_pair(side)
    M = F.copy()
    moved = np.arange(m) >= 3 * m // 4
    M[moved, 2] -= 150.0
    T = IDENTITY.copy()
    g = make_handle(engine, m, nr, True, WEIGHTED, POWER, True, False, 3.0)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, True, WEIGHTED, POWER, True, False, 3.0)
    assert words.tolist() == [0, m, 0, m - np.count_nonzero(moved)], words
    assert np.array_equal(acc, ~moved)
    g.close()


@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_factor_edges(engine, oracle, side, nr):
    """Factor 1e20: thr rounds to +inf and every candidate is accepted.  Factor 0.5: fewer than K are."""
    F, M, T, invalid, want, _ = _holes(side, nr)
    g = make_handle(engine, F.shape[0], nr, True, WEIGHTED, POWER, True, invalid, 1e20)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, True, WEIGHTED, POWER, True, invalid, 1e20, want)
    assert words[2] == INF_BITS and words[3] == words[1] > 0, words
    g.set_median_rejection(0.5)
    g.write(engine.Memory.T, T, block=True)
    g.step()
    acc, words = check_step(engine, oracle, g, F, M, T, side, True, WEIGHTED, POWER, True, invalid, 0.5, want)
    assert 0 < words[3] < (int(words[1]) + 1) // 2, words
    g.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_nothing_left_is_the_identity_step(engine, side, nr, fused):
    """Every pair rejected in front of the rule (n == 0): the run stops after one identity step, T as it was, ICP_MEM_MEDIAN zeros."""
    F, M = engine.synth_pair(side)
    T0 = _t0()
    g = engine.ICP(0)
    g.init(side * side, nr, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    g.set_rejection(False, 1e-3)
    g.set_median_rejection(2.0)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0, block=True)
    assert g.run() == 1
    Mem = engine.Memory
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert np.all(g.read(Mem.MEDIAN) == 0)
    assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W) == 0.0)
    g.close()


# ---- 4. composition: one-to-one in front, trimming behind

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_between_one_to_one_and_trimming(engine, oracle, side, nr, fused, weighted):
    """ICP_MEM_MEDIAN's n is the winner count, ICP_MEM_TRIM's n this rule's accepted count; the pieces against the three numpy rules
    applied in that order."""
    F, M, T, invalid, want, _ = _holes(side, nr)
    Mem = engine.Memory
    keep = 0.75
    PF, PM, W0 = oracle_pairs(oracle, F, M, T, want, weighted, invalid)
    win, _, _ = unique_ref.unique_rule(want[0]["id"], PF, PM, W0)
    factor = pick_factor(geo_of(PF, PM)[win], 0.15)
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, fused, invalid, factor, unique=True, trimming=keep)
    one_step(engine, g, F, M, T)
    win, _, counts, W0 = icp_checks.unique_rule_of(engine, g, M, weighted, invalid)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W1 = np.where(win, W0, np.float32(0)).astype(np.float32)
    acc_m, words_m = median_rule(PF, PM, W1, factor)
    acc_t, words_t = trim_rule(PF, PM, np.where(acc_m, W1, np.float32(0)).astype(np.float32), keep)
    assert_words(engine, g, "UNIQUE", counts)
    assert_words(engine, g, "MEDIAN", words_m)
    assert_words(engine, g, "TRIM", words_t)
    assert words_m[1] == counts[1] and words_t[1] == words_m[3] and 0 < words_t[3] < words_m[3] < words_m[1], (counts, words_m, words_t)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, POWER, fused, ~acc_t, want)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_behind_projective_association(engine, oracle, fused):
    """The same three rules behind the projection (r = 1) in the search's place."""
    import projective_ref as pref
    Mem = engine.Memory
    side, nr, zf, keep = 30, 4, 0.1, 0.75
    seed = pref.BATCH[1][0]
    F, M, T = pref.scene(side, zf, seed)
    res = pref.at(side, zf, 1, seed)
    nn = pref.clipped(res.nn_id, res.miss)
    PF, PM = np.ascontiguousarray(res.NN[:, :4]), np.ascontiguousarray(res.QT[:, :4])
    W0 = weights_before_trim(nn, M, PF, PM, WEIGHTED, True)
    win, _, _ = unique_ref.unique_rule(nn["id"], PF, PM, W0)
    factor = pick_factor(geo_of(PF, PM)[win], 0.15)
    g = icp_checks.projective_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 1,
                                     unique=True, trimming=keep)
    g.set_median_rejection(factor)
    assert g.launches_per_iteration() == (2 if fused else 4) + 2 + 1 + 2          # (tail; claim + resolve; the rule; select + apply)
    one_step(engine, g, F, M, T)
    icp_checks.check_projective_outputs(engine, g, res)
    gn = g.read(Mem.NN_ID)
    miss = gn["id"] == pref.NONE
    nn = pref.clipped(gn, miss)
    win, _, counts, W0 = icp_checks.unique_rule_of(engine, g, M, WEIGHTED, True, nn_id=nn)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W1 = np.where(win, W0, np.float32(0)).astype(np.float32)
    acc_m, words_m = median_rule(PF, PM, W1, factor)
    acc_t, words_t = trim_rule(PF, PM, np.where(acc_m, W1, np.float32(0)).astype(np.float32), keep)
    assert_words(engine, g, "UNIQUE", counts)
    assert_words(engine, g, "MEDIAN", words_m)
    assert_words(engine, g, "TRIM", words_t)
    assert words_m[1] == counts[1] and words_t[1] == words_m[3] and 0 < words_t[3] < words_m[3] < words_m[1], (counts, words_m, words_t)
    zero = ~acc_t
    W, sw, means, S, Tk = icp_checks.expected_pieces(oracle, F, M, T, nn, side, fused, WEIGHTED, POWER, fused, zero)
    gW = g.read(Mem.W)
    assert_bits(gW, W, "weights")
    assert np.count_nonzero(np.ascontiguousarray(gW[zero]).view(np.uint32)) == 0
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    icp_checks.assert_bits_nan(g.read(Mem.TK), Tk, "Tk")
    g.close()


# ---- 5. the plane metrics read the weights in their moments

@pytest.mark.parametrize("metric", ["point_to_plane", "symmetric"])
@pytest.mark.parametrize("side,nr", [(50, 4), (130, 4)])
def test_plane_metrics(engine, side, nr, metric):
    """One step: ICP_MEM_PLANE_SYSTEM, T, R, TK against the metric's float64 restatement fed the numpy rule's weights."""
    F, M, T, invalid, _, factor = _holes(side, nr)
    Mem = engine.Memory
    mu = 0.05
    g = icp_checks.make_plane(engine, side, nr, mu=mu, metric=P2PL, symmetric=True if metric == "symmetric" else None)
    g.set_rejection(True, None)
    g.set_median_rejection(factor)
    assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + (1 if side * side <= ONE_BLOCK_MAX else 4)     # (no apply pass)
    icp_checks.load(engine, g, F, M)
    g.buildRBC()
    g.write(Mem.T, T, block=True)
    T0, R0, k0 = icp_checks.before(engine, g)
    g.step()
    nn_id, PF, PM = g.read(Mem.NN_ID), g.read(Mem.NN), g.read(Mem.QT)
    W0 = weights_before_trim(nn_id, M, PF, PM, True, invalid)
    acc, words = median_rule(PF, PM, W0, factor)
    assert_words(engine, g, "MEDIAN", words)
    assert 0 < words[3] < words[1], words
    weights = np.where(acc, W0, np.float32(0)).astype(np.float32)
    assert_bits(PF[:, 3], weights, "weights")
    restate = icp_checks.restate_symmetric(mu) if metric == "symmetric" else icp_checks.restate_p2pl(mu)
    system = icp_checks.check_last(engine, g, restate, T0, R0, k0, weights=weights)
    assert system[27] == 1.0
    g.close()


# ---- 6. run and run_fixed equal steps; a new factor reaches a captured graph

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_run_equals_steps(engine, side, nr, fused, weighted):
    F, M, _, invalid, _, _ = _holes(side, nr)
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, fused, invalid, 2.0)
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    read = lambda: [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.MEDIAN).copy()]
    run = read()
    assert 0 < run[2][3] < run[2][1]
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    for a, b, what in zip(run, read(), ("T", "W", "MEDIAN")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    for factor in (2.0, 1.25):                          # (the second: a new factor in the graph captured with the first)
        g.set_median_rejection(factor)
        g.reset_transform(); g.buildRBC()
        g.run_fixed(5)
        fixed = read()
        g.reset_transform(); g.buildRBC()
        for _ in range(5):
            g.step()
        for a, b, what in zip(fixed, read(), ("T", "W", "MEDIAN")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, factor)
    assert 0 < fixed[2][3] < fixed[2][1]
    g.close()


# ---- 7. batches

@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch4(engine, oracle, fused):
    """Four registrations on one handle, each with its own n, t_med and thr; the last has every pair rejected in front of the rule (a
    moving frame of invalid points)."""
    from icp_amd import workloads as W
    side, nr, B = 50, 4, 4
    pairs = [icp_checks.holes_pair(engine, side, W.BASE_SEED + 5 * b) for b in range(B - 1)]
    pairs.append((pairs[0][0], np.zeros_like(pairs[0][1])))
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, 2.0, batch=B)
    step_batch(engine, g, pairs, T)
    seen = set()
    for b, (F, M) in enumerate(pairs[:B - 1]):
        acc, words = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, 2.0, b=b)
        assert 0 < words[3] < words[1], (b, words)
        seen.add(int(words[0]))
    assert len(seen) == B - 1, "the registrations' medians differ"
    # (n == 0: the sum W == 0 identity step, which the oracle's pieces do not state)
    Mem, b = engine.Memory, B - 1
    assert g.read(Mem.MEDIAN, batch_index=b).tolist() == [0, 0, 0, 0]
    assert np.all(g.read(Mem.W, batch_index=b) == 0.0) and g.read(Mem.SUM_W, batch_index=b)[0] == 0.0
    assert_bits(g.read(Mem.T, batch_index=b), T, "T of the registration without candidates")
    assert_bits(g.read(Mem.TK, batch_index=b), IDENTITY, "Tk of the registration without candidates")
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_a_converged_registration_keeps_its_words(engine, fused):
    """A checked run of three registrations, the first done at k = 1 (F against itself): each ends as the same pair alone does, the
    first with the words of its only iteration."""
    Mem = engine.Memory
    pairs = icp_checks.converged_pairs()
    side, nr = 128, 64
    read = lambda g, b: (g.state(b).k, g.read(Mem.T, b).copy(), g.read(Mem.W, b).copy(), g.read(Mem.MEDIAN, b).copy())
    alone = []
    for F, M in pairs:
        h = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, 2.0)
        icp_checks.load(engine, h, F, M)
        h.buildRBC()
        assert h.run() == h.state().k
        alone.append(read(h, 0))
        h.close()
    assert alone[0][0] == 1 and alone[1][0] >= 3 and alone[2][0] >= 3, [a[0] for a in alone]
    assert alone[0][3][0] == 0 and alone[0][3][2] == 0 and alone[0][3][3] > 0, alone[0][3]       # (every valid point finds itself)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, 2.0, batch=3)
    for b, (F, M) in enumerate(pairs):
        icp_checks.load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    for b in range(3):
        got = read(g, b)
        assert got[0] == alone[b][0], "k of registration %d: %d, alone %d" % (b, got[0], alone[b][0])
        for x, y, name in zip(got[1:], alone[b][1:], ("T", "W", "MEDIAN")):
            assert_bits(x, y, "%s of registration %d against the same pair alone" % (name, b))
    g.close()


def test_icp_batch_equals_single_handles(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [icp_checks.holes_pair(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    bt.set_median_rejection(2.0)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_rejection(True, None)
        g.set_median_rejection(2.0)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        words = g.read(engine.Memory.MEDIAN)
        assert np.array_equal(bt.read(i, engine.Memory.MEDIAN), words) and 0 < words[3] < words[1], (i, words)
        g.close()
    bt.close()


# ---- 8. off again

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_off_again_equals_never_on(engine, side, nr):
    """Factor 0 after the rule had been on (graphs cached with it): the same k, T, ids and weights as a handle that never had it, and
    ICP_MEM_MEDIAN reads zeros."""
    F, M, _, _, _, _ = _holes(side, nr)
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], nr, A, C_)
        g.set_rejection(True, None)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        if toggled:
            g.set_median_rejection(2.0)
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(engine.Memory.MEDIAN)[1] > 0
            g.set_median_rejection(0.0)
            assert g.median_rejection() == 0.0
            assert np.all(g.read(engine.Memory.MEDIAN) == 0)
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy(),
                    g.read(engine.Memory.W).view(np.uint32).copy()))
        assert np.all(g.read(engine.Memory.MEDIAN) == 0)
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


# ---- 9. form and launch count

def test_form_and_launch_count(engine):
    """With the rule on the iteration is the separate form: search, the rule (one launch up to 16384 pairs, four beyond), on
    point-to-point the apply pass, the tail; off again, the former form is back."""
    for side, nr, rule in ((128, 256, 1), (130, 4, 4)):
        g = engine.ICP(0)
        g.init(side * side, nr, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0, n0 = g.run_form(), g.launches_per_iteration()
        g.set_median_rejection(2.0)
        assert g.run_form() == 0
        tail = 3 if ((side * side + 63) // 64 + 127) // 128 > 2 else 2           # (the search and the fused tail)
        assert g.launches_per_iteration() == tail + rule + 1
        g.set_trimming(0.8)                                  # (the apply pass runs anyway: trimming adds its selection alone)
        assert g.launches_per_iteration() == tail + rule + 1 + (1 if rule == 1 else 3)
        g.set_trimming(1.0)
        g.set_normals(1, side)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + rule       # (the apply pass is absent)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT, 0.0)
        g.set_median_rejection(0.0)
        assert g.run_form() == form0 and g.launches_per_iteration() == n0
        g.close()


# ---- 10. the set of the last iteration

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_last_iteration_pairs_are_the_accepted(engine, oracle, side, nr):
    F, M, T, invalid, want, factor = _holes(side, nr)
    g = make_handle(engine, F.shape[0], nr, True, WEIGHTED, POWER, True, invalid, factor)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, True, WEIGHTED, POWER, True, invalid, factor, want)
    rec = g.correspondences(engine.Pairs.LAST_ITERATION)
    assert len(rec) == words[3] and np.array_equal(rec["moving"], np.nonzero(acc)[0])
    assert np.array_equal(rec["fixed"], want[0]["id"][acc])
    g.close()


# ---- 11. tracking is not provided

def test_tracking_is_refused_while_the_rule_is_on(engine):
    g = engine.ICP(0)
    g.init(16384, 256, A, C_)
    g.set_median_rejection(2.0)
    with pytest.raises(engine.ICPError) as e:
        g.track_next(engine.synth_cloud_vga())
    assert e.value.code == ESTATE
    g.set_median_rejection(0.0)
    assert g.track_next(engine.synth_cloud_vga()) is None
    assert g.track_next(engine.synth_cloud_vga(moved=1)) >= 1
    g.close()


# ---- 13. what it is for: partial overlap

@pytest.mark.parametrize("fused", [True, False])
def test_median_rejection_copes_with_partial_overlap(engine, fused):
    """icp_checks._partial_overlap: a quarter of the moving frame has no counterpart.  The rule off against the factors 1.5, 2 and 3;
    the best of them (by translation error) ends closer to T_true than the off run in rotation and in translation.
    Measured on an MI355X (fused; reference order differs at factor 2 alone: 0.134 deg / 4.16 mm): off 0.431 deg / 8.27 mm (k = 30),
    factor 1.5 0.158 deg / 3.12 mm (35), factor 2 0.136 deg / 4.08 mm (37), factor 3 0.136 deg / 3.72 mm (28): every factor ends
    closer than the off run, 1.5 closest in translation."""
    from icp_amd import workloads as W
    F, M, T_true = _partial_overlap(engine)
    res = {}
    for factor in (0.0, 1.5, 2.0, 3.0):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_median_rejection(factor)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        T = g.read(engine.Memory.T).copy()
        g.close()
        res[factor] = (W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])), k)
    for factor, (rot, t, k) in res.items():
        print("partial overlap %s: factor %.1f: %.3f deg %.2f mm (k = %d)" % ("fused" if fused else "reference order", factor, rot, t, k))
    best = min((1.5, 2.0, 3.0), key=lambda f: res[f][1])
    assert res[best][0] < res[0.0][0] and res[best][1] < res[0.0][1], res


# ---- pyramid levels take the rule through their handles

def test_pyramid_levels_take_the_rule(engine):
    """The rule set on the level handles of a two-level pyramid: every level's last iteration has the words of the numpy rule on that
    level's own outputs, and the coarse level's threshold is its own (the median scales with the level)."""
    Mem = engine.Memory
    F, M = icp_checks.holes_pair(engine, 128, 0x1C9D5EED)
    p = engine.ICPPyramid(0)
    p.init(128 * 128, (256, 64), A, C_)
    try:
        for l in range(p.levels):
            lv = p.level(l)
            lv.set_rejection(True, None)
            lv.set_median_rejection(2.0)
            assert lv.median_rejection() == 2.0 and lv.run_form() == 0
        p.write(Mem.F, F)
        p.write(Mem.M, M)
        p.buildRBC()
        p.run()
        p.sync()
        thr = []
        for l in range(p.levels):
            lv = p.level(l)
            nn_id, PF, PM, Ml = lv.read(Mem.NN_ID), lv.read(Mem.NN), lv.read(Mem.QT), lv.read(Mem.M)
            acc, words = median_rule(PF, PM, weights_before_trim(nn_id, Ml, PF, PM, True, True), 2.0)
            got = lv.read(Mem.MEDIAN)
            assert np.array_equal(got, words), (l, got, words)
            assert 0 < got[3] < got[1] <= (128 >> l) ** 2, (l, got)
            assert np.array_equal(lv.read(Mem.W) != 0, acc), l
            thr.append(int(got[2]))
        assert thr[0] != thr[1]
    finally:
        p.close()
