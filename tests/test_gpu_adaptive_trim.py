"""Adaptive trimming (icp_set_adaptive_trimming): every iteration chooses the kept fraction itself — the bin end of a table of 4096
thresholds that minimises (sum of the geo at or below it) / (their number)^q between the ranks r_lo and r_hi — and gives the pairs
above it the weight +0; the search is not touched.

The accepted set and the eight words come from numpy (tests/adaptive_trim_ref.py: the rule of include/icp_amd.h applied to the engine's
own NN / QT outputs), the reference values from the oracle's piecewise entries with the rejected rows zeroed, bit for bit.
ICP_MEM_TRIM holds (t, n, K, accepted), ICP_MEM_TRIM_ADAPTIVE (j*, r_lo, r_hi, candidate bins) of the last iteration.

The shapes: (6, 4) — 36 pairs, most threads of the one workgroup hold no key —, (50, 4) — 2500, no multiple of 1024 —, (128, 256) —
exactly 16384, the one-workgroup limit —, (130, 4) — 16900, the smallest multi-workgroup shape: nine workgroups, the last partly filled."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks      # noqa: E402
import robust_ref      # noqa: E402
import unique_ref      # noqa: E402
from adaptive_trim_ref import adaptive_trim_rule      # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, P2PL, POWER, REGULAR, WEIGHTED, assert_bits, assert_words, geo_of,  # noqa: E402
                        one_step, only_invalid, set_modes, step_batch, weights_before_trim, _partial_overlap, _t0)
from median_ref import median_rule, pick_factor      # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4
SHAPES = [(6, 4), (50, 4), (128, 256), (130, 4)]
EDGE_SHAPES = [(128, 256), (130, 4)]
LO, HI = 0.05, 0.95
RULE = (LO, HI, 3)


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, rule, batch=1, **options):
    g = icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid), **options)
    if rule:
        g.set_adaptive_trimming(*rule)
    return g


@functools.lru_cache(maxsize=None)
def _holes(side, nr):
    import icp_amd as engine
    from oracle import oracle
    return icp_checks.scene(engine, oracle, side, nr, "holes")       # F, M, T, invalid, want


def assert_rule_words(engine, g, words, b=0):
    assert_words(engine, g, "TRIM", words[:4], b)
    assert_words(engine, g, "TRIM_ADAPTIVE", words[4:], b)


def check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, rule, want=None, b=0):
    """ICP_MEM_TRIM and ICP_MEM_TRIM_ADAPTIVE against adaptive_trim_rule on the engine's own NN / QT, then the pieces.  Returns
    (accepted, the eight words)."""
    Mem = engine.Memory
    nn_id = icp_checks.correspondences(engine, g, want, b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    acc, words = adaptive_trim_rule(PF, PM, weights_before_trim(nn_id, M, PF, PM, weighted, invalid), *rule)
    print("side %d: words %s" % (side, words.tolist()))
    assert_rule_words(engine, g, words, b)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, ~acc, want, b)
    return acc, words


def assert_inside(side, words):
    """Beyond the smallest shape the winner lies strictly inside the admissible range, and the table offers a real choice."""
    if side > 6:
        assert words[5] < words[2] < words[6] and words[7] >= 60, words


# ---- the arguments, the getter and the exclusion with fixed trimming

def test_arguments_and_getter(engine):
    L = engine.lib()
    g = engine.ICP(0)
    nan = float("nan")
    assert g.adaptive_trimming() == (0.0, 0.0, 0)
    for lo, hi, q in ((0.05, 0.95, 1), (0.05, 0.95, 9), (0.0, 0.95, 3), (-0.1, 0.95, 3), (0.6, 0.5, 3), (0.05, 1.5, 3), (nan, 0.95, 3), (0.05, nan, 3)):
        assert L.icp_set_adaptive_trimming(g._h, lo, hi, q) == EINVAL, (lo, hi, q)
    assert L.icp_set_adaptive_trimming(None, 0.05, 0.95, 3) == EINVAL
    assert g.adaptive_trimming() == (0.0, 0.0, 0)
    g.set_adaptive_trimming(0.25, 0.75, 8)
    assert g.adaptive_trimming() == (0.25, 0.75, 8)
    g.init(256, 16, A, C_)                               # the setting survives icp_init
    assert g.adaptive_trimming() == (0.25, 0.75, 8)
    assert np.all(g.read(engine.Memory.TRIM) == 0) and np.all(g.read(engine.Memory.TRIM_ADAPTIVE) == 0)      # (no iteration yet)
    g.set_adaptive_trimming(1.0, 1.0, 2)
    assert g.adaptive_trimming() == (1.0, 1.0, 2)
    g.set_adaptive_trimming(nan, 7.0, 0)                 # (off: the fractions are ignored and read back as 0)
    assert g.adaptive_trimming() == (0.0, 0.0, 0)
    g.set_adaptive_trimming()
    assert g.adaptive_trimming() == (float(np.float32(0.05)), float(np.float32(0.95)), 4)
    g.close()


def test_fixed_and_adaptive_trimming_exclude_each_other(engine):
    L = engine.lib()
    g = engine.ICP(0)
    g.init(256, 16, A, C_)
    g.set_adaptive_trimming(*RULE)
    assert L.icp_set_trimming(g._h, 0.5) == ESTATE and g.trimming() == 1.0
    g.set_trimming(1.0)                                  # (always passes)
    assert g.adaptive_trimming()[2] == 3
    g.set_adaptive_trimming(LO, HI, 0)
    g.set_trimming(0.5)
    assert L.icp_set_adaptive_trimming(g._h, LO, HI, 3) == ESTATE and g.adaptive_trimming() == (0.0, 0.0, 0)
    g.set_adaptive_trimming(LO, HI, 0)                   # (off stays allowed)
    assert g.trimming() == 0.5
    g.set_trimming(1.0)
    g.set_adaptive_trimming(*RULE)
    assert g.adaptive_trimming()[2] == 3
    g.close()


# ---- one step at every shape, every mode

@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_one_step(engine, oracle, side, nr, fused, weighted, rot, power_fast):
    F, M, T, invalid, want = _holes(side, nr)
    g = make_handle(engine, side * side, nr, fused, weighted, rot, power_fast, invalid, RULE)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, RULE, want)
    assert 0 < words[2] <= words[1], words
    assert_inside(side, words)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_one_step_at_the_seventh_power(engine, oracle, side, nr, fused):
    F, M, T, invalid, want = _holes(side, nr)
    rule = (LO, HI, 7)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, invalid, rule)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, invalid, rule, want)
    assert 0 < words[2] <= words[1], words
    g.close()


# ---- the search is untouched

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_search_is_untouched(engine, side, nr):
    """At the same T the correspondences, distances and nearest representatives are those of a run with the rule off, bit for bit."""
    F, M, T, invalid, _ = _holes(side, nr)
    out = []
    for rule in (None, RULE):
        g = make_handle(engine, F.shape[0], nr, True, WEIGHTED, POWER, True, invalid, rule)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")


# ---- edges

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_nothing_left_is_the_identity_step(engine, side, nr, fused):
    """Every pair rejected in front of the rule (n == 0): the run stops after one identity step, T as it was, eight zero words."""
    F, M = engine.synth_pair(side)
    T0 = _t0()
    g = engine.ICP(0)
    g.init(side * side, nr, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    g.set_rejection(False, 1e-3)
    g.set_adaptive_trimming(*RULE)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0, block=True)
    assert g.run() == 1
    Mem = engine.Memory
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert np.all(g.read(Mem.TRIM) == 0) and np.all(g.read(Mem.TRIM_ADAPTIVE) == 0)
    assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W) == 0.0)
    g.close()


@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_ties_at_t_are_kept(engine, oracle, side, nr):
    """Integer coordinates moved by an integer translation (the scene of trimming's test_ties_at_t_are_kept): geo is an integer, many
    pairs share a value — a bin is kept whole, so every pair whose geo equals a kept pair's is kept."""
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
        g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, (0.25, 0.75, 2))
        one_step(engine, g, F, M, T)
        acc, words = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, (0.25, 0.75, 2))
        geo = geo_of(g.read(engine.Memory.NN), g.read(engine.Memory.QT))
        kept = np.unique(geo[acc])
        ties = np.isin(geo, kept)
        assert np.count_nonzero(ties) > 1000 and np.count_nonzero(geo == kept.max()) > 1, words
        assert np.all(g.read(engine.Memory.W)[ties] != 0.0), "every tie of a kept pair is kept"
        assert words[3] == words[2] == np.count_nonzero(acc)
        g.close()


# ---- composition: one-to-one and median-distance rejection in front

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_behind_one_to_one_and_median(engine, oracle, side, nr, fused, weighted):
    """ICP_MEM_MEDIAN's n is the winner count, ICP_MEM_TRIM's n median rejection's accepted count; the pieces against the three numpy
    rules applied in that order."""
    F, M, T, invalid, want = _holes(side, nr)
    Mem = engine.Memory
    nn_id = want[0]
    PF, PM = np.ascontiguousarray(F[nn_id["id"]][:, :4]), np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])
    W0 = weights_before_trim(nn_id, M, PF, PM, weighted, invalid)
    win, _, _ = unique_ref.unique_rule(nn_id["id"], PF, PM, W0)
    factor = pick_factor(geo_of(PF, PM)[win], 0.15)
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, fused, invalid, None, unique=True)
    g.set_median_rejection(factor)
    g.set_adaptive_trimming(*RULE)
    one_step(engine, g, F, M, T)
    win, _, counts, W0 = icp_checks.unique_rule_of(engine, g, M, weighted, invalid)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W1 = np.where(win, W0, np.float32(0)).astype(np.float32)
    acc_m, words_m = median_rule(PF, PM, W1, factor)
    acc_t, words_t = adaptive_trim_rule(PF, PM, np.where(acc_m, W1, np.float32(0)).astype(np.float32), *RULE)
    assert_words(engine, g, "UNIQUE", counts)
    assert_words(engine, g, "MEDIAN", words_m)
    assert_rule_words(engine, g, words_t)
    assert words_m[1] == counts[1] and words_t[1] == words_m[3] and 0 < words_t[3] <= words_m[3] < words_m[1], (counts, words_m, words_t)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, POWER, fused, ~acc_t, want)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_behind_projective_association(engine, oracle, fused):
    """One-to-one and the rule behind the projection (r = 1) in the search's place."""
    import projective_ref as pref
    Mem = engine.Memory
    side, nr, zf = 30, 4, 0.1
    seed = pref.BATCH[1][0]
    F, M, T = pref.scene(side, zf, seed)
    res = pref.at(side, zf, 1, seed)
    g = icp_checks.projective_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 1, unique=True)
    g.set_adaptive_trimming(*RULE)
    assert g.launches_per_iteration() == (2 if fused else 4) + 2 + 2          # (projection and tail; claim + resolve; selection + apply)
    one_step(engine, g, F, M, T)
    icp_checks.check_projective_outputs(engine, g, res)
    gn = g.read(Mem.NN_ID)
    miss = gn["id"] == pref.NONE
    nn = pref.clipped(gn, miss)
    win, _, counts, W0 = icp_checks.unique_rule_of(engine, g, M, WEIGHTED, True, nn_id=nn)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W1 = np.where(win, W0, np.float32(0)).astype(np.float32)
    acc_t, words_t = adaptive_trim_rule(PF, PM, W1, *RULE)
    assert_words(engine, g, "UNIQUE", counts)
    assert_rule_words(engine, g, words_t)
    assert words_t[1] == counts[1] and 0 < words_t[3] <= words_t[1], (counts, words_t)
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


# ---- the plane metrics read the weights the apply pass leaves in their moments

@pytest.mark.parametrize("metric", ["point_to_plane", "symmetric"])
@pytest.mark.parametrize("side,nr", [(50, 4), (130, 4)])
def test_plane_metrics(engine, side, nr, metric):
    """One step: ICP_MEM_PLANE_SYSTEM, T, R, TK against the metric's float64 restatement fed the numpy rule's weights.  The iteration is
    trimming's under a plane metric: the search, the selection, the pass that zeroes the weights, the two launches of the plane tail."""
    F, M, T, invalid, _ = _holes(side, nr)
    Mem = engine.Memory
    mu = 0.05
    g = icp_checks.make_plane(engine, side, nr, mu=mu, metric=P2PL, symmetric=True if metric == "symmetric" else None)
    g.set_rejection(True, None)
    g.set_adaptive_trimming(*RULE)
    assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + 1 + 1
    icp_checks.load(engine, g, F, M)
    g.buildRBC()
    g.write(Mem.T, T, block=True)
    T0, R0, k0 = icp_checks.before(engine, g)
    g.step()
    nn_id, PF, PM = g.read(Mem.NN_ID), g.read(Mem.NN), g.read(Mem.QT)
    W0 = weights_before_trim(nn_id, M, PF, PM, True, invalid)
    acc, words = adaptive_trim_rule(PF, PM, W0, *RULE)
    assert_rule_words(engine, g, words)
    assert_inside(side, words)
    weights = np.where(acc, W0, np.float32(0)).astype(np.float32)
    assert_bits(PF[:, 3], weights, "weights")
    restate = icp_checks.restate_symmetric(mu) if metric == "symmetric" else icp_checks.restate_p2pl(mu)
    system = icp_checks.check_last(engine, g, restate, T0, R0, k0, weights=weights)
    assert system[27] == 1.0
    g.close()


# ---- the robust loss behind the rule

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", [(50, 4), (130, 4)])
def test_the_robust_loss_behind_the_rule(engine, oracle, side, nr, fused):
    """Cauchy at 12 mm on point-to-point: the loss weighs the pairs the rule accepts, W' = W omega, and the pieces are fed W'."""
    F, M, T, invalid, want = _holes(side, nr)
    Mem = engine.Memory
    loss, scale = robust_ref.CAUCHY, 12.0
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, invalid, RULE, robust_loss=(loss, scale))
    assert g.launches_per_iteration() == (2 if fused else 4) + (1 if fused and ((side * side + 63) // 64 + 127) // 128 > 2 else 0) + 2
    one_step(engine, g, F, M, T)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W0 = weights_before_trim(want[0], M, PF, PM, True, invalid)
    acc, words = adaptive_trim_rule(PF, PM, W0, *RULE)
    assert_rule_words(engine, g, words)
    W = robust_ref.p2p_weights(np.where(acc, W0, np.float32(0)).astype(np.float32), PF, PM, loss, scale)
    icp_checks.check_pieces(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, W == 0, want, 0, W)
    g.close()


# ---- run and run_fixed equal steps; new parameters reach a captured graph

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_run_equals_steps(engine, side, nr, fused, weighted):
    F, M, _, invalid, _ = _holes(side, nr)
    Mem = engine.Memory
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, fused, invalid, RULE)
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    read = lambda: [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.TRIM).copy(), g.read(Mem.TRIM_ADAPTIVE).copy()]
    names = ("T", "W", "TRIM", "TRIM_ADAPTIVE")
    run = read()
    assert 0 < run[2][3] <= run[2][1]
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    for a, b, what in zip(run, read(), names):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    seen = []
    for rule in (RULE, (0.5, 0.8, 5)):                   # (the second: new fractions and a new power in the graph captured with the first)
        g.set_adaptive_trimming(*rule)
        g.reset_transform(); g.buildRBC()
        g.run_fixed(5)
        fixed = read()
        g.reset_transform(); g.buildRBC()
        for _ in range(5):
            g.step()
        for a, b, what in zip(fixed, read(), names):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, rule)
        n = int(fixed[2][1])
        assert fixed[3][1] == min(int(np.ceil(float(np.float32(rule[0])) * n)), n) and fixed[3][1] <= fixed[2][2], (rule, fixed[2], fixed[3])
        seen.append(fixed[3].tolist())
    assert seen[0] != seen[1]
    g.close()


# ---- batches

@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch4(engine, oracle, fused):
    """Four registrations on one handle, each with its own words; the last has every pair rejected in front of the rule (a moving
    frame of invalid points)."""
    from icp_amd import workloads as W
    side, nr, B = 50, 4, 4
    pairs = [icp_checks.holes_pair(engine, side, W.BASE_SEED + 5 * b) for b in range(B - 1)]
    pairs.append((pairs[0][0], np.zeros_like(pairs[0][1])))
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, RULE, batch=B)
    step_batch(engine, g, pairs, T)
    seen = set()
    for b, (F, M) in enumerate(pairs[:B - 1]):
        acc, words = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, RULE, b=b)
        assert 0 < words[3] <= words[1], (b, words)
        seen.add(tuple(words.tolist()))
    assert len(seen) == B - 1, "the registrations' words differ"
    # (n == 0: the sum W == 0 identity step, which the oracle's pieces do not state)
    Mem, b = engine.Memory, B - 1
    assert g.read(Mem.TRIM, batch_index=b).tolist() == [0, 0, 0, 0] and g.read(Mem.TRIM_ADAPTIVE, batch_index=b).tolist() == [0, 0, 0, 0]
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
    read = lambda g, b: (g.state(b).k, g.read(Mem.T, b).copy(), g.read(Mem.W, b).copy(), g.read(Mem.TRIM, b).copy(), g.read(Mem.TRIM_ADAPTIVE, b).copy())
    alone = []
    for F, M in pairs:
        h = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, RULE)
        icp_checks.load(engine, h, F, M)
        h.buildRBC()
        assert h.run() == h.state().k
        alone.append(read(h, 0))
        h.close()
    assert alone[0][0] == 1 and alone[1][0] >= 3 and alone[2][0] >= 3, [a[0] for a in alone]
    assert alone[0][3][1] > 0 and alone[0][4][0] == 0, (alone[0][3], alone[0][4])       # (every valid point finds itself: geo 0, bin 0)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, RULE, batch=3)
    for b, (F, M) in enumerate(pairs):
        icp_checks.load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    for b in range(3):
        got = read(g, b)
        assert got[0] == alone[b][0], "k of registration %d: %d, alone %d" % (b, got[0], alone[b][0])
        for x, y, name in zip(got[1:], alone[b][1:], ("T", "W", "TRIM", "TRIM_ADAPTIVE")):
            assert_bits(x, y, "%s of registration %d against the same pair alone" % (name, b))
    g.close()


def test_icp_batch_equals_single_handles(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 4
    m = side * side
    Mem = engine.Memory
    pairs = [icp_checks.holes_pair(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    bt.set_adaptive_trimming(*RULE)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, Mem.F, F); bt.write(i, Mem.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_rejection(True, None)
        g.set_adaptive_trimming(*RULE)
        g.write(Mem.F, F); g.write(Mem.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, Mem.T), g.read(Mem.T), "T of registration %d" % i)
        words = g.read(Mem.TRIM)
        assert np.array_equal(bt.read(i, Mem.TRIM), words) and 0 < words[3] <= words[1], (i, words)
        assert np.array_equal(bt.read(i, Mem.TRIM_ADAPTIVE), g.read(Mem.TRIM_ADAPTIVE)), i
        g.close()
    bt.close()


# ---- off again

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_off_again_equals_never_on(engine, side, nr):
    """Power 0 after the rule had been on (graphs cached with it): the same k, T, ids and weights as a handle that never had it, the
    same form and launch count, and both memory objects read zeros."""
    F, M, _, _, _ = _holes(side, nr)
    Mem = engine.Memory
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], nr, A, C_)
        g.set_rejection(True, None)
        g.write(Mem.F, F); g.write(Mem.M, M)
        if toggled:
            g.set_adaptive_trimming(*RULE)
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(Mem.TRIM)[1] > 0 and g.read(Mem.TRIM_ADAPTIVE)[3] > 0
            g.set_adaptive_trimming(LO, HI, 0)
            assert g.adaptive_trimming() == (0.0, 0.0, 0)
            assert np.all(g.read(Mem.TRIM) == 0) and np.all(g.read(Mem.TRIM_ADAPTIVE) == 0)
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(Mem.T).view(np.uint32).copy(), g.read(Mem.NN_ID)["id"].copy(), g.read(Mem.W).view(np.uint32).copy(),
                    np.array([g.run_form(), g.launches_per_iteration()])))
        assert np.all(g.read(Mem.TRIM) == 0) and np.all(g.read(Mem.TRIM_ADAPTIVE) == 0)
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


# ---- form and launch count

def test_form_and_launch_count(engine):
    """With the rule on the iteration is the separate form: the search, one selection launch at either size, the apply pass, the tail;
    off again, the former form is back."""
    for side, nr in ((128, 256), (130, 4)):
        g = engine.ICP(0)
        g.init(side * side, nr, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0, n0 = g.run_form(), g.launches_per_iteration()
        g.set_adaptive_trimming(*RULE)
        assert g.run_form() == 0
        tail = 3 if ((side * side + 63) // 64 + 127) // 128 > 2 else 2           # (the search and the fused tail)
        assert g.launches_per_iteration() == tail + 1 + 1
        g.set_median_rejection(2.0)                          # (the apply pass runs anyway: the median adds its own launches alone)
        assert g.launches_per_iteration() == tail + 1 + 1 + (1 if side * side <= 16384 else 4)
        g.set_median_rejection(0.0)
        g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
        assert g.run_form() == 0 and g.launches_per_iteration() == 4 + 1 + 1
        g.setReduceMode(engine.ReduceMode.FUSED)
        g.set_normals(1, side)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + 1 + 1       # (as for trimming under a plane metric)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT, 0.0)
        g.set_adaptive_trimming(LO, HI, 0)
        assert g.run_form() == form0 and g.launches_per_iteration() == n0
        g.close()


# ---- the set of the last iteration

@pytest.mark.parametrize("side,nr", EDGE_SHAPES)
def test_last_iteration_pairs_are_the_accepted(engine, oracle, side, nr):
    F, M, T, invalid, want = _holes(side, nr)
    g = make_handle(engine, F.shape[0], nr, True, WEIGHTED, POWER, True, invalid, RULE)
    one_step(engine, g, F, M, T)
    acc, words = check_step(engine, oracle, g, F, M, T, side, True, WEIGHTED, POWER, True, invalid, RULE, want)
    rec = g.correspondences(engine.Pairs.LAST_ITERATION)
    assert len(rec) == words[3] and np.array_equal(rec["moving"], np.nonzero(acc)[0])
    assert np.array_equal(rec["fixed"], want[0]["id"][acc])
    g.close()


# ---- tracking is not provided

def test_tracking_is_refused_while_the_rule_is_on(engine):
    g = engine.ICP(0)
    g.init(16384, 256, A, C_)
    g.set_adaptive_trimming(*RULE)
    with pytest.raises(engine.ICPError) as e:
        g.track_next(engine.synth_cloud_vga())
    assert e.value.code == ESTATE
    g.set_adaptive_trimming(LO, HI, 0)
    assert g.track_next(engine.synth_cloud_vga()) is None
    assert g.track_next(engine.synth_cloud_vga(moved=1)) >= 1
    g.close()


# ---- what it is for: partial overlap

@pytest.mark.parametrize("fused", [True, False])
def test_adaptive_trimming_copes_with_partial_overlap(engine, fused):
    """icp_checks._partial_overlap: a quarter of the moving frame has no counterpart, and the rule is told no fraction (0.05 .. 0.95).
    The rule off against q = 3, 4 and 7; the best of them (by translation error) ends closer to T_true than the off run in rotation and
    in translation, and its last K / n lies in [0.6, 0.9] (the true overlap is 0.75).
    Measured on an MI355X (fused; reference order alike but q = 7: 4.08 mm, k = 27): off 0.431 deg / 8.27 mm (k = 30), q = 3
    0.174 deg / 2.84 mm (32) keeping 0.672, q = 4 0.141 deg / 3.92 mm (26) keeping 0.737, q = 7 0.131 deg / 4.07 mm (28) keeping 0.766:
    every power ends closer than the off run, q = 3 closest in translation; fixed trimming at 0.75 ends 0.135 deg / 4.14 mm."""
    from icp_amd import workloads as W
    F, M, T_true = _partial_overlap(engine)
    res = {}
    for q in (0, 3, 4, 7):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_adaptive_trimming(LO, HI, q)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        T = g.read(engine.Memory.T).copy()
        words = g.read(engine.Memory.TRIM).copy()
        g.close()
        res[q] = (W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])), k,
                  float(words[2]) / float(words[1]) if words[1] else 0.0)
    for q, (rot, t, k, kept) in res.items():
        print("partial overlap %s: q %d: %.3f deg %.2f mm (k = %d), kept %.3f" % ("fused" if fused else "reference order", q, rot, t, k, kept))
    best = min((3, 4, 7), key=lambda q: res[q][1])
    assert res[best][0] < res[0][0] and res[best][1] < res[0][1], res
    assert 0.6 <= res[best][3] <= 0.9, res


# ---- pyramid levels take the rule through their handles

def test_pyramid_levels_take_the_rule(engine):
    """The rule set on the level handles of a two-level pyramid: every level's last iteration has the words of the numpy rule on that
    level's own outputs."""
    Mem = engine.Memory
    F, M = icp_checks.holes_pair(engine, 128, 0x1C9D5EED)
    p = engine.ICPPyramid(0)
    p.init(128 * 128, (256, 64), A, C_)
    try:
        for l in range(p.levels):
            lv = p.level(l)
            lv.set_rejection(True, None)
            lv.set_adaptive_trimming(*RULE)
            assert lv.adaptive_trimming()[2] == 3 and lv.run_form() == 0
        p.write(Mem.F, F)
        p.write(Mem.M, M)
        p.buildRBC()
        p.run()
        p.sync()
        ts = []
        for l in range(p.levels):
            lv = p.level(l)
            nn_id, PF, PM, Ml = lv.read(Mem.NN_ID), lv.read(Mem.NN), lv.read(Mem.QT), lv.read(Mem.M)
            acc, words = adaptive_trim_rule(PF, PM, weights_before_trim(nn_id, Ml, PF, PM, True, True), *RULE)
            got = np.concatenate([lv.read(Mem.TRIM), lv.read(Mem.TRIM_ADAPTIVE)])
            assert np.array_equal(got, words), (l, got, words)
            assert 0 < got[3] <= got[1] <= (128 >> l) ** 2, (l, got)
            assert np.array_equal(lv.read(Mem.W) != 0, acc), l
            ts.append(int(got[1]))
        assert ts[0] != ts[1]
    finally:
        p.close()
