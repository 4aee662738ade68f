"""Reciprocal correspondences without a device: the inverse transform of tests/reciprocal_ref.py against a float64 4 x 4 inverse, the
rule on hand-made arrays at its edges, the guard, and the counts the GPU tests pin — from the CPU oracle alone (the back search is the
oracle's search with F and M swapped and the inverse transform)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks                                                # noqa: E402
import quality_ref                                               # noqa: E402
import reciprocal_ref as ref                                     # noqa: E402
from reciprocal_ref import EXACT, NEAR_20, rotation_T            # noqa: E402
from icp_checks import IDENTITY, _t0, oracle_search              # noqa: E402

F32 = np.float32

# the smallest non-exact gap of the small shapes, mm (rounded)
SMALLEST_GAP = {(6, 4): 183, (14, 4): 82, (16, 16): 62, (30, 4): 31}


def matrix_of(T):
    x, y, z, w, tx, ty, tz, s = (float(v) for v in T)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)
    A = np.eye(4)
    A[:3, :3] = s * R
    A[:3, 3] = (tx, ty, tz)
    return A


@pytest.mark.parametrize("T", [_t0(), IDENTITY, rotation_T(10.0, (0.2, -0.5, 0.8), (25.0, -40.0, 12.5), 1.02),
                               rotation_T(10.0, (1.0, 0.3, -0.4), (-7.0, 3.0, 90.0), 0.97), rotation_T(179.0, (0, 0, 1), (1e3, 2e3, -3e3), 2.5)])
def test_inverse_against_a_float64_matrix_inverse(T):
    Ti, ok = ref.inverse(T)
    assert ok and Ti.dtype == F32
    want = np.linalg.inv(matrix_of(T))
    got = matrix_of(Ti)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max()), (got, want)
    assert np.array_equal(Ti[:3].view(np.uint32), (-T[:3]).view(np.uint32)) and Ti[3] == T[3], "the three sign flips are exact"


@pytest.mark.parametrize("s", [0.0, -1.0, np.nan, np.inf, -np.inf])
def test_guard_rejects_everything(s):
    T = _t0().copy()
    T[7] = s
    Ti, ok = ref.inverse(T)
    assert not ok and np.array_equal(Ti, IDENTITY)
    ids = np.arange(8, dtype=np.uint32)
    exact, near, zero, counts = ref.reciprocal_rule(ids, ids, np.zeros((8, 4), F32), np.ones(8, F32), 50.0, ok)
    assert counts.tolist() == [8, 0, 0, 0] and zero.all() and not exact.any() and not near.any()


def test_guard_for_a_component_that_overflows():
    T = _t0().copy()
    T[7] = 1e-30
    T[4] = 1e30                                                   # t / s is beyond float
    Ti, ok = ref.inverse(T)
    assert not ok and np.array_equal(Ti, IDENTITY)


def test_rule_on_hand_made_arrays():
    """Six queries on four fixed points.  Queries 0 and 1 tie on j = 0, whose back search gives 1: 1 is exact, 0 is near or rejected by
    its gap to query 1.  Query 2's fixed point answers with an index past m.  Query 3's gap is NaN.  Query 4 has no weight: no
    candidate.  Query 5 is exact."""
    m = 6
    ids = np.array([0, 0, 1, 2, 3, 3], np.uint32)
    rev = np.array([1, m + 7, 4, 5, 0, 0], np.uint32)             # per fixed point; (entries 4, 5 are never looked up)
    QT = np.zeros((m, 4), F32)
    QT[0, :3] = (3.0, 4.0, 0.0)                                   # gap to query 1 (at the origin): exactly 5
    QT[3, 0] = np.nan
    QT[4, :3] = (1.0, 0.0, 0.0)
    W0 = np.array([1, 1, 1, 1, 0, 1], F32)
    exact, near, zero, counts = ref.reciprocal_rule(ids, rev, QT, W0, 0.0)
    assert np.flatnonzero(exact).tolist() == [1, 5] and not near.any() and counts.tolist() == [5, 2, 0, 2]
    assert np.flatnonzero(zero).tolist() == [0, 2, 3, 4]
    # max_gap exactly at the gap: <= accepts it; the float below does not
    exact, near, zero, counts = ref.reciprocal_rule(ids, rev, QT, W0, 5.0)
    assert np.flatnonzero(near).tolist() == [0] and counts.tolist() == [5, 2, 1, 3]
    exact, near, zero, counts = ref.reciprocal_rule(ids, rev, QT, W0, np.nextafter(F32(5.0), F32(0.0)))
    assert not near.any() and counts.tolist() == [5, 2, 0, 2]
    # i' >= m and the NaN gap stay rejected whatever the gap
    exact, near, zero, counts = ref.reciprocal_rule(ids, rev, QT, W0, 1e18)
    assert np.flatnonzero(near).tolist() == [0] and zero[2] and zero[3] and zero[4]
    # an id that is no index into F is no candidate
    ids2 = ids.copy(); ids2[5] = m
    assert ref.reciprocal_rule(ids2, rev, QT, W0, 0.0)[3].tolist() == [4, 1, 0, 1]


@pytest.mark.parametrize("side,nr", list(EXACT))
def test_pinned_counts_of_the_oracle(engine, oracle, side, nr):
    """synth_pair (side) at _t0 (), alpha = 200, T' in the rule's order: the counts tests/test_gpu_reciprocal.py asserts of the engine,
    from the oracle alone.  The same forward search gives the 5589 and 151 distinct fixed points tests/test_gpu_unique.py pins."""
    F, M = engine.synth_pair(side)
    T = _t0()
    fwd, _ = oracle_search(oracle, F, M, T, nr)
    (rev, _), ok = ref.back_search(oracle, F, M, T, nr)
    assert ok
    QT = oracle.transform_q(M, T)
    W0 = np.ones(side * side, F32)
    m = side * side
    _, _, zero, counts = ref.reciprocal_rule(fwd["id"], rev["id"], QT, W0, 0.0)
    assert counts.tolist() == [m, EXACT[side, nr], 0, EXACT[side, nr]] and np.count_nonzero(~zero) == EXACT[side, nr]
    _, _, _, counts = ref.reciprocal_rule(fwd["id"], rev["id"], QT, W0, 20.0)
    assert counts.tolist() == [m, EXACT[side, nr], NEAR_20[side, nr], EXACT[side, nr] + NEAR_20[side, nr]]
    if (side, nr) == (128, 256):
        assert counts.tolist() == [16384, 1367, 2111, 3478] and len(np.unique(fwd["id"])) == 5589
    if (side, nr) == (16, 16):
        assert len(np.unique(fwd["id"])) == 151
    g = ref.gaps(fwd["id"], rev["id"], QT, W0)
    if (side, nr) in SMALLEST_GAP:
        assert round(g[0]) == SMALLEST_GAP[side, nr] and g[0] > 20.0
        # the GPU test's choice for these shapes: the lower quartile of the non-exact gaps bites and leaves work
        gap = F32(np.quantile(g, 0.25))
        _, _, _, c = ref.reciprocal_rule(fwd["id"], rev["id"], QT, W0, gap)
        assert 0 < c[2] and c[3] < c[0]


# ---- the conditions tests/test_gpu_reciprocal.py relies on in every search layout, for a converged registration and at the rule's
# ---- edges, each from the oracle alone ------------------------------------------------------------------------------------------------

# (side, |R|, batch, zero) -> max_gap to three decimals, per registration ICP_MEM_RECIPROCAL's words and the size of the trimmed set,
# and the back answers that name an origin row of M
LAYOUT_RECIPROCAL = {
    (256, 256, 1, 0.0): (51.840, [([57671, 2725, 31878, 34603], 25953)], 0),
    (256, 512, 1, 0.1): (51.579, [([51925, 2522, 28633, 31155], 23367)], 6576),
    (128, 64, 3, 0.0): (51.756, [([14418, 1382, 7269, 8651], 6489), ([13335, 1144, 6401, 7545], 5659), ([12422, 1025, 5827, 6852], 5139)], 0),
    (64, 64, 9, 0.0): (54.201, [([3604, 651, 1511, 2162], 1622), ([3333, 578, 1338, 1916], 1437), ([3131, 479, 1240, 1719], 1290),
                                ([2936, 445, 1161, 1606], 1205), ([2759, 426, 1044, 1470], 1103), ([2604, 396, 958, 1354], 1016),
                                ([2485, 379, 914, 1293], 970), ([2373, 357, 902, 1259], 945), ([2263, 335, 841, 1176], 882)], 0),
    (256, 8192, 1, 0.0): (50.653, [([57671, 2294, 32309, 34603], 25953)], 0),
    (192, 2048, 1, "blobs30"): (55.619, [([22324, 1072, 12322, 13394], 10046)], 12072)}


@pytest.mark.parametrize("case", icp_checks.LAYOUT_CASES, ids=lambda c: "%d-%d-%d-%d-%s" % c[:5])
def test_layout_scenes_with_the_rule(engine, oracle, case):
    """icp_checks.layout_reciprocal: max_gap between 50.6 and 55.7 mm, accepted 60 % of registration 0's candidates, and the conditions
    the device test asserts again (icp_checks.layout_reciprocal_conditions).  In the two scenes with holes every invalid fixed point
    is a query of the back search, and its answer is one of M's thousands of coincident origin points: a tie only the search's
    tie-break decides."""
    side, nr, batch, fused, zero, _ = case
    sc, lr = icp_checks.layout_scene(side, nr, batch, zero), icp_checks.layout_reciprocal(side, nr, batch, zero)
    assert 50.6 <= lr.max_gap <= 55.7 and float(F32(lr.max_gap)) == lr.max_gap, lr.max_gap
    words = [r.words["RECIPROCAL"] for r in lr.rules]
    finals = [int(np.count_nonzero(r.W)) for r in lr.rules]
    counted = [int(np.count_nonzero(quality_ref.masks(M, pf, pm, 0.0)[0])) for (_, M), pf, pm in zip(sc.pairs, sc.PF, sc.PM)]
    origin = sum(int(np.count_nonzero(icp_checks.origin_rows(M)[back[0][0]["id"]])) for (_, M), back in zip(sc.pairs, lr.backs))
    holes = any(icp_checks.origin_rows(M).any() for _, M in sc.pairs)
    for (F, M), back, r, w in zip(sc.pairs, lr.backs, lr.rules, words):
        assert back[1] and back[0][0]["id"].shape[0] == F.shape[0] and (back[0][0]["id"] < M.shape[0]).all()
        assert r.words["TRIM"][1] == w[3] and r.words["TRIM"][3] == np.count_nonzero(r.W), "trimming's candidates are the pairs the rule accepts"
        if holes:                                                 # (every invalid fixed point's answer is an origin row of M)
            assert icp_checks.origin_rows(M)[back[0][0]["id"]][icp_checks.origin_rows(F)].all() and icp_checks.origin_rows(M).sum() > 1000
    assert abs(int(words[0][3]) - 0.6 * int(words[0][0])) <= 1.0, words[0]
    icp_checks.layout_reciprocal_conditions(words, finals, counted, origin / (batch * side * side) if holes else None, str(case[:5]))
    gap, rows, origin_want = LAYOUT_RECIPROCAL[(side, nr, batch, zero)]
    assert abs(lr.max_gap - gap) <= 1e-3 and origin == origin_want, (lr.max_gap, origin)
    assert [(w.tolist(), f) for w, f in zip(words, finals)] == rows, [(w.tolist(), f) for w, f in zip(words, finals)]


def test_a_registration_of_a_frame_with_itself_is_done_at_once(engine, oracle):
    """icp_checks.converged_pairs' registration 0 at the identity: every one of the 14742 valid points finds itself at distance 0 in
    both directions, the rule's words are [14742, 14742, 0, 14742], and the step's Tk is the identity — ICP::check stops at k = 1."""
    import p2pl_ref
    (F, M), _, _ = icp_checks.converged_pairs()
    s = icp_checks.route_scene("batch0")
    T = np.array(IDENTITY, F32)
    want = oracle_search(oracle, F, M, T, s.nr)
    (rev, _), ok = ref.back_search(oracle, F, M, T, s.nr)
    valid = ~icp_checks.origin_rows(F)
    rows = np.flatnonzero(valid)
    assert ok and len(rows) == 14742
    assert np.array_equal(want[0]["id"][valid], rows) and not want[0]["dist"][valid].any()
    assert np.array_equal(rev["id"][valid], rows) and not rev["dist"][valid].any()
    PF, PM = np.ascontiguousarray(F[want[0]["id"]]), oracle.transform_q(M, T)
    W0 = icp_checks.weights_before_trim(want[0], M, PF, PM, True, True, s.max_dist)
    _, _, zero, counts = ref.reciprocal_rule(want[0]["id"], rev["id"], PM, W0, s.max_gap, ok)
    assert counts.tolist() == [14742, 14742, 0, 14742] and np.array_equal(~zero, valid)
    for fused in (True, False):
        Tk = icp_checks.expected_pieces(oracle, F, M, T, want[0], s.side, fused, True, icp_checks.POWER, fused, zero)[4]
        # (the power method leaves 1e-24 in the quaternion's vector part: the identity to every threshold)
        assert np.allclose(Tk, IDENTITY, rtol=0, atol=1e-12) and p2pl_ref.check_converged(Tk, 0.001, 0.01), Tk


def test_a_max_gap_that_squares_to_a_pair_s_gap_exists(engine, oracle):
    """Scene 30 behind the search's rejection: 142 of the 269 distinct squared gaps (fp32) of the non-exact candidates are the float
    square of some float max_gap.  The median one belongs to one pair; at that max_gap the pair is near, at the next float below it
    is not, and nothing else changes."""
    s = icp_checks.route_scene("30")
    ids, rev = s.want[0]["id"], s.back[0][0]["id"]
    W0 = icp_checks.weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, s.max_dist)
    g2, gap, below, pairs, (distinct, have) = ref.equality_gap(ids, rev, s.PM, W0)
    assert (distinct, have) == (269, 142) and pairs >= 1
    assert F32(np.float64(F32(gap)) * np.float64(F32(gap))) == g2 and F32(np.float64(F32(below)) * np.float64(F32(below))) < g2
    assert float(F32(gap)) == gap and float(F32(below)) == below < gap
    at, under = ref.reciprocal_rule(ids, rev, s.PM, W0, gap), ref.reciprocal_rule(ids, rev, s.PM, W0, below)
    assert at[3][2] - under[3][2] == pairs and at[3][1] == under[3][1] and at[3][0] == under[3][0], (at[3], under[3])
    assert np.count_nonzero(at[1] & ~under[1]) == pairs and not (under[1] & ~at[1]).any() and 0 < under[3][2]


@pytest.mark.parametrize("side,nr", icp_checks.MESSY_SHAPES)
def test_non_finite_moving_rows_are_no_answer_of_the_back_search(engine, oracle, side, nr):
    s = icp_checks.messy_scene(side, nr)
    icp_checks.messy_conditions(s.finite, s.W0, s.back[0][0]["id"], s.rule[3], "the oracle, (%d, %d)" % (side, nr))
    assert s.back[1] and np.isfinite(s.back[0][0]["dist"]).all()
