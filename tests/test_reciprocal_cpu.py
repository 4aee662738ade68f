"""Reciprocal correspondences without a device: the inverse transform of tests/reciprocal_ref.py against a float64 4 x 4 inverse, the
rule on hand-made arrays at its edges, the guard, and the counts the GPU tests pin — from the CPU oracle alone (the back search is the
oracle's search with F and M swapped and the inverse transform)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
