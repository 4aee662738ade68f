"""Reciprocal correspondences (icp_set_reciprocal, include/icp_amd.h) restated in numpy — TEST INFRASTRUCTURE (a plain module: pytest
collects nothing from it).

inverse (T): the inverse transform T' in the rule's order, in Python floats (doubles), no contraction.
back_search: the back search is the oracle's own search with F and M swapped and T' — icp_checks.oracle_search (oracle, M, F, T', nr).
reciprocal_rule: (exact, near, rows that weigh nothing, [n, exact, near, accepted]) from the forward ids, the back ids, the transformed
moving points, the weights before the rule and max_gap.
gaps / gaps2 / pick_gap: the gaps of the candidates that are not exact (their fp32 squares as the rule computes them), and a max_gap that
accepts a chosen share of the candidates.
equality_gap: a max_gap whose float square is exactly a pair's squared gap — the rule's <= at its edge."""
import math

import numpy as np

F32 = np.float32
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

# The counts the tests pin, from the CPU oracle alone (tests/test_reciprocal_cpu.py computes them again): synth_pair (side) at
# icp_checks._t0 (), alpha = 200.  (side, nr) -> exact pairs; -> near pairs at max_gap = 20.
EXACT = {(128, 256): 1367, (256, 1024): 2751, (6, 4): 18, (14, 4): 93, (16, 16): 109, (30, 4): 295}
NEAR_20 = {(128, 256): 2111, (256, 1024): 12812, (6, 4): 0, (14, 4): 0, (16, 16): 0, (30, 4): 0}


def rotation_T(deg, axis, t, s):
    """T = [q | t, s] of a rotation by deg degrees about axis."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = np.deg2rad(deg) / 2
    return np.array([*(np.sin(h) * a), np.cos(h), *t, s], F32)


def inverse(T):
    """(T' as 8 float32, ok).  ok False: s not finite or not > 0, or a component of T' not finite — T' is the identity and every
    candidate of the iteration is rejected."""
    x, y, z, w, tx, ty, tz = (float(F32(v)) for v in T[:7])
    s32 = F32(T[7])
    s = float(s32)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R00, R01, R02 = 1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)
    R10, R11, R12 = 2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)
    R20, R21, R22 = 2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)
    with np.errstate(all="ignore"):
        si = float(np.float64(1.0) / np.float64(s))          # (numpy: 1 / 0 is inf, not an exception)
        u0 = (R00 * tx + R10 * ty) + R20 * tz
        u1 = (R01 * tx + R11 * ty) + R21 * tz
        u2 = (R02 * tx + R12 * ty) + R22 * tz
        Ti = np.array([-F32(T[0]), -F32(T[1]), -F32(T[2]), F32(T[3]),
                       F32(np.float64(-(u0 * si))), F32(np.float64(-(u1 * si))), F32(np.float64(-(u2 * si))), F32(np.float64(si))], F32)
    ok = bool(math.isfinite(s) and s > 0.0 and np.isfinite(Ti).all())
    if not ok:
        Ti = np.array(IDENTITY, F32)
    return Ti, ok


def back_search(oracle, F, M, T, nr):
    """((nn_id, rid) of the back search — fixed-point order, ids into M —, ok) at the forward transform T."""
    import icp_checks
    Ti, ok = inverse(T)
    return icp_checks.oracle_search(oracle, M, F, Ti, nr), ok


def reciprocal_rule(ids, rev_ids, QT, W0, max_gap, ok=True):
    """ids: NN_ID.id per query; rev_ids: REVERSE_ID.id per fixed point; QT: the transformed moving points [m][>= 3]; W0: the weights
    before the rule; ok: inverse ()'s flag.  Candidates: W0 != 0 and id < m.  Returns (exact, near, zero, counts) — zero: the rows that
    weigh nothing behind the rule (no candidate with a weight, or a candidate the rule rejects)."""
    ids = np.asarray(ids, np.uint32)
    rev_ids = np.asarray(rev_ids, np.uint32)
    m = ids.shape[0]
    cand = (np.asarray(W0, F32) != 0) & (ids < m)
    i = np.arange(m, dtype=np.uint32)
    back = np.full(m, 0xFFFFFFFF, np.uint32)
    back[cand] = rev_ids[ids[cand]]
    exact = cand & (back == i) & ok
    near = np.zeros(m, bool)
    if ok and F32(max_gap) > 0:
        gap2 = F32(np.float64(F32(max_gap)) * np.float64(F32(max_gap)))
        rows = np.flatnonzero(cand & ~exact & (back < m))
        with np.errstate(all="ignore"):
            g = (np.asarray(QT, F32)[rows, :3] - np.asarray(QT, F32)[back[rows], :3]).astype(F32)
            gap = ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F32) + g[:, 2] * g[:, 2]).astype(F32)
            near[rows] = np.isfinite(gap) & (gap <= gap2)
    acc = exact | near
    counts = np.array([np.count_nonzero(cand), np.count_nonzero(exact), np.count_nonzero(near), np.count_nonzero(acc)], np.uint32)
    return exact, near, ~acc, counts


def gaps(ids, rev_ids, QT, W0):
    """The gaps (not squared, float64) of the candidates that are not exact and whose back id is a point of M, ascending."""
    ids = np.asarray(ids, np.uint32)
    m = ids.shape[0]
    cand = (np.asarray(W0, F32) != 0) & (ids < m)
    back = np.full(m, 0xFFFFFFFF, np.uint32)
    back[cand] = np.asarray(rev_ids, np.uint32)[ids[cand]]
    rows = np.flatnonzero(cand & (back != np.arange(m, dtype=np.uint32)) & (back < m))
    g = (np.asarray(QT, F32)[rows, :3] - np.asarray(QT, F32)[back[rows], :3]).astype(F32)
    gap = ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F32) + g[:, 2] * g[:, 2]).astype(F32)
    return np.sort(np.sqrt(gap[np.isfinite(gap)].astype(np.float64)))


def pick_gap(ids, rev_ids, QT, W0, keep=0.7):
    """A max_gap (a Python float that a float32 holds exactly) at which exact + near is about `keep` of the rule's candidates (the pairs
    W0 gives a weight): the quantile of the non-exact gaps that asks for keep * n - exact near pairs."""
    ids = np.asarray(ids, np.uint32)
    cand = (np.asarray(W0, F32) != 0) & (ids < ids.shape[0])
    n = int(np.count_nonzero(cand))
    exact = int(np.count_nonzero(cand & (np.asarray(rev_ids, np.uint32)[np.minimum(ids, ids.shape[0] - 1)] == np.arange(ids.shape[0]))))
    g = gaps(ids, rev_ids, QT, W0)
    q = (keep * n - exact) / len(g)
    assert 0.0 < q < 1.0, "no max_gap keeps %g of %d candidates: %d are exact, %d have a gap" % (keep, n, exact, len(g))
    return float(F32(np.quantile(g, q)))


def gaps2(ids, rev_ids, QT, W0):
    """The squared gaps in fp32, as the rule computes them, of the candidates that are not exact and whose back id is a point of M
    (unsorted; the non-finite ones included)."""
    ids = np.asarray(ids, np.uint32)
    m = ids.shape[0]
    cand = (np.asarray(W0, F32) != 0) & (ids < m)
    back = np.full(m, 0xFFFFFFFF, np.uint32)
    back[cand] = np.asarray(rev_ids, np.uint32)[ids[cand]]
    rows = np.flatnonzero(cand & (back != np.arange(m, dtype=np.uint32)) & (back < m))
    with np.errstate(all="ignore"):
        g = (np.asarray(QT, F32)[rows, :3] - np.asarray(QT, F32)[back[rows], :3]).astype(F32)
        return ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F32) + g[:, 2] * g[:, 2]).astype(F32)


def gap_with_square(g2):
    """The float32 max_gap with (float) ((double) max_gap * max_gap) == g2, or None when no float squares to g2."""
    r = F32(np.sqrt(np.float64(g2)))
    for c in (np.nextafter(r, F32(0)), r, np.nextafter(r, F32(np.inf))):
        if F32(np.float64(c) * np.float64(c)) == F32(g2):
            return F32(c)
    return None


def equality_gap(ids, rev_ids, QT, W0):
    """(g2, max_gap, the next float below max_gap, the number of pairs whose squared gap is g2): over the distinct finite squared gaps
    of the non-exact candidates that some float max_gap squares to exactly, the median one.  Also returns (distinct values, how many
    of them have such a float)."""
    g = gaps2(ids, rev_ids, QT, W0)
    values = np.unique(g[np.isfinite(g)])
    have = [(v, gap_with_square(v)) for v in values]
    have = [(v, c) for v, c in have if c is not None]
    v, c = have[len(have) // 2]
    return v, float(c), float(np.nextafter(c, F32(0))), int(np.count_nonzero(g == v)), (len(values), len(have))
