"""Projective data association (icp_set_projective, include/icp_amd.h) restated in numpy — TEST INFRASTRUCTURE (a plain module: pytest
collects nothing from it).

The rule per query i at the transform T:
  e = oracle.transform_q (M, T)[i].xyz — the transformed point, the bits of the search's transform; the query counts iff M[i].xyz is
  finite and not (0, 0, 0);
  the pixel in float64 from the float32 inputs, every expression in the order written:
      u = fx * (e.x / e.z) + cx, v = fy * (e.y / e.z) + cy, pu = floor (u + 0.5), pv = floor (v + 0.5);
  inside iff it counts, e is finite, e.z > 0, 0 <= pu <= gw - 1 and 0 <= pv <= rows - 1 (a NaN fails every comparison);
  candidates: the cells j = y gw + x of the window [pu - r, pu + r] x [pv - r, pv + r] clipped to the grid whose F[j].xyz is finite and
  not (0, 0, 0); d_j = oracle.metric8 (e | M[i].rgb, F[j], alpha), one call per candidate;
  the winner: the smallest d_j < +inf, a tie to the smallest j — the minimum of (bits (d_j), j);
  hit: d = dist_scale * d_j in fp32, NN_ID = {d, j}, NN = (F[j].xyz, w), w = weighted ? 100 / (100 + d) : 1;
  miss (does not count, not inside, no winner): NN_ID = {+inf, 0xFFFFFFFF}, NN = (0, 0, 0, +0), W = +0; QT = (e, d) for every row.
Counts (ICP_MEM_PROJECTIVE): n = counting queries, hits, outside = counting and not inside, empty = inside without a winner.

project: the rule.  pieces: the oracle's pieces of the step (icp_checks.expected_pieces) fed the rule's pairs, the misses and the rows
whose fp32 geo is not finite zeroed.  scene / at: the pairs the tests use and the rule on them, computed once per session."""
import collections
import functools

import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
DIST_ID = np.dtype([("dist", np.float32), ("id", np.uint32)])

Result = collections.namedtuple("Result", "nn_id NN QT counts miss inside pu pv")
Result.__doc__ = """nn_id: m x {dist, id};  NN: m x 4 (matched fixed xyz, w);  QT: m x 4 (e, d);  counts: uint32 (n, hits, outside,
empty);  miss: the rows without a pair;  inside, pu, pv: the inside mask and the pixel (float64; meaningful where inside)."""

# The counts the tests pin, from the CPU oracle alone (tests/test_projective_cpu.py computes them again): synth_pair (side, zero_fraction)
# at icp_checks._t0 () with grid_intrinsics (side), alpha = 200.  (side, zero_fraction, r) -> (n, hits, outside, empty).
EXACT = {(128, 0.0, 0): (16384, 14416, 1968, 0), (128, 0.0, 1): (16384, 14416, 1968, 0),
         (128, 0.1, 0): (14767, 11689, 1775, 1303), (128, 0.1, 1): (14767, 12992, 1775, 0),
         (6, 0.0, 0): (36, 30, 6, 0), (14, 0.0, 0): (196, 168, 28, 0), (16, 0.0, 0): (256, 224, 32, 0), (30, 0.0, 0): (900, 792, 108, 0),
         (50, 0.0, 0): (2500, 2191, 309, 0)}
SMALL = [(6, 4), (14, 4), (16, 16), (30, 4), (50, 4)]                # (side, nr) of the smallest shapes


def intrinsics32(intr):
    """The four intrinsics as the float32 the setter stores, in float64."""
    return tuple(np.float64(F32(x)) for x in intr)


def pixel(E, intr):
    """(u, v, pu, pv) in float64 of the transformed points E [m][>= 3] (float32)."""
    fx, fy, cx, cy = intrinsics32(intr)
    E = np.asarray(E, F32)
    ex, ey, ez = (E[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        u = fx * (ex / ez) + cx
        v = fy * (ey / ez) + cy
        return u, v, np.floor(u + 0.5), np.floor(v + 0.5)


def valid_rows(X):
    """xyz finite and not (0, 0, 0)."""
    X = np.asarray(X, F32)
    return np.isfinite(X[:, :3]).all(axis=1) & ~(X[:, :3] == 0).all(axis=1)


def inside_mask(M, E, intr, gw):
    """(inside, pu, pv): the rule's test, in double."""
    rows = M.shape[0] // gw
    _, _, pu, pv = pixel(E, intr)
    E = np.asarray(E, F32)
    with np.errstate(all="ignore"):
        ins = (valid_rows(M) & np.isfinite(E[:, :3]).all(axis=1) & (E[:, 2].astype(np.float64) > 0.0)
               & (pu >= 0.0) & (pu <= gw - 1.0) & (pv >= 0.0) & (pv <= rows - 1.0))
    return ins, pu, pv


def project(oracle, F, M, T, gw, intr, r, weighted, alpha=2e2, dist_scale=1.0):
    F, M = np.ascontiguousarray(F, F32), np.ascontiguousarray(M, F32)
    m = M.shape[0]
    assert m % gw == 0
    rows = m // gw
    E = oracle.transform_q(M, np.asarray(T, F32))
    counting = valid_rows(M)
    ins, pu, pv = inside_mask(M, E, intr, gw)
    fvalid = valid_rows(F)
    nn_id = np.zeros(m, DIST_ID)
    nn_id["dist"] = np.inf
    nn_id["id"] = NONE
    NN = np.zeros((m, 4), F32)
    q = np.empty(8, F32)
    for i in np.flatnonzero(ins):
        x, y = int(pu[i]), int(pv[i])
        q[:3] = E[i, :3]; q[3] = 0.0; q[4:7] = M[i, 4:7]; q[7] = 0.0
        best = None
        ys, xs = np.arange(max(0, y - r), min(rows - 1, y + r) + 1), np.arange(max(0, x - r), min(gw - 1, x + r) + 1)
        js = (ys[:, None] * gw + xs[None, :]).ravel()
        js = js[fvalid[js]]
        if js.size > 9:
            # A large window: only the candidates that can win get the exact call.  The metric is a sum of non-negative terms (alpha
            # >= 0), so its fp32 value lies within a few 2^-24 of the float64 value of the same expression, relatively: a candidate
            # more than 1e-5 above the smallest float64 value cannot be the fp32 minimum.  Non-finite values take the exact call.
            with np.errstate(all="ignore"):
                g = F[js, :3].astype(np.float64) - q[:3].astype(np.float64)
                c = F[js, 4:7].astype(np.float64) - q[4:7].astype(np.float64)
                approx = (g * g).sum(axis=1) + float(alpha) * (c * c).sum(axis=1)
            fin = np.isfinite(approx)
            if fin.any():
                js = js[~fin | (approx <= approx[fin].min() * (1.0 + 1e-5))]
        for j in js:
            d = F32(oracle.metric8(q, F[j], alpha))
            if not d < np.inf:
                continue
            key = (int(d.view(np.uint32)), int(j))
            if best is None or key < best:
                best = key
        if best is not None:
            d = F32(F32(dist_scale) * np.uint32(best[0]).view(F32))
            nn_id[i] = (d, best[1])
            NN[i, :3] = F[best[1], :3]
    miss = nn_id["id"] == NONE
    with np.errstate(all="ignore"):
        W = (F32(100.0) / (F32(100.0) + nn_id["dist"])).astype(F32) if weighted else np.ones(m, F32)
    W[miss] = 0.0
    NN[:, 3] = W
    QT = np.concatenate([E[:, :3], nn_id["dist"][:, None]], axis=1).astype(F32)
    n, hits = int(np.count_nonzero(counting)), int(np.count_nonzero(~miss))
    outside = int(np.count_nonzero(counting & ~ins))
    counts = np.array([n, hits, outside, int(np.count_nonzero(ins & miss))], np.uint32)
    assert hits + outside + counts[3] == n
    return Result(nn_id, NN, QT, counts, miss, ins, pu, pv)


def reweighted(res, weighted):
    """The result with the weights of the other mode (the pairs do not depend on it)."""
    with np.errstate(all="ignore"):
        W = (F32(100.0) / (F32(100.0) + res.nn_id["dist"])).astype(F32) if weighted else np.ones(res.miss.shape[0], F32)
    W[res.miss] = 0.0
    NN = res.NN.copy()
    NN[:, 3] = W
    return res._replace(NN=NN)


def clipped(nn_id, miss):
    """A copy of nn_id that indexes F everywhere: a miss has id 0 and dist +inf."""
    nn = np.array(nn_id, DIST_ID)
    nn["id"][miss] = 0
    nn["dist"][miss] = np.inf
    return nn


def zero_rows(NN, QT, miss):
    """The rows that weigh nothing: the misses, and the rows whose fp32 geo is not finite (the apply pass accepts no such pair)."""
    import icp_checks
    with np.errstate(all="ignore"):
        return miss | ~np.isfinite(icp_checks.geo_of(NN, QT))


def pieces(oracle, res, F, M, T, side, fused, weighted, rot, power_fast, zero=None, weights=None):
    """(W, sum_w, means, S, Tk) of the step at T from the oracle's pieces fed the rule's pairs.  zero: further rows that weigh nothing."""
    import icp_checks
    z = zero_rows(res.NN, res.QT, res.miss)
    if zero is not None:
        z = z | zero
    return icp_checks.expected_pieces(oracle, F, M, T, clipped(res.nn_id, res.miss), side, fused, weighted, rot, power_fast, z, weights)


@functools.lru_cache(maxsize=None)
def scene(side, zero_fraction=0.0, seed=0x1C9D5EED):
    """(F, M, T) read-only: synth_pair (side, zero_fraction) at icp_checks._t0 ()."""
    import icp_amd as engine
    import icp_checks
    F, M = engine.synth_pair(side, seed=seed, zero_fraction=zero_fraction)
    T = icp_checks._t0()
    for a in (F, M, T):
        a.flags.writeable = False
    return F, M, T


@functools.lru_cache(maxsize=None)
def at(side, zero_fraction, r, seed=0x1C9D5EED):
    """The rule (WEIGHTED) on scene (side, zero_fraction) with the grid's own intrinsics and radius r, computed once."""
    import icp_amd as engine
    from oracle import oracle
    F, M, T = scene(side, zero_fraction, seed)
    res = project(oracle, F, M, T, side, engine.grid_intrinsics(side), r, True)
    for a in res:
        a.flags.writeable = False
    return res


@functools.lru_cache(maxsize=None)
def at_self(side, r):
    """The rule on scene (side)'s F against itself at the identity: every point lands on its own cell."""
    import icp_amd as engine
    import icp_checks
    from oracle import oracle
    F = scene(side, 0.0)[0]
    res = project(oracle, F, F, icp_checks.IDENTITY, side, engine.grid_intrinsics(side), r, True)
    for a in res:
        a.flags.writeable = False
    return res


RECT_GW, RECT_ROWS = 32, 8
RECT_INTRINSICS = (40.0, 40.0, 15.5, 3.5)


@functools.lru_cache(maxsize=None)
def rect_scene():
    """(F, M, T) read-only: a fixed set of 256 points read as a grid 32 wide and 8 high — cell (u, v) holds the point of a wavy surface
    about 1 m away that the pinhole model RECT_INTRINSICS projects to (u, v) —, and a moving set that is F moved by (40, 20, 0) mm (1.6
    cells across, 0.8 down), at icp_checks._t0 ().  icp_init reads the 256 points as a 16 x 16 set; the rule reads them 32 wide."""
    import icp_checks
    fx, fy, cx, cy = RECT_INTRINSICS
    v, u = np.meshgrid(np.arange(RECT_ROWS, dtype=np.float64), np.arange(RECT_GW, dtype=np.float64), indexing="ij")
    z = 1000.0 + 50.0 * np.sin(u / 5.0) + 30.0 * np.cos(v / 2.0)
    rng = np.random.default_rng(0x9EC7)
    F = np.zeros((RECT_GW * RECT_ROWS, 8), F32)
    F[:, 0], F[:, 1], F[:, 2] = ((u - cx) * z / fx).ravel(), ((v - cy) * z / fy).ravel(), z.ravel()
    F[:, 4:7] = rng.random((F.shape[0], 3), dtype=np.float32)
    M = F.copy()
    M[:, 0] += 40.0
    M[:, 1] += 20.0
    T = icp_checks._t0()
    for a in (F, M, T):
        a.flags.writeable = False
    return F, M, T


def scaled_T():
    """icp_checks._t0 () with s = 1.25."""
    import icp_checks
    T = icp_checks._t0().copy()
    T[7] = 1.25
    return T


def turned_T():
    """A half turn about y: every transformed point lies behind the fixed camera (e.z < 0), every query is outside."""
    return np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], F32)


@functools.lru_cache(maxsize=None)
def messy_pair(side):
    """(F, M) read-only: icp_checks.messy_grid as F and messy_moving's M — holes, NaN / +-inf coordinates and points at the origin on both sides."""
    import icp_amd as engine
    import icp_checks
    F = icp_checks.messy_grid(engine, side, 0x5EED + side)
    _, M, _ = icp_checks.messy_moving(engine, side, 0x5EED + side)
    for a in (F, M):
        a.flags.writeable = False
    return F, M


BATCH_SIDE = 30
BATCH = ((0x1C9D5EED, 0.0), (0xBA7C4, 0.1), (0xBA7C5, 0.0))          # (seed, zero_fraction) of the three pairs of the batched tests


def batch_pairs():
    """[(F, M)] of the three registrations."""
    return [scene(BATCH_SIDE, zf, seed)[:2] for seed, zf in BATCH]
