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
  the winner: the smallest d_j < +inf as floats compare (a negative alpha makes negative distances), a tie to the smallest j — the
  minimum of (d_j, j);
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
        if js.size > 9 and alpha >= 0:
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
            key = (d, int(j))                                    # (float32 compares: -0 and +0 tie)
            if best is None or key < best:
                best = key
        if best is not None:
            d = F32(F32(dist_scale) * best[0])
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


def batch_pairs(side=BATCH_SIDE):
    """[(F, M)] of the three registrations."""
    return [scene(side, zf, seed)[:2] for seed, zf in BATCH]


# ---- the kernel's own edges (tests/test_gpu_projective_edges.py; tests/test_projective_cpu.py proves what they rely on) -----------------

# Shapes above batch * m = 65536, where a block of the kernel serves 1024 queries in four rounds: (side, nr, registrations).
#   258: 66 blocks, the last with 4 live lanes in round 0 and three rounds wholly past m (257 is refused: m is odd);
#   3 x 150: 22 blocks per registration, the last with 996 queries (round 3 partly filled);
#   74 x 30 and 73 x 30: one block per registration (it draws the only ticket), round 3 with 132 live lanes.
FOUR_ROUNDS = [(258, 4, 1), (150, 4, 3), (30, 4, 74), (30, 4, 73)]
EXACT.update({(258, 0.1, 0): (59940, 47465, 7264, 5211), (258, 0.1, 1): (59940, 52676, 7264, 0)})


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def centre_grid(gw, rows, intr, z):
    """A clean F: every cell holds the float32 back-projection of its own centre at depth z; no colour."""
    fx, fy, cx, cy = intrinsics32(intr)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    F = np.zeros((gw * rows, 8), F32)
    F[:, 0], F[:, 1], F[:, 2] = ((u - cx) * z / fx).ravel(), ((v - cy) * z / fy).ravel(), z
    return F


EXACT_SIDE, EXACT_INTRINSICS, EXACT_Z = 8, (1.0, 1.0, 3.5, 3.5), 3.0


@functools.lru_cache(maxsize=None)
def exact_scene():
    """(F, M, T, pu, pv) read-only: an 8 x 8 centre_grid with intrinsics (1, 1, 3.5, 3.5) at z = 3, the identity, and moving points
    whose pixel sum u + 0.5 IS an integer: x = 3 (k - 4), k = 0 .. 8, gives x / 3 = k - 4 exactly — only under a correctly rounded
    division — and u + 0.5 = k; each with the float32 below it, which the rule sends to k - 1 (below 0 is a denormal that the sum with
    3.5 absorbs: k = 4); and x = -0.  Rows 0 .. 18 carry them in x (y the centre of grid row i % 8), rows 19 .. 37 in y, the rest are
    F's own points.  pu, pv: the pixel each row must get, by this reasoning and not by the restatement."""
    import icp_checks
    F = centre_grid(EXACT_SIDE, EXACT_SIDE, EXACT_INTRINSICS, EXACT_Z)
    M = F.copy()
    idx = np.arange(EXACT_SIDE * EXACT_SIDE)
    pu, pv = (idx % EXACT_SIDE).astype(np.float64), (idx // EXACT_SIDE).astype(np.float64)
    values = []
    for k in range(9):
        c = F32(3.0 * (k - 4))
        values += [(c, k), (np.nextafter(c, F32(-np.inf)), k if c == 0 else k - 1)]
    values.append((F32(-0.0), 4))
    i = 0
    for axis, want in ((0, pu), (1, pv)):
        for x, k in values:
            centre = i % EXACT_SIDE
            M[i, :3] = F[centre * EXACT_SIDE + centre, :3]               # (the centre of column and row i % 8)
            M[i, axis] = x
            pu[i] = pv[i] = centre
            want[i] = k
            i += 1
    return _frozen(F, M, icp_checks.IDENTITY.copy(), pu, pv)


STRADDLE_SIDE, STRADDLE_Z = 30, 913.0


def straddle_intrinsics():
    import icp_amd as engine
    return engine.grid_intrinsics(STRADDLE_SIDE)


@functools.lru_cache(maxsize=None)
def straddle_scene():
    """(F, M, T, pu, pv) read-only: a 30 x 30 centre_grid with the grid's own intrinsics at z = 913, the identity, and for every
    boundary k = 0 .. 30 of the rounding, in x (rows 0 .. 61) and in y (rows 62 .. 123), the two adjacent float32 coordinates that the
    float64 rule sends to k - 1 and to k; the other coordinate is the centre of cell i % 30, the rest are F's own points.  pu, pv: the
    pixel each row must get."""
    import icp_checks
    intr = straddle_intrinsics()
    f = intrinsics32(intr)
    z = np.float64(F32(STRADDLE_Z))
    F = centre_grid(STRADDLE_SIDE, STRADDLE_SIDE, intr, STRADDLE_Z)
    M = F.copy()
    idx = np.arange(STRADDLE_SIDE * STRADDLE_SIDE)
    pu, pv = (idx % STRADDLE_SIDE).astype(np.float64), (idx // STRADDLE_SIDE).astype(np.float64)
    down, up = F32(-np.inf), F32(np.inf)
    i = 0
    for axis, want in ((0, pu), (1, pv)):
        fa, ca = f[axis], f[2 + axis]

        def cell(x):
            return np.floor(fa * (np.float64(x) / z) + ca + 0.5)

        for k in range(STRADDLE_SIDE + 1):
            lo = F32((k - 0.5 - ca) * z / fa)
            while cell(lo) >= k:
                lo = np.nextafter(lo, down)
            while cell(np.nextafter(lo, up)) < k:
                lo = np.nextafter(lo, up)
            for x, kk in ((lo, k - 1), (np.nextafter(lo, up), k)):
                centre = i % STRADDLE_SIDE
                M[i, :3] = F[centre * STRADDLE_SIDE + centre, :3]
                M[i, axis] = x
                pu[i] = pv[i] = centre
                want[i] = kk
                i += 1
    return _frozen(F, M, icp_checks.IDENTITY.copy(), pu, pv)


def named_inside(pu, pv, gw, rows):
    """The inside mask of a constructed scene from the pixels its rows must get."""
    return (pu >= 0) & (pu <= gw - 1) & (pv >= 0) & (pv <= rows - 1)


EZ_SIDE = 6
EZ_ROWS = {"z -0": 0, "z +0": 1, "z denormal": 2, "behind": 3, "denormal on the axis": 4, "denormal x": 5, "only a denormal": 6,
           "u beyond float": 7, "plain": 8}


@functools.lru_cache(maxsize=None)
def ez_scene():
    """(F, M) read-only: scene (6)'s F, and F again as the moving set (at the identity every point lands on its own cell) with rows
    0 .. 8 replaced by the edge cases of e.z (EZ_ROWS):
      0, 1  on the camera plane, e.z = -0 and +0;  2  a denormal e.z in front of a finite e.x (u is about 1e43);  3  behind the camera;
      4  a denormal depth on the optical axis: it counts, and projects to (cx, cy): inside;
      5  a denormal x on an otherwise plain point: inside, the pixel of (0, 50, 1000);
      6  a point whose only non-zero coordinate is a denormal: not (0, 0, 0), so it counts; e.z = 0: outside;
      7  e.x = 3e38 over the smallest denormal e.z: u is 1e84, beyond float and finite in double: outside;
      8  (100, 50, 1000): inside."""
    F = scene(EZ_SIDE, 0.0)[0]
    M = F.copy()
    M[:9, :3] = (100.0, 50.0, 1000.0)
    M[0, 2], M[1, 2], M[2, 2], M[3, 2] = -0.0, 0.0, 1e-40, -1000.0
    M[4, :3] = (0.0, 0.0, 1e-40)
    M[5, 0] = 1e-40
    M[6, :3] = (1e-40, 0.0, 0.0)
    M[7, :3] = (3e38, 0.0, 1.4e-45)
    return _frozen(F, M)


def collapsed_T():
    """s = 0: every finite point is sent to the translation (6, -4, 1000), which is inside scene (6)'s grid."""
    return np.array([0.0, 0.0, 0.0, 1.0, 6.0, -4.0, 1000.0, 0.0], F32)


TIES_SIDE = 16
TIES_RADII = (1, 2, 8)
TIES_ANCHORS = {"same row": (4, 4), "lower row": (4, 11), "overflow": (11, 4), "nan colour": (11, 11)}
TIES_HUGE, TIES_NAN_QUERY = (8, 2), (8, 13)                        # the pixels near which the two queries without any winner are taken


@functools.lru_cache(maxsize=None)
def ties_scene():
    """(F, M, T, rows) read-only: scene (16) at icp_checks._t0 () with constructed candidates.  rows names the queries:
      "same row": F at the cells left and right of the query's pixel is the query itself (e, M.rgb) twice, bit for bit: d = 0 at both,
          the winner is the left one;
      "lower row": the same record at (x + 1, y) and at (x - 1, y + 1): the winner is the smaller j, which has the larger column;
      "overflow": the 3 x 3 cells around the pixel hold (3e38, 3e38, 3e38): valid points whose distance is +inf — at r = 1 an inside
          query with nine candidates and no winner;
      "nan colour": the 3 x 3 cells around the pixel have a NaN colour: every d_j there is NaN;
      "huge": the query's point scaled by 2^56: e is finite and inside, every distance overflows, at every radius;
      "nan query": the query's own colour is NaN: every d_j is NaN, at every radius."""
    from oracle import oracle
    F, M, T = (a.copy() for a in scene(TIES_SIDE, 0.0))
    E = oracle.transform_q(M, T)
    ins, pu, pv = inside_mask(M, E, _ties_intrinsics(), TIES_SIDE)
    taken, rows = set(), {}

    def near(x, y):
        cheb = np.maximum(np.abs(pu - x), np.abs(pv - y))
        cheb[~ins] = np.inf
        for i in taken:
            cheb[i] = np.inf
        i = int(np.argmin(cheb))
        assert cheb[i] <= 1, (x, y)
        taken.add(i)
        return i, int(pu[i]), int(pv[i])

    def record(i):
        rec = np.zeros(8, F32)
        rec[:3], rec[4:7] = E[i, :3], M[i, 4:7]
        return rec

    for name, (ax, ay) in TIES_ANCHORS.items():
        i, x, y = near(ax, ay)
        rows[name] = i
        if name == "same row":
            F[y * TIES_SIDE + x - 1] = F[y * TIES_SIDE + x + 1] = record(i)
        elif name == "lower row":
            F[y * TIES_SIDE + x + 1] = F[(y + 1) * TIES_SIDE + x - 1] = record(i)
        else:
            for yy in range(y - 1, y + 2):
                for xx in range(x - 1, x + 2):
                    if name == "overflow":
                        F[yy * TIES_SIDE + xx, :3] = 3e38
                    else:
                        F[yy * TIES_SIDE + xx, 4:7] = np.nan
    rows["huge"] = near(*TIES_HUGE)[0]
    M[rows["huge"], :3] *= F32(2.0 ** 56)
    rows["nan query"] = near(*TIES_NAN_QUERY)[0]
    M[rows["nan query"], 4:7] = np.nan
    _frozen(F, M, T)
    return F, M, T, rows


def _ties_intrinsics():
    import icp_amd as engine
    return engine.grid_intrinsics(TIES_SIDE)


METRIC_SCALE = 0.37                                                  # setMetricScale: no power of two
ALPHAS = (137.0, 1e5, float(np.nextafter(F32(0), F32(1))))           # setAlpha: near 200, one at which the colour picks the pairs, and the smallest positive one
METRIC_SCENES = ((30, 0.1, BATCH[1][0]), (50, 0.1, 0x1C9D5EED))      # (side, zero_fraction, seed), nr = 4


@functools.lru_cache(maxsize=None)
def at_metric(side, zero_fraction, seed, alpha, r=1):
    """The rule (WEIGHTED) on scene (side, zero_fraction, seed) with alpha and dist_scale = METRIC_SCALE, computed once."""
    import icp_amd as engine
    from oracle import oracle
    F, M, T = scene(side, zero_fraction, seed)
    res = project(oracle, F, M, T, side, engine.grid_intrinsics(side), r, True, alpha, METRIC_SCALE)
    for a in res:
        a.flags.writeable = False
    return res


def metric_max_dist(res):
    """A max_dist between the two readings of icp_set_rejection's distance test behind a scaled metric: the geometric mean of the 0.88
    quantiles of the hits' geometric distance (the rule's reading) and of their scaled distance d (the other one)."""
    import icp_checks
    hit = ~res.miss
    geo = icp_checks.geo_of(res.NN, res.QT)[hit].astype(np.float64)
    d = res.nn_id["dist"][hit].astype(np.float64)
    return float(F32(np.sqrt(np.sqrt(np.quantile(geo, 0.88) * np.quantile(d, 0.88)))))


def metric_rejected(res, max_dist, scaled=False):
    """The hits the distance test rejects: by the geometric distance (the rule), or — scaled — by d (the reading the rule excludes)."""
    import icp_checks
    d2 = F32(max_dist) * F32(max_dist)
    q = res.nn_id["dist"] if scaled else icp_checks.geo_of(res.NN, res.QT)
    with np.errstate(all="ignore"):
        return ~res.miss & ~(q <= d2)


# ---- pyramid levels (tests/test_gpu_pyramid.py) -------------------------------------------------------------------------------------------

PYRAMID_SIDE, PYRAMID_NR, PYRAMID_SEED = 128, (256, 64, 64), 7
PYRAMID_MEAN, PYRAMID_PICK = 0, 1


def pyramid_intrinsics(l, kind):
    """The intrinsics of level l of a PYRAMID_SIDE wide synth_pair grid by include/icp_amd.h: f / 2^l, and (c - (2^l - 1) / 2) / 2^l
    under ICP_PYRAMID_MEAN (icp_amd.register.level_intrinsics), c / 2^l under ICP_PYRAMID_PICK."""
    import icp_amd as engine
    from icp_amd import register
    intr = engine.grid_intrinsics(PYRAMID_SIDE)
    return register.level_intrinsics(intr, 1 << l) if kind == PYRAMID_MEAN else tuple(x / (1 << l) for x in intr)


PyramidLevel = collections.namedtuple("PyramidLevel", "side F M T intr res pieces T_next")


@functools.lru_cache(maxsize=None)
def pyramid_chain(kind, r=1):
    """[PyramidLevel] finest first: one projective iteration per level, coarsest first, on pyramid_ref.build's levels of the blobs30
    pair (contiguous holes in both frames), from the CPU alone.  T is what the level starts from — the identity at the coarsest level,
    T_next of the level above at a finer one (the hand-over is a write of T: R is re-derived from it) —, res the rule there, pieces the
    oracle's pieces fed its pairs (fused, the squared power start: a level's defaults), T_next = p2pl_ref.compose (T, R, Tk), the
    engine's composition with Rk from the quaternion."""
    import icp_amd as engine
    import icp_checks
    import p2pl_ref
    import pyramid_ref
    from oracle import oracle
    levels = len(PYRAMID_NR)
    F, M = icp_checks.holes_pair(engine, PYRAMID_SIDE, PYRAMID_SEED, "blobs30")
    Fs, Ms = pyramid_ref.build(F, PYRAMID_SIDE, levels, kind), pyramid_ref.build(M, PYRAMID_SIDE, levels, kind)
    T = icp_checks.IDENTITY.copy()
    out = [None] * levels
    for l in reversed(range(levels)):
        side, intr = PYRAMID_SIDE >> l, pyramid_intrinsics(l, kind)
        res = project(oracle, Fs[l], Ms[l], T, side, intr, r, True)
        pcs = pieces(oracle, res, Fs[l], Ms[l], T, side, True, 1, icp_checks.POWER, True)
        T_next = p2pl_ref.compose(T, oracle.quat_to_rot(T[:4]).ravel(), pcs[4])[0]
        out[l] = PyramidLevel(side, Fs[l], Ms[l], T, intr, res, pcs, T_next)
        _frozen(Fs[l], Ms[l], T, T_next, *res)
        T = T_next.copy()
    return out
