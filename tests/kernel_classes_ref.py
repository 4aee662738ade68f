"""Plain numpy references, inputs and comparisons for the per-kernel classes (ICPLMs, ICPReps, ICPWeights, ICPMean<>, ICPDevs,
ICPS<>) and the cloud transforms.  No oracle and no engine in here: test_kernel_classes_cpu.py holds the oracle's twins against
this module, test_gpu_kernel_classes.py the engine against the oracle and against this module.

Two kinds of reference:
  * EXACT float32 rules, where every output is one correctly rounded IEEE operation (or a copy) and so has one possible value:
    the weights, the deviations, the landmark slice, the representatives' source index.
  * FLOAT64 restatements of what an operation means, with no tree and no padding: the sum of the weights, the means, the eleven
    S terms, the three transforms.

Comparing bits: copies (landmarks, representatives, lanes 3..7 of a transformed point) are compared as raw uint32, NaN payloads
included.  Results of arithmetic are compared as raw bits too, except that two NaNs are equal whatever their sign and payload:
IEEE 754 leaves both open for a NaN an operation generates (inf - inf is 0xffc00000 on x86 and 0x7fc00000 on a GPU)."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)          # 2^-23
TOL = 8 * EPS                                  # weights, their sum, the means and S against float64, each in its own norm
F_RANGE, M_RANGE = 10000.0, 255.0              # the reference tests' input ranges of the mean (U[0, 10000), U[0, 255))

DIST_ID = np.dtype([("dist", np.float32), ("id", np.uint32)])

# the transforms against float64, in EPS of |s| |q|^2 |p| + |t| (quaternion kinds) or of sum_k |T_rk p_k| (matrix kind): four times the
# oracle's worst error over every finite case of test_kernel_classes_cpu.py (1.977, 1.714 and 1.385)
TRANSFORM_TOL = {"q": 7.9, "q2": 6.9, "m": 5.5}

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# weights and means (n even): one group of 128 with one pair / full / just above; 2 or 3 groups padded to 4; 4 and 5 (padded to
# 8) groups; 16 groups; a second mean level of 128, then 129 groups (two groups at the third); 512 partials in one chunk of the
# double sum, then 513 (padded to 516) in two
N_EVEN = (2, 4, 6, 126, 128, 130, 254, 256, 258, 384, 386, 510, 512, 514, 640, 642, 2046, 2048, 2050, 16382, 16384, 16386, 65536, 65538)
N_DEVS = (1, 2, 3, 255, 256, 257, 1000)
# S: G = ceil (m / 4) below 4 and every m % 4; 511, 512 and 513 columns; two levels; two levels with a padded count and m % 4 = 1
M_S = (1, 2, 3, 4, 5, 7, 8, 13, 16, 17, 2044, 2047, 2048, 2049, 2052, 2053, 8191, 8192, 8193, 16384, 70001)
S_SCALINGS = [(m, c) for m in (13, 8193) for c in (1e-6, 1.0, 0.0)]
N_PADDED = (130, 642)                          # weights / means: sizes whose last group is ragged and whose group count is padded
M_PADDED = (13, 2049)                          # S: likewise
REPS_CASES = ((1, 1), (2, 1), (2, 2), (2, 4), (6, 4), (8, 2), (8, 8), (8, 32), (8, 64), (16, 128), (20, 16), (128, 1), (128, 16384))
# the transforms, in this order on one handle: the cloud buffer grows, is reused smaller, then reused at full size with new data
TRANSFORM_N = (1, 257, 2, 307200, 255, 256, 511, 513, 1000, 307200)
TRANSFORM_CLOUD_SEEDS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 1)

DENORM_MIN = float(np.float32(1e-45))
WEIGHT_EDGES = (0.0, -0.0, DENORM_MIN, 1e30, 3.4e38, float(np.finfo(np.float32).max), np.inf, -np.inf, np.nan, -100.0, -50.0)
WEIGHT_EDGE_POS = (0, 127, 129)                # first of the first group, last of the first group, the last point (third group)


# ---- comparing bits -------------------------------------------------------------------------------------------------------------
def _raw(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_raw_bits(got, want, what=""):
    """Copies: every bit, NaN payloads included."""
    g, w = _raw(got), _raw(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d elements differ, first at %d: %#x, expected %#x" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


def assert_bits(got, want, what=""):
    """Arithmetic: every bit, but any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    g, w = _raw(got), _raw(want)
    assert g.shape == w.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, g.shape, w.shape)
    bad = np.flatnonzero((g != w) & ~(np.isnan(got.reshape(-1)) & np.isnan(want.reshape(-1))))
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r (%#x), expected %r (%#x)" % (
        what, bad.size, bad[0], got.reshape(-1)[bad[0]], g[bad[0]], want.reshape(-1)[bad[0]], w[bad[0]])


# ---- inputs (the reference tests' ranges, tests/testsICP.cpp:248, :346-347, :620) -------------------------------------------------
def _rng(*key):
    return np.random.default_rng(list(key))


def dist_id(n, salt=0):
    r = _rng(n, salt, 1)
    nn = np.zeros(n, DIST_ID)
    nn["dist"] = r.random(n, dtype=np.float32)                                     # U[0, 1)
    nn["id"] = r.integers(0, n, n)
    return nn


def clouds(n, salt=0):
    """F in U[0, 10000), M in U[0, 255), float8."""
    r = _rng(n, salt, 2)
    return (r.random((n, 8), dtype=np.float32) * 10000).astype(np.float32), (r.random((n, 8), dtype=np.float32) * 255).astype(np.float32)


def deviations(m, salt=0):
    """DM, DF in U(-1000, 1000), float4."""
    r = _rng(m, salt, 3)
    return ((r.random((m, 4), dtype=np.float32) * 2000 - 1000).astype(np.float32), (r.random((m, 4), dtype=np.float32) * 2000 - 1000).astype(np.float32))


def weights_in(m, salt=0):
    """Weights as ICPWeights leaves them for dist in U[0, 1)."""
    return weights_exact(dist_id(m, salt + 7)["dist"])


# ---- exact float32 rules --------------------------------------------------------------------------------------------------------
def weights_exact(dist):
    dist = np.ascontiguousarray(dist, np.float32)
    with np.errstate(all="ignore"):
        return np.float32(100) / (np.float32(100) + dist)


def devs_exact(F, M, mean8):
    F, M, mean8 = (np.ascontiguousarray(a, np.float32) for a in (F, M, mean8))
    with np.errstate(all="ignore"):
        return F.reshape(-1, 8)[:, :4] - mean8[:4], M.reshape(-1, 8)[:, :4] - mean8[4:]


def lms_exact(cloud):
    return np.ascontiguousarray(np.ascontiguousarray(cloud, np.float32).reshape(480, 640, 8)[49:49 + 384:3, 65:65 + 512:4]).reshape(16384, 8)


def reps_grid_rule(m, nr):
    """(nrx, nry, side) of the representative grid, or None where (m, nr) is refused: nr a power of two, at most m; m a square; both
    grid sides divide the landmark grid's side."""
    if m <= 0 or nr <= 0 or nr > m or nr & (nr - 1):
        return None
    side = int(np.sqrt(m) + 0.5)
    if side * side != m:
        return None
    pw = nr.bit_length() - 1
    nrx, nry = 2 ** (pw - pw // 2), 2 ** (pw // 2)
    if side % nrx or side % nry:
        return None
    return nrx, nry, side


def reps_index(m, nr):
    """Source index of every representative, row-major over the (nry, nrx) grid."""
    nrx, nry, side = reps_grid_rule(m, nr)

    def axis(count):
        step, g = side // count, np.arange(count)
        return g if step == 1 else g * step + step // 2 - 1

    return (axis(nry)[:, None] * side + axis(nrx)[None, :]).reshape(-1)


def index_cloud(side):
    """A side x side landmark set whose lanes 0..2 hold the point's own (x, y, index); lanes 3..7 tell the points apart too."""
    m = side * side
    i = np.arange(m)
    F = np.empty((m, 8), np.float32)
    F[:, 0], F[:, 1], F[:, 2], F[:, 3] = i % side, i // side, i, 1
    F[:, 4:] = (i[:, None] * 4 + np.arange(4)[None, :]) * 0.25
    return F


def pixel_cloud(seed=0):
    """A 640 x 480 cloud whose lanes hold (col, row, pixel index, 1) and four lanes of arbitrary bit patterns: NaNs with payloads,
    infinities, denormals and -0.0 among them."""
    i = np.arange(640 * 480)
    c = np.empty((640 * 480, 8), np.float32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = i % 640, i // 640, i, 1
    pat = _rng(seed, 4).integers(0, 2 ** 32, (640 * 480, 4), dtype=np.uint64).astype(np.uint32)
    pat[::5, 0] = 0x7fc00001 + (i[::5] & 0xffff)           # quiet NaNs, payload = the pixel
    pat[1::5, 1] = 0xff800001 + (i[1::5] & 0xffff)          # signalling NaNs, sign set
    pat[2::5, 2] = 0x80000000                               # -0.0
    pat[3::5, 3] = 1 + (i[3::5] & 0xff)                     # denormals
    c[:, 4:] = pat.view(np.float32)
    return c


# ---- float64 restatements -------------------------------------------------------------------------------------------------------
def sum_w64(W):
    with np.errstate(all="ignore"):
        return float(np.sum(np.asarray(W, np.float64)))


def means64(F, M, W=None, sum_w=None):
    """[mean_F, 0 | mean_M, 0]: sum (W x) / sum_w, or sum (x) / n."""
    F, M = np.asarray(F, np.float64).reshape(-1, 8)[:, :3], np.asarray(M, np.float64).reshape(-1, 8)[:, :3]
    out = np.zeros(8)
    if W is None:
        out[:3], out[4:7] = F.sum(0) / F.shape[0], M.sum(0) / M.shape[0]
    else:
        W = np.asarray(W, np.float64)[:, None]
        out[:3], out[4:7] = (W * F).sum(0) / sum_w, (W * M).sum(0) / sum_w
    return out


def s64(DM, DF, W, c):
    """(S[11], scale[11]): S[3 a + b] = sum w (c DM_a) (c DF_b), S[9] = sum w |c DF|^2, S[10] = sum w |c DM|^2 with c as the float32
    the kernel receives; scale = the same sums over absolute values (what a rounding error of a term is relative to)."""
    c = float(np.float32(c))
    Mp, Fp = c * np.asarray(DM, np.float64).reshape(-1, 4)[:, :3], c * np.asarray(DF, np.float64).reshape(-1, 4)[:, :3]
    w = np.ones(Mp.shape[0]) if W is None else np.asarray(W, np.float64)
    S, scale = np.empty(11), np.empty(11)
    for a in range(3):
        for b in range(3):
            t = w * Mp[:, a] * Fp[:, b]
            S[3 * a + b], scale[3 * a + b] = t.sum(), np.abs(t).sum()
    for k, P in ((9, Fp), (10, Mp)):
        S[k], scale[k] = (w[:, None] * P * P).sum(), (np.abs(w)[:, None] * P * P).sum()
    return S, scale


def _lanes(cloud, k):
    """Lanes 0..k-1 of a float8 cloud in float64 (the other lanes may hold signalling NaNs: they are never converted)."""
    return np.asarray(cloud, np.float32).reshape(-1, 8)[:, :k].astype(np.float64)


def _sandwich(q):
    """The matrix of p -> q p q* for any quaternion q = (x, y, z, w), not divided by |q|^2."""
    x, y, z, w = np.asarray(q, np.float64)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), w * w - x * x + y * y - z * z, 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), w * w - x * x - y * y + z * z]])


def transform_q64(cloud, T, variant=1):
    """s (q p q*) + t in float64 from T = [q | t, s].

    variant 2 (icpTransform_Quaternion_2) forms the two quaternion products, so this holds for any q.  variant 1
    (icpTransform_Quaternion) evaluates s (p + 2 v x (v x p + w p)) + t, which the reference equates with the sandwich for the unit
    quaternions it documents (kernels/icp_kernels.cl:753-754, :798): off the unit sphere the two differ by (1 - |q|^2) p, the term
    added here, so that the restatement stays the operation the kernel is specified to perform."""
    T = np.asarray(T, np.float32).astype(np.float64)
    q, t, s = T[:4], T[4:7], T[7]
    A = _sandwich(q)
    if variant == 1:
        A = A + (1.0 - q @ q) * np.eye(3)
    return s * (_lanes(cloud, 3) @ A.T) + t


def transform_q_scale(cloud, T):
    """|s| |q|^2 |p| + |t| per point (the norm of the quaternion kinds' error)."""
    T = np.asarray(T, np.float32).astype(np.float64)
    p = _lanes(cloud, 3)
    return abs(T[7]) * (T[:4] @ T[:4]) * np.sqrt((p * p).sum(1)) + np.sqrt(T[4:7] @ T[4:7])


def transform_m64(cloud, T16):
    """(rows 0..2 of T) times the point as stored, lane 3 included; and sum_k |T_rk p_k| per output."""
    T = np.asarray(T16, np.float32).astype(np.float64).reshape(4, 4)[:3]
    p = _lanes(cloud, 4)
    return p @ T.T, np.abs(p) @ np.abs(T).T


# ---- tolerances: error of a result in its norm, in units of EPS -----------------------------------------------------------------
def weights_err(W, sw, dist):
    """(max |W - 100 / (100 + dist)|, |sw - sum W| / sum W) in EPS."""
    want = 100.0 / (100.0 + np.asarray(dist, np.float64))
    s = sum_w64(weights_exact(dist))
    return float(np.abs(np.asarray(W, np.float64) - want).max()) / EPS, abs(sw - s) / s / EPS


def means_err(mean8, want):
    """max over the six means of |error| / the input range, in EPS; lanes 3 and 7 must be exactly 0."""
    mean8 = np.asarray(mean8, np.float64)
    assert mean8[3] == 0 and mean8[7] == 0, mean8
    d = np.abs(mean8 - want)
    return max(float(d[:3].max()) / F_RANGE, float(d[4:7].max()) / M_RANGE) / EPS


def s_err(S, want, scale):
    """max over the eleven terms of |error| / scale, in EPS; a term whose scale is 0 must be exactly 0."""
    d = np.abs(np.asarray(S, np.float64) - want)
    assert np.all(d[scale == 0] == 0), (S, want)
    return float((d[scale > 0] / scale[scale > 0]).max()) / EPS if np.any(scale > 0) else 0.0


def transform_err(out, want, scale):
    """max |error| / scale over the points' xyz, in EPS; where the scale is 0 the result must be exact."""
    d = np.abs(_lanes(out, 3) - want)
    scale = scale if np.ndim(scale) == 2 else np.asarray(scale)[:, None]
    if scale.min() > 0:
        return float((d / scale).max()) / EPS
    scale = np.broadcast_to(scale, d.shape)
    assert np.all(d[scale == 0] == 0)
    return float((d[scale > 0] / scale[scale > 0]).max()) / EPS if np.any(scale > 0) else 0.0


# ---- the transforms' inputs -----------------------------------------------------------------------------------------------------
def transform_cloud_in(seed):
    """307200 points: xyz in U[0, 255) (the reference's ICP::rNum_0_255), lane 3 = 1 but for every seventh point (the matrix kind
    multiplies the translation by it), lanes 4..7 arbitrary bit patterns, NaNs with payloads among them."""
    r = _rng(seed, 5)
    n = 307200
    c = (r.random((n, 8), dtype=np.float32) * 255).astype(np.float32)
    c[:, 3] = 1
    c[::7, 3] = (r.random(c[::7].shape[0], dtype=np.float32) * 4 - 2).astype(np.float32)
    pat = r.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    pat[::3, 1] = 0x7fc00000 + (np.arange(n)[::3] & 0x3fffff)
    pat[1::3, 2] = 0xffa00000 + (np.arange(n)[1::3] & 0xfffff)
    c[:, 4:] = pat.view(np.float32)
    return c


def nonfinite_points():
    """24 points with +inf, -inf or NaN in one of x, y, z, lane 3 (the rest finite)."""
    r = _rng(6)
    c = (r.random((24, 8), dtype=np.float32) * 255).astype(np.float32)
    c[:, 3] = 1
    k = 0
    for v in (np.inf, -np.inf, np.nan):
        for lane in (0, 1, 2, 3):
            c[k, lane] = v
            c[k + 1, lane] = v
            k += 2
    return c


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt(v @ v)


def quaternion_transforms():
    """[(name, T = [q | t, s])] for both quaternion kinds."""
    r = _rng(8)
    q = _unit(r.normal(size=4))
    t = r.uniform(0, 255, 3)
    s = r.uniform(0.1, 1)

    def T(q, t, s):
        return np.concatenate([q, t, [s]]).astype(np.float32)

    return [("identity", T([0, 0, 0, 1], [0, 0, 0], 1)),
            ("unit", T(q, t, s)),
            ("norm_2", T(2 * q, t, s)),
            ("norm_half", T(0.5 * q, t, s)),
            ("q_zero", T([0, 0, 0, 0], t, s)),
            ("half_turn", T(np.concatenate([_unit(r.normal(size=3)), [0]]), t, s)),
            ("s_zero", T(q, t, 0)),
            ("s_minus_one", T(q, t, -1)),
            ("s_milli", T(q, t, 1e-3)),
            ("t_zero", T(q, [0, 0, 0], s))]


def matrix_transforms():
    """[(name, row-major 4x4)] for the matrix kind."""
    r = _rng(9)
    R = _sandwich(_unit(r.normal(size=4)))
    t = r.uniform(0, 255, 3)

    def T(A, t, row3=(0, 0, 0, 1)):
        M = np.zeros((4, 4))
        M[:3, :3], M[:3, 3], M[3] = A, t, row3
        return M.astype(np.float32)

    return [("identity", T(np.eye(3), [0, 0, 0])),
            ("rigid", T(0.7 * R, t)),
            ("row3", T(0.7 * R, t, (3, -5, 7, 11))),
            ("s_zero", T(0 * R, t)),
            ("s_minus_one", T(-R, t)),
            ("s_milli", T(1e-3 * R, t)),
            ("t_zero", T(0.7 * R, [0, 0, 0])),
            ("general", T(r.uniform(-2, 2, (3, 3)), t))]


def check_transforms(cloud, transform_q, transform_m):
    """Every transformation on one cloud: lanes 3..7 untouched, xyz against float64.  Returns the worst error per kind, in EPS."""
    worst = {"q": 0.0, "q2": 0.0, "m": 0.0}
    for name, T in quaternion_transforms():
        scale = transform_q_scale(cloud, T)
        for variant, kind in ((1, "q"), (2, "q2")):
            out = transform_q(cloud, T, variant)
            assert_raw_bits(out[:, 3:], cloud[:, 3:], name + ": lanes 3..7")
            worst[kind] = max(worst[kind], transform_err(out, transform_q64(cloud, T, variant), scale))
            if name == "identity":
                assert np.array_equal(out[:, :3], cloud[:, :3])
    for name, T in matrix_transforms():
        out = transform_m(cloud, T)
        assert_raw_bits(out[:, 3:], cloud[:, 3:], name + ": lanes 3..7")
        want, scale = transform_m64(cloud, T)
        worst["m"] = max(worst["m"], transform_err(out, want, scale))
        if name == "identity":
            assert np.array_equal(out[:, :3], cloud[:, :3])
        if name == "row3":
            assert_raw_bits(out, transform_m(cloud, dict(matrix_transforms())["rigid"]), "row 3 of T is ignored")
    return worst
