"""The standalone Reduce / Scan classes (icp_reduce, icp_scan, icp_rs_*) at their value and shape edges.

Every check compares the engine with an independent reference of the same operation: MIN_F with numpy's fmin (the reference's
kernels/reduce_kernels.cl:89-101: NaN loses to any number), MAX_UI with an unsigned max, SUM_F bit for bit with the oracle's
reduce_sum_f tree and with a float64 sum inside the error bound of that tree, the scans with int64 prefix sums wrapped to int32.
The shapes cover the first 512-column group of SUM, the padding of its work-group count to a multiple of 4, one, two and three
SUM passes, ragged and mostly empty per-thread chunks of the scan, and more rows than a grid's y dimension of 65535."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = (4, 8, 252, 256, 260, 508, 512, 516, 1020, 1024, 1536, 2044, 2048, 2052, 4100, 262144, 2 ** 20 + 4)
SCAN_COLS = COLS + (65540,)
MAX_ELEMS = 1024 * 4100                        # the large-cols cases at a few rows only


def _shapes(cols):
    return [(rows, c) for c in cols for rows in (1, 3, 1024) if rows * c <= MAX_ELEMS]


SHAPES = _shapes(COLS)
SCAN_SHAPES = _shapes(SCAN_COLS)
TALL = [(65539, 4), (65539, 516)]             # SUM puts rows on grid.y
MIN, MAX, SUM = 0, 1, 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
U = 2.0 ** -24
BELOW = np.float32(-3e30)                     # below every mixed value: the row's unique minimum where it is planted


def _ids(shapes):
    return ["%dx%d" % s for s in shapes]


def _rng(rows, cols, salt):
    return np.random.default_rng([rows, cols, salt])


def sum_levels(cols):
    """reduce_sum_f passes over `cols` columns (src/ICP/algorithms.cpp:140-142): 512 columns per work-group, the count padded
    to a multiple of 4 unless it is 1."""
    n = 0
    while True:
        wg = (cols + 511) // 512
        wgp = wg if wg == 1 or wg % 4 == 0 else wg + 4 - wg % 4
        n, cols = n + 1, wgp
        if wgp == 1:
            return n


def mixed(r, shape, lo=-30.0, hi=30.0):
    """Random signs and magnitudes 10^[lo, hi): mixed-sign floats across the whole scale."""
    m = 10.0 ** r.uniform(lo, hi, shape)
    return np.where(r.random(shape) < 0.5, -m, m).astype(np.float32)


def same_or_both_nan(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (got == want) | (np.isnan(got) & np.isnan(want))


def assert_min(engine, a, what):
    got, want = engine.reduce(a, MIN), np.fmin.reduce(a, axis=1)
    bad = np.flatnonzero(~same_or_both_nan(got, want))
    assert bad.size == 0, "%s: %d rows differ, first row %d: got %r, fmin %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def wrap32(x):
    """int64 -> int32 two's complement."""
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def per_row_cols(r, rows, lo, hi):
    """One column per row, uniform in [lo, hi)."""
    return r.integers(lo, hi, rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# MIN_F

@pytest.mark.parametrize("rows,cols", SHAPES, ids=_ids(SHAPES))
def test_min_values(engine, rows, cols):
    """Mixed signs over [-1e30, 1e30], infinities, signed zeros and the smallest subnormals."""
    r = _rng(rows, cols, 1)
    a = mixed(r, (rows, cols))
    assert_min(engine, a, "mixed")
    b = a.copy()                                    # rows cycle through: one -inf; +inf among numbers; all +inf
    ri = np.arange(rows)
    b[ri, per_row_cols(r, rows, 0, cols)] = np.where(ri % 3 == 0, -np.inf, np.inf)
    b[ri % 3 == 2] = np.inf
    assert_min(engine, b, "infinities")
    z = r.choice(np.array([-0.0, 0.0, 1.0, 2.5], np.float32), (rows, cols))
    z[1::2] = r.choice(np.array([-0.0, 0.0], np.float32), z[1::2].shape)
    assert_min(engine, z, "signed zeros")
    # subnormals k * 2^-149, no zeros: the minimum is one bit pattern (-1.4e-45 = 0x80000001 where k = -1 is present)
    k = r.choice(np.array([-1, 1, 2, 3]), (rows, cols))
    k[1::2] = np.abs(k[1::2])
    s = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert np.all(s != 0)
    got = engine.reduce(s, MIN)
    assert np.array_equal(got.view(np.uint32), s.min(1).view(np.uint32))
    assert got[0].view(np.uint32) == (0x80000001 if (k[0] == -1).any() else 0x00000001)


@pytest.mark.parametrize("rows,cols", SHAPES, ids=_ids(SHAPES))
def test_min_nan(engine, rows, cols):
    """NaN loses to any number wherever it sits in a thread's strip (columns t + 256 k), its wave or the row; a row is NaN only
    when all of it is."""
    r = _rng(rows, cols, 2)
    base = mixed(r, (rows, cols))
    ri = np.arange(rows)
    a = base.copy()
    a[:, 0] = np.nan                                # thread 0's first value: the one every combine starts from
    assert_min(engine, a, "NaN at column 0")
    a = base.copy()                                 # NaN at t in 1..255, the row minimum elsewhere in thread t's strip
    if cols > 256:
        t = per_row_cols(r, rows, 1, min(256, cols - 256))
        kmax = (cols - 1 - t) // 256
        a[ri, t] = np.nan
        a[ri, t + 256 * r.integers(1, kmax + 1)] = BELOW
    else:                                           # ... or in its wave when the strip is t alone
        t = per_row_cols(r, rows, 1, cols)
        w0 = (t // 64) * 64
        other = w0 + (t - w0 + r.integers(1, np.minimum(64, cols - w0))) % np.minimum(64, cols - w0)
        a[ri, t] = np.nan
        a[ri, other] = BELOW
    assert_min(engine, a, "NaN in a strip that holds the minimum")
    if cols > 64:                                   # NaN at a wave's first lane (64 w), the minimum in the same wave
        a = base.copy()
        w = r.integers(1, min(4, (cols - 2) // 64 + 1), rows)
        a[ri, 64 * w] = np.nan
        a[ri, 64 * w + 1] = BELOW
        assert_min(engine, a, "NaN at a wave's first column")
    if cols > 256:
        a = base.copy()
        a[ri, per_row_cols(r, rows, 256, cols)] = np.nan
        assert_min(engine, a, "NaN at a column >= 256")
    a = np.full((rows, cols), np.nan, np.float32)
    assert np.all(np.isnan(engine.reduce(a, MIN)))
    a = np.full((rows, cols), np.nan, np.float32)   # all NaN but one column (the first, the last, anywhere)
    j = per_row_cols(r, rows, 0, cols)
    j[0] = 0
    j[-1] = cols - 1
    a[ri, j] = base[ri, j]
    got = engine.reduce(a, MIN)
    assert np.array_equal(got.view(np.uint32), base[ri, j].view(np.uint32))
    a = base.copy()                                 # NaN scattered over about a third of the row
    a[r.random((rows, cols)) < 0.3] = np.nan
    assert_min(engine, a, "scattered NaN")


# ---------------------------------------------------------------------------------------------------------------------------------
# MAX_UI

@pytest.mark.parametrize("rows,cols", SHAPES, ids=_ids(SHAPES))
def test_max_ui(engine, rows, cols):
    """Unsigned compare around 0x7FFFFFFF / 0x80000000 / 0xFFFFFFFF; the maximum at column 0, at cols - 1 (where threads t >= cols
    start) and in a thread's strip beyond its first column."""
    r = _rng(rows, cols, 3)
    d = r.integers(-8, 8, (rows, cols))
    around = np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFF7, 0], np.int64)
    pick = r.integers(0, 2, (rows, cols)) + np.where(np.arange(rows) % 2 == 0, 0, 2)[:, None]   # even rows: signed-bit edge only
    u = ((around[pick] + d) % 2 ** 32).astype(np.uint32)
    assert np.array_equal(engine.reduce(u, MAX), u.max(1))
    ri = np.arange(rows)
    base = r.integers(0, 2 ** 31, (rows, cols), dtype=np.uint32)
    places = [np.zeros(rows, np.int64), np.full(rows, cols - 1)]
    if cols > 256:
        t = per_row_cols(r, rows, 0, min(256, cols - 256))
        places.append(t + 256 * r.integers(1, (cols - 1 - t) // 256 + 1))
    for p in places:
        a = base.copy()
        a[ri, p] = np.uint32(0x80000000) + r.integers(0, 2 ** 31, rows).astype(np.uint32)
        got = engine.reduce(a, MAX)
        assert np.array_equal(got, a.max(1)) and np.array_equal(got, a[ri, p])


# ---------------------------------------------------------------------------------------------------------------------------------
# SUM_F

def assert_sum(engine, oracle, a):
    """Against a float64 sum within the tree's bound gamma_D * sum |a_i| (every pass is ((c0 + c1) + c2) + c3 and row_tree8's
    7 levels, D = 10 per pass), then bit for bit against the oracle's tree.  The bound holds for any order of a tree that deep;
    the bits pin the reference's order."""
    got = engine.reduce(a, SUM)
    D = 10 * sum_levels(a.shape[1])
    gamma = D * U / (1 - D * U)
    a64 = a.astype(np.float64)
    err, bound = np.abs(got - a64.sum(1)), gamma * np.abs(a64).sum(1)
    assert np.all(err <= bound), (D, float((err / bound).max()))
    assert np.array_equal(got.view(np.uint32), oracle.reduce_sum_f(a).view(np.uint32)), "within the float64 bound, not the oracle's bits"


@pytest.mark.parametrize("rows,cols", SHAPES, ids=_ids(SHAPES))
def test_sum(engine, oracle, rows, cols):
    """Mixed signs over about 2^-20 .. 2^20; rows with +inf (sum +inf), +inf and -inf (NaN), a NaN (NaN)."""
    r = _rng(rows, cols, 4)
    m = np.exp2(r.uniform(-20, 20, (rows, cols)))
    a = np.where(r.random((rows, cols)) < 0.5, -m, m).astype(np.float32)
    assert_sum(engine, oracle, a)
    b = a.copy()
    ri = np.arange(rows)
    c1, c2 = per_row_cols(r, rows, 0, cols), per_row_cols(r, rows, 0, cols)
    c2 = np.where(c2 == c1, (c1 + 1) % cols, c2)
    b[ri, c1] = np.where(ri % 3 == 2, np.nan, np.inf)
    b[ri[ri % 3 == 1], c2[ri % 3 == 1]] = -np.inf
    got = engine.reduce(b, SUM)
    with np.errstate(invalid="ignore"):
        want = b.astype(np.float64).sum(1)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    assert np.isposinf(got[ri % 3 == 0]).all() and np.isnan(got[ri % 3 != 0]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# Scan

def scan_refs(a):
    c = np.cumsum(a.astype(np.int64), axis=1)
    return wrap32(c), wrap32(c - a)


def scan_input(r, rows, cols):
    """Uniform over the whole int32 range with a run of INT32_MAX and one of INT32_MIN in every row."""
    a = r.integers(I32_MIN, I32_MAX + 1, (rows, cols), dtype=np.int64)
    idx = np.arange(cols)
    for v in (I32_MAX, I32_MIN):
        s = per_row_cols(r, rows, 0, cols)[:, None]
        a[(idx >= s) & (idx < s + max(1, cols // 8))] = v
    return a.astype(np.int32)


@pytest.mark.parametrize("rows,cols", SCAN_SHAPES, ids=_ids(SCAN_SHAPES))
def test_scan(engine, rows, cols):
    """Inclusive and exclusive scans against int64 prefix sums wrapped to int32, element by element; ragged chunks (260, 1020,
    65540), threads with empty chunks (4, 8)."""
    a = scan_input(_rng(rows, cols, 5), rows, cols)
    inc, exc = scan_refs(a)
    got = engine.scan(a, True)
    assert np.array_equal(got, inc), np.argwhere(got != inc)[:4]
    got = engine.scan(a, False)
    assert np.all(got[:, 0] == 0)
    assert np.array_equal(got, exc), np.argwhere(got != exc)[:4]


# ---------------------------------------------------------------------------------------------------------------------------------
# More rows than grid.y holds

@pytest.mark.parametrize("rows,cols", TALL, ids=_ids(TALL))
def test_tall(engine, oracle, rows, cols):
    """65539 rows: above 65535 on SUM's grid.y (k_rs_sum_level); MIN, MAX and the scans put rows on grid.x."""
    r = _rng(rows, cols, 6)
    m = np.exp2(r.uniform(-20, 20, (rows, cols)))
    assert_sum(engine, oracle, np.where(r.random((rows, cols)) < 0.5, -m, m).astype(np.float32))
    a = mixed(r, (rows, cols))
    a[::7, 0] = np.nan
    a[-1] = np.nan
    assert_min(engine, a, "tall")
    u = r.integers(0, 2 ** 32, (rows, cols), dtype=np.uint32)
    assert np.array_equal(engine.reduce(u, MAX), u.max(1))
    s = scan_input(r, rows, cols)
    inc, exc = scan_refs(s)
    assert np.array_equal(engine.scan(s, True), inc)
    assert np.array_equal(engine.scan(s, False), exc)


# ---------------------------------------------------------------------------------------------------------------------------------
# Entry forms and the output buffer

KINDS = [MIN, MAX, SUM, "inclusive", "exclusive"]


def kind_case(oracle, kind, rows, cols, salt, nan=True):
    """(input, reference answer) for one kind; MIN's input has NaN unless nan=False."""
    r = _rng(rows, cols, salt)
    if kind == MIN:
        a = mixed(r, (rows, cols))
        if nan:
            a[r.random((rows, cols)) < 0.2] = np.nan
            a[:, 0] = np.nan
        return a, np.fmin.reduce(a, axis=1)
    if kind == MAX:
        a = r.integers(0, 2 ** 32, (rows, cols), dtype=np.uint32)
        return a, a.max(1)
    if kind == SUM:
        a = mixed(r, (rows, cols), -6, 6)
        return a, oracle.reduce_sum_f(a)
    a = scan_input(r, rows, cols)
    return a, scan_refs(a)[0 if kind == "inclusive" else 1]


def one_shot(engine, kind, a):
    return engine.scan(a, kind == "inclusive") if isinstance(kind, str) else engine.reduce(a, kind)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


@pytest.mark.parametrize("kind", KINDS)
def test_entry_forms_agree(engine, oracle, kind):
    """One-shot call, resident object (write, run twice, rewrite, run) and the reference answer are identical."""
    rows, cols = 3, 2052
    rs = engine.ReduceScan(kind, cols, rows)
    try:
        for salt in (7, 8):
            a, want = kind_case(oracle, kind, rows, cols, salt)
            rs.write(a)
            rs.run()
            if salt == 7:
                rs.run()
            got = rs.read()
            assert np.array_equal(bits(got), bits(want))
            assert np.array_equal(bits(one_shot(engine, kind, a)), bits(want))
    finally:
        rs.close()


def _hip():
    """hipMemcpy / hipDeviceSynchronize of the HIP runtime the engine library is linked against."""
    H = C.CDLL(__import__("icp_amd").lib_path())
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipMemcpy.restype = C.c_int
    H.hipDeviceSynchronize.restype = C.c_int
    return H


STABLE = [(SUM, 512), (SUM, 1024), (SUM, 2 ** 20 + 4), (MIN, 1024), (MAX, 1024), ("inclusive", 1024), ("exclusive", 1024)]


@pytest.mark.parametrize("kind,cols", STABLE, ids=["%s-%d" % (k if isinstance(k, str) else "min max sum".split()[k], c) for k, c in STABLE])
def test_output_pointer_is_stable(engine, oracle, kind, cols):
    """icp_rs_device_ptr(r, 1), taken before the first run, holds every run's result (one, two and three SUM passes)."""
    rows = 3
    H = _hip()
    rs = engine.ReduceScan(kind, cols, rows)
    try:
        p = rs.device_ptr(True)
        assert p and p != rs.device_ptr(False)
        for salt in (9, 10):
            a, want = kind_case(oracle, kind, rows, cols, salt, nan=False)
            rs.write(a)
            rs.run()
            got = rs.read()
            assert np.array_equal(bits(got), bits(want))
            assert rs.device_ptr(True) == p
            host = np.empty_like(got)
            assert H.hipDeviceSynchronize() == 0
            assert H.hipMemcpy(host.ctypes.data, p, host.nbytes, 2) == 0           # hipMemcpyDeviceToHost
            assert np.array_equal(bits(host), bits(got)), "the output pointer taken before the first run holds something else"
    finally:
        rs.close()
