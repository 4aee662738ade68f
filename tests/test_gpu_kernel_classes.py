"""The per-kernel classes (icp_kernel_*, KernelObject: ICPLMs, ICPReps, ICPWeights, ICPMean<>, ICPDevs, ICPS<>) and the cloud
kernels (k_get_lms, k_transform_cloud, k_transform_cloud_ex<>) at their shape and value edges.

Every output is checked (a) bit for bit against the oracle's twin, (b) bit for bit against the exact numpy rule where one rounded
operation decides the result, (c) against a float64 restatement within the tolerances of tests/kernel_classes_ref.py on the finite
cases.  test_kernel_classes_cpu.py holds the oracle's twins against the same numpy references at the same shapes and values."""
import ctypes as C

import numpy as np
import pytest

import kernel_classes_ref as ref
from kernel_classes_ref import EPS, TOL, assert_bits, assert_raw_bits

pytestmark = pytest.mark.gpu


def assert_f64_bits(got, want, what):
    assert_bits(np.array([got], np.float64), np.array([want], np.float64), what)


# ---- weights and means ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.N_EVEN)
def test_weights_and_means(engine, oracle, n):
    nn = ref.dist_id(n)
    W, sw = engine.kernel_weights(nn)
    Wo, swo = oracle.weights(nn)
    assert_bits(W, Wo, "W against the oracle")
    assert_f64_bits(sw, swo, "sum_w against the oracle")
    assert_bits(W, ref.weights_exact(nn["dist"]), "W against the exact rule")
    eW, eS = ref.weights_err(W, sw, nn["dist"])
    assert eW <= TOL / EPS and eS <= TOL / EPS, (n, eW, eS)
    F, M = ref.clouds(n)
    mw, mr = engine.kernel_mean(F, M, W, sw), engine.kernel_mean(F, M)
    assert_bits(mw, oracle.mean_weighted(F, M, Wo, swo), "weighted means against the oracle")
    assert_bits(mr, oracle.mean(F, M), "means against the oracle")
    ew, er = ref.means_err(mw, ref.means64(F, M, W, sw)), ref.means_err(mr, ref.means64(F, M))
    assert ew <= TOL / EPS and er <= TOL / EPS, (n, ew, er)


@pytest.mark.parametrize("edge", ref.WEIGHT_EDGES, ids=[repr(e) for e in ref.WEIGHT_EDGES])
def test_weights_value_edges(engine, oracle, edge):
    for pos in ref.WEIGHT_EDGE_POS:
        nn = ref.dist_id(130, salt=pos)
        nn["dist"][pos] = edge
        W, sw = engine.kernel_weights(nn)
        Wo, swo = oracle.weights(nn)
        want = ref.weights_exact(nn["dist"])
        assert_bits(W, Wo, "W against the oracle")
        assert_bits(W, want, "W against the exact rule")
        assert_f64_bits(sw, swo, "sum_w against the oracle")
        s = ref.sum_w64(want)
        assert np.isnan(sw) == np.isnan(s) and np.isinf(sw) == np.isinf(s), (edge, pos, sw, s)
        if np.isfinite(s):
            assert abs(sw - s) <= TOL * abs(s), (edge, pos, sw, s)
        if edge == np.inf:
            assert W[pos] == 0 and not np.signbit(W[pos]) and np.isfinite(sw)
        if edge == -100.0:
            assert W[pos] == np.inf and sw == np.inf


def test_weights_all_edges_in_one_input(engine, oracle):
    nn = ref.dist_id(130, salt=99)
    nn["dist"][3:3 + len(ref.WEIGHT_EDGES)] = ref.WEIGHT_EDGES
    W, sw = engine.kernel_weights(nn)
    assert_bits(W, oracle.weights(nn)[0], "W against the oracle")
    assert_bits(W, ref.weights_exact(nn["dist"]), "W against the exact rule")
    assert np.isnan(sw)


@pytest.mark.parametrize("n", ref.N_PADDED)
def test_weighted_mean_value_edges(engine, oracle, n):
    F, M = ref.clouds(n, salt=1)
    W = ref.weights_in(n, salt=1)
    assert_raw_bits(engine.kernel_mean(F, M, np.zeros(n, np.float32), 1.0), np.zeros(8, np.float32), "all weights zero")
    for j in (0, 1, 127, 128, n - 1):           # one nonzero weight: the mean is that point
        one = np.zeros(n, np.float32)
        one[j] = W[j]
        got = engine.kernel_mean(F, M, one, float(one[j]))
        want = np.concatenate([F[j, :3], [0], M[j, :3], [0]])
        assert np.all(np.abs(got - want) <= 2 * EPS * np.abs(want)), (j, got, want)
        assert_bits(got, oracle.mean_weighted(F, M, one, float(one[j])), "one weight against the oracle")
    assert_bits(engine.kernel_mean(F, M, W, 0.0), oracle.mean_weighted(F, M, W, 0.0), "sum_w = 0 against the oracle")


# ---- deviations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.N_DEVS)
def test_devs(engine, oracle, n):
    F, M = ref.clouds(n, salt=2)
    F[:, 3] = M[:, 3] = 1
    nonfinite = np.array([np.inf, 1, 2, 0, 3, np.nan, 4, -np.inf], np.float32)
    for mean8 in (ref.means64(F, M).astype(np.float32), np.array([1, 2, 3, 2.5, -4, 5, 6, -1], np.float32), nonfinite):
        if mean8 is nonfinite:
            F[::3, 0], F[1::3, 1], M[::2, 2], M[1::2, 3] = np.inf, -np.inf, np.nan, np.inf
        DF, DM = engine.kernel_devs(F, M, mean8)
        DFo, DMo = oracle.devs(F, M, mean8)
        wF, wM = ref.devs_exact(F, M, mean8)
        assert_bits(DF, DFo, "DF against the oracle")
        assert_bits(DM, DMo, "DM against the oracle")
        assert_bits(DF, wF, "DF against the exact rule")
        assert_bits(DM, wM, "DM against the exact rule")
        if mean8[3] == 2.5:
            assert np.all(DF[:, 3] == -1.5) and np.all(DM[:, 3] == 2)            # lane 3 is subtracted like the others


# ---- S ----------------------------------------------------------------------------------------------------------------------------
def check_s(engine, oracle, m, c, salt=0):
    DM, DF = ref.deviations(m, salt)
    W = ref.weights_in(m, salt)
    out = []
    for w in (W, None):
        S = engine.kernel_s(DM, DF, w, c)
        assert_bits(S, oracle.sij(DM, DF, w, c), "S against the oracle (m = %d, c = %g, %s)" % (m, c, "regular" if w is None else "weighted"))
        want, scale = ref.s64(DM, DF, w, c)
        e = ref.s_err(S, want, scale)
        assert e <= TOL / EPS, (m, c, w is None, e)
        out.append(S)
    return out


@pytest.mark.parametrize("m", ref.M_S)
def test_s(engine, oracle, m):
    check_s(engine, oracle, m, 1e-6)


@pytest.mark.parametrize("m,c", ref.S_SCALINGS)
def test_s_scalings(engine, oracle, m, c):
    Sw, Sr = check_s(engine, oracle, m, c, salt=1)
    if c == 0.0:
        assert_raw_bits(Sw, np.zeros(11, np.float32), "c = 0, weighted")
        assert_raw_bits(Sr, np.zeros(11, np.float32), "c = 0, regular")


@pytest.mark.parametrize("m", ref.M_PADDED)
def test_s_value_edges(engine, oracle, m):
    DM, DF = ref.deviations(m, salt=2)
    assert_raw_bits(engine.kernel_s(DM, DF, np.zeros(m, np.float32), 1e-6), np.zeros(11, np.float32), "zero weights")
    bM, bF = (np.sign(DM) * np.float32(1e19)).astype(np.float32), (np.sign(DF) * np.float32(1e19)).astype(np.float32)
    for w in (ref.weights_in(m, 2), None):       # the products overflow: inf and NaN in the oracle's places, its bits elsewhere
        S, So = engine.kernel_s(bM, bF, w, 1.0), oracle.sij(bM, bF, w, 1.0)
        assert_bits(S, So, "overflowing S against the oracle")
        assert np.all(np.isposinf(S[9:]))


# ---- resident objects -------------------------------------------------------------------------------------------------------------
def test_set_scaling(engine, oracle):
    m = 2049
    DM, DF = ref.deviations(m, salt=3)
    W = ref.weights_in(m, salt=3)
    S = engine.KernelObject("s_weighted", m, c=1e-6)
    S.write(0, DM); S.write(1, DF); S.write(2, W)
    S.run()
    assert_bits(S.read(3), oracle.sij(DM, DF, W, 1e-6), "c = 1e-6")
    S.set_scaling(1e-3)
    S.run()
    assert_bits(S.read(3), oracle.sij(DM, DF, W, 1e-3), "after set_scaling (1e-3)")
    assert not np.array_equal(oracle.sij(DM, DF, W, 1e-3), oracle.sij(DM, DF, W, 1e-6))
    S.close()


@pytest.mark.parametrize("n", ref.N_PADDED)
def test_weights_and_means_after_a_poisoned_run(engine, oracle, n):
    """NaN everywhere, then clean inputs on the same objects: nothing stale survives in the planes, the partials or their pads."""
    nn = ref.dist_id(n, salt=4)
    F, M = ref.clouds(n, salt=4)
    bad = np.zeros(n, engine.DIST_ID)
    bad["dist"] = np.nan
    wts, mean = engine.KernelObject("weights", n), engine.KernelObject("mean_weighted", n)
    wts.write(0, bad)
    wts.run()
    assert np.all(np.isnan(wts.read(1))) and np.isnan(wts.read(2, np.float64)[0])
    mean.write(0, np.full((n, 8), np.nan, np.float32)); mean.write(1, np.full((n, 8), np.nan, np.float32))
    mean.write(2, np.full(n, np.nan, np.float32)); mean.write(3, np.array([np.nan]))
    mean.run()
    assert np.all(np.isnan(mean.read(4)[[0, 1, 2, 4, 5, 6]]))
    wts.write(0, nn)
    wts.run()
    W, sw = wts.read(1), wts.read(2, np.float64)[0]
    Wf, swf = engine.kernel_weights(nn)                                             # a fresh object
    assert_raw_bits(W, Wf, "W after poison")
    assert_f64_bits(sw, swf, "sum_w after poison")
    assert_bits(W, oracle.weights(nn)[0], "W against the oracle")
    mean.write(0, F); mean.write(1, M); mean.write(2, W); mean.write(3, np.array([sw]))
    mean.run()
    assert_raw_bits(mean.read(4), engine.kernel_mean(F, M, W, sw), "means after poison")
    assert_bits(mean.read(4), oracle.mean_weighted(F, M, W, sw), "means against the oracle")
    wts.close(); mean.close()


@pytest.mark.parametrize("m", ref.M_PADDED)
def test_s_after_a_poisoned_run(engine, oracle, m):
    DM, DF = ref.deviations(m, salt=5)
    S = engine.KernelObject("s", m, c=1e-6)
    S.write(0, np.full((m, 4), np.nan, np.float32)); S.write(1, np.full((m, 4), np.nan, np.float32))
    S.run()
    assert np.all(np.isnan(S.read(3)))
    S.write(0, DM); S.write(1, DF)
    S.run()
    assert_raw_bits(S.read(3), engine.kernel_s(DM, DF, None, 1e-6), "S after poison")
    assert_bits(S.read(3), oracle.sij(DM, DF, None, 1e-6), "S against the oracle")
    S.close()


def test_adopt_into_a_used_slot(engine, oracle):
    n = 258
    F, M = ref.clouds(n, salt=6)
    W = ref.weights_in(n, salt=6)
    sw = ref.sum_w64(W)
    own = np.array([1, 2, 3, 2.5, -4, 5, 6, -1], np.float32)
    mean, devs = engine.KernelObject("mean_weighted", n), engine.KernelObject("devs", n)
    devs.write(0, F); devs.write(1, M); devs.write(2, own)                          # slot 2 in use: a buffer of its own
    devs.run()
    first = devs.get(2)
    assert_bits(devs.read(3).reshape(n, 4), ref.devs_exact(F, M, own)[0], "DF with its own means")
    mean.write(0, F); mean.write(1, M); mean.write(2, W); mean.write(3, np.array([sw]))
    mean.run()
    devs.adopt(2, mean.get(4))
    assert devs.get(2) == mean.get(4) and devs.get(2) != first
    devs.run()
    m8 = mean.read(4)
    assert_bits(m8, oracle.mean_weighted(F, M, W, sw), "means against the oracle")
    assert_raw_bits(devs.read(2), m8, "the adopted slot reads the producer's buffer")
    wF, wM = ref.devs_exact(F, M, m8)
    assert_bits(devs.read(3).reshape(n, 4), wF, "DF follows the adopted means")
    assert_bits(devs.read(4).reshape(n, 4), wM, "DM follows the adopted means")
    devs.close(); mean.close()


def test_error_paths(engine):
    def refused(fn, *args, **kw):
        with pytest.raises(engine.ICPError) as e:
            fn(*args, **kw)
        assert str(e.value).split(": ", 1)[1].strip(), e.value

    for kind in ("weights", "mean", "mean_weighted"):
        for n in (0, 1, 7, 129):
            refused(engine.KernelObject, kind, n)
    for kind in ("devs", "s", "s_weighted"):
        refused(engine.KernelObject, kind, 0)
    L, h = engine.lib(), C.c_void_p()
    for kind in (-1, 8, 99):
        refused(lambda: engine._kchk(L.icp_ko_create(C.byref(h), 0, kind, 2, 0, 1e-6)))
        assert not h.value
    k = engine.KernelObject("weights", 2)         # three slots
    other = engine.KernelObject("weights", 2)
    for slot in (-1, 3, 5):
        refused(k.get, slot)
        refused(k.read, slot)
        refused(k.adopt, slot, other.get(1))
    for slot, a in ((0, np.zeros(3, engine.DIST_ID)), (1, np.zeros(1, np.float32)), (2, np.zeros(2, np.float64))):
        with pytest.raises(ValueError):
            k.write(slot, a)
    k.close(); other.close()


# ---- representatives and landmarks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,nr", ref.REPS_CASES)
def test_reps(engine, oracle, side, nr):
    F = ref.index_cloud(side)
    want = F[ref.reps_index(side * side, nr)]
    R = engine.kernel_reps(F, nr)
    assert_raw_bits(R, want, "kernel_reps against the numpy index")
    assert_raw_bits(R, oracle.get_reps(F, nr)[0], "kernel_reps against the oracle")
    k = engine.KernelObject("reps", side * side, nr)
    k.write(0, F)
    k.run()
    assert_raw_bits(k.read(1), want, "KernelObject (reps) against the numpy index")
    k.close()


def test_reps_refusals(engine):
    for side in range(1, 25):
        m, nr = side * side, 1
        while nr <= m:
            if ref.reps_grid_rule(m, nr) is None:
                with pytest.raises(engine.ICPError):
                    engine.KernelObject("reps", m, nr)
            else:
                engine.KernelObject("reps", m, nr).close()                          # (creation launches nothing)
            nr *= 2
    for m, nr in ((15, 1), (24, 4), (16383, 256), (16, 3), (16, 0), (16, 32), (0, 1)):    # no square; no power of two; nr > m; nothing
        with pytest.raises(engine.ICPError):
            engine.KernelObject("reps", m, nr)
    with pytest.raises(engine.ICPError):
        engine.kernel_reps(ref.index_cloud(4)[:15], 1)


def test_landmarks(engine, oracle):
    cloud = ref.pixel_cloud()
    want = ref.lms_exact(cloud)
    assert_raw_bits(oracle.get_lms(cloud), want, "oracle")
    assert_raw_bits(engine.kernel_lms(cloud), want, "kernel_lms")
    k = engine.KernelObject("lms")
    k.write(0, cloud)
    k.run()
    assert_raw_bits(k.read(1), want, "KernelObject (lms)")
    k.close()
    g = engine.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    g.write_cloud(engine.Memory.F, cloud)
    other = ref.pixel_cloud(seed=1)
    g.write_cloud(engine.Memory.M, other)
    assert_raw_bits(g.read(engine.Memory.F), want, "write_cloud (F)")
    assert_raw_bits(g.read(engine.Memory.M), ref.lms_exact(other), "write_cloud (M)")
    g.close()
    g = engine.ICP(0)
    g.init(4096, 64, 2e2, 1e-6)
    with pytest.raises(engine.ICPError):
        g.write_cloud(engine.Memory.F, cloud)
    g.close()


# ---- transforms -------------------------------------------------------------------------------------------------------------------
def test_transforms(engine, oracle):
    """One handle, every n in an order that makes its cloud buffer grow, be reused smaller, and be reused at full size with new data."""
    K = engine.TransformKind
    g = engine.ICP(0)
    clouds = [ref.transform_cloud_in(0), ref.transform_cloud_in(1)]

    def transform_q(cloud, T, variant):
        out = g.transform_cloud(cloud, T, K.QUATERNION if variant == 1 else K.QUATERNION_2)
        assert_bits(out, oracle.transform_q(cloud, T, variant), "quaternion kind %d against the oracle" % variant)
        return out

    def transform_m(cloud, T):
        out = g.transform_cloud(cloud, T, K.MATRIX)
        assert_bits(out, oracle.transform_m(cloud, T), "matrix kind against the oracle")
        return out

    for i, n in enumerate(ref.TRANSFORM_N):
        worst = ref.check_transforms(clouds[ref.TRANSFORM_CLOUD_SEEDS[i]][:n], transform_q, transform_m)
        for kind, e in worst.items():
            assert e <= ref.TRANSFORM_TOL[kind], (n, kind, e)
    pts = ref.nonfinite_points()                  # +-inf or NaN in one coordinate: the oracle's bits, lanes 3..7 untouched
    for name, T in ref.quaternion_transforms():
        for variant in (1, 2):
            assert_raw_bits(transform_q(pts, T, variant)[:, 3:], pts[:, 3:], name)
    for name, T in ref.matrix_transforms():
        assert_raw_bits(transform_m(pts, T)[:, 3:], pts[:, 3:], name)
    g.close()


def test_transform_with_the_state_of_a_run(engine, oracle):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = engine.ICP(0)
    g.init(side * side, nr, 2e2, 1e-6, max_iterations=3)
    g.write(engine.Memory.F, F)
    g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run()
    T = g.read(engine.Memory.T)
    assert not np.array_equal(T, np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float32))
    cloud = ref.transform_cloud_in(0)
    for n in (1, 257, 1000):
        out = g.transform_cloud(cloud[:n])
        assert_raw_bits(out, g.transform_cloud(cloud[:n], T, engine.TransformKind.QUATERNION), "state's T against an explicit T")
        assert_bits(out, oracle.transform_q(cloud[:n], T), "state's T against the oracle")
    with pytest.raises(engine.ICPError):
        g.transform_cloud(cloud[:0])
    g.close()
