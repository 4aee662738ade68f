"""The oracle's twins of the per-kernel classes and of the cloud transforms against plain numpy (tests/kernel_classes_ref.py), at
every shape and value test_gpu_kernel_classes.py runs the engine at.  The GPU tests compare the engine's bits with these twins;
this module pins the twins themselves to references that share nothing with them: exact float32 rules where one rounded
operation decides the result, float64 restatements without trees or padding elsewhere.

Worst error of the oracle against float64 over every case of this module (its seeds, the reference tests' input ranges), in
eps = 2^-23 of the norm each check states; test_report_measured_worst_cases prints them again (pytest -s):

    W                        0.568   absolute
    sum of the weights       0.577   of the sum
    means, regular           0.461   of the input range (10000 for F, 255 for M)
    means, weighted          0.500   likewise
    S, regular               1.258   of sum |c a| |c b| of the term
    S, weighted              1.094   of sum w |c a| |c b| of the term
    transform, quaternion    1.977   of |s| |q|^2 |p| + |t|
    transform, quaternion 2  1.714   likewise
    transform, matrix        1.385   of sum_k |T_rk p_k|

None exceeds 2 eps, what a tree of correctly rounded additions gives: the first six are asserted at 8 eps, the transforms at four
times their measurement (7.9, 6.9 and 5.5 eps, kernel_classes_ref.TRANSFORM_TOL).

The float64 restatement of icpTransform_Quaternion is s (q p q*) + t plus the term (1 - |q|^2) s p: the kernel evaluates
s (p + 2 v x (v x p + w p)) + t (kernels/icp_kernels.cl:798), which is the sandwich product for unit quaternions only.  The
engine and the oracle both follow that line; with |q| = 2, 0.5 or 0 the bare sandwich is another function.  The reference's own
literal q (four decimals, |q|^2 = 1 + 1.1e-5) already separates the two by 1.2e-3 on U[0, 255) points.

Two one-line changes of the oracle are invisible at every size these classes accept, here and anywhere: dropping the
`wgp != 1` exception in orc_weights pads one partial with three zeros and sums the same double; `idx & ~1` and `idx` guard the
same positions for every even n."""
import json
import os

import numpy as np
import pytest

import kernel_classes_ref as ref
from kernel_classes_ref import EPS, TOL, assert_bits, assert_raw_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}                                      # quantity -> worst error seen in this session, in EPS (printed by the last test)


def note(what, err):
    WORST[what] = max(WORST.get(what, 0.0), err)
    return err


# ---- weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.N_EVEN)
def test_weights(oracle, n):
    nn = ref.dist_id(n)
    W, sw = oracle.weights(nn)
    assert_bits(W, ref.weights_exact(nn["dist"]), "W")
    eW, eS = ref.weights_err(W, sw, nn["dist"])
    assert note("W", eW) <= TOL / EPS and note("sum_w", eS) <= TOL / EPS, (n, eW, eS)
    if n == 16384:                              # the reference's own checks at its size (tests/testsICP.cpp: 42 eps, 4200 eps, absolute)
        assert eW <= 42 and abs(sw - ref.sum_w64(W)) <= 4200 * EPS


@pytest.mark.parametrize("edge", ref.WEIGHT_EDGES, ids=[repr(e) for e in ref.WEIGHT_EDGES])
def test_weights_value_edges(oracle, edge):
    for pos in ref.WEIGHT_EDGE_POS:
        nn = ref.dist_id(130, salt=pos)
        nn["dist"][pos] = edge
        W, sw = oracle.weights(nn)
        want = ref.weights_exact(nn["dist"])
        assert_bits(W, want, "W")
        s = ref.sum_w64(want)
        assert np.isnan(sw) == np.isnan(s) and np.isinf(sw) == np.isinf(s), (edge, pos, sw, s)
        if np.isfinite(s):
            assert abs(sw - s) <= TOL * abs(s), (edge, pos, sw, s)
        if edge == np.inf:
            assert W[pos] == 0 and not np.signbit(W[pos]) and np.isfinite(sw)
        if edge == -100.0:
            assert W[pos] == np.inf and sw == np.inf


def test_weights_all_edges_in_one_input(oracle):
    nn = ref.dist_id(130, salt=99)
    nn["dist"][3:3 + len(ref.WEIGHT_EDGES)] = ref.WEIGHT_EDGES
    W, sw = oracle.weights(nn)
    assert_bits(W, ref.weights_exact(nn["dist"]), "W")
    assert np.isnan(sw) and np.isnan(ref.sum_w64(W))


# ---- means ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.N_EVEN)
def test_means(oracle, n):
    F, M = ref.clouds(n)
    W = ref.weights_in(n)
    sw = ref.sum_w64(W)
    ew = note("mean_weighted", ref.means_err(oracle.mean_weighted(F, M, W, sw), ref.means64(F, M, W, sw)))
    er = note("mean", ref.means_err(oracle.mean(F, M), ref.means64(F, M)))
    assert ew <= TOL / EPS and er <= TOL / EPS, (n, ew, er)                       # (and so inside the reference's 420000 eps, absolute)


@pytest.mark.parametrize("n", ref.N_PADDED)
def test_weighted_mean_value_edges(oracle, n):
    F, M = ref.clouds(n, salt=1)
    W = ref.weights_in(n, salt=1)
    assert np.all(oracle.mean_weighted(F, M, np.zeros(n, np.float32), 1.0) == 0)
    for j in (0, 1, 127, 128, n - 1):           # one nonzero weight: the mean is that point
        one = np.zeros(n, np.float32)
        one[j] = W[j]
        got = oracle.mean_weighted(F, M, one, float(one[j]))
        want = np.concatenate([F[j, :3], [0], M[j, :3], [0]])
        assert np.all(np.abs(got - want) <= 2 * EPS * np.abs(want)), (j, got, want)
    inf = oracle.mean_weighted(F, M, W, 0.0)     # sum_w = 0: W / 0 = inf, times a positive coordinate
    assert np.all(np.isposinf(inf[[0, 1, 2, 4, 5, 6]])) and inf[3] == 0 and inf[7] == 0


# ---- deviations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.N_DEVS)
def test_devs(oracle, n):
    F, M = ref.clouds(n, salt=2)
    F[:, 3] = M[:, 3] = 1
    for mean8 in (ref.means64(F, M).astype(np.float32), np.array([1, 2, 3, 2.5, -4, 5, 6, -1], np.float32)):
        DF, DM = oracle.devs(F, M, mean8)
        wF, wM = ref.devs_exact(F, M, mean8)
        assert_bits(DF, wF, "DF")
        assert_bits(DM, wM, "DM")
    assert np.all(DF[:, 3] == -1.5) and np.all(DM[:, 3] == 2)                    # lane 3 is subtracted like the others
    F[::3, 0], F[1::3, 1], M[::2, 2], M[1::2, 3] = np.inf, -np.inf, np.nan, np.inf
    mean8 = np.array([np.inf, 1, 2, 0, 3, np.nan, 4, -np.inf], np.float32)
    DF, DM = oracle.devs(F, M, mean8)
    wF, wM = ref.devs_exact(F, M, mean8)
    assert_bits(DF, wF, "DF, non-finite")
    assert_bits(DM, wM, "DM, non-finite")


# ---- S ----------------------------------------------------------------------------------------------------------------------------
def check_s(oracle, m, c, salt=0):
    DM, DF = ref.deviations(m, salt)
    W = ref.weights_in(m, salt)
    out = []
    for w, name in ((W, "S_weighted"), (None, "S")):
        S = oracle.sij(DM, DF, w, c)
        want, scale = ref.s64(DM, DF, w, c)
        e = note(name, ref.s_err(S, want, scale))
        assert e <= TOL / EPS, (m, c, name, e)
        out.append((S, want))
    return out


@pytest.mark.parametrize("m", ref.M_S)
def test_s(oracle, m):
    (Sw, want_w), _ = check_s(oracle, m, 1e-6)
    if m == 16384:                              # the reference's check (4200 eps, absolute) at its size
        assert np.abs(Sw - want_w).max() <= 4200 * EPS


@pytest.mark.parametrize("m,c", ref.S_SCALINGS)
def test_s_scalings(oracle, m, c):
    (Sw, _), (Sr, _) = check_s(oracle, m, c, salt=1)
    if c == 0.0:
        assert_raw_bits(Sw, np.zeros(11, np.float32), "c = 0, weighted")
        assert_raw_bits(Sr, np.zeros(11, np.float32), "c = 0, regular")


@pytest.mark.parametrize("m", ref.M_PADDED)
def test_s_value_edges(oracle, m):
    DM, DF = ref.deviations(m, salt=2)
    assert_raw_bits(oracle.sij(DM, DF, np.zeros(m, np.float32), 1e-6), np.zeros(11, np.float32), "zero weights")
    big = (np.sign(DM) * np.float32(1e19)).astype(np.float32), (np.sign(DF) * np.float32(1e19)).astype(np.float32)
    fmax = float(np.finfo(np.float32).max)
    for w in (ref.weights_in(m, 2), None):       # products of 1e38: the sums of squares overflow, the mixed sums may (inf, or inf - inf = NaN)
        S = oracle.sij(big[0], big[1], w, 1.0)
        want, scale = ref.s64(big[0], big[1], w, 1.0)
        assert np.all(np.isposinf(S[9:])) and np.all(want[9:] > 2 * fmax), S
        for k in range(9):                       # a finite term is the float64 sum; a term can leave the finite range only where sum |term| does
            if np.isfinite(S[k]):
                assert abs(S[k] - want[k]) <= TOL * scale[k], (k, S[k], want[k])
            else:
                assert scale[k] > fmax, (k, S[k], scale[k])
        if m >= 2049:
            assert np.any(np.isnan(S[:9]))


# ---- representatives --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,nr", ref.REPS_CASES)
def test_reps(oracle, side, nr):
    F = ref.index_cloud(side)
    idx = ref.reps_index(side * side, nr)
    R, src = oracle.get_reps(F, nr)
    assert np.array_equal(src, idx)
    assert_raw_bits(R, F[idx], "R")
    assert oracle.reps_grid(side * side, nr) == ref.reps_grid_rule(side * side, nr)


def test_reps_grid_accepts_what_the_rule_accepts(oracle):
    for side in range(1, 25):
        m, nr = side * side, 1
        while nr <= m:
            assert oracle.reps_grid(m, nr) == ref.reps_grid_rule(m, nr), (side, nr)
            nr *= 2
        for bad_nr in (0, 3, m + 1, 2 * m):
            assert oracle.reps_grid(m, bad_nr) is None and ref.reps_grid_rule(m, bad_nr) is None
        if side > 1:
            assert oracle.reps_grid(m - 1, 1) is None and ref.reps_grid_rule(m - 1, 1) is None      # no square


# ---- landmarks --------------------------------------------------------------------------------------------------------------------
def test_landmarks(oracle):
    cloud = ref.pixel_cloud()
    want = ref.lms_exact(cloud)
    assert_raw_bits(oracle.get_lms(cloud), want, "landmarks")
    g = np.arange(16384)
    assert np.array_equal(want[:, 0], 65 + 4 * (g % 128)) and np.array_equal(want[:, 1], 49 + 3 * (g // 128))


# ---- transforms -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transform_clouds():
    return [ref.transform_cloud_in(0), ref.transform_cloud_in(1)]


@pytest.mark.parametrize("i", range(len(ref.TRANSFORM_N)), ids=["%d_%d" % (i, n) for i, n in enumerate(ref.TRANSFORM_N)])
def test_transforms(oracle, transform_clouds, i):
    n = ref.TRANSFORM_N[i]
    cloud = transform_clouds[ref.TRANSFORM_CLOUD_SEEDS[i]][:n]
    worst = ref.check_transforms(cloud, oracle.transform_q, oracle.transform_m)
    for kind, e in worst.items():
        note("transform_" + kind, e)
        assert e <= ref.TRANSFORM_TOL[kind], (n, kind, e)


def test_transforms_reference_literals_and_caps(oracle, transform_clouds):
    """The reference's own tolerances on U[0, 255) inputs (tests/testsICP.cpp:796-932: 4200 eps for the quaternion kinds, 42000 eps
    for the matrix kind, absolute) cap every finite case.  Its literal quaternion has four decimals, |q|^2 = 1 + 1.1e-5: there the
    two quaternion kinds already differ by (1 - |q|^2) s p, 1.2e-3 at these inputs — the term transform_q64 carries for variant 1."""
    cloud = transform_clouds[0][:1000]
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))
    q = np.array(kat["transform_quaternion"]["q"], np.float32)
    T = np.concatenate([q, [10, 20, 30, 0.5]]).astype(np.float32)
    gap = np.abs(ref.transform_q64(cloud, T, 1) - ref.transform_q64(cloud, T, 2)).max()
    qq = float(q.astype(np.float64) @ q.astype(np.float64))
    assert abs(gap - abs(1 - qq) * 0.5 * cloud[:, :3].max()) < 1e-9 and gap > 4200 * EPS
    for variant in (1, 2):
        assert np.abs(oracle.transform_q(cloud, T, variant)[:, :3] - ref.transform_q64(cloud, T, variant)).max() <= 4200 * EPS
    for name, T in ref.quaternion_transforms():
        for variant in (1, 2):
            assert np.abs(oracle.transform_q(cloud, T, variant)[:, :3] - ref.transform_q64(cloud, T, variant)).max() <= 4200 * EPS, name
    for name, T in ref.matrix_transforms():
        assert np.abs(oracle.transform_m(cloud, T)[:, :3] - ref.transform_m64(cloud, T)[0]).max() <= 42000 * EPS, name


def test_transforms_nonfinite_points_keep_their_lanes(oracle):
    pts = ref.nonfinite_points()
    for name, T in ref.quaternion_transforms():
        for variant in (1, 2):
            out = oracle.transform_q(pts, T, variant)
            assert_raw_bits(out[:, 3:], pts[:, 3:], name)
    for name, T in ref.matrix_transforms():
        assert_raw_bits(oracle.transform_m(pts, T)[:, 3:], pts[:, 3:], name)


def test_report_measured_worst_cases():
    """Prints the worst error per quantity of this session (pytest -s): the figures of the module's docstring."""
    print("\nworst errors in EPS: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
