"""The point-to-plane and colored systems stated a second time, independently of tests/p2pl_ref.py's closed forms.

p2pl_ref.pair_terms and colored_ref.pair_terms copy the kernels' expressions for J, G, g and J_C term for term, so a wrong sign or a
swapped index would be in both and every bit-for-bit test would still pass.  Here the objective of include/icp_amd.h
(icp_set_error_metric, ICP_METRIC_COLORED) is written down as residual rows in float64, one pair at a time:
    sqrt(w) N . (P + omega x P + tau - Q)                         (one row)
    sqrt(w mu) (P + omega x P + tau - Q)                          (three rows)
    sqrt(w kappa) (C_Q + t . (P + omega x P + tau - Q) - C_P)     (one row, colored: t = d - (d . N) N)
The rows are affine in x = (omega, tau); the Jacobian is the linear part evaluated at the six unit vectors (np.cross, no closed form),
and the normal equations J^T J x = -J^T r0 must be the restatement's 27 sums.  ldlt_solve must be the least-squares solution of the
stacked rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_ref as cref                                      # noqa: E402
import p2pl_ref as ref                                          # noqa: E402
from p2pl_ref import unpack                                     # noqa: E402

F32 = np.float32
UPPER = [(a, c) for a in range(6) for c in range(a, 6)]          # the 21 upper-triangle terms, row-major


def lstsq_of_system(s):
    """(x, cond A) of the 27 sums by numpy's least squares (an independent solver of A x = b)."""
    A, b = unpack(s)
    return np.linalg.lstsq(A, b, rcond=None)[0], np.linalg.cond(A)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def make_pairs(rng, m, scale, w_zero=0.1, n_zero=0.1, n_nan=0.02):
    """Random float32 inputs in the engine's layout: PF = (Q, w), PM = (P, dist), ids, the fixed frame's normals (a table indexed by id).
    Some pairs have w = 0 (one of them with NaN coordinates: selected, not multiplied), some a zero or a non-finite normal."""
    centre = np.array([0.1, -0.2, 1.0]) * scale
    P = (centre + rng.normal(size=(m, 3)) * 0.3 * scale).astype(F32)
    Q = (P + rng.normal(size=(m, 3)) * 0.01 * scale).astype(F32)
    w = rng.uniform(0.2, 1.0, m).astype(F32)
    w[rng.random(m) < w_zero] = 0.0
    Nrm = rng.normal(size=(m, 3))
    Nrm = (Nrm / np.linalg.norm(Nrm, axis=1, keepdims=True)).astype(F32)
    Nrm[rng.random(m) < n_zero] = 0.0
    Nrm[rng.random(m) < n_nan, 1] = np.nan
    ids = rng.permutation(m).astype(np.uint32)
    table = np.zeros((m, 4), F32)
    table[ids, :3] = Nrm                                         # (normals[ids[i]] is pair i's normal)
    if m > 2:
        zero = np.nonzero(w == 0)[0]
        if zero.size:
            P[zero[0]] = np.nan
    PF = np.zeros((m, 4), F32)
    PF[:, :3], PF[:, 3] = Q, w
    PM = np.zeros((m, 4), F32)
    PM[:, :3] = P
    return PF, PM, ids, table


def make_colours(rng, m, ids, d_nan=0.02):
    """COLOR_GRAD_F table (d, C_Q) indexed by id and the moving landmarks M (m x 8, rgb in 4..6) in query order."""
    grads = np.zeros((m, 4), F32)
    d = (rng.normal(size=(m, 3)) * 0.02).astype(F32)
    d[rng.random(m) < d_nan, 2] = np.inf
    grads[ids, :3] = d
    grads[ids, 3] = rng.uniform(0.0, 1.0, m).astype(F32)
    M = np.zeros((m, 8), F32)
    M[:, 3] = 1.0
    M[:, 4:7] = rng.uniform(0.0, 1.0, (m, 3)).astype(F32)
    M[:, 7] = 1.0
    return grads, M


# ---- the objective as rows ----------------------------------------------------------------------------------------------------------

def _finite_or_zero(V):
    V = np.asarray(V, np.float64).copy()
    V[~np.isfinite(V).all(-1)] = 0.0
    return V


def rows(PF, PM, ids, normals, mu, x, affine, colour=None):
    """The residual rows of the selected pairs (w != 0) at x (6,) in float64: the linear part, plus the constant when `affine`.
    colour = (grads, M, kappa) adds the photometric row."""
    PF, PM = np.asarray(PF, F32), np.asarray(PM, F32)
    sel = PF[:, 3] != 0
    P = PM[sel, :3].astype(np.float64)
    Q = PF[sel, :3].astype(np.float64)
    w = PF[sel, 3].astype(np.float64)
    idx = np.asarray(ids)[sel]
    N = _finite_or_zero(np.asarray(normals, F32)[idx, :3])
    omega, tau = np.asarray(x[:3], np.float64), np.asarray(x[3:], np.float64)
    e = np.cross(omega, P) + tau                                  # the step's displacement of P
    if affine:
        e = e + (P - Q)
    mu = np.float64(F32(mu))
    out = [np.sqrt(w) * np.einsum("ij,ij->i", N, e)]
    out += [np.sqrt(w * mu) * e[:, k] for k in range(3)]
    if colour is not None:
        grads, M, kappa = colour
        G = np.asarray(grads, F32)[idx]
        d = _finite_or_zero(G[:, :3])
        t = d - np.einsum("ij,ij->i", d, N)[:, None] * N          # d in Q's tangent plane
        Mq = np.asarray(M, F32)[sel]
        CP = ((Mq[:, 4] + Mq[:, 5]) + Mq[:, 6]) / F32(3)          # the header's intensity, fp32
        ph = np.einsum("ij,ij->i", t, e)
        if affine:
            ph = ph + (G[:, 3].astype(np.float64) - CP.astype(np.float64))
        out.append(np.sqrt(w * np.float64(F32(kappa))) * ph)
    return np.concatenate(out)


def stacked(PF, PM, ids, normals, mu, colour=None):
    """(J, r0): the Jacobian by evaluating the linear part at the unit vectors, and the rows at x = 0."""
    J = np.stack([rows(PF, PM, ids, normals, mu, np.eye(6)[k], False, colour) for k in range(6)], axis=1)
    r0 = rows(PF, PM, ids, normals, mu, np.zeros(6), True, colour)
    return J, r0


def assert_same_system(s, J, r0, rtol=1e-12):
    """The 27 sums s against J^T J and -J^T r0, each entry to rtol of its Cauchy-Schwarz scale (sqrt(A_aa A_cc), sqrt(A_aa |r0|^2))."""
    A, b = unpack(s)
    A0, b0 = J.T @ J, -(J.T @ r0)
    dA = np.sqrt(np.outer(np.diag(A0), np.diag(A0)))
    db = np.sqrt(np.diag(A0) * (r0 @ r0))
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(b))
    badA = np.abs(A - A0) > rtol * dA
    assert not badA.any(), ("A", np.argwhere(badA)[:4].tolist(), A[badA][:4], A0[badA][:4])
    badb = np.abs(b - b0) > rtol * db
    assert not badb.any(), ("b", np.nonzero(badb)[0].tolist(), b[badb], b0[badb])


CASES = [  # (m, scale, mu, seed): sizes around the block of 256, metres and millimetres (|P| up to about 3000)
    (1, 1.0, 0.05, 1), (37, 1.0, 0.05, 2), (256, 1000.0, 0.0, 3), (1000, 3000.0, 0.05, 4), (5000, 1000.0, 1.0, 5),
    (70001, 3000.0, 0.05, 6),
]


# ---- 1. the system -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,scale,mu,seed", CASES)
def test_point_to_plane_system_is_the_objective(m, scale, mu, seed):
    rng = np.random.default_rng(seed)
    PF, PM, ids, normals = make_pairs(rng, m, scale)
    s = ref.reduce_terms(ref.pair_terms(PF, PM, ids, normals, mu))
    J, r0 = stacked(PF, PM, ids, normals, mu)
    assert_same_system(s, J, r0)


@pytest.mark.parametrize("m,scale,mu,seed", CASES)
@pytest.mark.parametrize("kappa", [0.0, 1000.0])
def test_colored_system_is_the_objective(m, scale, mu, seed, kappa):
    rng = np.random.default_rng(seed + 100)
    PF, PM, ids, normals = make_pairs(rng, m, scale)
    grads, M = make_colours(rng, m, ids)
    s = ref.reduce_terms(cref.pair_terms(PF, PM, ids, normals, grads, M, mu, kappa))
    J, r0 = stacked(PF, PM, ids, normals, mu, (grads, M, kappa))
    assert_same_system(s, J, r0)


def test_every_term_is_reached():
    """With mu > 0, large coordinates and the photometric row, no entry of A or b is zero: a swapped or dropped term cannot hide."""
    rng = np.random.default_rng(7)
    PF, PM, ids, normals = make_pairs(rng, 500, 3000.0, n_zero=0.0, n_nan=0.0)
    grads, M = make_colours(rng, 500, ids, d_nan=0.0)
    s = ref.reduce_terms(cref.pair_terms(PF, PM, ids, normals, grads, M, 0.05, 1000.0))
    assert np.all(s != 0.0)


def test_zero_weight_pairs_contribute_nothing():
    """Pairs with w = 0 and NaN coordinates leave the sums as the same set without them, bit for bit."""
    rng = np.random.default_rng(8)
    PF, PM, ids, normals = make_pairs(rng, 300, 1000.0, w_zero=0.0)
    s = ref.reduce_terms(ref.pair_terms(PF, PM, ids, normals, 0.05))
    PF2, PM2 = PF.copy(), PM.copy()
    PF2[::7, 3] = 0.0
    PF2[::7, 0] = np.nan
    PM2[::7, 1] = np.inf
    t = ref.reduce_terms(ref.pair_terms(PF2, PM2, ids, normals, 0.05))
    keep = np.ones(300, bool)
    keep[::7] = False
    assert np.all(np.isfinite(t))
    J, r0 = stacked(PF2, PM2, ids, normals, 0.05)
    assert J.shape[0] == 4 * np.count_nonzero(keep)
    assert_same_system(t, J, r0)
    assert not np.array_equal(s, t)


# ---- 2. the solve ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,scale,mu,seed", [c for c in CASES if c[0] >= 37])
@pytest.mark.parametrize("colored", [False, True])
def test_ldlt_solve_is_the_least_squares_solution(m, scale, mu, seed, colored):
    rng = np.random.default_rng(seed + 200)
    PF, PM, ids, normals = make_pairs(rng, m, scale)
    colour = None
    if colored:
        grads, M = make_colours(rng, m, ids)
        colour = (grads, M, 1000.0)
        s = ref.reduce_terms(cref.pair_terms(PF, PM, ids, normals, grads, M, mu, 1000.0))
    else:
        s = ref.reduce_terms(ref.pair_terms(PF, PM, ids, normals, mu))
    J, r0 = stacked(PF, PM, ids, normals, mu, colour)
    x_ls, _, rank, sv = np.linalg.lstsq(J, -r0, rcond=None)
    assert rank == 6
    x, ok = ref.ldlt_solve(s)
    assert ok
    cond = sv[0] / sv[-1]
    tol = 1e-14 * cond * cond + 1e-12                           # (LDL^T works on the normal equations: cond(J)^2)
    assert np.linalg.norm(np.array(x) - x_ls) <= tol * np.linalg.norm(x_ls), (x, x_ls, cond)


def test_ldlt_solve_refuses_a_rank_deficient_system():
    """One plane, every normal alike and mu = 0: the rows have rank 3 (omega about N and tau in the plane move nothing), and the solve
    reports the identity step."""
    rng = np.random.default_rng(9)
    m = 400
    P = np.zeros((m, 3), F32)
    P[:, :2] = rng.uniform(-500, 500, (m, 2))
    P[:, 2] = 1000.0
    Q = P.copy()
    Q[:, 2] += 3.0
    PF = np.concatenate([Q, np.ones((m, 1), F32)], 1)
    PM = np.concatenate([P, np.zeros((m, 1), F32)], 1)
    ids = np.arange(m, dtype=np.uint32)
    normals = np.zeros((m, 4), F32)
    normals[:, 2] = -1.0
    J, r0 = stacked(PF, PM, ids, normals, 0.0)
    assert np.linalg.matrix_rank(J) == 3
    s = ref.reduce_terms(ref.pair_terms(PF, PM, ids, normals, 0.0))
    assert_same_system(s, J, r0)
    _, ok = ref.ldlt_solve(s)
    assert not ok


def test_increment_of_the_lstsq_solution():
    """ref.increment's quaternion carries omega (2 qk / qk.w = omega) and tk carries tau, to float32 rounding."""
    rng = np.random.default_rng(10)
    PF, PM, ids, normals = make_pairs(rng, 2000, 1000.0)
    s = ref.reduce_terms(ref.pair_terms(PF, PM, ids, normals, 0.05))
    x, _ = lstsq_of_system(s)
    Tk = ref.increment(x)
    omega = 2.0 * Tk[:3].astype(np.float64) / np.float64(Tk[3])
    eps = np.finfo(F32).eps
    assert np.linalg.norm(omega - x[:3]) <= 4 * eps * np.linalg.norm(x[:3])
    assert np.linalg.norm(Tk[4:7] - x[3:]) <= 4 * eps * np.linalg.norm(x[3:])
