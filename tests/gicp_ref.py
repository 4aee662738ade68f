"""Generalized ICP (icp_set_plane_to_plane, include/icp_amd.h: "plane-to-plane") restated in numpy.

pair_terms_gicp / pair_terms_gicp_robust follow the expression order of icp_gicp.hip so that the 27 terms of every pair are bit for
bit the engine's; everything behind them is point-to-plane's and comes from tests/p2pl_ref.py (the trees, LDL^T, the increment, the
composition and the convergence test), the robust loss's omega from tests/robust_ref.py.  Neither is edited.  numpy evaluates each
elementwise operation on its own (no fused multiply-add), as the engine does with -ffp-contract=off."""
import numpy as np

import p2pl_ref as p2pl
from p2pl_ref import grid_normals, reduce_terms, ldlt_solve, increment, compose, check_converged      # noqa: F401
import robust_ref

F32 = np.float32


def _d64(a):
    return np.asarray(a, F32).astype(np.float64)


def _lookup(normals, ids, m):
    """normals[ids] (m x 3 float32): zeros for an id beyond the set and for a non-finite normal."""
    ids = np.asarray(ids, np.uint32)
    N = np.zeros((m, 3), F32)
    inb = ids < m
    N[inb] = np.asarray(normals, F32)[ids[inb], :3]
    N[~np.isfinite(N).all(-1)] = 0
    return N


def covariance(nx, ny, nz, eps):
    """The covariance of a normal (float64 components), upper triangle [c00, c01, c02, c11, c12, c22]: delta_ab - k (n_a n_b) with
    k = (1 - eps) / nn where nn = |n|^2 is > 0 and finite, the identity elsewhere."""
    with np.errstate(all="ignore"):
        nn = (nx * nx + ny * ny) + nz * nz
        ok = (nn > 0) & np.isfinite(nn)
        k = (1.0 - eps) / nn
        C = [1.0 - k * (nx * nx), 0.0 - k * (nx * ny), 0.0 - k * (nx * nz), 1.0 - k * (ny * ny), 0.0 - k * (ny * nz), 1.0 - k * (nz * nz)]
    I = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    return [np.where(ok, c, i) for c, i in zip(C, I)]


def weight_matrix(NQ, NM, R, eps):
    """(M as a 3 x 3 list of (m,) float64 arrays, usable): M = (C_Q + C_P)^-1 by cofactors, N_P = R N_M; usable = det > 0 and finite."""
    eps = float(F32(eps))
    R = _d64(np.asarray(R, F32).ravel())
    nx, ny, nz = _d64(NQ[:, 0]), _d64(NQ[:, 1]), _d64(NQ[:, 2])
    mx, my, mz = _d64(NM[:, 0]), _d64(NM[:, 1]), _d64(NM[:, 2])
    with np.errstate(all="ignore"):
        CQ = covariance(nx, ny, nz, eps)
        CP = covariance((R[0] * mx + R[1] * my) + R[2] * mz, (R[3] * mx + R[4] * my) + R[5] * mz, (R[6] * mx + R[7] * my) + R[8] * mz, eps)
        s00, s01, s02, s11, s12, s22 = (a + b for a, b in zip(CQ, CP))
        c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
        c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
        det = (s00 * c00 + s01 * c01) + s02 * c02
        usable = (det > 0) & np.isfinite(det)
        M = [[c00 / det, c01 / det, c02 / det], [c01 / det, c11 / det, c12 / det], [c02 / det, c12 / det, c22 / det]]
    return M, usable


def _terms(PF, PM, ids, normals_f, normals_m, R, mu, eps, loss=None, scale=None):
    PF = np.asarray(PF, F32)
    PM = np.asarray(PM, F32)
    m = PF.shape[0]
    w32 = PF[:, 3]
    sel = w32 != 0
    NQ = _lookup(normals_f, ids, m)
    NM = _lookup(normals_m, np.arange(m, dtype=np.uint32), m)
    M, usable = weight_matrix(NQ, NM, R, eps)
    px, py, pz = _d64(PM[:, 0]), _d64(PM[:, 1]), _d64(PM[:, 2])
    qx, qy, qz = _d64(PF[:, 0]), _d64(PF[:, 1]), _d64(PF[:, 2])
    w, mu = _d64(w32), float(F32(mu))
    one, zero = np.ones(m), np.zeros(m)
    with np.errstate(all="ignore"):
        npx, npy, npz = -px, -py, -pz
        u = [[None] * 3 for _ in range(6)]
        for r in range(3):
            u[0][r] = M[r][1] * npz + M[r][2] * py
            u[1][r] = M[r][0] * pz + M[r][2] * npx
            u[2][r] = M[r][0] * npy + M[r][1] * px
            u[3][r], u[4][r], u[5][r] = M[r][0], M[r][1], M[r][2]
        dx, dy, dz = qx - px, qy - py, qz - pz
        pp = (px * px + py * py) + pz * pz
        G = [pp - px * px, -(px * py), -(px * pz), zero, -pz, py,
             pp - py * py, -(py * pz), pz, zero, -px,
             pp - pz * pz, -py, px, zero,
             one, zero, zero,
             one, zero,
             one]
        g = [py * qz - pz * qy, pz * qx - px * qz, px * qy - py * qx, dx, dy, dz]

        def hu(a, c):
            if a == 0:
                return npz * u[c][1] + py * u[c][2]
            if a == 1:
                return pz * u[c][0] + npx * u[c][2]
            if a == 2:
                return npy * u[c][0] + px * u[c][1]
            return u[c][a - 3]

        wG = None
        if loss is not None:
            ud = [(M[r][0] * dx + M[r][1] * dy) + M[r][2] * dz for r in range(3)]
            sG2 = ((ud[0] * dx + ud[1] * dy) + ud[2] * dz) + mu * ((dx * dx + dy * dy) + dz * dz)
            wG = robust_ref.omega(loss, sG2 / robust_ref.k2(scale))
        out = np.zeros((m, 27))
        t = 0
        for a in range(6):
            for c in range(a, 6):
                x = hu(a, c) + mu * G[t]
                out[:, t] = w * x if wG is None else w * np.where(wG != 0, wG * x, 0.0)
                t += 1
        for a in range(6):
            x = ((u[a][0] * dx + u[a][1] * dy) + u[a][2] * dz) + mu * g[a]
            out[:, 21 + a] = w * x if wG is None else w * np.where(wG != 0, wG * x, 0.0)
    out[~(sel & usable)] = 0.0
    return out


def pair_terms_gicp(PF, PM, ids, normals_f, normals_m, R, mu, eps):
    """(m, 27) float64: the plane-to-plane terms of every pair.  PF = NN output (xyz, w), PM = QT output (xyz), ids = NN_ID.id,
    normals_f = NORMALS_F, normals_m = NORMALS_M (query order), R = the cumulative rotation before the step (9 floats, row-major)."""
    return _terms(PF, PM, ids, normals_f, normals_m, R, mu, eps)


def pair_terms_gicp_robust(PF, PM, ids, normals_f, normals_m, R, mu, eps, loss, scale):
    """The same with a robust loss (robust_ref.HUBER / CAUCHY / TUKEY) of the scale `scale`."""
    return _terms(PF, PM, ids, normals_f, normals_m, R, mu, eps, loss, scale)


def step(PF, PM, ids, normals_f, normals_m, mu, eps, T, R, loss=None, scale=None):
    """One plane-to-plane iteration: (system[28], T', R', Tk, Rk).  Singular: the identity step (T, R unchanged)."""
    s = reduce_terms(_terms(PF, PM, ids, normals_f, normals_m, R, mu, eps, loss, scale))
    x, ok = ldlt_solve(s)
    system = np.concatenate([s, [1.0 if ok else 0.0]])
    if not ok:
        return system, np.asarray(T, F32).copy(), np.asarray(R, F32).copy(), p2pl.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    Tk = increment(x)
    Tn, Rn, Rk = compose(T, R, Tk)
    return system, Tn, Rn, Tk, Rk
