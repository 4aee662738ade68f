"""Symmetric ICP (icp_set_symmetric, include/icp_amd.h; Rusinkiewicz 2019) restated in numpy.

pair_terms_sym / pair_terms_sym_robust follow the expression order of icp_symmetric.hip so that the 27 terms of every pair are bit for
bit the engine's, and increment_sym follows the symmetric branch of k_p2pl_finalize.  Everything else is point-to-plane's and comes from
tests/p2pl_ref.py (the trees, LDL^T, the composition and the convergence test), the robust loss's omega from tests/robust_ref.py.
Neither is edited.  numpy evaluates each elementwise operation on its own (no fused multiply-add), as the engine does with
-ffp-contract=off."""
import math

import numpy as np

import p2pl_ref as p2pl
from p2pl_ref import grid_normals, reduce_terms, ldlt_solve, compose, check_converged      # noqa: F401
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


def mean_normal(NQ, NM, R):
    """n = 0.5 (N_Q + N_P) as three (m,) float64 arrays: N_P = R N_M, negated where N_Q . N_P < 0."""
    R = _d64(np.asarray(R, F32).ravel())
    nqx, nqy, nqz = _d64(NQ[:, 0]), _d64(NQ[:, 1]), _d64(NQ[:, 2])
    mx, my, mz = _d64(NM[:, 0]), _d64(NM[:, 1]), _d64(NM[:, 2])
    with np.errstate(all="ignore"):
        npx = (R[0] * mx + R[1] * my) + R[2] * mz
        npy = (R[3] * mx + R[4] * my) + R[5] * mz
        npz = (R[6] * mx + R[7] * my) + R[8] * mz
        o = (nqx * npx + nqy * npy) + nqz * npz
        flip = o < 0
        npx, npy, npz = np.where(flip, -npx, npx), np.where(flip, -npy, npy), np.where(flip, -npz, npz)
        return (nqx + npx) * 0.5, (nqy + npy) * 0.5, (nqz + npz) * 0.5


def _terms(PF, PM, ids, normals_f, normals_m, R, mu, loss=None, scale=None):
    PF = np.asarray(PF, F32)
    PM = np.asarray(PM, F32)
    m = PF.shape[0]
    w32 = PF[:, 3]
    sel = w32 != 0
    NQ = _lookup(normals_f, ids, m)
    NM = _lookup(normals_m, np.arange(m, dtype=np.uint32), m)
    nx, ny, nz = mean_normal(NQ, NM, R)
    px, py, pz = _d64(PM[:, 0]), _d64(PM[:, 1]), _d64(PM[:, 2])
    qx, qy, qz = _d64(PF[:, 0]), _d64(PF[:, 1]), _d64(PF[:, 2])
    w, mu = _d64(w32), float(F32(mu))
    one, zero = np.ones(m), np.zeros(m)
    with np.errstate(all="ignore"):
        sx, sy, sz = px + qx, py + qy, pz + qz
        dx, dy, dz = qx - px, qy - py, qz - pz
        J = [sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz]
        r = (dx * nx + dy * ny) + dz * nz
        ss = (sx * sx + sy * sy) + sz * sz
        G = [ss - sx * sx, -(sx * sy), -(sx * sz), zero, -sz, sy,
             ss - sy * sy, -(sy * sz), sz, zero, -sx,
             ss - sz * sz, -sy, sx, zero,
             one, zero, zero,
             one, zero,
             one]
        g = [sy * dz - sz * dy, sz * dx - sx * dz, sx * dy - sy * dx, dx, dy, dz]
        wG = None
        if loss is not None:
            sG2 = r * r + mu * ((dx * dx + dy * dy) + dz * dz)
            wG = robust_ref.omega(loss, sG2 / robust_ref.k2(scale))
        out = np.zeros((m, 27))
        t = 0
        for a in range(6):
            for c in range(a, 6):
                x = J[a] * J[c] + mu * G[t]
                out[:, t] = w * x if wG is None else w * np.where(wG != 0, wG * x, 0.0)
                t += 1
        for a in range(6):
            x = J[a] * r + mu * g[a]
            out[:, 21 + a] = w * x if wG is None else w * np.where(wG != 0, wG * x, 0.0)
    out[~sel] = 0.0
    return out


def pair_terms_sym(PF, PM, ids, normals_f, normals_m, R, mu):
    """(m, 27) float64: the symmetric terms of every pair.  PF = NN output (xyz, w), PM = QT output (xyz), ids = NN_ID.id,
    normals_f = NORMALS_F, normals_m = NORMALS_M (query order), R = the cumulative rotation before the step (9 floats, row-major)."""
    return _terms(PF, PM, ids, normals_f, normals_m, R, mu)


def pair_terms_sym_robust(PF, PM, ids, normals_f, normals_m, R, mu, loss, scale):
    """The same with a robust loss (robust_ref.HUBER / CAUCHY / TUKEY) of the scale `scale`."""
    return _terms(PF, PM, ids, normals_f, normals_m, R, mu, loss, scale)


def increment_sym(x):
    """Tk = [qk | tk, sk] (float32) from x = (a, t): qk the rotation by 2 theta about a with tan theta = |a|, tk = R_a (cos theta t)."""
    ax, ay, az, tx, ty, tz = (float(v) for v in x)
    aa = (ax * ax + ay * ay) + az * az
    c = 1.0 / math.sqrt(aa + 1.0)
    ux, uy, uz = ay * tz - az * ty, az * tx - ax * tz, ax * ty - ay * tx
    at = (ax * tx + ay * ty) + az * tz
    c2 = c * c
    k3 = (c2 * c) / (1.0 + c)
    return np.array([ax * c, ay * c, az * c, c,
                     (c2 * tx + c2 * ux) + ax * (at * k3), (c2 * ty + c2 * uy) + ay * (at * k3), (c2 * tz + c2 * uz) + az * (at * k3),
                     1.0], F32)


def step(PF, PM, ids, normals_f, normals_m, mu, T, R, loss=None, scale=None):
    """One symmetric iteration: (system[28], T', R', Tk, Rk).  Singular: the identity step (T, R unchanged)."""
    s = reduce_terms(_terms(PF, PM, ids, normals_f, normals_m, R, mu, loss, scale))
    x, ok = ldlt_solve(s)
    system = np.concatenate([s, [1.0 if ok else 0.0]])
    if not ok:
        return system, np.asarray(T, F32).copy(), np.asarray(R, F32).copy(), p2pl.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    Tk = increment_sym(x)
    Tn, Rn, Rk = compose(T, R, Tk)
    return system, Tn, Rn, Tk, Rk
