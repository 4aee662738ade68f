"""Colored ICP restated in numpy (the rule of include/icp_amd.h: ICP_METRIC_COLORED, icp_set_color_weight).

Every function follows the engine's expression order so that the results are bit for bit those of icp_p2pl.hip:
  - intensity:  C = ((r + g) + b) / 3 in float32;
  - grid_gradients:  COLOR_GRAD_F of ICP_NORMALS_GRID, the 3 x 3 least squares in float64 and its LDL^T, rounded to float32 once;
  - photometric:  d in Q's tangent plane, J_C and r_C of a pair in float64;
  - pair_terms:  the 27 per-pair terms of the colored system.
The trees, the 6 x 6 LDL^T, the increment, the composition and the convergence test are point-to-plane's: tests/p2pl_ref.py.
numpy evaluates each elementwise operation on its own (no fused multiply-add), as the engine does with -ffp-contract=off."""
import numpy as np

import p2pl_ref as p2pl

F32 = np.float32


def intensity(X):
    """C of landmarks X (n x 8 float32: [x y z 1 r g b 1]), float32."""
    X = np.asarray(X, F32)
    return ((X[:, 4] + X[:, 5]) + X[:, 6]) / F32(3)


# ---- COLOR_GRAD_F of ICP_NORMALS_GRID ------------------------------------------------------------------------------------------------

def _ldlt3(A, b):
    """Batched 3 x 3 LDL^T in k_p2pl_finalize's order: (x[3] arrays, ok).  A = dict (i, j) -> array for i <= j, b = [3 arrays]."""
    M = lambda i, j: A[(min(i, j), max(i, j))]
    L, E, d = {}, {}, [None] * 3
    ok = np.ones_like(b[0], dtype=bool)
    for j in range(3):
        v = M(j, j)
        for k in range(j):
            v = v - E[(j, k)] * L[(j, k)]
        d[j] = v
        ok &= np.isfinite(v) & ~(v <= 1e-12 * M(j, j))
        for i in range(j + 1, 3):
            u = M(i, j)
            for k in range(j):
                u = u - L[(i, k)] * E[(j, k)]
            L[(i, j)] = u / v
            E[(i, j)] = L[(i, j)] * v
    y = [None] * 3
    for i in range(3):
        u = b[i]
        for k in range(i):
            u = u - L[(i, k)] * y[k]
        y[i] = u
    x = [None] * 3
    for i in range(2, -1, -1):
        u = y[i] / d[i]
        for k in range(i + 1, 3):
            u = u - L[(k, i)] * x[k]
        x[i] = u
    return x, ok


def grid_gradients(F, normals, width):
    """COLOR_GRAD_F (m x 4 float32 [gx gy gz C]) of F (m x 8) read as a row-major grid `width` wide, with its NORMALS_F."""
    F = np.asarray(F, F32)
    m = F.shape[0]
    assert m % width == 0
    H, W = m // width, width
    P = F[:, :3].reshape(H, W, 3)
    C = intensity(F).reshape(H, W)
    N = np.asarray(normals, F32)[:, :3].reshape(H, W, 3)
    valid = p2pl._valid(P)
    d64 = lambda a: a.astype(np.float64)
    px, py, pz, pc = d64(P[..., 0]), d64(P[..., 1]), d64(P[..., 2]), d64(C)
    nx, ny, nz = d64(N[..., 0]), d64(N[..., 1]), d64(N[..., 2])
    z = np.zeros((H, W))
    A = {(0, 0): z, (0, 1): z, (0, 2): z, (1, 1): z, (1, 2): z, (2, 2): z}
    b = [z, z, z]
    K = np.zeros((H, W), np.int64)
    Pp = np.pad(P, ((1, 1), (1, 1), (0, 0)))
    Cp = np.pad(C, 1)
    Vp = np.pad(valid, 1)                                  # (outside the grid: not valid)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                Q = Pp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                use = Vp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                vx, vy, vz = d64(Q[..., 0]) - px, d64(Q[..., 1]) - py, d64(Q[..., 2]) - pz
                vn = (vx * nx + vy * ny) + vz * nz
                u = (vx - vn * nx, vy - vn * ny, vz - vn * nz)
                dC = d64(Cp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]) - pc
                for (i, j) in A:
                    A[(i, j)] = np.where(use, A[(i, j)] + u[i] * u[j], A[(i, j)])
                b = [np.where(use, b[i] + u[i] * dC, b[i]) for i in range(3)]
                K = K + use
        k = K.astype(np.float64)
        kn = (k * nx, k * ny, k * nz)
        for (i, j) in A:
            A[(i, j)] = A[(i, j)] + kn[i] * kn[j]
        x, ok = _ldlt3(A, b)
        g = np.stack([x[0], x[1], x[2]], -1).astype(F32)
    ok &= (K >= 3) & valid & ~(N == 0).all(-1)
    out = np.zeros((H, W, 4), F32)
    out[..., :3] = np.where(ok[..., None], g, F32(0))
    out[..., 3] = C
    return out.reshape(m, 4)


# ---- the pair terms -------------------------------------------------------------------------------------------------------------------

def photometric(P, Q, N, d, CQ, CP):
    """(J_C (6 arrays), r_C) in float64 from float64 arrays P, Q, N, d (3 each) and CQ, CP: the header's order."""
    px, py, pz = P
    qx, qy, qz = Q
    nx, ny, nz = N
    gx, gy, gz = d
    dn = (gx * nx + gy * ny) + gz * nz
    tx, ty, tz = gx - dn * nx, gy - dn * ny, gz - dn * nz
    JC = [py * tz - pz * ty, pz * tx - px * tz, px * ty - py * tx, tx, ty, tz]
    ex, ey, ez = px - qx, py - qy, pz - qz
    rc = CP - (CQ + ((tx * ex + ty * ey) + tz * ez))
    return JC, rc


def _lookup(table, ids, m):
    """table[ids] (float32 m x 4) with ids >= m as zeros and a non-finite xyz as zero xyz (.w kept)."""
    out = np.zeros((m, 4), F32)
    inb = ids < m
    out[inb] = np.asarray(table, F32)[ids[inb]]
    out[~np.isfinite(out[:, :3]).all(-1), :3] = 0
    return out


def pair_terms(PF, PM, ids, normals, grads, M, mu, kappa):
    """(m, 27) float64: the colored terms of every pair.  PF / PM / ids as p2pl_ref.pair_terms, grads = COLOR_GRAD_F, M = the moving
    landmarks (m x 8, query order)."""
    PF = np.asarray(PF, F32)
    PM = np.asarray(PM, F32)
    m = PF.shape[0]
    w32 = PF[:, 3]
    sel = w32 != 0
    ids = np.asarray(ids, np.uint32)
    N = _lookup(normals, ids, m)
    Gd = _lookup(grads, ids, m)
    d64 = lambda a: a.astype(np.float64)
    px, py, pz = d64(PM[:, 0]), d64(PM[:, 1]), d64(PM[:, 2])
    qx, qy, qz = d64(PF[:, 0]), d64(PF[:, 1]), d64(PF[:, 2])
    nx, ny, nz = d64(N[:, 0]), d64(N[:, 1]), d64(N[:, 2])
    w, mu, kappa = d64(w32), float(F32(mu)), float(F32(kappa))
    one, zero = np.ones(m), np.zeros(m)
    with np.errstate(all="ignore"):
        J = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
        dx, dy, dz = qx - px, qy - py, qz - pz
        r = (dx * nx + dy * ny) + dz * nz
        pp = (px * px + py * py) + pz * pz
        G = [pp - px * px, -(px * py), -(px * pz), zero, -pz, py,
             pp - py * py, -(py * pz), pz, zero, -px,
             pp - pz * pz, -py, px, zero,
             one, zero, zero,
             one, zero,
             one]
        g = [py * qz - pz * qy, pz * qx - px * qz, px * qy - py * qx, dx, dy, dz]
        JC, rc = photometric((px, py, pz), (qx, qy, qz), (nx, ny, nz), (d64(Gd[:, 0]), d64(Gd[:, 1]), d64(Gd[:, 2])),
                             d64(Gd[:, 3]), d64(intensity(M)))
        out = np.zeros((m, 27))
        t = 0
        for a in range(6):
            for c in range(a, 6):
                out[:, t] = w * ((J[a] * J[c] + mu * G[t]) + kappa * (JC[a] * JC[c]))
                t += 1
        for a in range(6):
            out[:, 21 + a] = w * ((J[a] * r + mu * g[a]) + kappa * (JC[a] * rc))
    out[~sel] = 0.0
    return out


def step(PF, PM, ids, normals, grads, M, mu, kappa, T, R):
    """One colored iteration: (system[28], T', R', Tk, Rk), point-to-plane's solve and composition (p2pl_ref)."""
    s = p2pl.reduce_terms(pair_terms(PF, PM, ids, normals, grads, M, mu, kappa))
    x, ok = p2pl.ldlt_solve(s)
    system = np.concatenate([s, [1.0 if ok else 0.0]])
    if not ok:
        return system, np.asarray(T, F32).copy(), np.asarray(R, F32).copy(), p2pl.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    Tk = p2pl.increment(x)
    Tn, Rn, Rk = p2pl.compose(T, R, Tk)
    return system, Tn, Rn, Tk, Rk
