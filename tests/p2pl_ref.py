"""Point-to-plane ICP restated in numpy (the rule of include/icp_amd.h: icp_set_error_metric, icp_set_normals).

Every function follows the engine's expression order so that the results are bit for bit those of icp_p2pl.hip:
  - grid_normals:  ICP_NORMALS_GRID in float32;
  - pair_terms / reduce_terms:  the 27 per-pair terms in float64 and the two halving trees, by explicit halving;
  - ldlt_solve:  LDL^T and the two triangular solves in Python floats;
  - increment / compose / check_converged:  qk, tk, sk from the solution and the engine's composition (icp_compose) and
    convergence test (icp_check_converged) restated in float32.
numpy evaluates each elementwise operation on its own (no fused multiply-add), as the engine does with -ffp-contract=off."""
import math

import numpy as np

BLOCK = 256          # pairs per block of the first tree level (ICP_P2PL_BLOCK)
F32 = np.float32


# ---- ICP_NORMALS_GRID ------------------------------------------------------------------------------------------------------------

def _valid(P):
    with np.errstate(invalid="ignore"):
        return np.isfinite(P).all(-1) & ~(P == 0).all(-1)


def _axis_diff(prev, has_prev, c, nxt, has_next):
    """(difference, present): central if both neighbours are valid, else one-sided against the centre, the next neighbour first."""
    vp, vn = has_prev & _valid(prev), has_next & _valid(nxt)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where((vp & vn)[..., None], nxt - prev, np.where(vn[..., None], nxt - c, np.where(vp[..., None], c - prev, F32(0))))
    return d.astype(F32), vp | vn


def grid_normals(F, width):
    """NORMALS_F (m x 4 float32) of F (m x 8 or m x 3) read as a row-major grid `width` wide."""
    P = np.ascontiguousarray(np.asarray(F, F32)[:, :3])
    m = P.shape[0]
    assert m % width == 0
    H = m // width
    G = P.reshape(H, width, 3)
    zero = np.zeros_like(G)
    left = np.concatenate([zero[:, :1], G[:, :-1]], axis=1)
    right = np.concatenate([G[:, 1:], zero[:, :1]], axis=1)
    up = np.concatenate([zero[:1], G[:-1]], axis=0)
    down = np.concatenate([G[1:], zero[:1]], axis=0)
    x = np.arange(width)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(width, 1)
    dh, okh = _axis_diff(left, x > 0, G, right, x + 1 < width)
    dv, okv = _axis_diff(up, y > 0, G, down, y + 1 < H)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cx = dh[..., 1] * dv[..., 2] - dh[..., 2] * dv[..., 1]
        cy = dh[..., 2] * dv[..., 0] - dh[..., 0] * dv[..., 2]
        cz = dh[..., 0] * dv[..., 1] - dh[..., 1] * dv[..., 0]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        good = _valid(G) & okh & okv & (ln > 0) & (ln < np.inf)
        n = np.stack([cx / ln, cy / ln, cz / ln], -1).astype(F32)
        dot = (n[..., 0] * G[..., 0] + n[..., 1] * G[..., 1]) + n[..., 2] * G[..., 2]
    n = np.where((dot > 0)[..., None], -n, n)
    out = np.zeros((H, width, 4), F32)
    out[..., :3] = np.where(good[..., None], n, F32(0))
    return out.reshape(m, 4)


# ---- the system ------------------------------------------------------------------------------------------------------------------

def pair_terms(PF, PM, ids, normals, mu):
    """(m, 27) float64: the terms of every pair.  PF = NN output (xyz, w), PM = QT output (xyz), ids = NN_ID.id, normals = NORMALS_F."""
    PF = np.asarray(PF, F32)
    PM = np.asarray(PM, F32)
    m = PF.shape[0]
    w32 = PF[:, 3]
    sel = w32 != 0
    ids = np.asarray(ids, np.uint32)
    N = np.zeros((m, 3), F32)
    inb = ids < m
    N[inb] = np.asarray(normals, F32)[ids[inb], :3]
    N[~np.isfinite(N).all(-1)] = 0
    d64 = lambda a: a.astype(np.float64)
    px, py, pz = d64(PM[:, 0]), d64(PM[:, 1]), d64(PM[:, 2])
    qx, qy, qz = d64(PF[:, 0]), d64(PF[:, 1]), d64(PF[:, 2])
    nx, ny, nz = d64(N[:, 0]), d64(N[:, 1]), d64(N[:, 2])
    w, mu = d64(w32), float(np.float32(mu))
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
        out = np.zeros((m, 27))
        t = 0
        for a in range(6):
            for c in range(a, 6):
                out[:, t] = w * (J[a] * J[c] + mu * G[t])
                t += 1
        for a in range(6):
            out[:, 21 + a] = w * (J[a] * r + mu * g[a])
    out[~sel] = 0.0
    return out


def _halve(x):
    """Halving tree along axis 1 (its length a power of two): x[:, i] += x[:, i + h] for h = n/2 .. 1."""
    while x.shape[1] > 1:
        h = x.shape[1] // 2
        x = x[:, :h] + x[:, h:]
    return x[:, 0]


def reduce_terms(terms):
    """The 27 sums: halving trees inside blocks of BLOCK pairs, then over the block partials zero-padded to a power of two."""
    m = terms.shape[0]
    nblk = -(-m // BLOCK)
    x = np.zeros((nblk * BLOCK, 27))
    x[:m] = terms
    part = _halve(x.reshape(nblk, BLOCK, 27))          # (nblk, 27)
    P = 1
    while P < nblk:
        P *= 2
    y = np.zeros((P, 27))
    y[:nblk] = part
    return _halve(np.ascontiguousarray(y.T))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def ldlt_solve(s27):
    """(x[6], ok) for A x = b, A from its upper triangle row-major (s27[:21]), b = s27[21:], by LDL^T in the engine's order."""
    A = [[0.0] * 6 for _ in range(6)]
    t = 0
    for a in range(6):
        for c in range(a, 6):
            A[a][c] = A[c][a] = float(s27[t])
            t += 1
    b = [float(v) for v in s27[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    E = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ok = True
    for j in range(6):
        v = A[j][j]
        for k in range(j):
            v = v - E[j][k] * L[j][k]
        d[j] = v
        if not math.isfinite(v) or v <= 1e-12 * A[j][j]:
            ok = False
        for i in range(j + 1, 6):
            u = A[i][j]
            for k in range(j):
                u = u - L[i][k] * E[j][k]
            L[i][j] = _div(u, v)
            E[i][j] = L[i][j] * v
    y = [0.0] * 6
    for i in range(6):
        u = b[i]
        for k in range(i):
            u = u - L[i][k] * y[k]
        y[i] = u
    x = [0.0] * 6
    for i in range(5, -1, -1):
        u = _div(y[i], d[i])
        for k in range(i + 1, 6):
            u = u - L[k][i] * x[k]
        x[i] = u
    return x, ok


def increment(x):
    """Tk = [qk | tk, sk] (float32) from x = (omega, tau)."""
    hx, hy, hz = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    inv = 1.0 / math.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    return np.array([hx * inv, hy * inv, hz * inv, inv, x[3], x[4], x[5], 1.0], F32)


# ---- the engine's composition and check, float32 ----------------------------------------------------------------------------------

def quat_to_rot(q):
    x, y, z, w = (F32(v) for v in q)
    two, one = F32(2), F32(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([one - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, one - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, one - (txx + tyy)], F32)


def rot_to_quat(m):
    m = [F32(v) for v in m]
    q = [F32(0)] * 4
    half, one = F32(0.5), F32(1)
    t = (m[0] + m[4]) + m[8]
    if t > 0:
        t = np.sqrt(t + one)
        q[3] = half * t
        t = half / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i1 = m[4] > m[0]
        i2 = m[8] > (m[4] if i1 else m[0])
        i = 2 if i2 else (1 if i1 else 0)
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(((m[i * 4] - m[j * 4]) - m[k * 4]) + one)
        q[i] = half * t
        t = half / t
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return np.array(q, F32)


def compose(T, R, Tk):
    """icp_compose with Rk from qk: (T', R', Rk)."""
    T, R, Tk = np.asarray(T, F32), np.asarray(R, F32), np.asarray(Tk, F32)
    Rk = quat_to_rot(Tk[:4])
    sk = Tk[7]
    Rn = np.zeros(9, F32)
    for i in range(3):
        for j in range(3):
            Rn[i * 3 + j] = (Rk[i * 3] * R[j] + Rk[i * 3 + 1] * R[3 + j]) + Rk[i * 3 + 2] * R[6 + j]
    q = rot_to_quat(Rn)
    Tn = np.zeros(8, F32)
    Tn[:4] = q
    for i in range(3):
        r0, r1, r2 = sk * Rk[i * 3], sk * Rk[i * 3 + 1], sk * Rk[i * 3 + 2]
        Tn[4 + i] = ((r0 * T[4] + r1 * T[5]) + r2 * T[6]) + Tk[4 + i]
    Tn[7] = sk * T[7]
    return Tn, Rn, Rk


def check_converged(Tk, angle_threshold, translation_threshold):
    Tk = np.asarray(Tk, F32)
    vn = np.sqrt((Tk[0] * Tk[0] + Tk[1] * Tk[1]) + Tk[2] * Tk[2])
    tn = np.sqrt((Tk[4] * Tk[4] + Tk[5] * Tk[5]) + Tk[6] * Tk[6])
    tan_half = math.tan(angle_threshold * math.pi / 360.0)
    return bool(Tk[3] > 0 and float(vn) < float(Tk[3]) * tan_half and float(tn) < translation_threshold)


IDENTITY_TK = np.array([0, 0, 0, 1, 0, 0, 0, 1], F32)


def step(PF, PM, ids, normals, mu, T, R):
    """One point-to-plane iteration: (system[28], T', R', Tk, Rk).  Singular: the identity step (T, R unchanged)."""
    s = reduce_terms(pair_terms(PF, PM, ids, normals, mu))
    x, ok = ldlt_solve(s)
    system = np.concatenate([s, [1.0 if ok else 0.0]])
    if not ok:
        return system, np.asarray(T, F32).copy(), np.asarray(R, F32).copy(), IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    Tk = increment(x)
    Tn, Rn, Rk = compose(T, R, Tk)
    return system, Tn, Rn, Tk, Rk


UPPER = [(a, c) for a in range(6) for c in range(a, 6)]          # the 21 upper-triangle terms of a system, row-major


def unpack(s):
    """(A 6 x 6, b 6) of a 27-term system."""
    A = np.zeros((6, 6))
    for t, (a, c) in enumerate(UPPER):
        A[a, c] = A[c, a] = s[t]
    return A, np.asarray(s[21:27], np.float64)
