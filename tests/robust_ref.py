"""The robust loss (icp_set_robust_loss, include/icp_amd.h) restated in numpy: the IRLS weight omega, the point-to-point weights W',
the weighted plane terms (point-to-plane and colored), and sum W of the reference-order weights over arbitrary weights.

Takes the plane system's trees, LDL^T and composition from tests/p2pl_ref.py and the photometric pieces from tests/colored_ref.py
(neither is edited); the geometric pair pieces are restated here because the weights act inside the terms."""
import numpy as np

import colored_ref
import p2pl_ref as p2pl

F32 = np.float32
NONE, HUBER, CAUCHY, TUKEY = 0, 1, 2, 3
LOSSES = {"huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY}


def omega(loss, u):
    """omega (u) in float64 by the header's formulas, in the order written; 0 where u is NaN."""
    u = np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        if loss == HUBER:
            w = np.where(u <= 1.0, 1.0, 1.0 / np.sqrt(u))
        elif loss == CAUCHY:
            w = 1.0 / (1.0 + u)
        elif loss == TUKEY:
            w = np.where(u < 1.0, (1.0 - u) * (1.0 - u), 0.0)
        else:
            raise ValueError(loss)
    return np.where(np.isnan(u), 0.0, w)


def rho(loss, s, k):
    """The loss rho (s) whose IRLS weight omega is (rho'(s) / s), in float64."""
    s, k = np.asarray(s, np.float64), float(k)
    if loss == HUBER:
        return np.where(s <= k, s * s / 2, k * s - k * k / 2)
    if loss == CAUCHY:
        return (k * k / 2) * np.log1p(s * s / (k * k))
    if loss == TUKEY:
        return np.where(s <= k, (k * k / 6) * (1 - (1 - s * s / (k * k)) ** 3), k * k / 6)
    raise ValueError(loss)


def k2(scale):
    k = float(F32(scale))
    return k * k


def geo(PF, PM):
    """The rejection rule's geo in fp32: (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2, summed in that order."""
    g = (np.asarray(PM, F32)[:, :3] - np.asarray(PF, F32)[:, :3]).astype(F32)
    return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def p2p_weights(W0, PF, PM, loss, scale):
    """W' = (float) ((double) w * omega (geo / k^2)) for the pairs with w != 0 and a finite geo (W0: the weights after rejection and
    trimming), +0 for every other pair."""
    W0 = np.asarray(W0, F32)
    g = geo(PF, PM)
    cand = (W0 != 0) & np.isfinite(g)
    with np.errstate(all="ignore"):
        W = (W0.astype(np.float64) * omega(loss, g.astype(np.float64) / k2(scale))).astype(F32)
    W[~cand] = 0.0
    return W


def _tree_f(x):
    """The oracle's tree_f over 128 floats: x[i] += x[i + d] for d = 64 .. 1, in fp32."""
    x = x.copy()
    d = x.shape[-1] // 2
    while d > 0:
        x[..., :d] = x[..., :d] + x[..., d:2 * d]
        d //= 2
    return x[..., 0]


def sum_w_reference(W):
    """sum W of the reference-order reduction (orc_weights' tree) over arbitrary weights: tree_f per group of 128, groups padded to a
    multiple of 4 unless one; one group: its float; else chunks of 4 x 128 partials, each ((x + y) + z) + w in double and the chunk's
    128 such sums halved, the chunks summed in index order."""
    W = np.asarray(W, F32)
    n = W.shape[0]
    wg = -(-n // 128)
    wgp = wg if wg == 1 or wg % 4 == 0 else wg + 4 - wg % 4
    x = np.zeros(wgp * 128, F32)
    x[:n] = W
    part = _tree_f(x.reshape(wgp, 128))
    if wgp == 1:
        return float(part[0])
    total = None
    for c0 in range(0, wgp, 4 * 128):
        dd = np.zeros(128)
        for p in range(128):
            i4 = c0 + 4 * p
            if i4 < wgp:
                a, b, c, d = (float(v) for v in part[i4:i4 + 4])
                dd[p] = ((a + b) + c) + d
        d = 64
        while d > 0:
            dd[:d] = dd[:d] + dd[d:2 * d]
            d //= 2
        total = dd[0] if total is None else total + dd[0]
    return float(total)


def plane_terms(PF, PM, ids, normals, mu, loss, scale, grads=None, M=None, kappa=0.0):
    """(m, 27) float64: the robust plane terms of every pair (colored when grads is given), PF / PM / ids as p2pl_ref.pair_terms."""
    PF = np.asarray(PF, F32)
    PM = np.asarray(PM, F32)
    m = PF.shape[0]
    w32 = PF[:, 3]
    sel = w32 != 0
    ids = np.asarray(ids, np.uint32)
    N = colored_ref._lookup(np.asarray(normals, F32), ids, m)
    d64 = lambda a: a.astype(np.float64)
    px, py, pz = d64(PM[:, 0]), d64(PM[:, 1]), d64(PM[:, 2])
    qx, qy, qz = d64(PF[:, 0]), d64(PF[:, 1]), d64(PF[:, 2])
    nx, ny, nz = d64(N[:, 0]), d64(N[:, 1]), d64(N[:, 2])
    w, mu, kk = d64(w32), float(F32(mu)), k2(scale)
    one, zero = np.ones(m), np.zeros(m)
    colored = grads is not None
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
        wG = omega(loss, (r * r + mu * ((dx * dx + dy * dy) + dz * dz)) / kk)
        if colored:
            kappa = float(F32(kappa))
            Gd = colored_ref._lookup(np.asarray(grads, F32), ids, m)
            JC, rc = colored_ref.photometric((px, py, pz), (qx, qy, qz), (nx, ny, nz), (d64(Gd[:, 0]), d64(Gd[:, 1]), d64(Gd[:, 2])),
                                             d64(Gd[:, 3]), d64(colored_ref.intensity(M)))
            wC = omega(loss, (kappa * (rc * rc)) / kk)
            kwC = kappa * wC
        out = np.zeros((m, 27))
        t = 0
        for a in range(6):
            for c in range(a, 6):
                x = np.where(wG != 0, wG * (J[a] * J[c] + mu * G[t]), 0.0)
                if colored:
                    x = x + np.where(wC != 0, kwC * (JC[a] * JC[c]), 0.0)
                out[:, t] = w * x
                t += 1
        for a in range(6):
            x = np.where(wG != 0, wG * (J[a] * r + mu * g[a]), 0.0)
            if colored:
                x = x + np.where(wC != 0, kwC * (JC[a] * rc), 0.0)
            out[:, 21 + a] = w * x
    out[~sel] = 0.0
    return out


def plane_step(PF, PM, ids, normals, mu, loss, scale, T, R, grads=None, M=None, kappa=0.0):
    """One robust plane iteration: (system[28], T', R', Tk, Rk), point-to-plane's trees, solve and composition (p2pl_ref)."""
    s = p2pl.reduce_terms(plane_terms(PF, PM, ids, normals, mu, loss, scale, grads, M, kappa))
    x, ok = p2pl.ldlt_solve(s)
    system = np.concatenate([s, [1.0 if ok else 0.0]])
    if not ok:
        return system, np.asarray(T, F32).copy(), np.asarray(R, F32).copy(), p2pl.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    Tk = p2pl.increment(x)
    Tn, Rn, Rk = p2pl.compose(T, R, Tk)
    return system, Tn, Rn, Tk, Rk


# ---- the edge scene: pairs whose u = s2 / k2 is known to the bit ----------------------------------------------------------------------

IDENTITY_T = np.array([0, 0, 0, 1, 0, 0, 0, 1], F32)
EDGE_CLASSES = ("zero", "at_k", "below_k", "above_k", "half_k", "two_k", "subnormal_geo", "far")


def edge_offsets(k):
    """The eight z offsets of the edge scene for the scale k (fp32): 0, k, one ulp below and above k, k / 2, 2 k, 1e-20 (its square is
    a float subnormal) and 192 (a far outlier); named by EDGE_CLASSES."""
    k = F32(k)
    return np.array([0.0, k, np.nextafter(k, F32(0)), np.nextafter(k, F32(np.inf)), k / F32(2), F32(2) * k, F32(1e-20), 192.0], F32)


def edge_scene(side, template, offsets):
    """(F, M, class of every point): F a flat grid x = 64 (col + 1), y = 64 (row + 1), z = 0 of one colour (the other words as in
    `template`, m x 8), M = F with z = offsets[i % len (offsets)].  Under the identity transform geo of pair i is fp32 (offset^2) exactly
    and every query's nearest neighbour is its own index (the grid step, 64, is far above every offset's share)."""
    m = side * side
    F = np.array(template, F32).reshape(m, 8).copy()
    i = np.arange(m)
    F[:, 0] = 64.0 * (i % side + 1)
    F[:, 1] = 64.0 * (i // side + 1)
    F[:, 2] = 0.0
    F[:, 4:7] = 0.5
    cls = i % len(offsets)
    M = F.copy()
    M[:, 2] = np.asarray(offsets, F32)[cls]
    return F, M, cls


def edge_geo(offsets):
    """geo of each class in fp32: (0 * 0 + 0 * 0) + o * o."""
    o = np.asarray(offsets, F32)
    return (o * o).astype(F32)


def intensity_channel(target):
    """A float32 r with ((r + 0) + 0) / 3 == target in fp32 (colored_ref.intensity of the colour (r, 0, 0)), searched among the floats
    next to 3 * target; None when there is none."""
    target = F32(target)
    r = F32(3) * target
    lo = hi = r
    for _ in range(8):
        for c in (lo, hi):
            if F32(c) / F32(3) == target:
                return F32(c)
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    return None
