"""The surface extraction of the TSDF volume restated in numpy (the rule of include/icp_amd.h: icp_tsdf_extract_surface), on the volumes
of tsdf_ref.py, and the analytic room corner to hold that rule against.

Everything of the rule is float32 with each operation on its own, as icp_tsdf_surface.hip evaluates it with -ffp-contract=off.  A plain
module: it collects no tests."""
import numpy as np

import tsdf_ref as T

F32 = np.float32


def usable(dw, min_weight=1.0):
    """(nz, ny, nx) bool: W >= min_weight and |D| < 1 (float comparisons: a NaN in either fails)."""
    with np.errstate(invalid="ignore"):
        return (dw[..., 1] >= F32(min_weight)) & (np.abs(dw[..., 0]) < F32(1))


def _shift(x, a, d):
    """x at v + d e_a (a = 0, 1, 2 for x, y, z), and where that voxel is inside the volume; x elsewhere is x's own value."""
    ax = 2 - a                                            # the arrays are (k, j, i, ..)
    inside = np.zeros(x.shape[:3], bool)
    out = x.copy()
    n = x.shape[ax]
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    src[ax], dst[ax] = (slice(d, n), slice(0, n - d)) if d > 0 else (slice(0, n + d), slice(-d, n))
    out[tuple(dst)] = x[tuple(src)]
    inside[tuple(dst[:3])] = True
    return out, inside


def gradient(dw):
    """(G (nz, ny, nx, 3), known (nz, ny, nx)): G_b (u) = D (u + e_b) - D (u - e_b), known iff all six neighbours are inside and have W > 0."""
    D, W = dw[..., 0], dw[..., 1]
    G = np.zeros(D.shape + (3,), F32)
    known = np.ones(D.shape, bool)
    with np.errstate(invalid="ignore"):
        for b in range(3):
            dp, ip = _shift(D, b, 1)
            dm, im = _shift(D, b, -1)
            wp, _ = _shift(W, b, 1)
            wm, _ = _shift(W, b, -1)
            G[..., b] = dp - dm
            known &= ip & im & (wp > 0) & (wm > 0)
    return G, known


def members(dw, min_weight=1.0):
    """[(nz, ny, nx) bool per axis]: edge (v, a) is a member."""
    D = dw[..., 0]
    ok = usable(dw, min_weight)
    out = []
    with np.errstate(invalid="ignore"):
        for a in range(3):
            d1, inside = _shift(D, a, 1)
            ok1, _ = _shift(ok, a, 1)
            out.append(inside & ok & ok1 & ((D > 0) != (d1 > 0)))
    return out


def extract(vol, min_weight=1.0, info=None):
    """(cloud (n, 8), normals (n, 4)) of a tsdf_ref.Volume, in the rule's order.  info: a dict that receives, per member, what the tests'
    conditions on their own inputs ask about: axis, index (n, 3) = (i, j, k) of the low voxel, t, grad_known (both ends' gradients are)."""
    c = vol.cfg
    dw = vol.dw
    D = dw[..., 0]
    nz, ny, nx = D.shape
    mem = members(dw, min_weight)
    G, known = gradient(dw)
    vx = F32(c["voxel"])
    recs = []
    for a in range(3):
        k, j, i = np.nonzero(mem[a])
        key = 3 * ((k * ny + j) * nx + i) + a
        hi = [k + (a == 2), j + (a == 1), i + (a == 0)]
        d0, d1 = D[k, j, i], D[hi[0], hi[1], hi[2]]
        with np.errstate(all="ignore"):
            t = d0 / (d0 - d1)
            idx = [i.astype(F32), j.astype(F32), k.astype(F32)]
            p = [F32(c["origin"][b]) + (idx[b] + t if b == a else idx[b]) * vx for b in range(3)]
            col = np.zeros((k.size, 3), F32)
            if vol.rgb is not None:
                c0, c1 = vol.rgb[k, j, i], vol.rgb[hi[0], hi[1], hi[2]]
                col = c0 + t[:, None] * (c1 - c0)
            g0, g1 = G[k, j, i], G[hi[0], hi[1], hi[2]]
            g = g0 + t[:, None] * (g1 - g0)
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            gk = known[k, j, i] & known[hi[0], hi[1], hi[2]]
            has_n = gk & (ln > 0)
            nrm = np.where(has_n[:, None], g / ln[:, None], F32(0))
        recs.append((key, p, col, nrm, t, gk, np.full(k.size, a), np.stack([i, j, k], 1)))
    key = np.concatenate([r[0] for r in recs])
    order = np.argsort(key, kind="stable")
    n = key.size
    cloud = np.zeros((n, 8), F32)
    cloud[:, 3] = cloud[:, 7] = 1
    for b in range(3):
        cloud[:, b] = np.concatenate([r[1][b] for r in recs])
    cloud[:, 4:7] = np.concatenate([r[2] for r in recs])
    normals = np.zeros((n, 4), F32)
    normals[:, :3] = np.concatenate([r[3] for r in recs])
    if info is not None:
        info.update(t=np.concatenate([r[4] for r in recs])[order], grad_known=np.concatenate([r[5] for r in recs])[order],
                    axis=np.concatenate([r[6] for r in recs])[order], index=np.concatenate([r[7] for r in recs])[order])
    return cloud[order], normals[order]


def edge_count(nx, ny, nz):
    return (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)


# ---- the analytic scene ---------------------------------------------------------------------------------------------------------------

def corner_surface_figures(cloud, normals):
    """What the CPU test asserts of the fused corner's surface: the points' distance from the nearest quarter-plane of the corner
    (x = 0, y = 0 or z = 0 with the other two coordinates >= 0), the share of points with a normal, and the angle (degrees) between the
    normal and the nearest plane's (e_plane, toward the room) on points more than 100 from a crease."""
    p = cloud[:, :3].astype(np.float64)
    q = np.maximum(p, 0.0)
    dist = np.empty((p.shape[0], 3))
    for a in range(3):
        foot = q.copy()
        foot[:, a] = 0.0
        dist[:, a] = np.linalg.norm(p - foot, axis=1)
    plane = np.argmin(dist, 1)
    d = dist[np.arange(p.shape[0]), plane]
    has_n = np.any(normals[:, :3] != 0, axis=1)
    crease = np.sort(np.abs(p), 1)[:, 1]                   # the distance from the second-nearest plane
    far = has_n & (crease > 100.0)
    cosang = np.clip(normals[np.arange(p.shape[0]), plane].astype(np.float64), -1, 1)
    return dict(count=p.shape[0], dist=d, normals=has_n.mean() if p.shape[0] else 0.0, angles=np.degrees(np.arccos(cosang[far])))
