"""Registration quality restated in numpy (the rule of include/icp_amd.h: icp_evaluate) — TEST INFRASTRUCTURE, collects nothing.

Every function follows the engine's expression order so that the results are bit for bit those of icp_quality.hip:
  - geo in float32, (gx gx + gy gy) + gz gz;
  - the 22 terms of a pair in float64: the 21 upper-triangle entries, row-major, of G about the fixed point, then geo;
  - the two halving trees of the plane system (p2pl_ref._halve over blocks of p2pl_ref.BLOCK pairs, then over the block partials
    zero-padded to a power of two);
  - fitness and the inlier RMSE by the host formulas in float64.
numpy evaluates each elementwise operation on its own (no fused multiply-add), as the engine does with -ffp-contract=off."""
import collections
import math

import numpy as np

from p2pl_ref import BLOCK, _halve

F32 = np.float32
TERMS = 22

Quality = collections.namedtuple("Quality", "sums n_moving n_inliers fitness inlier_rmse information counted inlier geo")
Quality.__doc__ = """sums: the 22 float64 sums (21 of G, then sum_geo);  information: the symmetric 6 x 6;  counted / inlier: the masks
per pair;  geo: float32 per pair."""


def threshold(max_dist):
    """(distance test on, (float) ((double) max_dist * max_dist)) of a max_dist as the C interface takes it (a float)."""
    md = F32(0.0 if max_dist is None else max_dist)
    on = bool(md > 0 and np.isfinite(md))
    return on, F32(np.float64(md) * np.float64(md)) if on else F32(0)


def geo_of(PF, PM):
    with np.errstate(all="ignore"):
        g = (np.asarray(PM, F32)[:, :3] - np.asarray(PF, F32)[:, :3]).astype(F32)
        return ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F32)


def masks(M, PF, PM, max_dist):
    """(counted, inlier, geo): M = the moving set as written (m x 8), PF / PM = the search's fixed / transformed moving points."""
    M, PF = np.asarray(M, F32), np.asarray(PF, F32)
    with np.errstate(all="ignore"):
        counted = np.isfinite(M[:, :3]).all(axis=1) & ~(M[:, :3] == 0).all(axis=1)
        geo = geo_of(PF, PM)
        inlier = counted & ~(PF[:, :3] == 0).all(axis=1) & np.isfinite(geo)
        on, d2 = threshold(max_dist)
        if on:
            inlier &= geo <= d2
    return counted, inlier, geo


def pair_terms(PF, inlier, geo):
    """(m, 22) float64: G about Q = PF.xyz (plane_point_share's G with Q in A's place), then geo; exact zeros where no inlier."""
    PF = np.asarray(PF, F32)
    m = PF.shape[0]
    d64 = lambda a: a.astype(np.float64)
    qx, qy, qz = d64(PF[:, 0]), d64(PF[:, 1]), d64(PF[:, 2])
    one, zero = np.ones(m), np.zeros(m)
    with np.errstate(all="ignore"):
        qq = (qx * qx + qy * qy) + qz * qz
        G = [qq - qx * qx, -(qx * qy), -(qx * qz), zero, -qz, qy,
             qq - qy * qy, -(qy * qz), qz, zero, -qx,
             qq - qz * qz, -qy, qx, zero,
             one, zero, zero,
             one, zero,
             one]
        out = np.zeros((m, TERMS))
        for t in range(21):
            out[:, t] = G[t]
        out[:, 21] = d64(geo)
    out[~inlier] = 0.0
    return out


def reduce_terms(terms):
    """The sums of the columns: halving trees inside blocks of BLOCK pairs, then over the block partials zero-padded to a power of two."""
    m, nt = terms.shape
    nblk = -(-m // BLOCK)
    x = np.zeros((nblk * BLOCK, nt))
    x[:m] = terms
    part = _halve(x.reshape(nblk, BLOCK, nt))            # (nblk, nt)
    P = 1
    while P < nblk:
        P *= 2
    y = np.zeros((P, nt))
    y[:nblk] = part
    return _halve(np.ascontiguousarray(y.T))


def information_of(sums):
    A = np.zeros((6, 6))
    t = 0
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = sums[t]
            t += 1
    return A


def host_numbers(sum_geo, n_moving, n_inliers):
    """(fitness, inlier_rmse) in float64 by the host formulas."""
    fitness = float(np.float64(n_inliers) / np.float64(n_moving)) if n_moving else 0.0
    rmse = float(np.sqrt(np.float64(sum_geo) / np.float64(n_inliers))) if n_inliers else 0.0
    return fitness, rmse


def evaluate(M, PF, PM, max_dist):
    counted, inlier, geo = masks(M, PF, PM, max_dist)
    sums = reduce_terms(pair_terms(PF, inlier, geo))
    nm, ni = int(np.count_nonzero(counted)), int(np.count_nonzero(inlier))
    fitness, rmse = host_numbers(sums[21], nm, ni)
    return Quality(sums, nm, ni, fitness, rmse, information_of(sums), counted, inlier, geo)


def sums_of(q):
    """The 22 device sums as the record carries them: the upper triangle of `information`, row-major, then sum_geo."""
    A = q.information_matrix()
    return np.array([A[a, c] for a in range(6) for c in range(a, 6)] + [q.sum_geo])


def check_record(q, want, m, what):
    """A device record (icp_quality_t) against evaluate's Quality: the counts exactly, the 22 sums and the information matrix by
    their bits, fitness and the inlier RMSE within 1 ulp of the host formula."""
    import icp_checks as K                               # (icp_checks imports this module through pairs_ref)
    print(what, "device", q.n_moving, q.n_inliers, q.fitness, q.inlier_rmse, "reference", want.n_moving, want.n_inliers, want.fitness, want.inlier_rmse)
    assert (q.n, q.n_moving, q.n_inliers, q.reserved) == (m, want.n_moving, want.n_inliers, 0), (what, q.n, q.n_moving, q.n_inliers)
    K.assert_bits(sums_of(q), want.sums, "%s: the 22 sums" % what)
    A = q.information_matrix()
    assert np.array_equal(A, A.T) and not np.isnan(A).any(), what
    K.assert_bits(A, want.information, "%s: information" % what)
    fitness, rmse = host_numbers(q.sum_geo, q.n_moving, q.n_inliers)
    assert abs(q.fitness - fitness) <= np.spacing(fitness), (what, q.fitness, fitness)
    assert abs(q.inlier_rmse - rmse) <= np.spacing(rmse), (what, q.inlier_rmse, rmse)


def independent(PF, inlier, geo):
    """An independent float64 statement: Open3D's three rows of G per pair, G^T G, every entry and geo summed with math.fsum.
    Returns (6 x 6 information, sum_geo)."""
    PF = np.asarray(PF, np.float64)
    idx = np.nonzero(inlier)[0]
    mats = np.zeros((idx.size, 6, 6))
    for n, i in enumerate(idx):
        x, y, z = PF[i, 0], PF[i, 1], PF[i, 2]
        G = np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]])
        mats[n] = G.T @ G
    A = np.array([[math.fsum(mats[:, a, c]) for c in range(6)] for a in range(6)])
    return A, math.fsum(np.asarray(geo, np.float64)[idx])
