"""Boundary and normal rejection restated in numpy (the rule of include/icp_amd.h: icp_set_boundary_rejection,
icp_set_normal_rejection; the engine's pass is icp_amd/csrc/icp_pair_filter.hip).

  - boundary_mask:  which fixed points of a row-major grid are boundary points (rim, invalid, beside an invalid point);
  - cosine_terms / compatible:  qq, pp, o in float64 from the float32 normals and R, each expression in the rule's order (numpy
    evaluates every elementwise operation on its own, as the engine does with -ffp-contract=off), and the comparison;
  - pair_filter:  the three masks and (n, at_boundary, incompatible, accepted) from the engine's own NN_ID ids, the weights before
    the rules (tests/test_gpu_trimming.py: weights_before_trim), F, NORMALS_F / NORMALS_M and R as read back."""
import numpy as np

F32, F64 = np.float32, np.float64


def valid(P):
    """xyz finite and not (0, 0, 0) — the icp_set_normals rule."""
    P = np.asarray(P, F32)[..., :3]
    with np.errstate(invalid="ignore"):
        return np.isfinite(P).all(-1) & ~(P == 0).all(-1)


def boundary_mask(F, gw):
    """bool[m]: fixed point id = (x, y) = (id % gw, id // gw) is a boundary point."""
    m = np.asarray(F).shape[0]
    assert gw > 0 and m % gw == 0
    rows = m // gw
    ok = valid(F).reshape(rows, gw)
    pad = np.zeros((rows + 2, gw + 2), bool)             # (outside the grid counts as invalid: the rim is boundary anyway)
    pad[1:-1, 1:-1] = ok
    allok = np.ones((rows, gw), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            allok &= pad[dy:dy + rows, dx:dx + gw]
    return ~allok.reshape(m)


def _finite_or_zero(N):
    N = np.array(np.asarray(N, F32)[:, :3], F32)
    N[~np.isfinite(N).all(-1)] = 0
    return N.astype(F64)


def cosine_terms(NQ, NM, R):
    """(qq, pp, o) in float64: N_P = R N_M with each component (R_a0 mx + R_a1 my) + R_a2 mz."""
    q, mv = _finite_or_zero(NQ), _finite_or_zero(NM)
    R = np.asarray(R, F32).reshape(3, 3).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([(R[a, 0] * mv[:, 0] + R[a, 1] * mv[:, 1]) + R[a, 2] * mv[:, 2] for a in range(3)], -1)
        qq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        o = (q[:, 0] * p[:, 0] + q[:, 1] * p[:, 1]) + q[:, 2] * p[:, 2]
    return qq, pp, o


def compatible_from_terms(qq, pp, o, min_cos):
    with np.errstate(invalid="ignore", over="ignore"):
        return (qq > 0) & (pp > 0) & (o >= F64(F32(min_cos)) * np.sqrt(qq * pp))


def compatible(NQ, NM, R, min_cos):
    """bool per pair: NQ = NORMALS_F[id], NM = NORMALS_M[i]."""
    return compatible_from_terms(*cosine_terms(NQ, NM, R), min_cos)


def cosines(NQ, NM, R):
    """o / sqrt (qq pp) per pair (NaN without both normals): for choosing a threshold from data, not part of the rule."""
    qq, pp, o = cosine_terms(NQ, NM, R)
    with np.errstate(invalid="ignore", divide="ignore"):
        return o / np.sqrt(qq * pp)


def pair_filter(ids, W0, F=None, gw=None, normals_f=None, normals_m=None, R=None, min_cos=None):
    """(at_boundary, incompatible, accepted, counts).  gw None / 0: the boundary rule is off; min_cos None: the normal rule is off."""
    ids = np.asarray(ids).astype(np.int64)
    n = ids.shape[0]
    m = np.asarray(F).shape[0] if F is not None else np.asarray(normals_f).shape[0] if normals_f is not None else n      # |F| (the engine: |F| = |M|)
    cand = (np.asarray(W0) != 0) & (ids < m)
    safe = np.where(ids < m, ids, 0)
    bnd = np.zeros(n, bool)
    if gw:
        bnd = cand & boundary_mask(F, gw)[safe]
    inc = np.zeros(n, bool)
    if min_cos is not None:
        inc = cand & ~bnd & ~compatible(np.asarray(normals_f)[safe], normals_m, R, min_cos)
    acc = cand & ~bnd & ~inc
    counts = np.array([np.count_nonzero(cand), np.count_nonzero(bnd), np.count_nonzero(inc), np.count_nonzero(acc)], np.uint32)
    return bnd, inc, acc, counts
