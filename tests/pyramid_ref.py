"""The pyramid rule of include/icp_amd.h (icp_pyramid_*) restated in numpy: the reduction of a level from the one below it, the chain
of levels, and the coarse-to-fine chain of registrations on the CPU oracle.  Test infrastructure: nothing here touches the engine."""
import numpy as np

MEAN, PICK = 0, 1
F32 = np.float32


def valid(X):
    """The icp_set_normals rule: xyz finite and not (0, 0, 0).  X: (.., 8)."""
    xyz = X[..., :3]
    return np.isfinite(xyz).all(axis=-1) & ~(xyz == 0).all(axis=-1)


def band_of(max_dz, l):
    """band_l = max_dz * (float) (1u << (l - 1)) in fp32; None: no band test (max_dz 0 or +inf)."""
    max_dz = F32(max_dz)
    if max_dz == 0 or np.isinf(max_dz):
        return None
    with np.errstate(over="ignore"):
        return F32(max_dz * F32(1 << (l - 1)))


def blocks_of(X, side):
    """(side/2, side/2, 4, 8): the 2 x 2 blocks of a row-major side x side level in block order (2x,2y) (2x+1,2y) (2x,2y+1) (2x+1,2y+1)."""
    G = np.ascontiguousarray(X, F32).reshape(side, side, 8)
    return np.stack([G[0::2, 0::2], G[0::2, 1::2], G[1::2, 0::2], G[1::2, 1::2]], axis=2)


def included(B, band):
    """(included mask (.., 4), valid mask (.., 4)) of blocks B (.., 4, 8)."""
    v = valid(B)
    first = np.argmax(v, axis=-1)                                    # the first valid point in block order (0 where none is)
    zref = np.take_along_axis(B[..., 2], first[..., None], axis=-1)
    inc = v.copy()
    if band is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            inc &= np.abs((B[..., 2] - zref).astype(F32)) <= band
    return inc, v


def reduce_level(X, side, l, kind=MEAN, max_dz=0.0):
    """Level l (side/2 x side/2 points, (n, 8) float32) from level l - 1 (X, side x side)."""
    B = blocks_of(X, side)
    out = B[:, :, 0, :].copy()                                       # PICK, and a block without a valid point: element 0's bits
    if kind == PICK:
        return out.reshape(-1, 8)
    inc, v = included(B, band_of(max_dz, l))
    any_valid = v.any(axis=-1)
    n = inc.sum(axis=-1)
    cols = [0, 1, 2, 4, 5, 6]
    s = np.zeros(B.shape[:2] + (6,), F32)
    seen = np.zeros(B.shape[:2], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(4):                                           # s = the first included value, then s = s + next, in block order
            e = B[:, :, i, :][..., cols]
            take = inc[:, :, i]
            s = np.where((take & ~seen)[..., None], e, np.where((take & seen)[..., None], (s + e).astype(F32), s))
            seen |= take
        mean = (s / np.maximum(n, 1).astype(F32)[..., None]).astype(F32)
    res = np.empty_like(out)
    res[..., [0, 1, 2]] = mean[..., :3]
    res[..., [4, 5, 6]] = mean[..., 3:]
    res[..., 3] = 1.0
    res[..., 7] = 1.0
    # bits, not values: element 0 may hold NaN payloads
    o32, r32 = out.view(np.uint32), res.view(np.uint32)
    o32[any_valid] = r32[any_valid]
    return out.reshape(-1, 8)


def build(X, side, levels, kind=MEAN, max_dz=0.0):
    """[level 0, level 1, ..]: each level from the one before it."""
    out = [np.ascontiguousarray(X, F32).reshape(-1, 8).copy()]
    for l in range(1, levels):
        out.append(reduce_level(out[-1], side >> (l - 1), l, kind, max_dz))
    return out


def block_census(X, side, l, max_dz=0.0):
    """What the rule does at the transition to level l from X (level l - 1): blocks, blocks without a valid point, blocks with 1 - 3
    included points, blocks with four, and blocks with a valid point from which the band excludes one."""
    B = blocks_of(X, side)
    inc, v = included(B, band_of(max_dz, l))
    n = inc.sum(axis=-1)
    return dict(blocks=n.size, none=int((~v.any(axis=-1)).sum()), some=int(((n >= 1) & (n <= 3)).sum()), four=int((n == 4).sum()),
                with_valid=int(v.any(axis=-1).sum()), band_cut=int((v & ~inc).any(axis=-1).sum()))


def oracle_chain(O, Fs, Ms, nr, max_iterations=40, T0=None, fixed=None, **kw):
    """The coarse-to-fine chain on the CPU oracle: a fresh OracleICP per level, coarsest first, T handed on with write_t.
    Fs / Ms: the levels (finest first); fixed: steps per level (finest first) instead of checked runs.
    Returns a list per level, finest first, of dict(T, R, k, converged)."""
    levels = len(Fs)
    its = [max_iterations] * levels if np.isscalar(max_iterations) else list(max_iterations)
    res = [None] * levels
    T = np.array([0, 0, 0, 1, 0, 0, 0, 1], F32) if T0 is None else np.asarray(T0, F32)
    for l in reversed(range(levels)):
        o = O.OracleICP(Fs[l].shape[0], nr[l], max_iterations=its[l], **kw)
        o.write_f(Fs[l])
        o.write_m(Ms[l])
        o.write_t(T)
        o.build_rbc()
        if fixed is None:
            k = o.run()
        else:
            for _ in range(fixed[l]):
                o.step()
            k = fixed[l]
        T = o.T
        res[l] = dict(T=T.copy(), R=o.R.copy(), k=int(k), converged=o.converged)
    return res


def error_to(T, T_true):
    """(degrees, mm) between two transforms [q | t, s]."""
    q, p = np.asarray(T[:4], np.float64), np.asarray(T_true[:4], np.float64)
    d = abs(float(np.dot(q / np.linalg.norm(q), p / np.linalg.norm(p))))
    return float(np.degrees(2.0 * np.arccos(min(1.0, d)))), float(np.linalg.norm(np.asarray(T[4:7], np.float64) - np.asarray(T_true[4:7], np.float64)))


_BASIN = {}


def basin_case(engine, O):
    """The 10 degree pair a single level does not register and three levels do, with both oracle runs (computed once per process):
    dict(F, M, T_true, nr, Fs, Ms, single, chain), the runs as oracle_chain returns them (fused, squared power start, weighted)."""
    if not _BASIN:
        F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_CURVED, rot_deg=10.0)
        kw = dict(a=2e2, c=1e-6, power_fast=True, fused=True, threads=4)
        nr = (256, 64, 64)
        Fs, Ms = build(F, 128, 3), build(M, 128, 3)
        _BASIN.update(F=F, M=M, T_true=T_true, nr=nr, Fs=Fs, Ms=Ms, single=oracle_chain(O, [F], [M], [256], 40, **kw),
                      chain=oracle_chain(O, Fs, Ms, nr, 40, **kw))
    return _BASIN
