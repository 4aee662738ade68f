"""The opt-in paths of the iteration (point-to-plane, colored, trimming, rejection) at the sizes where their kernels branch.

The bit-for-bit modules of each path run at a few sizes only; this one takes their checks, unchanged, to the shapes they miss:
  - point-to-plane / colored: m below one block of 256 (nblk = 1: the finalize's tree has no level), a partly filled last block
    (the clamp and the i < m guard of the moments), block counts that are no power of two (the finalize's zero padding), P > 256 (the
    finalize's multi-pass tree: 8, 4, 2, 1 terms per pass) up to m = 2^20, batches with such block counts;
  - trimming: the multi-workgroup select (m > 16384) with a partly filled last workgroup, just above the one-workgroup limit, batched
    (each registration its own histogram, arrival counter and keys) and in runs whose registrations stop at different iterations;
  - rejection and trimming at sides that are not a multiple of 8 (fused mode's linear 64-query blocks) and in the dense layouts.
  - the route of an iteration (form and launch count) for every combination of the opt-in passes, and the apply pass that accepts
    every candidate (one-to-one and the boundary rule without trimming) at partly filled blocks.
Every check is teacher-forced: the restatement (tests/p2pl_ref.py, tests/colored_ref.py) or the oracle's pieces are fed the engine's own
correspondences of the step.  The point-to-plane steps are also compared with numpy's least-squares solution of their own system."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                  # noqa: E402
import robust_ref as rref                                        # noqa: E402
import unique_ref                                                # noqa: E402
from icp_checks import (A, C_, COLORED, LOSSES, P2PL, POWER, REGULAR, SCALE, WEIGHTED, assert_bits, before, check_last,  # noqa: E402
                        check_p2p_or_identity, check_pair_filter_step, check_pieces, check_plane, check_rejection_step, check_step,
                        check_trim_step, check_unique_step, holes_pair as _holes, load, make_handle, make_plane,
                        messy_grid, one_step, oracle_search, p2p_handle, pair_filter_rule_of, pick_max_dist, plane_handle,
                        restate_colored, restate_gicp, restate_p2pl, restate_symmetric, set_modes, trim_rule,
                        weights_before_trim, step_batch, _t0)

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)


def check_lstsq(engine, g, b=0):
    """The step of registration b against numpy's least-squares solution of the engine's own system A x = b, at float32 rounding:
    omega from TK's quaternion (2 qk / qk.w), tau from TK[4:7].  Compared in the variables scaled by sqrt(diag A) (the scale in which
    LDL^T's error is bounded by the scaled condition number).  Returns False for an identity step (nothing to compare)."""
    s = g.read(engine.Memory.PLANE_SYSTEM, b)
    if s[27] != 1.0:
        return False
    Am, bv = p2pl_ref.unpack(s[:27])
    d = 1.0 / np.sqrt(np.diag(Am))
    As = Am * np.outer(d, d)
    ys = np.linalg.lstsq(As, bv * d, rcond=None)[0]
    Tk = g.read(engine.Memory.TK, b).astype(np.float64)
    x = np.concatenate([2.0 * Tk[:3] / Tk[3], Tk[4:7]])
    ye = x / d
    tol = 8 * EPS32 + 100 * np.linalg.cond(As) * EPS64
    for part, what in ((slice(0, 3), "omega"), (slice(3, 6), "tau")):
        err = np.linalg.norm(ye[part] - ys[part])
        assert err <= tol * np.linalg.norm(ys), (what, b, ye, ys, tol)
    return True


# ---- 1. point-to-plane and colored at the finalize's shapes -------------------------------------------------------------------

# (side, nr): m, nblk = ceil (m / 256), P = nblk padded to a power of two
#   (6, 4) 36 and (14, 4) 196: nblk = 1, no tree level in the finalize;  (30, 4) 900: a partly filled last block, nblk = 4;
#   (96, 64) 9216: nblk = 36 padded to 64;  (150, 4) 22500: a partly filled last block, nblk = 88;  (320, 256) 102400: P = 512, the
#   multi-pass tree (8 terms per pass);  (512, 1024) 2^18: P = 1024;  (1000, 64) 10^6: a partly filled last block, nblk = 3907 padded to
#   4096, 27 passes of one term;  (1024, 4096) 2^20 (config C): nblk = 4096, the largest m icp_init accepts.
PLANE_SHAPES = [(6, 4), (14, 4), (30, 4), (96, 64), (150, 4), (320, 256), (512, 1024), (1000, 64), (1024, 4096)]


@pytest.mark.parametrize("side,nr", PLANE_SHAPES)
def test_point_to_plane_steps(engine, side, nr):
    F, M = engine.synth_pair(side, seed=0x9A1E + side)
    g = make_plane(engine, side, nr, mu=0.05)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        s = check_step(engine, g, restate_p2pl(0.05))
        assert s[27] == 1.0
        assert check_lstsq(engine, g)
    g.close()


@pytest.mark.parametrize("side,nr", [(30, 4), (150, 4), (1000, 64)])
def test_point_to_plane_messy_grid(engine, side, nr):
    """Holes, NaN / inf and zero points in F (grid normals of zero around them), REGULAR weights."""
    seed = 0xBAD + side
    F = messy_grid(engine, side, seed)
    M = engine.synth_pair(side, seed=seed)[1]
    g = make_plane(engine, side, nr, weighted=REGULAR, mu=0.05, fused=False)
    load(engine, g, F, M)
    g.buildRBC()
    assert np.count_nonzero(g.read(engine.Memory.NORMALS_F)[:, :3].any(axis=1)) < side * side * 0.9
    for _ in range(2):
        check_step(engine, g, restate_p2pl(0.05))
        check_lstsq(engine, g)
    g.close()


@pytest.mark.parametrize("side,nr", [(6, 4), (30, 4), (150, 4), (320, 256), (1024, 4096)])
def test_colored_steps(engine, side, nr):
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0xC01 + side)
    g = make_plane(engine, side, nr, mu=0.05, metric=COLORED, kappa=1000.0)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        s = check_step(engine, g, restate_colored(0.05, 1000.0))
        assert s[27] == 1.0
        assert check_lstsq(engine, g)
    g.close()


def test_point_to_plane_batch3_at_P512(engine):
    """Three registrations of 102400 (nblk = 400 each, P = 512): each checked on its own and against a single handle."""
    side, nr, n = 320, 256, 3
    pairs = [engine.synth_pair(side, seed=0x7A00 + i, rot_deg=1.0 + 1.5 * i) for i in range(n)]
    g = make_plane(engine, side, nr, batch=n, mu=0.05)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    Mem = engine.Memory
    for _ in range(2):
        T0 = [(g.read(Mem.T, b).copy(), g.read(Mem.R, b).ravel().copy()) for b in range(n)]
        g.step()
        for b in range(n):
            check_last(engine, g, restate_p2pl(0.05), T0[b][0], T0[b][1], None, b)
            assert check_lstsq(engine, g, b)
    systems = [g.read(Mem.PLANE_SYSTEM, b).copy() for b in range(n)]
    assert not np.array_equal(systems[0], systems[1]) and not np.array_equal(systems[1], systems[2])
    for b in range(n):
        h = make_plane(engine, side, nr, mu=0.05)
        load(engine, h, *pairs[b])
        h.buildRBC()
        h.step(); h.step()
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.PLANE_SYSTEM, b), h.read(Mem.PLANE_SYSTEM), "system of registration %d" % b)
        assert np.array_equal(g.read(Mem.NN_ID, b)["id"], h.read(Mem.NN_ID)["id"]), b
        h.close()
    g.close()


@pytest.mark.parametrize("metric", [P2PL, COLORED])
def test_run_batch2_at_a_partial_block(engine, metric):
    """ICP::run on two registrations of 22500 (nblk = 88, the last block partly filled) against single handles: k, T, the system."""
    side, nr = 150, 4
    if metric == COLORED:
        pairs = [engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0x7B00 + i, rot_deg=1.0 + 2.0 * i)[:2] for i in range(2)]
        mk = lambda batch=1: make_plane(engine, side, nr, mu=0.05, metric=COLORED, kappa=1000.0, batch=batch)
    else:
        pairs = [engine.synth_pair(side, seed=0x7B00 + i, rot_deg=1.0 + 2.0 * i) for i in range(2)]
        mk = lambda batch=1: make_plane(engine, side, nr, mu=0.05, batch=batch)
    g = mk(2)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    Mem = engine.Memory
    for b, (F, M) in enumerate(pairs):
        h = mk()
        load(engine, h, F, M)
        h.buildRBC()
        k = h.run()
        assert 1 < k <= 40, k
        assert g.state(b).k == k, (b, g.state(b).k, k)
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.PLANE_SYSTEM, b), h.read(Mem.PLANE_SYSTEM), "system of registration %d" % b)
        h.close()
    g.close()


# ---- 2. trimming's multi-workgroup select ----------------------------------------------------------------------------------------

# m > ICP_TRIM_ONE_BLOCK_MAX (16384): the select in three multi-workgroup passes of 2048 pairs per workgroup.  (130, 4) 16900: just
# above the one-workgroup limit, 516 pairs in the last workgroup;  (150, 4) 22500: a side that is no multiple of 8 (fused mode's linear
# 64-query blocks in k_trim_apply), 2020 in the last workgroup;  (200, 64) 40000: the tiled order, 1088 in the last workgroup.
TRIM_SHAPES = [(130, 4), (150, 4), (200, 64)]
TRIM_MODES = [(True, WEIGHTED), (False, REGULAR)]


@pytest.mark.parametrize("side,nr", TRIM_SHAPES)
@pytest.mark.parametrize("fused,weighted", TRIM_MODES)
def test_trim_one_step_large_select(engine, oracle, side, nr, fused, weighted):
    F, M = _holes(engine, side, 0x7E1 + side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, weighted, POWER, fused, rejection=(True, None), trimming=0.75)
    one_step(engine, g, F, M, T)
    _, t = check_trim_step(engine, oracle, g, F, M, T, side, fused, weighted, POWER, fused, True, 0.75)
    n, K = int(t[1]), int(t[2])
    assert n > side * side // 3 and K <= t[3] < n, t
    g.close()


def _varied_pairs(engine, side, n, seed):
    """n pairs with different motions and hole patterns (blobs 30 %, scattered 10 %, blobs 10 %, ..)."""
    from icp_amd import workloads as W
    names = ["blobs30", "scattered10", "blobs10"]
    out = []
    for b in range(n):
        pattern, fraction, keep = W.HOLES[names[b % 3]]
        F, M = engine.synth_pair(side, seed=seed + 17 * b, rot_deg=0.5 + 1.75 * b, t=(25.0 - 9 * b, -10.0 + 4 * b, 15.0 - 5 * b))
        F = engine.punch_holes(F, side, side, pattern, fraction, keep, seed=seed + 17 * b + 101)
        M = engine.punch_holes(M, side, side, pattern, fraction, keep, seed=seed + 17 * b + 202)
        out.append((F, M))
    return out


@pytest.mark.parametrize("side,nr", [(150, 4), (200, 64)])
@pytest.mark.parametrize("fused,weighted", TRIM_MODES)
def test_trim_batch3_large_select(engine, oracle, side, nr, fused, weighted):
    """Three registrations in one handle, each with its own histogram, arrival counter and keys: every one checked."""
    n = 3
    pairs = _varied_pairs(engine, side, n, 0x7E2 + side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, weighted, POWER, fused, n, rejection=(True, None), trimming=0.75)
    step_batch(engine, g, pairs, T)
    ts = set()
    for b, (F, M) in enumerate(pairs):
        _, t = check_trim_step(engine, oracle, g, F, M, T, side, fused, weighted, POWER, fused, True, 0.75, b=b)
        ts.add((int(t[0]), int(t[1])))
    assert len(ts) == n, ts
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_trim_batch3_run_against_single_handles(engine, fused):
    """ICP::run on three registrations of 22500 that stop at different iterations (converged ones skip the select's passes): each
    one's k, T and ICP_MEM_TRIM equal a single handle's.  Registration 0 registers a frame to itself (it converges at once); the
    other two have motions and holes of their own."""
    side, nr, n = 150, 4, 3
    pairs = _varied_pairs(engine, side, n, 0x7E3)
    pairs[0] = (pairs[0][0], pairs[0][0].copy())

    def handle(batch):
        g = engine.ICP(0)
        g.init(side * side, nr, A, C_, angle_threshold=0.01, translation_threshold=0.05, batch=batch)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_rejection(True, None)
        g.set_trimming(0.75)
        return g

    g = handle(n)
    for b, (F, M) in enumerate(pairs):
        g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
    g.buildRBC()
    g.run()
    ks = []
    for b, (F, M) in enumerate(pairs):
        h = handle(1)
        h.write(engine.Memory.F, F); h.write(engine.Memory.M, M)
        h.buildRBC()
        k = h.run()
        ks.append(k)
        assert g.state(b).k == k, (b, g.state(b).k, k)
        assert_bits(g.read(engine.Memory.T, b), h.read(engine.Memory.T), "T of registration %d" % b)
        assert np.array_equal(g.read(engine.Memory.TRIM, b), h.read(engine.Memory.TRIM)), b
        h.close()
    assert len(set(ks)) > 1 and min(ks) < 40, ks
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_point_to_plane_with_trimming_large_select(engine, fused):
    """The select of 22500 pairs feeds the plane moments: the accepted set by the rule, then the system by the restatement."""
    side, nr = 150, 4
    F, M = _holes(engine, side, 0x7E4)
    g = make_plane(engine, side, nr, mu=0.05, fused=fused)
    g.set_rejection(True, None)
    g.set_trimming(0.75)
    load(engine, g, F, M)
    g.buildRBC()
    Mem = engine.Memory
    for _ in range(2):
        check_step(engine, g, restate_p2pl(0.05))
        PF, PM, nn_id = g.read(Mem.NN), g.read(Mem.QT), g.read(Mem.NN_ID)
        W0 = weights_before_trim(nn_id, M, PF, PM, True, True)
        acc, t = trim_rule(PF, PM, W0, 0.75)
        assert np.array_equal(g.read(Mem.TRIM), t), (g.read(Mem.TRIM), t)
        assert_bits(PF[acc, 3], W0[acc], "accepted weights")
        assert np.all(PF[~acc, 3].view(np.uint32) == 0), "a trimmed or rejected pair's weight is +0"
        assert t[3] < t[1]
        check_lstsq(engine, g)
    g.close()


# ---- 3. rejection and trimming at tiny and odd sides, and in the dense layouts ------------------------------------------------------

TINY = [(2, 1), (2, 4), (4, 2), (8, 64), (10, 4), (14, 4), (30, 4)]


def _tiny_pair(engine, side):
    """synth_pair with invalid points planted by hand: the first moving point, and about one in seven points of either set beyond it."""
    F, M = engine.synth_pair(side, seed=0x71 + side)
    m = side * side
    M[0, :3] = 0.0
    F[m - 1, :3] = 0.0
    F[np.arange(3, m - 1, 7), :3] = 0.0
    M[np.arange(5, m, 7), :3] = 0.0
    return F, M


@pytest.mark.parametrize("side,nr", TINY)
@pytest.mark.parametrize("fused", [True, False])
def test_rejection_tiny_and_odd(engine, oracle, side, nr, fused):
    F, M = _tiny_pair(engine, side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, rejection=(True, 1.0))
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    for _ in range(2):
        T = g.read(engine.Memory.T).copy()
        md = pick_max_dist(oracle, F, M, T, nr, frac=0.3)             # (a cap that rejects some valid pair at this step's T)
        g.set_rejection(True, md)
        g.step()
        rej = check_rejection_step(engine, oracle, g, F, M, T, side, nr, fused, WEIGHTED, POWER, fused, True, md)
        invalid = (M[:, :3] == 0).all(1) | (g.read(engine.Memory.NN)[:, :3] == 0).all(1)
        assert invalid.any() and (rej & ~invalid).any(), "both rules reject some pair"
    g.close()


@pytest.mark.parametrize("side,nr", TINY)
@pytest.mark.parametrize("fused", [True, False])
def test_trimming_tiny_and_odd(engine, oracle, side, nr, fused):
    F, M = _tiny_pair(engine, side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, rejection=(True, None), trimming=0.5)
    one_step(engine, g, F, M, T)
    for it in range(2):
        if it:
            T = g.read(engine.Memory.T).copy()
            g.step()
        acc, t = check_trim_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, 0.5,
                                 oracle_search(oracle, F, M, T, nr))
        assert 0 < t[3] < t[1], t                                      # (some pair trimmed, some kept)
    g.close()


@pytest.mark.parametrize("side,nr,batch", [(256, 256, 1), (128, 64, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_rejection_dense_layouts(engine, oracle, side, nr, batch, fused):
    """The stage-2 layouts with lanes as candidates (dense, and dense by batch): their REJ variants."""
    pairs = [_holes(engine, side, 0x7E5 + 11 * b, "blobs30" if b % 2 == 0 else "scattered10") for b in range(batch)]
    T = _t0()
    md = pick_max_dist(oracle, pairs[0][0], pairs[0][1], T, nr)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, batch, rejection=(True, md))
    if fused:
        assert g.search_layout() == (1, 256, 1)
    step_batch(engine, g, pairs, T)
    for b, (F, M) in enumerate(pairs):
        check_rejection_step(engine, oracle, g, F, M, T, side, nr, fused, WEIGHTED, POWER, fused, True, md, b=b)
    g.close()


# ---- 4. the robust loss at the sizes where its kernels branch ---------------------------------------------------------------------
#
# tests/test_gpu_robust_loss.py runs every check at side 128 with 256 representatives.  Here its checks, unchanged, reach: m < 64 and
# one partly filled block of the apply pass, fused mode's linear 64-query blocks (a side that is no multiple of 8) also beyond 16384
# pairs, the dense search layouts (single, batched, masked, several representative tiles), the loss behind trimming's three-pass
# select, m = 2^20 (k_moment_level1 in front of the finalize); for the plane metrics the clamp ic = min (i, m - 1) with a partly filled
# last block and the finalize's padded multi-pass tree; and batches whose registrations stop at different iterations (both robust
# kernels return for a registration that is done).  Plane-to-plane and the symmetric objective take the pair's guard i < m, the clamp,
# the loss's weight and the block tree from the same header as the kernels above (icp_plane_moments.h): they are taken, loss off and
# on, to m < 256, to a partly filled last block and to a batch whose registrations stop at different iterations.

ROBUST_DENSE = [(256, 256, 1), (128, 64, 3), (256, 1024, 1), (192, 2048, 1)]


def _robust_p2p_step(engine, oracle, pairs, side, nr, fused, loss, invalid=True, keep=1.0):
    """One step from _t0 () of a handle with len (pairs) registrations, every registration by check_p2p.  Returns the handle and W'."""
    T, n = _t0(), len(pairs)
    g = p2p_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, loss, SCALE[loss], invalid=invalid, keep=keep, batch=n)
    step_batch(engine, g, pairs, T)
    Ws = [check_p2p_or_identity(oracle, g, engine, M, T, side, fused, WEIGHTED, POWER, fused, invalid=invalid, keep=keep, loss=loss,
                                   scale=SCALE[loss], b=b)[0] for b, (F, M) in enumerate(pairs)]
    return g, Ws


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", TINY + [(150, 4)])
@pytest.mark.parametrize("fused", [True, False])
def test_robust_p2p_tiny_and_odd(engine, oracle, side, nr, fused, loss):
    """m < 64, one partly filled block, linear 64-query blocks (also at m = 22500), with invalid points planted by hand.  Below side
    30 the grid is so coarse that every residual is beyond Tukey's 30 mm: those cases are the identity step (nothing accepted)."""
    g, (W,) = _robust_p2p_step(engine, oracle, [_tiny_pair(engine, side)], side, nr, fused, loss)
    assert np.count_nonzero(W == 0) > 0                                # (the planted invalid pairs at least)
    g.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr,batch", ROBUST_DENSE)
@pytest.mark.parametrize("fused", [True, False])
def test_robust_p2p_dense_layouts(engine, oracle, side, nr, batch, fused, loss):
    """The dense search layouts in front of the apply pass: single, batched, masked (|R| = 1024), several representative tiles."""
    pairs = [_holes(engine, side, 0x7E6 + 11 * b, "blobs30" if b % 2 == 0 else "scattered10") for b in range(batch)]
    g, Ws = _robust_p2p_step(engine, oracle, pairs, side, nr, fused, loss)
    if fused:
        assert g.search_layout()[0] == 1, g.search_layout()           # (a dense layout)
    for W in Ws:
        assert 0 < np.count_nonzero(W) < W.size
    g.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", TRIM_SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_robust_p2p_behind_the_large_select(engine, oracle, side, nr, fused, loss):
    """keep = 0.8 at m > 16384: the loss weighs what the three-pass select accepts."""
    g, (W,) = _robust_p2p_step(engine, oracle, [_holes(engine, side, 0x7E7 + side)], side, nr, fused, loss, keep=0.8)
    t = g.read(engine.Memory.TRIM)
    assert 0 < t[2] <= t[3] < t[1] and np.count_nonzero(W) <= t[3], t
    g.close()


def test_robust_p2p_at_2_pow_20(engine, oracle):
    """m = 2^20 (config C), fused, Cauchy, one step: 16384 tiles, k_moment_level1 in front of the finalize."""
    side, nr = 1024, 4096
    F, M = engine.synth_pair(side, seed=0x9A1E + side)
    g, (W,) = _robust_p2p_step(engine, oracle, [(F, M)], side, nr, True, rref.CAUCHY, invalid=False)
    assert np.count_nonzero(W) == side * side
    g.close()


def _robust_plane_steps(engine, g, metric, loss, Ms, steps=2):
    """`steps` steps of a loaded handle: every registration by check_plane, and by check_lstsq where its status word is 1."""
    Mem = engine.Memory
    for _ in range(steps):
        T0 = [(g.read(Mem.T, b).copy(), g.read(Mem.R, b).ravel().copy()) for b in range(len(Ms))]
        g.step()
        for b, M in enumerate(Ms):
            s = check_plane(engine, g, metric, loss, SCALE[loss], T0[b][0], T0[b][1], M=M, b=b)
            assert check_lstsq(engine, g, b) == (s[27] == 1.0)
            assert np.isfinite(s).all() and s[:27].any()


# (every loss up to 102400 pairs; the two cases of about 10^6 pairs with one loss each, for the suite's time)
ROBUST_PLANE_CASES = [(side, nr, loss) for side, nr in PLANE_SHAPES[:6] for loss in LOSSES] + [(1000, 64, rref.TUKEY),
                                                                                                  (1024, 4096, rref.CAUCHY)]


@pytest.mark.parametrize("side,nr,loss", ROBUST_PLANE_CASES)
def test_robust_point_to_plane_steps(engine, side, nr, loss):
    F, M = engine.synth_pair(side, seed=0x9A1E + side)
    g = plane_handle(engine, side, nr, P2PL, loss, SCALE[loss])
    load(engine, g, F, M)
    g.buildRBC()
    _robust_plane_steps(engine, g, P2PL, loss, [M])
    g.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", [(6, 4), (150, 4), (320, 256)])
def test_robust_colored_steps(engine, side, nr, loss):
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0xC01 + side)
    g = plane_handle(engine, side, nr, COLORED, loss, SCALE[loss])
    load(engine, g, F, M)
    g.buildRBC()
    _robust_plane_steps(engine, g, COLORED, loss, [M])
    g.close()


def test_robust_point_to_plane_batch3_at_P512(engine):
    """Three registrations of 102400 with Tukey on: each by the restatement and against a single handle."""
    side, nr, n, loss = 320, 256, 3, rref.TUKEY
    pairs = [engine.synth_pair(side, seed=0x7A00 + i, rot_deg=1.0 + 1.5 * i) for i in range(n)]
    g = plane_handle(engine, side, nr, P2PL, loss, SCALE[loss], batch=n)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    _robust_plane_steps(engine, g, P2PL, loss, [M for _, M in pairs])
    Mem = engine.Memory
    for b in range(n):
        h = plane_handle(engine, side, nr, P2PL, loss, SCALE[loss])
        load(engine, h, *pairs[b])
        h.buildRBC()
        h.step(); h.step()
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.PLANE_SYSTEM, b), h.read(Mem.PLANE_SYSTEM), "system of registration %d" % b)
        h.close()
    g.close()


@pytest.mark.parametrize("metric", [P2PL, COLORED])
def test_robust_run_batch2_at_a_partial_block(engine, metric):
    """ICP::run with Cauchy on, two registrations of 22500 against single handles: k, T, the system."""
    side, nr, loss = 150, 4, rref.CAUCHY
    if metric == COLORED:
        pairs = [engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0x7B00 + i, rot_deg=1.0 + 2.0 * i)[:2] for i in range(2)]
    else:
        pairs = [engine.synth_pair(side, seed=0x7B00 + i, rot_deg=1.0 + 2.0 * i) for i in range(2)]
    mk = lambda batch=1: plane_handle(engine, side, nr, metric, loss, SCALE[loss], batch=batch)
    g = mk(2)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    Mem = engine.Memory
    for b, (F, M) in enumerate(pairs):
        h = mk()
        load(engine, h, F, M)
        h.buildRBC()
        k = h.run()
        assert 1 < k <= 40, k
        assert g.state(b).k == k, (b, g.state(b).k, k)
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.PLANE_SYSTEM, b), h.read(Mem.PLANE_SYSTEM), "system of registration %d" % b)
        h.close()
    g.close()


@pytest.mark.parametrize("side,nr", [(64, 64), (128, 64)])
@pytest.mark.parametrize("fused", [True, False])
def test_robust_p2p_batch3_runs_end_at_different_iterations(engine, side, nr, fused):
    """ICP::run with Cauchy on, three registrations whose pairs start 0.5, 3 and 6 degrees apart, against three single handles: a
    registration that is done is skipped by the apply pass while the others go on."""
    n, loss = 3, rref.CAUCHY
    pairs = [engine.synth_pair(side, seed=0x7C00 + i, rot_deg=(0.5, 3.0, 6.0)[i]) for i in range(n)]

    def handle(batch):
        g = engine.ICP(0)
        g.init(side * side, nr, A, C_, angle_threshold=0.01, translation_threshold=0.05, batch=batch)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_robust_loss(loss, SCALE[loss])
        return g

    Mem = engine.Memory
    g = handle(n)
    for b, (F, M) in enumerate(pairs):
        g.write(Mem.F, F, batch_index=b); g.write(Mem.M, M, batch_index=b)
    g.buildRBC()
    g.run()
    ks = []
    for b, (F, M) in enumerate(pairs):
        h = handle(1)
        h.write(Mem.F, F); h.write(Mem.M, M)
        h.buildRBC()
        ks.append(h.run())
        assert g.state(b).k == ks[-1], (b, g.state(b).k, ks)
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.W, b), h.read(Mem.W), "W' of registration %d" % b)
        assert_bits(g.read(Mem.SUM_W, b), h.read(Mem.SUM_W), "sum W of registration %d" % b)
        assert np.array_equal(g.read(Mem.NN_ID, b)["id"], h.read(Mem.NN_ID)["id"]), b
        h.close()
    assert len(set(ks)) > 1 and min(ks) < 40, ks
    g.close()


# (side, nr): m = 36 and 196, one partly filled block (nblk = 1); 900, nblk = 4 with 132 pairs in the last block
SHARED_BODY_SHAPES = PLANE_SHAPES[:3]
GICP_EPS = 1e-3


def _two_normals_handle(engine, metric, side, nr, loss, batch=1):
    """A plane-to-plane ("gicp") or symmetric ("sym") handle, mu = 0.05, with the loss on when one is given; and its step check."""
    if metric == "gicp":
        g = make_plane(engine, side, nr, mu=0.05, batch=batch, plane_to_plane=GICP_EPS)
        restate = restate_gicp(0.05, GICP_EPS, loss, SCALE.get(loss))
    else:
        g = make_plane(engine, side, nr, mu=0.05, batch=batch, symmetric=True)
        restate = restate_symmetric(0.05, loss, SCALE.get(loss))
    check = lambda T0, R0, k0, b: check_last(engine, g, restate, T0, R0, k0, b)
    if loss is not None:
        g.set_robust_loss(loss, SCALE[loss])
    return g, check


@pytest.mark.parametrize("loss", [None, rref.CAUCHY, rref.TUKEY])
@pytest.mark.parametrize("side,nr", SHARED_BODY_SHAPES)
@pytest.mark.parametrize("metric", ["gicp", "sym"])
def test_two_normals_metrics_below_and_across_a_block(engine, metric, side, nr, loss):
    """Two steps, each against the metric's restatement (tests/gicp_ref.py, tests/sym_ref.py) fed the engine's own outputs."""
    F, M = engine.synth_pair(side, seed=0x9A1E + side)
    g, check = _two_normals_handle(engine, metric, side, nr, loss)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        T0, R0, k0 = before(engine, g)
        g.step()
        s = check(T0, R0, k0, 0)
        assert np.isfinite(s).all()
        if loss != rref.TUKEY:                                      # (Tukey at these coarse grids may accept nothing: the identity step)
            assert s[27] == 1.0 and s[:27].any()
    g.close()


@pytest.mark.parametrize("loss", [None, rref.CAUCHY])
@pytest.mark.parametrize("metric", ["gicp", "sym"])
def test_two_normals_metrics_run_batch2_at_a_partial_block(engine, metric, loss):
    """ICP::run on two registrations of 2500 (nblk = 10, 196 pairs in the last block) against single handles: k, T, the system.  The
    two stop at different iterations by construction, whatever the metric and the loss: registration 0 moves a set onto itself (M = F:
    every d = Q - P is zero, so the right-hand side b is six exact zeros, x = 0, the step is the identity and the run ends at k = 1),
    registration 1 starts 4 degrees away and cannot end there.  From iteration 2 on the moments return for registration 0."""
    side, nr = 50, 4
    F0 = engine.synth_pair(side, seed=0x7D00)[0]
    pairs = [(F0, F0.copy()), engine.synth_pair(side, seed=0x7D01, rot_deg=4.0)]
    g, _ = _two_normals_handle(engine, metric, side, nr, loss, batch=2)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    g.run()
    Mem = engine.Memory
    ks = []
    for b, (F, M) in enumerate(pairs):
        h, _ = _two_normals_handle(engine, metric, side, nr, loss)
        load(engine, h, F, M)
        h.buildRBC()
        ks.append(h.run())
        assert g.state(b).k == ks[-1], (b, g.state(b).k, ks)
        assert_bits(g.read(Mem.T, b), h.read(Mem.T), "T of registration %d" % b)
        assert_bits(g.read(Mem.PLANE_SYSTEM, b), h.read(Mem.PLANE_SYSTEM), "system of registration %d" % b)
        h.close()
    assert ks[0] == 1 and 1 < ks[1] <= 40, ks
    g.close()


# ---- 5. the route of an iteration: form and launch count of every combination of the opt-in passes ----------------------------------
#
# Only icp_init and setters: no iteration runs.  The literals follow include/icp_amd.h (icp_launches_per_iteration, icp_run_form and
# the paragraphs of the setters).  Point-to-point: the tail — 4 launches in reference order; fused 2, or 3 where the first level of the
# moment tree is a launch of its own (more than 256 blocks of 64 pairs: m = 22500 has 352), or 1 chained launch when no pass is on —
# plus 1 for the pair filter, 2 for one-to-one (claim, resolve), trimming's selection (1 launch up to 16384 pairs, 3 beyond) and 1
# apply pass as soon as any of the four is on (the loss adds nothing else).  The plane metrics, whatever the reduce mode: search,
# moments, finalize = 3, plus 1 for the pair filter, 2 for one-to-one, the selection and its apply pass for trimming, nothing for the
# loss (the moments weigh the pairs).  The second-level launches of the reference-order reductions (beyond 65536 / 16384 pairs) do
# not count.  Index = bit 0 the pair filter (the boundary rule), bit 1 one-to-one, bit 2 trimming, bit 3 the robust loss.
ROUTE_LAUNCHES = {
    ("p2p", True, 30): [1, 4, 5, 6, 4, 5, 6, 7, 3, 4, 5, 6, 4, 5, 6, 7],
    ("p2p", True, 150): [1, 5, 6, 7, 7, 8, 9, 10, 4, 5, 6, 7, 7, 8, 9, 10],
    ("p2p", False, 30): [4, 6, 7, 8, 6, 7, 8, 9, 5, 6, 7, 8, 6, 7, 8, 9],
    ("p2p", False, 150): [4, 6, 7, 8, 8, 9, 10, 11, 5, 6, 7, 8, 8, 9, 10, 11],
    ("plane", True, 30): [3, 4, 5, 6, 5, 6, 7, 8, 3, 4, 5, 6, 5, 6, 7, 8],
    ("plane", True, 150): [3, 4, 5, 6, 7, 8, 9, 10, 3, 4, 5, 6, 7, 8, 9, 10],
}
ROUTE_LAUNCHES["plane", False, 30] = ROUTE_LAUNCHES["plane", True, 30]
ROUTE_LAUNCHES["plane", False, 150] = ROUTE_LAUNCHES["plane", True, 150]
FORM_SEPARATE, FORM_CHAINED = 0, 1


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("side", [30, 150])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("metric", ["p2p", "plane"])
def test_route_table(engine, metric, fused, side, mask):
    g = engine.ICP(0)
    g.init(side * side, 4, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    if metric == "plane":
        g.set_normals(1, side)                               # Normals.GRID: no data needed
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
    if mask & 1:
        g.set_boundary_rejection(side)
    if mask & 2:
        g.set_unique(True)
    if mask & 4:
        g.set_trimming(0.75)
    if mask & 8:
        g.set_robust_loss(rref.CAUCHY, SCALE[rref.CAUCHY])
    chained = metric == "p2p" and fused and mask == 0
    got = (g.run_form(), g.launches_per_iteration())
    g.close()
    assert got == (FORM_CHAINED if chained else FORM_SEPARATE, ROUTE_LAUNCHES[metric, fused, side][mask]), got


# ---- 6. the apply pass that accepts every candidate, at the edges of its blocks ----------------------------------------------------
#
# One-to-one correspondences alone, the boundary rule alone (grid width = side) and both, with trimming and the loss off: the apply
# pass keeps every pair the passes in front of it left.  (6, 4): m = 36, one partly filled block of 64 pairs; (30, 4): m = 900, the
# last block of 64 (fused) and the last group of 128 (reference order) partly filled.  The modules' own checks, bit for bit, and
# ICP_MEM_UNIQUE / ICP_MEM_PAIR_FILTER against the restatements' counts.


@pytest.mark.parametrize("case", ["unique", "boundary", "both"])
@pytest.mark.parametrize("side,nr", [(6, 4), (30, 4)])
@pytest.mark.parametrize("fused", [True, False])
def test_accept_all_apply_pass_at_block_edges(engine, oracle, fused, side, nr, case):
    Mem = engine.Memory
    unique, boundary = case != "boundary", case != "unique"
    F, M = engine.synth_pair(side)
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, boundary=side if boundary else None)
    if unique:
        g.set_unique(True)
    assert g.trimming() == 1.0 and g.robust_loss()[0] == 0
    R0 = one_step(engine, g, F, M, T)
    want = oracle_search(oracle, F, M, T, nr)
    if case == "unique":
        _, counts = check_unique_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, want)
        assert counts[0] == side * side and 0 < counts[1] <= counts[0], counts
    elif case == "boundary":
        counts, _ = check_pair_filter_step(engine, oracle, g, F, M, T, R0, side, fused, WEIGHTED, POWER, fused, False, side, None, want)
        assert counts[0] == side * side and counts[1] > 0 and counts[2] == 0 and counts[3] > 0, counts
    else:
        nn_id = g.read(Mem.NN_ID)
        assert np.array_equal(nn_id["id"], want[0]["id"])
        _, counts, W0, (_, _, acc) = pair_filter_rule_of(engine, g, F, M, R0, True, False, side, None)
        assert np.array_equal(g.read(Mem.PAIR_FILTER), counts) and counts[1] > 0 and counts[3] > 0, (g.read(Mem.PAIR_FILTER), counts)
        win, _, ucounts = unique_ref.unique_rule(nn_id["id"], g.read(Mem.NN), g.read(Mem.QT), np.where(acc, W0, np.float32(0)).astype(np.float32))
        got = g.read(Mem.UNIQUE)
        assert np.array_equal(got, ucounts) and got[0] == counts[3] and 0 < got[1] <= got[0], (got, ucounts, counts)
        check_pieces(engine, oracle, g, F, M, T, side, fused, True, POWER, fused, ~win)
        assert np.all(g.read(Mem.W)[win] != 0)
    g.close()
