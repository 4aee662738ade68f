"""The robust loss (icp_set_robust_loss) at the edges of its rule, bit for bit against tests/robust_ref.py, and its point-to-point step
against a float64 solution that shares no code with the oracle.

  - the edge scene (robust_ref.edge_scene): a flat grid and a copy of it lifted by offsets whose squares are exact in fp32, so that
    u = geo / k^2 is 1 exactly, one ulp to either side, 0, a float subnormal's quotient, and far beyond 1 — known to the bit, for
    point-to-point and (with sG2 = r^2 + mu |d|^2) for the plane metrics; for colored a second fixture puts kappa r_C^2 / k^2 at 1;
  - scales at the ends of float: 1e-45 (a subnormal), the smallest normal, 1e-20, 1e19 (k^2 above FLT_MAX), 3e38;
  - NaN and infinite points with a loss on;
  - the step the engine takes with its own W' and correspondences, solved again in numpy float64 (tests/float64_ref.py).
Every check is teacher-forced, as in tests/test_gpu_robust_loss.py, whose handles and checks are used here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ref as f64                                        # noqa: E402
import robust_ref as ref                                         # noqa: E402
from icp_checks import (A, C_, COLORED, GIVEN, LOSSES, P2PL, POWER, REGULAR, SCALE, WEIGHTED, assert_bits, check_p2p,  # noqa: E402
                        check_p2p_or_identity, check_plane, one_step, p2p_expected, p2p_handle, plane_handle, _outlier_scene, _t0)

pytestmark = pytest.mark.gpu

F32 = np.float32
IDENTITY = ref.IDENTITY_T
NEG_ZERO = 0x80000000
EDGE_SIDES = [(128, 256), (30, 4)]
DT_OVER_T_BOUND = 2 * 1.35e-4          # (twice the oracle's measured distance from float64: test_p2p_step_against_float64)
EXTREME_SCALES = [1e-45, 1.1754944e-38, 1e-20, 1e19, 3e38]


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def search_weights(g, engine, weighted, b=0):
    """w of every pair before the loss: 100 / (100 + dist) in fp32 from the engine's NN_ID, or 1."""
    dist = g.read(engine.Memory.NN_ID, batch_index=b)["dist"].astype(F32)
    return (F32(100.0) / (F32(100.0) + dist)).astype(F32) if weighted else np.ones_like(dist)


def no_bad_weights(W, w):
    assert not np.isnan(W).any() and not (u32(W) == NEG_ZERO).any(), "a W' is NaN or -0"
    assert (W <= w).all() and (W >= 0).all(), "a W' above its w"


def edge_honest(g, engine, cls, offsets):
    """The condition that keeps the edge tests honest: every class holds at least m / 10 pairs whose id is their own index and whose
    geo, from the engine's NN and QT, has the expected bits.  Returns that mask."""
    Mem = engine.Memory
    ids = g.read(Mem.NN_ID)["id"]
    geo = ref.geo(g.read(Mem.NN), g.read(Mem.QT))
    m = cls.size
    good = (ids == np.arange(m)) & (u32(geo) == u32(ref.edge_geo(offsets)[cls]))
    for c in range(len(offsets)):
        assert np.count_nonzero(good & (cls == c)) >= m / 10, (ref.EDGE_CLASSES[c], np.count_nonzero(good & (cls == c)), m)
    return good


@pytest.fixture(scope="module")
def templates(engine):
    return {side: engine.synth_pair(side)[0] for side, _ in EDGE_SIDES}


# ---- the rule's edges, point-to-point -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", EDGE_SIDES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("k", [8.0, 7.3])
def test_p2p_at_the_switch_point(engine, oracle, templates, k, fused, weighted, side, nr, loss):
    """k = 8: the class lifted by k has geo == k^2 == 64 in fp32 and in double, u == 1.  k = 7.3: fp32 geo of that class is below the
    double k^2 (u < 1): the pair falls on Tukey's accepting side."""
    offsets = ref.edge_offsets(k)
    F, M, cls = ref.edge_scene(side, templates[side], offsets)
    g = p2p_handle(engine, side * side, nr, fused, weighted, POWER, fused, loss, k)
    one_step(engine, g, F, M, IDENTITY)
    good = edge_honest(g, engine, cls, offsets)
    W = check_p2p(oracle, g, engine, M, IDENTITY, side, fused, weighted, POWER, fused, loss=loss, scale=k)
    w = search_weights(g, engine, weighted)
    no_bad_weights(W, w)
    name = {n: good & (cls == i) for i, n in enumerate(ref.EDGE_CLASSES)}
    gW = g.read(engine.Memory.W)
    u = ref.edge_geo(offsets).astype(np.float64) / ref.k2(k)
    assert (u32(gW[name["zero"]]) == u32(w[name["zero"]])).all(), "residual 0: the bits of w"
    if k == 8.0:
        assert u[1] == 1.0 and u[2] < 1.0 < u[3] and 0 < u[6] < 1e-30
        if loss == ref.HUBER:
            assert (u32(gW[name["at_k"]]) == u32(w[name["at_k"]])).all(), "Huber at u == 1: the bits of w"
            assert (u32(gW[name["below_k"]]) == u32(w[name["below_k"]])).all()
            assert (gW[name["above_k"]] <= w[name["above_k"]]).all()
        if loss == ref.TUKEY:
            assert (u32(gW[name["at_k"]]) == 0).all(), "Tukey at u == 1: +0"
            assert (u32(gW[name["above_k"]]) == 0).all() and (u32(gW[name["two_k"]]) == 0).all()
            below = (w[name["below_k"]].astype(np.float64) * ((1.0 - u[2]) * (1.0 - u[2]))).astype(F32)
            assert (u32(gW[name["below_k"]]) == u32(below)).all(), "Tukey one ulp below 1: float (w (1 - u)^2)"
            assert (below > 0).all()
    else:
        assert u[1] < 1.0                                    # (fp32 (k k) below (double) k (double) k)
        if loss == ref.TUKEY:
            assert (gW[name["at_k"]] > 0).all(), "Tukey: u < 1 is accepted"
        if loss == ref.HUBER:
            assert (u32(gW[name["at_k"]]) == u32(w[name["at_k"]])).all()
    g.close()


# ---- the rule's edges, the plane metrics ----------------------------------------------------------------------------------------

def _plane_edge_steps(engine, g, metric, loss, k, mu, kappa, M, first=None):
    """Two steps: PLANE_SYSTEM, T, Tk by check_plane (a singular system, status word 0: T unchanged, Tk the identity); first (): a
    check of the first step's inputs, which start from the identity."""
    Mem = engine.Memory
    for it in range(2):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        if it == 0 and first:
            first()
        s = check_plane(engine, g, metric, loss, k, T0, R0, mu=mu, kappa=kappa, M=M)
        assert not np.isnan(s).any()
        if s[27] != 1.0:
            assert_bits(g.read(Mem.T), T0, "T behind a singular system")
            assert_bits(g.read(Mem.TK), IDENTITY, "Tk behind a singular system")


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", EDGE_SIDES)
@pytest.mark.parametrize("mu,k", [(0.0, 8.0), (3.0, 16.0)])
def test_point_to_plane_at_the_switch_point(engine, templates, mu, k, side, nr, loss):
    """The grid normals of the flat F are (0, 0, +-1): r = -+offset, sG2 = (1 + mu) offset^2 exactly in double, and sG2 / k^2 == 1 for
    the class lifted by 8 in both settings."""
    offsets = ref.edge_offsets(8.0)
    F, M, cls = ref.edge_scene(side, templates[side], offsets)
    g = plane_handle(engine, side, nr, P2PL, loss, k, mu=mu)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M); g.buildRBC()
    N = g.read(engine.Memory.NORMALS_F)
    assert (N[:, :2] == 0).all() and (np.abs(N[:, 2]) == 1).all()
    o = offsets.astype(np.float64)
    assert ((o * o + float(F32(mu)) * o * o) / ref.k2(k))[1] == 1.0
    assert_bits(g.read(engine.Memory.T), IDENTITY, "the start")
    _plane_edge_steps(engine, g, P2PL, loss, k, mu, 0.0, M, first=lambda: edge_honest(g, engine, cls, offsets))
    g.close()


COLOR_DELTAS = [4.0, float(np.nextafter(F32(4), F32(0))), float(np.nextafter(F32(4), F32(8))), 0.0, 2.0, 12.0]


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr", EDGE_SIDES)
def test_colored_at_the_photometric_switch_point(engine, templates, side, nr, loss):
    """GIVEN normals (0, 0, 1) and gradients (0.5, 0.25, 0) with C_Q = 0; the moving colours (r, 0, 0) have intensities 4, one ulp below
    and above, 0, 2, 12, so r_C = C_P exactly (the gradient is in the plane and P - Q is along the normal), and with kappa = 4, k = 8
    kappa r_C^2 / k^2 is 1 exactly, one ulp to either side, 0, 1 / 4 and 9."""
    kappa, k, mu = 4.0, 8.0, 0.05
    offsets = ref.edge_offsets(k)
    F, M, cls = ref.edge_scene(side, templates[side], offsets)
    m = side * side
    F[:, 4:7] = 0.0
    chan = [ref.intensity_channel(d) for d in COLOR_DELTAS]
    assert all(c is not None for c in chan), chan
    ccls = (np.arange(m) // 8) % len(chan)                     # (every geometric class meets every intensity)
    M[:, 4] = np.array(chan, F32)[ccls]
    M[:, 5:7] = 0.0
    import colored_ref
    cp = colored_ref.intensity(M).astype(np.float64)
    assert np.array_equal(cp, np.array(COLOR_DELTAS)[ccls])
    uC = kappa * (cp * cp) / ref.k2(k)
    assert (uC[ccls == 0] == 1.0).all() and (uC[ccls == 1] < 1.0).all() and (uC[ccls == 2] > 1.0).all()
    N = np.zeros((m, 4), F32); N[:, 2] = 1.0
    G = np.zeros((m, 4), F32); G[:, 0] = 0.5; G[:, 1] = 0.25
    g = plane_handle(engine, side, nr, COLORED, loss, k, mu=mu, kappa=kappa, normals=GIVEN)
    Mem = engine.Memory
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.write(Mem.NORMALS_F, N); g.write(Mem.COLOR_GRAD_F, G)
    g.buildRBC()
    T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
    g.step()
    assert np.array_equal(g.read(Mem.NN_ID)["id"], np.arange(m))
    s = check_plane(engine, g, COLORED, loss, k, T0, R0, mu=mu, kappa=kappa, M=M)
    assert np.isfinite(s).all()
    # (the restatement itself sees the edge: the photometric residual of the pairs, from the engine's outputs, is C_P to the bit)
    Gd = g.read(Mem.COLOR_GRAD_F)
    assert_bits(Gd, G, "given gradients")
    T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
    g.step()
    check_plane(engine, g, COLORED, loss, k, T0, R0, mu=mu, kappa=kappa, M=M)
    g.close()


# ---- scale extremes -------------------------------------------------------------------------------------------------------------

def _scene(engine, templates, which):
    if which == "curved":
        F, M = engine.synth_pair(128)
        return F, M, _t0()
    F, M, _ = ref.edge_scene(128, templates[128], ref.edge_offsets(8.0))
    return F, M, IDENTITY.copy()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("scale", EXTREME_SCALES)
@pytest.mark.parametrize("which", ["curved", "edge"])
def test_p2p_scale_extremes(engine, oracle, templates, which, scale, loss):
    F, M, T = _scene(engine, templates, which)
    Mem = engine.Memory
    g = p2p_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, loss, scale)
    assert g.robust_loss() == (loss, float(F32(scale)))
    one_step(engine, g, F, M, T)
    W, nothing = check_p2p_or_identity(oracle, g, engine, M, T, 128, True, WEIGHTED, POWER, True, loss=loss, scale=scale)
    w = search_weights(g, engine, WEIGHTED)
    no_bad_weights(W, w)
    geo = ref.geo(g.read(Mem.NN), g.read(Mem.QT))
    kf = float(F32(scale))
    if loss == ref.TUKEY:
        # every residual above k: nothing accepted, the identity step (the curved scene at the three small scales)
        assert nothing == bool((geo.astype(np.float64) >= kf * kf).all())
        assert nothing == (which == "curved" and scale < 1.0)
    elif loss == ref.CAUCHY:
        # (w / (1 + u) with u around 1e80 and more is below the smallest float subnormal: every W' rounds to +0)
        assert nothing == (which == "curved" and scale < 1e-30)
    else:
        assert not nothing
    if nothing:
        g.reset_transform(); g.buildRBC()
        T1 = g.read(Mem.T).copy()
        assert g.run() == 1
        assert_bits(g.read(Mem.T), T1, "T after run ()")
        assert_bits(g.read(Mem.TK), IDENTITY, "Tk after run ()")
    if loss == ref.HUBER and which == "curved" and scale == 1.1754944e-38:
        assert np.count_nonzero((W > 0) & (W < np.finfo(F32).tiny)) > 0, "Huber's w / sqrt (u) among the float subnormals"
    if loss == ref.HUBER and which == "curved" and scale == 1e-45:
        assert np.count_nonzero(u32(W) == 0) > 0, "Huber's w / sqrt (u) below the smallest subnormal: +0"
    if loss == ref.HUBER and scale == 3e38:
        h = p2p_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, ref.NONE, 0.0)
        one_step(engine, h, F, M, T)
        for mem in (Mem.T, Mem.TK, Mem.S, Mem.MEANS, Mem.SUM_W, Mem.W, Mem.NN, Mem.QT, Mem.NN_ID):
            a, b = g.read(mem), h.read(mem)
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), mem
        h.close()
    g.close()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("scale", EXTREME_SCALES)
@pytest.mark.parametrize("which", ["curved", "edge"])
def test_point_to_plane_scale_extremes(engine, templates, which, scale, loss):
    F, M, T = _scene(engine, templates, which)
    Mem = engine.Memory
    mu = 0.05
    g = plane_handle(engine, 128, 256, P2PL, loss, scale, mu=mu)
    g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
    T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
    g.step()
    s = check_plane(engine, g, P2PL, loss, scale, T0, R0, mu=mu, M=M)
    assert not np.isnan(s).any()
    if loss == ref.TUKEY and scale < 1e-10 and which == "curved":
        assert (s == 0).all(), "every residual above k: an all-zero system"
        assert_bits(g.read(Mem.T), T0, "T")
        assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
        g.reset_transform(); g.buildRBC()
        assert g.run() == 1
        assert_bits(g.read(Mem.T), T0, "T after run ()")
    if loss == ref.HUBER and scale == 3e38:
        h = plane_handle(engine, 128, 256, P2PL, ref.NONE, 0.0, mu=mu)
        h.write(Mem.F, F); h.write(Mem.M, M); h.buildRBC()
        h.step()
        assert np.array_equal(g.read(Mem.PLANE_SYSTEM), h.read(Mem.PLANE_SYSTEM))      # (values: the sign of a zero may differ)
        assert_bits(g.read(Mem.T), h.read(Mem.T), "T")
        h.close()
    g.close()


# ---- non-finite points with a loss on -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("side,nr,fused,weighted", [(64, 64, True, WEIGHTED), (64, 64, False, WEIGHTED), (128, 256, True, WEIGHTED),
                                                    (256, 1024, True, WEIGHTED), (64, 64, True, REGULAR), (64, 64, False, REGULAR)])
def test_p2p_nan_and_inf_points(engine, oracle, side, nr, fused, weighted, loss):
    """The input of test_nan_and_inf_points_do_not_break_the_search (tests/test_gpu_parity.py), where T ends all NaN with the loss off.
    With a loss on a pair whose geo is not finite is no candidate: W' is +0, its terms are exact zeros, and the step is finite.
    REGULAR (w = 1 for every pair) reaches the rule through geo alone; WEIGHTED also through w = 100 / (100 + inf) = 0."""
    m = side * side
    F, M = engine.synth_pair(side)
    rng = np.random.default_rng(5)
    for idx in rng.choice(m, 6, replace=False):
        M[idx, rng.integers(0, 7)] = np.nan
    for idx in rng.choice(m, 4, replace=False):
        F[idx, rng.integers(0, 7)] = np.inf
    M[9, 0] = -np.inf
    T = _t0()
    Mem = engine.Memory
    g = p2p_handle(engine, m, nr, fused, weighted, POWER, fused, loss, 30.0)
    one_step(engine, g, F, M, T)
    W = check_p2p(oracle, g, engine, M, T, side, fused, weighted, POWER, fused, loss=loss, scale=30.0)
    geo = ref.geo(g.read(Mem.NN), g.read(Mem.QT))
    bad = ~np.isfinite(geo)
    assert bad.any() and (u32(W[bad]) == 0).all(), "a pair without a finite geo: W' is +0"
    no_bad_weights(W, search_weights(g, engine, weighted))
    for mem in (Mem.T, Mem.TK, Mem.MEANS, Mem.S, Mem.SUM_W):
        assert np.isfinite(g.read(mem)).all(), mem
    g.close()


# ---- the step against float64 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["clean", "outliers"])
def test_p2p_step_against_float64(engine, oracle, which, fused, loss):
    """The engine's W' and correspondences of one step from _t0 (), the weighted similarity step solved again in numpy float64
    (Float64ICP.step with weights=, the transform of M included): the blocks of Tk against the project's contract,
    |dq| and |ds| / s <= 1e-5.  fused + squared power method, and reference order + literal.

    The translation block needs more than 1e-5 on the reference side too.  Measured on an MI355X, the oracle's Tk on the same W' is at
    the engine's distance from float64 to every printed digit (the two agree bit for bit): |dq| 0.8e-8 .. 6.9e-8, |ds| / s 0.3e-8 ..
    6.3e-8, |dt| / |t_k| 2.1e-5 .. 1.35e-4 (the largest: clean scene, reference order, Cauchy; 4e-5 .. 1.8e-4 mm absolute).  This step
    starts next to the solution, so |t_k| is 0.8 .. 2 mm while t_k = mean_f - s_k R_k mean_m is a difference of centroids about
    1800 mm from the origin: fp32 rounding of the transformed points and of R_k leaves about 1e-4 mm, a 1e-7 share of the centroids
    but a 1e-4 share of this t_k.  The bound for |dt| / |t_k| is therefore twice the oracle's largest measured distance, 2.7e-4."""
    F, M = engine.synth_pair(128) if which == "clean" else _outlier_scene(engine)[:2]
    T = _t0()
    Mem = engine.Memory
    g = p2p_handle(engine, F.shape[0], 256, fused, WEIGHTED, POWER, fused, loss, SCALE[loss])
    one_step(engine, g, F, M, T)
    W = g.read(Mem.W).copy()
    ids = g.read(Mem.NN_ID)["id"]
    x = f64.Float64ICP(F, M, A, C_)
    x.set_T(T)
    Rk, tk, sk = x.step(ids, weights=W)
    Tk64 = np.concatenate([f64.rot_to_quat(Rk), tk, [sk]])
    e = f64.errors_against(g.read(Mem.TK), Tk64, 1.0)
    _, _, _, _, oTk = p2p_expected(oracle, g, engine, M, T, 128, fused, WEIGHTED, POWER, fused, False, None, 1.0, loss, SCALE[loss])
    eo = f64.errors_against(oTk, Tk64, 1.0)
    print("robust step vs float64 (%s, fused=%s, loss=%d): engine dq %.3g dt/|t| %.3g ds/s %.3g | oracle dq %.3g dt/|t| %.3g ds/s %.3g"
          % (which, fused, loss, e["dq"], e["dt_over_t"], e["ds_over_s"], eo["dq"], eo["dt_over_t"], eo["ds_over_s"]))
    assert 0 < np.count_nonzero(W) and np.linalg.norm(tk) > 0.1
    assert e["dq"] <= 1e-5 and e["ds_over_s"] <= 1e-5, e
    assert e["dt_over_t"] <= DT_OVER_T_BOUND, (e, eo)
    g.close()
