"""Robust loss (icp_set_robust_loss) on the device, bit for bit against tests/robust_ref.py.

Point-to-point: the weights W' come from numpy — the rule of include/icp_amd.h applied to the engine's own NN / QT outputs after
rejection and trimming —, and the reference values from the oracle's pieces fed W' with the rows of W' == 0 zeroed (the construction
of tests/test_gpu_trimming.py; in reference order sum W is robust_ref.sum_w_reference, orc_weights' tree over arbitrary weights).
The plane metrics: robust_ref.plane_step on the engine's own search outputs of the step, as tests/test_gpu_point_to_plane.py does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_ref as ref                                        # noqa: E402
from icp_checks import (A, C_, COLORED, EIGEN, GIVEN, GRID, LOSSES, P2P, P2PL, POWER, REGULAR, SCALE, WEIGHTED, assert_bits,  # noqa: E402
                        check_p2p, check_plane, holes_pair as _holes, one_step, p2p_handle, plane_handle, _outlier_scene, step_batch, _t0)

pytestmark = pytest.mark.gpu


# ---- point-to-point


@pytest.fixture(scope="module")
def scenes(engine):
    side = 128
    F, M = engine.synth_pair(side)
    Fh, Mh = _holes(engine, side, 0x1C9D5EED)
    return {"clean": (F, M), "holes": (Fh, Mh)}


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("rot,power_fast", [(POWER, True), (POWER, False), (EIGEN, False)])
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_p2p_one_step(engine, oracle, scenes, fused, weighted, rot, power_fast, loss):
    F, M = scenes["clean"]
    T = _t0()
    g = p2p_handle(engine, F.shape[0], 256, fused, weighted, rot, power_fast, loss, SCALE[loss])
    assert g.robust_loss() == (loss, pytest.approx(SCALE[loss]))
    one_step(engine, g, F, M, T)
    W = check_p2p(oracle, g, engine, M, T, 128, fused, weighted, rot, power_fast, loss=loss, scale=SCALE[loss])
    assert 0 < np.count_nonzero(W) and (loss != ref.TUKEY or np.count_nonzero(W == 0) > 0)
    g.close()


@pytest.mark.parametrize("variant", ["invalid", "max_dist", "trim"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("loss", LOSSES)
def test_p2p_with_rejection_and_trimming(engine, oracle, scenes, loss, fused, variant):
    F, M = scenes["holes"]
    T = _t0()
    kw = {"invalid": dict(invalid=True), "max_dist": dict(invalid=True, max_dist=60.0), "trim": dict(invalid=True, keep=0.8)}[variant]
    g = p2p_handle(engine, F.shape[0], 256, fused, WEIGHTED, POWER, fused, loss, SCALE[loss], **kw)
    one_step(engine, g, F, M, T)
    check_p2p(oracle, g, engine, M, T, 128, fused, WEIGHTED, POWER, fused, loss=loss, scale=SCALE[loss], **kw)
    assert g.rejection()[0] is True
    if variant == "trim":
        assert g.read(engine.Memory.TRIM)[1] > 0
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_p2p_batch(engine, oracle, fused):
    """Eight registrations of one handle with different holes: each its own W'."""
    side, B, loss = 128, 8, ref.CAUCHY
    pairs = [_holes(engine, side, 0x2000 + b, "blobs30" if b % 2 else "scattered10") for b in range(B)]
    T = _t0()
    g = p2p_handle(engine, side * side, 256, fused, WEIGHTED, POWER, fused, loss, SCALE[loss], invalid=True, batch=B)
    step_batch(engine, g, pairs, T)
    for b, (F, M) in enumerate(pairs):
        check_p2p(oracle, g, engine, M, T, side, fused, WEIGHTED, POWER, fused, invalid=True, loss=loss, scale=SCALE[loss], b=b)
    g.close()


def test_huber_beyond_every_residual_is_the_loss_off_iteration(engine, scenes):
    """omega == 1: WEIGHTED fused point-to-point gives the loss-off bits for every output, step after step."""
    F, M = scenes["clean"]
    Mem = engine.Memory
    hs = []
    for loss in (ref.NONE, ref.HUBER):
        g = p2p_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, loss, 1e30)
        g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
        hs.append(g)
    for _ in range(4):
        for g in hs:
            g.step()
        for mem in (Mem.T, Mem.TK, Mem.S, Mem.MEANS, Mem.SUM_W, Mem.W, Mem.NN, Mem.QT, Mem.NN_ID):
            a, b = hs[0].read(mem), hs[1].read(mem)
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), mem
    for g in hs:
        g.close()


@pytest.mark.parametrize("metric", [P2P, P2PL, COLORED])
def test_tukey_below_every_residual_is_the_identity_step(engine, scenes, metric):
    F, M = scenes["clean"]
    Mem = engine.Memory
    g = engine.ICP(0)
    g.init(F.shape[0], 256, A, C_)
    if metric != P2P:
        g.set_normals(GRID, 128)
        g.set_color_weight(1e3)
        g.set_error_metric(metric, 0.05)
    g.set_robust_loss(ref.TUKEY, 1e-6)
    g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
    T0 = g.read(Mem.T).copy()
    k = g.run()
    assert k == 1, k
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float32), "Tk")
    if metric == P2P:
        assert (g.read(Mem.W) == 0).all() and g.read(Mem.SUM_W)[0] == 0
    else:
        assert (g.read(Mem.PLANE_SYSTEM) == 0).all()
    g.close()


# ---- plane metrics

@pytest.mark.parametrize("keep", [1.0, 0.8])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("metric", [P2PL, COLORED])
def test_plane_steps(engine, metric, loss, keep):
    """keep = 0.8: trimming's apply pass zeroes the trimmed weights (loss-off k_trim_apply: the plane metrics weigh in their moments),
    then the robust moments weigh the pairs it keeps."""
    side = 128
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    g = plane_handle(engine, side, 256, metric, loss, SCALE[loss], keep=keep)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M); g.buildRBC()
    Mem = engine.Memory
    for _ in range(3):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        check_plane(engine, g, metric, loss, SCALE[loss], T0, R0, M=M)
        if keep < 1.0:
            t = g.read(Mem.TRIM)
            w = g.read(Mem.W)
            assert 0 < t[2] <= t[3] < t[1] and np.count_nonzero(w) == t[3], t   # (W holds trimming's zeros, no robust factor)
    g.close()


@pytest.mark.parametrize("metric", [P2PL, COLORED])
def test_plane_given_normals_and_gradients_with_zeros_and_nans(engine, metric):
    side = 128
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    rng = np.random.default_rng(7)
    g0 = plane_handle(engine, side, 256, metric, ref.CAUCHY, 12.0)
    g0.write(engine.Memory.F, F); g0.write(engine.Memory.M, M); g0.buildRBC()
    N = g0.read(engine.Memory.NORMALS_F).copy()
    G = g0.read(engine.Memory.COLOR_GRAD_F).copy() if metric == COLORED else None
    g0.close()
    idx = rng.choice(side * side, 600, replace=False)
    N[idx[:200], :3] = 0.0
    N[idx[200:300], 0] = np.nan
    if G is not None:
        G[idx[300:400], :3] = 0.0
        G[idx[400:500], 1] = np.nan
        G[idx[500:], 3] = np.nan                   # (a NaN intensity: a NaN photometric residual, wC = 0)
    g = plane_handle(engine, side, 256, metric, ref.CAUCHY, 12.0, normals=GIVEN)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.write(engine.Memory.NORMALS_F, N)
    if G is not None:
        g.write(engine.Memory.COLOR_GRAD_F, G)
    g.buildRBC()
    Mem = engine.Memory
    for _ in range(2):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        s = check_plane(engine, g, metric, ref.CAUCHY, 12.0, T0, R0, M=M)
        assert np.isfinite(s).all()
    g.close()


@pytest.mark.parametrize("metric", [P2PL, COLORED])
def test_plane_huber_beyond_every_residual_is_the_loss_off_system(engine, metric):
    side = 128
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    Mem = engine.Memory
    hs = []
    for loss in (ref.NONE, ref.HUBER):
        g = plane_handle(engine, side, 256, metric, loss, 1e30)
        g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
        hs.append(g)
    for _ in range(3):
        for g in hs:
            g.step()
        a, b = hs[0].read(Mem.PLANE_SYSTEM), hs[1].read(Mem.PLANE_SYSTEM)
        assert np.array_equal(a, b)                 # (values: the sign of a zero may differ)
        assert_bits(hs[1].read(Mem.T), hs[0].read(Mem.T), "T")
    for g in hs:
        g.close()


# ---- updates, forms, batches

@pytest.mark.parametrize("metric", [P2P, P2PL])
def test_new_scale_reaches_a_captured_graph_and_off_restores(engine, scenes, metric):
    F, M = scenes["clean"]
    Mem = engine.Memory

    def make(loss, scale):
        if metric == P2P:
            g = p2p_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, loss, scale)
        else:
            g = plane_handle(engine, 128, 256, P2PL, loss, scale)
        g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
        return g

    off = make(ref.NONE, 0.0)
    off.run_fixed(3)
    T_off, form_off, n_off = off.read(Mem.T).copy(), off.run_form(), off.launches_per_iteration()
    off.close()
    g = make(ref.CAUCHY, 30.0)
    g.run_fixed(3)                                   # (captures the run graph)
    g.set_robust_loss(ref.CAUCHY, 10.0)
    assert g.robust_loss() == (ref.CAUCHY, 10.0)
    g.reset_transform(); g.buildRBC()
    g.run_fixed(3)
    fresh = make(ref.CAUCHY, 10.0)
    fresh.run_fixed(3)
    assert_bits(g.read(Mem.T), fresh.read(Mem.T), "T after a new scale")
    assert g.launches_per_iteration() == fresh.launches_per_iteration()
    fresh.close()
    g.set_robust_loss(ref.NONE, 0.0)
    assert g.robust_loss() == (0, 0.0)
    g.reset_transform(); g.buildRBC()
    g.run_fixed(3)
    assert_bits(g.read(Mem.T), T_off, "T with the loss off again")
    assert g.run_form() == form_off and g.launches_per_iteration() == n_off
    g.close()


def test_p2p_loss_takes_the_separate_form(engine, scenes):
    F, M = scenes["clean"]
    Mem = engine.Memory
    g = p2p_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, ref.NONE, 0.0)
    g.write(Mem.F, F); g.write(Mem.M, M); g.buildRBC()
    form_off, n_off = g.run_form(), g.launches_per_iteration()
    g.set_robust_loss(ref.TUKEY, 30.0)
    assert g.run_form() == 0                          # ICP_FORM_SEPARATE
    assert g.launches_per_iteration() == 3            # (search, apply, finalize)
    g.set_robust_loss(ref.NONE, 0.0)
    assert (g.run_form(), g.launches_per_iteration()) == (form_off, n_off)
    g.close()


@pytest.mark.parametrize("metric", [P2P, P2PL])
def test_batched_handle_64_equals_single_handles(engine, metric):
    from icp_amd import workloads as W
    side, B, loss, scale = 128, 64, ref.CAUCHY, 12.0
    pairs = [W.pair(engine, b) for b in range(B)]
    Mem = engine.Memory
    if metric == P2P:
        g = p2p_handle(engine, side * side, 256, True, WEIGHTED, POWER, True, loss, scale, batch=B)
    else:
        g = plane_handle(engine, side, 256, P2PL, loss, scale, batch=B)
    for b, (F, M) in enumerate(pairs):
        g.write(Mem.F, F, batch_index=b); g.write(Mem.M, M, batch_index=b)
    g.buildRBC()
    g.run_fixed(3)
    for b in (0, 17, 63):
        F, M = pairs[b]
        h = p2p_handle(engine, side * side, 256, True, WEIGHTED, POWER, True, loss, scale) if metric == P2P \
            else plane_handle(engine, side, 256, P2PL, loss, scale)
        h.write(Mem.F, F); h.write(Mem.M, M); h.buildRBC()
        h.run_fixed(3)
        assert_bits(g.read(Mem.T, batch_index=b), h.read(Mem.T), "T of registration %d" % b)
        h.close()
    g.close()


def test_icp_batch_slots_equal_single_handles(engine):
    side, n, loss, scale = 128, 3, ref.TUKEY, 30.0
    pairs = [engine.synth_pair(side, seed=0x6000 + i) for i in range(n)]
    Mem = engine.Memory
    bt = engine.ICPBatch([0])
    bt.init(n, side * side, 256, A, C_)
    bt.set_robust_loss(loss, scale)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, Mem.F, F); bt.write(i, Mem.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        h = engine.ICP(0)
        h.init(side * side, 256, A, C_)
        h.set_robust_loss(loss, scale)
        h.write(Mem.F, F); h.write(Mem.M, M); h.buildRBC()
        h.run()
        assert_bits(bt.read(i, Mem.T), h.read(Mem.T), "T of registration %d" % i)
        h.close()
    bt.close()


@pytest.mark.parametrize("metric", [P2P, P2PL])
def test_tracking_equals_fresh_handles(engine, oracle, metric):
    """icp_track_next over synthetic VGA frames with a robust loss on equals ICP::run on fresh handles per landmark pair: point-to-point
    (Cauchy, with ICP_REJECT_INVALID on hole-punched frames) and point-to-plane with grid normals (Tukey)."""
    if metric == P2P:
        frames = [engine.punch_holes(engine.synth_cloud_vga(moved=f), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=91 + f)
                  for f in range(4)]
        make = lambda: p2p_handle(engine, 16384, 256, True, WEIGHTED, POWER, True, ref.CAUCHY, 20.0, invalid=True)
    else:
        frames = [engine.synth_cloud_vga(moved=f) for f in range(4)]
        make = lambda: plane_handle(engine, 128, 256, P2PL, ref.TUKEY, 50.0)
    lms = [oracle.get_lms(c) for c in frames]
    Mem = engine.Memory
    g = make()
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h = make()
        h.write(Mem.F, lms[i - 1]); h.write(Mem.M, lms[i])
        h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(Mem.T), h.read(Mem.T), "T of hop %d" % i)
        assert np.array_equal(g.read(Mem.NN_ID)["id"], h.read(Mem.NN_ID)["id"]), i
        if metric == P2P:
            assert_bits(g.read(Mem.W), h.read(Mem.W), "W' of hop %d" % i)
            assert np.count_nonzero(g.read(Mem.W) == 0) > 0
        else:
            assert_bits(g.read(Mem.PLANE_SYSTEM), h.read(Mem.PLANE_SYSTEM), "system of hop %d" % i)
        h.close()
    g.close()


# ---- accuracy

def _register(engine, F, M, metric, loss, scale):
    from icp_amd import workloads as W
    g = engine.ICP(0)
    g.init(F.shape[0], 256, A, C_)
    if metric != P2P:
        g.set_normals(GRID, 128)
        g.set_error_metric(metric, 0.0)
    if loss:
        g.set_robust_loss(loss, scale)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()
    T = g.read(engine.Memory.T).copy()
    g.close()
    return T, k


def test_accuracy_curved_scene_with_outliers(engine):
    """Measured on an MI355X (outliers 300 mm toward the sensor): point-to-plane (mu = 0) 0.0028 deg / 0.415 mm in 9 iterations without
    the loss, Cauchy k = 20 0.0047 deg / 0.139 mm in 14, Tukey k = 50 0.0047 deg / 0.112 mm in 16: the translation error drops three- to
    fourfold.  Point-to-point gains nothing here: 0.1144 deg / 8.578 mm without, Cauchy k = 100 0.1178 deg / 8.454 mm, Tukey k = 200
    0.1170 deg / 8.427 mm, all 40 iterations — its error is the moving frame's half-cell sampling offset (8.8 mm on the clean scene,
    tests/test_gpu_point_to_plane.py), and the weighted search already discounts the far outliers; scales below the start's tens of mm
    of motion make it worse (Cauchy k = 20: 74 mm).  The bounds are about twice the measured values."""
    from icp_amd import workloads as W
    F, M, T_true = _outlier_scene(engine)
    res = {}
    for metric, runs in ((P2P, ((ref.NONE, 0.0), (ref.CAUCHY, 100.0), (ref.TUKEY, 200.0))),
                         (P2PL, ((ref.NONE, 0.0), (ref.CAUCHY, 20.0), (ref.TUKEY, 50.0)))):
        for loss, scale in runs:
            T, k = _register(engine, F, M, metric, loss, scale)
            res[(metric, loss)] = (W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])), k)
    print("outlier scene: " + " | ".join("%s/%s %.4f deg %.3f mm k=%d" % (("p2p", "p2pl")[m], ("none", "huber", "cauchy", "tukey")[l], *v)
                                         for (m, l), v in res.items()))
    r0, t0, _ = res[(P2PL, ref.NONE)]
    for loss in (ref.CAUCHY, ref.TUKEY):
        r, t, k = res[(P2PL, loss)]
        assert t < 0.3 and r < 0.01 and k <= 32 and t < 0.5 * t0, (loss, res)
        r, t, k = res[(P2P, loss)]
        assert t < 17.0 and r < 0.25, (loss, res)
