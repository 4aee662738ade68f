"""Colored ICP (ICP_METRIC_COLORED, icp_set_color_weight) on the device, bit for bit against tests/colored_ref.py.

Every iteration is checked teacher-forced, as tests/test_gpu_point_to_plane.py does for point-to-plane: the restatement takes the
engine's own search outputs of that iteration (NN, QT, NN_ID), its NORMALS_F, COLOR_GRAD_F and moving landmarks and the transform
before the step, and must give the same PLANE_SYSTEM, T, R, TK and RK bits."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_ref as cref                                      # noqa: E402
import p2pl_ref as ref                                          # noqa: E402
from icp_checks import (A, C_, COLORED, GIVEN, GRID, P2P, P2PL, REGULAR, SIZES, WEIGHTED, assert_bits, check_last, load,  # noqa: E402
                        make_plane, messy_grid as _messy_grid, register as _register, restate_colored, _errors)
import icp_checks      # noqa: E402

pytestmark = pytest.mark.gpu

make = functools.partial(make_plane, metric=COLORED)         # (kappa 1000 unless given)


def check_step(engine, g, mu, kappa, b=0):
    return icp_checks.check_step(engine, g, restate_colored(mu, kappa), b)


def grads_of(F, width):
    return cref.grid_gradients(F, ref.grid_normals(F, width), width)


# ---- 1. grid gradients

@pytest.mark.parametrize("side,nr", [(32, 64), (128, 256), (256, 1024)])
def test_grid_gradients(engine, side, nr):
    F = _messy_grid(engine, side, 0xC0 + side)
    g = make(engine, side, nr)
    load(engine, g, F, F)
    g.buildRBC()
    want = grads_of(F, side)
    assert np.count_nonzero(want[:, 0]) > side * side // 2
    assert_bits(g.read(engine.Memory.NORMALS_F), ref.grid_normals(F, side), "NORMALS_F")
    assert_bits(g.read(engine.Memory.COLOR_GRAD_F), want, "COLOR_GRAD_F")
    g.close()


def test_grid_gradients_non_square_width_and_batch(engine):
    side = 128
    g = make(engine, side, 256, batch=2)
    g.set_normals(GRID, 64)
    Fs = [_messy_grid(engine, side, 21), _messy_grid(engine, side, 22)]
    for b, F in enumerate(Fs):
        load(engine, g, F, F, b)
    g.buildRBC()
    for b, F in enumerate(Fs):
        assert_bits(g.read(engine.Memory.COLOR_GRAD_F, b), grads_of(F, 64), "COLOR_GRAD_F %d" % b)
    g.close()


def test_grid_gradients_through_write_cloud(engine, oracle):
    cloud = engine.punch_holes(engine.synth_cloud_vga(), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=7)
    g = make(engine, 128, 256)
    g.write_cloud(engine.Memory.F, cloud)
    g.write_cloud(engine.Memory.M, cloud)
    g.buildRBC()
    F = oracle.get_lms(cloud)
    assert_bits(g.read(engine.Memory.F), F, "landmarks")
    assert_bits(g.read(engine.Memory.COLOR_GRAD_F), grads_of(F, 128), "COLOR_GRAD_F")
    g.close()


def test_point_to_plane_computes_no_gradients(engine):
    side = 128
    F, M = engine.synth_pair(side)
    g = make(engine, side, 256)
    g.set_error_metric(P2PL, 0.05)
    load(engine, g, F, M)
    g.buildRBC()
    assert (g.read(engine.Memory.COLOR_GRAD_F) == 0).all()
    g.close()


# ---- 2. single steps, bit for bit

@pytest.mark.parametrize("size", ["small", "A"])
@pytest.mark.parametrize("weighted", [REGULAR, WEIGHTED])
@pytest.mark.parametrize("mu,kappa", [(0.0, 1000.0), (0.05, 100.0), (1.0, 10000.0), (0.05, 0.0)])
def test_steps_bit_exact(engine, size, weighted, mu, kappa):
    side, nr = SIZES[size]
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    g = make(engine, side, nr, weighted=weighted, mu=mu, kappa=kappa)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        s = check_step(engine, g, mu, kappa)
        assert s[27] == 1.0 or (mu == 0.0 and kappa == 0.0)
    assert g.state().k == 2
    g.close()


def test_given_gradients_with_zeros_and_nans(engine):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    N = ref.grid_normals(F, side)
    G = cref.grid_gradients(F, N, side)
    rng = np.random.default_rng(4)
    idx = rng.choice(side * side, 3000, replace=False)
    G[idx[:1000], :3] = 0.0
    G[idx[1000:1500], 1] = np.nan
    G[idx[1500:2000], 2] = -np.inf
    G[idx[2000:], :3] *= np.float32(3.0)           # (used as given)
    g = make(engine, side, nr, normals=GIVEN, mu=0.05, kappa=1000.0)
    assert (g.read(engine.Memory.COLOR_GRAD_F) == 0).all()          # (zeros until written)
    load(engine, g, F, M)
    g.write(engine.Memory.NORMALS_F, N)
    g.write(engine.Memory.COLOR_GRAD_F, G)
    g.buildRBC()
    assert_bits(g.read(engine.Memory.COLOR_GRAD_F), G, "COLOR_GRAD_F as written")
    for _ in range(3):
        check_step(engine, g, 0.05, 1000.0)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_with_rejection_and_trimming(engine, fused):
    from icp_amd import workloads as W
    side, nr = 128, 256
    F, M = W.holes_pair(engine, "blobs30", side, seed=W.BASE_SEED + 5)
    for setting in ("reject", "trim"):
        g = make(engine, side, nr, mu=0.05, kappa=1000.0, fused=fused)
        g.set_rejection(True, 60.0)
        if setting == "trim":
            g.set_trimming(0.8)
        load(engine, g, F, M)
        g.buildRBC()
        for _ in range(3):
            check_step(engine, g, 0.05, 1000.0)
        W_ = g.read(engine.Memory.W)
        assert np.count_nonzero(W_ == 0) > side * side // 10, setting
        g.close()


# ---- 3. batches and runs

def test_batch_of_64_at_A(engine):
    side, nr, n = 128, 256, 64
    pairs = [engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0x3000 + i, rot_deg=1.0 + 0.05 * i)[:2] for i in range(n)]
    g = make(engine, side, nr, batch=n)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    T0 = [(g.read(engine.Memory.T, b).copy(), g.read(engine.Memory.R, b).ravel().copy()) for b in range(n)]
    g.step()
    for b in range(n):
        check_last(engine, g, restate_colored(0.05, 1000.0), T0[b][0], T0[b][1], None, b)
    for b in (0, 17, 63):
        h = make(engine, side, nr)
        load(engine, h, *pairs[b])
        h.buildRBC()
        h.step()
        assert_bits(g.read(engine.Memory.T, b), h.read(engine.Memory.T), "T of registration %d" % b)
        assert_bits(g.read(engine.Memory.PLANE_SYSTEM, b), h.read(engine.Memory.PLANE_SYSTEM), "system of registration %d" % b)
        assert_bits(g.read(engine.Memory.COLOR_GRAD_F, b), h.read(engine.Memory.COLOR_GRAD_F), "gradients of registration %d" % b)
        h.close()
    g.close()


def test_icp_batch_equals_single_handles(engine):
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [engine.synth_pair_scene(side, engine.SCENE_WALL, seed=0x4000 + i)[:2] for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    for kappa in (-1.0, float("nan")):                          # (refused up front, with the batch entry's own message)
        with pytest.raises(engine.ICPError) as e:
            bt.set_color_weight(kappa)
        assert e.value.code == 1 and "icp_batch_set_color_weight" in str(e.value), e.value
    bt.set_normals(GRID, side)
    bt.set_color_weight(1000.0)
    bt.set_error_metric(COLORED, 0.05)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_normals(GRID, side)
        g.set_color_weight(1000.0)
        g.set_error_metric(COLORED, 0.05)
        load(engine, g, F, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        assert_bits(bt.read(i, engine.Memory.PLANE_SYSTEM), g.read(engine.Memory.PLANE_SYSTEM), "system %d" % i)
        assert_bits(bt.read(i, engine.Memory.COLOR_GRAD_F), g.read(engine.Memory.COLOR_GRAD_F), "gradients %d" % i)
        g.close()
    bt.close()


def test_teacher_forced_run(engine):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    g = make(engine, side, nr, mu=0.05, kappa=1000.0)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(8):
        check_step(engine, g, 0.05, 1000.0)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_run_and_run_fixed_equal_steps(engine, fused):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL, rot_deg=1.0, t=(8.0, -4.0, 5.0))
    g = make(engine, side, nr, fused=fused)
    assert g.run_form() == 0
    assert g.launches_per_iteration() == 3
    load(engine, g, F, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    Mem = engine.Memory
    run = [g.read(Mem.T).copy(), g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.NN_ID)["id"].copy()]
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    steps = [g.read(Mem.T).copy(), g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.NN_ID)["id"].copy()]
    for a, b, what in zip(run, steps, ("T", "PLANE_SYSTEM", "ids")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    n = 5
    g.reset_transform(); g.buildRBC()
    g.run_fixed(n)
    fixed = g.read(Mem.T).copy()
    g.reset_transform(); g.buildRBC()
    for _ in range(n):
        g.step()
    assert_bits(fixed, g.read(Mem.T), "run_fixed T")
    g.close()


def test_kappa_update_is_a_parameter_update(engine):
    """A new kappa while the metric stays colored reaches the cached run graphs (it is a device word, not a captured argument)."""
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    g = make(engine, side, nr, kappa=100.0)
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    g.set_color_weight(5000.0)
    assert g.color_weight() == 5000.0 and g.error_metric() == (COLORED, np.float32(0.05))
    g.reset_transform(); g.buildRBC()
    g.run_fixed(3)
    got = g.read(engine.Memory.T).copy()
    h = make(engine, side, nr, kappa=5000.0)
    load(engine, h, F, M)
    h.buildRBC()
    for _ in range(3):
        h.step()
    assert_bits(got, h.read(engine.Memory.T), "T after the kappa update")
    # and it survives icp_init
    g.init(side * side, nr, A, C_)
    assert g.color_weight() == 5000.0
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T after init")
    g.close(); h.close()


def test_switching_to_colored_needs_a_new_build(engine):
    """ICP_NORMALS_GRID: the buildRBC before the switch computed no gradients — the next run is refused until buildRBC runs again."""
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    for before in (P2PL, P2P):
        g = make(engine, side, nr)
        g.set_error_metric(before, 0.05)
        load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(2)
        g.set_error_metric(COLORED, 0.05)
        for call in (g.run, g.step, lambda: g.run_fixed(2)):
            with pytest.raises(engine.ICPError) as e:
                call()
            assert e.value.code == 4, e.value                     # ICP_ESTATE
        assert (g.read(engine.Memory.COLOR_GRAD_F) == 0).all()
        g.reset_transform(); g.buildRBC()
        assert_bits(g.read(engine.Memory.COLOR_GRAD_F), grads_of(F, side), "COLOR_GRAD_F after the new build")
        check_step(engine, g, 0.05, 1000.0)
        # a new kappa or mu, or switching back and forth between colored settings, keeps the build
        g.set_color_weight(10.0)
        g.set_error_metric(COLORED, 0.5)
        check_step(engine, g, 0.5, 10.0)
        g.close()
    # given gradients: nothing to recompute, the build stands
    g = make(engine, side, nr, normals=GIVEN)
    g.set_error_metric(P2PL, 0.05)
    load(engine, g, F, M)
    g.write(engine.Memory.NORMALS_F, ref.grid_normals(F, side))
    g.write(engine.Memory.COLOR_GRAD_F, grads_of(F, side))
    g.buildRBC()
    g.step()
    g.set_error_metric(COLORED, 0.05)
    check_step(engine, g, 0.05, 1000.0)
    g.close()


# ---- 4. tracking

def test_tracking_equals_fresh_handles(engine, oracle):
    frames = [engine.synth_cloud_vga(moved=f) for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    g = make(engine, 128, 256)
    g.set_normals(GIVEN)
    with pytest.raises(engine.ICPError) as e:
        g.track_next(frames[0])
    assert e.value.code == 4                       # ICP_ESTATE: tracking needs GRID normals
    g.set_normals(GRID, 128)
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h = make(engine, 128, 256)
        load(engine, h, lms[i - 1], lms[i])
        h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert_bits(g.read(engine.Memory.PLANE_SYSTEM), h.read(engine.Memory.PLANE_SYSTEM), "system of hop %d" % i)
        h.close()
    g.close()


# ---- 5. switching back, kappa = 0

@pytest.mark.parametrize("fused", [True, False])
def test_switching_back_gives_point_to_plane_and_point_to_point(engine, fused):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    Mem = engine.Memory
    g = make(engine, side, nr, fused=fused)
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(2)
    # -> point-to-plane: its kernels and bits
    g.set_error_metric(P2PL, 0.05)
    h = engine.ICP(0)
    h.init(side * side, nr, A, C_)
    h.setPowerMode(engine.PowerMode.SQUARED)
    h.setReduceMode(engine.ReduceMode.FUSED if fused else engine.ReduceMode.REFERENCE_ORDER)
    h.set_normals(GRID, side)
    h.set_error_metric(P2PL, 0.05)
    load(engine, h, F, M)
    for x in (g, h):
        x.reset_transform(); x.buildRBC()
        for _ in range(3):
            x.step()
    for mem in (Mem.T, Mem.PLANE_SYSTEM, Mem.W):
        a, b = g.read(mem), h.read(mem)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), mem
    # -> point-to-point
    g.set_error_metric(P2P, 0.0)
    h.set_error_metric(P2P, 0.0)
    for x in (g, h):
        x.reset_transform(); x.buildRBC()
        for _ in range(3):
            x.step()
    for mem in (Mem.T, Mem.S, Mem.MEANS, Mem.SUM_W, Mem.W):
        a, b = g.read(mem), h.read(mem)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), mem
    for x in (g, h):
        x.reset_transform(); x.buildRBC()
    assert g.run() == h.run()
    assert_bits(g.read(Mem.T), h.read(Mem.T), "T of run")
    assert g.run_form() == h.run_form() and g.launches_per_iteration() == h.launches_per_iteration()
    g.close(); h.close()


def test_kappa_zero_is_point_to_plane(engine):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_WALL)
    Mem = engine.Memory
    out = []
    for metric in (COLORED, P2PL):
        g = make(engine, side, nr, kappa=0.0)
        g.set_error_metric(metric, 0.05)
        load(engine, g, F, M)
        g.buildRBC()
        for _ in range(4):
            g.step()
        out.append([g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.T).copy(), g.read(Mem.R).copy()])
        g.close()
    for a, b, what in zip(out[0], out[1], ("PLANE_SYSTEM", "T", "R")):
        assert np.array_equal(a, b), what


# ---- 6. accuracy

KAPPAS = (0.0, 1e2, 1e3, 1e4)


def _sweep(engine, F, M, T_true):
    res = {}
    T, k, c = _register(engine, F, M, P2P)
    res["p2p"] = _errors(T, T_true) + (k, c)
    T, k, c = _register(engine, F, M, P2PL, 0.05)
    res["p2pl"] = _errors(T, T_true) + (k, c)
    for kappa in KAPPAS:
        T, k, c = _register(engine, F, M, COLORED, 0.05, kappa)
        res[kappa] = _errors(T, T_true) + (k, c)
    print(" | ".join("%s %.4f deg %.3f mm k=%d" % (("colored kappa=%g" % n) if not isinstance(n, str) else n, *v[:3])
                     for n, v in res.items()))
    return res


def test_accuracy_wall_scene_default_motion(engine):
    """The wall at its default motion, 3 degrees about its normal and 31 mm in its plane, where no geometric variant gets there in
    40 iterations.  Measured on an MI355X: point-to-point 1.826 deg / 41.1 mm (k = 40), point-to-plane mu = 0.05 3.395 deg / 24.8 mm
    (k = 40); colored mu = 0.05: kappa = 0 as point-to-plane, 1e2 0.436 deg / 2.48 mm (k = 40, not converged), 1e3 0.0223 deg /
    3.19 mm (k = 21), 1e4 0.0247 deg / 3.26 mm (k = 15).  The bounds are at least twice the measured values."""
    F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_WALL)
    res = _sweep(engine, F, M, T_true)
    best_r = min(res["p2p"][0], res["p2pl"][0])
    best_t = min(res["p2p"][1], res["p2pl"][1])
    for kappa in (1e3, 1e4):
        r, t, k, conv = res[kappa]
        assert conv == 1 and k <= 30, (kappa, res)
        assert r < 0.05 and t < 7.0, (kappa, res)
        assert r < best_r / 10 and t < best_t / 3, (kappa, res)
    assert np.array_equal(res[0.0], res["p2pl"])                 # (kappa = 0 is point-to-plane)


def test_accuracy_curved_scene(engine):
    """Colored ICP does not end worse than twice point-to-plane's error where geometry alone suffices.  Measured on an MI355X with
    mu = 0.05: point-to-plane 0.0056 deg / 0.173 mm (k = 15), colored kappa = 1e3 0.0056 deg / 0.173 mm (k = 15), kappa = 1e4
    0.0053 deg / 0.164 mm (k = 15)."""
    F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_CURVED)
    res = _sweep(engine, F, M, T_true)
    rp, tp, _, _ = res["p2pl"]
    for kappa in (1e3, 1e4):
        r, t, k, conv = res[kappa]
        assert conv == 1, (kappa, res)
        assert r <= 2 * rp and t <= 2 * tp, (kappa, res)
