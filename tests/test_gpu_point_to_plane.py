"""Point-to-plane ICP (icp_set_error_metric, icp_set_normals) on the device, bit for bit against tests/p2pl_ref.py.

Every iteration is checked teacher-forced: the restatement takes the engine's own search outputs of that iteration (NN, QT, NN_ID —
stored every iteration with the metric on) and its transform before the step, and must give the same PLANE_SYSTEM, T, R, TK and RK
bits.  The search itself is the unchanged one (tests/test_gpu_parity.py checks it against the oracle)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref as ref                                          # noqa: E402
from icp_checks import (A, C_, EIGEN, GIVEN, GRID, IDENTITY as IDENTITY8, P2P, P2PL, POWER, REGULAR, SIZES, WEIGHTED,  # noqa: E402
                        assert_bits, check_last, load, make_plane as make, messy_grid as _messy_grid, register as _register,
                        restate_p2pl, _errors)
import icp_checks      # noqa: E402

pytestmark = pytest.mark.gpu


def check_step(engine, g, mu, b=0, normals=None):
    """One step of handle g (all registrations), checked for registration b against the restatement.  Returns the system."""
    return icp_checks.check_step(engine, g, restate_p2pl(mu, normals), b)


# ---- 0. the composition restatement against the engine's own point-to-point steps

def test_composition_restatement_matches_point_to_point_steps(engine):
    F, M = engine.synth_pair(128)
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(128 * 128, 256, A, C_)
    load(engine, g, F, M)
    g.buildRBC()
    Mem = engine.Memory
    for _ in range(4):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        T, R, Rk = ref.compose(T0, R0, g.read(Mem.TK))
        assert_bits(g.read(Mem.T), T, "T")
        assert_bits(g.read(Mem.R).ravel(), R, "R")
        assert_bits(g.read(Mem.RK).ravel(), Rk, "RK")
    assert (g.read(Mem.PLANE_SYSTEM) == 0).all()
    g.close()


# ---- 1. grid normals

@pytest.mark.parametrize("side,nr", [(32, 64), (128, 256), (256, 1024)])
def test_grid_normals(engine, side, nr):
    F = _messy_grid(engine, side, 0x5EED + side)
    g = make(engine, side, nr)
    g.write(engine.Memory.F, F)
    g.write(engine.Memory.M, F)
    g.buildRBC()
    got = g.read(engine.Memory.NORMALS_F)
    want = ref.grid_normals(F, side)
    assert np.count_nonzero(want[:, 2]) > side * side // 2
    assert_bits(got, want, "NORMALS_F")
    g.close()


def test_grid_normals_non_square_width_and_batch(engine):
    """Width 64 on a 128 x 128 set (a 64 x 256 grid), two registrations of one handle: each its own normals."""
    side = 128
    g = make(engine, side, 256, batch=2)
    g.set_normals(GRID, 64)
    Fs = [_messy_grid(engine, side, 11), _messy_grid(engine, side, 12)]
    for b, F in enumerate(Fs):
        load(engine, g, F, F, b)
    g.buildRBC()
    for b, F in enumerate(Fs):
        assert_bits(g.read(engine.Memory.NORMALS_F, b), ref.grid_normals(F, 64), "NORMALS_F %d" % b)
    g.close()


def test_grid_normals_through_write_cloud(engine, oracle):
    cloud = engine.punch_holes(engine.synth_cloud_vga(), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=5)
    g = make(engine, 128, 256)
    g.write_cloud(engine.Memory.F, cloud)
    g.write_cloud(engine.Memory.M, cloud)
    g.buildRBC()
    F = oracle.get_lms(cloud)
    assert_bits(g.read(engine.Memory.F), F, "landmarks")
    assert_bits(g.read(engine.Memory.NORMALS_F), ref.grid_normals(F, 128), "NORMALS_F")
    g.close()


def test_grid_width_must_divide_m(engine):
    g = engine.ICP(0)
    g.init(128 * 128, 256, A, C_)
    with pytest.raises(engine.ICPError):
        g.set_normals(GRID, 100)
    g.close()
    g = engine.ICP(0)
    g.set_normals(GRID, 100)                       # (no handle size yet: accepted, checked by buildRBC)
    g.init(128 * 128, 256, A, C_)
    F, M = engine.synth_pair(128)
    load(engine, g, F, M)
    with pytest.raises(engine.ICPError) as e:
        g.buildRBC()
    assert e.value.code == 4                       # ICP_ESTATE
    assert g.normals() == (GRID, 100)
    g.close()


# ---- 2. one step, bit for bit

@pytest.mark.parametrize("size", ["small", "A", "B"])
@pytest.mark.parametrize("weighted", [REGULAR, WEIGHTED])
@pytest.mark.parametrize("mu", [0.0, 0.05, 1.0])
def test_steps_bit_exact(engine, size, weighted, mu):
    side, nr = SIZES[size]
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, weighted=weighted, mu=mu)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        s = check_step(engine, g, mu)
        assert s[27] == 1.0
    assert g.state().k == 2
    g.close()


def test_given_normals_with_zeros_and_nans(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    N = ref.grid_normals(F, side)
    rng = np.random.default_rng(3)
    idx = rng.choice(side * side, 3000, replace=False)
    N[idx[:1000]] = 0.0
    N[idx[1000:1500], 1] = np.nan
    N[idx[1500:2000], 0] = np.inf
    N[idx[2000:], :3] *= np.float32(0.5)           # (not unit: used as given)
    g = make(engine, side, nr, normals=GIVEN, mu=0.05)
    assert (g.read(engine.Memory.NORMALS_F) == 0).all()             # (zeros until written)
    load(engine, g, F, M)
    g.write(engine.Memory.NORMALS_F, N)
    g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_F), N, "NORMALS_F as written")
    for _ in range(3):
        check_step(engine, g, 0.05)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_with_rejection_and_trimming(engine, fused):
    from icp_amd import workloads as W
    side, nr = 128, 256
    F, M = W.holes_pair(engine, "blobs30", side, seed=W.BASE_SEED + 3)
    for setting in ("reject", "trim"):
        g = make(engine, side, nr, mu=0.05, fused=fused)
        g.set_rejection(True, 60.0)
        if setting == "trim":
            g.set_trimming(0.8)
        load(engine, g, F, M)
        g.buildRBC()
        for _ in range(3):
            check_step(engine, g, 0.05)
        W_ = g.read(engine.Memory.W)
        assert np.count_nonzero(W_ == 0) > side * side // 10, setting
        g.close()


def test_bits_do_not_depend_on_rot_power_or_reduce_mode(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    out = []
    for rot, fast, fused in ((POWER, True, True), (POWER, False, False), (EIGEN, False, True), (EIGEN, True, False)):
        g = make(engine, side, nr, rot=rot, power_fast=fast, fused=fused, mu=0.05)
        load(engine, g, F, M)
        g.buildRBC()
        for _ in range(3):
            g.step()
        out.append([g.read(engine.Memory.T).copy(), g.read(engine.Memory.PLANE_SYSTEM).copy(), g.read(engine.Memory.NN_ID)["id"].copy()])
        g.close()
    for o in out[1:]:
        for a, b, what in zip(out[0], o, ("T", "PLANE_SYSTEM", "ids")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


# ---- 3. batches and runs

def test_batch_of_64_at_A(engine):
    side, nr, n = 128, 256, 64
    pairs = [engine.synth_pair(side, seed=0x1000 + i, rot_deg=1.0 + 0.05 * i) for i in range(n)]
    g = make(engine, side, nr, batch=n, mu=0.05)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    T0 = [(g.read(engine.Memory.T, b).copy(), g.read(engine.Memory.R, b).ravel().copy()) for b in range(n)]
    g.step()
    for b in range(n):
        check_last(engine, g, restate_p2pl(0.05), T0[b][0], T0[b][1], None, b)
    # a few registrations against single handles
    for b in (0, 17, 63):
        h = make(engine, side, nr, mu=0.05)
        load(engine, h, *pairs[b])
        h.buildRBC()
        h.step()
        assert_bits(g.read(engine.Memory.T, b), h.read(engine.Memory.T), "T of registration %d" % b)
        assert_bits(g.read(engine.Memory.PLANE_SYSTEM, b), h.read(engine.Memory.PLANE_SYSTEM), "system of registration %d" % b)
        h.close()
    g.close()


def test_icp_batch_equals_single_handles(engine):
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [engine.synth_pair(side, seed=0x2000 + i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    for source, width in ((5, 128), (GRID, 0)):                 # (refused up front, with the batch entry's own message)
        with pytest.raises(engine.ICPError) as e:
            bt.set_normals(source, width)
        assert e.value.code == 1 and "icp_batch_set_normals" in str(e.value), e.value
    bt.set_normals(GRID, side)
    bt.set_error_metric(P2PL, 0.05)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_normals(GRID, side)
        g.set_error_metric(P2PL, 0.05)
        load(engine, g, F, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        assert_bits(bt.read(i, engine.Memory.PLANE_SYSTEM), g.read(engine.Memory.PLANE_SYSTEM), "system %d" % i)
        g.close()
    bt.close()


def test_teacher_forced_run(engine):
    side, nr = 128, 256
    F, M, _ = engine.synth_pair_scene(side, engine.SCENE_CURVED)
    g = make(engine, side, nr, mu=0.05)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(8):
        check_step(engine, g, 0.05)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_run_and_run_fixed_equal_steps(engine, fused):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, mu=0.05, fused=fused)
    assert g.run_form() == 0
    assert g.launches_per_iteration() == 3
    load(engine, g, F, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k < 40, k
    Mem = engine.Memory
    run = [g.read(Mem.T).copy(), g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.NN_ID)["id"].copy()]
    assert g.state().converged == 1
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


def test_mu_update_is_a_parameter_update(engine):
    """A new mu while the metric stays on reaches the cached run graphs."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, mu=0.05)
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    g.set_error_metric(P2PL, 1.0)
    assert g.error_metric() == (P2PL, 1.0)
    g.reset_transform(); g.buildRBC()
    g.run_fixed(3)
    got = g.read(engine.Memory.T).copy()
    h = make(engine, side, nr, mu=1.0)
    load(engine, h, F, M)
    h.buildRBC()
    for _ in range(3):
        h.step()
    assert_bits(got, h.read(engine.Memory.T), "T after the mu update")
    g.close(); h.close()


# ---- 4. the identity step

def _exact_plane_pair(side):
    gx, gy = np.meshgrid((np.arange(side) - side // 2) * 8.0, (np.arange(side) - side // 2) * 8.0)
    F = np.zeros((side * side, 8), np.float32)
    F[:, 0], F[:, 1] = gx.ravel(), gy.ravel()
    F[:, 2] = 1000.0 + F[:, 0] / 4 - F[:, 1] / 2
    F[:, 3] = 1.0
    F[:, 4:7] = 0.5
    F[:, 7] = 1.0
    M = F.copy()
    M[:, 2] += 2.0                                  # (the same plane shifted: every pair on it, normals all alike)
    return F, M


def test_exact_plane_without_point_term_is_the_identity_step(engine):
    side, nr = 64, 256
    F, M = _exact_plane_pair(side)
    g = make(engine, side, nr, mu=0.0)
    load(engine, g, F, M)
    g.buildRBC()
    T0 = g.read(engine.Memory.T).copy()
    s = check_step(engine, g, 0.0)
    assert s[27] == 0.0
    assert_bits(g.read(engine.Memory.T), T0, "T")
    assert_bits(g.read(engine.Memory.TK), IDENTITY8, "TK")
    g.reset_transform(); g.buildRBC()
    assert g.run() == 1
    assert g.state().converged == 1
    assert_bits(g.read(engine.Memory.T), IDENTITY8, "T after run")
    g.close()


# ---- 5. tracking

def test_tracking_equals_fresh_handles(engine, oracle):
    frames = [engine.synth_cloud_vga(moved=f) for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    g = make(engine, 128, 256, mu=0.05)
    g.set_normals(GIVEN)
    with pytest.raises(engine.ICPError) as e:
        g.track_next(frames[0])
    assert e.value.code == 4                       # ICP_ESTATE: tracking needs GRID normals
    g.set_normals(GRID, 128)
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h = make(engine, 128, 256, mu=0.05)
        load(engine, h, lms[i - 1], lms[i])
        h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert_bits(g.read(engine.Memory.PLANE_SYSTEM), h.read(engine.Memory.PLANE_SYSTEM), "system of hop %d" % i)
        h.close()
    g.close()


@pytest.mark.parametrize("metric", [P2PL, P2P])
def test_tracking_refuses_a_grid_width_that_does_not_divide_m(engine, metric):
    """A width set before init (accepted: the handle has no size yet) that does not divide m: a tracked frame builds its RBC without
    icp_build_rbc, and icp_track_next refuses it with ICP_ESTATE before anything is enqueued — the metric on or off, since buildRBC
    computes grid normals whenever the source is ICP_NORMALS_GRID."""
    g = engine.ICP(0)
    g.set_normals(GRID, 100)
    g.init(16384, 256, A, C_)
    g.set_error_metric(metric, 0.05)
    frame = engine.synth_cloud_vga()
    for _ in range(2):
        with pytest.raises(engine.ICPError) as e:
            g.track_next(frame)
        assert e.value.code == 4, e.value                 # ICP_ESTATE
        assert "grid width" in str(e.value)
    g.set_normals(GRID, 128)                              # a width that divides m: tracking goes ahead
    assert g.track_next(frame) is None
    assert g.track_next(engine.synth_cloud_vga(moved=1)) > 0
    g.close()


# ---- 6. switching back

@pytest.mark.parametrize("fused", [True, False])
def test_switching_back_is_point_to_point(engine, fused):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, mu=0.05, fused=fused)
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(2)
    assert g.read(engine.Memory.PLANE_SYSTEM)[27] == 1.0
    g.set_error_metric(P2P, 0.0)
    assert (g.read(engine.Memory.PLANE_SYSTEM) == 0).all()
    h = engine.ICP(0)
    h.init(side * side, nr, A, C_)
    h.setPowerMode(engine.PowerMode.SQUARED)
    h.setReduceMode(engine.ReduceMode.FUSED if fused else engine.ReduceMode.REFERENCE_ORDER)
    load(engine, h, F, M)
    Mem = engine.Memory
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
    assert g.run_form() == h.run_form()
    assert (g.read(engine.Memory.PLANE_SYSTEM) == 0).all()
    g.close(); h.close()


# ---- 7. accuracy

def test_accuracy_curved_scene(engine):
    """Scene 0, mu = 0 converges.  Measured on an MI355X: point-to-point 0.1251 deg / 8.810 mm in 36 iterations (the half-cell sampling
    offset of the moving frame), point-to-plane 0.0051 deg / 0.121 mm in 8; the bounds are more than twice the measured values."""
    F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_CURVED)
    Tp, kp, _ = _register(engine, F, M, P2P)
    T, k, conv = _register(engine, F, M, P2PL, 0.0)
    (rp, tp), (r, t) = _errors(Tp, T_true), _errors(T, T_true)
    print("curved scene: point-to-point %.4f deg %.3f mm k=%d | point-to-plane mu=0 %.4f deg %.3f mm k=%d"
          % (rp, tp, kp, r, t, k))
    assert conv == 1 and k <= 20, k
    assert r < 0.015 and t < 0.3, (r, t)


def test_accuracy_wall_scene(engine):
    """The wall moved in its own plane (1 degree about its normal, an in-plane shift): with mu = 0.05 the in-plane motion is recovered.
    Measured on an MI355X: point-to-point 0.055 deg / 7.68 mm (k = 32), point-to-plane mu = 0.05 0.040 deg / 2.77 mm (k = 31),
    mu = 0 0.066 deg / 0.13 mm (k = 6: the wall's millimetre of roughness is geometry both frames share), mu = 1 0.053 deg / 8.14 mm.
    (With the scene's default motion, 3 degrees and 31 mm, no variant gets there in 40 iterations: DESIGN.md.)"""
    F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_WALL, rot_deg=1.0, t=(8.0, -4.0, 5.0))
    Tp, kp, _ = _register(engine, F, M, P2P)
    (rp, tp) = _errors(Tp, T_true)
    line = "wall scene: point-to-point %.4f deg %.3f mm k=%d" % (rp, tp, kp)
    res = {}
    for mu in (0.0, 0.05, 1.0):
        T, k, conv = _register(engine, F, M, P2PL, mu)
        res[mu] = _errors(T, T_true) + (k, conv)
        line += " | point-to-plane mu=%g %.4f deg %.3f mm k=%d" % (mu, res[mu][0], res[mu][1], k)
    print(line)
    r, t, k, conv = res[0.05]
    assert conv == 1, res
    assert r < 0.1 and t < 6.0, res
    r, t, k, conv = res[0.0]                        # (the roughness of the wall pins the in-plane directions)
    assert conv == 1, res
    assert r < 0.15 and t < 0.3, res
