"""Generalized ICP (icp_set_plane_to_plane, icp_gicp.hip) on the device, bit for bit against tests/gicp_ref.py.

Every iteration is checked teacher-forced, as tests/test_gpu_point_to_plane.py checks point-to-plane: the restatement takes the engine's
own search outputs of that iteration (NN, QT, NN_ID), its NORMALS_F and NORMALS_M and the state's T and R before the step, and must give
the same PLANE_SYSTEM, T, R, TK and RK bits and the same k.  One test runs free: the accuracy of a converged run against point-to-plane.

Convergence, measured on an MI355X (scene 0, side 128, the benchmark's motion, 20 % holes in both frames, ICP_REJECT_INVALID; the errors
against T_true8): see test_convergence_against_point_to_plane's docstring."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref as ref                                          # noqa: E402
import robust_ref                                               # noqa: E402
from icp_checks import (A, C_, COLORED, GIVEN, GRID, IDENTITY as IDENTITY8, P2PL, POWER, REGULAR, STEP_SIZES as SIZES, WEIGHTED,  # noqa: E402
                        assert_bits, load, make_plane, punch_cloud as _holes, restate_gicp, _errors)
import icp_checks      # noqa: E402

pytestmark = pytest.mark.gpu


def make(engine, side, nr, weighted=WEIGHTED, mu=0.05, eps=1e-3, normals=GRID, batch=1, max_iterations=40):
    return make_plane(engine, side, nr, weighted, mu, normals, batch, max_iterations, plane_to_plane=eps)


def check_step(engine, g, mu, eps, b=0, loss=None, scale=None):
    return icp_checks.check_step(engine, g, restate_gicp(mu, eps, loss, scale), b)


def check_fixed_run(engine, g, n, mu, eps, loss=None, scale=None):
    return icp_checks.check_fixed_run(engine, g, n, restate_gicp(mu, eps, loss, scale))


# ---- 1. the moving frame's grid normals

@pytest.mark.parametrize("side,nr", [(128, 256), (50, 4)])
def test_grid_normals_of_the_moving_set(engine, side, nr):
    F, M = engine.synth_pair(side)
    M = _holes(engine, M, side, 31)
    g = make(engine, side, nr)
    assert (g.read(engine.Memory.NORMALS_M) == 0).all()         # (zeros until computed)
    load(engine, g, F, M)
    g.buildRBC()
    want = ref.grid_normals(M, side)
    assert np.count_nonzero(want[:, 2]) > side * side // 2
    assert_bits(g.read(engine.Memory.NORMALS_M), want, "NORMALS_M after buildRBC")
    assert_bits(g.read(engine.Memory.NORMALS_F), ref.grid_normals(F, side), "NORMALS_F")
    M2 = _holes(engine, engine.synth_pair(side, seed=77)[1], side, 41)
    g.write(engine.Memory.M, M2)                                # (a later write of M: computed again, no buildRBC)
    assert_bits(g.read(engine.Memory.NORMALS_M), ref.grid_normals(M2, side), "NORMALS_M after a write of M")
    check_step(engine, g, 0.05, 1e-3)
    g.close()


def test_plane_to_plane_off_computes_no_moving_normals(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, eps=0.0)
    load(engine, g, F, M)
    g.buildRBC()
    g.step()
    assert (g.read(engine.Memory.NORMALS_M) == 0).all()
    assert g.plane_to_plane() == 0.0
    g.close()


# ---- 2. steps and fixed runs, bit for bit

@pytest.mark.parametrize("side,nr", SIZES)
@pytest.mark.parametrize("weighted", [REGULAR, WEIGHTED])
@pytest.mark.parametrize("mu,eps", [(0.0, 1e-3), (0.05, 1e-3), (0.05, 1.0), (0.0, 1.0)])
def test_steps_and_fixed_run_bit_exact(engine, side, nr, weighted, mu, eps):
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, weighted=weighted, mu=mu, eps=eps)
    assert g.plane_to_plane() == np.float32(eps) and g.error_metric() == (P2PL, np.float32(mu))
    assert g.run_form() == 0 and g.launches_per_iteration() == 3
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(2):
        s = check_step(engine, g, mu, eps)
        assert s[27] == 1.0
    check_fixed_run(engine, g, 5, mu, eps)
    g.close()


def test_given_normals_with_zeros_nans_and_other_lengths(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    NF, NM = ref.grid_normals(F, side), ref.grid_normals(M, side)
    rng = np.random.default_rng(3)
    for N in (NF, NM):
        idx = rng.choice(side * side, 3000, replace=False)
        N[idx[:1000]] = 0.0
        N[idx[1000:1500], 1] = np.nan
        N[idx[1500:2000], 0] = np.inf
        N[idx[2000:], :3] *= np.float32(0.5)                    # (not unit: used as given)
    g = make(engine, side, nr, normals=GIVEN, mu=0.05, eps=1e-3)
    load(engine, g, F, M)
    g.write(engine.Memory.NORMALS_F, NF)
    g.write(engine.Memory.NORMALS_M, NM)
    g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_M), NM, "NORMALS_M as written")
    for _ in range(3):
        check_step(engine, g, 0.05, 1e-3)
    g.write(engine.Memory.M, M)                                 # (GIVEN: a write of M leaves the normals alone)
    assert_bits(g.read(engine.Memory.NORMALS_M), NM, "NORMALS_M after a write of M")
    g.close()


@pytest.mark.parametrize("setting", ["reject", "trim", "huber", "cauchy", "tukey"])
def test_with_rejection_trimming_and_robust_losses(engine, setting):
    from icp_amd import workloads as W
    side, nr = 128, 256
    F, M = W.holes_pair(engine, "blobs30", side, seed=W.BASE_SEED + 3)
    g = make(engine, side, nr, mu=0.05, eps=1e-3)
    loss = scale = None
    if setting in ("reject", "trim"):
        g.set_rejection(True, 60.0)
        if setting == "trim":
            g.set_trimming(0.7)
    else:
        g.set_rejection(True)
        loss, scale = robust_ref.LOSSES[setting], 20.0
        g.set_robust_loss(loss, scale)
    load(engine, g, F, M)
    g.buildRBC()
    for _ in range(3):
        s = check_step(engine, g, 0.05, 1e-3, loss=loss, scale=scale)
        assert s[27] == 1.0
    assert np.count_nonzero(g.read(engine.Memory.W) == 0) > side * side // 10, setting
    check_fixed_run(engine, g, 5, 0.05, 1e-3, loss, scale)
    g.close()


# ---- 3. batches

def test_batch_of_three_equals_single_handles(engine):
    side, nr, n = 128, 256, 3
    m = side * side
    pairs = [engine.synth_pair(side, seed=0x3000 + i, rot_deg=1.5 + 0.5 * i) for i in range(n)]
    pairs = [(F, _holes(engine, M, side, 50 + i)) for i, (F, M) in enumerate(pairs)]
    singles = []
    for F, M in pairs:
        h = make(engine, side, nr, mu=0.05, eps=1e-3)
        load(engine, h, F, M)
        h.buildRBC()
        k = h.run()
        singles.append((k, h.read(engine.Memory.T).copy(), h.read(engine.Memory.PLANE_SYSTEM).copy(), h.read(engine.Memory.NORMALS_M).copy()))
        h.close()
    # one handle, three registrations
    g = make(engine, side, nr, mu=0.05, eps=1e-3, batch=n)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    check_step(engine, g, 0.05, 1e-3, 1)                         # (one step of the whole handle, registration 1 against the restatement)
    g.reset_transform(); g.buildRBC()
    g.run()
    for b in range(n):
        assert g.state(b).k == singles[b][0], b
        assert_bits(g.read(engine.Memory.T, b), singles[b][1], "T of registration %d" % b)
        assert_bits(g.read(engine.Memory.PLANE_SYSTEM, b), singles[b][2], "system of registration %d" % b)
        assert_bits(g.read(engine.Memory.NORMALS_M, b), singles[b][3], "NORMALS_M of registration %d" % b)
    g.close()
    # icp_batch_*
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_normals(GRID, side)
    bt.set_error_metric(P2PL, 0.05)
    bt.set_plane_to_plane(1e-3)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i in range(n):
        assert bt.state(i).k == singles[i][0], i
        assert_bits(bt.read(i, engine.Memory.T), singles[i][1], "T of batch registration %d" % i)
        assert_bits(bt.read(i, engine.Memory.PLANE_SYSTEM), singles[i][2], "system of batch registration %d" % i)
        assert_bits(bt.read(i, engine.Memory.NORMALS_M), singles[i][3], "NORMALS_M of batch registration %d" % i)
    bt.close()


# ---- 4. the identity step

def test_all_weights_zero_is_the_identity_step_and_all_normals_zero_is_the_point_share(engine):
    """Every pair rejected: 27 exact zeros, the identity step with status 0.  Every normal zero on both sides: by the rule C = I on
    both sides, so M = I / 2 for every pair and the system is (0.5 + mu) times the point-to-point share — a regular system, solved
    (status 1), not the identity step point-to-plane takes with zero normals and mu = 0; it is checked against the restatement."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    for mu in (0.0, 0.05):
        g = make(engine, side, nr, normals=GIVEN, mu=mu, eps=1e-3)
        load(engine, g, F, M)
        g.buildRBC()
        assert (g.read(engine.Memory.NORMALS_F) == 0).all() and (g.read(engine.Memory.NORMALS_M) == 0).all()
        s = check_step(engine, g, mu, 1e-3)
        assert s[27] == 1.0
        w = g.read(engine.Memory.W).astype(np.float64)
        assert s[15] > 0 and abs(s[15] - (0.5 + float(np.float32(mu))) * w.sum()) <= 1e-9 * s[15]      # (term (3, 3): sum w (1 / 2 + mu))
        g.close()
    g = make(engine, side, nr, mu=0.05, eps=1e-3)
    g.set_rejection(False, 1e-3)                                # (a micron: every pair of the noisy scene is rejected)
    load(engine, g, F, M)
    g.buildRBC()
    T0 = g.read(engine.Memory.T).copy()
    s = check_step(engine, g, 0.05, 1e-3)
    assert (s == 0).all()
    assert (g.read(engine.Memory.W) == 0).all()
    assert_bits(g.read(engine.Memory.T), T0, "T")
    assert_bits(g.read(engine.Memory.TK), IDENTITY8, "TK")
    g.reset_transform(); g.buildRBC()
    assert g.run() == 1 and g.state().converged == 1
    g.close()


# ---- 5. the setter: a parameter update while on, off means off, the refusals

def test_a_new_epsilon_is_a_parameter_update(engine):
    """A new epsilon between two fixed runs goes to a device word: the cached run graph stays (the call costs no capture — well under a
    millisecond, as tests/test_gpu_facade.py::test_setters_leave_the_graphs_standing asks of the other setters) and the second run
    uses it (the bits of a handle created with it)."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, mu=0.05, eps=1e-3)
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed_fresh(5); g.sync()
    first = g.read(engine.Memory.T).copy()
    t0 = time.perf_counter()
    g.set_plane_to_plane(0.25)
    dt = time.perf_counter() - t0
    assert dt < 50e-6 * 20, dt                                  # (the bar is 50 us; a 20 x margin for a loaded test host)
    assert g.plane_to_plane() == 0.25
    t0 = time.perf_counter()
    g.run_fixed_fresh(5); g.sync()                              # the cached graph of 5 iterations, as captured
    dt_run = time.perf_counter() - t0
    got = g.read(engine.Memory.T).copy()
    h = make(engine, side, nr, mu=0.05, eps=0.25)
    load(engine, h, F, M)
    h.buildRBC()
    for _ in range(5):
        h.step()
    assert_bits(got, h.read(engine.Memory.T), "T after the epsilon update")
    assert not np.array_equal(got, first)
    print("set_plane_to_plane: %.1f us; the run behind it: %.1f us" % (dt * 1e6, dt_run * 1e6))
    # and it survives icp_init
    g.init(side * side, nr, A, C_)
    assert g.plane_to_plane() == 0.25
    load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(5)
    assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T after init")
    g.close(); h.close()


def test_off_means_off(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    out = []
    for touched in (True, False):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, nr, A, C_)
        g.set_normals(GRID, side)
        g.set_error_metric(P2PL, 0.05)
        if touched:
            g.set_plane_to_plane(0.001)
            g.set_plane_to_plane(0.0)
        load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(4)
        out.append([g.read(engine.Memory.PLANE_SYSTEM).copy(), g.read(engine.Memory.T).copy()])
        k = g.run()
        out[-1] += [np.array([k]), g.read(engine.Memory.T).copy()]
        g.close()
    for a, b, what in zip(out[0], out[1], ("PLANE_SYSTEM", "T", "k of run", "T of run")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    # point-to-point ignores it, as it ignores mu
    Ts = []
    for eps in (0.0, 0.001):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, nr, A, C_)
        g.set_plane_to_plane(eps)
        load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(4)
        Ts.append(g.read(engine.Memory.T).copy())
        g.close()
    assert_bits(Ts[0], Ts[1], "point-to-point T")


def test_refusals(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    # the colored metric: every run and step is refused, naming both settings
    g = make(engine, side, nr, mu=0.05, eps=1e-3)
    g.set_color_weight(100.0)
    g.set_error_metric(COLORED, 0.05)
    load(engine, g, F, M)
    g.buildRBC()
    for call in (g.step, g.run, lambda: g.run_fixed(2), lambda: g.run_fixed_fresh(2)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == 4, e.value                       # ICP_ESTATE
        assert "icp_set_plane_to_plane" in str(e.value) and "ICP_METRIC_COLORED" in str(e.value)
    g.set_plane_to_plane(0.0)                                   # (one of them off: it runs)
    g.buildRBC()
    g.step()
    g.close()
    bt = engine.ICPBatch([0])
    bt.init(2, side * side, nr, A, C_)
    bt.set_normals(GRID, side)
    bt.set_color_weight(100.0)
    bt.set_error_metric(COLORED, 0.05)
    bt.set_plane_to_plane(1e-3)
    for i in range(2):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    with pytest.raises(engine.ICPError) as e:
        bt.run()
    assert e.value.code == 4 and "icp_set_plane_to_plane" in str(e.value), e.value
    bt.close()
    # GRID: switching it on leaves the handle without moving normals until buildRBC has run again
    g = make(engine, side, nr, mu=0.05, eps=0.0)
    load(engine, g, F, M)
    g.buildRBC()
    g.step()
    g.set_plane_to_plane(1e-3)
    for call in (g.step, g.run, lambda: g.run_fixed(2)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == 4, e.value
    g.reset_transform(); g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_M), ref.grid_normals(M, side), "NORMALS_M")
    check_step(engine, g, 0.05, 1e-3)
    g.close()
    # tracking is not provided
    g = make(engine, side, nr, mu=0.05, eps=1e-3)
    frame = engine.synth_cloud_vga()
    for _ in range(2):
        with pytest.raises(engine.ICPError) as e:
            g.track_next(frame)
        assert e.value.code == 4 and "plane-to-plane" in str(e.value), e.value
    g.set_plane_to_plane(0.0)
    assert g.track_next(frame) is None
    g.close()


# ---- 6. convergence, the one free-running check

def test_convergence_against_point_to_plane(engine):
    """Scene 0 at side 128 with the benchmark's motion, 20 % holes in both frames and ICP_REJECT_INVALID: a checked run with
    epsilon = 1e-3 and mu = 0 against a point-to-plane run (mu = 0.05, plane-to-plane off) on the same handle and pair; the latter is
    the reference, and plane-to-plane's rotation and translation errors against T_true8 may be at most twice its errors (both minimise
    along-normal residuals of the same noisy grid normals).  Measured on an MI355X: point-to-plane 0.01036 deg / 0.2812 mm in 15 iterations,
    plane-to-plane 0.00304 deg / 0.0656 mm in 5."""
    from icp_amd import workloads as W
    side, nr = 128, 256
    F, M, T_true = engine.synth_pair_scene(side, engine.SCENE_CURVED)
    F = engine.punch_holes(F, side, side, engine.HOLES_CONTIGUOUS, 0.2, True, seed=W.BASE_SEED + 101)
    M = engine.punch_holes(M, side, side, engine.HOLES_CONTIGUOUS, 0.2, True, seed=W.BASE_SEED + 202)
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, nr, A, C_)
    g.set_normals(GRID, side)
    g.set_rejection(True)
    load(engine, g, F, M)
    res = {}
    for name, mu, eps in (("point-to-plane", 0.05, 0.0), ("plane-to-plane", 0.0, 1e-3)):
        g.set_error_metric(P2PL, mu)
        g.set_plane_to_plane(eps)
        g.reset_transform(); g.buildRBC()
        k = g.run()
        res[name] = _errors(g.read(engine.Memory.T), T_true) + (k, g.state().converged)
    g.close()
    (rp, tp, kp, cp), (rg, tg, kg, cg) = res["point-to-plane"], res["plane-to-plane"]
    print("convergence: point-to-plane mu=0.05 %.5f deg %.4f mm k=%d conv=%d | plane-to-plane eps=1e-3 mu=0 %.5f deg %.4f mm k=%d conv=%d"
          % (rp, tp, kp, cp, rg, tg, kg, cg))
    assert cp == 1 and cg == 1, res
    assert rg <= 2 * rp and tg <= 2 * tp, res
