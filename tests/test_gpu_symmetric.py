"""Symmetric ICP (icp_set_symmetric, icp_symmetric.hip and the symmetric increment of k_p2pl_finalize) on the device, bit for bit against
tests/sym_ref.py.

Every iteration is checked teacher-forced, as tests/test_gpu_gicp.py checks plane-to-plane: the restatement takes the engine's own
search outputs of that iteration (NN, QT, NN_ID), its NORMALS_F and NORMALS_M and the state's T and R before the step, and must give the
same PLANE_SYSTEM, T, R, TK and RK bits and the same k.  One test runs free: a converged run against point-to-plane
(test_convergence_against_point_to_plane, whose docstring has the measured figures)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref as ref                                          # noqa: E402
import robust_ref                                               # noqa: E402
from icp_checks import (A, C_, COLORED, GIVEN, GRID, IDENTITY as IDENTITY8, P2PL, POWER, REGULAR, STEP_SIZES as SIZES, WEIGHTED,  # noqa: E402
                        assert_bits, load, make_plane, punch_cloud as _holes, restate_symmetric, _errors)
import icp_checks      # noqa: E402

pytestmark = pytest.mark.gpu

ESTATE = 4

def make(engine, side, nr, weighted=WEIGHTED, mu=0.05, sym=True, normals=GRID, batch=1, max_iterations=40):
    return make_plane(engine, side, nr, weighted, mu, normals, batch, max_iterations, symmetric=sym)


def check_step(engine, g, mu, b=0, loss=None, scale=None):
    return icp_checks.check_step(engine, g, restate_symmetric(mu, loss, scale), b)


def check_fixed_run(engine, g, n, mu, loss=None, scale=None):
    return icp_checks.check_fixed_run(engine, g, n, restate_symmetric(mu, loss, scale))


# ---- 1. steps and fixed runs, bit for bit

@pytest.mark.parametrize("side,nr", SIZES)
@pytest.mark.parametrize("weighted", [REGULAR, WEIGHTED])
@pytest.mark.parametrize("mu", [0.0, 0.05])
def test_steps_and_fixed_run_bit_exact(engine, side, nr, weighted, mu):
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, weighted=weighted, mu=mu)
    assert g.symmetric() is True and g.error_metric() == (P2PL, np.float32(mu))
    assert g.run_form() == 0 and g.launches_per_iteration() == 3
    load(engine, g, F, M)
    g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_M), ref.grid_normals(M, side), "NORMALS_M after buildRBC")
    for _ in range(2):
        s = check_step(engine, g, mu)
        assert s[27] == 1.0
    check_fixed_run(engine, g, 5, mu)
    g.close()


def test_given_normals_with_edge_values_and_the_flip_rule(engine):
    """ICP_NORMALS_GIVEN with zeros, NaNs, infinities and non-unit lengths on both sides, bit for bit; and the same run with N_M negated
    for every other point gives the same T: N_P is turned to N_Q's side before it is used."""
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
    NMneg = NM.copy()
    NMneg[::2, :3] = -NMneg[::2, :3]
    Ts = []
    for normals_m in (NM, NMneg):
        g = make(engine, side, nr, normals=GIVEN, mu=0.05)
        load(engine, g, F, M)
        g.write(engine.Memory.NORMALS_F, NF)
        g.write(engine.Memory.NORMALS_M, normals_m)
        g.buildRBC()
        assert_bits(g.read(engine.Memory.NORMALS_M), normals_m, "NORMALS_M as written")
        for _ in range(3):
            check_step(engine, g, 0.05)
        g.write(engine.Memory.M, M)                             # (GIVEN: a write of M leaves the normals alone)
        assert_bits(g.read(engine.Memory.NORMALS_M), normals_m, "NORMALS_M after a write of M")
        Ts.append(g.read(engine.Memory.T).copy())
        g.close()
    assert (Ts[0] == Ts[1]).all(), Ts


@pytest.mark.parametrize("side,nr", [(128, 256), (50, 4)])
@pytest.mark.parametrize("setting", ["reject", "trim", "huber", "cauchy", "tukey"])
def test_with_rejection_trimming_and_robust_losses(engine, setting, side, nr):
    from icp_amd import workloads as W
    F, M = W.holes_pair(engine, "blobs30", side, seed=W.BASE_SEED + 3)
    g = make(engine, side, nr, mu=0.05)
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
        s = check_step(engine, g, 0.05, loss=loss, scale=scale)
        assert s[27] == 1.0
    assert np.count_nonzero(g.read(engine.Memory.W) == 0) > side * side // 10, setting
    check_fixed_run(engine, g, 5, 0.05, loss, scale)
    g.close()


# ---- 2. batches

def test_batch_of_three_equals_single_handles(engine):
    side, nr, n = 128, 256, 3
    m = side * side
    pairs = [engine.synth_pair(side, seed=0x3000 + i, rot_deg=1.5 + 0.5 * i) for i in range(n)]
    pairs = [(F, _holes(engine, M, side, 50 + i)) for i, (F, M) in enumerate(pairs)]
    singles = []
    for F, M in pairs:
        h = make(engine, side, nr, mu=0.05)
        load(engine, h, F, M)
        h.buildRBC()
        k = h.run()
        singles.append((k, h.read(engine.Memory.T).copy(), h.read(engine.Memory.PLANE_SYSTEM).copy(), h.read(engine.Memory.NORMALS_M).copy()))
        h.close()
    # one handle, three registrations
    g = make(engine, side, nr, mu=0.05, batch=n)
    for b, (F, M) in enumerate(pairs):
        load(engine, g, F, M, b)
    g.buildRBC()
    check_step(engine, g, 0.05, 1)                               # (one step of the whole handle, registration 1 against the restatement)
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
    bt.set_symmetric(True)
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


# ---- 3. off means off, point-to-point ignores it

def _configure(g, metric, side):
    if metric != "p2p":
        g.set_normals(GRID, side)
    if metric == "p2pl":
        g.set_error_metric(P2PL, 0.05)
    elif metric == "colored":
        g.set_color_weight(100.0)
        g.set_error_metric(COLORED, 0.05)
    elif metric == "gicp":
        g.set_error_metric(P2PL, 0.05)
        g.set_plane_to_plane(1e-3)


@pytest.mark.parametrize("metric", ["p2p", "p2pl", "colored", "gicp"])
def test_off_means_off(engine, metric):
    """The setting never touched, and set on and then off: a 4-iteration fixed run of each metric gives identical T bits; NORMALS_M
    stays zero where neither setting is on."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    out = []
    for touched in (False, True):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, nr, A, C_)
        _configure(g, metric, side)
        if touched:
            g.set_symmetric(True)
            assert g.symmetric() is True
            g.set_symmetric(False)
        assert g.symmetric() is False
        load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(4)
        out.append(g.read(engine.Memory.T).copy())
        if metric != "gicp":
            assert (g.read(engine.Memory.NORMALS_M) == 0).all()
        g.close()
    assert_bits(out[0], out[1], "T of " + metric)


def test_point_to_point_ignores_it(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    Ts = []
    for on in (False, True):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, nr, A, C_)
        g.set_symmetric(on)
        load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(4)
        Ts.append(g.read(engine.Memory.T).copy())
        g.close()
    assert_bits(Ts[0], Ts[1], "point-to-point T")


def test_survives_init_and_switching_captures_anew(engine):
    """The setting survives icp_init; on -> off -> on between fixed runs of the same length gives each time the bits of a handle that
    had the setting from the start (a graph captured under the other setting is not replayed)."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    want = {}
    for on in (False, True):
        h = make(engine, side, nr, mu=0.05, sym=on)
        load(engine, h, F, M)
        h.buildRBC()
        h.run_fixed(5)
        want[on] = h.read(engine.Memory.T).copy()
        h.close()
    assert not np.array_equal(want[False], want[True])
    g = make(engine, side, nr, mu=0.05, sym=True)
    g.init(side * side, nr, A, C_)
    assert g.symmetric() is True
    load(engine, g, F, M)
    for on in (True, False, True):
        g.set_symmetric(on)
        g.reset_transform(); g.buildRBC()
        g.run_fixed(5)
        assert_bits(g.read(engine.Memory.T), want[on], "T with symmetric %s" % on)
    g.close()


# ---- 4. the identity step

def test_all_weights_zero_is_the_identity_step_and_all_normals_zero_is_the_mu_share(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    g = make(engine, side, nr, normals=GIVEN, mu=0.05)
    load(engine, g, F, M)
    g.buildRBC()
    assert (g.read(engine.Memory.NORMALS_F) == 0).all() and (g.read(engine.Memory.NORMALS_M) == 0).all()
    s = check_step(engine, g, 0.05)
    assert s[27] == 1.0
    w = g.read(engine.Memory.W).astype(np.float64)
    assert s[15] > 0 and abs(s[15] - float(np.float32(0.05)) * w.sum()) <= 1e-9 * s[15]         # (term (3, 3): sum w mu)
    g.close()
    g = make(engine, side, nr, mu=0.05)
    g.set_rejection(False, 1e-3)                                # (a micron: every pair of the noisy scene is rejected)
    load(engine, g, F, M)
    g.buildRBC()
    T0 = g.read(engine.Memory.T).copy()
    s = check_step(engine, g, 0.05)
    assert (s == 0).all()
    assert (g.read(engine.Memory.W) == 0).all()
    assert_bits(g.read(engine.Memory.T), T0, "T")
    assert_bits(g.read(engine.Memory.TK), IDENTITY8, "TK")
    g.close()


# ---- 5. the refusals

def _refused(engine, g, *words):
    for call in (g.step, g.run, lambda: g.run_fixed(2), lambda: g.run_fixed_fresh(2)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == ESTATE, e.value
        for wd in words:
            assert wd in str(e.value), e.value


def test_refusals(engine):
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    # the colored metric: every run and step is refused, naming both settings
    g = make(engine, side, nr, mu=0.05)
    g.set_color_weight(100.0)
    g.set_error_metric(COLORED, 0.05)
    load(engine, g, F, M)
    g.buildRBC()
    _refused(engine, g, "icp_set_symmetric", "ICP_METRIC_COLORED")
    g.set_symmetric(False)                                      # (one of them off: it runs)
    g.buildRBC()
    g.step()
    g.close()
    # plane-to-plane at the same time: refused, naming both setters
    g = make(engine, side, nr, mu=0.05)
    g.set_plane_to_plane(1e-3)
    load(engine, g, F, M)
    g.buildRBC()
    _refused(engine, g, "icp_set_symmetric", "icp_set_plane_to_plane")
    g.set_plane_to_plane(0.0)
    g.reset_transform(); g.buildRBC()
    check_step(engine, g, 0.05)
    g.close()
    bt = engine.ICPBatch([0])
    bt.init(2, side * side, nr, A, C_)
    bt.set_normals(GRID, side)
    bt.set_error_metric(P2PL, 0.05)
    bt.set_plane_to_plane(1e-3)
    bt.set_symmetric(True)
    for i in range(2):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    with pytest.raises(engine.ICPError) as e:
        bt.run()
    assert e.value.code == ESTATE and "icp_set_symmetric" in str(e.value) and "icp_set_plane_to_plane" in str(e.value), e.value
    bt.close()
    # GRID: switching it on leaves the handle without moving normals until buildRBC has run again
    g = make(engine, side, nr, mu=0.05, sym=False)
    load(engine, g, F, M)
    g.buildRBC()
    g.step()
    assert (g.read(engine.Memory.NORMALS_M) == 0).all()
    g.set_symmetric(True)
    _refused(engine, g)
    g.reset_transform(); g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_M), ref.grid_normals(M, side), "NORMALS_M")
    check_step(engine, g, 0.05)
    M2 = _holes(engine, engine.synth_pair(side, seed=77)[1], side, 41)
    g.write(engine.Memory.M, M2)                                # (a later write of M: computed again, no buildRBC)
    assert_bits(g.read(engine.Memory.NORMALS_M), ref.grid_normals(M2, side), "NORMALS_M after a write of M")
    g.close()
    # tracking is not provided
    g = make(engine, side, nr, mu=0.05)
    frame = engine.synth_cloud_vga()
    for _ in range(2):
        with pytest.raises(engine.ICPError) as e:
            g.track_next(frame)
        assert e.value.code == ESTATE and "icp_set_symmetric" in str(e.value), e.value
    g.set_symmetric(False)
    assert g.track_next(frame) is None
    g.close()


# ---- 6. convergence, the one free-running check

def test_convergence_against_point_to_plane(engine):
    """Scene 0 at side 128 with the benchmark's motion, 20 % contiguous holes in both frames and ICP_REJECT_INVALID (the pair of
    tests/test_gpu_gicp.py::test_convergence_against_point_to_plane): a checked run of point-to-plane (mu = 0.05) and one of symmetric
    (mu = 0) on the same handle.  Point-to-plane is the reference.  Both converge; symmetric's rotation and translation errors against
    T_true are at most twice point-to-plane's (both minimise along-normal residuals of the same noisy grid normals), and its k is at most
    point-to-plane's.  Measured on an MI355X: point-to-plane 0.01036 deg / 0.2812 mm in 15 iterations,
    symmetric 0.00530 deg / 0.0884 mm in 7."""
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
    for name, mu, sym in (("point-to-plane", 0.05, False), ("symmetric", 0.0, True)):
        g.set_error_metric(P2PL, mu)
        g.set_symmetric(sym)
        g.reset_transform(); g.buildRBC()
        k = g.run()
        res[name] = _errors(g.read(engine.Memory.T), T_true) + (k, g.state().converged)
    g.close()
    (rp, tp, kp, cp), (rs, ts, ks, cs) = res["point-to-plane"], res["symmetric"]
    print("convergence: point-to-plane mu=0.05 %.5f deg %.4f mm k=%d conv=%d | symmetric mu=0 %.5f deg %.4f mm k=%d conv=%d"
          % (rp, tp, kp, cp, rs, ts, ks, cs))
    assert cp == 1 and cs == 1, res
    assert rs <= 2 * rp and ts <= 2 * tp, res
    assert ks <= kp, res
