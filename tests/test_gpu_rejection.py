"""Correspondence rejection (icp_set_rejection): pairs with an invalid endpoint (a Kinect pixel without depth: a point at the
origin) and / or pairs farther apart than max_dist get the weight +0; the search is not touched.

The reference values come from the oracle's piecewise entries, which take W as an input: for every rejected pair its row of W,
NN (the matched fixed point) and tM (the transformed moving point) is zeroed before the call — what "the pair contributes exact
zeros" means.  The rejected set itself is pinned against one computed in numpy from the engine's own per-query outputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_checks import (A, C_, IDENTITY, POWER, EIGEN, REGULAR, WEIGHTED, assert_bits, check_rejection_step as check_one_step,  # noqa: E402
                        holes_pair as _holes, pick_max_dist, set_modes, step_batch, _t0)
import icp_checks      # noqa: E402

pytestmark = pytest.mark.gpu


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, max_dist, batch=1):
    return icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=(invalid, max_dist))


KINDS = [("invalid", True, False), ("distance", False, True), ("both", True, True)]


@pytest.fixture(scope="module")
def pair_A(engine, oracle):
    side, nr = 128, 256
    F, M = _holes(engine, side, 0x1C9D5EED)
    T = _t0()
    return F, M, T, pick_max_dist(oracle, F, M, T, nr)


# ---- 1. off is off

def test_off_is_off(engine, pair_A):
    """Never set, set to (0, 0), and switched on (a graph cached with it) then off again: T, k and every id bit for bit."""
    F, M, _, md = pair_A
    m, nr = F.shape[0], 256
    out = []
    for how in ("never", "zero", "toggled"):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        if how == "zero":
            g.set_rejection(False, None)
            assert g.rejection() == (False, None)
        if how == "toggled":
            g.set_rejection(True, md)
            assert g.rejection() == (True, pytest.approx(md))
            g.buildRBC(); g.run()
            g.set_rejection(False, 0.0)
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy()))
        g.close()
    for k, T, ids in out[1:]:
        assert k == out[0][0]
        assert np.array_equal(T, out[0][1])
        assert np.array_equal(ids, out[0][2])


# ---- 2. one step, bit for bit, every mode

@pytest.mark.parametrize("kind,invalid,dist", KINDS)
@pytest.mark.parametrize("rot,power_fast", [(POWER, False), (POWER, True), (EIGEN, False)])
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, pair_A, fused, weighted, rot, power_fast, kind, invalid, dist):
    F, M, T, md = pair_A
    side, nr = 128, 256
    max_dist = md if dist else None
    g = make_handle(engine, F.shape[0], nr, fused, weighted, rot, power_fast, invalid, max_dist)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    g.step()
    rej = check_one_step(engine, oracle, g, F, M, T, side, nr, fused, weighted, rot, power_fast, invalid, max_dist)
    if dist:                                         # the distance test alone rejects 5 - 20 % of the valid pairs
        valid = ~((M[:, :3] == 0).all(axis=1) | (g.read(engine.Memory.NN)[:, :3] == 0).all(axis=1))
        frac = np.count_nonzero(rej & valid) / np.count_nonzero(valid)
        assert 0.05 <= frac <= 0.2, frac
    g.close()


# ---- 3. teacher-forced run

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_teacher_forced_run(engine, oracle, pair_A, fused, weighted):
    """A checked run with rejection on (per-query outputs every iteration) to its end, then the same iterations as single steps
    from the same start: every iteration's Tk against the oracle's pieces fed the engine's own T, and the steps end where the run
    ended — the same T, correspondences and weights."""
    F, M, _, md = pair_A
    side, nr = 128, 256
    power_fast = fused
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, power_fast, True, md)
    g.set_output_mode(True)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()                                      # (converged, or max_iterations)
    assert 1 < k <= 40, k
    T_run, ids_run, w_run = g.read(engine.Memory.T).copy(), g.read(engine.Memory.NN_ID)["id"].copy(), g.read(engine.Memory.W).copy()
    g.reset_transform(); g.buildRBC()
    for it in range(k):
        T = g.read(engine.Memory.T).copy()
        g.step()
        check_one_step(engine, oracle, g, F, M, T, side, nr, fused, weighted, POWER, power_fast, True, md)
    assert_bits(g.read(engine.Memory.T), T_run, "T of the steps")
    assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], ids_run)
    assert_bits(g.read(engine.Memory.W), w_run, "last weights")
    g.close()


# ---- 4. dense, batched and tracked

@pytest.mark.parametrize("fused,weighted,rot", [(True, WEIGHTED, POWER), (False, REGULAR, EIGEN)])
def test_one_step_config_B(engine, oracle, fused, weighted, rot):
    side, nr = 256, 1024
    F, M = _holes(engine, side, 0x1C9D5EED + 7)
    T = _t0()
    md = pick_max_dist(oracle, F, M, T, nr)
    g = make_handle(engine, F.shape[0], nr, fused, weighted, rot, fused, True, md)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    g.step()
    check_one_step(engine, oracle, g, F, M, T, side, nr, fused, weighted, rot, fused, True, md)
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch64(engine, oracle, fused):
    """64 registrations of 16384 with holes in one handle (the dense search): the one-step checks on eight of them."""
    from icp_amd import workloads as W
    side, nr, B = 128, 256, 64
    pairs = [_holes(engine, side, W.BASE_SEED + 3 * b, "blobs30" if b % 2 else "scattered10") for b in range(B)]
    T = _t0()
    md = pick_max_dist(oracle, pairs[0][0], pairs[0][1], T, nr)
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, md, batch=B)
    step_batch(engine, g, pairs, T)
    for b in W.CHECKED:
        F, M = pairs[b]
        check_one_step(engine, oracle, g, F, M, T, side, nr, fused, WEIGHTED, POWER, fused, True, md, b=b)
    g.close()


def test_icp_batch_equals_single_handles(engine):
    """icp_batch_*: every registration equals a single handle with the same setting."""
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [_holes(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, 60.0)
    assert bt.rejection() == (True, 60.0)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_rejection(True, 60.0)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        g.close()
    bt.close()


def test_tracking_equals_run_on_the_landmarks(engine, oracle):
    """icp_track_next on a hole-punched VGA sequence with rejection on equals ICP::run on the same landmark pairs."""
    frames = [engine.punch_holes(engine.synth_cloud_vga(moved=f), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=77 + f)
              for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    g = engine.ICP(0)
    g.init(16384, 256, A, C_)
    g.set_rejection(True, 60.0)
    h = engine.ICP(0)
    h.init(16384, 256, A, C_)
    h.set_rejection(True, 60.0)
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h.write(engine.Memory.F, lms[i - 1]); h.write(engine.Memory.M, lms[i])
        h.reset_transform(); h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], h.read(engine.Memory.NN_ID)["id"]), i
    g.close(); h.close()


# ---- 5. what it is for

def _accuracy(engine, F, M, T_true, fused, invalid, max_dist):
    from icp_amd import workloads as W
    g = engine.ICP(0)
    g.init(F.shape[0], 256, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    if invalid or max_dist:
        g.set_rejection(invalid, max_dist)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run()
    T = g.read(engine.Memory.T).copy()
    g.close()
    return W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7]))


@pytest.mark.parametrize("fused", [True, False])
def test_rejection_removes_the_bias_of_holes(engine, fused):
    """A scene with known T_true and contiguous holes (30 %) at different places in F and M: with the invalid-point rule and a cap
    of 60 mm (above the initial misalignment) the registration is clearly closer to T_true than without rejection."""
    F, M, T_true = engine.synth_pair_scene(128)
    F = engine.punch_holes(F, 128, 128, engine.HOLES_CONTIGUOUS, 0.3, True, seed=0x1C9D5EED + 101)
    M = engine.punch_holes(M, 128, 128, engine.HOLES_CONTIGUOUS, 0.3, True, seed=0x1C9D5EED + 202)
    rot_off, t_off = _accuracy(engine, F, M, T_true, fused, False, None)
    rot_on, t_on = _accuracy(engine, F, M, T_true, fused, True, 60.0)
    print("rejection %s: off %.3f deg %.2f mm, on %.3f deg %.2f mm" % ("fused" if fused else "reference order", rot_off, t_off, rot_on, t_on))
    assert t_off > 20.0 and rot_off > 0.5, (rot_off, t_off)
    assert t_on < 15.0 and rot_on < 0.4, (rot_on, t_on)


# ---- 6. nothing accepted

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("holes", [True, False])
def test_nothing_accepted_is_the_identity_step(engine, fused, holes):
    """A cap that rejects every pair: the run stops after one iteration with the identity step, T as it was, means / S / sum W 0 and
    no NaN anywhere in the state."""
    side, nr = 128, 256
    m = side * side
    F, M = _holes(engine, side, 0x1C9D5EED) if holes else engine.synth_pair(side)
    T0 = _t0()
    g = engine.ICP(0)
    g.init(m, nr, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    g.set_rejection(holes, 1e-3)                     # (holes: the invalid <-> invalid pairs lie at distance 0 and need the flag)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0, block=True)
    assert g.run() == 1
    Mem = engine.Memory
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert_bits(g.read(Mem.RK).reshape(-1), np.eye(3, dtype=np.float32).reshape(-1), "Rk")
    assert np.all(g.read(Mem.S).view(np.uint32) == 0) and np.all(g.read(Mem.MEANS).view(np.uint32) == 0)
    assert g.read(Mem.SUM_W)[0] == 0.0
    assert np.all(g.read(Mem.W) == 0.0)
    st = g.state()
    for f in ("R", "q", "t", "Rk", "qk", "tk"):
        assert np.isfinite(np.array(list(getattr(st, f)), np.float32)).all(), f
    assert np.isfinite(st.s) and np.isfinite(st.sk) and st.converged
    g.close()
