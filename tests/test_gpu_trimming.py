"""Trimmed ICP (icp_set_trimming): every iteration keeps the closest fraction of the pairs that rejection leaves and gives the rest
the weight +0; the search is not touched.

The trimmed set comes from numpy — the rule of include/icp_amd.h applied to the engine's own NN / QT outputs (np.sort, geo <= t) —,
and the reference values from the oracle's piecewise entries with the trimmed and rejected rows zeroed (tests/test_gpu_rejection.py's
construction).  ICP_MEM_TRIM holds (t bits, n, K, accepted) of the last iteration."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks      # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, POWER, EIGEN, REGULAR, WEIGHTED, assert_bits, check_trim_step as check_step,  # noqa: E402
                        holes_pair as _holes, one_step, oracle_search, only_invalid, set_modes, trim_rule, weights_before_trim,
                        _partial_overlap, step_batch, _t0)

pytestmark = pytest.mark.gpu


def make_handle(engine, m, nr, fused, weighted, rot, power_fast, invalid, keep, batch=1):
    return icp_checks.make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid), trimming=keep)


@pytest.fixture(scope="module")
def scenes_A(engine, oracle):
    """name -> (F, M, T, invalid flag, the oracle's (nn_id, rid) at T): a clean pair and a blobs30 holes pair."""
    return icp_checks.scenes_A(engine, oracle)


# ---- 1. one step at A, every mode, clean and with holes

@pytest.mark.parametrize("keep", [0.5, 0.8])
@pytest.mark.parametrize("scene", ["clean", "holes"])
@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, scenes_A, fused, weighted, rot, power_fast, scene, keep):
    F, M, T, invalid, want = scenes_A[scene]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, rot, power_fast, invalid, keep)
    assert g.trimming() == pytest.approx(keep)
    one_step(engine, g, F, M, T)
    acc, trim = check_step(engine, oracle, g, F, M, T, 128, fused, weighted, rot, power_fast, invalid, keep, want)
    n, K = int(trim[1]), int(trim[2])
    assert K == int(np.ceil(np.float64(np.float32(keep)) * n)) and K <= trim[3] < n
    g.close()


def test_search_is_untouched(engine, scenes_A):
    """At the same T the correspondences and nearest representatives are those of a run with trimming off, bit for bit."""
    F, M, T, invalid, _ = scenes_A["holes"]
    out = []
    for keep in (1.0, 0.6):
        g = make_handle(engine, F.shape[0], 256, True, WEIGHTED, POWER, True, invalid, keep)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")


# ---- 2. sizes: B, a batch of 64 with different overlap, one above the single-workgroup selection

@pytest.mark.parametrize("fused,weighted,rot", [(True, WEIGHTED, POWER), (False, REGULAR, EIGEN)])
def test_one_step_config_B(engine, oracle, fused, weighted, rot):
    side, nr = 256, 1024
    F, M = _holes(engine, side, 0x1C9D5EED + 7)
    T = _t0()
    g = make_handle(engine, F.shape[0], nr, fused, weighted, rot, fused, True, 0.8)
    one_step(engine, g, F, M, T)
    check_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, fused, True, 0.8, oracle_search(oracle, F, M, T, nr))
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch64(engine, oracle, fused):
    """64 registrations of 16384 (the dense search) with different holes and motions: each has its own n, K and t."""
    from icp_amd import workloads as W
    side, nr, B = 128, 256, 64
    pairs = []
    for b in range(B):
        F, M = W.pair(engine, b)
        if b % 3:
            F, M = _holes(engine, side, W.BASE_SEED + 3 * b, "blobs30" if b % 3 == 1 else "scattered10")
        pairs.append((F, M))
    T = _t0()
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, True, 0.7, batch=B)
    step_batch(engine, g, pairs, T)
    ts = set()
    for b in range(B):
        F, M = pairs[b]
        PF, PM = g.read(engine.Memory.NN, batch_index=b), g.read(engine.Memory.QT, batch_index=b)
        nn_id = g.read(engine.Memory.NN_ID, batch_index=b)
        _, trim = trim_rule(PF, PM, weights_before_trim(nn_id, M, PF, PM, True, True), 0.7)
        assert np.array_equal(g.read(engine.Memory.TRIM, batch_index=b), trim), b
        ts.add(int(trim[0]))
    assert len(ts) > 32, "the registrations' thresholds differ"
    for b in W.CHECKED:
        F, M = pairs[b]
        check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, True, 0.7, oracle_search(oracle, F, M, T, nr), b=b)
    g.close()


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_one_step_2_18(engine, oracle, fused, weighted):
    """2^18 pairs: the selection in three multi-workgroup passes; the oracle's pieces fed the engine's own correspondences."""
    side, nr = 512, 1024
    F, M = _holes(engine, side, 0x1C9D5EED + 13, "blobs10")
    T = _t0()
    g = make_handle(engine, F.shape[0], nr, fused, weighted, POWER, fused, True, 0.75)
    one_step(engine, g, F, M, T)
    acc, trim = check_step(engine, oracle, g, F, M, T, side, fused, weighted, POWER, fused, True, 0.75)
    assert trim[1] > 200000
    g.close()


# ---- 3. ties and edges

def test_ties_at_t_are_kept(engine, oracle):
    """Integer coordinates moved by an integer translation: geo is an integer, many pairs share the value at t — all are kept."""
    side, nr = 128, 256
    j, i = np.mgrid[0:side, 0:side]
    F = np.zeros((side * side, 8), np.float32)
    F[:, 0] = (10 * i).reshape(-1) - 640
    F[:, 1] = (10 * j).reshape(-1) - 640
    F[:, 2] = 1000 + ((i * j) % 5).reshape(-1)
    F[:, 3] = 1.0
    F[:, 4:7] = 0.5
    M = F.copy()
    M[:, 0] -= 3.0
    M[:, 1] += 4.0
    T = IDENTITY.copy()
    for fused in (True, False):
        g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, False, 0.5)
        one_step(engine, g, F, M, T)
        acc, trim = check_step(engine, oracle, g, F, M, T, side, fused, WEIGHTED, POWER, fused, False, 0.5)
        t = np.uint32(trim[0]).view(np.float32)
        PF, PM = g.read(engine.Memory.NN), g.read(engine.Memory.QT)
        gg = (PM[:, :3] - PF[:, :3]).astype(np.float32)
        geo = (gg[:, 0] * gg[:, 0] + gg[:, 1] * gg[:, 1]) + gg[:, 2] * gg[:, 2]
        ties = geo == t
        assert np.count_nonzero(ties) > 1000 and trim[3] > trim[2], trim
        assert np.all(g.read(engine.Memory.W)[ties] != 0.0), "every tie at t is kept"
        g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_k_is_one(engine, oracle, scenes_A, fused):
    F, M, T, invalid, want = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, fused, WEIGHTED, POWER, fused, invalid, 1e-6)
    one_step(engine, g, F, M, T)
    _, trim = check_step(engine, oracle, g, F, M, T, 128, fused, WEIGHTED, POWER, fused, invalid, 1e-6, want)
    assert trim[2] == 1 and trim[3] >= 1
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_nothing_left_is_the_identity_step(engine, fused):
    """Every pair rejected before trimming (n == 0): the run stops after one identity step, T as it was, ICP_MEM_TRIM zeros."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    T0 = _t0()
    g = engine.ICP(0)
    g.init(side * side, nr, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    g.set_rejection(False, 1e-3)
    g.set_trimming(0.8)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0, block=True)
    assert g.run() == 1
    Mem = engine.Memory
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert np.all(g.read(Mem.TRIM) == 0)
    assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W) == 0.0)
    g.close()


def test_off_again_equals_never_trimmed(engine, scenes_A):
    """keep = 1 after trimming had been on (graphs cached with it): the same k, T, ids and weights as a handle that never trimmed,
    and ICP_MEM_TRIM reads zeros."""
    F, M, _, _, _ = scenes_A["holes"]
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        g.set_rejection(True, None)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        if toggled:
            g.set_trimming(0.7)
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(engine.Memory.TRIM)[1] > 0
            g.set_trimming(1.0)
            assert g.trimming() == 1.0
            assert np.all(g.read(engine.Memory.TRIM) == 0)
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy(),
                    g.read(engine.Memory.W).view(np.uint32).copy()))
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


# ---- 4. multi-iteration: run, run_fixed, icp_batch, tracking

@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_run_equals_steps(engine, scenes_A, fused, weighted):
    """A checked run and run_fixed with trimming on against the same iterations as single steps: T, weights and ICP_MEM_TRIM bit for
    bit (the lazily produced outputs of the run show the trimmed weights)."""
    F, M, _, invalid, _ = scenes_A["holes"]
    g = make_handle(engine, F.shape[0], 256, fused, weighted, POWER, fused, invalid, 0.8)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    Mem = engine.Memory
    run = [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.TRIM).copy(), g.read(Mem.NN_ID)["id"].copy()]
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    steps = [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.TRIM).copy(), g.read(Mem.NN_ID)["id"].copy()]
    for a, b, what in zip(run, steps, ("T", "W", "TRIM", "ids")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    # run_fixed (a cached graph) against steps
    n = 5
    g.reset_transform(); g.buildRBC()
    g.run_fixed(n)
    fixed = [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.TRIM).copy()]
    g.reset_transform(); g.buildRBC()
    for _ in range(n):
        g.step()
    for a, b, what in zip(fixed, [g.read(Mem.T), g.read(Mem.W), g.read(Mem.TRIM)], ("T", "W", "TRIM")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what
    g.close()


def test_icp_batch_equals_single_handles(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 4
    m = side * side
    pairs = [_holes(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    bt.set_trimming(0.8)
    assert bt.trimming() == pytest.approx(0.8)
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = engine.ICP(0)
        g.init(m, nr, A, C_)
        g.set_rejection(True, None)
        g.set_trimming(0.8)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        assert np.array_equal(bt.read(i, engine.Memory.TRIM), g.read(engine.Memory.TRIM)), i
        g.close()
    bt.close()


def test_tracking_equals_run_on_the_landmarks(engine, oracle):
    """icp_track_next on a hole-punched VGA sequence with trimming on equals ICP::run on the same landmark pairs."""
    frames = [engine.punch_holes(engine.synth_cloud_vga(moved=f), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=77 + f)
              for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    handles = []
    for _ in range(2):
        x = engine.ICP(0)
        x.init(16384, 256, A, C_)
        x.set_rejection(True, None)
        x.set_trimming(0.8)
        handles.append(x)
    g, h = handles
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h.write(engine.Memory.F, lms[i - 1]); h.write(engine.Memory.M, lms[i])
        h.reset_transform(); h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], h.read(engine.Memory.NN_ID)["id"]), i
        assert np.array_equal(g.read(engine.Memory.TRIM), h.read(engine.Memory.TRIM)), i
    g.close(); h.close()


def test_form_and_launch_count(engine):
    """With trimming on the iteration is the separate form: search, select (one launch up to 16384 pairs, three beyond), apply, the
    fused tail; off again, the chained form of the latency-bound size is back."""
    for side, sel in ((128, 1), (256, 3)):
        g = engine.ICP(0)
        g.init(side * side, 256, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0 = g.run_form()
        g.set_trimming(0.8)
        assert g.run_form() == 0
        tail = 3 if (side * side // 64 + 127) // 128 > 2 else 2
        assert g.launches_per_iteration() == tail + sel + 1
        g.set_trimming(1.0)
        assert g.run_form() == form0
        g.close()


# ---- 5. what it is for: partial overlap

@pytest.mark.parametrize("fused", [True, False])
def test_trimming_copes_with_partial_overlap(engine, fused):
    """Keeping 70 % of the pairs ends clearly closer to T_true than keeping all.  Measured on an MI355X (both reduce modes alike):
    untrimmed 0.431 deg / 8.27 mm, trimmed 0.157 deg / 3.12 mm; the bounds leave room on both sides.  (With the scene's default
    motion, 3 degrees and 31 mm, the band's pairs are no farther than the inliers' at the start and 0.7 locks onto a wrong alignment;
    0.8 gets there: DESIGN.md.)"""
    from icp_amd import workloads as W
    F, M, T_true = _partial_overlap(engine)
    res = {}
    for keep in (1.0, 0.7):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        set_modes(engine, g, power_fast=fused, fused=fused)
        g.set_trimming(keep)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        g.run()
        T = g.read(engine.Memory.T).copy()
        g.close()
        res[keep] = (W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])))
    (rot_off, t_off), (rot_on, t_on) = res[1.0], res[0.7]
    print("partial overlap %s: untrimmed %.3f deg %.2f mm, trimmed 0.7: %.3f deg %.2f mm"
          % ("fused" if fused else "reference order", rot_off, t_off, rot_on, t_on))
    assert t_off > 6.0 and rot_off > 0.3, res
    assert t_on < 4.5 and rot_on < 0.25, res
