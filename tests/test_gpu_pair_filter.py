"""Rejection at the fixed grid's boundary (icp_set_boundary_rejection) and by normal compatibility (icp_set_normal_rejection): a
candidate pair that a rule rejects gets the weight +0 and is then a rejected pair.  The search is not touched.

The masks come from numpy — tests/pair_filter_ref.py, from the engine's own NN_ID / NN / QT outputs, the weights before the rules, F,
NORMALS_F / NORMALS_M and R as read back —, and the reference values from the oracle's piecewise entries with the rejected rows zeroed
(tests/test_gpu_trimming.py's construction).  ICP_MEM_PAIR_FILTER holds (n, at_boundary, incompatible, accepted) of the last
iteration.  Everything is compared bit for bit.

MIN_COS = 0.95: with the CPU oracle's correspondences at _t0 () and the numpy grid normals of both frames, the pairs' cosines have
their 80th percentile at 0.9494 (clean pair) and 0.9486 (holes pair): the synthetic frames' noise tilts the 128 x 128 grid normals a
lot.  COUNTS records what the numpy rule gives there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                 # noqa: E402
import pair_filter_ref as ref                                   # noqa: E402
import robust_ref                                               # noqa: E402
import icp_checks      # noqa: E402
from icp_checks import (A, C_, IDENTITY, MODES, POWER, EIGEN, REGULAR, WEIGHTED, assert_bits,  # noqa: E402
                        check_pair_filter_step as check_step, expected_pieces, holes_pair as _holes, one_step, oracle_search,
                        only_invalid, pair_filter_rule_of as numpy_rule, set_modes, trim_rule,
                        _partial_overlap, _t0)

pytestmark = pytest.mark.gpu

MIN_COS = 0.95
RULES = {"boundary": (True, None), "normal": (False, MIN_COS), "both": (True, MIN_COS)}
# (n, at_boundary, incompatible, accepted) of the numpy rule on the CPU oracle's correspondences at _t0 (), side 128, |R| = 256
COUNTS = {("clean", "boundary"): [16384, 1659, 0, 14725], ("clean", "normal"): [16384, 0, 13124, 3260],
          ("clean", "both"): [16384, 1659, 12070, 2655], ("holes", "boundary"): [11429, 4543, 0, 6886],
          ("holes", "normal"): [11429, 0, 9235, 2194], ("holes", "both"): [11429, 4543, 5564, 1322]}
# What the header documents for icp_launches_per_iteration: the pass + the apply pass on point-to-point, the pass on the plane metrics.
ADDED_P2P, ADDED_PLANE = 2, 1


def make_handle(engine, side, nr, fused, weighted, rot, power_fast, invalid, boundary, min_cos, batch=1, gw=None):
    return icp_checks.make_handle(engine, side * side, nr, fused, weighted, rot, power_fast, batch, rejection=only_invalid(invalid),
                                  boundary=(gw or side) if boundary else None,
                                  normal_rejection=(gw or side, min_cos) if min_cos is not None else None)


@pytest.fixture(scope="module")
def scenes_A(engine, oracle):
    """name -> (F, M, T, invalid flag, the oracle's (nn_id, rid) at T): a clean pair and a blobs30 holes pair."""
    return icp_checks.scenes_A(engine, oracle)


# ---- 0. arguments and getters

def test_arguments_and_getters(engine):
    g = engine.ICP(0)
    L = engine.lib()
    assert g.normal_rejection() is None and g.boundary_rejection() is None
    assert L.icp_set_normal_rejection(g._h, 2, 0.5) == 1 and L.icp_set_normal_rejection(g._h, -1, 0.5) == 1      # ICP_EINVAL
    for c in (float("nan"), 1.0000001, -1.5, float("inf")):
        assert L.icp_set_normal_rejection(g._h, 1, c) == 1, c
    assert g.normal_rejection() is None
    g.set_normal_rejection(0.5); g.set_boundary_rejection(16)
    assert g.normal_rejection() == 0.5 and g.boundary_rejection() == 16
    fl = C.c_int32(7)
    assert L.icp_get_rejection(g._h, C.byref(fl), None) == 0 and fl.value == 0       # (the rules' bits are no rejection flags)
    g.init(256, 16, A, C_)                               # both settings survive icp_init
    assert g.normal_rejection() == 0.5 and g.boundary_rejection() == 16
    assert np.all(g.read(engine.Memory.PAIR_FILTER) == 0)                # (no iteration yet)
    assert g.run_form() == 0
    assert L.icp_set_boundary_rejection(g._h, 7) == 4                    # ICP_ESTATE: 256 % 7 != 0
    assert "multiple of the grid width" in L.icp_last_error(g._h).decode()
    assert g.boundary_rejection() == 16
    g.set_normal_rejection(-1.0); g.set_normal_rejection(1.0)
    assert g.normal_rejection() == 1.0
    g.set_normal_rejection(None); g.set_boundary_rejection(None)
    assert g.normal_rejection() is None and g.boundary_rejection() is None
    on, c = C.c_int32(7), C.c_float(7)
    assert L.icp_get_normal_rejection(g._h, C.byref(on), C.byref(c)) == 0 and (on.value, c.value) == (0, 0.0)
    g.close()


def test_a_width_that_does_not_divide_m_is_refused_by_build_rbc(engine):
    g = engine.ICP(0)
    g.set_boundary_rejection(24)                         # (no m yet: accepted, as icp_set_normals accepts its width)
    g.init(256, 16, A, C_)
    F, M = engine.synth_pair(16)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    with pytest.raises(engine.ICPError) as e:
        g.buildRBC()
    assert e.value.code == 4 and "icp_set_boundary_rejection" in str(e.value)
    g.set_boundary_rejection(32)                         # 8 rows of 32
    g.buildRBC(); g.step()
    assert g.read(engine.Memory.PAIR_FILTER)[0] == 256
    g.close()


def test_switching_the_normal_rule_on_with_grid_normals_needs_a_new_build(engine):
    F, M = engine.synth_pair(16)
    g = engine.ICP(0)
    g.init(256, 16, A, C_)
    g.set_normals(1, 16)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC(); g.step()
    assert np.all(g.read(engine.Memory.NORMALS_M) == 0), "point-to-point without the rule computes no moving normals"
    g.set_normal_rejection(0.0)
    with pytest.raises(engine.ICPError) as e:
        g.step()
    assert e.value.code == 4
    g.buildRBC()
    assert_bits(g.read(engine.Memory.NORMALS_M), p2pl_ref.grid_normals(M, 16), "NORMALS_M from the grid")
    M2 = M.copy(); M2[:, 2] += np.linspace(0, 30, 256, dtype=np.float32)
    g.write(engine.Memory.M, M2)                         # a later write of M computes them again
    assert_bits(g.read(engine.Memory.NORMALS_M), p2pl_ref.grid_normals(M2, 16), "NORMALS_M follow M")
    g.step()
    g.close()


# ---- 1. one step at the latency layout, every mode, each rule alone and both, clean and with holes

@pytest.mark.parametrize("scene", ["clean", "holes"])
@pytest.mark.parametrize("rule", ["boundary", "normal", "both"])
@pytest.mark.parametrize("rot,power_fast", MODES)
@pytest.mark.parametrize("weighted", [WEIGHTED, REGULAR])
@pytest.mark.parametrize("fused", [True, False])
def test_one_step_config_A(engine, oracle, scenes_A, fused, weighted, rot, power_fast, rule, scene):
    F, M, T, invalid, want = scenes_A[scene]
    boundary, min_cos = RULES[rule]
    g = make_handle(engine, 128, 256, fused, weighted, rot, power_fast, invalid, boundary, min_cos)
    R0 = one_step(engine, g, F, M, T)
    counts, _ = check_step(engine, oracle, g, F, M, T, R0, 128, fused, weighted, rot, power_fast, invalid, 128 if boundary else None, min_cos, want)
    n = int(counts[0])
    if boundary:
        assert 0.01 * n <= counts[1] <= 0.9 * n, counts
    else:
        assert counts[1] == 0
    if min_cos is not None:
        assert 0.01 * n <= counts[2] <= 0.9 * n, counts
    else:
        assert counts[2] == 0
    assert counts.tolist() == COUNTS[scene, rule], counts
    g.close()


# ---- 2. small and odd shapes, a batch, 65536 pairs

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr,gw", [(50, 4, 50), (50, 4, 20), (30, 4, 30), (30, 4, 90)])
def test_small_shapes(engine, oracle, side, nr, gw, fused):
    """m = 2500 and 900: no multiple of 256, blocks with lanes past m, rows no power of two; a grid width other than the side."""
    F, M = engine.synth_pair(side)
    T = _t0()
    g = make_handle(engine, side, nr, fused, WEIGHTED, POWER, fused, False, True, 0.5, gw=gw)
    R0 = one_step(engine, g, F, M, T)
    counts, _ = check_step(engine, oracle, g, F, M, T, R0, side, fused, WEIGHTED, POWER, fused, False, gw, 0.5, oracle_search(oracle, F, M, T, nr))
    assert counts[0] == side * side and counts[1] > 0 and counts[3] > 0, counts
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_one_step_batch3(engine, oracle, fused):
    from icp_amd import workloads as W
    side, nr, B = 128, 256, 3
    pairs = [W.pair(engine, 0), _holes(engine, side, W.BASE_SEED + 3, "blobs30"), _holes(engine, side, W.BASE_SEED + 6, "scattered10")]
    T = _t0()
    g = make_handle(engine, side, nr, fused, WEIGHTED, POWER, fused, True, True, MIN_COS, batch=B)
    for b, (F, M) in enumerate(pairs):
        g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
    g.buildRBC()
    R0 = []
    for b in range(B):
        g.write(engine.Memory.T, T, batch_index=b, block=True)
        R0.append(g.read(engine.Memory.R, batch_index=b).ravel().copy())
    g.step()
    seen = set()
    for b, (F, M) in enumerate(pairs):
        counts, _ = check_step(engine, oracle, g, F, M, T, R0[b], side, fused, WEIGHTED, POWER, fused, True, side, MIN_COS,
                               oracle_search(oracle, F, M, T, nr), b=b)
        seen.add(tuple(counts.tolist()))
    assert len(seen) == B, seen                          # each registration keeps its own counts
    g.close()


@pytest.mark.parametrize("fused,weighted,rot", [(True, WEIGHTED, POWER), (False, REGULAR, EIGEN)])
def test_one_step_65536(engine, oracle, fused, weighted, rot):
    """m = 65536, |R| = 1024: the pass spans 256 blocks; the oracle's pieces fed the engine's own correspondences."""
    side, nr = 256, 1024
    F, M = _holes(engine, side, 0x1C9D5EED + 7)
    T = _t0()
    g = make_handle(engine, side, nr, fused, weighted, rot, fused, True, True, MIN_COS)
    R0 = one_step(engine, g, F, M, T)
    counts, _ = check_step(engine, oracle, g, F, M, T, R0, side, fused, weighted, rot, fused, True, side, MIN_COS)
    assert counts[1] > 1000 and counts[2] > 1000 and counts[3] > 1000, counts
    g.close()


# ---- 3. edges

@pytest.mark.parametrize("fused", [True, False])
def test_corner_edge_hole_and_beside_a_hole(engine, oracle, fused):
    """M = F at the identity: query i is matched to fixed point i (geo 0).  A hole punched into the fixed grid and one at its rim: the
    pairs at a corner, on an edge, beside a hole and — the hole itself being matched to whatever is nearest — all behave by the rule."""
    side, nr = 32, 64
    F, _ = engine.synth_pair(side)
    F = F.copy()
    hole, rim_hole = 10 * side + 12, 17 * side + 0
    F[hole, :3] = 0.0
    F[rim_hole, :3] = 0.0
    M = F.copy()
    g = make_handle(engine, side, nr, fused, WEIGHTED, POWER, fused, False, True, None)
    R0 = one_step(engine, g, F, M, IDENTITY.copy())
    ids = g.read(engine.Memory.NN_ID)["id"]
    keep = np.ones(side * side, bool); keep[[hole, rim_hole]] = False
    assert np.array_equal(ids[keep], np.arange(side * side, dtype=np.uint32)[keep]), "every valid point is its own nearest neighbour"
    counts, (bnd, _, acc) = check_step(engine, oracle, g, F, M, IDENTITY.copy(), R0, side, fused, WEIGHTED, POWER, fused, False, side, None)
    W = g.read(engine.Memory.W)
    for i in (0, side - 1, side * side - 1, 5, 7 * side, 9 * side + 11, 9 * side + 12, 10 * side + 11, 11 * side + 13, 16 * side + 1, 18 * side + 1):
        assert bnd[i] and W[i].view(np.uint32) == 0, i   # corners, edges, the 8 neighbours of the hole, beside the rim's hole
    for i in (8 * side + 12, 10 * side + 14, 12 * side + 10, 17 * side + 2):
        assert acc[i] and W[i] != 0, i                   # two away from a hole
    # the hole itself as a fixed point: no valid query claims it; as a query (at the origin, no rejection flag) it is matched somewhere
    assert bnd[hole] == ref.boundary_mask(F, side)[ids[hole]]
    # (the two queries at the origin are matched to a point at the origin, geo 0: a boundary point either way)
    interior = (side - 2) ** 2 - 9 - 3                   # the hole and its 8 neighbours, the 3 interior neighbours of the rim's hole
    assert counts.tolist() == [side * side, side * side - interior, 0, interior], counts
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_given_normals_at_the_threshold(engine, oracle, fused):
    """ICP_NORMALS_GIVEN, the identity (R = I): N_Q = (1, 1, 0) everywhere, N_M = (1, 0, 1) — 60 degrees, o = 1 = 0.5 sqrt (2 * 2)
    exactly —, (1 - ulp, 0, 1) just below and (1 + ulp, 0, 1) just above; min_cos = 0.5."""
    side, nr = 32, 64
    m = side * side
    F, M = engine.synth_pair(side)
    one = np.float32(1)
    NF = np.zeros((m, 4), np.float32); NF[:, :2] = 1.0
    NM = np.zeros((m, 4), np.float32); NM[:, 0] = 1.0; NM[:, 2] = 1.0
    NM[1::3, 0] = np.nextafter(one, np.float32(0)); NM[2::3, 0] = np.nextafter(one, np.float32(2))
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(m, nr, A, C_)
    set_modes(engine, g, fused, fused)
    g.set_normal_rejection(0.5)                          # (GIVEN normals: no new build needed, none computed)
    Mem = engine.Memory
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    g.write(Mem.NORMALS_F, NF); g.write(Mem.NORMALS_M, NM)
    g.write(Mem.T, IDENTITY.copy(), block=True)
    R0 = g.read(Mem.R).ravel().copy()
    assert np.array_equal(R0, np.eye(3, dtype=np.float32).ravel())
    g.step()
    counts, (_, inc, acc) = check_step(engine, oracle, g, F, M, IDENTITY.copy(), R0, side, fused, WEIGHTED, POWER, fused, False, None, 0.5)
    assert acc[0::3].all() and inc[1::3].all() and acc[2::3].all()
    assert counts.tolist() == [m, 0, len(range(1, m, 3)), m - len(range(1, m, 3))]
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_normals_left_at_zero_reject_everything(engine, fused):
    """GIVEN normals nobody wrote: no pair can be shown compatible, even at min_cos = -1 — the identity step, T unchanged."""
    side, nr = 32, 64
    F, M = engine.synth_pair(side)
    T0 = _t0()
    Mem = engine.Memory
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, nr, A, C_)
    set_modes(engine, g, fused, fused)
    g.set_normal_rejection(-1.0)
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    g.write(Mem.T, T0, block=True)
    assert g.run() == 1
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert g.read(Mem.PAIR_FILTER).tolist() == [side * side, 0, side * side, 0]
    assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W).view(np.uint32) == 0)
    g.close()


def test_min_cos_minus_one_on_complete_normals(engine, oracle):
    """Every pair has both normals (GIVEN, random directions): min_cos = -1 finds none incompatible."""
    side, nr = 32, 64
    m = side * side
    F, M = engine.synth_pair(side)
    rng = np.random.default_rng(11)
    NF = np.zeros((m, 4), np.float32); NM = np.zeros((m, 4), np.float32)
    NF[:, :3] = rng.normal(size=(m, 3)); NM[:, :3] = rng.normal(size=(m, 3))
    NM[:64, :3] = -NF[:64, :3]
    Mem = engine.Memory
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(m, nr, A, C_)
    g.set_normal_rejection(-1.0)
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    g.write(Mem.NORMALS_F, NF); g.write(Mem.NORMALS_M, NM)
    T = _t0()
    g.write(Mem.T, T, block=True)
    R0 = g.read(Mem.R).ravel().copy()
    g.step()
    counts, _ = check_step(engine, oracle, g, F, M, T, R0, side, True, WEIGHTED, POWER, True, False, None, -1.0)
    assert counts.tolist() == [m, 0, 0, m]
    g.close()


# ---- 4. the search is untouched; off again equals never on

def test_search_is_untouched(engine, scenes_A):
    F, M, T, invalid, _ = scenes_A["holes"]
    out = []
    for on in (False, True):
        g = make_handle(engine, 128, 256, True, WEIGHTED, POWER, True, invalid, on, MIN_COS if on else None)
        one_step(engine, g, F, M, T)
        out.append((g.read(engine.Memory.NN_ID).copy(), g.read(engine.Memory.RID).copy(), g.read(engine.Memory.QT).copy(),
                    g.read(engine.Memory.NN)[:, :3].copy()))
        g.close()
    assert np.array_equal(out[0][0]["id"], out[1][0]["id"]) and np.array_equal(out[0][1], out[1][1])
    assert_bits(out[0][0]["dist"], out[1][0]["dist"], "distances")
    assert_bits(out[0][2], out[1][2], "transformed moving points")
    assert_bits(out[0][3], out[1][3], "matched fixed points")


def test_off_again_equals_never_on(engine, scenes_A):
    F, M, _, _, _ = scenes_A["holes"]
    out = []
    for toggled in (False, True):
        g = engine.ICP(0)
        g.init(F.shape[0], 256, A, C_)
        g.set_rejection(True, None)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        form0 = g.run_form()
        if toggled:
            g.set_boundary_rejection(128); g.set_normals(1, 128); g.set_normal_rejection(MIN_COS)
            assert g.run_form() == 0
            g.buildRBC(); g.run(); g.run_fixed(3)
            assert g.read(engine.Memory.PAIR_FILTER)[3] > 0
            g.set_boundary_rejection(None)
            assert g.read(engine.Memory.PAIR_FILTER)[0] > 0      # (one rule is still on)
            g.set_normal_rejection(None)
            assert np.all(g.read(engine.Memory.PAIR_FILTER) == 0)
            g.set_normals(0, 0)
            assert g.run_form() == form0
            g.reset_transform()
        g.buildRBC()
        k = g.run()
        out.append((k, g.read(engine.Memory.T).view(np.uint32).copy(), g.read(engine.Memory.NN_ID)["id"].copy(),
                    g.read(engine.Memory.W).view(np.uint32).copy()))
        g.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


# ---- 5. composition

@pytest.mark.parametrize("fused", [True, False])
def test_with_one_to_one(engine, oracle, scenes_A, fused):
    """A rejected pair claims no fixed point: ICP_MEM_UNIQUE's n is this pass's accepted, the winners numpy's rule on the accepted."""
    import unique_ref
    F, M, T, invalid, want = scenes_A["holes"]
    Mem = engine.Memory
    g = make_handle(engine, 128, 256, fused, WEIGHTED, POWER, fused, invalid, True, MIN_COS)
    g.set_unique(True)
    assert g.launches_per_iteration() == (2 if fused else 4) + 1 + 3     # (tail, the pass, claim + resolve + apply)
    R0 = one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    assert np.array_equal(nn_id["id"], want[0]["id"])
    zero, counts, W0, (_, _, acc) = numpy_rule(engine, g, F, M, R0, True, invalid, 128, MIN_COS)
    assert np.array_equal(g.read(Mem.PAIR_FILTER), counts)
    W1 = np.where(acc, W0, np.float32(0)).astype(np.float32)
    win, cand, ucounts = unique_ref.unique_rule(nn_id["id"], g.read(Mem.NN), g.read(Mem.QT), W1)
    got = g.read(Mem.UNIQUE)
    assert np.array_equal(got, ucounts) and got[0] == counts[3] and 0 < got[1] < got[0], (got, ucounts, counts)
    W, sw, means, S, Tk = expected_pieces(oracle, F, M, T, nn_id, 128, fused, True, POWER, fused, ~win)
    assert_bits(g.read(Mem.W), W, "weights")
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits(g.read(Mem.TK), Tk, "Tk")
    g.close()


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_with_trimming(engine, oracle, scenes_A, fused, weighted):
    """Trimming's candidates are the accepted pairs: ICP_MEM_TRIM's n is `accepted`."""
    F, M, T, invalid, want = scenes_A["holes"]
    keep = 0.8
    Mem = engine.Memory
    g = make_handle(engine, 128, 256, fused, weighted, POWER, fused, invalid, True, MIN_COS)
    g.set_trimming(keep)
    assert g.launches_per_iteration() == (2 if fused else 4) + 2 + 1     # (tail, select + apply, the pass)
    R0 = one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    assert np.array_equal(nn_id["id"], want[0]["id"])
    _, counts, W0, (_, _, acc0) = numpy_rule(engine, g, F, M, R0, weighted, invalid, 128, MIN_COS)
    assert np.array_equal(g.read(Mem.PAIR_FILTER), counts)
    acc, trim = trim_rule(g.read(Mem.NN), g.read(Mem.QT), np.where(acc0, W0, np.float32(0)).astype(np.float32), keep)
    got = g.read(Mem.TRIM)
    assert np.array_equal(got, trim), ("ICP_MEM_TRIM", got, trim)
    assert got[1] == counts[3] and got[3] < got[1]
    W, sw, means, S, Tk = expected_pieces(oracle, F, M, T, nn_id, 128, fused, weighted, POWER, fused, ~acc)
    assert_bits(g.read(Mem.W), W, "weights")
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits(g.read(Mem.TK), Tk, "Tk")
    g.close()


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_with_a_huber_loss(engine, oracle, scenes_A, fused, weighted):
    """The loss weighs the accepted pairs: W' = robust_ref.p2p_weights on the weights behind the rules."""
    F, M, T, invalid, _ = scenes_A["holes"]
    scale = 8.0
    Mem = engine.Memory
    g = make_handle(engine, 128, 256, fused, weighted, POWER, fused, invalid, True, MIN_COS)
    g.set_robust_loss(robust_ref.HUBER, scale)
    assert g.launches_per_iteration() == (2 if fused else 4) + 1 + 1     # (tail, the loss's apply pass, the pass)
    R0 = one_step(engine, g, F, M, T)
    nn_id = g.read(Mem.NN_ID)
    _, counts, W0, (_, _, acc) = numpy_rule(engine, g, F, M, R0, weighted, invalid, 128, MIN_COS)
    assert np.array_equal(g.read(Mem.PAIR_FILTER), counts)
    PF, PM = g.read(Mem.NN), g.read(Mem.QT)
    W = robust_ref.p2p_weights(np.where(acc, W0, np.float32(0)).astype(np.float32), PF, PM, robust_ref.HUBER, scale)
    assert_bits(g.read(Mem.W), W, "W'")
    assert np.count_nonzero(W) == counts[3] and np.count_nonzero((W != 0) & (W != W0)) > 100
    zero = W == 0
    NNz, tMz = np.ascontiguousarray(F[nn_id["id"]]), oracle.transform_q(M, T)
    NNz[zero] = 0.0; tMz[zero] = 0.0
    if fused:
        sw, means, S = oracle.moments_fused(NNz, tMz, W, 128, C_)
    else:
        sw = robust_ref.sum_w_reference(W)
        means = oracle.mean_weighted(NNz, tMz, W, sw)
        DF, DM = oracle.devs(NNz, tMz, means)
        S = oracle.sij(DM, DF, W, C_)
    Tk, _ = oracle.power_method(S, means, fast=fused)
    assert_bits(g.read(Mem.SUM_W), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), means, "means")
    assert_bits(g.read(Mem.S), S, "S")
    assert_bits(g.read(Mem.TK), Tk, "Tk")
    g.close()


@pytest.mark.parametrize("fused", [True, False])
def test_with_point_to_plane(engine, scenes_A, fused):
    """ICP_MEM_PLANE_SYSTEM, T, R, TK against tests/p2pl_ref.py's float64 restatement fed the accepted pairs' weights, three steps."""
    F, M, _, invalid, _ = scenes_A["holes"]
    mu, side = 0.05, 128
    Mem = engine.Memory
    g = engine.ICP(0, POWER, WEIGHTED)
    g.init(side * side, 256, A, C_)
    set_modes(engine, g, fused, fused)
    g.set_normals(1, side)
    g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, mu)
    g.set_rejection(True, None)
    g.set_boundary_rejection(side); g.set_normal_rejection(MIN_COS)
    assert g.run_form() == 0 and g.launches_per_iteration() == 1 + 2 + ADDED_PLANE
    g.write(Mem.F, F); g.write(Mem.M, M)
    g.buildRBC()
    for _ in range(3):
        T0, R0 = g.read(Mem.T).copy(), g.read(Mem.R).ravel().copy()
        g.step()
        zero, counts, W0, _ = numpy_rule(engine, g, F, M, R0, True, invalid, side, MIN_COS)
        assert np.array_equal(g.read(Mem.PAIR_FILTER), counts) and 0 < counts[3] < counts[0] and counts[1] > 0 and counts[2] > 0
        PF = g.read(Mem.NN).copy()
        assert_bits(PF[:, 3], np.where(zero, np.float32(0), W0).astype(np.float32), "weights")
        PF[:, 3] = np.where(zero, np.float32(0), W0)
        system, T, R, Tk, Rk = p2pl_ref.step(PF, g.read(Mem.QT), g.read(Mem.NN_ID)["id"], g.read(Mem.NORMALS_F), mu, T0, R0)
        assert system[27] == 1.0
        assert_bits(g.read(Mem.PLANE_SYSTEM), system, "PLANE_SYSTEM")
        assert_bits(g.read(Mem.T), T, "T")
        assert_bits(g.read(Mem.R).ravel(), R, "R")
        assert_bits(g.read(Mem.TK), Tk, "TK")
    g.close()


@pytest.mark.parametrize("metric", ["colored", "plane_to_plane", "symmetric"])
def test_other_plane_metrics_equal_removal_by_rejection(engine, scenes_A, metric):
    """Colored, plane-to-plane and symmetric: a step with the rules on equals a step with the rules off on a moving set whose rejected
    pairs were removed another way — put at the origin, which ICP_REJECT_INVALID rejects — (tests/test_gpu_unique.py's construction)."""
    F, M, T, invalid, _ = scenes_A["holes"]
    side = 128
    Mem = engine.Memory

    def handle(on):
        g = engine.ICP(0, POWER, WEIGHTED)
        g.init(side * side, 256, A, C_)
        g.set_normals(1, side)
        if metric == "colored":
            g.set_color_weight(1000.0)
            g.set_error_metric(engine.ErrorMetric.COLORED, 0.05)
        else:
            if metric == "plane_to_plane":
                g.set_plane_to_plane(0.001)
            else:
                g.set_symmetric(True)
            g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        g.set_rejection(True, None)
        if on:
            g.set_boundary_rejection(side); g.set_normal_rejection(MIN_COS)
        return g

    g = handle(True)
    assert g.launches_per_iteration() == 1 + 2 + ADDED_PLANE
    R0 = one_step(engine, g, F, M, T)
    zero, counts, W0, _ = numpy_rule(engine, g, F, M, R0, True, invalid, side, MIN_COS)
    assert np.array_equal(g.read(Mem.PAIR_FILTER), counts) and counts[1] > 0 and counts[2] > 0 and counts[3] > 0
    assert_bits(g.read(Mem.W), np.where(zero, np.float32(0), W0).astype(np.float32), "weights")
    on = [g.read(Mem.PLANE_SYSTEM).copy(), g.read(Mem.T).copy()]
    Mz = M.copy()
    Mz[zero] = 0.0
    h = handle(False)
    h.set_normals(0, 0) if metric != "colored" else None                 # Normals.GIVEN: the same normals as the run with the rules on
    h.write(Mem.F, F); h.write(Mem.M, Mz)
    h.buildRBC()
    if metric != "colored":
        h.write(Mem.NORMALS_F, g.read(Mem.NORMALS_F)); h.write(Mem.NORMALS_M, g.read(Mem.NORMALS_M))
    h.write(Mem.T, T, block=True)
    h.step()
    assert np.array_equal(h.read(Mem.W) == 0, zero), "the same pairs weigh nothing"
    assert np.array_equal(h.read(Mem.NN_ID)["id"][~zero], g.read(Mem.NN_ID)["id"][~zero])
    assert_bits(h.read(Mem.PLANE_SYSTEM), on[0], "PLANE_SYSTEM")
    assert_bits(h.read(Mem.T), on[1], "T")
    g.close(); h.close()


# ---- 6. multi-iteration: run, run_fixed, twice on one handle, icp_batch, tracking

def _snapshot(engine, g):
    Mem = engine.Memory
    return [g.read(Mem.T).copy(), g.read(Mem.W).copy(), g.read(Mem.PAIR_FILTER).copy(), g.read(Mem.NN_ID)["id"].copy()]


def _same(a, b):
    for x, y, what in zip(a, b, ("T", "W", "PAIR_FILTER", "ids")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


@pytest.mark.parametrize("fused,weighted", [(True, WEIGHTED), (False, REGULAR)])
def test_run_equals_steps(engine, scenes_A, fused, weighted):
    """A checked run and run_fixed against the same iterations as single steps — where counts not cleared between iterations would
    show —, and the same registration twice on one handle."""
    F, M, _, invalid, _ = scenes_A["holes"]
    g = make_handle(engine, 128, 256, fused, weighted, POWER, fused, invalid, True, 0.5)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()
    assert 1 < k <= 40, k
    run = _snapshot(engine, g)
    assert run[2][0] == run[2][1:].sum() and run[2][1] > 0 and run[2][2] > 0 and run[2][3] > 0
    assert np.count_nonzero(run[1]) == run[2][3], "the lazily read weights show the rules' zeros"
    g.reset_transform(); g.buildRBC()
    for _ in range(k):
        g.step()
    _same(run, _snapshot(engine, g))
    g.reset_transform(); g.buildRBC()
    assert g.run() == k
    _same(run, _snapshot(engine, g))                    # twice on one handle
    n = 5
    out = []
    for _ in range(2):                                   # run_fixed twice on one handle
        g.reset_transform(); g.buildRBC()
        g.run_fixed(n)
        out.append(_snapshot(engine, g))
    _same(out[0], out[1])
    g.reset_transform(); g.buildRBC()
    for _ in range(n):
        g.step()
    _same(out[0], _snapshot(engine, g))
    g.close()


def test_a_min_cos_update_takes_effect_in_a_captured_graph(engine, scenes_A):
    """run_fixed (3) captures a graph; a new min_cos while the rule stays on is a device word that graph reads: the same form and
    launch count, no new build, and the counts and the transform of single steps taken under the new threshold."""
    F, M, _, invalid, _ = scenes_A["holes"]
    g = make_handle(engine, 128, 256, True, WEIGHTED, POWER, True, invalid, True, MIN_COS)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run_fixed(3)
    first = _snapshot(engine, g)
    stats = (g.run_form(), g.launches_per_iteration())
    g.set_normal_rejection(0.0)
    assert (g.run_form(), g.launches_per_iteration()) == stats
    g.reset_transform(); g.buildRBC()
    g.run_fixed(3)
    second = _snapshot(engine, g)
    assert second[2][2] < first[2][2] and second[2][3] > first[2][3], (first[2], second[2])
    g.reset_transform(); g.buildRBC()
    for _ in range(3):
        g.step()
    _same(second, _snapshot(engine, g))
    g.profile_run(2)                                     # (the pass times with the search stage)
    g.close()


def test_icp_batch_equals_single_handles(engine):
    from icp_amd import workloads as W
    side, nr, n = 128, 256, 3
    m = side * side
    pairs = [_holes(engine, side, W.BASE_SEED + 11 * i) for i in range(n)]
    bt = engine.ICPBatch([0])
    bt.init(n, m, nr, A, C_)
    bt.set_rejection(True, None)
    assert bt.boundary_rejection() is None and bt.normal_rejection() is None
    bt.set_normals(1, side)
    bt.set_boundary_rejection(side); bt.set_normal_rejection(0.5)
    assert bt.boundary_rejection() == side and bt.normal_rejection() == 0.5
    for i, (F, M) in enumerate(pairs):
        bt.write(i, engine.Memory.F, F); bt.write(i, engine.Memory.M, M)
    bt.buildRBC()
    bt.run()
    for i, (F, M) in enumerate(pairs):
        g = make_handle(engine, side, nr, True, WEIGHTED, POWER, True, True, True, 0.5)
        g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
        g.buildRBC()
        k = g.run()
        assert bt.state(i).k == k, i
        assert_bits(bt.read(i, engine.Memory.T), g.read(engine.Memory.T), "T of registration %d" % i)
        u = bt.read(i, engine.Memory.PAIR_FILTER)
        assert np.array_equal(u, g.read(engine.Memory.PAIR_FILTER)) and u[1] > 0 and u[2] > 0 and u[3] > 0, i
        g.close()
    bt.close()


def test_tracking_with_the_boundary_rule_equals_run_on_the_landmarks(engine, oracle):
    frames = [engine.punch_holes(engine.synth_cloud_vga(moved=f), 640, 480, engine.HOLES_CONTIGUOUS, 0.2, True, seed=77 + f)
              for f in range(4)]
    lms = [oracle.get_lms(c) for c in frames]
    g, h = (make_handle(engine, 128, 256, True, WEIGHTED, POWER, True, True, True, None) for _ in range(2))
    assert g.track_next(frames[0]) is None
    for i in range(1, 4):
        k = g.track_next(frames[i])
        h.write(engine.Memory.F, lms[i - 1]); h.write(engine.Memory.M, lms[i])
        h.reset_transform(); h.buildRBC()
        assert k == h.run(), i
        assert_bits(g.read(engine.Memory.T), h.read(engine.Memory.T), "T of hop %d" % i)
        assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], h.read(engine.Memory.NN_ID)["id"]), i
        u = g.read(engine.Memory.PAIR_FILTER)
        assert np.array_equal(u, h.read(engine.Memory.PAIR_FILTER)) and u[1] > 0 and u[3] > 0 and u[2] == 0, i
    g.close(); h.close()


def test_tracking_with_the_normal_rule_is_refused(engine):
    g = engine.ICP(0)
    g.init(16384, 256, A, C_)
    g.set_normals(1, 128)
    g.set_normal_rejection(0.5)
    with pytest.raises(engine.ICPError) as e:
        g.track_next(engine.synth_cloud_vga(moved=0))
    assert e.value.code == 4 and "icp_set_normal_rejection" in str(e.value)
    g.close()


# ---- 7. the form and the launch counts

def test_form_and_launch_count(engine):
    """With a rule on the iteration is the separate form; the launches added are the header's: the pass and the apply pass on
    point-to-point, the pass on point-to-plane; both rules together are still one pass."""
    for side in (128, 256):
        g = engine.ICP(0)
        g.init(side * side, 256, A, C_)
        g.setReduceMode(engine.ReduceMode.FUSED)
        form0, tail = g.run_form(), (3 if (side * side // 64 + 127) // 128 > 2 else 2)
        g.set_boundary_rejection(side)
        assert g.run_form() == 0
        assert g.launches_per_iteration() == tail + ADDED_P2P
        g.set_normal_rejection(0.5)
        assert g.launches_per_iteration() == tail + ADDED_P2P
        g.set_boundary_rejection(None)
        assert g.run_form() == 0 and g.launches_per_iteration() == tail + ADDED_P2P
        g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
        assert g.launches_per_iteration() == 4 + ADDED_P2P
        g.setReduceMode(engine.ReduceMode.FUSED)
        g.set_normals(1, side)
        g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.05)
        plane_on = g.launches_per_iteration()
        g.set_normal_rejection(None)
        assert plane_on == g.launches_per_iteration() + ADDED_PLANE == 1 + 2 + ADDED_PLANE
        g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT, 0.0)
        assert g.run_form() == form0
        g.close()


# ---- 8. what it is for: partial overlap, measured

def _partial_overlap_run(engine, fused, boundary, angle):
    from icp_amd import workloads as W
    from icp_amd.register import normal_cosine
    F, M, T_true = _partial_overlap(engine)
    g = engine.ICP(0)
    g.init(F.shape[0], 256, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    if boundary:
        g.set_boundary_rejection(128)
    if angle is not None:
        g.set_normals(1, 128)
        g.set_normal_rejection(normal_cosine(angle))
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    k = g.run()
    T = g.read(engine.Memory.T).copy()
    counts = g.read(engine.Memory.PAIR_FILTER).tolist()
    g.close()
    return k, W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7])), counts


@pytest.mark.parametrize("fused", [True, False])
def test_the_rules_cope_with_partial_overlap(engine, fused):
    """tests/test_gpu_trimming.py's partial-overlap scene (1 degree, (8, -4, 5) mm, a quarter of M pushed 150 mm off): the run with
    boundary rejection and the normal rule (45 degrees) against the same run without; rotation / translation error against T_true.
    Measured on an MI355X (both reduce modes alike): without the rules 0.431 deg / 8.27 mm in 30 iterations; with them 0.242 deg /
    2.96 mm in 31 (the last iteration rejects 1237 pairs at the boundary and 1222 by their normals, of 16384).  Each bound is halfway
    between the two measured values.  (For the record: the boundary rule alone 0.334 deg / 5.38 mm, the normal rule alone at 60 degrees
    0.366 deg / 6.09 mm; both with 30 degrees 0.199 deg / 2.63 mm, with 60 degrees 0.287 deg / 3.91 mm.)"""
    ROT_BOUND, TRANS_BOUND = (0.431 + 0.242) / 2, (8.27 + 2.96) / 2
    res = {"off": _partial_overlap_run(engine, fused, False, None), "on": _partial_overlap_run(engine, fused, True, 45.0)}
    for name in ("off", "on"):
        print("partial overlap %s, rules %s: k = %d, %.3f deg %.2f mm, last PAIR_FILTER %s" % ("fused" if fused else "reference order", name, *res[name]))
    assert 1 < res["on"][0] <= 40, res
    assert res["on"][1] < ROT_BOUND < res["off"][1], res
    assert res["on"][2] < TRANS_BOUND < res["off"][2], res


# ---- 9. every option at once survives icp_init

def _set_every_option(engine, g, moving):
    """Every setting a setter stores, at a value that is not its default and that a float holds exactly."""
    g.setPowerMode(engine.PowerMode.LITERAL); g.setReduceMode(engine.ReduceMode.REFERENCE_ORDER)
    g.setMetricScale(2.0)
    g.set_normals(engine.Normals.GRID, 16)
    g.set_error_metric(engine.ErrorMetric.POINT_TO_PLANE, 0.0625)
    g.set_color_weight(250.0)
    g.set_robust_loss(engine.RobustLoss.HUBER, 32.0)
    g.set_rejection(True, 512.0)
    g.set_trimming(0.75)
    g.set_unique(True)
    g.set_boundary_rejection(16)
    g.set_normal_rejection(0.25)
    if moving == "plane_to_plane":
        g.set_plane_to_plane(0.125)
    else:
        g.set_symmetric(True)


def _every_getter(g):
    return (g.getMetricScale(), g.normals(), g.error_metric(), g.color_weight(), g.robust_loss(), g.rejection(), g.trimming(), g.unique(),
            g.boundary_rejection(), g.normal_rejection(), g.plane_to_plane(), g.symmetric())


_RESULT_WORDS = ("TRIM", "UNIQUE", "PAIR_FILTER", "PLANE_SYSTEM")


def _run_and_read(engine, g, F, M):
    """T and the per-registration result words after a run of three iterations from the identity."""
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.run_fixed(3)
    out = {"T": g.read(engine.Memory.T).copy()}
    for name in _RESULT_WORDS:
        out[name] = g.read(getattr(engine.Memory, name)).copy()
    return out


def _switch_off_and_expect_zeros(engine, g):
    g.set_trimming(1.0); g.set_unique(False); g.set_normal_rejection(None); g.set_boundary_rejection(None)
    g.set_error_metric(engine.ErrorMetric.POINT_TO_POINT)
    for name in _RESULT_WORDS:
        assert np.all(g.read(getattr(engine.Memory, name)).view(np.uint32) == 0), "%s reads zeros while its feature is off" % name


@pytest.mark.parametrize("moving", ["plane_to_plane", "symmetric"])
def test_every_option_survives_icp_init(engine, moving):
    """The union of the per-feature "survives icp_init" cases.  A handle gets every option BEFORE its first icp_init and is then
    initialised three times in a row — m = 256, |R| = 16; m = 1024, |R| = 64; m = 256 again — with no setter called in between.  After
    each icp_init every getter returns what was set, and a run of three iterations gives the bits of T, ICP_MEM_TRIM, ICP_MEM_UNIQUE,
    ICP_MEM_PAIR_FILTER and ICP_MEM_PLANE_SYSTEM of a fresh handle that got the same options AFTER its icp_init.  Switching the features
    off must leave their result areas reading zeros: checked on each shape's fresh handle, and on the handle under test once its
    third icp_init has been checked (switching them off earlier would leave the later calls of icp_init nothing to keep).
    (The grid width 16 is the landmark grid's at m = 256; at m = 1024 it divides m and reads the 32 x 32 grid as 64 rows of 16: the normals
    and the rim are then not the surface's, which the comparison does not need.)"""
    want = (2.0, (engine.Normals.GRID, 16), (engine.ErrorMetric.POINT_TO_PLANE, 0.0625), 250.0, (engine.RobustLoss.HUBER, 32.0),
            (True, 512.0), 0.75, True, 16, 0.25, 0.125 if moving == "plane_to_plane" else 0.0, moving == "symmetric")
    g = engine.ICP(0)
    _set_every_option(engine, g, moving)
    assert _every_getter(g) == want
    for side, nr in ((16, 16), (32, 64), (16, 16)):
        F, M = engine.synth_pair(side)
        g.init(side * side, nr, A, C_)
        assert _every_getter(g) == want, (side, _every_getter(g))
        got = _run_and_read(engine, g, F, M)
        fresh = engine.ICP(0)
        fresh.init(side * side, nr, A, C_)
        _set_every_option(engine, fresh, moving)
        ref = _run_and_read(engine, fresh, F, M)
        print("m = %d:" % (side * side), {k: v.tolist() for k, v in ref.items() if k != "PLANE_SYSTEM"}, "system status", ref["PLANE_SYSTEM"][27])
        assert ref["PAIR_FILTER"][0] > 0 and ref["UNIQUE"][0] > 0 and ref["TRIM"][1] > 0, "the rules had candidates to work on"
        for name in ("T",) + _RESULT_WORDS:
            assert_bits(got[name], ref[name], "%s at m = %d against a handle set up after icp_init" % (name, side * side))
        _switch_off_and_expect_zeros(engine, fresh)
        fresh.close()
    _switch_off_and_expect_zeros(engine, g)
    g.close()
