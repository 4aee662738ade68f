"""Every combination of the per-iteration passes, numerically: the pair filter, reciprocal correspondences, one-to-one, trimming and the
robust loss behind the search, in front of each tail (reference order, fused with and without k_moment_level1, the plane system).

The order is icp_route_of's (icp_amd/csrc/icp_kernels.hip): the reciprocal rule's candidates are the pairs the filter leaves, a pair
either of them rejects claims no fixed point, trimming's candidates are the
winners, the apply pass comes last, the plane metrics read the weights — and carry the loss — in their moments.  icp_checks.composed_rule
states it in numpy from the single rules; every comparison here is bit for bit.  Mask bits as in test_route_table: bit 0 the pair filter
(the boundary rule at the grid width and the normal rule with GRID normals), bit 1 one-to-one, bit 2 trimming, bit 3 the robust loss;
bit 4 the reciprocal rule at the scene's max_gap.  Rejection by invalid points and a maximum distance is on throughout.  With bit 4 on
every step also compares ICP_MEM_REVERSE_ID — every fixed point's id and the bits of its distance — with the oracle's back search at the
step's T (reciprocal_ref.back_search) and ICP_MEM_RECIPROCAL with the rule's words.

The scenes, the options (max_dist, min_cos, keep, the scales) and why they are what they are: icp_checks.ROUTE_SCENES / route_scene.
tests/test_route_rule_cpu.py proves from the oracle alone that under them every stage of every mask removes at least 2 % of its
candidates and keeps at least half; a first step's result words are compared with the counts of that proof, so the conditions hold
on the device too.  A second step starts at the first's own T, which no proof covers (the frames lie closer, the normal rule at the
same min_cos finds less to reject): there every pass must still remove some pair and keep half.

Behind every step the ICP_PAIRS_LAST_ITERATION set of every registration is compared with the set composed_rule's weights give on the
oracle's pairs (icp_checks.check_route_pairs: nothing of the expectation is read from the handle); with every pass on, beyond the grid,
also ICP_PAIRS_EVALUATED and icp_evaluate at the T the step left, which the handle's options must not influence.
tests/test_pairs_routes_cpu.py proves from the oracle alone that every expected set holds between 20 % and 90 % of the pairs.

Section 2b runs the grid once more with the projection (icp_set_projective) at the head of the route instead of the RBC search.

Shapes (test_route_table's): (30, 4), m = 900 — the last block of 64 / 128 / 256 pairs partly filled, the selection in one block —;
(150, 4), m = 22500 — a side that is no multiple of 8, the three-pass selection, 352 blocks and so a k_moment_level1 tail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                  # noqa: E402
import pairs_ref                                                 # noqa: E402
import quality_ref                                               # noqa: E402
import robust_ref as rref                                        # noqa: E402
from icp_checks import (PROJ_ROUTE_BATCH, ROUTE_BATCH, ROUTE_METRICS, ROUTE_WORDS, assert_bits, back_at, before, check_route_pairs,  # noqa: E402
                        check_route_plane_step, check_route_step, evaluated_expectation, oracle_search, route_handle, route_pairs_of, route_proof,
                        route_restate, route_scene, route_scene_options, route_want)

pytestmark = pytest.mark.gpu

GRID = ["30", "150"]
MODES = [True, False]                                            # fused + the squared power start; reference order + the literal one


def _load(engine, g, scenes):
    """Load the scenes (one per registration), build, start every registration at the scene's T.  Returns R as the first search uses it."""
    Mem = engine.Memory
    for b, s in enumerate(scenes):
        g.write(Mem.F, s.F, batch_index=b); g.write(Mem.M, s.M, batch_index=b)
    g.buildRBC()
    R0 = []
    for b, s in enumerate(scenes):
        g.write(Mem.T, s.T, batch_index=b, block=True)
        R0.append(g.read(Mem.R, batch_index=b).ravel().copy())
        assert_bits(R0[b], s.R0, "R at the start against the oracle's")
    return R0


def _check_evaluated(engine, oracle, g, scenes, Ts, wants, what):
    """ICP_PAIRS_EVALUATED and icp_evaluate at the transforms Ts the step left, max_dist the scenes' own: every registration's set and
    record bit for bit against the oracle's search there (wants), whatever passes and metric the handle has on."""
    max_dist = scenes[0].max_dist
    recs = g.evaluate(max_dist)
    for b, (s, T, want) in enumerate(zip(scenes, Ts, wants)):
        m = s.M.shape[0]
        e, q = evaluated_expectation(oracle, s.F, s.M, T, s.nr, max_dist, want)
        assert 0 < q.n_inliers < q.n_moving < m, (what, q.n_inliers, q.n_moving)
        got = g.correspondences(engine.Pairs.EVALUATED, max_dist, batch_index=b)
        pairs_ref.check_set(got, e, "the EVALUATED set (%s, registration %d)" % (what, b))
        quality_ref.check_record(recs[b], q, m, "%s, registration %d" % (what, b))
        assert len(got) == recs[b].n_inliers, (what, b, len(got), recs[b].n_inliers)


def _steps(engine, oracle, names, mask, metric, fused=None, loss=rref.CAUCHY, steps=2, evaluated=False):
    """`steps` steps of one handle over the scenes `names`, every registration of every step checked: the step itself, then the
    ICP_PAIRS_LAST_ITERATION set against the oracle's pairs (check_route_pairs).  The first step starts at the scene's T (its words are
    the CPU proof's), each later one at the step's own T.  evaluated: behind every step also the evaluation at the T it left
    (_check_evaluated) — the oracle's search there is the next step's expectation as well.  With the reciprocal rule on (mask bit 4)
    the oracle's back search at the step's T stands beside the forward one: the scene's own at the first step, back_at's at a later
    one.  Returns the last step's sets."""
    Mem = engine.Memory
    scenes = [route_scene(n) for n in names]
    s0 = scenes[0]
    os_ = [route_scene_options(s, mask, loss) for s in scenes]
    assert all(o == os_[0] for o in os_), "a handle has one set of options"
    assert all(s.projective == s0.projective for s in scenes), "a handle has one way to find its pairs"
    assert not (evaluated and s0.projective), "the evaluation is the RBC search's: its expectation is no projective one"
    g = route_handle(engine, s0.side, s0.nr, os_[0], metric, fused, batch=len(scenes), projective=s0.projective)
    if len(scenes) > 1 and fused is not False and s0.projective is None:
        assert g.search_layout()[0] == 1, g.search_layout()       # (the dense layout by batch)
    _load(engine, g, scenes)
    wants = [s.want for s in scenes]
    for it in range(steps):
        state = [before(engine, g, b) for b in range(len(scenes))]
        g.step()
        sets = []
        for b, (s, o, name) in enumerate(zip(scenes, os_, names)):
            T0, Rb, k0 = state[b]
            want = wants[b]
            proof = route_proof(name, mask, loss)[0] if it == 0 else None
            back = None if not mask & 16 else s.back if it == 0 else back_at(name, s.F, s.M, T0, s.nr)
            what = "%s, scene %s, mask %d, loss %d, step %d" % (metric, name, mask, loss, it)
            if metric == "p2p":
                r = check_route_step(engine, oracle, g, s.F, s.M, s.NF, s.NM, T0, Rb, want, o, fused, b, proof, what, back)
            else:
                r = check_route_plane_step(engine, g, s.F, s.M, s.NF, s.NM, T0, Rb, k0, want, o, route_restate(metric, o, s.M), b, proof, what, back)
            PF, PM = (s.PF, s.PM) if it == 0 else route_pairs_of(oracle, s, want, T0)
            if it == 0:                                           # (the first step's weights from the reference's pairs too: the CPU proof's)
                r = route_proof(name, mask, loss, metric != "p2p")[0]
            sets.append(check_route_pairs(engine, g, want[0], PF, PM, r, metric != "p2p", o, b, what))
        if evaluated or it + 1 < steps:
            Ts = [g.read(Mem.T, b).copy() for b in range(len(scenes))]
            wants = [route_want(oracle, s, T) for s, T in zip(scenes, Ts)]
        if evaluated:
            _check_evaluated(engine, oracle, g, scenes, Ts, wants, "%s, mask %d, loss %d, behind step %d" % (metric, mask, loss, it))
    g.close()
    return sets


# ---- 1. the grid: every mask at both shapes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", range(32))
@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("name", GRID)
def test_point_to_point(engine, oracle, name, fused, mask):
    _steps(engine, oracle, [name], mask, "p2p", fused)


@pytest.mark.parametrize("mask", range(32))
@pytest.mark.parametrize("metric", ROUTE_METRICS)
@pytest.mark.parametrize("name", GRID)
def test_plane_family(engine, oracle, name, metric, mask):
    _steps(engine, oracle, [name], mask, metric)


# ---- 2. every pass on, beyond the grid ------------------------------------------------------------------------------------------------

CASES = [("p2p", True), ("p2p", False)] + [(metric, None) for metric in ROUTE_METRICS]


@pytest.mark.parametrize("loss", [rref.HUBER, rref.TUKEY])
@pytest.mark.parametrize("metric,fused", CASES)
def test_every_pass_with_the_other_losses(engine, oracle, metric, fused, loss):
    _steps(engine, oracle, ["30"], 31, metric, fused, loss, evaluated=True)


def test_tukey_zeroes_show_in_the_point_to_point_set_only(engine, oracle):
    """Tukey's loss alone (mask 8) zeroes the pairs beyond its scale.  On point-to-point it acts on W, so those pairs leave the
    LAST_ITERATION set; a plane metric carries the loss in its moments and keeps the search's weight, so they stay.  One step of a
    point-to-plane handle and of a point-to-point one in either mode, each set against its expectation (_steps); the point-to-point
    set is a strict subset of the plane one by `moving`.  (Under mask 15 trimming has already removed what Tukey would zero, and the
    two sets are equal: tests/test_pairs_routes_cpu.py proves both statements from the oracle alone.)"""
    plane = _steps(engine, oracle, ["30"], 8, "p2pl", None, rref.TUKEY, steps=1)[0]
    for fused in MODES:
        p2p = _steps(engine, oracle, ["30"], 8, "p2p", fused, rref.TUKEY, steps=1)[0]
        assert 0 < len(p2p) < len(plane), (fused, len(p2p), len(plane))
        assert np.isin(p2p["moving"], plane["moving"]).all(), fused


@pytest.mark.parametrize("metric,fused", CASES[:3])
def test_every_pass_in_a_batch_of_three(engine, oracle, metric, fused):
    """Three different scenes at (128, 64) in one handle, the dense layout by batch: each registration by its index."""
    _steps(engine, oracle, list(ROUTE_BATCH), 31, metric, fused, evaluated=True)


@pytest.mark.parametrize("metric,fused", CASES)
def test_every_pass_at_config_A(engine, oracle, metric, fused):
    _steps(engine, oracle, ["A"], 31, metric, fused, evaluated=True)


# ---- 2b. the projection at the head of the route ------------------------------------------------------------------------------------------
#
# icp_set_projective in the RBC search's place (scenes "p30", "p150": the frames of "30" and "150", icp_checks.PROJ_ROUTE_SCENES): the
# expectation of a step is projective_ref.project at the step's T — check_search then compares ICP_MEM_NN_ID, NN, QT and
# ICP_MEM_PROJECTIVE with it —, everything behind it is what it is behind the search.  The reciprocal rule (bit 4) does not combine with
# the projection: masks 0 .. 15.  r = 1 and a max_dist of the projective pairs' own: icp_checks._projective_route_scene.

PGRID = ["p30", "p150"]


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("name", PGRID)
def test_point_to_point_behind_the_projection(engine, oracle, name, fused, mask):
    _steps(engine, oracle, [name], mask, "p2p", fused)


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("metric", ROUTE_METRICS)
@pytest.mark.parametrize("name", PGRID)
def test_plane_family_behind_the_projection(engine, oracle, name, metric, mask):
    _steps(engine, oracle, [name], mask, metric)


@pytest.mark.parametrize("loss", [rref.HUBER, rref.TUKEY])
@pytest.mark.parametrize("metric,fused", CASES)
def test_every_pass_with_the_other_losses_behind_the_projection(engine, oracle, metric, fused, loss):
    _steps(engine, oracle, ["p30"], 15, metric, fused, loss)


@pytest.mark.parametrize("metric,fused", CASES[:3])
def test_every_pass_in_a_batch_of_three_behind_the_projection(engine, oracle, metric, fused):
    """Three different scenes at (150, 4) in one handle: 3 x 22500 points, which the projection serves in four rounds per block."""
    _steps(engine, oracle, list(PROJ_ROUTE_BATCH), 15, metric, fused)


def test_the_reciprocal_rule_does_not_combine_with_the_projection(engine):
    """Both on: every run returns ICP_ESTATE (include/icp_amd.h); the reciprocal rule off again, the handle steps."""
    s = route_scene("p30")
    g = route_handle(engine, s.side, s.nr, route_scene_options(s, 15), "p2p", True, projective=s.projective)
    g.write(engine.Memory.F, s.F); g.write(engine.Memory.M, s.M)
    g.buildRBC()
    g.set_reciprocal(True, route_scene("30").max_gap)
    for call in (g.step, g.run, lambda: g.run_fixed(2)):
        with pytest.raises(engine.ICPError) as e:
            call()
        assert e.value.code == 4
    g.set_reciprocal(False)
    g.step()
    assert g.read(engine.Memory.PROJECTIVE)[1] > 0
    g.close()


# ---- 3. several iterations --------------------------------------------------------------------------------------------------------------

RUNS = [("p2p", True), ("p2p", False), ("p2pl", None)]
ANGLE, TRANSLATION, MAX_IT = 0.001, 0.01, 40                     # (icp_init's defaults, which route_handle leaves)


def _snapshot(engine, g):
    Mem = engine.Memory
    out = ([g.read(Mem.T).copy(), g.read(Mem.W).copy()] + [g.read(getattr(Mem, name)).copy() for name in ROUTE_WORDS]
           + [g.correspondences(engine.Pairs.LAST_ITERATION).view(np.uint32)])
    if g.reciprocal() is not None:
        out.append(g.read(Mem.REVERSE_ID).view(np.uint32).copy())
    return out


def _same(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for x, y, name in zip(a, b, ("T", "W") + tuple(ROUTE_WORDS) + ("the LAST_ITERATION set", "REVERSE_ID")):
        assert_bits(x, y, "%s: %s" % (what, name))


def _loaded(engine, mask, metric, fused, name="30"):
    s = route_scene(name)
    g = route_handle(engine, s.side, s.nr, route_scene_options(s, mask), metric, fused, projective=s.projective)
    g.write(engine.Memory.F, s.F); g.write(engine.Memory.M, s.M)
    g.buildRBC()
    return g, s


@pytest.mark.parametrize("mask", [7, 15, 31])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_fixed_equals_steps(engine, metric, fused, mask):
    _run_fixed_equals_steps(engine, metric, fused, mask)


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_fixed_equals_steps_behind_the_projection(engine, metric, fused, mask):
    _run_fixed_equals_steps(engine, metric, fused, mask, "p30")


def _run_fixed_equals_steps(engine, metric, fused, mask, name="30"):
    g, _ = _loaded(engine, mask, metric, fused, name)
    g.run_fixed(4)
    fixed = _snapshot(engine, g)
    assert fixed[2][3] > 0 and fixed[3][1] > 0 and fixed[4][3] > 0, fixed[2:]
    assert (0 < fixed[5][3] < fixed[5][0] and len(fixed) == 8) if mask & 16 else not fixed[5].any(), fixed[5]
    g.reset_transform(); g.buildRBC()
    for _ in range(4):
        g.step()
    _same(fixed, _snapshot(engine, g), "run_fixed (4) against four steps")
    g.close()


@pytest.mark.parametrize("mask", [7, 15, 31])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_equals_stepping_until_done(engine, metric, fused, mask):
    _run_equals_stepping_until_done(engine, metric, fused, mask)


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_equals_stepping_until_done_behind_the_projection(engine, metric, fused, mask):
    _run_equals_stepping_until_done(engine, metric, fused, mask, "p30")


def _run_equals_stepping_until_done(engine, metric, fused, mask, name="30"):
    """Done is the header's: the step's Tk under both thresholds (p2pl_ref.check_converged) or max_iterations steps taken."""
    g, _ = _loaded(engine, mask, metric, fused, name)
    k = g.run()
    assert 1 < k <= MAX_IT, k
    run = _snapshot(engine, g)
    g.reset_transform(); g.buildRBC()
    steps = 0
    while True:
        g.step()
        steps += 1
        if steps == MAX_IT or p2pl_ref.check_converged(g.read(engine.Memory.TK), ANGLE, TRANSLATION):
            break
    assert steps == k and g.state().k == k, (steps, g.state().k, k)
    _same(run, _snapshot(engine, g), "run () against stepping until done")
    g.close()


@pytest.mark.parametrize("mask", [7, 15, 31])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_every_pass_off_again_equals_never_on(engine, metric, fused, mask):
    _every_pass_off_again_equals_never_on(engine, metric, fused, mask)


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_every_pass_off_again_equals_never_on_behind_the_projection(engine, metric, fused, mask):
    _every_pass_off_again_equals_never_on(engine, metric, fused, mask, "p30")


def _every_pass_off_again_equals_never_on(engine, metric, fused, mask, name="30"):
    g, s = _loaded(engine, mask, metric, fused, name)
    h = route_handle(engine, s.side, s.nr, route_scene_options(s, 0), metric, fused, projective=s.projective)
    h.write(engine.Memory.F, s.F); h.write(engine.Memory.M, s.M)
    stats = (h.run_form(), h.launches_per_iteration())
    g.run(); g.run_fixed(3)
    assert g.read(engine.Memory.TRIM)[3] > 0
    assert (g.read(engine.Memory.RECIPROCAL)[3] > 0) == bool(mask & 16)
    g.set_robust_loss(rref.NONE); g.set_trimming(1.0); g.set_unique(False); g.set_reciprocal(False)
    g.set_normal_rejection(None); g.set_boundary_rejection(None)
    for name in ROUTE_WORDS:
        assert np.all(g.read(getattr(engine.Memory, name)) == 0), name
    if metric == "p2p":
        g.set_normals(0, 0)
    assert (g.run_form(), g.launches_per_iteration()) == stats
    g.reset_transform(); g.buildRBC()
    h.buildRBC()
    assert g.run() == h.run()
    _same(_snapshot(engine, g), _snapshot(engine, h), "off again against never on")
    assert np.array_equal(g.read(engine.Memory.NN_ID)["id"], h.read(engine.Memory.NN_ID)["id"])
    g.close(); h.close()
