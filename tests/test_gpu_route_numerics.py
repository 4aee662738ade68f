"""Every combination of the per-iteration passes, numerically: the pair filter, one-to-one, trimming and the robust loss behind the
search, in front of each tail (reference order, fused with and without k_moment_level1, the plane system).

The order is icp_route_of's (icp_amd/csrc/icp_kernels.hip): a pair the filter rejects claims no fixed point, trimming's candidates are the
winners, the apply pass comes last, the plane metrics read the weights — and carry the loss — in their moments.  icp_checks.composed_rule
states it in numpy from the single rules; every comparison here is bit for bit.  Mask bits as in test_route_table: bit 0 the pair filter
(the boundary rule at the grid width and the normal rule with GRID normals), bit 1 one-to-one, bit 2 trimming, bit 3 the robust loss.
Rejection by invalid points and a maximum distance is on throughout.

The scenes, the options (max_dist, min_cos, keep, the scales) and why they are what they are: icp_checks.ROUTE_SCENES / route_scene.
tests/test_route_rule_cpu.py proves from the oracle alone that under them every stage of every mask removes at least 2 % of its
candidates and keeps at least half; a first step's result words are compared with the counts of that proof, so the conditions hold
on the device too.  A second step starts at the first's own T, which no proof covers (the frames lie closer, the normal rule at the
same min_cos finds less to reject): there every pass must still remove some pair and keep half.

Shapes (test_route_table's): (30, 4), m = 900 — the last block of 64 / 128 / 256 pairs partly filled, the selection in one block —;
(150, 4), m = 22500 — a side that is no multiple of 8, the three-pass selection, 352 blocks and so a k_moment_level1 tail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                  # noqa: E402
import robust_ref as rref                                        # noqa: E402
from icp_checks import (ROUTE_BATCH, ROUTE_METRICS, ROUTE_WORDS, assert_bits, before, check_route_plane_step, check_route_step,  # noqa: E402
                        oracle_search, route_handle, route_proof, route_restate, route_scene, route_scene_options)

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


def _steps(engine, oracle, names, mask, metric, fused=None, loss=rref.CAUCHY, steps=2):
    """`steps` steps of one handle over the scenes `names`, every registration of every step checked.  The first step starts at the
    scene's T (its words are the CPU proof's), each later one at the step's own T."""
    Mem = engine.Memory
    scenes = [route_scene(n) for n in names]
    s0 = scenes[0]
    os_ = [route_scene_options(s, mask, loss) for s in scenes]
    assert all(o == os_[0] for o in os_), "a handle has one set of options"
    g = route_handle(engine, s0.side, s0.nr, os_[0], metric, fused, batch=len(scenes))
    if len(scenes) > 1 and fused is not False:
        assert g.search_layout()[0] == 1, g.search_layout()       # (the dense layout by batch)
    R0 = _load(engine, g, scenes)
    for it in range(steps):
        state = [before(engine, g, b) for b in range(len(scenes))]
        g.step()
        for b, (s, o, name) in enumerate(zip(scenes, os_, names)):
            T0, Rb, k0 = state[b]
            want = s.want if it == 0 else oracle_search(oracle, s.F, s.M, T0, s.nr)
            proof = route_proof(name, mask, loss)[0] if it == 0 else None
            what = "%s, scene %s, mask %d, loss %d, step %d" % (metric, name, mask, loss, it)
            if metric == "p2p":
                check_route_step(engine, oracle, g, s.F, s.M, s.NF, s.NM, T0, Rb, want, o, fused, b, proof, what)
            else:
                check_route_plane_step(engine, g, s.F, s.M, s.NF, s.NM, T0, Rb, k0, want, o, route_restate(metric, o, s.M), b, proof, what)
    g.close()


# ---- 1. the grid: every mask at both shapes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("name", GRID)
def test_point_to_point(engine, oracle, name, fused, mask):
    _steps(engine, oracle, [name], mask, "p2p", fused)


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("metric", ROUTE_METRICS)
@pytest.mark.parametrize("name", GRID)
def test_plane_family(engine, oracle, name, metric, mask):
    _steps(engine, oracle, [name], mask, metric)


# ---- 2. every pass on, beyond the grid ------------------------------------------------------------------------------------------------

CASES = [("p2p", True), ("p2p", False)] + [(metric, None) for metric in ROUTE_METRICS]


@pytest.mark.parametrize("loss", [rref.HUBER, rref.TUKEY])
@pytest.mark.parametrize("metric,fused", CASES)
def test_every_pass_with_the_other_losses(engine, oracle, metric, fused, loss):
    _steps(engine, oracle, ["30"], 15, metric, fused, loss)


@pytest.mark.parametrize("metric,fused", CASES[:3])
def test_every_pass_in_a_batch_of_three(engine, oracle, metric, fused):
    """Three different scenes at (128, 64) in one handle, the dense layout by batch: each registration by its index."""
    _steps(engine, oracle, list(ROUTE_BATCH), 15, metric, fused)


@pytest.mark.parametrize("metric,fused", CASES)
def test_every_pass_at_config_A(engine, oracle, metric, fused):
    _steps(engine, oracle, ["A"], 15, metric, fused)


# ---- 3. several iterations --------------------------------------------------------------------------------------------------------------

RUNS = [("p2p", True), ("p2p", False), ("p2pl", None)]
ANGLE, TRANSLATION, MAX_IT = 0.001, 0.01, 40                     # (icp_init's defaults, which route_handle leaves)


def _snapshot(engine, g):
    Mem = engine.Memory
    return [g.read(Mem.T).copy(), g.read(Mem.W).copy()] + [g.read(getattr(Mem, name)).copy() for name in ROUTE_WORDS]


def _same(a, b, what):
    for x, y, name in zip(a, b, ("T", "W") + tuple(ROUTE_WORDS)):
        assert_bits(x, y, "%s: %s" % (what, name))


def _loaded(engine, mask, metric, fused):
    s = route_scene("30")
    g = route_handle(engine, s.side, s.nr, route_scene_options(s, mask), metric, fused)
    g.write(engine.Memory.F, s.F); g.write(engine.Memory.M, s.M)
    g.buildRBC()
    return g, s


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_fixed_equals_steps(engine, metric, fused, mask):
    g, _ = _loaded(engine, mask, metric, fused)
    g.run_fixed(4)
    fixed = _snapshot(engine, g)
    assert fixed[2][3] > 0 and fixed[3][1] > 0 and fixed[4][3] > 0, fixed[2:]
    g.reset_transform(); g.buildRBC()
    for _ in range(4):
        g.step()
    _same(fixed, _snapshot(engine, g), "run_fixed (4) against four steps")
    g.close()


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_run_equals_stepping_until_done(engine, metric, fused, mask):
    """Done is the header's: the step's Tk under both thresholds (p2pl_ref.check_converged) or max_iterations steps taken."""
    g, _ = _loaded(engine, mask, metric, fused)
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


@pytest.mark.parametrize("mask", [7, 15])
@pytest.mark.parametrize("metric,fused", RUNS)
def test_every_pass_off_again_equals_never_on(engine, metric, fused, mask):
    g, s = _loaded(engine, mask, metric, fused)
    h = route_handle(engine, s.side, s.nr, route_scene_options(s, 0), metric, fused)
    h.write(engine.Memory.F, s.F); h.write(engine.Memory.M, s.M)
    stats = (h.run_form(), h.launches_per_iteration())
    g.run(); g.run_fixed(3)
    assert g.read(engine.Memory.TRIM)[3] > 0
    g.set_robust_loss(rref.NONE); g.set_trimming(1.0); g.set_unique(False)
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
