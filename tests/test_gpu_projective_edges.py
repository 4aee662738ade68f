"""Projective data association (icp_set_projective, icp_projective.hip) at the kernel's own edges: the four-round launch above
batch m = 65536 — rounds partly and wholly past m, one block that draws the only ticket, the running words left at zero —; pixels that
sit exactly on a rounding boundary and pairs of adjacent floats on either side of one; e.z at zero, denormal and behind the camera;
exact ties and candidates that can never win; a metric scale and an alpha other than the defaults, with icp_set_rejection's distance
test between the scaled and the unscaled distance.

The reference of every comparison is tests/projective_ref.py::project (float64 pixels, the oracle's transform and metric) and the
oracle's pieces fed its pairs, bit for bit, through icp_checks.check_projective_step.  tests/test_projective_cpu.py proves from the oracle
alone that every scene holds the case it is here for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks                                               # noqa: E402
import projective_ref as ref                                    # noqa: E402
from icp_checks import IDENTITY, POWER, WEIGHTED, _t0, one_step, step_batch    # noqa: E402
from icp_checks import check_projective_step as check_step, projective_handle as make_handle    # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---- A1. four rounds per block

@functools.lru_cache(maxsize=None)
def _pieces(key, r, fused):
    """ref.pieces of scene (*key) — key = (side, zero_fraction[, seed]) — at ref.at (.., r), computed once for the registrations that
    share the pair."""
    from oracle import oracle
    F, M, T = ref.scene(*key)
    return ref.pieces(oracle, ref.at(key[0], key[1], r, *key[2:]), F, M, T, key[0], fused, WEIGHTED, POWER, fused)


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr,batch", ref.FOUR_ROUNDS)
def test_four_rounds(engine, oracle, side, nr, batch, fused, r):
    """One step of every shape of ref.FOUR_ROUNDS, every registration checked by its index; then T written again and a second step:
    the same words and outputs, so the running words and the ticket were left at zero."""
    T = _t0()
    keys = [(side, 0.1)] if batch == 1 else [(side, zf, seed) for seed, zf in ref.BATCH]
    pairs = [ref.scene(*keys[b % len(keys)])[:2] for b in range(batch)]
    g = make_handle(engine, side * side, nr, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), r, batch=batch)
    step_batch(engine, g, pairs, T)
    for again in (False, True):
        if again:
            for b in range(batch):
                g.write(engine.Memory.T, T, batch_index=b, block=True)
            g.step()
        seen = set()
        for b, (F, M) in enumerate(pairs):
            key = keys[b % len(keys)]
            got = check_step(engine, oracle, g, ref.at(key[0], key[1], r, *key[2:]), F, M, T, side, fused, WEIGHTED, POWER, fused, b=b,
                             pieces=_pieces(key, r, fused))
            seen.add(tuple(got.tolist()))
        assert len(seen) == len(keys), seen
        if batch == 1:
            assert seen == {ref.EXACT[side, 0.1, r]}
    g.close()


# ---- A2. pixels on and next to a rounding boundary

def _named(engine, oracle, scene, side, intr, fused, r):
    """One step of a constructed scene whose rows name their pixel: check_step against the restatement, and the inside / outside
    pattern and — at r = 0, on a clean F whose cell j holds the back-projection of its own centre — the cell itself, by name."""
    F, M, T, pu, pv = scene
    res = ref.project(oracle, F, M, T, side, intr, r, True)
    g = make_handle(engine, side * side, 4, fused, WEIGHTED, POWER, fused, side, intr, r)
    one_step(engine, g, F, M, T)
    gn = g.read(engine.Memory.NN_ID)
    inside = ref.named_inside(pu, pv, side, side)
    bad = np.flatnonzero((gn["id"] != ref.NONE) != inside)
    assert bad.size == 0, "rows inside / outside against their names: %r (pu, pv named %r)" % (bad, [(pu[i], pv[i]) for i in bad])
    if r == 0:
        cell = (pv * side + pu)[inside].astype(np.uint32)
        bad = np.flatnonzero(gn["id"][inside] != cell)
        assert bad.size == 0, "cells against their names: rows %r got %r want %r" % (np.flatnonzero(inside)[bad], gn["id"][inside][bad], cell[bad])
    got = check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused)
    assert got.tolist() == [side * side, np.count_nonzero(inside), np.count_nonzero(~inside), 0]
    g.close()


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("fused", [True, False])
def test_pixels_exactly_on_a_boundary(engine, oracle, fused, r):
    """u + 0.5 == k exactly (ref.exact_scene): floor gives k; pixel 0 is inside at k = 0, k = 8 is outside, the float below k = 0 is
    outside.  A float pixel, rint, or an inexact division moves rows."""
    _named(engine, oracle, ref.exact_scene(), ref.EXACT_SIDE, ref.EXACT_INTRINSICS, fused, r)


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("fused", [True, False])
def test_adjacent_floats_straddle_every_boundary(engine, oracle, fused, r):
    """Two adjacent float32 coordinates on either side of every boundary k = 0 .. 30, in x and in y, within 1.2e-6 of a pixel of it
    (ref.straddle_scene): a pixel computed in float moves 51 of the 124 rows."""
    _named(engine, oracle, ref.straddle_scene(), ref.STRADDLE_SIDE, ref.straddle_intrinsics(), fused, r)


# ---- A3. e.z

@pytest.mark.parametrize("collapsed", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_edge_cases_of_ez(engine, oracle, fused, collapsed):
    """ref.ez_scene: e.z = +-0, a denormal e.z, a point behind the camera, denormal coordinates that count, a pixel beyond float; and
    the same set under a transform with s = 0, which sends every point to one cell."""
    side = ref.EZ_SIDE
    F, M = ref.ez_scene()
    T = ref.collapsed_T() if collapsed else IDENTITY
    intr = engine.grid_intrinsics(side)
    res = ref.project(oracle, F, M, T, side, intr, 0, True)
    g = make_handle(engine, side * side, 4, fused, WEIGHTED, POWER, fused, side, intr, 0)
    one_step(engine, g, F, M, T)
    got = check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused)
    assert got.tolist() == ([36, 36, 0, 0] if collapsed else [36, 30, 6, 0])
    if not collapsed:
        ids = g.read(engine.Memory.NN_ID)["id"]
        row = ref.EZ_ROWS
        out = [row[k] for k in ("z -0", "z +0", "z denormal", "behind", "only a denormal", "u beyond float")]
        assert (ids[out] == ref.NONE).all() and ids[row["denormal on the axis"]] == 3 * side + 3 and ids[row["denormal x"]] != ref.NONE
    g.close()


# ---- A4. ties and candidates that never win

@pytest.mark.parametrize("r", ref.TIES_RADII)
@pytest.mark.parametrize("fused", [True, False])
def test_ties_and_candidates_that_never_win(engine, oracle, fused, r):
    """ref.ties_scene: bitwise duplicate records at distance 0 in one window — the smaller j wins, in the same row and where it has the
    larger column —; candidates at +inf or NaN, and queries all of whose candidates are: inside, valid candidates, no winner: "empty"."""
    side = ref.TIES_SIDE
    F, M, T, rows = ref.ties_scene()
    intr = engine.grid_intrinsics(side)
    res = ref.project(oracle, F, M, T, side, intr, r, True)
    g = make_handle(engine, side * side, 16, fused, WEIGHTED, POWER, fused, side, intr, r)
    one_step(engine, g, F, M, T)
    gn = g.read(engine.Memory.NN_ID)
    x, y = int(res.pu[rows["same row"]]), int(res.pv[rows["same row"]])
    assert tuple(gn[rows["same row"]]) == (0.0, y * side + x - 1)
    x, y = int(res.pu[rows["lower row"]]), int(res.pv[rows["lower row"]])
    assert tuple(gn[rows["lower row"]]) == (0.0, y * side + x + 1)
    empty = ["huge", "nan query"] + (["overflow", "nan colour"] if r == 1 else [])
    assert all(gn[rows[name]]["id"] == ref.NONE for name in empty), [(name, gn[rows[name]]) for name in empty]
    got = check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused)
    assert got[3] >= len(empty) and got[1] > 150
    g.close()


# ---- A5. the metric's scale and alpha

@pytest.mark.parametrize("rejection", [False, True])
@pytest.mark.parametrize("alpha", ref.ALPHAS)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,zf,seed", ref.METRIC_SCENES)
def test_scale_and_alpha(engine, oracle, side, zf, seed, fused, alpha, rejection):
    """setMetricScale (0.37) and setAlpha: d and the weight take the scaled distance; icp_set_rejection's distance test takes the
    geometric one — max_dist lies between the two, so the other reading rejects other pairs (at least 2 % of the hits differ)."""
    F, M, T = ref.scene(side, zf, seed)
    res = ref.at_metric(side, zf, seed, alpha)
    max_dist = ref.metric_max_dist(res)
    options = dict(rejection=(False, max_dist)) if rejection else {}
    g = make_handle(engine, side * side, 4, fused, WEIGHTED, POWER, fused, side, engine.grid_intrinsics(side), 1, **options)
    g.setAlpha(alpha)
    g.setMetricScale(ref.METRIC_SCALE)
    one_step(engine, g, F, M, T)
    zero = ref.metric_rejected(res, max_dist) if rejection else None
    check_step(engine, oracle, g, res, F, M, T, side, fused, WEIGHTED, POWER, fused, zero=zero)
    if rejection:
        assert np.count_nonzero(g.read(engine.Memory.W)) == res.counts[1] - np.count_nonzero(zero) < res.counts[1]
    g.close()
