"""The search over the whole range of alpha, in every layout: icp_init and icp_set_alpha refuse 0, NaN and +-inf only, so a negative, a
tiny, a denormal and a huge alpha go straight into k_search — the bodies it takes without pruning (`a > 0` is the switch), distances
below zero, distances that tie to the last bit, distances of +inf.  Every other search test of the suite runs at alpha = 200.

What is compared: the RBC structure (the owner search is the same kernel with the same alpha) and, per teacher-forced search, the
nearest representatives, the ids and the distances' bits against the oracle's serial scan — and nothing behind the search: what the tail
of an iteration makes of a negative distance (100 / (100 + d) at d = -100) is not the subject, so the handles weigh REGULAR.  Three
transforms per case: the identity, icp_checks._t0 () and the T the oracle reaches after three steps at alpha = 200.

search_alpha_cases.py has the alphas, the scenes and the layouts (shapes and layout tuples as in test_gpu_parity.py);
tests/test_search_alpha_cpu.py proves on the CPU that the alphas do on these scenes what their names say.  Not here: the 1024-tile with
lanes = candidates needs 2^20 points (|R| = 8192 with lists of 128); it shares ks_stage2_wave with the 256-tile shapes that are here.

The other routes that launch the search — icp_evaluate and icp_correspondences (EVALUATED), the back search of reciprocal
correspondences — and projective association, which states its winner by the same order, run once each at the negative and at the huge
alpha."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks as K                  # noqa: E402
import pairs_ref                        # noqa: E402
import projective_ref                   # noqa: E402
import quality_ref                      # noqa: E402
import reciprocal_ref                   # noqa: E402
import search_alpha_cases as cases      # noqa: E402
from icp_checks import assert_bits      # noqa: E402

pytestmark = pytest.mark.gpu

ROUTE_ALPHAS = ("neg_winners", "huge")


def _check_rbc(engine, g, want, b):
    Mem = engine.Memory
    assert_bits(g.read(Mem.REPS, batch_index=b), want.reps, "representatives of registration %d" % b)
    for mem, arr in (("RBC_OWNER", want.owner), ("RBC_N", want.N), ("RBC_O", want.O), ("RBC_PERM", want.perm)):
        got = g.read(getattr(Mem, mem), batch_index=b)
        assert np.array_equal(got, arr), "%s of registration %d: %d differ" % (mem, b, np.count_nonzero(got != arr))


def _check_search(engine, g, want, b, what):
    Mem = engine.Memory
    nn_id, rid = want
    grid = g.read(Mem.RID, batch_index=b)
    assert np.array_equal(grid, rid), "%s: nearest representatives, %d differ (first at %d)" % (
        what, np.count_nonzero(grid != rid), np.flatnonzero(grid != rid)[0])
    gn = g.read(Mem.NN_ID, batch_index=b)
    bad = np.flatnonzero(gn["id"] != nn_id["id"])
    assert bad.size == 0, "%s: ids, %d differ, first at %d: got %r want %r" % (what, bad.size, bad[0], gn[bad[0]], nn_id[bad[0]])
    assert_bits(gn["dist"], nn_id["dist"], what + ": distances")


@pytest.mark.parametrize("name", list(cases.ALPHAS))
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_search_at_alpha(engine, oracle, monkeypatch, case, name):
    Mem = engine.Memory
    if case.env is None:
        monkeypatch.delenv("ICP_AMD_S2WAVE", raising=False)
    else:
        monkeypatch.setenv("ICP_AMD_S2WAVE", case.env)               # (read by icp_init: forces stage 2 with lanes = candidates)
    monkeypatch.delenv("ICP_AMD_CHAIN", raising=False)
    side, nr, batch = case.scenes[0].side, case.scenes[0].nr, len(case.scenes)
    alpha = cases.alpha_of(name, side)
    g = engine.ICP(0, K.POWER, K.REGULAR)
    g.init(side * side, nr, alpha, K.C_, batch=batch)
    K.set_modes(engine, g, power_fast=case.fused, fused=case.fused)
    assert g.search_layout() == case.layout and g.run_form() == case.chained, (g.search_layout(), g.run_form())
    assert g.getAlpha() == alpha
    for b, scene in enumerate(case.scenes):
        F, M = cases.frames(scene, name)
        g.write(Mem.F, F, batch_index=b); g.write(Mem.M, M, batch_index=b)
    g.buildRBC()
    for b, scene in enumerate(case.scenes):
        _check_rbc(engine, g, cases.searched(scene, name), b)
    # the chained form is what run_fixed launches (one search kernel with the finalize in its prologue); step () launches the separate
    # search of the same layout: both where the handle chains
    forms = (("run_fixed", lambda: g.run_fixed(1)), ("step", g.step)) if case.chained else (("step", g.step),)
    for k in range(3):
        for form, launch in forms:
            for b, scene in enumerate(case.scenes):
                g.write(Mem.T, cases.transforms(scene)[k], batch_index=b, block=True)
            launch()
            for b, scene in enumerate(case.scenes):
                _check_search(engine, g, cases.searched(scene, name).steps[k], b, "%s, transform %d, registration %d" % (form, k, b))
    g.close()


# ---- the other routes that launch the search ---------------------------------------------------------------------------------------

EVAL_SCENE = cases.Scene(128, 64, "synth", 0, 0.1)                    # with batch 3: the dense 256-tile, lanes = candidates
BATCH_SCENES = tuple(cases.Scene(128, 64, "synth", b, 0.1) for b in range(3))


def _batch_handle(engine, name, weighted=K.REGULAR):
    g = engine.ICP(0, K.POWER, weighted)
    g.init(128 * 128, 64, cases.alpha_of(name, 128), K.C_, batch=3)
    K.set_modes(engine, g, power_fast=True, fused=True)
    assert g.search_layout() == cases.WAVE_256
    for b, scene in enumerate(BATCH_SCENES):
        F, M = cases.frames(scene, name)
        g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
    g.buildRBC()
    for b, scene in enumerate(BATCH_SCENES):
        g.write(engine.Memory.T, cases.transforms(scene)[1], batch_index=b, block=True)
    return g


@pytest.mark.parametrize("name", ROUTE_ALPHAS)
def test_evaluate_and_evaluated_pairs(engine, oracle, name):
    """icp_evaluate and icp_correspondences (EVALUATED) run the search of the handle's layout with the handle's alpha: against
    quality_ref / pairs_ref fed the oracle's search at that alpha, at _t0 (), registration by registration."""
    g = _batch_handle(engine, name)
    for b, scene in enumerate(BATCH_SCENES):
        F, M = cases.frames(scene, name)
        T = cases.transforms(scene)[1]
        nn_id, _ = cases.searched(scene, name).steps[1]
        max_dist = K.pick_max_dist(oracle, F, M, T, scene.nr, frac=0.3, nn_id=nn_id)
        PF = np.ascontiguousarray(F[nn_id["id"]][:, :4])
        PM = np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])
        want = quality_ref.evaluate(M, PF, PM, max_dist)
        assert 0.1 <= want.n_inliers / want.n_moving <= 0.9, (want.n_inliers, want.n_moving)
        quality_ref.check_record(g.evaluate(max_dist)[b], want, F.shape[0], "%s, registration %d" % (name, b))
        pairs_ref.check_set(g.correspondences(engine.Pairs.EVALUATED, max_dist, batch_index=b),
                            pairs_ref.evaluated(M, PF, PM, nn_id["id"], max_dist), "%s, registration %d" % (name, b))
    g.close()


@pytest.mark.parametrize("name", ROUTE_ALPHAS)
def test_reciprocal_back_search(engine, oracle, name):
    """The back search of reciprocal correspondences (F's points into M's own RBC at the inverse transform): ICP_MEM_REVERSE_ID against
    the oracle's search with the frames swapped, at the handle's alpha."""
    g = _batch_handle(engine, name)
    g.set_reciprocal(True, 20.0)
    g.buildRBC()
    for b, scene in enumerate(BATCH_SCENES):
        g.write(engine.Memory.T, cases.transforms(scene)[1], batch_index=b, block=True)
    g.step()
    for b, scene in enumerate(BATCH_SCENES):
        F, M = cases.frames(scene, name)
        Ti, ok = reciprocal_ref.inverse(cases.transforms(scene)[1])
        assert ok
        back, _ = K.oracle_search(oracle, M, F, Ti, scene.nr, cases.alpha_of(name, scene.side))
        got = g.read(engine.Memory.REVERSE_ID, batch_index=b)
        bad = np.flatnonzero(got["id"] != back["id"])
        assert bad.size == 0, "registration %d: back search ids, %d differ, first at %d: got %r want %r" % (b, bad.size, bad[0], got[bad[0]], back[bad[0]])
        assert_bits(got["dist"], back["dist"], "back search distances of registration %d" % b)
        _check_search(engine, g, cases.searched(scene, name).steps[1], b, "forward search, registration %d" % b)
    g.close()


PROJ_SCENE = cases.Scene(64, 64, "synth", 0, 0.1)


def _projective_argmin(oracle, F, M, T, gw, intr, r, alpha):
    """nn_id of the projection's rule with the winner by FLOAT comparison: the smallest d, a NaN or +inf never wins, a tie to the
    smallest j (projective_ref has the pixel and the inside test; its winner is not used)."""
    m, rows = M.shape[0], M.shape[0] // gw
    E = oracle.transform_q(M, T)
    ins, pu, pv = projective_ref.inside_mask(M, E, intr, gw)
    fvalid = projective_ref.valid_rows(F)
    nn_id = np.zeros(m, projective_ref.DIST_ID)
    nn_id["dist"], nn_id["id"] = np.inf, projective_ref.NONE
    q = np.zeros(8, np.float32)
    for i in np.flatnonzero(ins):
        x, y = int(pu[i]), int(pv[i])
        q[:3], q[4:7] = E[i, :3], M[i, 4:7]
        best, bj = np.float32(np.inf), None
        for yy in range(max(0, y - r), min(rows - 1, y + r) + 1):
            for xx in range(max(0, x - r), min(gw - 1, x + r) + 1):
                j = yy * gw + xx
                if fvalid[j]:
                    d = np.float32(oracle.metric8(q, F[j], alpha))
                    if d < best:                                 # (j ascends: the first of equal distances stays)
                        best, bj = d, j
        if bj is not None:
            nn_id[i] = (best, bj)
    return nn_id


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("name", ROUTE_ALPHAS)
def test_projective_winner_by_float_order(engine, oracle, name, r):
    scene = PROJ_SCENE
    F, M = cases.frames(scene, name)
    T, alpha, intr = cases.transforms(scene)[1], cases.alpha_of(name, scene.side), engine.grid_intrinsics(scene.side)
    want = _projective_argmin(oracle, F, M, T, scene.side, intr, r, alpha)
    hit = want["id"] != projective_ref.NONE
    if name == "neg_winners":
        assert np.count_nonzero(hit) > F.shape[0] // 2
        assert 4 * np.count_nonzero(want["dist"][hit] < 0) >= np.count_nonzero(hit), "a quarter of the winners are negative"
    else:                                                            # (huge: a window of 9 or 25 cells seldom holds a colour near enough)
        assert 20 <= np.count_nonzero(hit) < F.shape[0] // 2
    g = K.projective_handle(engine, F.shape[0], scene.nr, True, K.REGULAR, K.POWER, True, scene.side, intr, r)
    g.setAlpha(alpha)
    K.load(engine, g, F, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    g.step()
    gn = g.read(engine.Memory.NN_ID)
    bad = np.flatnonzero(gn["id"] != want["id"])
    assert bad.size == 0, "ids: %d differ, first at %d: got %r want %r" % (bad.size, bad[0], gn[bad[0]], want[bad[0]])
    assert_bits(gn["dist"], want["dist"], "distances")
    g.close()
