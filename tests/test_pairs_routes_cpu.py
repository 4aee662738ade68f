"""The conditions tests/test_gpu_route_numerics.py and tests/test_gpu_pairs_layouts.py rely on for the correspondence sets, proven from
the oracle alone (no device): an expected set that held nearly every pair, or nearly none, would let a wrong predicate or a wrong
position pass.

1. Member shares: for every (scene, mask, loss, metric family) the route tests run a first step with, the expected
   ICP_PAIRS_LAST_ITERATION set holds between 20 % and 90 % of the m pairs, and its size is the word of the last acting stage
   (icp_checks.last_stage_count) — the header's statement about the count, from composed_rule alone.  SHARES records the sizes.
2. The Tukey condition: with the loss alone (mask 8) the point-to-point set is smaller than the plane set by at least 5 % of it; with
   every pass on (mask 15) the two are equal — trimming has removed what Tukey would zero —, which is why the device test uses mask 8.
   Both hold again with the reciprocal rule on (masks 24 and 31).
3. The layout scenes (icp_checks.LAYOUT_CASES): the LAST_ITERATION expectation at _t0 () and the EVALUATED expectation at the oracle's T
   after that step each hold between 10 % and 90 % of the points icp_evaluate counts.  LAYOUT_SHARES records them.

pairs_ref.last_iteration on hand-made arrays (a NaN weight is a member, -0 and +0 are none, `moving` ascends) is
tests/test_pairs_cpu.py::test_weights_nan_is_a_member_and_both_zeros_are_none and is not repeated here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref                                                  # noqa: E402
import pairs_ref                                                 # noqa: E402
import quality_ref                                               # noqa: E402
import robust_ref as rref                                        # noqa: E402
from icp_checks import (LAYOUT_CASES, POWER, ROUTE_BATCH, evaluated_expectation, expected_pieces, last_stage_count, layout_scene,  # noqa: E402
                        pick_max_dist, route_proof, route_scene, route_scene_options, ROUTE_SCENES)

# scene -> the size of the expected set per mask 0 .. 31 (Cauchy), (point-to-point, a plane metric); they differ only where the
# point-to-point loss zeroes a weight, which Cauchy and Huber never do.  Masks 16 .. 31: the reciprocal rule on as well.
SHARES = {"30": [(706, 706), (500, 500), (505, 505), (396, 396), (530, 530), (375, 375), (379, 379), (297, 297)] * 2
                + [(494, 494), (360, 360), (449, 449), (337, 337), (371, 371), (270, 270), (337, 337), (253, 253)] * 2,
          "150": [(17642, 17642), (14199, 14199), (10821, 10821), (10158, 10158), (13232, 13232), (10650, 10650), (8116, 8116),
                  (7619, 7619)] * 2                              # (78.4 % of m at mask 0 down to 33.0 % and 33.9 % with every stage on)
                 + [(12349, 12349), (10519, 10519), (9065, 9065), (8309, 8309), (9262, 9262), (7890, 7890), (6799, 6799),
                    (6232, 6232)] * 2}                           # (54.9 % of m at mask 16 down to 28.1 % and 27.7 % at mask 31)
# (scene, loss) -> the sizes beyond the grid: every pass on but the reciprocal rule (mask 15), and every pass on (mask 31)
BEYOND = {("30", rref.HUBER): (297, 297), ("30", rref.TUKEY): (297, 297), ("A", rref.CAUCHY): (5298, 5298),
          ("batch0", rref.CAUCHY): (5406, 5406), ("batch1", rref.CAUCHY): (4647, 4647), ("batch2", rref.CAUCHY): (5937, 5937)}
BEYOND_31 = {("30", rref.HUBER): (253, 253), ("30", rref.TUKEY): (253, 253), ("A", rref.CAUCHY): (4337, 4337),
             ("batch0", rref.CAUCHY): (4430, 4430), ("batch1", rref.CAUCHY): (3702, 3702), ("batch2", rref.CAUCHY): (5057, 5057)}
# scene -> mask 8 with Tukey: (point-to-point, a plane metric); mask 24, the reciprocal rule in front of it
TUKEY = {"30": (635, 706), "150": (15877, 17642)}
TUKEY_24 = {"30": (449, 494), "150": (11473, 12349)}


def _sizes(name, mask, loss):
    """(size of the point-to-point set, size of a plane metric's) of the first step's expectation, each proven to be the last acting
    stage's word and the number of records pairs_ref.last_iteration makes of the weights."""
    s = route_scene(name)
    o = route_scene_options(s, mask, loss)
    out = []
    for plane in (False, True):
        r, _ = route_proof(name, mask, loss, plane)
        W = r.W_before_loss if plane else r.W
        want = pairs_ref.last_iteration(s.want[0], W, s.PF[:, :4], s.PM[:, :4])
        stage, n = last_stage_count(r, o, plane)
        assert len(want) == n == np.count_nonzero(W), (name, mask, loss, plane, stage, len(want), n)
        assert (np.diff(want["moving"].astype(np.int64)) > 0).all() and np.isfinite(want["geo"]).all()
        out.append(len(want))
    return tuple(out)


def _in_range(n, m, what):
    assert 0.2 * m <= n <= 0.9 * m, "%s: the expected set holds %d of %d pairs" % (what, n, m)


@pytest.mark.parametrize("mask", range(32))
@pytest.mark.parametrize("name", ["30", "150"])
def test_member_shares_of_the_grid(engine, oracle, name, mask):
    m = route_scene(name).M.shape[0]
    got = _sizes(name, mask, rref.CAUCHY)
    print(name, mask, got, [round(100.0 * n / m, 1) for n in got])
    for n in got:
        _in_range(n, m, "scene %s, mask %d" % (name, mask))
    assert got == SHARES[name][mask], (got, SHARES[name][mask])


@pytest.mark.parametrize("name,loss", list(BEYOND))
def test_member_shares_beyond_the_grid(engine, oracle, name, loss):
    m = route_scene(name).M.shape[0]
    got = _sizes(name, 15, loss)
    for n in got:
        _in_range(n, m, "scene %s, mask 15, loss %d" % (name, loss))
    assert got == BEYOND[(name, loss)], (got, BEYOND[(name, loss)])


@pytest.mark.parametrize("name,loss", list(BEYOND_31))
def test_member_shares_beyond_the_grid_with_the_reciprocal_rule(engine, oracle, name, loss):
    """Mask 31: what tests/test_gpu_route_numerics.py runs beyond the grid."""
    m = route_scene(name).M.shape[0]
    got = _sizes(name, 31, loss)
    for n in got:
        _in_range(n, m, "scene %s, mask 31, loss %d" % (name, loss))
    assert got == BEYOND_31[(name, loss)], (got, BEYOND_31[(name, loss)])


def test_the_smallest_set_of_the_new_masks(engine, oracle):
    """Every scene, mask 16 .. 31, loss and family: the smallest expected set is 22.6 % of m (batch1 with the filter, the rule, one-to-one
    and trimming on, whatever the loss and the family): inside the band of _in_range, like every other."""
    sizes = {}
    for name in ROUTE_SCENES:
        m = route_scene(name).M.shape[0]
        for mask in range(16, 32):
            for loss in ((rref.HUBER, rref.CAUCHY, rref.TUKEY) if mask & 8 else (rref.CAUCHY,)):
                for plane, n in enumerate(_sizes(name, mask, loss)):
                    _in_range(n, m, "scene %s, mask %d, loss %d" % (name, mask, loss))
                    sizes[name, mask, loss, plane] = n / m
    low = min(sizes, key=sizes.get)
    assert low[0] == "batch1" and low[1] & 23 == 23 and round(1000 * sizes[low]) == 226, (low, sizes[low])
    assert sizes["batch1", 31, rref.TUKEY, 1] == sizes[low], "(no loss changes the size there: the sets of masks 23 and 31 tie)"


def test_the_batch_has_three_different_sets(engine, oracle):
    assert len({BEYOND[(n, rref.CAUCHY)] for n in ROUTE_BATCH}) == 3
    assert len({BEYOND_31[(n, rref.CAUCHY)] for n in ROUTE_BATCH}) == 3
    accepted = [int(route_proof(n, 31)[0].words["RECIPROCAL"][3]) for n in ROUTE_BATCH]
    assert accepted == [7488, 6478, 8545], accepted


@pytest.mark.parametrize("name", list(TUKEY))
def test_the_tukey_condition(engine, oracle, name):
    m = route_scene(name).M.shape[0]
    p2p, plane = _sizes(name, 8, rref.TUKEY)
    _in_range(p2p, m, "Tukey alone, point-to-point"); _in_range(plane, m, "Tukey alone, a plane metric")
    assert (p2p, plane) == TUKEY[name], (p2p, plane)
    assert plane - p2p >= 0.05 * plane, "Tukey alone zeroes %d of %d weights" % (plane - p2p, plane)
    s = route_scene(name)
    r8, rp = route_proof(name, 8, rref.TUKEY, False)[0], route_proof(name, 8, rref.TUKEY, True)[0]
    assert not (rp.W_before_loss[r8.W != 0] == 0).any(), "the point-to-point set is a subset of the plane set"
    both = _sizes(name, 15, rref.TUKEY)
    assert both[0] == both[1], "every pass on: trimming has removed what Tukey would zero (%r)" % (both,)
    # the same two statements with the reciprocal rule in front (masks 24 and 31): re-established, not corrected — the rule removes
    # pairs of every residual, Tukey still zeroes more than 5 % of what it leaves, and trimming still removes all of those
    p2p, plane = _sizes(name, 24, rref.TUKEY)
    _in_range(p2p, m, "the rule and Tukey, point-to-point"); _in_range(plane, m, "the rule and Tukey, a plane metric")
    assert (p2p, plane) == TUKEY_24[name], (p2p, plane)
    assert plane - p2p >= 0.05 * plane, "behind the rule Tukey zeroes %d of %d weights" % (plane - p2p, plane)
    both = _sizes(name, 31, rref.TUKEY)
    assert both[0] == both[1], "every pass on, the rule included: trimming has removed what Tukey would zero (%r)" % (both,)
    assert s.scale[rref.TUKEY] > 0


# ---- 3. the layout scenes -------------------------------------------------------------------------------------------------------------

# (side, |R|, batch, fused, zero) -> per registration (counted points, LAST_ITERATION members at _t0 (), counted points and EVALUATED
# members at the T after the step)
LAYOUT_SHARES = {
    (256, 256, 1, True, 0.0): [(65536, 43254, 65536, 45875)],
    (256, 512, 1, True, 0.1): [(59006, 38944, 59006, 41304)],
    (256, 512, 1, False, 0.1): [(59006, 38944, 59006, 41304)],
    (128, 64, 3, True, 0.0): [(16384, 10814, 16384, 11469), (16384, 10002, 16384, 10540), (16384, 9317, 16384, 9818)],
    (64, 64, 9, True, 0.0): [(4096, 2703, 4096, 2867), (4096, 2500, 4096, 2627), (4096, 2349, 4096, 2453), (4096, 2202, 4096, 2275),
                             (4096, 2070, 4096, 2141), (4096, 1953, 4096, 2032), (4096, 1864, 4096, 1945), (4096, 1780, 4096, 1846),
                             (4096, 1698, 4096, 1790)],
    (256, 8192, 1, True, 0.0): [(65536, 43254, 65536, 45875)],
    (192, 2048, 1, True, "blobs30"): [(25369, 16743, 25369, 17758)]}


def layout_after(oracle, case):
    """Per registration of a LAYOUT_CASES row the oracle's T after one step from _t0 (): Tk from the oracle's pieces fed the rule's
    weights (expected_pieces), composed as icp_compose does (p2pl_ref.compose)."""
    side, nr, batch, fused, zero, _ = case
    sc = layout_scene(side, nr, batch, zero)
    R0 = oracle.quat_to_rot(sc.T[:4]).ravel()
    out = []
    for (F, M), want, r in zip(sc.pairs, sc.wants, sc.rules):
        Tk = expected_pieces(oracle, F, M, sc.T, want[0], side, fused, True, POWER, fused, r.W == 0)[4]
        out.append(p2pl_ref.compose(sc.T, R0, Tk)[0])
    return out


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: "%d-%d-%d-%d-%s" % c[:5])
def test_layout_scenes_have_members_and_non_members(engine, oracle, case):
    side, nr, batch, fused, zero, _ = case
    sc = layout_scene(side, nr, batch, zero)
    Ts = layout_after(oracle, case)
    F0, M0 = sc.pairs[0]
    max_dist = pick_max_dist(oracle, F0, M0, Ts[0], nr, frac=0.3)
    rows = []
    for (F, M), want, pf, pm, r, T in zip(sc.pairs, sc.wants, sc.PF, sc.PM, sc.rules, Ts):
        counted = int(np.count_nonzero(quality_ref.masks(M, pf, pm, 0.0)[0]))
        last = pairs_ref.last_iteration(want[0], r.W, pf[:, :4], pm[:, :4])
        assert len(last) == int(r.words["TRIM"][3]) == last_stage_count(r, sc.options, False)[1]
        ev, q = evaluated_expectation(oracle, F, M, T, nr, max_dist)
        assert len(ev) == q.n_inliers
        rows.append((counted, len(last), q.n_moving, len(ev)))
        assert 0.1 * counted <= len(last) <= 0.9 * counted, "LAST_ITERATION holds %d of %d counted points" % (len(last), counted)
        assert 0.1 * q.n_moving <= len(ev) <= 0.9 * q.n_moving, "EVALUATED holds %d of %d counted points" % (len(ev), q.n_moving)
    print(case[:5], rows)
    if batch > 1:
        assert len({r[1] for r in rows}) == batch and len({r[3] for r in rows}) == batch, "the counts of a batch are pairwise distinct: %r" % (rows,)
    assert rows == LAYOUT_SHARES[case[:5]], rows


# ---- the projection at the head of the route (tests/test_gpu_route_numerics.py section 2b) ------------------------------------------------

# scene -> the size of the expected set per mask 0 .. 15 (Cauchy), (point-to-point, a plane metric)
PROJ_SHARES = {"p30": [(640, 640), (471, 471), (467, 467), (377, 377), (480, 480), (354, 354), (351, 351), (283, 283)] * 2,
               "p150": [(15136, 15136), (12700, 12700), (11960, 11960), (10717, 10717), (11352, 11352), (9525, 9525), (8970, 8970),
                        (8038, 8038)] * 2}
PROJ_BEYOND = {("p30", rref.HUBER): (283, 283), ("p30", rref.TUKEY): (283, 283), ("p150", rref.CAUCHY): (8038, 8038),
               ("p150b1", rref.CAUCHY): (7281, 7281), ("p150b2", rref.CAUCHY): (8934, 8934)}


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("name", list(PROJ_SHARES))
def test_member_shares_behind_the_projection(engine, oracle, name, mask):
    """The expectation is projective_ref.project's pairs under composed_rule: the set holds between 20 % and 90 % of the m pairs."""
    m = route_scene(name).M.shape[0]
    got = _sizes(name, mask, rref.CAUCHY)
    print(name, mask, got, [round(100.0 * n / m, 1) for n in got])
    for n in got:
        _in_range(n, m, "scene %s, mask %d" % (name, mask))
    assert got == PROJ_SHARES[name][mask], (got, PROJ_SHARES[name][mask])


@pytest.mark.parametrize("name,loss", list(PROJ_BEYOND))
def test_member_shares_behind_the_projection_beyond_the_grid(engine, oracle, name, loss):
    m = route_scene(name).M.shape[0]
    got = _sizes(name, 15, loss)
    for n in got:
        _in_range(n, m, "scene %s, mask 15, loss %d" % (name, loss))
    assert got == PROJ_BEYOND[(name, loss)], (got, PROJ_BEYOND[(name, loss)])
