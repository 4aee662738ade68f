"""The composed rule of an iteration's passes (icp_checks.composed_rule) without a device: against the single rules and the pair
compositions the feature modules spell out by hand, against a plain per-pair restatement in Python floats, and the proof that under
the chosen options every stage of every mask has pairs to remove and pairs to keep (tests/test_gpu_route_numerics.py relies on it).

The choices, from the oracle's pairs at _t0 () (icp_checks.route_scene): max_dist rejects 12 % of the valid pairs, min_cos 10 % of the
normal rule's candidates, keep = 0.75, Huber 8 mm and Cauchy 12 mm (icp_checks.SCALE), Tukey's scale above 90 % of the surviving
residuals, max_gap accepts 70 % of the reciprocal rule's candidates behind the search's rejection (reciprocal_ref.pick_gap on the
oracle's back search).  CHOSEN, COUNTS and COUNTS_RECIPROCAL record what that gives.

Mask bit 4 is the reciprocal rule (icp_set_reciprocal), between the pair filter and one-to-one: masks 16 to 31 are the sixteen
combinations of the other passes with it on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_filter_ref                                           # noqa: E402
import reciprocal_ref                                            # noqa: E402
import robust_ref as rref                                        # noqa: E402
import unique_ref                                                # noqa: E402
from icp_checks import (LOSSES, ROUTE_KEEP, ROUTE_SCENES, RouteOptions, assert_bits, assert_every_stage_bites, composed_rule,  # noqa: E402
                        route_options, route_proof, route_scene, route_scene_options, stage_shares, trim_rule, weights_before_trim)

F32 = np.float32

# scene -> (max_dist, min_cos, Tukey's scale, max_gap), to three decimals
CHOSEN = {"30": (75.336, 0.485, 65.574, 51.039), "150": (60.682, 0.157, 55.019, 22.874), "A": (61.772, 0.117, 55.713, 25.528),
          "batch0": (60.540, 0.154, 55.096, 24.791), "batch1": (60.540, 0.154, 55.096, 24.791), "batch2": (60.540, 0.154, 55.096, 24.791)}
# scene -> with every pass on: ICP_MEM_PAIR_FILTER (n, at_boundary, incompatible, accepted), ICP_MEM_UNIQUE (n, winners), ICP_MEM_TRIM's
# (n, K, accepted), and the pairs Huber / Cauchy / Tukey re-weigh
COUNTS = {"30": ([706, 147, 59, 500], [500, 396], [396, 297, 297], [297, 297, 297]),
          "150": ([17642, 1766, 1677, 14199], [14199, 10158], [10158, 7619, 7619], [6694, 7619, 7619]),
          "A": ([12670, 1362, 1166, 10142], [10142, 7063], [7063, 5298, 5298], [4658, 5298, 5298]),
          "batch0": ([12709, 1343, 1213, 10153], [10153, 7207], [7207, 5406, 5406], [4782, 5406, 5406]),
          "batch1": ([11527, 916, 1468, 9143], [9143, 6196], [6196, 4647, 4647], [4121, 4647, 4647]),
          "batch2": ([13685, 1492, 1079, 11114], [11114, 7915], [7915, 5937, 5937], [5318, 5937, 5937])}
# scene -> the same with the reciprocal rule on as well (mask 31; ICP_MEM_PAIR_FILTER is COUNTS'): ICP_MEM_RECIPROCAL (n, exact, near,
# accepted), ICP_MEM_UNIQUE, ICP_MEM_TRIM's (n, K, accepted), and the pairs Huber / Cauchy / Tukey re-weigh
COUNTS_RECIPROCAL = {"30": ([500, 320, 40, 360], [360, 337], [337, 253, 253], [253, 253, 253]),
                     "150": ([14199, 4517, 6002, 10519], [10519, 8309], [8309, 6232, 6232], [5307, 6232, 6232]),
                     "A": ([10142, 3342, 4113, 7455], [7455, 5782], [5782, 4337, 4337], [3698, 4337, 4337]),
                     "batch0": ([10153, 3490, 3998, 7488], [7488, 5906], [5906, 4430, 4430], [3806, 4430, 4430]),
                     "batch1": ([9143, 2815, 3663, 6478], [6478, 4935], [4935, 3702, 3702], [3176, 3702, 3702]),
                     "batch2": ([11114, 4085, 4460, 8545], [8545, 6742], [6742, 5057, 5057], [4438, 5057, 5057])}


# ---- 1. every stage bites, from the oracle alone ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ROUTE_SCENES))
def test_the_choices_are_the_recorded_ones(engine, oracle, name):
    s = route_scene(name)
    got = (s.max_dist, s.min_cos, s.scale[rref.TUKEY], s.max_gap)
    assert np.allclose(got, CHOSEN[name], rtol=0, atol=1e-3), (got, CHOSEN[name])
    assert s.scale[rref.HUBER] == 8.0 and s.scale[rref.CAUCHY] == 12.0 and ROUTE_KEEP == 0.75
    assert float(F32(s.max_dist)) == s.max_dist and float(F32(s.min_cos)) == s.min_cos, "the engine's floats hold the options exactly"
    assert float(F32(s.max_gap)) == s.max_gap > 0.0
    changed = []
    for loss in LOSSES:
        r, shares = route_proof(name, 15, loss)
        changed.append(shares["loss"][1])
    t = r.words["TRIM"]
    assert (r.words["PAIR_FILTER"].tolist(), r.words["UNIQUE"].tolist(), [int(t[1]), int(t[2]), int(t[3])], changed) == COUNTS[name]
    assert r.words["RECIPROCAL"] is None
    changed = []
    for loss in LOSSES:
        r, shares = route_proof(name, 31, loss)
        changed.append(shares["loss"][1])
    t = r.words["TRIM"]
    assert r.words["PAIR_FILTER"].tolist() == COUNTS[name][0]
    assert (r.words["RECIPROCAL"].tolist(), r.words["UNIQUE"].tolist(), [int(t[1]), int(t[2]), int(t[3])], changed) == COUNTS_RECIPROCAL[name]
    # the choice itself: exact + near is 70 % of the candidates the rule has with the filter off, to the pair the quantile names
    r16 = route_proof(name, 16)[0].words["RECIPROCAL"]
    assert r16[3] == r16[1] + r16[2] and (name not in ("30", "150", "A", "batch0") or abs(int(r16[3]) - 0.7 * int(r16[0])) <= 1.0), r16


@pytest.mark.parametrize("mask", range(32))
@pytest.mark.parametrize("name", list(ROUTE_SCENES))
def test_every_stage_bites(engine, oracle, name, mask):
    """Search with the oracle at _t0 (), PF = F[ids], PM = the oracle's transformed moving set, the normals of p2pl_ref.grid_normals:
    every stage that is on removes at least 2 % of its own candidates and keeps at least half of them, the loss leaves at least 2 % of
    its candidates with a weight that is neither their input weight nor zero (route_proof asserts it: assert_every_stage_bites)."""
    for loss in (LOSSES if mask & 8 else LOSSES[:1]):
        for plane in (False, True):
            r, shares = route_proof(name, mask, loss, plane)
            want = [n for bit, names in ((1, ("boundary", "normal", "filter")), (2, ("unique",)), (4, ("trim",)), (16, ("reciprocal",)))
                    if mask & bit for n in names]
            assert sorted(shares) == sorted(want + (["loss"] if mask & 8 and not plane else [])), shares
            for n, removed, kept in shares.values():
                assert 50 * removed >= n and 2 * kept >= n
    # each stage's candidates are what the stage in front left (the route's order)
    # (the filter, the reciprocal rule, one-to-one, trimming: include/icp_amd.h)
    w = r.words
    if mask & 17 == 17:
        assert w["RECIPROCAL"][0] == w["PAIR_FILTER"][3]
    if mask & 2:
        front = w["RECIPROCAL"][3] if mask & 16 else w["PAIR_FILTER"][3] if mask & 1 else None
        assert front is None or w["UNIQUE"][0] == front
    if mask & 4:
        front = w["UNIQUE"][1] if mask & 2 else w["RECIPROCAL"][3] if mask & 16 else w["PAIR_FILTER"][3] if mask & 1 else None
        assert front is None or w["TRIM"][1] == front
    if mask & 16:
        assert w["RECIPROCAL"][3] == w["RECIPROCAL"][1] + w["RECIPROCAL"][2] and w["RECIPROCAL"][1] > 0 and w["RECIPROCAL"][2] > 0
        if not mask & 1:
            assert w["RECIPROCAL"][0] == np.count_nonzero(r.W0), "with the filter off the rule's candidates are the pairs the search left a weight"
    for stage, name_ in ((1, "PAIR_FILTER"), (2, "UNIQUE"), (4, "TRIM"), (16, "RECIPROCAL")):
        assert (w[name_] is None) == (not mask & stage), "a stage that is off reports no words"
    assert (r.reciprocal is None) == (not mask & 16)


# ---- 2. against the single rules and the pair compositions ------------------------------------------------------------------------------

def _scene():
    s = route_scene("30")
    return s, s.want[0], s.want[0]["id"], weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, s.max_dist)


def _zeroed(W0, keep):
    return np.where(keep, W0, F32(0)).astype(F32)


def test_one_stage_on_equals_its_own_rule(engine, oracle):
    s, nn_id, ids, W0 = _scene()
    run = lambda mask: composed_rule(nn_id, s.PF, s.PM, s.F, s.M, s.R0, s.NF, s.NM, route_scene_options(s, mask, rref.HUBER), back=s.back)
    r = run(0)
    assert_bits(r.W, W0, "no stage on"); assert r.W is r.W_before_loss and not any(v is not None for v in r.words.values())
    assert r.filter is None and r.unique is None and r.trim is None and r.reciprocal is None
    r = run(16)
    exact, near, zero, counts = reciprocal_ref.reciprocal_rule(ids, s.back[0][0]["id"], s.PM, W0, s.max_gap, s.back[1])
    assert np.array_equal(r.reciprocal[0], exact) and np.array_equal(r.reciprocal[1], near) and np.array_equal(r.reciprocal[2], ~zero & (W0 != 0))
    assert np.array_equal(r.words["RECIPROCAL"], counts) and counts[0] == np.count_nonzero(W0) and 0 < counts[2] and 0 < counts[1]
    assert_bits(r.W, _zeroed(W0, ~zero), "the reciprocal rule alone")
    assert r.filter is None and r.unique is None and r.trim is None and r.W is r.W_before_loss
    r = run(1)
    bnd, inc, acc, counts = pair_filter_ref.pair_filter(ids, W0, s.F, s.side, s.NF, s.NM, s.R0, s.min_cos)
    assert all(np.array_equal(a, b) for a, b in zip(r.filter, (bnd, inc, acc))) and np.array_equal(r.words["PAIR_FILTER"], counts)
    assert_bits(r.W, _zeroed(W0, acc), "the filter alone")
    r = run(2)
    win, cand, counts = unique_ref.unique_rule(ids, s.PF, s.PM, W0)
    assert np.array_equal(r.unique[0], win) and np.array_equal(r.unique[1], cand) and np.array_equal(r.words["UNIQUE"], counts)
    assert_bits(r.W, unique_ref.weights_after(W0, win, cand), "one-to-one alone")
    r = run(4)
    acc, counts = trim_rule(s.PF, s.PM, W0, ROUTE_KEEP)
    assert np.array_equal(r.trim, acc) and np.array_equal(r.words["TRIM"], counts)
    assert_bits(r.W, _zeroed(W0, acc), "trimming alone")
    r = run(8)
    assert_bits(r.W_before_loss, W0, "the loss alone: its input")
    assert_bits(r.W, rref.p2p_weights(W0, s.PF, s.PM, rref.HUBER, 8.0), "the loss alone")
    o = route_scene_options(s, 8, rref.HUBER)
    assert composed_rule(nn_id, s.PF, s.PM, s.F, s.M, s.R0, s.NF, s.NM, o, plane=True).W is not r.W
    assert_bits(composed_rule(nn_id, s.PF, s.PM, s.F, s.M, s.R0, s.NF, s.NM, o, plane=True).W, W0, "a plane metric: the loss is the moments'")


def test_two_stages_on_equal_the_compositions_by_hand(engine, oracle):
    """tests/test_gpu_pair_filter.py's and tests/test_gpu_unique.py's test_with_* constructions."""
    s, nn_id, ids, W0 = _scene()
    run = lambda mask, **k: composed_rule(nn_id, s.PF, s.PM, s.F, s.M, s.R0, s.NF, s.NM, route_scene_options(s, mask, rref.HUBER)._replace(**k),
                                          back=s.back)
    _, _, facc, fcounts = pair_filter_ref.pair_filter(ids, W0, s.F, s.side, s.NF, s.NM, s.R0, s.min_cos)
    W1 = _zeroed(W0, facc)
    r = run(3)                                                   # a rejected pair claims no fixed point
    win, cand, counts = unique_ref.unique_rule(ids, s.PF, s.PM, W1)
    assert np.array_equal(r.words["UNIQUE"], counts) and counts[0] == fcounts[3] and np.array_equal(r.words["PAIR_FILTER"], fcounts)
    assert_bits(r.W, _zeroed(W0, win), "filter + one-to-one")
    r = run(5)                                                   # trimming's candidates are the accepted pairs
    acc, counts = trim_rule(s.PF, s.PM, W1, ROUTE_KEEP)
    assert np.array_equal(r.words["TRIM"], counts) and counts[1] == fcounts[3]
    assert_bits(r.W, _zeroed(W0, acc), "filter + trimming")
    r = run(9)
    assert_bits(r.W, rref.p2p_weights(W1, s.PF, s.PM, rref.HUBER, 8.0), "filter + loss")
    win, cand, ucounts = unique_ref.unique_rule(ids, s.PF, s.PM, W0)
    r = run(6)                                                   # trimming's candidates are the winners
    acc, counts = trim_rule(s.PF, s.PM, _zeroed(W0, win), ROUTE_KEEP)
    assert np.array_equal(r.words["TRIM"], counts) and counts[1] == ucounts[1] and np.array_equal(r.words["UNIQUE"], ucounts)
    assert_bits(r.W, _zeroed(W0, acc), "one-to-one + trimming")
    r = run(10)
    assert_bits(r.W, rref.p2p_weights(_zeroed(W0, win), s.PF, s.PM, rref.HUBER, 8.0), "one-to-one + loss")
    r = run(12)
    acc, _ = trim_rule(s.PF, s.PM, W0, ROUTE_KEEP)
    assert_bits(r.W, rref.p2p_weights(_zeroed(W0, acc), s.PF, s.PM, rref.HUBER, 8.0), "trimming + loss")
    # the reciprocal rule with each neighbour: its candidates are the pairs the filter leaves; a pair it rejects claims no fixed point;
    # trimming's candidates are the pairs it accepts
    rev, ok = s.back[0][0]["id"], s.back[1]
    rule = lambda W, gap=s.max_gap: reciprocal_ref.reciprocal_rule(ids, rev, s.PM, W, gap, ok)
    r = run(17)
    _, _, zero, counts = rule(W1)
    assert np.array_equal(r.words["RECIPROCAL"], counts) and counts[0] == fcounts[3] and np.array_equal(r.words["PAIR_FILTER"], fcounts)
    assert_bits(r.W, _zeroed(W0, ~zero), "filter + the reciprocal rule")
    _, _, zero, rcounts = rule(W0)
    W2 = _zeroed(W0, ~zero)
    r = run(18)
    win, cand, counts = unique_ref.unique_rule(ids, s.PF, s.PM, W2)
    assert np.array_equal(r.words["UNIQUE"], counts) and counts[0] == rcounts[3] and np.array_equal(r.words["RECIPROCAL"], rcounts)
    assert 0 < counts[1] < counts[0], "max_gap > 0: a near pair may share its fixed point with the exact one"
    assert_bits(r.W, _zeroed(W0, win), "the reciprocal rule + one-to-one")
    r = run(20)
    acc, counts = trim_rule(s.PF, s.PM, W2, ROUTE_KEEP)
    assert np.array_equal(r.words["TRIM"], counts) and counts[1] == rcounts[3]
    assert_bits(r.W, _zeroed(W0, acc), "the reciprocal rule + trimming")
    r = run(24)
    assert_bits(r.W, rref.p2p_weights(W2, s.PF, s.PM, rref.HUBER, 8.0), "the reciprocal rule + loss")
    # max_gap = 0: a strictly reciprocal set is one to one already (a fixed point's back search names one query), so one-to-one behind
    # it removes nothing — why the grid's max_gap is not 0
    r = run(18, max_gap=0.0)
    _, _, zero, rcounts = rule(W0, 0.0)
    assert r.words["RECIPROCAL"].tolist() == rcounts.tolist() == [706, 437, 0, 437] and r.words["UNIQUE"].tolist() == [437, 437]
    assert_bits(r.W, _zeroed(W0, ~zero), "the strictly reciprocal set + one-to-one")


# ---- 3. against a plain restatement: one loop over the pairs in Python floats, a sort for the trim --------------------------------------

GW, ROWS = 15, 20
R90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)          # (x, y, z) -> (-y, x, z): exact


def _valid(p):
    return all(math.isfinite(float(v)) for v in p[:3]) and any(float(v) != 0.0 for v in p[:3])


def _at_boundary(F, j):
    x, y = j % GW, j // GW
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            xx, yy = x + dx, y + dy
            if not (0 <= xx < GW and 0 <= yy < ROWS) or not _valid(F[yy * GW + xx]):
                return True
    return False


def _compatible(nq, nm, R, c):
    q = [float(v) for v in nq[:3]] if all(math.isfinite(float(v)) for v in nq[:3]) else [0.0] * 3
    mv = [float(v) for v in nm[:3]] if all(math.isfinite(float(v)) for v in nm[:3]) else [0.0] * 3
    p = [(float(R[a][0]) * mv[0] + float(R[a][1]) * mv[1]) + float(R[a][2]) * mv[2] for a in range(3)]
    qq = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    oo = (q[0] * p[0] + q[1] * p[1]) + q[2] * p[2]
    return qq > 0 and pp > 0 and oo >= float(F32(c)) * math.sqrt(qq * pp)


def plain(ids, PF, PM, F, M, R, NF, NM, o, rev=None):
    """(masks, words) of the route in its prose order, pair by pair."""
    m, mf = len(ids), F.shape[0]
    geo, w = [], []
    for i in range(m):
        d = [float(PM[i][c]) - float(PF[i][c]) for c in range(3)]
        geo.append((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        rejected = o.invalid and (not any(float(v) != 0.0 for v in M[i][:3]) or not any(float(v) != 0.0 for v in PF[i][:3]))
        if o.max_dist:
            rejected = rejected or not geo[i] <= float(F32(o.max_dist)) ** 2
        w.append(not rejected)
    masks, words = {"search": list(w)}, {"PAIR_FILTER": None, "RECIPROCAL": None, "UNIQUE": None, "TRIM": None}
    if o.gw or o.min_cos is not None:
        bnd, inc, acc = [False] * m, [False] * m, [False] * m
        for i in range(m):
            if w[i] and ids[i] < mf:
                bnd[i] = bool(o.gw) and _at_boundary(F, int(ids[i]))
                inc[i] = not bnd[i] and o.min_cos is not None and not _compatible(NF[ids[i]], NM[i], R, o.min_cos)
                acc[i] = not bnd[i] and not inc[i]
        words["PAIR_FILTER"] = [sum(bnd) + sum(inc) + sum(acc), sum(bnd), sum(inc), sum(acc)]
        masks.update(boundary=bnd, incompatible=inc, accepted=acc)
        w = acc
    if o.max_gap is not None:                                     # (rev: the back search's id per fixed point; the gap between transformed moving points)
        exact, near, n = [False] * m, [False] * m, 0
        for i in range(m):
            if w[i] and ids[i] < mf:
                n += 1
                i2 = int(rev[ids[i]])
                exact[i] = i2 == i
                if not exact[i] and float(F32(o.max_gap)) > 0.0 and i2 < m:
                    d = [float(PM[i][c]) - float(PM[i2][c]) for c in range(3)]
                    gap = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    near[i] = math.isfinite(gap) and gap <= float(F32(float(F32(o.max_gap)) * float(F32(o.max_gap))))
        words["RECIPROCAL"] = [n, sum(exact), sum(near), sum(exact) + sum(near)]
        masks.update(exact=exact, near=near)
        w = [exact[i] or near[i] for i in range(m)]
    if o.unique:
        best = {}
        for i in range(m):
            if w[i] and math.isfinite(geo[i]) and (ids[i] not in best or (geo[i], i) < best[ids[i]]):
                best[ids[i]] = (geo[i], i)
        cand = [w[i] and math.isfinite(geo[i]) for i in range(m)]
        win = [cand[i] and best[ids[i]][1] == i for i in range(m)]
        words["UNIQUE"] = [sum(cand), sum(win)]
        masks["winners"] = win
        w = [w[i] and (win[i] or not cand[i]) for i in range(m)]
    if o.keep is not None:
        cand = [w[i] and math.isfinite(geo[i]) for i in range(m)]
        n = sum(cand)
        K = min(int(math.ceil(float(F32(o.keep)) * n)), n)
        t = sorted(geo[i] for i in range(m) if cand[i])[K - 1]
        w = [cand[i] and geo[i] <= t for i in range(m)]
        words["TRIM"] = [int(F32(t).view(np.uint32)), n, K, sum(w)]
        masks["trim's candidates"], masks["trimmed to"] = cand, list(w)
    if o.loss is not None:
        k2 = float(F32(o.scale)) ** 2
        w = [w[i] and math.isfinite(geo[i]) and float(F32(rref.omega(o.loss, geo[i] / k2))) != 0.0 for i in range(m)]
    masks["final"] = w
    return masks, words


def _case(seed):
    """300 pairs on a 15 x 20 fixed grid, every coordinate a small multiple of 1/4 (float32 and Python floats agree to the bit), with
    the ties planted: equal geo on one fixed point (pairs 10, 11 and 12, 13), many equal geo (so also at the trim threshold), a cosine
    exactly at min_cos = 0.5 (pair 20, accepted) and just below it (pair 21), fixed points on the rim and beside a hole."""
    rng = np.random.default_rng(seed)
    m = GW * ROWS
    F = np.zeros((m, 8), F32)
    F[:, 0] = 4.0 * (np.arange(m) % GW); F[:, 1] = 4.0 * (np.arange(m) // GW) + 4.0; F[:, 2] = 64.0 + rng.integers(0, 8, m) / 4.0
    holes = [GW * 5 + 6, GW * 12 + 3]
    F[holes, :3] = 0.0
    F[GW * 15 + 9, 2] = np.nan
    ids = rng.integers(0, m, m).astype(np.uint32)
    ids[::3] = rng.integers(0, m // 6, len(ids[::3]))              # (crowded fixed points)
    interior = GW * 8 + 7
    ids[(ids == interior) | (ids == interior + 2)] = interior + 1   # (the two planted fixed points have no other claimant)
    ids[[10, 11, 12, 13]] = [interior, interior, interior + 2, interior + 2]
    ids[[20, 21]] = [interior + 4, GW * 9 + 7]
    ids[[30, 31, 32, 33]] = [0, GW - 1, GW * 5 + 7, holes[1]]     # a corner, the rim, beside a hole, a hole
    inner = GW * 10 + 4                                           # (two more interior fixed points with two claimants each: the gap's edge)
    ids[(ids == inner) | (ids == inner + 2)] = inner + 1
    ids[[60, 61, 62, 63]] = [inner, inner, inner + 2, inner + 2]
    PF = np.ascontiguousarray(F[ids][:, :4])
    off = np.zeros((m, 3), F32)                                   # along one axis, nine lengths: few values of geo, many ties
    off[np.arange(m), rng.integers(0, 3, m)] = rng.choice(np.array([0.0, 1.0, 2.0, 4.0, 6.0, 8.0, 12.0, 12.25, 13.0], F32), m)
    PM = np.zeros((m, 4), F32)
    PM[:, :3] = PF[:, :3] + off
    PM[[10, 11], :3] = PF[[10, 11], :3] + F32(2.0)                  # equal geo, the lower index wins
    PM[12, :3] = PF[12, :3] + np.array([0, 0, 3], F32); PM[13, :3] = PF[13, :3] + np.array([3, 0, 0], F32)
    PM[[61, 63], :3] = PF[[61, 63], :3]                           # the fixed point's own answer; 60 lies exactly 8 from 61, 62 8.25 from 63
    PM[60, :3] = PF[60, :3] + np.array([8, 0, 0], F32); PM[62, :3] = PF[62, :3] + np.array([0, 8.25, 0], F32)
    planted = [20, 21, 30, 31, 32, 33]
    PM[planted, :3] = PF[planted, :3] + np.array([0, 0, 1], F32)
    PM[40, 0] = np.inf
    M = PM.copy()
    M[rng.choice(m, 12, replace=False), :3] = 0.0                 # invalid moving points
    M[[10, 11, 12, 13, 60, 61, 62, 63] + planted, :3] = 1.0
    NF = np.zeros((m, 4), F32); NM = np.zeros((m, 4), F32)
    NF[:, :3] = rng.integers(-2, 3, (m, 3)); NM[:, :3] = rng.integers(-2, 3, (m, 3))
    NF[[interior, interior + 2, inner, inner + 2], :3] = [0, 0, 1]; NM[[10, 11, 12, 13, 60, 61, 62, 63], :3] = [0, 0, 2]
    NF[[interior + 4, GW * 9 + 7], :3] = [1, 1, 0]
    NM[20, :3] = [0, -1, 1]                                       # R90 takes it to (1, 0, 1): o = 1 = 0.5 sqrt (2 * 2)
    NM[21, :3] = [0, -np.nextafter(F32(1), F32(0)), 1]
    NM[50, 0] = np.nan
    # the back search's answer per fixed point (a generator of its own: the arrays above are what they were without it): one of the
    # fixed point's claimants (that pair is exact, the others depend on their gap to it), any query, or an index past m
    rng = np.random.default_rng(seed + 77)
    rev = rng.integers(0, m, m).astype(np.uint32)
    for j in range(m):
        claim = np.flatnonzero(ids == j)
        if len(claim) and rng.random() < 0.6:
            rev[j] = rng.choice(claim)
    rev[rng.choice(m, 20, replace=False)] = m + 5
    rev[[inner, inner + 2]] = [61, 63]
    if ids[41] not in (interior, interior + 2, inner, inner + 2):
        rev[ids[41]] = 40                                         # (a gap to the row with an infinite coordinate: not finite, rejected)
    return ids, PF, PM, F, M, NF, NM, rev


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("mask", range(32))
def test_against_the_plain_restatement(mask, seed):
    ids, PF, PM, F, M, NF, NM, rev = _case(4000 + seed)
    back = ((np.zeros(len(rev), np.dtype([("dist", F32), ("id", np.uint32)])), None), True)
    back[0][0]["id"] = rev
    nn_id = np.zeros(len(ids), np.dtype([("dist", F32), ("id", np.uint32)]))
    nn_id["id"] = ids
    loss = (rref.TUKEY, rref.HUBER, rref.CAUCHY)[seed]
    o = RouteOptions(False, True, 12.0, GW if mask & 1 else None, 0.5 if mask & 1 else None, bool(mask & 2), 0.75 if mask & 4 else None,
                     loss if mask & 8 else None, 8.0 if mask & 8 else None, 8.0 if mask & 16 else None)
    r = composed_rule(nn_id, PF, PM, F, M, R90.ravel(), NF, NM, o, back=back)
    masks, words = plain(ids, PF, PM, F, M, R90, NF, NM, o, rev)
    same = lambda a, b: np.array_equal(np.asarray(a, bool), np.asarray(b, bool))
    assert same(r.W0 != 0, masks["search"]), "the search's rejection"
    assert same(r.W != 0, masks["final"]), "the final weights"
    for name in words:
        assert (r.words[name] is None) == (words[name] is None) and (words[name] is None or r.words[name].tolist() == words[name]), \
            (name, r.words[name], words[name])
    if mask & 1:
        assert same(r.filter[0], masks["boundary"]) and same(r.filter[1], masks["incompatible"]) and same(r.filter[2], masks["accepted"])
        assert r.filter[2][20] and r.filter[1][21], "a cosine at min_cos is compatible, one below it is not"
        assert r.filter[0][[30, 31, 32]].all() and r.filter[2][[10, 11, 12, 13]].all()
    if mask & 16:
        assert same(r.reciprocal[0], masks["exact"]) and same(r.reciprocal[1], masks["near"])
        assert r.reciprocal[0][[61, 63]].all() and r.reciprocal[1][60] and not r.reciprocal[2][62], "a gap at max_gap is near, one above it is not"
        w = r.words["RECIPROCAL"]
        assert 0 < w[1] and 0 < w[2] and w[3] < w[0] and np.count_nonzero(rev[ids][r.W0 != 0] >= len(ids)) > 0
        below = o._replace(max_gap=float(np.nextafter(F32(8.0), F32(0.0))))
        rb = composed_rule(nn_id, PF, PM, F, M, R90.ravel(), NF, NM, below, back=back)
        mb, wb = plain(ids, PF, PM, F, M, R90, NF, NM, below, rev)
        assert rb.words["RECIPROCAL"].tolist() == wb["RECIPROCAL"] and same(rb.reciprocal[1], mb["near"]) and not rb.reciprocal[1][60]
        assert rb.words["RECIPROCAL"][2] < w[2], "the next float below the gap: the pairs exactly at it are near no longer"
    if mask & 2 and not mask & 16:
        assert same(r.unique[0], masks["winners"])
        assert r.unique[0][10] and not r.unique[0][11] and r.unique[0][12] and not r.unique[0][13], "a tie goes to the lowest query index"
    elif mask & 2:                                                # (whether 10 .. 13 are still candidates is the back search's to say)
        assert same(r.unique[0], masks["winners"])
    if mask & 4:
        assert same(r.trim, masks["trimmed to"])
        # a keep whose K-th and (K + 1)-th smallest geo are equal: the tie at the threshold, made on purpose
        n = int(r.words["TRIM"][1])
        geo = np.sort(unique_ref.geo(PF, PM)[masks["trim's candidates"]])
        K = 1 + int(np.flatnonzero(geo[:-1] == geo[1:])[len(geo) // 4])
        tied = o._replace(keep=(K - 0.5) / n)
        rt = composed_rule(nn_id, PF, PM, F, M, R90.ravel(), NF, NM, tied, back=back)
        mt, wt = plain(ids, PF, PM, F, M, R90, NF, NM, tied, rev)
        assert rt.words["TRIM"].tolist() == wt["TRIM"] and same(rt.trim, mt["trimmed to"]) and same(rt.W != 0, mt["final"])
        assert rt.words["TRIM"][2] == K and rt.words["TRIM"][3] > K, "pairs that tie at the threshold are all accepted"
    assert not r.W0[40] and 0 < np.count_nonzero(r.W) < np.count_nonzero(r.W0) + (0 if mask & 23 else 1)


# ---- 4. the projection at the head of the route ---------------------------------------------------------------------------------------
#
# tests/test_gpu_route_numerics.py section 2b: the pairs are projective_ref.project's at r = 1 (icp_checks.PROJ_ROUTE_SCENES), max_dist
# is the 0.88 quantile of the hits' own distances, min_cos and the scales are those of the scene the frames come from.

# scene -> (max_dist, min_cos, Tukey's scale), to three decimals
PROJ_CHOSEN = {"p30": (67.823, 0.485, 65.574), "p150": (120.935, 0.157, 55.019), "p150b1": (120.935, 0.157, 55.019), "p150b2": (120.935, 0.157, 55.019)}
# scene -> ICP_MEM_PROJECTIVE at _t0 (), and with every pass on ICP_MEM_PAIR_FILTER, ICP_MEM_UNIQUE and ICP_MEM_TRIM's (n, K, accepted)
PROJ_COUNTS = {"p30": ([803, 728, 60, 15], [640, 110, 59, 471], [471, 377], [377, 283, 283]),
               "p150": ([20048, 17200, 1363, 1485], [15136, 554, 1882, 12700], [12700, 10717], [10717, 8038, 8038]),
               "p150b1": ([19797, 17331, 1312, 1154], [14467, 626, 2076, 11765], [11765, 9707], [9707, 7281, 7281]),
               "p150b2": ([20196, 17408, 1031, 1757], [16502, 888, 1576, 14038], [14038, 11912], [11912, 8934, 8934])}


@pytest.mark.parametrize("name", list(PROJ_COUNTS))
def test_the_projective_choices_are_the_recorded_ones(engine, oracle, name):
    from icp_checks import PROJ_ROUTE_BATCH, PROJ_ROUTE_RADIUS, PROJ_ROUTE_SCENES, ProjectiveWant, geo_of
    import projective_ref
    assert list(PROJ_ROUTE_SCENES) == list(PROJ_COUNTS) and PROJ_ROUTE_RADIUS == 1
    s = route_scene(name)
    assert isinstance(s.want, ProjectiveWant) and s.max_gap is None and s.back is None
    assert s.projective == (s.side,) + tuple(engine.grid_intrinsics(s.side)) + (1,)
    got = (s.max_dist, s.min_cos, s.scale[rref.TUKEY])
    assert np.allclose(got, PROJ_CHOSEN[name], rtol=0, atol=1e-3), (got, PROJ_CHOSEN[name])
    assert float(F32(s.max_dist)) == s.max_dist and float(F32(s.min_cos)) == s.min_cos
    res = s.want.res
    # the expectation: the rule's pairs, the misses clipped to a row of F and weighing nothing; the tables the rules read are the rule's
    assert np.array_equal(s.want[0]["id"][~res.miss], res.nn_id["id"][~res.miss]) and not s.want[0]["id"][res.miss].any()
    assert np.isinf(s.want[0]["dist"][res.miss]).all() and s.PF is res.NN and s.PM is res.QT and not s.PF[res.miss].any()
    W0 = weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, s.max_dist)
    assert not W0[res.miss].any() and np.array_equal(s.T, route_scene(name[1:4].rstrip("b")).T)
    if name in PROJ_ROUTE_BATCH[:1] + ("p30",):                   # (max_dist is the 0.88 quantile of the hits' own distances)
        hits = int(res.counts[1])
        beyond = np.count_nonzero(~(geo_of(s.PF, s.PM)[~res.miss] <= F32(s.max_dist) * F32(s.max_dist)))
        assert abs(beyond - 0.12 * hits) <= 1.0, (beyond, hits)
    r, _ = route_proof(name, 15)
    t = r.words["TRIM"]
    assert (res.counts.tolist(), r.words["PAIR_FILTER"].tolist(), r.words["UNIQUE"].tolist(), [int(t[1]), int(t[2]), int(t[3])]) == PROJ_COUNTS[name]
    if name == "p150":                                            # (the figures the choice was made on)
        assert np.count_nonzero(r.W0 == 0) == 7364 and s.M.shape[0] == 22500
    if isinstance(PROJ_ROUTE_SCENES[name], str):                  # the two choices that do not work
        base = route_scene(PROJ_ROUTE_SCENES[name])
        assert s.F is base.F and s.M is base.M
        far = np.count_nonzero(W0) - np.count_nonzero(weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, base.max_dist))
        if name == "p150":
            assert np.count_nonzero(weights_before_trim(s.want[0], s.M, s.PF, s.PM, True, True, base.max_dist)) < s.M.shape[0] // 2, far
        else:                                                     # (r = 0: a cell has one query, seldom two: one-to-one has nothing to remove)
            r0 = projective_ref.project(oracle, s.F, s.M, s.T, s.side, engine.grid_intrinsics(s.side), 0, True)
            nn0 = projective_ref.clipped(r0.nn_id, r0.miss)
            o = route_scene_options(s, 2)
            u = composed_rule(nn0, r0.NN, r0.QT, s.F, s.M, s.R0, s.NF, s.NM, o).words["UNIQUE"]
            assert u[0] - u[1] <= 1, u


@pytest.mark.parametrize("mask", range(16))
@pytest.mark.parametrize("name", list(PROJ_COUNTS))
def test_every_stage_bites_behind_the_projection(engine, oracle, name, mask):
    """As test_every_stage_bites, on the projection's pairs: every scene, mask, loss and family the device grid runs (and more: every
    loss and both families on every scene)."""
    for loss in (LOSSES if mask & 8 else LOSSES[:1]):
        for plane in (False, True):
            r, shares = route_proof(name, mask, loss, plane)
            want = [n for bit, names in ((1, ("boundary", "normal", "filter")), (2, ("unique",)), (4, ("trim",))) if mask & bit for n in names]
            assert sorted(shares) == sorted(want + (["loss"] if mask & 8 and not plane else [])), shares
            for n, removed, kept in shares.values():
                assert 50 * removed >= n and 2 * kept >= n
    w = r.words
    if mask & 2:
        assert not mask & 1 or w["UNIQUE"][0] == w["PAIR_FILTER"][3]
    if mask & 4:
        front = w["UNIQUE"][1] if mask & 2 else w["PAIR_FILTER"][3] if mask & 1 else None
        assert front is None or w["TRIM"][1] == front
    assert w["RECIPROCAL"] is None and r.reciprocal is None
