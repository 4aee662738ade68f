"""What tests/test_gpu_projective.py relies on, from the CPU oracle and numpy alone (no device): the scenes have hits, queries that land
outside the grid and — where the fixed set has invalid points — empty cells; no query's pixel lies at a rounding boundary, so the
float64 restatement and the device must agree on every cell; radius 0 pairs a query with the pixel itself; a window that covers the grid
is the brute-force nearest neighbour; the edge cases of e.z.

And what tests/test_gpu_projective_edges.py and the projective tests of tests/test_gpu_pyramid.py rely on: the four-round shapes and
their pinned counts; the constructed scenes whose pixels sit on a rounding boundary or straddle one (there the device is asked exactly
what the scenes above avoid: the same IEEE operations in double give the same cell, a float pixel or rint does not); the ties and the
candidates that never win; a metric scale and alphas that separate the two readings of the distance test; the pyramid levels' shares."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_checks                                               # noqa: E402
import projective_ref as ref                                    # noqa: E402
from icp_checks import A, IDENTITY                              # noqa: E402

F32 = np.float32


def shares(counts, what, empty=False):
    n, hits, outside, none = (int(x) for x in counts)
    assert hits + outside + none == n, (what, counts)
    assert 2 * hits >= n, "%s: hits %d of %d" % (what, hits, n)
    assert 100 * outside >= n, "%s: outside %d of %d" % (what, outside, n)
    if empty:
        assert 100 * none >= n, "%s: empty %d of %d" % (what, none, n)


def test_pinned_counts(engine, oracle):
    """The issue's float64 simulation gave n 16384 / hits 14416 / outside 1968 on the clean pair and 14767 / 11689 / 1775 / 1303 with a
    tenth of the points invalid; the exact restatement gives the same.  EXACT pins them for the device."""
    for (side, zf, r), want in ref.EXACT.items():
        res = ref.at(side, zf, r)
        assert tuple(int(x) for x in res.counts) == want, (side, zf, r, res.counts)
        shares(res.counts, (side, zf, r), empty=zf > 0 and r == 0)
    assert ref.EXACT[128, 0.0, 0] == (16384, 14416, 1968, 0) and ref.EXACT[128, 0.1, 0] == (14767, 11689, 1775, 1303)
    assert ref.EXACT[128, 0.1, 1][3] == 0
    for side, _ in ref.SMALL:
        n, hits = ref.EXACT[side, 0.0, 0][:2]
        assert 0.83 <= hits / n <= 0.885, (side, hits, n)


def test_every_other_scene_has_its_shares(engine, oracle):
    F, M, T = ref.rect_scene()
    for r in (0, 1):
        shares(ref.project(oracle, F, M, T, ref.RECT_GW, ref.RECT_INTRINSICS, r, True).counts, ("rect", r))
    for side, _ in icp_checks.MESSY_SHAPES:
        F, M = ref.messy_pair(side)
        intr = engine.grid_intrinsics(side)
        shares(ref.project(oracle, F, M, ref.scaled_T(), side, intr, 0, True).counts, ("messy", side), empty=True)
        res = ref.project(oracle, F, M, ref.turned_T(), side, intr, 1, True)
        assert res.counts[1] == 0 and res.counts[2] == res.counts[0] > 0 and res.miss.all(), res.counts     # (a half turn: every query outside)
        assert np.count_nonzero(~np.isfinite(M[:, :3]).all(axis=1)) == 30 and np.count_nonzero(~np.isfinite(F[:, :3]).all(axis=1)) == 30
    for seed, zf in ref.BATCH:
        shares(ref.at(ref.BATCH_SIDE, zf, 0, seed).counts, ("batch", seed), empty=zf > 0)
    counts = [tuple(ref.at(ref.BATCH_SIDE, zf, 1, seed).counts) for seed, zf in ref.BATCH]
    assert len(set(counts)) == 3, counts                            # (three different registrations)


def all_scenes(engine):
    out = [(ref.scene(side, zf) + (side, engine.grid_intrinsics(side))) for side, zf, _ in ref.EXACT]
    out += [ref.scene(ref.BATCH_SIDE, zf, seed) + (ref.BATCH_SIDE, engine.grid_intrinsics(ref.BATCH_SIDE)) for seed, zf in ref.BATCH]
    out.append(ref.rect_scene() + (ref.RECT_GW, ref.RECT_INTRINSICS))
    for side, _ in icp_checks.MESSY_SHAPES:
        out.append(ref.messy_pair(side) + (ref.scaled_T(), side, engine.grid_intrinsics(side)))
    return out


def test_no_pixel_at_a_rounding_boundary(engine, oracle):
    """pu = floor (u + 0.5) in double: the device and numpy evaluate the same IEEE operations, and no query comes within 1e-9 of the
    integer where a last-bit difference could move it to another cell (the closest, over all the scenes, is some 1e-6 away)."""
    closest = np.inf
    for F, M, T, gw, intr in all_scenes(engine):
        u, v, _, _ = ref.pixel(oracle.transform_q(M, T), intr)
        for w in (u, v):
            w = w[np.isfinite(w)] + 0.5
            closest = min(closest, float(np.abs(w - np.round(w)).min()))
    print("closest to an integer:", closest)
    assert closest > 1e-9


def test_radius_0_is_the_pixel(engine, oracle):
    for key in ((128, 0.1, 0), (30, 0.0, 0)):
        res = ref.at(*key)
        hit = ~res.miss
        assert np.array_equal(res.nn_id["id"][hit], (res.pv[hit] * key[0] + res.pu[hit]).astype(np.uint32))
        assert res.inside[hit].all()
        if key[1] == 0:                                             # (a clean fixed set: every inside query hits)
            assert np.array_equal(hit, res.inside)


def test_a_window_over_the_grid_is_the_nearest_neighbour(engine, oracle):
    """r >= side - 1 on a clean scene: the window of an inside query is all of F, and the winner is oracle.nn_brute's."""
    for side in (6, 9):
        F, M, T = ref.scene(side, 0.0)
        res = ref.project(oracle, F, M, T, side, engine.grid_intrinsics(side), side - 1, True)
        Q = oracle.transform_q(M, T)
        Q[:, 4:7] = M[:, 4:7]
        brute = oracle.nn_brute(Q, F, A)
        ins = res.inside
        assert ins.any() and np.array_equal(~res.miss, ins)
        assert np.array_equal(res.nn_id["id"][ins], brute["id"][ins])
        icp_checks.assert_bits(res.nn_id["dist"][ins], brute["dist"][ins], "distances")
        assert (res.nn_id["id"][~ins] == ref.NONE).all() and np.isinf(res.nn_id["dist"][~ins]).all()


def test_edge_cases_of_ez(engine, oracle):
    """ref.ez_scene (the device runs it in tests/test_gpu_projective_edges.py): a point on the camera plane (e.z = +-0), behind it, a
    denormal e.z in front of a finite e.x, or a pixel beyond float: a miss, with QT = (e, +inf).  A denormal coordinate is a number
    like any other: a point whose only non-zero coordinate is one counts, a denormal depth on the axis is inside."""
    side = ref.EZ_SIDE
    F, M = ref.ez_scene()
    row = ref.EZ_ROWS
    res = ref.project(oracle, F, M, IDENTITY, side, engine.grid_intrinsics(side), 0, True)
    out = [row[k] for k in ("z -0", "z +0", "z denormal", "behind", "only a denormal", "u beyond float")]
    assert res.miss[out].all() and not res.inside[out].any()
    ins = np.ones(side * side, bool)
    ins[out] = False
    assert np.array_equal(res.inside, ins) and np.array_equal(~res.miss, ins)
    assert np.isinf(res.QT[out, 3]).all() and (res.nn_id["id"][out] == ref.NONE).all()
    assert not res.NN[out].any() and np.count_nonzero(np.ascontiguousarray(res.NN[out]).view(np.uint32)) == 0   # (+0, not -0)
    assert res.counts.tolist() == [36, 30, 6, 0]                    # (every row counts, the point that is only a denormal too)
    E = oracle.transform_q(M, IDENTITY)
    assert np.array_equal(E[:9, :3], M[:9, :3]) and E[2, 2] == E[4, 2] == E[5, 0] == E[6, 0] == F32(1e-40) != 0      # (the identity keeps the denormals)
    u = ref.pixel(E, engine.grid_intrinsics(side))[0]
    assert np.isfinite(u[row["u beyond float"]]) and u[row["u beyond float"]] > 3.5e38 and u[row["z denormal"]] > 1e40
    assert (res.pu[row["denormal on the axis"]], res.pv[row["denormal on the axis"]]) == (3.0, 3.0)
    assert np.array_equal(res.nn_id["id"][9:], np.arange(9, side * side))                   # (the rest: every point on its own cell)
    # s = 0 sends every point to the translation: one cell, 36 hits on it
    res = ref.project(oracle, F, M, ref.collapsed_T(), side, engine.grid_intrinsics(side), 0, True)
    assert res.counts.tolist() == [36, 36, 0, 0] and len(set(res.nn_id["id"].tolist())) == 1
    assert np.array_equal(res.QT[:, :3], np.tile(ref.collapsed_T()[4:7], (36, 1)))


def test_four_round_shapes(engine, oracle):
    """ref.FOUR_ROUNDS: every shape is above batch m = 65536 and the one below it is not; the blocks, the live lanes of the last block's
    rounds and the counts the device is pinned to; every scene has its shares."""
    live = {}
    for side, nr, batch in ref.FOUR_ROUNDS:
        m = side * side
        assert batch * m > 65536 and m % 2 == 0
        blocks = -(-m // 1024)
        last = m - (blocks - 1) * 1024
        live[side, batch] = (blocks, [max(0, min(256, last - 256 * rd)) for rd in range(4)])
    assert live == {(258, 1): (66, [4, 0, 0, 0]), (150, 3): (22, [256, 256, 256, 228]), (30, 74): (1, [256, 256, 256, 132]),
                    (30, 73): (1, [256, 256, 256, 132])}
    assert 257 * 257 % 2 == 1 and 256 * 256 == 65536 and 72 * 900 <= 65536 < 73 * 900
    for r in (0, 1):
        res = ref.at(258, 0.1, r)
        assert tuple(int(x) for x in res.counts) == ref.EXACT[258, 0.1, r]
        shares(res.counts, (258, r), empty=r == 0)
        counts = [tuple(ref.at(150, zf, r, seed).counts) for seed, zf in ref.BATCH]
        assert len(set(counts)) == 3, counts
        for (seed, zf), c in zip(ref.BATCH, counts):
            shares(c, (150, seed, r), empty=zf > 0 and r == 0)


def test_exact_scene_sits_on_the_rounding_boundaries(engine, oracle):
    """ref.exact_scene: u + 0.5 (v + 0.5) of the boundary rows IS the integer k — in double, with a correctly rounded division —, the
    float32 below gives k - 1, and the restatement's pixels are the named ones.  Pixel 0 is inside at k = 0, k = 8 is outside, below
    k = 0 is outside; rint (u) in place of floor (u + 0.5) would move rows."""
    F, M, T, pu, pv = ref.exact_scene()
    side, intr = ref.EXACT_SIDE, ref.EXACT_INTRINSICS
    E = oracle.transform_q(M, T)
    assert np.array_equal(E[:, :3], M[:, :3]) and np.signbit(M[18, 0]) and np.signbit(M[37, 1])
    u, v, gu, gv = ref.pixel(E, intr)
    assert np.array_equal(gu, pu) and np.array_equal(gv, pv)
    on = (u + 0.5 == np.round(u + 0.5)) | (v + 0.5 == np.round(v + 0.5))
    assert np.count_nonzero(on[:38]) == 2 * 11 and not on[38:].any()                        # (k = 0 .. 8, -0, and below 0)
    assert sorted(set(pu[:19].tolist())) == list(range(-1, 9)) and sorted(set(pv[19:38].tolist())) == list(range(-1, 9))
    with np.errstate(all="ignore"):
        assert np.count_nonzero(np.rint(u) != gu) == 4 and np.count_nonzero(np.rint(v) != gv) == 4     # (k = 1, 3, 5, 7: ties to even)
    inside = ref.named_inside(pu, pv, side, side)
    assert np.count_nonzero(~inside) == 2 * 2                       # (per axis: below k = 0, and k = 8)
    assert inside[0] and pu[0] == 0 and not inside[1] and pu[1] == -1 and not inside[16] and pu[16] == 8 and inside[17] and pu[17] == 7
    for r in (0, 1):
        res = ref.project(oracle, F, M, T, side, intr, r, True)
        assert np.array_equal(res.inside, inside) and np.array_equal(~res.miss, inside)
        if r == 0:
            assert np.array_equal(res.nn_id["id"][inside], (pv * side + pu).astype(np.uint32)[inside])
    # (at r = 1 a row on a boundary is 1.5 from the centres of both cells it lies between, k = 1 .. 7, -0 and below 0: ties, which go
    # to the smaller j; k = 0 has one such cell)
    assert np.count_nonzero(res.nn_id["dist"][:38] == F32(1.5 * 1.5)) == 2 * 10


def test_straddle_scene_straddles(engine, oracle):
    """ref.straddle_scene: each pair of adjacent float32 coordinates really lies on either side of its boundary under the float64 rule,
    within 1e-6 of a pixel of it; the rule evaluated in float32 sends some of them to the wrong cell."""
    F, M, T, pu, pv = ref.straddle_scene()
    side, intr = ref.STRADDLE_SIDE, ref.straddle_intrinsics()
    intrinsics = ref.intrinsics32(intr)
    E = oracle.transform_q(M, T)
    assert np.array_equal(E[:, :3].view(np.uint32), M[:, :3].view(np.uint32))
    u, v, gu, gv = ref.pixel(E, intr)
    assert np.array_equal(gu, pu) and np.array_equal(gv, pv)
    for w, want, lo in ((u, pu, 0), (v, pv, 62)):
        rows = np.arange(lo, lo + 62)
        assert np.array_equal(want[rows], np.repeat(np.arange(31), 2) + np.tile([-1.0, 0.0], 31))
        assert np.array_equal(M[rows[1::2], lo // 62], np.nextafter(M[rows[0::2], lo // 62], F32(np.inf)))
        off = np.abs(w[rows] + 0.5 - np.round(w[rows] + 0.5))
        print("distance to the boundary, in pixels: %.2g .. %.2g" % (off.min(), off.max()))
        # (the pair is one float32 step apart, about 1.2e-6 of a pixel: both lie within that of the boundary, and hundreds of float64
        # steps of u + 0.5 from it — the device evaluates the same IEEE operations as numpy and has no room to disagree)
        step = intrinsics[lo // 62] * float(np.spacing(np.abs(M[rows, lo // 62]).max())) / ref.STRADDLE_Z
        assert 200 * np.spacing(31.0) < 1e-12 < off.min() and off.max() <= step < 2e-6
    fx, fy, cx, cy = (F32(x) for x in intr)
    u32 = np.floor(fx * (E[:, 0] / E[:, 2]) + cx + F32(0.5))
    v32 = np.floor(fy * (E[:, 1] / E[:, 2]) + cy + F32(0.5))
    flipped = np.count_nonzero(u32 != pu) + np.count_nonzero(v32 != pv)
    print("a float32 pixel moves %d of 124 rows" % flipped)
    assert flipped >= 10
    inside = ref.named_inside(pu, pv, side, side)
    assert np.count_nonzero(~inside) == 4 and inside[124:].all()    # (per axis: the lower neighbour at k = 0, the upper one at k = 30)
    for r in (0, 1):
        res = ref.project(oracle, F, M, T, side, intr, r, True)
        assert np.array_equal(res.inside, inside) and np.array_equal(~res.miss, inside)
        if r == 0:
            assert np.array_equal(res.nn_id["id"][inside], (pv * side + pu).astype(np.uint32)[inside])


def test_ties_scene_has_every_case(engine, oracle):
    """ref.ties_scene: the duplicates are bitwise duplicates at distance 0 and the winner is the smaller j, in both orders; the queries
    without a winner are inside, have valid candidates, and land in "empty"."""
    F, M, T, rows = ref.ties_scene()
    side, intr = ref.TIES_SIDE, engine.grid_intrinsics(ref.TIES_SIDE)
    fvalid = ref.valid_rows(F)
    E = oracle.transform_q(M, T)
    assert len(set(rows.values())) == len(rows) == 6
    for r in ref.TIES_RADII:
        res = ref.project(oracle, F, M, T, side, intr, r, True)
        x, y = res.pu.astype(int), res.pv.astype(int)
        for name in ("same row", "lower row"):
            i = rows[name]
            a, b = ((y[i] * side + x[i] - 1, y[i] * side + x[i] + 1) if name == "same row"
                    else (y[i] * side + x[i] + 1, (y[i] + 1) * side + x[i] - 1))
            assert a < b and F[a].tobytes() == F[b].tobytes() and oracle.metric8(np.r_[E[i, :4], M[i, 4:]], F[b], icp_checks.A) == 0.0
            assert res.nn_id[i]["id"] == a and res.nn_id[i]["dist"] == 0.0, (name, r)
            if name == "lower row":
                assert a % side > b % side                          # (the smaller j has the larger column)
        empty = res.inside & res.miss
        for name in ("huge", "nan query") + (("overflow", "nan colour") if r == 1 else ()):
            i = rows[name]
            ys, xs = np.arange(max(0, y[i] - r), min(side - 1, y[i] + r) + 1), np.arange(max(0, x[i] - r), min(side - 1, x[i] + r) + 1)
            js = (ys[:, None] * side + xs[None, :]).ravel()
            assert empty[i] and fvalid[js].all() and np.isfinite(E[i, :3]).all(), (name, r)
            d = np.array([oracle.metric8(np.r_[E[i, :4], M[i, 4:]], F[j], icp_checks.A) for j in js], F32)
            with np.errstate(all="ignore"):                         # (a far window of "huge" also reaches the cells with a NaN colour)
                assert not (d < np.inf).any() and (np.isnan(d).all() if name.startswith("nan") else np.isposinf(d).any()), (name, r)
        assert res.counts[3] == np.count_nonzero(empty) >= (4 if r == 1 else 2)
        assert res.counts[1] > 150
        for name in ("overflow", "nan colour"):                     # (at a larger radius the window reaches cells that can win)
            assert res.inside[rows[name]] and (r == 1 or not res.miss[rows[name]])
    assert np.count_nonzero(F[:, 0] == F32(3e38)) == 9 and np.count_nonzero(np.isnan(F[:, 4])) == 9 and fvalid.all()


def test_scale_and_alpha_separate_the_two_readings(engine, oracle):
    """ref.METRIC_SCENES with dist_scale = 0.37 and each alpha of ref.ALPHAS: the scaled distance differs from the unscaled one, alpha
    changes every distance and, at 1e5, the pairs, and ref.metric_max_dist separates the rule's reading of the distance test (the geometric distance) from the
    other one (the scaled d): each rejects between 2 % and half of the hits, and they differ in at least 2 % of the hits."""
    assert ref.ALPHAS[2] > 0 and F32(ref.ALPHAS[2]) / F32(2) == 0 and ref.METRIC_SCALE != 2.0 ** np.round(np.log2(ref.METRIC_SCALE))
    for side, zf, seed in ref.METRIC_SCENES:
        base = ref.at(side, zf, 1, seed)
        ids = []
        for alpha in ref.ALPHAS:
            res = ref.at_metric(side, zf, seed, alpha)
            hits = int(res.counts[1])
            shares(res.counts, (side, alpha))
            ids.append(res.nn_id["id"])
            assert np.array_equal(res.miss, base.miss)
            assert np.count_nonzero(res.nn_id["dist"] != base.nn_id["dist"]) == hits, (side, alpha)
            md = ref.metric_max_dist(res)
            rule, other = ref.metric_rejected(res, md), ref.metric_rejected(res, md, scaled=True)
            print(side, alpha, "hits", hits, "rejected by geo", np.count_nonzero(rule), "by d", np.count_nonzero(other),
                  "differ", np.count_nonzero(rule != other))
            for rej in (rule, other):
                assert 0.02 * hits <= np.count_nonzero(rej) <= 0.5 * hits, (side, alpha)
            assert np.count_nonzero(rule != other) >= 0.02 * hits, (side, alpha)
        assert np.count_nonzero(ids[0] != ids[1]) >= 0.02 * hits and np.count_nonzero(ids[2] != ids[1]) >= 0.02 * hits     # (alpha picks pairs)


def test_clipped_ids_and_zero_rows(engine, oracle):
    res = ref.at(128, 0.1, 0)
    nn = ref.clipped(res.nn_id, res.miss)
    assert (nn["id"] < 128 * 128).all() and np.isinf(nn["dist"][res.miss]).all() and np.array_equal(nn[~res.miss], res.nn_id[~res.miss])
    assert np.array_equal(ref.zero_rows(res.NN, res.QT, res.miss), res.miss)


def test_helpers():
    import icp_amd as engine
    assert engine.grid_intrinsics(128) == (119.0, 595.0 * 128 / 480.0, 63.9, 239.5 * 128 / 480.0)
    assert engine.landmark_intrinsics() == (148.75, 595.0 / 3.0, 63.625, 190.5 / 3.0)
    assert engine.Memory.PROJECTIVE == 29


def test_the_kernel_needs_no_scratch():
    """k_projective as the compiler reports it (tools/diag/kernel_resources.py; needs hipcc only): no scratch, and registers that leave
    its 256-thread blocks the full eight waves per SIMD."""
    from kernel_resources import kernel_resources
    r = kernel_resources("icp_amd/csrc/icp_projective.hip")
    k = [v for n, v in r.items() if n.startswith("k_projective")]
    assert len(k) == 1, sorted(r)
    assert k[0]["scratch"] == 0 and k[0]["dynamic_stack"] in (0, "False", False) and k[0]["vgprs"] <= 64, k[0]


def test_pyramid_levels_have_their_shares(engine, oracle):
    """ref.pyramid_chain (tests/test_gpu_pyramid.py runs it on the device): at the T every level starts from, under both reductions,
    no pixel lies within 1e-9 of a rounding boundary, and there are hits, outside queries and empty cells (r = 1: the holes of blobs30
    are wider than a window); a level's intrinsics put a clean point of the level's own grid on its own cell."""
    for kind in (ref.PYRAMID_MEAN, ref.PYRAMID_PICK):
        chain = ref.pyramid_chain(kind)
        assert [lv.side for lv in chain] == [128, 64, 32] and np.array_equal(chain[2].T, IDENTITY)
        for l, lv in enumerate(chain):
            u, v, _, _ = ref.pixel(oracle.transform_q(lv.M, lv.T), lv.intr)
            closest = min(float(np.abs(w[np.isfinite(w)] + 0.5 - np.round(w[np.isfinite(w)] + 0.5)).min()) for w in (u, v))
            print("reduction", kind, "level", l, "counts", lv.res.counts, "closest to a boundary", closest)
            assert closest > 1e-9
            shares(lv.res.counts, (kind, l), empty=True)
            if l < 2:
                assert np.array_equal(lv.T, chain[l + 1].T_next) and not np.array_equal(lv.T, IDENTITY)
            # the fixed frame at the identity: a valid point of the level lands on its own cell, which is what the level's intrinsics say
            own = ref.project(oracle, lv.F, lv.F, IDENTITY, lv.side, lv.intr, 0, True)
            hit = ~own.miss
            assert np.array_equal(hit, ref.valid_rows(lv.F)) and np.array_equal(own.nn_id["id"][hit], np.flatnonzero(hit))
