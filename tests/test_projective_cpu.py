"""What tests/test_gpu_projective.py relies on, from the CPU oracle and numpy alone (no device): the scenes have hits, queries that land
outside the grid and — where the fixed set has invalid points — empty cells; no query's pixel lies at a rounding boundary, so the
float64 restatement and the device must agree on every cell; radius 0 pairs a query with the pixel itself; a window that covers the grid
is the brute-force nearest neighbour; the edge cases of e.z."""
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
    """A point on the camera plane (e.z = +-0), behind it, or a denormal e.z in front of a finite e.x: a miss, with QT = (e, +inf)."""
    side = 6
    F, _, _ = ref.scene(side, 0.0)
    M = np.zeros((side * side, 8), F32)
    M[:, :3] = (100.0, 50.0, 1000.0)
    M[0, 2], M[1, 2], M[2, 2], M[3, 2] = -0.0, 0.0, 1e-40, -1000.0
    M[4, :3] = (0.0, 0.0, 1e-40)                                    # (a denormal depth on the optical axis projects to (cx, cy): inside)
    res = ref.project(oracle, F, M, IDENTITY, side, engine.grid_intrinsics(side), 0, True)
    assert res.miss[:4].all() and not res.inside[:4].any()
    assert res.inside[4] and res.inside[5:].all()
    assert np.isinf(res.QT[:4, 3]).all() and (res.nn_id["id"][:4] == ref.NONE).all()
    assert not res.NN[:4].any() and np.count_nonzero(np.ascontiguousarray(res.NN[:4]).view(np.uint32)) == 0     # (+0, not -0)


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
