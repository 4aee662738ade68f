"""Both correspondence sets (icp_correspondences, include/icp_amd.h) in every search layout, on frames with nothing in them and with
non-finite moving points.

1. Every layout (icp_checks.LAYOUT_CASES): one step from _t0 () with rejection (invalid points, max_dist) and trimming on, WEIGHTED —
   the icp_search_rej.hip instantiation of the layout.  ICP_PAIRS_LAST_ITERATION of every registration against composed_rule on the
   oracle's search at _t0 () (icp_checks.check_route_pairs); ICP_PAIRS_EVALUATED and icp_evaluate at the T the step left against the
   oracle's search there — evaluation_search in the handle's layout.  Nothing of an expectation is read from the handle but that T.
   tests/test_pairs_routes_cpu.py proves from the oracle alone that every expected set holds between 10 % and 90 % of the counted
   points and that the counts of a batch are pairwise distinct; both are asserted on the device's expectation again.
2. Frames with nothing in them: the compaction's corner cases — a registration with count 0, a single member in the first or the last
   lane of the set, a fixed frame of invalid points only — in the latency layout and dense by batch.
3. Non-finite moving points: a NaN and an infinite coordinate in M.

Comparisons are exact: the count, then the records by their raw bytes."""
import ctypes as C

import numpy as np
import pytest

import icp_checks as K
import pairs_ref
import quality_ref
from pairs_ref import check_set
from quality_ref import check_record

pytestmark = pytest.mark.gpu

UNTOUCHED = 0xFFFFFFF7


def _counts(engine, g, source, max_dist, count):
    """icp_correspondences for registrations 0 .. count - 1 into an array of the batch's length filled with UNTOUCHED."""
    out = (C.c_uint32 * g.batch)(*([UNTOUCHED] * g.batch))
    rc = engine.lib().icp_correspondences(g._h, source, max_dist, out, count)
    assert rc == 0, (rc, engine.lib().icp_last_error(g._h))
    return list(out)


def _batch_interface(engine, g, source, max_dist, sets, what):
    """The sets of a batch are pairwise different in size; a call for registration 0 alone leaves counts[1:] untouched; after one call
    for all of them icp_correspondences_read delivers every registration's set."""
    sizes = [len(s) for s in sets]
    assert len(set(sizes)) == len(sizes), "%s: the counts of the batch are not pairwise distinct: %r" % (what, sizes)
    assert _counts(engine, g, source, max_dist, 1) == sizes[:1] + [UNTOUCHED] * (g.batch - 1), what
    assert _counts(engine, g, source, max_dist, g.batch) == sizes, what
    for b, s in enumerate(sets):
        check_set(g.correspondences_read(b), s, "%s: icp_correspondences_read (%d) behind one call" % (what, b))


# ---- 1. every search layout -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.LAYOUT_CASES, ids=lambda c: "%d-%d-%d-%s-%s" % (c[0], c[1], c[2], "fused" if c[3] else "reference_order", c[4]))
def test_both_sets_in_every_layout(engine, oracle, case):
    side, nr, batch, fused, zero, layout = case
    m = side * side
    Mem, Pairs = engine.Memory, engine.Pairs
    sc = K.layout_scene(side, nr, batch, zero)
    g = K.make_handle(engine, m, nr, fused, K.WEIGHTED, K.POWER, fused, batch, rejection=(True, sc.max_dist), trimming=K.LAYOUT_KEEP)
    assert g.search_layout() == layout, g.search_layout()
    if batch == 1:
        K.one_step(engine, g, sc.pairs[0][0], sc.pairs[0][1], sc.T)
    else:
        K.step_batch(engine, g, sc.pairs, sc.T)
    last = []
    for b, ((F, M), want, r) in enumerate(zip(sc.pairs, sc.wants, sc.rules)):
        what = "side %d, |R| %d, registration %d of %d" % (side, nr, b, batch)
        K.check_search(engine, g, want, b)
        K.assert_words(engine, g, "TRIM", r.words["TRIM"], b)
        counted = int(np.count_nonzero(quality_ref.masks(M, sc.PF[b], sc.PM[b], 0.0)[0]))
        assert 0.1 * counted <= np.count_nonzero(r.W) <= 0.9 * counted, (what, np.count_nonzero(r.W), counted)
        last.append(K.check_route_pairs(engine, g, want[0], sc.PF[b], sc.PM[b], r, False, sc.options, b, what))
        assert len(np.unique(last[b]["weight"])) > 100, "WEIGHTED: the weights carry non-trivial bits"
    if batch > 1:
        _batch_interface(engine, g, Pairs.LAST_ITERATION, 0.0, last, "LAST_ITERATION")
    # the evaluation at the T the step left
    Ts = [g.read(Mem.T, b).copy() for b in range(batch)]
    wants = [K.oracle_search(oracle, F, M, T, nr) for (F, M), T in zip(sc.pairs, Ts)]
    max_dist = K.pick_max_dist(oracle, sc.pairs[0][0], sc.pairs[0][1], Ts[0], nr, frac=0.3, nn_id=wants[0][0])
    recs = g.evaluate(max_dist)
    ev = []
    for b, ((F, M), T, want) in enumerate(zip(sc.pairs, Ts, wants)):
        what = "side %d, |R| %d, registration %d of %d, evaluated" % (side, nr, b, batch)
        e, q = K.evaluated_expectation(oracle, F, M, T, nr, max_dist, want)
        assert 0.1 * q.n_moving <= len(e) <= 0.9 * q.n_moving, (what, len(e), q.n_moving)
        check_set(g.correspondences(Pairs.EVALUATED, max_dist, batch_index=b), e, what)
        check_record(recs[b], q, m, what)
        assert len(e) == recs[b].n_inliers
        ev.append(e)
    if batch > 1:
        _batch_interface(engine, g, Pairs.EVALUATED, max_dist, ev, "EVALUATED")
    for b in range(batch):                               # (the evaluation has left the iteration's outputs alone)
        check_set(g.correspondences(Pairs.LAST_ITERATION, batch_index=b), last[b], "LAST_ITERATION behind the evaluation, registration %d" % b)
    g.close()


# ---- 2. frames with nothing in them -----------------------------------------------------------------------------------------------------

EMPTY_CASES = "abcd"


def _empty_pair(engine, side, case, seed):
    """(F, M, the index of M's only valid point or None): (a) M all (0, 0, 0); (b) F all (0, 0, 0), M clean; (c) M valid only at index 0;
    (d) M valid only at index m - 1.  The colours stay."""
    F, M = engine.synth_pair(side, seed=seed)
    m = side * side
    only = {"c": 0, "d": m - 1}.get(case)
    if case == "b":
        F[:, :3] = 0.0
    else:
        keep = M[only, :3].copy() if only is not None else None
        M[:, :3] = 0.0
        if only is not None:
            M[only, :3] = keep
    return F, M, only


def _check_empties(engine, oracle, side, nr, cases, dense):
    """One handle with a registration per case of `cases`, ICP_REJECT_INVALID on, in the latency (dense = 0) or the dense layout.

    EVALUATED and icp_evaluate run at _t0 (), in front of the step, against the oracle's search there, without a distance test: the
    step of such a frame leaves no usable T (one accepted pair is a degenerate S; the solver's NaN).  LAST_ITERATION runs behind the
    step against the handle's own NN_ID / W / NN / QT (pairs_ref.last_iteration): icp_checks.composed_rule is not defined for an
    empty candidate set (its stages and their proofs speak of scenes in which every stage has pairs to remove and pairs to keep).
    Behind the step, where T may be NaN, only the count of EVALUATED is compared, with icp_evaluate's."""
    m, batch = side * side, len(cases)
    Mem, Pairs, L = engine.Memory, engine.Pairs, engine.lib()
    frames = [_empty_pair(engine, side, c, 0x3A7 + 13 * b) for b, c in enumerate(cases)]
    g = K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, batch, rejection=(True, None))
    assert g.search_layout()[0] == dense, g.search_layout()
    T = K._t0()
    for b, (F, M, _) in enumerate(frames):
        K.load(engine, g, F, M, b)
    g.buildRBC()
    for b in range(batch):
        g.write(Mem.T, T, batch_index=b, block=True)
    recs = g.evaluate(0.0)
    sizes = _counts(engine, g, Pairs.EVALUATED, 0.0, batch)
    n = C.c_uint32(99)
    for b, (case, (F, M, only)) in enumerate(zip(cases, frames)):
        what = "side %d, case %s, evaluated" % (side, case)
        e, q = K.evaluated_expectation(oracle, F, M, T, nr, 0.0)
        got = g.correspondences_read(b)
        check_set(got, e, what)
        check_record(recs[b], q, m, what)
        assert sizes[b] == len(e) == recs[b].n_inliers
        if case in "ab":
            assert len(got) == 0
            n.value = 99
            assert L.icp_correspondences_read(g._h, b, None, 0, C.byref(n)) == 0 and n.value == 0, (what, n.value)
            assert recs[b].n_moving == (0 if case == "a" else m) and recs[b].n_inliers == 0 and recs[b].fitness == 0.0, what
        else:
            assert len(got) == 1 and got["moving"][0] == only and got["weight"][0] == 1.0 and np.isfinite(got["geo"][0]), (what, got)
            assert recs[b].n_moving == 1 and recs[b].n_inliers == 1 and recs[b].fitness == 1.0, what
    g.step()
    sizes = _counts(engine, g, Pairs.LAST_ITERATION, 0.0, batch)
    for b, (case, (F, M, only)) in enumerate(zip(cases, frames)):
        what = "side %d, case %s, the last iteration" % (side, case)
        want = pairs_ref.last_iteration(g.read(Mem.NN_ID, b), g.read(Mem.W, b), g.read(Mem.NN, b), g.read(Mem.QT, b))
        got = g.correspondences_read(b)
        check_set(got, want, what)
        assert sizes[b] == len(got) == (0 if case in "ab" else 1), (what, sizes[b])
        if case in "ab":
            n.value = 99
            assert L.icp_correspondences_read(g._h, b, None, 0, C.byref(n)) == 0 and n.value == 0, (what, n.value)
        else:
            assert got["moving"][0] == only and got["weight"][0] != 0 and np.isfinite(got["geo"][0]), (what, got)
    after = g.evaluate(0.0)                              # (T may be NaN here: the counts only)
    sizes = _counts(engine, g, Pairs.EVALUATED, 0.0, batch)
    for b, case in enumerate(cases):
        assert sizes[b] == len(g.correspondences_read(b)) == after[b].n_inliers and after[b].n_moving == recs[b].n_moving, (case, sizes[b])
        if case in "ab":
            assert sizes[b] == 0
    g.close()


@pytest.mark.parametrize("case", EMPTY_CASES)
def test_frames_with_nothing_in_them_latency(engine, oracle, case):
    """(30, 4): m = 900, four blocks of 256 pairs, the last one ragged — case d's only member sits in its last occupied lane."""
    _check_empties(engine, oracle, 30, 4, case, 0)


def test_frames_with_nothing_in_them_dense_by_batch(engine, oracle):
    """(128, 256) in a batch of four, registrations 0 .. 3 carrying cases a .. d: one launch set, the empty sets beside the others."""
    _check_empties(engine, oracle, 128, 256, EMPTY_CASES, 1)


# ---- 3. non-finite moving points ----------------------------------------------------------------------------------------------------------

def test_non_finite_moving_points(engine, oracle):
    """(50, 4), REGULAR weights, no rejection; a NaN coordinate in one row of M, +inf in another.

    EVALUATED at _t0 (): neither row is a member, the set is the oracle expectation's.  LAST_ITERATION behind one step: the set of the
    handle's own four arrays; geo is compared by assert_bits_nan's rule (NaN in the same places, bits elsewhere: the payload of an
    invalid operation differs between the device and numpy).  Whether the two rows are members is ICP_MEM_W's to say, and is printed."""
    side, nr = 50, 4
    m = side * side
    Mem, Pairs = engine.Memory, engine.Pairs
    F, M = engine.synth_pair(side)
    T = K._t0()
    clean, _ = K.evaluated_expectation(oracle, F, M, T, nr, 0.0)
    assert len(clean) == m
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)   # (on the clean pair: a quantile of finite distances)
    rows = (1237, 300)                                   # (inside block 4 of 256 pairs; inside block 1)
    M[rows[0], 1] = np.nan
    M[rows[1], 2] = np.inf
    g = K.make_handle(engine, m, nr, True, K.REGULAR, K.POWER, True)
    K.load(engine, g, F, M)
    g.buildRBC()
    g.write(Mem.T, T, block=True)
    for md in (0.0, max_dist):
        e, q = K.evaluated_expectation(oracle, F, M, T, nr, md)
        assert not np.isin(rows, e["moving"]).any() and q.n_moving == m - 2
        assert len(e) == m - 2 if md == 0.0 else 0.1 * m <= len(e) <= 0.9 * m, len(e)
        check_set(g.correspondences(Pairs.EVALUATED, md), e, "non-finite rows, max_dist %g" % md)
        check_record(g.evaluate(md)[0], q, m, "non-finite rows, max_dist %g" % md)
    g.step()
    W = g.read(Mem.W)
    want = pairs_ref.last_iteration(g.read(Mem.NN_ID), W, g.read(Mem.NN), g.read(Mem.QT))
    got = g.correspondences(Pairs.LAST_ITERATION)
    print("ICP_MEM_W at the NaN row %r, at the inf row %r; members: %r" % (W[rows[0]], W[rows[1]], np.isin(rows, got["moving"]).tolist()))
    assert got.dtype == pairs_ref.PAIR and len(got) == len(want) >= m - 2, (len(got), len(want))
    for field in ("moving", "fixed"):
        assert np.array_equal(got[field], want[field]), field
    K.assert_bits(got["weight"], want["weight"], "weight")
    K.assert_bits_nan(got["geo"], want["geo"], "geo")
    assert np.array_equal(np.isin(rows, got["moving"]), W[list(rows)] != 0)
    assert np.isfinite(np.delete(got["geo"], np.nonzero(np.isin(got["moving"], rows))[0])).all()
    g.close()
