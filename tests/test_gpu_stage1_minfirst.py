"""Stage 1 of the one-block-per-CU search, minimum first and the index afterwards (ks_group_min_first, icp_search.h): every output bit
for bit against the oracle, in the fused chained form (run_fixed), the fused separate launches (step) and the reference-order latency
form, and the owner search of buildRBC (check_rbc), which shares the scan.

Shapes (side, nr): (8, 1) one pair with the NaN pad slot; (8, 2) one pair; (8, 8) and (8, 32) fewer pairs than a group's lanes can
take / one pair per lane, side 8 being a single block; (16, 32); (16, 128) half a group per lane (the PARTIAL form with every lane
busy); (32, 256) exactly one group; (64, 512) two groups; (64, 1024) four groups, a whole tile.
The representative count of a handle is a power of two whose grid divides the landmark grid (reps_grid, icp_capi.hip; the oracle's
orc_reps_grid): (8, 31), (16, 255) and (64, 272) are no handles at all — test_counts_that_are_no_power_of_two_are_refused pins that,
engine and oracle alike —, so an odd tile is nr = 1 alone and a partial group is nr < 256 alone; (8, 8), (8, 32), (16, 128) and
(64, 512) stand where those three cannot.

Ties.  synth_pair's zero_fraction leaves invalid points — coordinates AND colour zero —, so every representative sampled from one is
the same point: all of them are at the same distance from every query, and a query that is itself an invalid point (distance 0 under
the identity the registration starts from) has its nearest distance attained by every one of them.  The lowest index must win.  Which
lanes the tied representatives fall to — representative r is half r & 1 of pair r >> 1, pair P belongs to lane P mod 16 — is
asserted over the cases: one lane's same pair, one lane's different pairs (indices a multiple of 32 apart), different lanes."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_checks import A, C_, assert_bits, check_rbc, parity_check_step, parity_make, set_modes  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(8, 1), (8, 2), (8, 8), (8, 32), (16, 32), (16, 128), (32, 256), (64, 512), (64, 1024)]
REFUSED = [(8, 31), (16, 255), (64, 272)]
ZERO = 0.3
LPQ = 16                                             # lanes per query of the one-block-per-CU variants


def seed_of(side, nr):
    return 0x51 + 7 * side + nr


def zero_rows(X):
    return np.nonzero((X[:, [0, 1, 2, 4, 5, 6]] == 0.0).all(axis=1))[0]


def placements(z):
    """Which of the three placements the tied representatives `z` (ascending indices) take among a query's 16 lanes."""
    out = set()
    for a in range(len(z)):
        for b in range(a + 1, len(z)):
            pa, pb = z[a] >> 1, z[b] >> 1
            out.add("same pair" if pa == pb else "same lane" if pa % LPQ == pb % LPQ else "other lane")
    return out


@functools.lru_cache(maxsize=None)
def tie_facts(side, nr):
    """(tied representatives, queries that tie on them) of a case's scene, from the oracle's REPS — CPU only."""
    from oracle import oracle as O
    import icp_amd
    F, M = icp_amd.synth_pair(side, seed=seed_of(side, nr), zero_fraction=ZERO)
    o = O.OracleICP(side * side, nr, A, C_, threads=8)
    o.write_f(F); o.write_m(M); o.build_rbc()
    z, q = zero_rows(np.asarray(o.reps)), zero_rows(M)
    o.step()
    if len(z) and len(q):                            # the oracle's own answer: the lowest of the tied indices
        assert (np.asarray(o.rid)[q] == z[0]).all(), (side, nr, z[:4])
    return tuple(int(v) for v in z), len(q)


def test_the_scenes_tie_in_every_placement():
    seen = set()
    for side, nr in SHAPES:
        z, nq = tie_facts(side, nr)
        if nr >= 32:
            assert len(z) >= 2, "(%d, %d): fewer than two equal representatives" % (side, nr)
            assert nq >= 1, "(%d, %d): no query whose nearest distance two representatives attain" % (side, nr)
        if nq:
            seen |= placements(z)
    assert seen == {"same pair", "same lane", "other lane"}, seen


@pytest.mark.parametrize("side,nr", REFUSED)
def test_counts_that_are_no_power_of_two_are_refused(engine, oracle, side, nr):
    g = engine.ICP(0)
    with pytest.raises(engine.ICPError):
        g.init(side * side, nr, A, C_)
    g.close()
    with pytest.raises(ValueError):
        oracle.OracleICP(side * side, nr, A, C_)


@pytest.mark.parametrize("side,nr", SHAPES)
def test_fused_forms_bit_for_bit(engine, oracle, monkeypatch, side, nr):
    """buildRBC (the owner search), one iteration as separate launches, then the chained form: one launch, two more.  From 1024
    representatives on a handle takes the dense variants by itself: there ICP_AMD_CHAIN=1 (read at icp_create) forces the chained
    kernel — the one-block-per-CU stage 1 over a whole tile, four groups per lane — and every iteration runs through it."""
    tie_facts(side, nr)
    forced = nr >= 1024
    if forced:
        monkeypatch.setenv("ICP_AMD_CHAIN", "1")
    else:
        monkeypatch.delenv("ICP_AMD_CHAIN", raising=False)
    g, o, F, M = parity_make(engine, oracle, side, nr, power_fast=True, zero_fraction=ZERO, seed=seed_of(side, nr), fused=True)
    assert g.run_form() == 1 and g.launches_per_iteration() == 1              # chained
    assert forced or g.search_layout()[0] == 0                                # the one-block-per-CU variants
    g.buildRBC(); o.build_rbc()
    check_rbc(engine, g, o)
    if forced:
        g.run_fixed(1)
    else:
        g.step()
    o.step()
    parity_check_step(engine, g, o, weighted=False)
    for n in (1, 2):
        g.run_fixed(n)
        for _ in range(n):
            o.step()
        parity_check_step(engine, g, o, weighted=False)
    g.close()


@pytest.mark.parametrize("side,nr", SHAPES)
def test_reference_order_form_bit_for_bit(engine, oracle, side, nr):
    """The reference-order latency form, ks_latency<false> (from 1024 representatives on: the dense variant, which this scan is no part of)."""
    g, o, F, M = parity_make(engine, oracle, side, nr, zero_fraction=ZERO, seed=seed_of(side, nr))
    assert nr >= 1024 or g.search_layout()[0] == 0
    g.buildRBC(); o.build_rbc()
    check_rbc(engine, g, o)
    for _ in range(2):
        g.step(); o.step()
        parity_check_step(engine, g, o)
    g.close()


@pytest.mark.parametrize("fused,chained", [(True, True), (True, False), (False, False)])
def test_an_infinite_query_and_nan_representatives(engine, oracle, fused, chained):
    """A tenth of F's rows with a NaN coordinate — some representatives are NaN: their distances never equal a group's minimum —, queries
    with an infinite coordinate — every distance +inf or NaN: the group's minimum is not below +inf and names no position, representative 0
    as the serial scan would — and a NaN query: as test_nan_and_inf_points_do_not_break_the_search, at exactly one group."""
    side, nr = 32, 256
    m = side * side
    F, M = engine.synth_pair(side, seed=0x77)
    rng = np.random.default_rng(9)
    F[rng.choice(m, m // 10, replace=False), 1] = np.nan
    M[rng.choice(m, 3, replace=False), 0] = np.inf
    M[7, 2] = -np.inf
    M[300, 5] = np.nan
    g = engine.ICP(0)
    g.init(m, nr, A, C_)
    set_modes(engine, g, power_fast=fused, fused=fused)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    o = oracle.OracleICP(m, nr, A, C_, threads=8, power_fast=fused, fused=fused)
    o.write_f(F); o.write_m(M)
    g.buildRBC(); o.build_rbc()
    assert np.isnan(np.asarray(o.reps)[:, :3]).any(), "no NaN representative"
    check_rbc(engine, g, o)
    if chained:
        g.run_fixed(1)
    else:
        g.step()
    o.step()
    gn, on = g.read(engine.Memory.NN_ID), o.nn_id
    assert np.array_equal(g.read(engine.Memory.RID), o.rid)
    assert np.array_equal(gn["id"], on["id"])
    assert np.isinf(on["dist"]).any() and not np.isnan(on["dist"]).any()
    assert_bits(gn["dist"], on["dist"], "distances")
    assert np.isnan(g.read(engine.Memory.T)).all() and np.isnan(o.T).all()
    g.close()
