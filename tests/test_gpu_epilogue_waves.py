"""The epilogue of the fused one-block-per-CU search (ks_epilogue, icp_search.h; ks_latency<true>, ks_chained, with and without
rejection) at the shapes and rules where a form that deals the block's 18 moments over several finishing waves could go wrong: that
form was built, passed these tests and measured slower (profiles/epilogue_waves_ab.txt), so they now pin the one-wave form.
Everything the moments feed — S, the means, sum W, T — and the last iteration's per-query outputs, bit for bit against the oracle.

Sides 8 (one block), 12 (144 landmarks, not a multiple of 8: blocks of 64 consecutive queries, the last one with 16 of its 64 lanes
valid — the invalid lanes must add +0 to every tree) and 128 (nb = 256: the finalize reads the moments through its two-group path)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_checks import (A, C_, IDENTITY, POWER, _t0, assert_bits, check_rejection_step, holes_pair, make_handle, one_step,  # noqa: E402
                        parity_check_step, parity_make, pick_max_dist, set_modes)

pytestmark = pytest.mark.gpu

SHAPES = [(8, 16), (12, 16), (128, 256)]


def check_moments_state(engine, g, o, weighted):
    """What the block moments turn into (S, means, sum W, T) and the per-query outputs of the last iteration."""
    parity_check_step(engine, g, o, weighted=False)                 # ids, distances, nearest representatives, means, S, Tk, Rk, R, T
    if weighted:
        assert_bits(g.read(engine.Memory.W), o.W, "weights")
        assert_bits(g.read(engine.Memory.SUM_W), np.array([o.sum_w]), "sum of weights")
    else:
        assert np.all(g.read(engine.Memory.W) == 1.0), "REGULAR mode: every weight is 1"


@pytest.mark.parametrize("weighted", [1, 0])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_chained_run_of_three_iterations(engine, oracle, side, nr, weighted):
    """The chained form, one launch per iteration: the state after each of three iterations, then the separate launches' search
    (ks_latency<true>) continues from there."""
    g, o, F, M = parity_make(engine, oracle, side, nr, weighted=weighted, power_fast=True, fused=True)
    assert g.search_layout()[0] == 0 and g.launches_per_iteration() == 1
    g.buildRBC(); o.build_rbc()
    for it in range(3):
        g.run_fixed(1); o.step()
        check_moments_state(engine, g, o, weighted)
    g.step(); o.step()
    check_moments_state(engine, g, o, weighted)
    g.close()


@pytest.mark.parametrize("chained", [True, False])
def test_an_empty_list_falls_back_to_the_representative(engine, oracle, chained):
    """A negative alpha (d = geo + a pho may be below zero): a representative's own point can lie nearer another one, its list is then
    empty, and a query whose nearest representative it is takes the representative itself — asserted from the oracle's structure."""
    side, nr, a = 32, 256, -1e5
    m = side * side
    F, M = engine.synth_pair(side)
    g = engine.ICP(0)
    g.init(m, nr, a, C_)
    set_modes(engine, g, power_fast=True, fused=True)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    o = oracle.OracleICP(m, nr, a, C_, threads=8, power_fast=True, fused=True)
    o.write_f(F); o.write_m(M)
    g.buildRBC(); o.build_rbc()
    for it in range(2):
        if chained:
            g.run_fixed(1)
        else:
            g.step()
        o.step()
        assert it or (np.asarray(o.rbc_N)[np.asarray(o.rid)] == 0).any(), "no query with an empty list"
        check_moments_state(engine, g, o, True)
    g.close()


@pytest.mark.parametrize("weighted", [1, 0])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_rejection_with_accepted_and_rejected_pairs(engine, oracle, side, nr, weighted):
    """The REJ kernels share the epilogue: invalid points and a distance cap that rejects part of the pairs — a rejected pair adds +0 to
    every moment (check_rejection_step asserts that the set is neither empty nor everything)."""
    F, M = holes_pair(engine, side, 0x1C9D5EED) if side >= 32 else engine.synth_pair(side, zero_fraction=0.2)
    T = _t0()
    cap = pick_max_dist(oracle, F, M, T, nr, frac=0.2)
    g = make_handle(engine, side * side, nr, True, weighted, POWER, True, rejection=(True, cap))
    assert g.search_layout()[0] == 0
    one_step(engine, g, F, M, T)
    check_rejection_step(engine, oracle, g, F, M, T, side, nr, True, weighted, POWER, True, True, cap)
    g.close()


@pytest.mark.parametrize("side,nr", SHAPES)
def test_nothing_accepted_leaves_zero_moments(engine, side, nr):
    """sum W == 0 under rejection: every moment +0, the identity step (as test_nothing_accepted_is_the_identity_step), chained run."""
    F, M = engine.synth_pair(side)
    T0 = _t0()
    g = make_handle(engine, side * side, nr, True, 1, POWER, True, rejection=(False, 1e-3))
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0, block=True)
    assert g.run() == 1
    Mem = engine.Memory
    assert_bits(g.read(Mem.T), T0, "T")
    assert_bits(g.read(Mem.TK), IDENTITY, "Tk")
    assert np.all(g.read(Mem.S).view(np.uint32) == 0) and np.all(g.read(Mem.MEANS).view(np.uint32) == 0)
    assert g.read(Mem.SUM_W)[0] == 0.0 and np.all(g.read(Mem.W).view(np.uint32) == 0)
    g.close()
