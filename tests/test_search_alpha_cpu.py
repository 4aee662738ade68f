"""The premises of tests/test_gpu_search_alpha.py, from the CPU oracle alone (search_alpha_cases has the alphas and the scenes): on every
scene the GPU tests run, the alpha cases are what their names say.  A later change of the scene generator cannot empty them unnoticed.

(a) neg_winners: at least a quarter of the oracle's winning distances are below zero — and at least some are not: both signs meet in
    one reduction;
    neg_small: no winning distance is below zero with the queries at _t0 (), away from the fixed frame: the bodies the search takes
    without pruning run with the distances of a positive alpha (at the identity a frame's invalid points with their colours kept lie on
    the other frame's: geo = 0, d = a pho < 0);
(b) huge: at least a tenth of the queries have no finite distance, and at least a tenth have one;
(c) tiny, denormal: on every scene with invalid points at least a hundred queries win on a tie — two candidates of the scanned list have
    bit-equal minimal distance (search_alpha_cases.tie_queries: the list scanned backwards names another winner).
Every share is taken per scene over the three teacher-forced searches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_alpha_cases as cases      # noqa: E402

# (the scenes with 65536 points cost the oracle a second or more per search: the shares are asserted on every scene up to side 128 and on
# the scenes at side 256 with the fewest representatives — the 8192-representative scenes share their frames with those)
QUICK = [s for s in cases.SCENES if s.side < 256 or s.nr == 512 or s.kind != "synth"]


def _dists(scene, name):
    return [nn_id["dist"] for nn_id, _ in cases.searched(scene, name).steps]


@pytest.mark.parametrize("scene", QUICK, ids=str)
def test_negative_winners_share(engine, oracle, scene):
    d = np.concatenate(_dists(scene, "neg_winners"))
    neg = np.count_nonzero(d < 0)
    print(scene, "negative winners", neg, "of", d.size)
    assert 4 * neg >= d.size, (scene, neg, d.size)
    assert neg < d.size, (scene, "every winner is negative")
    small = _dists(scene, "neg_small")
    assert np.count_nonzero(small[1] < 0) == 0, (scene, [np.count_nonzero(x < 0) for x in small])


@pytest.mark.parametrize("scene", QUICK, ids=str)
def test_huge_alpha_shares(engine, oracle, scene):
    d = np.concatenate(_dists(scene, "huge"))
    none = np.count_nonzero(~(d < np.inf))
    print(scene, "queries without a finite distance", none, "of", d.size)
    assert 10 * none >= d.size and 10 * (d.size - none) >= d.size, (scene, none, d.size)
    assert not np.isnan(d).any()


@pytest.mark.parametrize("name", cases.TIE_ALPHAS)
@pytest.mark.parametrize("scene", [s for s in QUICK if s in cases.INVALID_SCENES], ids=str)
def test_tiny_alpha_ties(engine, oracle, scene, name):
    ties = [int(np.count_nonzero(cases.tie_queries(scene, name, k))) for k in range(3)]
    print(scene, name, "queries that win on a tie, per search", ties)
    assert sum(ties) >= 100, (scene, name, ties)


def test_the_oracle_refuses_what_the_engine_refuses(oracle):
    """orc_icp_init: alpha 0, NaN and +-inf are refused (icp_init's contract; tests/test_gpu_facade.py has the engine's side), every
    other float is taken."""
    for bad in (0.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            oracle.OracleICP(16, 4, bad)
    for name in cases.ALPHAS:
        oracle.OracleICP(16, 4, cases.alpha_of(name, 32))


def test_ordered_bits_order_every_float():
    """The key stage 2 reduces with lanes = candidates (ks_ordered_bits, icp_search.h), restated: u ^ ((int32 (u) >> 31) | 0x80000000).
    Its unsigned order is the float order over negative, zero, denormal, positive and infinite values, the plain bits' order is not, and
    the inverse gives the bits back."""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(1e4), rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array([-np.inf, -3.4e38, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 1.17549435e-38, 3.4e38, np.inf], np.float32)])
    v = np.unique(v[~np.isnan(v)])                                    # ascending by value (-0 and +0 are one value)
    u = v.view(np.uint32)
    key = u ^ ((u.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))
    assert (np.diff(key.astype(np.int64)) > 0).all()
    assert not (np.diff(u.astype(np.int64)) > 0).all()
    back = key ^ (((~key).view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))
    assert np.array_equal(back, u)
    assert key[v == np.inf][0] == key.max() and key[v == -np.inf][0] == key.min()
