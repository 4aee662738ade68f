"""The one radix select (icp_amd/csrc/icp_select.h) under its two rules, against each other and against numpy.

ceil (0.5 n) == (n + 1) // 2 for every n, and 0.5 is exact in float: trimming at keep = 0.5 and median-distance rejection select the same
rank of the same candidates.  Two handles on the same F, M and T take one step each, one with set_trimming (0.5), one with
set_median_rejection (2.0): word 0 (t bits) and word 1 (n) of ICP_MEM_TRIM and of ICP_MEM_MEDIAN are those of numpy on the pairs read
back — the (n + 1) // 2-th smallest candidate geo and the candidate count — and equal each other.

The shapes, the smallest that reach each path: (10, 4) — 100 pairs, most keys of the one workgroup are padding —, (128, 256) — exactly
16384, the last shape of the one-workgroup kernels —, (130, 4) — 16900, three multi-workgroup passes, the last workgroup partly
filled —, and three registrations of (130, 4) with different holes: per-registration state words, histograms and tickets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_checks import POWER, WEIGHTED, _t0, geo_of, holes_pair, make_handle, step_batch, weights_before_trim      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("side,nr,batch", [(10, 4, 1), (128, 256, 1), (130, 4, 1), (130, 4, 3)])
def test_trimming_at_half_and_the_median_select_the_same(engine, side, nr, batch):
    from icp_amd import workloads as W
    Mem = engine.Memory
    m = side * side
    pairs = [holes_pair(engine, side, W.BASE_SEED + 5 * b) for b in range(batch)]
    T = _t0()
    words = {}
    for mem in ("TRIM", "MEDIAN"):
        g = make_handle(engine, m, nr, True, WEIGHTED, POWER, True, batch, rejection=(True, None), trimming=0.5 if mem == "TRIM" else None)
        if mem == "MEDIAN":
            g.set_median_rejection(2.0)
        step_batch(engine, g, pairs, T)
        words[mem] = []
        for b, (F, M) in enumerate(pairs):
            nn_id, PF, PM = g.read(Mem.NN_ID, batch_index=b), g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
            geo = geo_of(PF, PM)
            cand = geo[(weights_before_trim(nn_id, M, PF, PM, True, True) != 0) & np.isfinite(geo)]
            n = cand.size
            assert 0 < n < m, (mem, b, n)
            t = np.sort(cand)[(n + 1) // 2 - 1]
            got = g.read(getattr(Mem, mem), batch_index=b)
            print("%s registration %d: got %s, numpy t bits %d n %d" % (mem, b, got.tolist(), t.view(np.uint32), n))
            assert (int(got[0]), int(got[1])) == (int(t.view(np.uint32)), n), (mem, b, got)
            words[mem].append((int(got[0]), int(got[1])))
        g.close()
    assert words["TRIM"] == words["MEDIAN"], words
    assert len(set(words["TRIM"])) == batch, "the registrations' candidates differ"
