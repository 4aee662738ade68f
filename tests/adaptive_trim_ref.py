"""Adaptive trimming (icp_set_adaptive_trimming, include/icp_amd.h) restated in numpy — TEST INFRASTRUCTURE (a plain module: pytest
collects nothing from it).

Candidates are the pairs with a weight != 0 (W0: what the passes in front have left) and a finite geo; n their number; the key of a
candidate is the bit pattern of its geo, its bin key >> 19.  Per bin c_j and B_j (the sum of its geo in double: exact in any order);
r_j the cumulative counts, S_j the cumulative sums in the rule's run order (64 runs of 64 bins, then the bases); the candidate bins
are the non-empty ones between the first with r_j >= r_lo and the first with r_j >= r_hi; cost_j = S_j / r_j^q by successive
multiplications; the winner has the smallest (cost, j).  The words are ICP_MEM_TRIM's (t, n, K, accepted) and ICP_MEM_TRIM_ADAPTIVE's
(j*, r_lo, r_hi, candidate bins).

brute_force is the rule's twin without a table: the candidates sorted, every bin end evaluated in Python floats, math.fsum per bin."""
import math

import numpy as np

from icp_checks import geo_of

BINS, SHIFT = 4096, 19


def rank(fraction, n):
    """min (ceil ((double) fraction n), n), the fraction a float (trimming's trim_rank)."""
    return min(int(math.ceil(float(np.float32(fraction)) * n)), n)


def candidates(PF, PM, W0):
    geo = geo_of(PF, PM)
    with np.errstate(invalid="ignore"):
        return geo, (np.asarray(W0) != 0) & np.isfinite(geo)


def table(geo):
    """(c, B) of the candidates' geo (float32, finite, non-negative)."""
    j = (np.ascontiguousarray(geo, np.float32).view(np.uint32) >> SHIFT).astype(np.int64)
    return np.bincount(j, minlength=BINS).astype(np.int64), np.bincount(j, weights=geo.astype(np.float64), minlength=BINS)


def run_order_sums(B):
    """S_j: cumulative within each of the 64 runs of 64 bins, then the bases added one after the other."""
    s = np.cumsum(B.reshape(64, 64), axis=1)                # (sequential along a run: s[u, i] = s[u, i - 1] + B[64 u + i])
    base = np.zeros(64)
    for u in range(1, 64):
        base[u] = base[u - 1] + s[u - 1, 63]
    return (base[:, None] + s).reshape(BINS)


def power(r, q):
    """r^q in double by q - 1 successive multiplications ((r r) r ..)."""
    P = r.astype(np.float64)
    for _ in range(q - 1):
        P = P * r.astype(np.float64)
    return P


def select(geo, min_fraction, max_fraction, q):
    """(j*, K, r_lo, r_hi, candidate bins, cost of j*) of the n >= 1 candidates' geo."""
    n = geo.size
    c, B = table(geo)
    r = np.cumsum(c)
    S = run_order_sums(B)
    r_lo, r_hi = rank(min_fraction, n), rank(max_fraction, n)
    j_lo, j_hi = int(np.searchsorted(r, r_lo)), int(np.searchsorted(r, r_hi))       # (the first bin with r_j >= the rank)
    cand = np.nonzero((c > 0) & (np.arange(BINS) >= j_lo) & (np.arange(BINS) <= j_hi))[0]
    cost = S[cand] / power(r[cand], q)
    best = cand[np.lexsort((cand, cost.view(np.uint64)))[0]]              # (the least cost bits, then the least j)
    return int(best), int(r[best]), r_lo, r_hi, int(cand.size), float(S[best] / power(r[best:best + 1], q)[0])


def adaptive_trim_rule(PF, PM, W0, min_fraction, max_fraction, q):
    """(accepted mask, the eight words: ICP_MEM_TRIM's four, then ICP_MEM_TRIM_ADAPTIVE's) of the pairs PF / PM (matched fixed xyz,
    transformed moving xyz per query) with the weights W0 in front of the rule."""
    geo, cand = candidates(PF, PM, W0)
    n = int(np.count_nonzero(cand))
    if n == 0:
        return np.zeros(PF.shape[0], bool), np.zeros(8, np.uint32)
    js, K, r_lo, r_hi, nbins, _ = select(geo[cand], min_fraction, max_fraction, q)
    t = ((js + 1) << SHIFT) - 1
    with np.errstate(invalid="ignore"):
        acc = cand & (np.ascontiguousarray(geo, np.float32).view(np.uint32) <= np.uint32(t))
    assert np.count_nonzero(acc) == K
    return acc, np.array([t, n, K, K, js, r_lo, r_hi, nbins], np.uint32)


def brute_force(PF, PM, W0, min_fraction, max_fraction, q):
    """The rule without a table, in Python floats: (j*, K, r_lo, r_hi, candidate bins, {j: exact B_j}).  The sums over a bin by math.fsum
    (exact, so equal to B_j), the cumulative sums in the rule's run order, the minimum by comparing (cost, j) tuples."""
    geo, cand = candidates(PF, PM, W0)
    g = np.sort(geo[cand])
    n = g.size
    if n == 0:
        return None
    keys = g.view(np.uint32)
    B, c = {}, {}
    for j in sorted(set(int(k) >> SHIFT for k in keys)):
        members = [float(x) for x, k in zip(g, keys) if int(k) >> SHIFT == j]
        B[j], c[j] = math.fsum(members), len(members)
    run_sum = {}                                           # S_j for every bin end
    base, r = 0.0, 0
    ends = []
    for u in range(64):
        s = None
        for i in range(64):
            j = 64 * u + i
            s = B.get(j, 0.0) if i == 0 else s + B.get(j, 0.0)
            r += c.get(j, 0)
            run_sum[j] = (base + s, r)
        base = base + s
    r_lo, r_hi = rank(min_fraction, n), rank(max_fraction, n)
    j_lo = min(j for j in range(BINS) if run_sum[j][1] >= r_lo)
    j_hi = min(j for j in range(BINS) if run_sum[j][1] >= r_hi)
    for j in range(j_lo, j_hi + 1):
        if j in c:
            S, rj = run_sum[j]
            P = float(rj)
            for _ in range(q - 1):
                P = P * float(rj)
            ends.append((S / P, j, rj))
    cost, js, K = min(ends)
    return js, K, r_lo, r_hi, len(ends), B
