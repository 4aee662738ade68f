"""Median-distance rejection (icp_set_median_rejection, include/icp_amd.h) restated in numpy — TEST INFRASTRUCTURE (a plain module:
pytest collects nothing from it).

Candidates are the pairs with a weight != 0 (W0: what the passes in front have left) and a finite geo; n their number; K = (n + 1) // 2;
t_med the K-th smallest geo (the lower median, an element of the set); thr = (float) ((double) f * (double) f * (double) t_med) with
f the factor as a float; accepted: the candidates with geo <= thr.  The words are ICP_MEM_MEDIAN's: (t_med bits, n, thr bits, accepted)."""
import numpy as np

from icp_checks import geo_of


def threshold(factor, t_med):
    """thr of the rule: float32, the product taken in double in the order written (a value beyond float's range rounds to +inf)."""
    f = np.float32(factor)
    with np.errstate(over="ignore"):
        return np.float32((np.float64(f) * np.float64(f)) * np.float64(np.float32(t_med)))


def median_of(geo):
    """(K, the lower median) of a non-empty array of candidates' geo."""
    K = (geo.size + 1) // 2
    return K, np.sort(geo)[K - 1]


def median_rule(PF, PM, W0, factor):
    """(accepted mask, [t_med bits, n, thr bits, accepted]) of the pairs PF / PM (matched fixed xyz, transformed moving xyz per query)
    with the weights W0 in front of the rule."""
    geo = geo_of(PF, PM)
    cand = (W0 != 0) & np.isfinite(geo)
    n = int(np.count_nonzero(cand))
    if n == 0:
        return np.zeros(PF.shape[0], bool), np.zeros(4, np.uint32)
    _, t = median_of(geo[cand])
    thr = threshold(factor, t)
    acc = cand & (geo <= thr)
    return acc, np.array([np.float32(t).view(np.uint32), n, thr.view(np.uint32), np.count_nonzero(acc)], np.uint32)


def pick_factor(geo, frac):
    """The factor (a float32 value) at which about `frac` of the candidates — geo: their geo, frac < 0.5 — lie above the threshold: thr
    falls half way between two neighbours of the sorted values, so that no rounding of the product decides a pair."""
    s = np.sort(np.asarray(geo, np.float32)).astype(np.float64)
    n = s.size
    _, t = median_of(s)
    assert t > 0, "pick_factor: the median is 0, no factor moves the threshold"
    j = min(max(int(np.ceil((1.0 - frac) * n)) - 1, (n + 1) // 2 - 1), n - 2)
    f = np.float32(np.sqrt(0.5 * (s[j] + s[j + 1]) / t))
    assert f > 0 and np.isfinite(f)
    return float(f)
