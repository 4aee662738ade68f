"""One-to-one correspondences (icp_set_unique, include/icp_amd.h) restated in numpy: of the candidate pairs that share a fixed point
only the one with the smallest key (bits (geo) << 32 | query index) keeps its weight.

Works from the engine's own NN_ID / NN / QT outputs and the weights before the rule (tests/test_gpu_trimming.py's
weights_before_trim)."""
import numpy as np

F32 = np.float32
FREE = np.uint64(0xFFFFFFFFFFFFFFFF)


def geo(PF, PM):
    """The rejection rule's geo in fp32: (ex - f0)^2 + (ey - f1)^2 + (ez - f2)^2, summed in that order."""
    g = (np.asarray(PM, F32)[:, :3] - np.asarray(PF, F32)[:, :3]).astype(F32)
    return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def keys_of(g):
    """The 64-bit claim keys of the pairs whose geo (fp32) is g: bits (geo) << 32 | query index."""
    g = np.ascontiguousarray(g, F32)
    return (g.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(g.shape[0], dtype=np.uint64)


def unique_from_keys(ids, g, cand, nfixed=None):
    """(winner mask, [n, winners]) from the ids, geo and candidate mask of the pairs: np.minimum.at on the keys."""
    ids = np.asarray(ids, np.int64)
    cand = np.asarray(cand, bool)
    key = keys_of(g)
    table = np.full(int(nfixed if nfixed is not None else ids.shape[0]), FREE, np.uint64)
    np.minimum.at(table, ids[cand], key[cand])
    win = np.zeros(ids.shape[0], bool)
    win[cand] = table[ids[cand]] == key[cand]
    return win, np.array([np.count_nonzero(cand), np.count_nonzero(win)], np.uint32)


def unique_rule(ids, PF, PM, W0):
    """(winner mask, candidate mask, [n, winners]).  Candidates: weight != 0 (W0: after rejection, before the rule) and a finite geo."""
    g = geo(PF, PM)
    with np.errstate(invalid="ignore"):
        cand = (np.asarray(W0, F32) != 0) & np.isfinite(g)
    win, counts = unique_from_keys(ids, g, cand)
    return win, cand, counts


def weights_after(W0, win, cand):
    """The weights behind the rule: a loser's is +0, every other pair's stays."""
    W = np.array(W0, F32, copy=True)
    W[cand & ~win] = 0.0
    return W
