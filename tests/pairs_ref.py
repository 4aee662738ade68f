"""The correspondence set restated in numpy (the rule of include/icp_amd.h: icp_correspondences) — TEST INFRASTRUCTURE, collects nothing.

A set is a structured array of PAIR records (moving, fixed, geo, weight), one per member pair in ascending moving index:
  - evaluated: the members are quality_ref.masks' inliers (icp_evaluate's rule), fixed the search's id, weight 1;
  - last_iteration: the members are the pairs with W != 0 as float32 compares (a NaN weight is a member, -0 and +0 are none), fixed the
    iteration's id, weight W itself, bit for bit;
geo is quality_ref.geo_of in both: float32, (gx gx + gy gy) + gz gz."""
import numpy as np

import quality_ref

PAIR = np.dtype([("moving", "<u4"), ("fixed", "<u4"), ("geo", "<f4"), ("weight", "<f4")])


def check_set(got, want, what):
    """A device's set against an expectation: the dtype, the count, then the records by their raw bytes."""
    print(what, "device", len(got), "reference", len(want))
    assert got.dtype == PAIR, (what, got.dtype)
    assert len(got) == len(want), "%s: %d records, the reference has %d" % (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        a, b = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
        bad = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError("%s: %d of %d records differ, first at %d: got %r want %r" % (what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]]))


def _set(member, ids, geo, weight):
    idx = np.nonzero(member)[0]
    out = np.zeros(idx.size, PAIR)
    out["moving"] = idx
    out["fixed"] = np.asarray(ids, np.uint32)[idx]
    out["geo"] = np.asarray(geo, np.float32)[idx]
    out["weight"].view(np.uint32)[...] = np.ascontiguousarray(weight, np.float32).view(np.uint32)[idx]     # (a NaN's payload as it is)
    return out


def evaluated(M, PF, PM, ids, max_dist):
    """The ICP_PAIRS_EVALUATED set: M the moving set as written (m x 8), PF / PM the search's fixed / transformed moving points, ids its
    fixed indices."""
    _, inlier, geo = quality_ref.masks(M, PF, PM, max_dist)
    return _set(inlier, ids, geo, np.ones(len(geo), np.float32))


def last_iteration(nn_id, W, PF, PM):
    """The ICP_PAIRS_LAST_ITERATION set from the four per-query outputs: nn_id (its "id" field, or plain indices), W, NN and QT."""
    ids = nn_id["id"] if getattr(nn_id, "dtype", None) is not None and nn_id.dtype.names else nn_id
    W = np.ascontiguousarray(W, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        member = W != np.float32(0)
    return _set(member, ids, quality_ref.geo_of(PF, PM), W)
