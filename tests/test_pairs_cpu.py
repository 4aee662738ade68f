"""The correspondence set (icp_correspondences, include/icp_amd.h) without a GPU: the numpy restatement on hand-made arrays, the record
and the constants as the header, the library and the Python layer spell them, and the compiler's view of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pairs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _pairs(m, seed=7):
    """m pairs a few mm apart, a metre from the origin: every one an inlier without a distance test."""
    rng = np.random.default_rng(seed)
    PF = np.ones((m, 4), F32)
    PF[:, :3] = rng.uniform(500, 1500, (m, 3))
    PM = PF.copy()
    PM[:, :3] += rng.normal(0, 3, (m, 3)).astype(F32)
    M = np.ones((m, 8), F32)
    M[:, :3] = PM[:, :3] - F32(5.0)
    ids = rng.integers(0, m, m).astype(np.uint32)
    return M, PF, PM, ids


def _plain_geo(PF, PM, i):
    g = [F32(PM[i, c]) - F32(PF[i, c]) for c in range(3)]
    return F32(F32(F32(g[0] * g[0]) + F32(g[1] * g[1])) + F32(g[2] * g[2]))


def test_record_layout():
    assert pairs_ref.PAIR.itemsize == 16 and pairs_ref.PAIR.names == ("moving", "fixed", "geo", "weight")
    assert [pairs_ref.PAIR.fields[n][1] for n in pairs_ref.PAIR.names] == [0, 4, 8, 12]


def test_every_pair_a_member_and_the_empty_set():
    m = 700
    M, PF, PM, ids = _pairs(m)
    s = pairs_ref.evaluated(M, PF, PM, ids, 0.0)
    assert s.dtype == pairs_ref.PAIR and len(s) == m
    assert np.array_equal(s["moving"], np.arange(m)) and np.array_equal(s["fixed"], ids) and (s["weight"] == 1).all()
    for i in (0, 255, 256, m - 1):
        assert s["geo"][i].view(np.uint32) == _plain_geo(PF, PM, i).view(np.uint32)
    assert len(pairs_ref.evaluated(M, PF, PM, ids, 1e-6)) == 0                       # (no pair is a micrometre apart)
    assert len(pairs_ref.evaluated(np.zeros_like(M), PF, PM, ids, 0.0)) == 0         # (no moving point counts)
    W = np.zeros(m, F32)
    e = pairs_ref.last_iteration(ids, W, PF, PM)
    assert e.dtype == pairs_ref.PAIR and len(e) == 0
    full = pairs_ref.last_iteration(ids, np.full(m, 0.25, F32), PF, PM)
    assert len(full) == m and np.array_equal(full["geo"].view(np.uint32), s["geo"].view(np.uint32)) and (full["weight"] == F32(0.25)).all()


def test_distance_rule_and_order():
    m = 600
    M, PF, PM, ids = _pairs(m)
    geo = np.array([_plain_geo(PF, PM, i) for i in range(m)], F32)
    md = float(np.sqrt(np.median(geo.astype(np.float64))))
    d2 = F32(np.float64(F32(md)) * np.float64(F32(md)))
    s = pairs_ref.evaluated(M, PF, PM, ids, md)
    want = np.nonzero(geo <= d2)[0]
    assert 0 < want.size < m and np.array_equal(s["moving"], want) and (np.diff(s["moving"].astype(np.int64)) > 0).all()
    assert np.array_equal(s["fixed"], ids[want]) and np.array_equal(s["geo"].view(np.uint32), geo[want].view(np.uint32))


def test_nan_coordinates_are_no_members_of_the_evaluated_set():
    m = 300
    M, PF, PM, ids = _pairs(m)
    M[3, 1] = np.nan                 # a moving point that does not count
    M[4, :3] = 0.0                   # the origin: invalid
    PF[5, :3] = 0.0                  # a fixed point at the origin
    PM[6, 0] = np.nan                # geo is NaN
    PM[7, 2] = np.inf                # geo is inf
    for md in (0.0, 1e6):
        s = pairs_ref.evaluated(M, PF, PM, ids, md)
        assert np.array_equal(s["moving"], np.setdiff1d(np.arange(m), [3, 4, 5, 6, 7])), md
        assert np.isfinite(s["geo"]).all()


def test_weights_nan_is_a_member_and_both_zeros_are_none():
    m = 8
    M, PF, PM, ids = _pairs(m)
    nan = np.array([0x7FC01234], np.uint32).view(F32)[0]                               # (a payload: the bits are kept)
    W = np.array([0.5, 0.0, -0.0, nan, 1.0, np.inf, -1.0, 1e-45], F32)
    PM[3, 0] = np.nan                                                                  # (membership is W's alone: geo may be anything)
    nn_id = np.zeros(m, np.dtype([("dist", F32), ("id", np.uint32)]))
    nn_id["id"] = ids
    s = pairs_ref.last_iteration(nn_id, W, PF, PM)
    assert s["moving"].tolist() == [0, 3, 4, 5, 6, 7]
    assert np.array_equal(s["weight"].view(np.uint32), W[[0, 3, 4, 5, 6, 7]].view(np.uint32))
    assert np.isnan(s["geo"][1]) and np.array_equal(s["fixed"], ids[[0, 3, 4, 5, 6, 7]])
    assert pairs_ref.last_iteration(ids, W, PF, PM).tobytes() == s.tobytes()


def test_python_record_matches_the_header(engine):
    """ctypes.sizeof of the Python record is 16 and its field offsets are the header's, through the C compiler; the constants agree."""
    P = engine._Pair
    assert C.sizeof(P) == 16 and (P.moving.offset, P.fixed.offset, P.geo.offset, P.weight.offset) == (0, 4, 8, 12)
    assert engine.PAIR == pairs_ref.PAIR and engine.PAIR.itemsize == C.sizeof(P)
    code = ('#include <stddef.h>\n#include "icp_amd.h"\n'
            '_Static_assert (sizeof (icp_pair_t) == 16, "size");\n'
            '_Static_assert (offsetof (icp_pair_t, moving) == 0 && offsetof (icp_pair_t, fixed) == 4 && offsetof (icp_pair_t, geo) == 8 '
            '&& offsetof (icp_pair_t, weight) == 12, "layout");\n'
            '_Static_assert (ICP_PAIRS_EVALUATED == %d && ICP_PAIRS_LAST_ITERATION == %d, "constants");\n'
            "int main (void) { return 0; }\n" % (engine.Pairs.EVALUATED, engine.Pairs.LAST_ITERATION))
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icp_amd.h")).read(), flags=re.S)
    consts = dict(re.findall(r"#define\s+(ICP_PAIRS_\w+)\s+(\d+)", hdr))
    assert consts == {"ICP_PAIRS_EVALUATED": str(engine.Pairs.EVALUATED), "ICP_PAIRS_LAST_ITERATION": str(engine.Pairs.LAST_ITERATION)}


def test_library_exports_the_interface(engine):
    L = engine.lib()
    n = C.c_uint32()
    for name in ("icp_correspondences", "icp_correspondences_read", "icp_correspondences_device_ptr", "icp_batch_correspondences"):
        assert hasattr(L, name), name
    assert L.icp_correspondences(None, 0, 0.0, C.byref(n), 1) == 1                    # ICP_EINVAL: no handle
    assert L.icp_correspondences_read(None, 0, None, 0, C.byref(n)) == 1
    assert L.icp_correspondences_device_ptr(None, 0, None, None) == 1
    assert L.icp_batch_correspondences(None, 0, 0, 0.0, None, 0, C.byref(n)) == 1
    assert callable(engine.ICPStep.correspondences) and callable(engine.ICPBatch.correspondences)
    assert engine._PyramidLevel.correspondences is engine.ICPStep.correspondences     # (pyramid levels inherit it)


def test_pairs_kernels_use_no_scratch():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_pairs.hip")
    assert sorted(res) == ["k_pairs_count<0>", "k_pairs_count<1>", "k_pairs_scatter<0>", "k_pairs_scatter<1>"], sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False"), (n, r)


def test_command_line_has_the_option():
    import sys
    out = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--pairs FILE" in out.stdout, out.stdout[-2000:]
