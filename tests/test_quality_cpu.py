"""Registration quality (icp_evaluate, include/icp_amd.h) without a GPU: the numpy restatement against an independent float64
statement, the interface as the header declares it and the library exports it, and the compiler's view of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import quality_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_pairs(seed, m):
    """Pairs as a depth camera sees them (mm): fixed points in a frustum 1 - 2 m away, the transformed moving points a few mm off;
    some moving points invalid (the origin, a NaN, an infinity), some fixed points at the origin, some pairs far apart."""
    rng = np.random.default_rng(seed)
    PF = np.ones((m, 4), np.float32)
    PF[:, 0] = rng.uniform(-600, 600, m)
    PF[:, 1] = rng.uniform(-450, 450, m)
    PF[:, 2] = rng.uniform(1000, 2000, m)
    PM = PF.copy()
    PM[:, :3] += rng.normal(0, 4, (m, 3)).astype(np.float32)
    far = rng.choice(m, m // 10, replace=False)
    PM[far, :3] += rng.normal(0, 60, (far.size, 3)).astype(np.float32)
    M = np.ones((m, 8), np.float32)
    M[:, :3] = PM[:, :3] + np.float32(7.0)
    bad = rng.choice(m, 60, replace=False)
    M[bad[:20], :3] = 0.0
    M[bad[20:30], 0] = np.nan
    M[bad[30:40], 2] = np.inf
    PF[bad[40:60], :3] = 0.0
    return M, PF, PM


def test_restatement_against_an_independent_float64_statement():
    """quality_ref (float32 geo, float64 terms, the explicit halving trees) against Open3D's three G rows per pair, G^T G and geo summed
    with math.fsum: every entry within 1e-12 relative, the counts equal — at a size below one block, at one that is no multiple of
    256 and at several blocks, with and without the distance test."""
    for seed, m in ((1, 200), (2, 2500), (3, 4096)):
        M, PF, PM = _random_pairs(seed, m)
        for max_dist in (0.0, 9.0):
            q = quality_ref.evaluate(M, PF, PM, max_dist)
            counted, inlier, geo = quality_ref.masks(M, PF, PM, max_dist)
            # the masks, stated once more in plain Python
            on, d2 = quality_ref.threshold(max_dist)
            n_moving = n_inliers = 0
            for i in range(m):
                mv, f = M[i, :3], PF[i, :3]
                c = bool(np.isfinite(mv).all() and (mv != 0).any())
                n_moving += c
                n_inliers += bool(c and (f != 0).any() and np.isfinite(geo[i]) and (not on or geo[i] <= d2))
            assert (q.n_moving, q.n_inliers) == (n_moving, n_inliers)
            assert 0 < q.n_inliers < q.n_moving < m
            A, sum_geo = quality_ref.independent(PF, inlier, geo)
            err = np.abs(q.information - A)
            assert (err <= 1e-12 * np.abs(A)).all(), (seed, m, max_dist, err.max())
            assert abs(q.sums[21] - sum_geo) <= 1e-12 * sum_geo
            assert np.array_equal(q.information, q.information.T) and not np.isnan(q.sums).any()
            assert q.fitness == n_inliers / n_moving and q.inlier_rmse == float(np.sqrt(q.sums[21] / n_inliers))


def test_threshold_is_the_rounded_double_product():
    assert quality_ref.threshold(0.0) == (False, 0) and quality_ref.threshold(float("inf"))[0] is False and quality_ref.threshold(None)[0] is False
    on, d2 = quality_ref.threshold(0.1)
    md = np.float32(0.1)
    assert on and d2.dtype == np.float32 and d2 == np.float32(np.float64(md) * np.float64(md))


def test_header_declares_and_library_exports_the_interface(engine):
    """Fails without the feature: the header declares icp_evaluate, icp_batch_evaluate and icp_quality_t, the library exports both."""
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+icp_evaluate\s*\(\s*icp_handle\s+\w+\s*,\s*float\s+\w+\s*,\s*icp_quality_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+icp_batch_evaluate\s*\(\s*icp_batch_handle\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s+\w+\s*,\s*icp_quality_t\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"\}\s*icp_quality_t\s*;", code)
    L = engine.lib()
    assert hasattr(L, "icp_evaluate") and hasattr(L, "icp_batch_evaluate")
    assert L.icp_evaluate(None, 0.0, None, 1) == 1 and L.icp_batch_evaluate(None, 0, 0.0, None) == 1      # ICP_EINVAL: no handle


def test_quality_record_is_39_doubles_and_4_words(engine):
    """sizeof (icp_quality_t) is 39 doubles + 4 uint32 with no padding, through ctypes and through the C compiler.  That is 328 bytes:
    the issue that asked for the record wrote "336 bytes: 39 doubles + 4 uint32", and 39 * 8 + 4 * 4 is 328 for the struct it spells
    out — the struct and the count of its members are kept, the sum is corrected."""
    assert C.sizeof(engine.Quality) == 39 * 8 + 4 * 4 == 328
    assert engine.Quality.information.offset == 24 and engine.Quality.n.offset == 312 and engine.Quality.reserved.offset == 324
    code = ('#include <stddef.h>\n#include "icp_amd.h"\n'
            "_Static_assert (sizeof (icp_quality_t) == 39 * sizeof (double) + 4 * sizeof (uint32_t) && sizeof (icp_quality_t) == 328, \"size\");\n"
            "_Static_assert (offsetof (icp_quality_t, information) == 24 && offsetof (icp_quality_t, n) == 312, \"layout\");\n"
            "int main (void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_quality_kernels_use_no_scratch():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_quality.hip")
    assert sorted(res) == ["k_quality_finish", "k_quality_pairs"], sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False"), (n, r)
        assert r["lds"] <= 64 * 1024, (n, r)


def test_register_functions_keep_one_shape_each():
    """register_clouds returns its four values as before; register_and_evaluate takes the same options and returns five."""
    import inspect
    from icp_amd import register
    opts = inspect.signature(register.register_clouds).parameters
    assert "evaluate" not in opts and opts["max_dist"].default is None
    # the two functions around it take exactly register_clouds' options, by name and with its defaults, behind fixed, moving, evaluate
    import facade_record
    import pytest
    names = list(opts)[2:]
    for f in (register.register_and_evaluate, register.register_with_pairs):
        assert list(inspect.signature(f).parameters)[:3] == ["fixed", "moving", "evaluate"]
        with facade_record.stand_ins(register) as (log, _):
            plain = f("F", "M", 1.0)
            assert len(plain) == (5 if f is register.register_and_evaluate else 6) and len(register.register_clouds("F", "M")) == 4
            for name in names:
                with pytest.raises(TypeError):
                    f("F", "M", 1.0, **{name + "_": opts[name].default})
                del log[:]
                assert len(f("F", "M", 1.0, **{name: opts[name].default})) == len(plain)
                explicit = list(log)
                del log[:]
                f("F", "M", 1.0)
                assert explicit == log, name                   # (the default, given by name, is what is taken without it)
