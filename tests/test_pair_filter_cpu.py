"""Boundary and normal rejection without a device: the numpy restatement of tests/pair_filter_ref.py on hand-made cases, the header, the
Python mirror, argument validation on no handle, the command line's argument checks and the compiler's resources of the new kernel.
(tests/test_gpu_pair_filter.py checks what the settings do.)"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_filter_ref as ref                                   # noqa: E402
from kernel_resources import kernel_resources                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3 = np.eye(3, dtype=np.float32)


# ---- the boundary rule

def _grid(rows, gw):
    F = np.zeros((rows * gw, 8), np.float32)
    F[:, 0] = np.tile(np.arange(gw), rows) + 1.0
    F[:, 1] = np.repeat(np.arange(rows), gw) + 1.0
    F[:, 2] = 500.0
    return F


def test_a_complete_4x4_grid_has_four_interior_points():
    b = ref.boundary_mask(_grid(4, 4), 4)
    assert np.flatnonzero(~b).tolist() == [5, 6, 9, 10]


@pytest.mark.parametrize("hole,how", [(0, "zero"), (3, "nan"), (5, "zero"), (5, "inf"), (7, "zero"), (10, "nan"), (15, "zero")])
def test_4x4_grid_with_one_hole(hole, how):
    """The interior ids 5, 6, 9, 10 stay interior unless the hole is one of them or one of their 8 neighbours."""
    F = _grid(4, 4)
    F[hole, :3] = 0.0 if how == "zero" else (np.nan if how == "nan" else np.inf)
    if how != "zero":
        F[hole, 1] = 1.0                                 # (one non-finite coordinate is enough)
    b = ref.boundary_mask(F, 4)
    hx, hy = hole % 4, hole // 4
    want = [i for i in (5, 6, 9, 10) if max(abs(i % 4 - hx), abs(i // 4 - hy)) > 1]
    assert np.flatnonzero(~b).tolist() == want
    assert b[hole]


def test_a_point_at_the_origin_with_a_colour_is_a_hole_and_a_wide_grid_has_more_rows_than_columns():
    F = _grid(5, 3)                                       # 3 wide, 5 rows: interior ids 4, 7, 10
    assert np.flatnonzero(~ref.boundary_mask(F, 3)).tolist() == [4, 7, 10]
    F[7, :3] = 0.0; F[7, 4:7] = 0.5
    assert ref.boundary_mask(F, 3).all()
    assert np.flatnonzero(~ref.boundary_mask(_grid(3, 5), 5)).tolist() == [6, 7, 8]


def test_a_depth_jump_between_valid_neighbours_is_no_boundary():
    F = _grid(4, 4)
    F[6, 2] = 5000.0
    assert np.flatnonzero(~ref.boundary_mask(F, 4)).tolist() == [5, 6, 9, 10]


# ---- the normal rule

def test_comparison_at_its_edge():
    """o equal to, one ulp below and one ulp above c sqrt (qq pp), in float64."""
    qq, pp = np.float64(2.0), np.float64(2.0)
    c = np.float32(0.5)
    thr = np.float64(c) * np.sqrt(qq * pp)
    o = np.array([thr, np.nextafter(thr, -np.inf), np.nextafter(thr, np.inf)])
    assert ref.compatible_from_terms(np.full(3, qq), np.full(3, pp), o, c).tolist() == [True, False, True]
    # the same edge from float32 normals: (1, 1, 0) against (1, 0, 1) is 60 degrees, o = 1 = 0.5 sqrt (2 * 2) exactly
    NQ = np.array([[1, 1, 0, 0]] * 3, np.float32)
    NM = np.array([[1, 0, 1, 0], [np.nextafter(np.float32(1), np.float32(0)), 0, 1, 0], [np.nextafter(np.float32(1), np.float32(2)), 0, 1, 0]], np.float32)
    qq, pp, o = ref.cosine_terms(NQ, NM, I3)
    assert o[0] == 0.5 * math.sqrt(qq[0] * pp[0]) and o[1] < 0.5 * math.sqrt(qq[1] * pp[1]) and o[2] > 0.5 * math.sqrt(qq[2] * pp[2])
    assert ref.compatible(NQ, NM, I3, 0.5).tolist() == [True, False, True]


def test_min_cos_is_read_as_a_float():
    """(double) min_cos: 0.8 as the float it is stored as, above 0.8 — a 3-4-5 pair, cosine exactly 0.8, is incompatible."""
    NQ = np.array([[1, 0, 0, 0]], np.float32); NM = np.array([[4, 3, 0, 0]], np.float32)
    assert np.float64(np.float32(0.8)) > 0.8
    assert not ref.compatible(NQ, NM, I3, 0.8)[0]
    assert ref.compatible(NQ, NM, I3, np.nextafter(np.float32(0.8), np.float32(0)))[0]


def test_zero_and_non_finite_normals_are_rejected():
    good = [0, 0, 1, 0]
    NQ = np.array([good, [0, 0, 0, 0], good, [np.nan, 0, 1, 0], good, [np.inf, 0, 0, 0], good], np.float32)
    NM = np.array([good, good, [0, 0, 0, 0], good, [0, np.nan, 1, 0], good, [0, 0, -np.inf, 0]], np.float32)
    for c in (-1.0, 0.0, 1.0):
        assert ref.compatible(NQ, NM, I3, c).tolist() == [True] + [False] * 6, c


def test_min_cos_minus_one_accepts_every_pair_with_both_normals_and_one_only_parallel_ones():
    rng = np.random.default_rng(5)
    NQ = rng.normal(size=(200, 4)).astype(np.float32); NM = rng.normal(size=(200, 4)).astype(np.float32)
    NM[:20, :3] = -NQ[:20, :3]                           # opposite: cosine -1 up to rounding
    NM[20:40, :3] = NQ[20:40, :3]
    NM[40, :3] = 0
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    got = ref.compatible(NQ, NM, I3, -1.0)
    assert got[41:].all() and got[20:40].all() and not got[40]
    axis = np.zeros((3, 4), np.float32); axis[0, 0] = axis[1, 1] = axis[2, 2] = 2.0     # (exact: opposite axis vectors pass -1)
    assert ref.compatible(axis, -axis, I3, -1.0).all() and not ref.compatible(axis, -axis, I3, np.float32(-0.999)).any()
    assert ref.compatible(axis, axis, I3, 1.0).all()
    assert not ref.compatible(axis, axis[[1, 2, 0]], I3, 1.0).any()
    # R acts on the moving normal: x -> y
    assert ref.compatible(axis[[1]], axis[[0]], R, 1.0)[0] and not ref.compatible(axis[[0]], axis[[0]], R, 1.0)[0]


def test_counts_boundary_first_and_every_pair_once():
    F = _grid(4, 4)
    F[15, :3] = 0.0                                       # interior 10 becomes boundary
    ids = np.array([5, 5, 6, 9, 10, 0, 3, 16, 5], np.uint32)      # (16: no index into F — no candidate)
    W0 = np.array([1, 0, 1, 1, 1, 1, 1, 1, 0.5], np.float32)
    NF = np.zeros((16, 4), np.float32); NF[:, 2] = 1.0; NF[6, :3] = 0.0
    NM = np.zeros((9, 4), np.float32); NM[:, 2] = 1.0; NM[3, :3] = (1, 0, 0); NM[5, 2] = -1.0
    bnd, inc, acc, counts = ref.pair_filter(ids, W0, F, 4, NF, NM, I3, 0.5)
    assert bnd.tolist() == [False, False, False, False, True, True, True, False, False]
    assert inc.tolist() == [False, False, True, True, False, False, False, False, False]      # (pair 5 is incompatible too: counted as boundary)
    assert acc.tolist() == [True, False, False, False, False, False, False, False, True]
    assert counts.tolist() == [7, 3, 2, 2] and counts[0] == counts[1:].sum()
    assert ref.pair_filter(ids, W0, F, 4)[3].tolist() == [7, 3, 0, 4]
    assert ref.pair_filter(ids, W0, normals_f=NF, normals_m=NM, R=I3, min_cos=0.5)[3].tolist() == [7, 0, 3, 4]
    assert ref.pair_filter(ids, W0, F)[3].tolist() == [7, 0, 0, 7]


# ---- the interface

def test_header():
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert hdr.index("ICP_MEM_UNIQUE = 25,") < hdr.index("ICP_MEM_PAIR_FILTER = 26,") < hdr.index("ICP_MEM_COUNT_")
    for decl in ("int icp_set_normal_rejection (icp_handle h, int on, float min_cos);",
                 "int icp_get_normal_rejection (icp_handle h, int *on, float *min_cos);",
                 "int icp_set_boundary_rejection (icp_handle h, uint32_t grid_width);",
                 "int icp_get_boundary_rejection (icp_handle h, uint32_t *grid_width);",
                 "int icp_batch_set_normal_rejection (icp_batch_handle b, int on, float min_cos);",
                 "int icp_batch_set_boundary_rejection (icp_batch_handle b, uint32_t grid_width);"):
        assert decl in hdr, decl


def test_python_mirror(engine):
    assert engine.Memory.PAIR_FILTER == 26
    assert engine._MEM_DTYPE[engine.Memory.PAIR_FILTER] == (np.uint32, None)
    for cls in (engine.ICPStep, engine.ICPBatch):
        for name in ("set_normal_rejection", "normal_rejection", "set_boundary_rejection", "boundary_rejection"):
            assert callable(getattr(cls, name)), name


def test_arguments_on_no_handle(engine):
    L = engine.lib()
    for on in (2, -1):
        assert L.icp_set_normal_rejection(None, on, 0.5) == 1                 # ICP_EINVAL
        assert "0 or 1" in L.icp_last_error(None).decode()
    for c in (float("nan"), 1.5, -1.0000001, float("inf")):
        assert L.icp_set_normal_rejection(None, 1, c) == 1
        assert "[-1, 1]" in L.icp_last_error(None).decode(), c
    assert L.icp_set_normal_rejection(None, 1, 0.5) == 1 and "null handle" in L.icp_last_error(None).decode()
    assert L.icp_set_boundary_rejection(None, 128) == 1 and "null handle" in L.icp_last_error(None).decode()
    on, c, w = C.c_int32(), C.c_float(), C.c_uint32()
    assert L.icp_get_normal_rejection(None, C.byref(on), C.byref(c)) == 1
    assert L.icp_get_boundary_rejection(None, C.byref(w)) == 1
    assert L.icp_batch_set_normal_rejection(None, 1, 0.5) == 1 and L.icp_batch_set_boundary_rejection(None, 128) == 1


def test_header_compiles_as_c_and_the_facades_expose_the_settings(tmp_path):
    c = tmp_path / "pair_filter.c"
    c.write_text('#include "icp_amd.h"\n'
                 'int f (icp_handle h, icp_batch_handle b) {\n'
                 '    int on; float c; uint32_t w, u[4];\n'
                 '    if (icp_set_normal_rejection (h, 1, 0.5f) || icp_get_normal_rejection (h, &on, &c)) return 1;\n'
                 '    if (icp_set_boundary_rejection (h, 128u) || icp_get_boundary_rejection (h, &w)) return 1;\n'
                 '    if (icp_read (h, ICP_MEM_PAIR_FILTER, u, sizeof u)) return 1;\n'
                 '    return icp_batch_set_normal_rejection (b, on, c) || icp_batch_set_boundary_rejection (b, w);\n'
                 '}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude", str(c)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "pair_filter.cpp"
    cpp.write_text('#include <ocl_icp_reg.hpp>\n'
                   'using namespace cl_algo::ICP;\n'
                   'bool f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
                   '        ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
                   '    float c = 0.f;\n'
                   '    reg.setNormalRejection (true, 0.5f); reg.setBoundaryRejection (128); app.setNormalRejection (false); app.setBoundaryRejection (0);\n'
                   '    return reg.getNormalRejection (&c) || reg.getBoundaryRejection () != 0u;\n'
                   '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude", str(cpp)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_register_command_line_checks_its_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "icp_amd.register", *a], capture_output=True, text=True, cwd=ROOT)
    r = run("--help")
    assert r.returncode == 0 and "--normal-angle" in r.stdout and "--reject-boundary" in r.stdout, r.stderr
    for bad in ("-1", "180.5", "nan", "wide"):
        r = run("--normal-angle", bad, "a.bin", "b.bin")
        assert r.returncode == 2 and "--normal-angle" in r.stderr, (bad, r.stderr)
    r = run("--reject-boundary", "yes", "a.bin", "b.bin", "c.bin")           # (a flag: it takes no value)
    assert r.returncode == 2
    from icp_amd.register import normal_cosine
    assert normal_cosine(0) == 1.0 and normal_cosine(180) == -1.0 and abs(normal_cosine(60) - 0.5) < 1e-15
    assert abs(normal_cosine(90)) < 1e-16


def test_the_kernel_has_zero_scratch():
    res = dict(kernel_resources("icp_amd/csrc/icp_pair_filter.hip"))
    assert sorted(res) == ["k_pair_filter"], sorted(res)
    assert res["k_pair_filter"]["scratch"] == 0 and res["k_pair_filter"]["dynamic_stack"] == "False", res
