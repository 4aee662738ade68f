"""Point-to-plane ICP without a device: argument validation of the C-ABI, the header as C, the C++ facade's and ICPReg's setters,
both command lines, the numpy restatement's solver and grid normals (tests/p2pl_ref.py), and the compiler's resources of the plane
kernels (point-to-plane and colored).  (tests/test_gpu_point_to_plane.py checks the engine against the restatement.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2pl_ref as ref                                     # noqa: E402
from kernel_resources import kernel_resources               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


def test_invalid_arguments_are_refused_with_a_message(L):
    for metric, mu in ((2, 0.0), (-1, 0.0), (1, -0.5), (1, float("nan")), (1, float("inf")), (0, -float("inf"))):
        assert L.icp_set_error_metric(None, metric, mu) == 1, (metric, mu)          # ICP_EINVAL
        assert "icp_set_error_metric" in L.icp_last_error(None).decode()
    assert L.icp_set_error_metric(None, 1, 0.05) == 1
    assert "null handle" in L.icp_last_error(None).decode()
    assert L.icp_set_normals(None, 2, 128) == 1
    assert L.icp_set_normals(None, 1, 0) == 1 and "grid width" in L.icp_last_error(None).decode()
    assert L.icp_set_normals(None, 1, 128) == 1 and "null handle" in L.icp_last_error(None).decode()
    m, w = C.c_int32(), C.c_float()
    assert L.icp_get_error_metric(None, C.byref(m), C.byref(w)) == 1
    s, g = C.c_int32(), C.c_uint32()
    assert L.icp_get_normals(None, C.byref(s), C.byref(g)) == 1
    assert L.icp_batch_set_error_metric(None, 1, 0.0) == 1
    assert L.icp_batch_set_normals(None, 1, 128) == 1


def test_memory_enum(engine):
    assert (engine.Memory.NORMALS_F, engine.Memory.PLANE_SYSTEM) == (21, 22)
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert hdr.index("ICP_MEM_TRIM = 20,") < hdr.index("ICP_MEM_NORMALS_F = 21,") < hdr.index("ICP_MEM_PLANE_SYSTEM = 22,") < hdr.index("ICP_MEM_COUNT_")
    assert engine.ErrorMetric.POINT_TO_PLANE == 1 and engine.Normals.GRID == 1


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b, const float *normals) {\n'
           '    int metric, source; float mu; uint32_t width; double sys[28];\n'
           '    if (icp_set_normals (h, ICP_NORMALS_GRID, 128)) return 1;\n'
           '    if (icp_get_normals (h, &source, &width)) return 1;\n'
           '    if (icp_set_error_metric (h, ICP_METRIC_POINT_TO_PLANE, 0.05f)) return 1;\n'
           '    if (icp_get_error_metric (h, &metric, &mu)) return 1;\n'
           '    if (icp_read (h, ICP_MEM_PLANE_SYSTEM, sys, sizeof sys)) return 1;\n'
           '    if (icp_batch_write (b, 0, ICP_MEM_NORMALS_F, normals)) return 1;\n'
           '    if (icp_batch_set_normals (b, ICP_NORMALS_GIVEN, 0)) return 1;\n'
           '    return icp_batch_set_error_metric (b, ICP_METRIC_POINT_TO_POINT, mu);\n'
           '}\n')
    _compile(tmp_path, "p2pl.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'float f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
           '         ICPStep<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &step,\n'
           '         ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
           '    int metric = 0; float mu = 0.f, mu2 = 0.f;\n'
           '    reg.setNormals (ICP_NORMALS_GRID, 128); reg.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 0.05f);\n'
           '    step.setNormals (ICP_NORMALS_GIVEN); step.setErrorMetric (ICP_METRIC_POINT_TO_PLANE);\n'
           '    app.setNormals (ICP_NORMALS_GRID, 128); app.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 1.f);\n'
           '    reg.getErrorMetric (metric, mu); app.getErrorMetric (metric, mu2);\n'
           '    return mu + mu2 + (float) metric;\n'
           '}\n')
    _compile(tmp_path, "p2pl.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--point-to-plane" in r.stdout
    for bad in ("-0.5", "nan", "inf"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--point-to-plane", bad],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--point-to-plane" in r.stderr, (bad, r.stderr)
    from icp_amd import register
    assert register._point_weight("0.05") == 0.05 and register._point_weight("0") == 0.0


def test_example_command_line_accepts_the_option():
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("-1", "nan", "inf"):
        r = subprocess.run([exe, "--point-to-plane", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--point-to-plane: MU must be finite and >= 0" in r.stderr, (bad, r.stderr)


def test_ldlt_agrees_with_numpy_on_spd_systems():
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = rng.standard_normal((6, 6)) * rng.uniform(0.1, 100.0, 6)
        A = B @ B.T + 1e-3 * np.eye(6)
        b = rng.standard_normal(6)
        s27 = np.concatenate([A[np.triu_indices(6)], b])
        x, ok = ref.ldlt_solve(s27)
        assert ok
        want = np.linalg.solve(A, b)
        assert np.allclose(x, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), (x, want)


def _plane(side, normal=(0.2, -0.3, 0.93), offset=1500.0, jitter=0.0, seed=3):
    """Points of the plane n . X = -offset on a side x side grid (z towards the sensor's far side), row-major."""
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    u = np.cross(n, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    gx, gy = np.meshgrid(np.arange(side) * 10.0 - side * 5.0, np.arange(side) * 10.0 - side * 5.0)
    X = gx[..., None] * u + gy[..., None] * v - offset * n
    F = np.zeros((side * side, 8), np.float32)
    F[:, :3] = X.reshape(-1, 3)
    F[:, 3] = 1.0
    return F, n


def test_exact_plane_without_point_term_is_singular():
    """All pairs on one plane, mu = 0: the three in-plane directions are unconstrained — the rule's identity step."""
    F, n = _plane(32)
    m = F.shape[0]
    N = np.zeros((m, 4), np.float32)
    N[:, :3] = n
    PF = np.zeros((m, 4), np.float32)
    PF[:, :3] = F[:, :3]
    PF[:, 3] = 1.0
    PM = PF.copy()
    PM[:, :3] += np.float32(0.5) * n.astype(np.float32)
    system, T, R, Tk, Rk = ref.step(PF, PM, np.arange(m, dtype=np.uint32), N, 0.0, [0, 0, 0, 1, 0, 0, 0, 1], np.eye(3).ravel())
    assert system[27] == 0.0
    assert np.array_equal(Tk, ref.IDENTITY_TK)
    # with a share of point-to-point the same system is regular
    system, T, R, Tk, Rk = ref.step(PF, PM, np.arange(m, dtype=np.uint32), N, 0.05, [0, 0, 0, 1, 0, 0, 0, 1], np.eye(3).ravel())
    assert system[27] == 1.0


def _exact_plane(side, step=8.0):
    """z = 1000 + x / 4 - y / 2 on an integer grid: every coordinate and every difference exact in float32.  Its unit normal."""
    gx, gy = np.meshgrid((np.arange(side) - side // 2) * step, (np.arange(side) - side // 2) * step)
    F = np.zeros((side * side, 8), np.float32)
    F[:, 0], F[:, 1] = gx.ravel(), gy.ravel()
    F[:, 2] = 1000.0 + F[:, 0] / 4 - F[:, 1] / 2
    F[:, 3] = 1.0
    n = np.array([-0.25, 0.5, 1.0]) / np.linalg.norm([-0.25, 0.5, 1.0])
    return F, n


def test_grid_normals_of_a_tilted_plane():
    side = 48
    F, n = _exact_plane(side)
    N = ref.grid_normals(F, side)
    assert np.isfinite(N).all() and (N[:, 3] == 0).all()
    assert np.allclose(N[:, :3], -n, atol=1e-6), np.abs(N[:, :3] + n).max()     # (-n: the side that faces the origin)
    # facing the sensor at the origin: n . C <= 0 everywhere
    assert ((N[:, :3].astype(np.float64) * F[:, :3]).sum(1) <= 0).all()
    # a hole and a non-finite point: the centres get zero normals, their neighbours fall back to one-sided differences
    G = F.copy()
    G[5 * side + 7, :3] = 0.0
    G[9 * side + 11, 0] = np.nan
    N2 = ref.grid_normals(G, side)
    assert (N2[5 * side + 7] == 0).all() and (N2[9 * side + 11] == 0).all()
    assert np.allclose(np.abs(N2[5 * side + 8, :3] @ n), 1.0, atol=1e-6)
    # a single row has no vertical difference: no normals
    assert (ref.grid_normals(F[:side], side) == 0).all()


def test_plane_kernels_have_zero_scratch():
    """The point-to-plane and colored kernels (one translation unit)."""
    res = dict(kernel_resources("icp_amd/csrc/icp_p2pl.hip"))
    names = sorted(res)
    assert names == ["k_color_grad_grid", "k_normals_grid", "k_p2pl_finalize", "k_plane_moments<false>", "k_plane_moments<true>"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])
