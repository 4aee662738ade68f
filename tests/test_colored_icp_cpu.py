"""Colored ICP without a device: argument validation of the C-ABI, the enum values, the header as C, the C++ facade's and ICPReg's
setters, both command lines, and two independent checks of the numpy restatement (tests/colored_ref.py): grid gradients of a linear
intensity ramp on a tilted plane, and J_C against a finite difference of r_C.  (tests/test_gpu_colored_icp.py checks the engine
against the restatement; tests/test_point_to_plane_cpu.py checks the compiler's resources of the plane kernels, colored ones included.)"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_ref as cref                                 # noqa: E402
import p2pl_ref as ref                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


def test_invalid_arguments_are_refused_with_a_message(L):
    for kappa in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert L.icp_set_color_weight(None, kappa) == 1, kappa                      # ICP_EINVAL
        assert "icp_set_color_weight: kappa must be finite and >= 0" in L.icp_last_error(None).decode()
        assert L.icp_batch_set_color_weight(None, kappa) == 1
    assert L.icp_set_color_weight(None, 100.0) == 1
    assert "icp_set_color_weight: null handle" in L.icp_last_error(None).decode()
    k = C.c_float()
    assert L.icp_get_color_weight(None, C.byref(k)) == 1
    assert L.icp_batch_set_color_weight(None, 100.0) == 1
    # the metric value is known now; a null handle is still refused by name, and 3 is unknown
    assert L.icp_set_error_metric(None, 2, 0.0) == 1
    assert "icp_set_error_metric: null handle" in L.icp_last_error(None).decode()
    assert L.icp_set_error_metric(None, 3, 0.0) == 1
    assert "icp_set_error_metric: unknown metric" in L.icp_last_error(None).decode()
    assert L.icp_set_error_metric(None, 2, -1.0) == 1
    assert "point_weight" in L.icp_last_error(None).decode()
    assert L.icp_batch_set_error_metric(None, 2, 0.0) == 1


def test_enum_values(engine):
    assert engine.ErrorMetric.COLORED == 2
    assert (engine.Memory.PLANE_SYSTEM, engine.Memory.COLOR_GRAD_F) == (22, 23)
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert hdr.index("ICP_MEM_PLANE_SYSTEM = 22,") < hdr.index("ICP_MEM_COLOR_GRAD_F = 23,") < hdr.index("ICP_MEM_COUNT_")
    assert "#define ICP_METRIC_COLORED 2" in hdr
    from icp_amd import _write_floats
    assert _write_floats(engine.Memory.COLOR_GRAD_F, 100) == 400


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b, const float *grads) {\n'
           '    float kappa; float g[4 * 16];\n'
           '    if (icp_set_color_weight (h, 1000.f)) return 1;\n'
           '    if (icp_get_color_weight (h, &kappa)) return 1;\n'
           '    if (icp_set_error_metric (h, ICP_METRIC_COLORED, 0.05f)) return 1;\n'
           '    if (icp_write (h, ICP_MEM_COLOR_GRAD_F, grads, 1)) return 1;\n'
           '    if (icp_read (h, ICP_MEM_COLOR_GRAD_F, g, sizeof g)) return 1;\n'
           '    if (icp_batch_write (b, 0, ICP_MEM_COLOR_GRAD_F, grads)) return 1;\n'
           '    if (icp_batch_set_error_metric (b, ICP_METRIC_COLORED, 0.f)) return 1;\n'
           '    return icp_batch_set_color_weight (b, kappa);\n'
           '}\n')
    _compile(tmp_path, "colored.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'float f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
           '         ICPStep<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &step,\n'
           '         ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
           '    static_assert (icp::ErrorMetric::COLORED == ICP_METRIC_COLORED, "metric value");\n'
           '    static_assert (icp::ErrorMetric::POINT_TO_PLANE == 1 && icp::ErrorMetric::POINT_TO_POINT == 0, "metric values");\n'
           '    reg.setNormals (ICP_NORMALS_GRID, 128); reg.setColorWeight (1000.f); reg.setErrorMetric (icp::ErrorMetric::COLORED, 0.05f);\n'
           '    step.setNormals (ICP_NORMALS_GIVEN); step.setColorWeight (10.f); step.setErrorMetric (ICP_METRIC_COLORED);\n'
           '    app.setNormals (ICP_NORMALS_GRID, 128); app.setColorWeight (100.f); app.setErrorMetric (ICP_METRIC_COLORED, 1.f);\n'
           '    return reg.getColorWeight () + step.getColorWeight () + app.getColorWeight ();\n'
           '}\n')
    _compile(tmp_path, "colored.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--colored" in r.stdout and "KAPPA" in r.stdout
    for bad in ("-0.5", "nan", "inf"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--colored", bad],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--colored" in r.stderr, (bad, r.stderr)
    import inspect
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["colored"].default is None


def test_example_command_line_accepts_the_option():
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("-1", "nan", "inf"):
        r = subprocess.run([exe, "--colored", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--colored: KAPPA must be finite and >= 0" in r.stderr, (bad, r.stderr)


# ---- (a) grid gradients of a linear intensity ramp on a tilted plane

def _ramp_plane(side, step=8.0, g=(1 / 64, 1 / 128, 1 / 32)):
    """z = 1000 + x / 4 - y / 2 on an integer grid (every coordinate exact in float32) with the intensity C = g . (x, y, z - 1000),
    dyadic and exact in float32 (r = g = b = C, so ((r + g) + b) / 3 = C exactly).  The plane's unit normal and the ramp's in-plane
    gradient."""
    gx, gy = np.meshgrid((np.arange(side) - side // 2) * step, (np.arange(side) - side // 2) * step)
    F = np.zeros((side * side, 8), np.float32)
    F[:, 0], F[:, 1] = gx.ravel(), gy.ravel()
    F[:, 2] = 1000.0 + F[:, 0] / 4 - F[:, 1] / 2
    F[:, 3] = 1.0
    g = np.asarray(g, np.float64)
    Cv = F[:, 0] * g[0] + F[:, 1] * g[1] + (F[:, 2] - 1000.0) * g[2]
    F[:, 4:7] = Cv[:, None]
    F[:, 7] = 1.0
    n = np.array([-0.25, 0.5, 1.0]) / np.linalg.norm([-0.25, 0.5, 1.0])
    return F, n, g - (g @ n) * n


def test_grid_gradients_of_a_linear_ramp_on_a_tilted_plane():
    side = 24
    F, n, want = _ramp_plane(side)
    assert np.array_equal(cref.intensity(F), F[:, 4])
    N = ref.grid_normals(F, side)
    G = cref.grid_gradients(F, N, side)
    assert np.array_equal(G[:, 3], F[:, 4])                     # .w = C(p)
    # every point of the full grid has at least 3 valid neighbours (a corner has 3): every gradient is the ramp's
    err = np.abs(G[:, :3].astype(np.float64) - want).max(1) / np.linalg.norm(want)
    assert err.max() < 1e-6, err.max()
    assert np.abs(G[:, :3].astype(np.float64) @ n).max() < 1e-6 * np.linalg.norm(want)
    # holes: an invalid centre gets zeros (C kept); a point left with fewer than 3 valid neighbours gets zeros; the rest is the ramp
    H = F.copy()
    H[5 * side + 7, :3] = 0.0
    H[0 * side + 1, :3] = 0.0
    H[1 * side + 0, :3] = np.nan                                 # (the corner (0, 0) keeps one neighbour, (1, 1))
    N2 = ref.grid_normals(H, side)
    G2 = cref.grid_gradients(H, N2, side)
    assert (G2[5 * side + 7, :3] == 0).all() and G2[5 * side + 7, 3] == H[5 * side + 7, 4]
    assert (G2[0, :3] == 0).all()
    ok = (N2[:, :3] != 0).any(1) & (G2[:, :3] != 0).any(1)
    assert ok.sum() > side * side - 20
    err = np.abs(G2[ok, :3].astype(np.float64) - want).max(1) / np.linalg.norm(want)
    assert err.max() < 1e-6, err.max()
    # a zero normal: no gradient
    N3 = N.copy()
    N3[3 * side + 3] = 0.0
    assert (cref.grid_gradients(F, N3, side)[3 * side + 3, :3] == 0).all()


# ---- (b) J_C against a central finite difference of r_C

def _rodrigues(w):
    th = math.sqrt(sum(v * v for v in w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def test_photometric_jacobian_matches_a_finite_difference_of_the_residual():
    """J_C x = r_C is the photometric match after the step x = (omega, tau): moving P by x changes r_C by -J_C x to first order."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        P = rng.uniform(-500, 500, 3) + np.array([0, 0, 1500.0])
        Q = P + rng.uniform(-20, 20, 3)
        N = rng.standard_normal(3)
        N /= np.linalg.norm(N)
        d = rng.standard_normal(3) * 0.01
        CQ, CP = rng.uniform(0, 1), rng.uniform(0, 1)
        JC, rc = cref.photometric(tuple(P), tuple(Q), tuple(N), tuple(d), CQ, CP)
        JC = np.array(JC)
        fd = np.zeros(6)
        for k in range(6):
            h = 1e-6 if k < 3 else 1e-3
            x = np.zeros(6)
            vals = []
            for sgn in (1.0, -1.0):
                x[k] = sgn * h
                Pm = _rodrigues(x[:3]) @ P + x[3:]
                vals.append(cref.photometric(tuple(Pm), tuple(Q), tuple(N), tuple(d), CQ, CP)[1])
            fd[k] = (vals[0] - vals[1]) / (2 * h)
        scale = np.abs(JC).max()
        assert np.allclose(JC, -fd, rtol=1e-6, atol=1e-6 * scale), (JC, -fd)
        # and the gradient used is the tangential one: J_C's translation part is d - (d . N) N
        t = d - (d @ N) * N
        assert np.allclose(JC[3:], t, rtol=1e-12, atol=1e-15) and abs(JC[3:] @ N) < 1e-12


def test_kappa_zero_terms_are_point_to_plane_values():
    """kappa = 0: the colored terms equal point-to-plane's as values (np.array_equal: a -0 may become +0)."""
    F = np.zeros((64, 8), np.float32)
    rng = np.random.default_rng(5)
    PF = rng.uniform(-500, 500, (64, 4)).astype(np.float32)
    PF[:, 3] = rng.uniform(0.3, 1, 64)
    PF[::7, 3] = 0.0
    PM = (PF + rng.uniform(-5, 5, (64, 4))).astype(np.float32)
    ids = rng.integers(0, 64, 64).astype(np.uint32)
    N = rng.standard_normal((64, 4)).astype(np.float32)
    G = rng.standard_normal((64, 4)).astype(np.float32)
    F[:, 4:7] = rng.uniform(0, 1, (64, 3))
    a = cref.pair_terms(PF, PM, ids, N, G, F, 0.05, 0.0)
    b = ref.pair_terms(PF, PM, ids, N, 0.05)
    assert np.array_equal(a, b)
    assert not np.array_equal(cref.pair_terms(PF, PM, ids, N, G, F, 0.05, 10.0), b)
