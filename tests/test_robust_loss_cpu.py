"""Robust loss without a device: argument validation of the C-ABI, the header as C, the C++ facade's and ICPReg's setters, both command
lines, the compiler's resources of the new kernels, and the restated weight function against the losses it is the IRLS weight of.
(tests/test_gpu_robust_loss.py checks what the option does.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from kernel_resources import kernel_resources

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_ref as ref                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_SCALES = (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf"))


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


def test_setter_refuses_unknown_losses_and_bad_scales_with_a_message(L):
    for loss in (-1, 4, 100):
        assert L.icp_set_robust_loss(None, loss, 10.0) == 1, loss                # ICP_EINVAL
        assert "unknown loss" in L.icp_last_error(None).decode()
    for loss in (1, 2, 3):
        for k in BAD_SCALES:
            assert L.icp_set_robust_loss(None, loss, k) == 1, (loss, k)
            assert "scale" in L.icp_last_error(None).decode(), (loss, k)
    for loss, k in ((0, float("nan")), (0, -5.0), (2, 30.0), (3, 1e-30), (1, 1e-45), (2, 3e38)):   # valid (NONE ignores the scale; a subnormal scale is > 0): only the null handle is refused
        assert L.icp_set_robust_loss(None, loss, k) == 1
        assert "null handle" in L.icp_last_error(None).decode()
    l, k = C.c_int32(), C.c_float()
    assert L.icp_get_robust_loss(None, C.byref(l), C.byref(k)) == 1


def test_batch_setter_refuses_them_too(L):
    """The batch setter checks its arguments before the handle, as the single setter does: each refusal names its reason, and valid
    arguments on no handle are refused as a null handle."""
    for loss in (-1, 4):
        assert L.icp_batch_set_robust_loss(None, loss, 30.0) == 1
        assert "unknown loss" in L.icp_batch_last_error(None).decode(), loss
    for k in BAD_SCALES:
        assert L.icp_batch_set_robust_loss(None, 1, k) == 1
        assert "scale" in L.icp_batch_last_error(None).decode(), k
    for loss, k in ((0, float("nan")), (2, 30.0)):
        assert L.icp_batch_set_robust_loss(None, loss, k) == 1
        assert "null handle" in L.icp_batch_last_error(None).decode(), (loss, k)


def test_python_names(engine):
    R = engine.RobustLoss
    assert (R.NONE, R.HUBER, R.CAUCHY, R.TUKEY) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    for name, v in (("NONE", 0), ("HUBER", 1), ("CAUCHY", 2), ("TUKEY", 3)):
        assert "#define ICP_ROBUST_%s %d" % (name, v) in hdr


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b) {\n'
           '    int loss; float k;\n'
           '    if (icp_set_robust_loss (h, ICP_ROBUST_TUKEY, 50.f)) return 1;\n'
           '    if (icp_get_robust_loss (h, &loss, &k)) return 1;\n'
           '    return icp_batch_set_robust_loss (b, ICP_ROBUST_CAUCHY, k);\n'
           '}\n')
    _compile(tmp_path, "robust.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'float f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
           '         ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
           '    reg.setRobustLoss (icp::RobustLoss::HUBER, 20.f);\n'
           '    icp::RobustLoss r; r.loss = icp::RobustLoss::TUKEY; r.scale = 50.f;\n'
           '    app.setRobustLoss (r); app.setRobustLoss (ICP_ROBUST_NONE);\n'
           '    return reg.getRobustLoss ().scale + (float) app.getRobustLoss ().loss;\n'
           '}\n')
    _compile(tmp_path, "robust.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--robust" in r.stdout, r.stderr
    from icp_amd.register import _robust
    assert _robust("cauchy:30") == (ref.CAUCHY, 30.0)
    for bad in ("foo:1", "huber:0", "tukey:-3", "cauchy:nan", "huber", "tukey:x"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--robust", bad], capture_output=True, text=True,
                           cwd=ROOT)
        assert r.returncode == 2 and "--robust" in r.stderr, (bad, r.stderr)


def test_example_command_line_accepts_the_option():
    """examples/registration (built by build()): --robust is an option of its own, its value is checked before anything touches a
    device; a good value gets past the check (and then needs a device)."""
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("foo:1", "huber:0", "tukey:", "cauchy:inf"):
        r = subprocess.run([exe, "--robust", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--robust: KIND:SCALE" in r.stderr, (bad, r.stderr)
    r = subprocess.run([exe, "--robust", "cauchy:30", "--device", "99"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 2 and "--robust" not in r.stderr and "unknown option" not in r.stderr, r.stderr


def test_robust_kernels_have_zero_scratch():
    res = dict(kernel_resources("icp_amd/csrc/icp_robust.hip"))
    names = sorted(res)
    assert names == ["k_plane_moments_robust<false>", "k_plane_moments_robust<true>", "k_trim_apply_robust<false>",
                     "k_trim_apply_robust<true>"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])


@pytest.mark.parametrize("loss", [ref.HUBER, ref.CAUCHY, ref.TUKEY])
def test_omega_is_the_irls_weight_of_rho(loss):
    """omega (s^2 / k^2) = rho'(s) / s by a central difference, u from 1e-6 to 1e3 and at the switch points u = 1 +- eps."""
    k = 7.5
    u = np.concatenate([np.logspace(-6, 3, 400), [1 - 1e-6, 1 + 1e-6, 1 - 1e-3, 1 + 1e-3]])
    s = k * np.sqrt(u)
    h = 1e-6 * s
    d = (ref.rho(loss, s + h, k) - ref.rho(loss, s - h, k)) / (2 * h)
    assert np.allclose(ref.omega(loss, u), d / s, rtol=2e-4, atol=1e-7), loss


def test_omega_edges():
    for loss in (ref.HUBER, ref.CAUCHY, ref.TUKEY):
        w = ref.omega(loss, [0.0, np.inf, np.nan])
        assert w[0] == 1.0 and w[1] == 0.0 and w[2] == 0.0, (loss, w)
    assert ref.omega(ref.HUBER, 1.0) == 1.0 and ref.omega(ref.HUBER, 4.0) == 0.5
    assert ref.omega(ref.TUKEY, 1.0) == 0.0 and ref.omega(ref.CAUCHY, 1.0) == 0.5


# ---- helpers of tests/test_gpu_robust_edges.py

@pytest.mark.parametrize("side,nr", [(128, 256), (30, 4)])
def test_edge_scene_is_exact_on_the_oracle(engine, oracle, side, nr):
    """The identity transform reproduces M bit for bit, every query keeps its own index, geo of each class is fp32 (offset^2), and
    u = geo / k^2 is 1 exactly for the class lifted by k = 8 and below 1 for k = 7.3 (fp32 geo below the double k^2)."""
    template = engine.synth_pair(side)[0]
    for k in (8.0, 7.3):
        offsets = ref.edge_offsets(k)
        F, M, cls = ref.edge_scene(side, template, offsets)
        tM = oracle.transform_q(M, ref.IDENTITY_T)
        assert np.array_equal(tM.view(np.uint32), M.view(np.uint32))
        o = oracle.OracleICP(side * side, nr, 2e2, 1e-6, threads=8)
        o.write_f(F); o.write_m(M)
        o.build_rbc()
        o.step()
        assert np.array_equal(o.nn_id["id"], np.arange(side * side))
        geo = ref.geo(F[o.nn_id["id"]], tM)
        assert np.array_equal(geo.view(np.uint32), ref.edge_geo(offsets)[cls].view(np.uint32))
        u = geo.astype(np.float64) / ref.k2(k)
        at, below, above = (u[cls == c] for c in (1, 2, 3))
        assert at.size >= side * side // 10
        if k == 8.0:
            assert (at == 1.0).all() and (below == 1.0 - 2.0 ** -23).all() and (above > 1.0).all()
            assert (u[cls == 0] == 0).all() and (geo[cls == 6] < np.finfo(np.float32).tiny).all() and (geo[cls == 6] > 0).all()
            assert ref.omega(ref.TUKEY, at).max() == 0 and ref.omega(ref.TUKEY, below).min() > 0
        else:
            assert (at < 1.0).all() and ref.omega(ref.TUKEY, at).min() > 0
            # (k^2 in float instead of double would put the class at u == 1)
            assert (geo[cls == 1] == np.float32(k) * np.float32(k)).all()


def test_intensity_channel_hits_its_target():
    import colored_ref
    for t in (4.0, np.nextafter(np.float32(4), np.float32(0)), np.nextafter(np.float32(4), np.float32(8)), 0.0, 2.0, 12.0):
        r = ref.intensity_channel(t)
        assert r is not None, t
        X = np.zeros((1, 8), np.float32)
        X[0, 4] = r
        assert colored_ref.intensity(X)[0] == np.float32(t), (t, r)


def test_float64_step_takes_given_weights(engine):
    """Float64ICP.step (weights=): the derived weights handed back give the same step; a pair of weight 0 takes no part, whatever its
    points hold."""
    import float64_ref as f64
    F, M = engine.synth_pair(16)
    ids = np.arange(256)
    a = f64.Float64ICP(F, M, 2e2, 1e-6)
    tM = M[:, :3].astype(np.float64)
    NN = F[:, :3].astype(np.float64)
    w = 100.0 / (100.0 + ((tM - NN) ** 2).sum(1) + 2e2 * ((M[:, 4:7].astype(np.float64) - F[:, 4:7]) ** 2).sum(1))
    Rk, tk, sk = a.step(ids)
    b = f64.Float64ICP(F, M, 2e2, 1e-6)
    Rk2, tk2, sk2 = b.step(ids, weights=w)
    assert np.array_equal(Rk, Rk2) and np.array_equal(tk, tk2) and sk == sk2
    w0 = w.copy(); w0[::5] = 0.0
    Mbad = M.copy(); Mbad[::5, :3] = np.nan
    c, d = f64.Float64ICP(F, M, 2e2, 1e-6), f64.Float64ICP(F, Mbad, 2e2, 1e-6)
    r1, r2 = c.step(ids, weights=w0), d.step(ids, weights=w0)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2)) and np.isfinite(r2[1]).all()
    T = np.array([0.01, 0.02, 0.03, 0.9993, 4.0, -3.0, 2.0, 1.0])
    c.set_T(T)
    assert np.allclose(c.T[:4], T[:4] / np.linalg.norm(T[:4])) and np.array_equal(c.T[4:], T[4:])
