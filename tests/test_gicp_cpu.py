"""Generalized ICP (icp_set_plane_to_plane) without a device: the C-ABI's declarations, exports and refusals, the enum values, the
header as C and the facade as C++, both command lines, and three independent checks of the numpy restatement (tests/gicp_ref.py):
zero normals against the point-to-point share of point-to-plane, a float64 least-squares statement of the objective, and the weights
of a pair displaced along and across a plane.  (tests/test_gpu_gicp.py checks the engine against the restatement.)

The float64 cross-check's tolerance.  x of ldlt_solve (reduce_terms (..)) is compared with numpy's least squares over the stacked rows,
as |x - x_ls| / |x_ls|, over CROSS_CASES.  Measured here on those inputs (the largest value over the cases):
    point-to-plane restatement (p2pl_ref.pair_terms, rows sqrt (w) N . e and sqrt (w mu) e):      3.76e-15
    plane-to-plane restatement (gicp_ref.pair_terms_gicp, rows sqrt (w) L^T e, L L^T = M + mu I):  3.76e-14  (9.99 x the first)
The first is what the trees and LDL^T on the normal equations lose on these inputs and is the reference.  The second is within the
10 x allowed by a hair, and most of it is the least-squares reference's own: against a solve of the normal equations in 80-bit
arithmetic the largest case (70001 pairs, epsilon = 1e-3, cond A = 8e7) has the restatement 1.7e-14 away and numpy's lstsq 3.7e-14.
(C_Q + C_P has the condition number 1 / epsilon, which point-to-plane's rows do not have; the reference here inverts it in extended
precision so that this step adds nothing — with numpy.linalg.inv in float64 the figure was 4.8e-14.)  The test measures the first figure again on
every run and allows the plane-to-plane restatement 10 x that value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gicp_ref as gref                                     # noqa: E402
import p2pl_ref as ref                                      # noqa: E402
from kernel_resources import kernel_resources               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports(L):
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    for decl in ("int icp_set_plane_to_plane (icp_handle h, float epsilon);", "int icp_get_plane_to_plane (icp_handle h, float *epsilon);",
                 "int icp_batch_set_plane_to_plane (icp_batch_handle b, float epsilon);"):
        assert decl in hdr, decl
    assert hdr.index("ICP_MEM_COLOR_GRAD_F = 23,") < hdr.index("ICP_MEM_NORMALS_M = 24,") < hdr.index("ICP_MEM_COUNT_")
    assert "icp_track_submit and icp_track_next return ICP_ESTATE while it is on" in hdr
    for name in ("icp_set_plane_to_plane", "icp_get_plane_to_plane", "icp_batch_set_plane_to_plane"):
        assert hasattr(L, name), name


def test_invalid_arguments_are_refused_with_a_message(L):
    L.icp_set_plane_to_plane.argtypes = [C.c_void_p, C.c_float]
    L.icp_batch_set_plane_to_plane.argtypes = [C.c_void_p, C.c_float]
    for eps in (-1.0, 1.5, float("nan"), float("inf"), -float("inf"), -1e-30):
        assert L.icp_set_plane_to_plane(None, eps) == 1, eps                       # ICP_EINVAL
        assert "icp_set_plane_to_plane: epsilon must be in [0, 1]" in L.icp_last_error(None).decode()
        assert L.icp_batch_set_plane_to_plane(None, eps) == 1, eps
        assert "icp_batch_set_plane_to_plane: epsilon must be in [0, 1]" in L.icp_batch_last_error(None).decode()
    for eps in (0.0, 0.001, 1.0):
        assert L.icp_set_plane_to_plane(None, eps) == 1
        assert "icp_set_plane_to_plane: null handle" in L.icp_last_error(None).decode()
        assert L.icp_batch_set_plane_to_plane(None, eps) == 1
        assert "icp_batch_set_plane_to_plane: null handle" in L.icp_batch_last_error(None).decode()
    e = C.c_float()
    assert L.icp_get_plane_to_plane(None, C.byref(e)) == 1
    # it is a setter of its own, not a metric: 3 is still unknown
    assert L.icp_set_error_metric(None, 3, 0.0) == 1
    assert "icp_set_error_metric: unknown metric" in L.icp_last_error(None).decode()


def test_enum_and_table_values(engine):
    assert engine.Memory.NORMALS_M == 24
    assert (engine.Memory.NORMALS_F, engine.Memory.PLANE_SYSTEM, engine.Memory.COLOR_GRAD_F) == (21, 22, 23)
    from icp_amd import _MEM_DTYPE, _write_floats
    assert _write_floats(engine.Memory.NORMALS_M, 100) == 400
    assert _MEM_DTYPE[engine.Memory.NORMALS_M] == (np.float32, 4)
    assert callable(engine.ICPStep.set_plane_to_plane) and callable(engine.ICPStep.plane_to_plane)
    assert callable(engine.ICPBatch.set_plane_to_plane)


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b, const float *normals) {\n'
           '    float eps; float n[4 * 16];\n'
           '    if (icp_set_plane_to_plane (h, 0.001f)) return 1;\n'
           '    if (icp_get_plane_to_plane (h, &eps)) return 1;\n'
           '    if (icp_set_error_metric (h, ICP_METRIC_POINT_TO_PLANE, 0.f)) return 1;\n'
           '    if (icp_write (h, ICP_MEM_NORMALS_M, normals, 1)) return 1;\n'
           '    if (icp_read (h, ICP_MEM_NORMALS_M, n, sizeof n)) return 1;\n'
           '    if (icp_batch_write (b, 0, ICP_MEM_NORMALS_M, normals)) return 1;\n'
           '    return icp_batch_set_plane_to_plane (b, eps);\n'
           '}\n')
    _compile(tmp_path, "gicp.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'typedef ICPStep<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> Step;\n'
           'float f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg, Step &step,\n'
           '         ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app, float *normals) {\n'
           '    reg.setNormals (ICP_NORMALS_GRID, 128); reg.setPlaneToPlane (0.001f); reg.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 0.f);\n'
           '    step.setNormals (ICP_NORMALS_GIVEN); step.setPlaneToPlane (1.f); step.write (Step::Memory::NORMALS_M, normals, true);\n'
           '    app.setNormals (ICP_NORMALS_GRID, 128); app.setPlaneToPlane (0.01f); app.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 0.f);\n'
           '    return reg.getPlaneToPlane () + step.getPlaneToPlane ();\n'
           '}\n')
    _compile(tmp_path, "gicp.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--plane-to-plane" in r.stdout and "EPS" in r.stdout
    for bad in ("0", "-0.5", "1.5", "nan", "inf"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--plane-to-plane", bad],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--plane-to-plane" in r.stderr, (bad, r.stderr)
    import inspect
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["plane_to_plane"].default is None


def test_example_command_line_accepts_the_option():
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    r = subprocess.run([exe, "--plane-to-plane", "0.001", "--device", "99"], capture_output=True, text=True, cwd=ROOT)
    assert "unknown option" not in r.stderr, r.stderr
    assert r.returncode != 2, r.stderr                          # (not a usage error: it went on to look for device 99)
    for bad in ("0", "-1", "1.5", "nan"):
        r = subprocess.run([exe, "--plane-to-plane", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--plane-to-plane: EPS must be in (0, 1]" in r.stderr, (bad, r.stderr)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def make_pairs(rng, m, scale, w_zero=0.1, n_zero=0.1, n_nan=0.02):
    """Random float32 inputs in the engine's layout: PF = (Q, w), PM = (P, dist), ids, NORMALS_F (a table indexed by id), NORMALS_M
    (query order) and a rotation R (row-major, float32).  Some pairs have w = 0, some a zero or a non-finite normal on either side."""
    centre = np.array([0.1, -0.2, 1.0]) * scale
    P = (centre + rng.normal(size=(m, 3)) * 0.3 * scale).astype(F32)
    Q = (P + rng.normal(size=(m, 3)) * 0.01 * scale).astype(F32)
    w = rng.uniform(0.2, 1.0, m).astype(F32)
    w[rng.random(m) < w_zero] = 0.0

    def unit():
        n = rng.normal(size=(m, 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
        n[rng.random(m) < n_zero] = 0.0
        n[rng.random(m) < n_nan, 1] = np.nan
        return n
    ids = rng.permutation(m).astype(np.uint32)
    NF = np.zeros((m, 4), F32)
    NF[ids, :3] = unit()
    NM = np.zeros((m, 4), F32)
    NM[:, :3] = unit()
    PF = np.zeros((m, 4), F32)
    PF[:, :3], PF[:, 3] = Q, w
    PM = np.zeros((m, 4), F32)
    PM[:, :3] = P
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    R = ref.quat_to_rot(q.astype(F32))
    return PF, PM, ids, NF, NM, R


def _finite_or_zero(V):
    V = np.asarray(V, np.float64).copy()
    V[~np.isfinite(V).all(-1)] = 0.0
    return V


def _H(P):
    """[-[P]x | I] of every pair, (m, 3, 6): e = d - H x for x = (omega, tau), since omega x P = -[P]x omega."""
    m = P.shape[0]
    H = np.zeros((m, 3, 6))
    for k in range(3):
        H[:, :, k] = np.cross(np.eye(3)[k], P)                  # (the displacement of P by a unit rotation about axis k)
        H[:, k, 3 + k] = 1.0
    return H


def lstsq_gicp(PF, PM, ids, NF, NM, R, mu, eps):
    """x of min sum w (d - H x)^T (M + mu I) (d - H x) in float64: rows sqrt (w) L^T [H | d] with L L^T = M + mu I by Cholesky, M the
    inverse of C_Q + C_P with the covariances written as I - (1 - eps) n n^T / |n|^2."""
    sel = PF[:, 3] != 0
    P, Q, w = PM[sel, :3].astype(np.float64), PF[sel, :3].astype(np.float64), PF[sel, 3].astype(np.float64)
    NQ = _finite_or_zero(NF[ids[sel], :3])
    NP = _finite_or_zero(NM[sel, :3]) @ np.asarray(R, np.float64).reshape(3, 3).T
    LD = np.longdouble
    e, mu = LD(F32(eps)), np.float64(F32(mu))

    def cov(n):
        n = n.astype(LD)
        nn = np.einsum("ij,ij->i", n, n)
        C_ = np.tile(np.eye(3, dtype=LD), (n.shape[0], 1, 1))
        ok = nn > 0
        C_[ok] -= (1 - e) * np.einsum("ij,ik->ijk", n[ok], n[ok]) / nn[ok, None, None]
        return C_
    # (C_Q + C_P)^-1 has the condition number 1 / eps: inverted in extended precision (the adjugate over the determinant) and rounded
    # to float64 once, so that the reference carries no error of its own from this step
    S = cov(NQ) + cov(NP)
    adj = np.empty_like(S)
    for i in range(3):
        for j in range(3):
            a, b, c, d = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            adj[:, j, i] = S[:, a, c] * S[:, b, d] - S[:, a, d] * S[:, b, c]
    det = np.einsum("ij,ij->i", S[:, 0, :], adj[:, :, 0])
    W = (adj / det[:, None, None]).astype(np.float64) + mu * np.eye(3)
    Lt = np.transpose(np.linalg.cholesky(W), (0, 2, 1))
    H, d = _H(P), Q - P
    A = (np.sqrt(w)[:, None, None] * (Lt @ H)).reshape(-1, 6)
    b = (np.sqrt(w)[:, None] * np.einsum("ijk,ik->ij", Lt, d)).reshape(-1)
    x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
    assert rank == 6
    return x


def lstsq_p2pl(PF, PM, ids, NF, mu):
    """The same for point-to-plane: rows sqrt (w) N . (d - H x) and sqrt (w mu) (d - H x)."""
    sel = PF[:, 3] != 0
    P, Q, w = PM[sel, :3].astype(np.float64), PF[sel, :3].astype(np.float64), PF[sel, 3].astype(np.float64)
    N = _finite_or_zero(NF[ids[sel], :3])
    mu = np.float64(F32(mu))
    H, d = _H(P), Q - P
    A = np.concatenate([np.sqrt(w)[:, None] * np.einsum("ij,ijk->ik", N, H), (np.sqrt(w * mu)[:, None, None] * H).reshape(-1, 6)])
    b = np.concatenate([np.sqrt(w) * np.einsum("ij,ij->i", N, d), (np.sqrt(w * mu)[:, None] * d).reshape(-1)])
    x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
    assert rank == 6
    return x


def _rel(x, y):
    return float(np.linalg.norm(np.asarray(x) - y) / np.linalg.norm(y))


CROSS_CASES = [  # (m, scale, mu, eps, seed): sizes around the block of 256, metres and millimetres
    (37, 1.0, 0.05, 1e-3, 2), (256, 1000.0, 0.05, 1.0, 3), (1000, 3000.0, 0.05, 1e-3, 4), (5000, 1000.0, 1.0, 1e-2, 5),
    (70001, 3000.0, 0.05, 1e-3, 6), (3000, 1000.0, 0.0, 1e-3, 7),
]


def _cross_errors():
    """(largest relative error of the point-to-plane restatement, of the plane-to-plane restatement) over CROSS_CASES."""
    ep = eg = 0.0
    for m, scale, mu, eps, seed in CROSS_CASES:
        PF, PM, ids, NF, NM, R = make_pairs(np.random.default_rng(seed), m, scale)
        if mu > 0:                                               # (mu = 0 with zero normals about: point-to-plane alone may be rank deficient)
            x, ok = ref.ldlt_solve(ref.reduce_terms(ref.pair_terms(PF, PM, ids, NF, mu)))
            assert ok
            ep = max(ep, _rel(x, lstsq_p2pl(PF, PM, ids, NF, mu)))
        x, ok = gref.ldlt_solve(gref.reduce_terms(gref.pair_terms_gicp(PF, PM, ids, NF, NM, R, mu, eps)))
        assert ok
        eg = max(eg, _rel(x, lstsq_gicp(PF, PM, ids, NF, NM, R, mu, eps)))
    return ep, eg


def test_float64_least_squares_cross_check():
    ep, eg = _cross_errors()
    print("float64 cross-check: point-to-plane %.3g, plane-to-plane %.3g (allowed %.3g)" % (ep, eg, 10 * ep))
    assert 0.0 < ep < 1e-8, ep                                   # (the reference itself is a rounding-sized number)
    assert eg <= 10 * ep, (eg, ep)


def test_zero_normals_give_the_point_to_point_share():
    """No normal on either side: M = I / 2, and the system is (0.5 + mu) times sum w G, sum w g — with mu = 0 the same x as
    point-to-plane's with N = 0 and mu = 1, to the cross-check's tolerance (the two evaluate |P|^2 - px^2 and py^2 + pz^2 differently)."""
    tol = 10 * _cross_errors()[0]
    for m, scale, seed in ((300, 1.0, 21), (5000, 1000.0, 22)):
        PF, PM, ids, NF, NM, R = make_pairs(np.random.default_rng(seed), m, scale)
        Z = np.zeros((m, 4), F32)
        tg = gref.pair_terms_gicp(PF, PM, ids, Z, Z, R, 0.0, 1e-3)
        xg, okg = gref.ldlt_solve(gref.reduce_terms(tg))
        xp, okp = ref.ldlt_solve(ref.reduce_terms(ref.pair_terms(PF, PM, ids, Z, 1.0)))
        assert okg and okp
        assert _rel(xg, np.asarray(xp)) <= tol, (xg, xp, tol)
        # and term for term: the translation block is exactly w / 2 on the diagonal
        sel = PF[:, 3] != 0
        assert np.array_equal(tg[sel, 15], PF[sel, 3].astype(np.float64) * 0.5)
        assert (tg[~sel] == 0).all()


@pytest.mark.parametrize("eps", [1e-3, 1e-2, 0.25])
def test_a_pair_on_two_planes_weighs_the_normal_direction(eps):
    """Both frames a plane with the unit normal n: M = diag (1 / (2 eps), 1 / 2, 1 / 2) in n's frame, so a displacement d in the shared
    tangent plane costs eps times what the same displacement along n costs.  e^T M e is read off the terms: term 21 + 3 + c is
    w (M d)_c with mu = 0."""
    n = np.array([2.0, -1.0, 2.0]) / 3.0                         # (unit to float32 rounding)
    t = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)                 # (a tangent: n . t = 0)
    P = np.array([[120.0, -40.0, 900.0]], F32)
    R = np.eye(3, dtype=F32).ravel()
    N4 = np.zeros((1, 4), F32)
    N4[0, :3] = n

    def cost(d):
        PF = np.zeros((1, 4), F32)
        PF[0, :3], PF[0, 3] = P[0] + d.astype(F32), 1.0
        PM = np.zeros((1, 4), F32)
        PM[0, :3] = P[0]
        dd = PF[0, :3].astype(np.float64) - PM[0, :3].astype(np.float64)
        terms = gref.pair_terms_gicp(PF, PM, np.zeros(1, np.uint32), N4, N4, R, 0.0, eps)
        return float(terms[0, 24:27] @ dd)
    along_tangent, along_normal = cost(4.0 * t), cost(4.0 * n)
    assert along_normal > 0 and along_tangent > 0
    ratio = along_tangent / along_normal
    assert eps / 2 <= ratio <= 2 * eps, (ratio, eps)
    assert abs(along_normal - 16.0 / (2 * float(F32(eps)))) <= 1e-4 * along_normal
    assert abs(along_tangent - 16.0 / 2) <= 1e-4 * along_tangent


def test_gicp_kernels_have_zero_scratch():
    """The plane-to-plane moments (loss off, loss on): the unit's complete kernel list, no scratch, no dynamic stack."""
    res = dict(kernel_resources("icp_amd/csrc/icp_gicp.hip"))
    names = sorted(res)
    assert names == ["k_gicp_moments<false>", "k_gicp_moments<true>"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])
