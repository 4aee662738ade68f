"""Symmetric ICP (icp_set_symmetric) without a device: the C-ABI's declarations, exports and refusals, the header as C and the facade as
C++, both command lines, and independent checks of the numpy restatement (tests/sym_ref.py): a float64 least-squares statement of the
objective, the increment against Rodrigues' formula, and the two properties that give the objective its meaning — it recovers a known
rigid motion from true pairs, and a pair of points on a common sphere leaves no residual, which point-to-plane does not see.
(tests/test_gpu_symmetric.py checks the engine against the restatement.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sym_ref as sref                                      # noqa: E402
import p2pl_ref as ref                                      # noqa: E402
from kernel_resources import kernel_resources               # noqa: E402
import robust_ref                                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports(L):
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    for decl in ("int icp_set_symmetric (icp_handle h, int on);", "int icp_get_symmetric (icp_handle h, int *on);",
                 "int icp_batch_set_symmetric (icp_batch_handle b, int on);"):
        assert decl in hdr, decl
    for name in ("icp_set_symmetric", "icp_get_symmetric", "icp_batch_set_symmetric"):
        assert hasattr(L, name), name


def test_invalid_arguments_are_refused_with_a_message(L):
    L.icp_set_symmetric.argtypes = [C.c_void_p, C.c_int]
    L.icp_batch_set_symmetric.argtypes = [C.c_void_p, C.c_int]
    for on in (-1, 2, 7, -2 ** 31):
        assert L.icp_set_symmetric(None, on) == 1, on                               # ICP_EINVAL
        assert "icp_set_symmetric: on must be 0 or 1" in L.icp_last_error(None).decode()
        assert L.icp_batch_set_symmetric(None, on) == 1, on
        assert "icp_batch_set_symmetric: on must be 0 or 1" in L.icp_batch_last_error(None).decode()
    for on in (0, 1):
        assert L.icp_set_symmetric(None, on) == 1
        assert "icp_set_symmetric: null handle" in L.icp_last_error(None).decode()
        assert L.icp_batch_set_symmetric(None, on) == 1
        assert "icp_batch_set_symmetric: null handle" in L.icp_batch_last_error(None).decode()
    v = C.c_int()
    assert L.icp_get_symmetric(None, C.byref(v)) == 1


def test_python_surface(engine):
    assert callable(engine.ICPStep.set_symmetric) and callable(engine.ICPStep.symmetric)
    assert callable(engine.ICPBatch.set_symmetric)
    import inspect
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["symmetric"].default is False


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b, const float *normals) {\n'
           '    int on;\n'
           '    if (icp_set_symmetric (h, 1)) return 1;\n'
           '    if (icp_get_symmetric (h, &on)) return 1;\n'
           '    if (icp_set_error_metric (h, ICP_METRIC_POINT_TO_PLANE, 0.f)) return 1;\n'
           '    if (icp_write (h, ICP_MEM_NORMALS_M, normals, 1)) return 1;\n'
           '    return icp_batch_set_symmetric (b, on);\n'
           '}\n')
    _compile(tmp_path, "sym.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'typedef ICPStep<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> Step;\n'
           'bool f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg, Step &step,\n'
           '        ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app, float *normals) {\n'
           '    reg.setNormals (ICP_NORMALS_GRID, 128); reg.setSymmetric (); reg.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 0.f);\n'
           '    step.setNormals (ICP_NORMALS_GIVEN); step.setSymmetric (true); step.write (Step::Memory::NORMALS_M, normals, true);\n'
           '    app.setNormals (ICP_NORMALS_GRID, 128); app.setSymmetric (true); app.setErrorMetric (ICP_METRIC_POINT_TO_PLANE, 0.f);\n'
           '    step.setSymmetric (false);\n'
           '    return reg.getSymmetric () && !step.getSymmetric ();\n'
           '}\n')
    _compile(tmp_path, "sym.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--symmetric" in r.stdout
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--symmetric", "1"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2, r.stderr                           # (a flag: it takes no value)


def test_example_command_line_accepts_the_option():
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    r = subprocess.run([exe, "--symmetric", "--device", "99"], capture_output=True, text=True, cwd=ROOT)
    assert "unknown option" not in r.stderr, r.stderr
    assert r.returncode != 2, r.stderr                          # (not a usage error: it went on to look for device 99)
    usage = open(os.path.join(ROOT, "examples", "registration.cpp")).read().split("#include")[0]
    assert "[--symmetric]" in usage and "icp_set_symmetric" in usage


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def make_pairs(rng, m, scale, w_zero=0.1, n_zero=0.1, n_nan=0.02):
    """Random float32 inputs in the engine's layout: PF = (Q, w), PM = (P, dist), ids, NORMALS_F (a table indexed by id), NORMALS_M
    (query order) and a rotation R (row-major, float32).  Some pairs have w = 0, some a zero or a non-finite normal on either side;
    the normals are independent of each other, so about half the pairs take the flip."""
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


def _H(S):
    """[-[S]x | I] of every pair, (m, 3, 6): a x S = -[S]x a."""
    m = S.shape[0]
    H = np.zeros((m, 3, 6))
    for k in range(3):
        H[:, :, k] = np.cross(np.eye(3)[k], S)
        H[:, k, 3 + k] = 1.0
    return H


def lstsq_sym(PF, PM, ids, NF, NM, R, mu):
    """x of min sum w [ (n . (d - H x))^2 + mu |d - H x|^2 ] in float64, H = [-[P + Q]x | I], d = Q - P, n the mean of N_Q and the
    flipped R N_M, all written independently of the restatement: the stacked rows sqrt (w) J and sqrt (w mu) H."""
    sel = PF[:, 3] != 0
    P, Q, w = PM[sel, :3].astype(np.float64), PF[sel, :3].astype(np.float64), PF[sel, 3].astype(np.float64)
    NQ = _finite_or_zero(NF[ids[sel], :3])
    NP = _finite_or_zero(NM[sel, :3]) @ np.asarray(R, np.float64).reshape(3, 3).T
    NP[np.einsum("ij,ij->i", NQ, NP) < 0] *= -1.0
    n = 0.5 * (NQ + NP)
    mu = np.float64(F32(mu))
    H, d = _H(P + Q), Q - P
    A = np.concatenate([np.sqrt(w)[:, None] * np.einsum("ij,ijk->ik", n, H), (np.sqrt(w * mu)[:, None, None] * H).reshape(-1, 6)])
    b = np.concatenate([np.sqrt(w) * np.einsum("ij,ij->i", n, d), (np.sqrt(w * mu)[:, None] * d).reshape(-1)])
    x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
    assert rank == 6
    return x


def _rel(x, y):
    return float(np.linalg.norm(np.asarray(x) - y) / np.linalg.norm(y))


CROSS_CASES = [  # (m, scale, mu, seed): sizes around the block of 256, metres and millimetres
    (37, 1.0, 0.05, 2), (256, 1000.0, 0.05, 3), (1000, 3000.0, 0.05, 4), (5000, 1000.0, 1.0, 5), (70001, 3000.0, 0.05, 6),
    (3000, 1000.0, 0.0, 7),
]


@pytest.mark.parametrize("m,scale,mu,seed", CROSS_CASES)
def test_float64_least_squares_cross_check(m, scale, mu, seed):
    PF, PM, ids, NF, NM, R = make_pairs(np.random.default_rng(seed), m, scale)
    x, ok = sref.ldlt_solve(sref.reduce_terms(sref.pair_terms_sym(PF, PM, ids, NF, NM, R, mu)))
    assert ok
    e = _rel(x, lstsq_sym(PF, PM, ids, NF, NM, R, mu))
    print("float64 cross-check m=%d mu=%g: %.3g" % (m, mu, e))
    assert e <= 1e-9, e


def test_robust_terms_are_the_plain_terms_weighed_by_omega():
    """The robust restatement against the plain one: every term of a pair is the plain term times omega (sG2 / k2) to rounding, and a
    pair whose omega is zero (Tukey beyond its scale) contributes exact zeros."""
    PF, PM, ids, NF, NM, R = make_pairs(np.random.default_rng(11), 3000, 1000.0)
    mu, scale = 0.05, 8.0
    plain = sref.pair_terms_sym(PF, PM, ids, NF, NM, R, mu)
    NQ, NMq = sref._lookup(NF, ids, 3000), sref._lookup(NM, np.arange(3000), 3000)
    n = np.stack(sref.mean_normal(NQ, NMq, R), -1)
    d = PF[:, :3].astype(np.float64) - PM[:, :3].astype(np.float64)
    sG2 = np.einsum("ij,ij->i", d, n) ** 2 + float(F32(mu)) * np.einsum("ij,ij->i", d, d)
    for name, loss in robust_ref.LOSSES.items():
        rob = sref.pair_terms_sym_robust(PF, PM, ids, NF, NM, R, mu, loss, scale)
        om = robust_ref.omega(loss, sG2 / robust_ref.k2(scale))
        assert np.allclose(rob, plain * om[:, None], rtol=1e-12, atol=0.0), name
        if name == "tukey":
            assert (om == 0).sum() > 100 and (rob[om == 0] == 0).all()


def _rodrigues(axis_angle):
    th = np.linalg.norm(axis_angle)
    if th == 0:
        return np.eye(3)
    k = axis_angle / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_increment_is_rot_trans_rot():
    """Rk built from qk equals R_a R_a and tk equals R_a (c t), R_a the rotation by theta = atan |a| about a by Rodrigues' formula in
    float64 and c = cos theta.  |a| up to 1 (theta up to 45 degrees); float rounding: qk and tk are float32, so a few float32 epsilons
    relative to the rotation's unit entries and to |t|."""
    rng = np.random.default_rng(5)
    eps = float(np.finfo(F32).eps)
    lengths = list(rng.uniform(0.0, 1.0, 200)) + [0.0, 1e-9, 1e-3, 1.0]
    for ln in lengths:
        a = rng.normal(size=3)
        a *= ln / np.linalg.norm(a)
        t = rng.normal(size=3) * 100.0
        Tk = sref.increment_sym(list(a) + list(t))
        assert Tk[7] == 1.0
        th = np.arctan(np.linalg.norm(a))
        Ra = _rodrigues(a / np.linalg.norm(a) * th) if ln > 0 else np.eye(3)
        Rk = ref.quat_to_rot(Tk[:4]).astype(np.float64).reshape(3, 3)
        assert np.abs(Rk - Ra @ Ra).max() <= 8 * eps, (ln, np.abs(Rk - Ra @ Ra).max())
        want = Ra @ (np.cos(th) * t)
        assert np.abs(Tk[4:7].astype(np.float64) - want).max() <= 2 * eps * np.linalg.norm(t), (ln, Tk[4:7], want)


def _as_inputs(P, Q, NQ, NM):
    m = P.shape[0]
    PF = np.zeros((m, 4), F32); PF[:, :3], PF[:, 3] = Q, 1.0
    PM = np.zeros((m, 4), F32); PM[:, :3] = P
    NF4 = np.zeros((m, 4), F32); NF4[:, :3] = NQ
    NM4 = np.zeros((m, 4), F32); NM4[:, :3] = NM
    return PF, PM, np.arange(m, dtype=np.uint32), NF4, NM4


def test_true_pairs_under_a_known_motion_are_recovered_within_6_steps():
    """Noise-free pairs under a known rigid motion (10 degrees), true correspondences, exact normals with N_M = R^T N_Q: iterating the
    restatement's step with the pairs held fixed reaches the true motion to 1e-6 relative within 6 steps."""
    rng = np.random.default_rng(8)
    m = 2000
    u, v = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    z = 2.0 + 0.3 * np.sin(2.5 * u) * np.cos(1.7 * v) + 0.2 * u * v
    Q = np.stack([u, v, z], -1) * 1000.0
    zu = 0.75 * np.cos(2.5 * u) * np.cos(1.7 * v) + 0.2 * v
    zv = -0.51 * np.sin(2.5 * u) * np.sin(1.7 * v) + 0.2 * u
    NQ = np.stack([-zu, -zv, np.ones(m)], -1)
    NQ /= np.linalg.norm(NQ, axis=1, keepdims=True)
    Rt = _rodrigues(np.array([0.3, 0.9, 0.1]) / np.linalg.norm([0.3, 0.9, 0.1]) * np.radians(10.0))
    tt = np.array([25.0, -10.0, 15.0])
    M = (Q - tt) @ Rt                                            # Rt M + tt = Q
    NM = NQ @ Rt                                                 # N_M = Rt^T N_Q
    T, R = ref.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    M32 = M.astype(F32)
    errs = []
    for _ in range(6):
        # the pairs held fixed: P = the current transform of M, in float32 as the search stores it
        R64, t64 = R.astype(np.float64).reshape(3, 3), T[4:7].astype(np.float64)
        P = (M32.astype(np.float64) @ R64.T + t64).astype(F32)
        PF, PM, ids, NF4, NM4 = _as_inputs(P, Q.astype(F32), NQ.astype(F32), NM.astype(F32))
        system, T, R, Tk, Rk = sref.step(PF, PM, ids, NF4, NM4, 0.0, T, R)
        assert system[27] == 1.0
        e_rot = np.linalg.norm(R.astype(np.float64).reshape(3, 3) - Rt) / np.linalg.norm(Rt)
        e_tr = np.linalg.norm(T[4:7].astype(np.float64) - tt) / np.linalg.norm(tt)
        errs.append((e_rot, e_tr))
    print("true pairs: " + "  ".join("%.2e/%.2e" % e for e in errs))
    assert min(max(e) for e in errs) <= 1e-6, errs
    # and it stays there, at float32's floor: R is kept in float32, and its rounding acts on the translation over the cloud's distance
    # from the origin (|Q| up to 2700 mm), which is more than 1e-6 of |t| = 31 mm
    lever = float(np.linalg.norm(Q, axis=1).max())
    for e_rot, e_tr in errs[1:]:
        assert e_rot <= 1e-6 and e_tr * np.linalg.norm(tt) <= 4 * float(np.finfo(F32).eps) * lever, errs


def _integer_sphere(rho):
    """Every integer point of the sphere |X| = rho about the origin, as float64."""
    pts = []
    for a in range(-rho, rho + 1):
        for b in range(-rho, rho + 1):
            c2 = rho * rho - a * a - b * b
            if c2 < 0:
                continue
            c = int(round(c2 ** 0.5))
            if c * c == c2:
                pts += [(a, b, c)] if c == 0 else [(a, b, c), (a, b, -c)]
    return np.array(pts, np.float64)


def _sphere_pairs(rng, centre, rho=65):
    """Pairs (P, Q, N_P, N_Q) of points of one sphere, paired at random among themselves within a cap.  The coordinates are integers and
    the outward normals are given with the length rho, X - centre (a normal is used as given, whatever its length), so float32 holds
    every input exactly and (Q - P) . (N_P + N_Q) = |Q - c|^2 - |P - c|^2 is an exact zero in double."""
    X = _integer_sphere(rho)
    j = rng.permutation(X.shape[0])
    keep = (np.einsum("ij,ij->i", X, X[j]) > 0.5 * rho * rho) & (j != np.arange(X.shape[0]))
    assert keep.sum() >= 40
    c = np.asarray(centre, np.float64)
    return X[keep] + c, X[j][keep] + c, X[keep], X[j][keep]


def test_pairs_on_a_sphere_leave_no_residual():
    """Points on a sphere with outward normals, paired at random among themselves, identity motion, mu = 0: every r is zero
    ((Q - P) . (N_P + N_Q) = (Q - P) . (P + Q - 2 c) = |Q - c|^2 - |P - c|^2), so the right-hand side is zero and the step is the
    identity to 1e-9.  p2pl_ref.step on the same pairs is not the identity: this is the property that separates the objective from
    point-to-plane.  The inputs are chosen so that float32 holds them exactly (_sphere_pairs); the restatement then has to give exact
    zeros, which is well inside 1e-9.

    One sphere alone leaves the three rotations about its centre undetermined (A is singular: whether the pivot test sees that or
    rounding lets a tiny pivot through, the step is the identity, by the identity step or by x = 0).  The second half of the test
    repeats the check on three spheres with centres that are not collinear, where the system is regular (status 1) and x = 0 is its
    solution."""
    T0, R0 = ref.IDENTITY_TK.copy(), np.eye(3, dtype=F32).ravel()
    centres = [(100, -50, 1500), (-300, 200, 1200), (250, 400, 1800)]
    for n_spheres in (1, 3):
        rng = np.random.default_rng(9)
        parts = [_sphere_pairs(rng, c) for c in centres[:n_spheres]]
        P, Q, NP_, NQ = (np.concatenate([p[k] for p in parts]) for k in range(4))
        PF, PM, ids, NF4, NM4 = _as_inputs(P, Q, NQ, NP_)
        for a32, a64 in ((PF[:, :3], Q), (PM[:, :3], P), (NF4[:, :3], NQ), (NM4[:, :3], NP_)):
            assert np.array_equal(a32.astype(np.float64), a64)       # (held exactly)
        system, T, R, Tk, Rk = sref.step(PF, PM, ids, NF4, NM4, 0.0, T0, R0)
        rhs_scale = np.abs(system[:21]).max()
        assert rhs_scale > 0 and np.abs(system[21:27]).max() <= 1e-9 * rhs_scale
        assert np.abs(Tk.astype(np.float64) - ref.IDENTITY_TK).max() <= 1e-9, (n_spheres, Tk)
        assert np.abs(T.astype(np.float64) - T0).max() <= 1e-9
        if n_spheres == 3:
            assert system[27] == 1.0
        # point-to-plane on the same pairs moves: by degrees and by millimetres
        sp, Tp, Rp, Tkp, Rkp = ref.step(PF, PM, ids, NF4, 0.0, T0, R0)
        assert sp[27] == 1.0
        moved = np.abs(Tkp.astype(np.float64) - ref.IDENTITY_TK)
        print("sphere(s) %d: status %g, symmetric Tk %s, point-to-plane Tk %s" % (n_spheres, system[27], Tk, Tkp))
        assert moved[:3].max() > 1e-3 or moved[4:7].max() > 1e-1, Tkp


def test_zero_normals_give_the_mu_share_and_zero_weights_the_identity_step():
    PF, PM, ids, NF, NM, R = make_pairs(np.random.default_rng(21), 3000, 1000.0)
    Z = np.zeros((3000, 4), F32)
    mu = 0.05
    t = sref.pair_terms_sym(PF, PM, ids, Z, Z, R, mu)
    # the mu share alone: w mu G and w mu g, with J = 0
    sel = PF[:, 3] != 0
    w = PF[:, 3].astype(np.float64)
    muf = float(F32(mu))
    d = PF[:, :3].astype(np.float64) - PM[:, :3].astype(np.float64)
    assert np.array_equal(t[sel, 15], w[sel] * (0.0 + muf * 1.0))                  # (term (3, 3))
    assert np.array_equal(t[sel, 24], w[sel] * (0.0 + muf * d[sel, 0]))            # (term 21 + 3)
    assert (t[~sel] == 0).all()
    # and with mu = 0 nothing at all: a singular system, the identity step, status 0
    T0, R0 = ref.IDENTITY_TK.copy(), R
    system, T, Rn, Tk, Rk = sref.step(PF, PM, ids, Z, Z, 0.0, T0, R0)
    assert (system == 0).all()
    assert np.array_equal(T, T0) and np.array_equal(Rn, R0) and np.array_equal(Tk, ref.IDENTITY_TK)
    # one absent normal counts a quarter: the (n, n) block is a quarter of point-to-plane's with the same normal
    one = sref.pair_terms_sym(PF, PM, ids, NF, Z, R, 0.0)
    NQ = sref._lookup(NF, ids, 3000).astype(np.float64)
    assert np.array_equal(one[sel, 15], w[sel] * ((NQ[sel, 0] * 0.5) * (NQ[sel, 0] * 0.5)))
    # all w zero
    PF0 = PF.copy(); PF0[:, 3] = 0
    system, T, Rn, Tk, Rk = sref.step(PF0, PM, ids, NF, NM, mu, T0, R0)
    assert (system == 0).all() and system[27] == 0.0
    assert np.array_equal(T, T0) and np.array_equal(Tk, ref.IDENTITY_TK)


def test_sym_kernels_have_zero_scratch():
    """The symmetric moments (loss off, loss on): the unit's complete kernel list, no scratch, no dynamic stack."""
    res = dict(kernel_resources("icp_amd/csrc/icp_symmetric.hip"))
    names = sorted(res)
    assert names == ["k_sym_moments<false>", "k_sym_moments<true>"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])
