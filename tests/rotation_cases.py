"""A deterministic corpus of rotation-solver inputs with float64 truth — TEST INFRASTRUCTURE (a plain module, not a conftest).

Each case is S[11], means[8] as the iteration hands them to its rotation solver (kernels/icp_kernels.cl:703-743, 989-999), built in
float64 from a point set P (the fixed side) and Q = (P - t) R (the moving side, so that P = R Q + t) and rounded to float32 once:

    S[0:9] = (c (Q - q_bar))^T (c (P - p_bar)) row-major (S_ab: a = moving, b = fixed),  S[9] = sum |c (P - p_bar)|^2,
    S[10] = sum |c (Q - q_bar)|^2,  means = [p_bar, 0, q_bar, 0]

The truth is taken from the SAME float32 S in float64: the top eigenvector of Horn's N (float64_ref.horn_matrix), the relative gap
(lambda1 - lambda2) / |N|, s_k = sqrt (S9 / S10) and t_k = m_f - s_k R(q) m_m.  Exact lines and two repeated points have no unique
optimum (any rotation about the line): `unique` is False there, and only properties that hold for every optimum are checked.

Families: an isotropic box, anisotropic boxes down to rods (small gaps without the planar +-lambda pairing), exact planes (axis-aligned
and tilted: S of rank 2), jittered planes, exact lines and two points (rank 1), mirrored correspondences (det S < 0: the SVD branch's
det fix).  Rotations from 0 to 180 degrees about each coordinate axis (exact zeros in q) and about generic axes, so that both branches
of rot_to_quat and each largest-diagonal axis of its trace <= 0 branch occur (asserted by cases()).  c from 1e-6 to 1, and S scaled
by powers of two so that the power method's exact rescale meets the largest exponents it handles and subnormal maxima.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ref as ref                                                 # noqa: E402

EPS32 = 2.0 ** -23
ANGLES = (0.0, 1e-3, 1.0, 30.0, 90.0, 119.0, 121.0, 150.0, 179.0, 180.0)
C_VALUES = (1e-6, 1e-4, 1e-3, 1e-2, 1.0)
GENERIC_AXES = ((0.3, 0.9, 0.1), (-0.6, 0.2, 0.77), (0.5, -0.5, 0.7071))
N_POINTS = 240
# max |N| = 2^e for the scaled cases: the edges of the solvers' float32 range (see in_range) and beyond it — the rescale's largest
# shift (2^126: scale 2^-126), the exponent it leaves alone (2^127) and subnormal maxima
SCALE_EXPONENTS = (60, 30, -30, -60, 126, 127, -127, -133)
POWER_RANGE = (-60, 60)
EIGEN_RANGE = (-30, 30)


class Case:
    """One solver input and its float64 truth."""

    def __init__(self, label, S, means, Rgen):
        self.label = label
        self.S = np.asarray(S, np.float32)
        self.means = np.asarray(means, np.float32)
        self.Rgen = Rgen                                                    # the rotation the points were generated with (float64)
        S64 = self.S.astype(np.float64)
        N = ref.horn_matrix(S64[:9].reshape(3, 3))
        w, V = np.linalg.eigh(N)
        self.lam = w[::-1].copy()                                           # lambda1 >= ... >= lambda4
        nrm = np.abs(w).max()
        self.gap = (w[3] - w[2]) / nrm if nrm > 0 else 0.0
        q = V[:, 3]
        self.q = q if q[np.argmax(np.abs(q))] > 0 else -q                   # (sign: largest component positive)
        self.sk = np.sqrt(S64[9] / S64[10])
        self.R = ref.quat_to_rot(self.q)
        self.tk = self.tk_of(self.R)
        self.unique = not (label.startswith("line") or label.startswith("twopoint")) and self.gap > 1e-9

    def tk_of(self, R):
        """t_k = m_f - s_k R m_m in float64 for a given rotation (the formula of :1050 / algorithms.cpp:3897)."""
        m = self.means.astype(np.float64)
        return m[0:3] - self.sk * (np.asarray(R, np.float64) @ m[4:7])

    @property
    def mean_scale(self):
        m = self.means.astype(np.float64)
        return np.linalg.norm(m[0:3]) + self.sk * np.linalg.norm(m[4:7])

    @property
    def top_exponent(self):
        top = np.abs(ref.horn_matrix(self.S[:9].astype(np.float64).reshape(3, 3))).max()
        return np.floor(np.log2(top)) if top > 0 else -np.inf

    def in_range(self, solver):
        """Whether the solver's float32 intermediates are finite and normal for this S, so that the float64 bounds apply: the power
        methods form (u.u)(v.v), of the order of max|N|^2 (range 2^+-60 for max |N|), the SVD forms products of squared column norms,
        of the order of max|S|^4 (2^+-30).  Outside, the results are compared bit for bit with the oracle only."""
        lo, hi = EIGEN_RANGE if solver == "eigen" else POWER_RANGE
        return lo <= self.top_exponent <= hi

    @property
    def branch(self):
        """The branch Eigen's matrix -> quaternion takes on the truth rotation: 'w' (trace > 0) or the largest diagonal 0 | 1 | 2."""
        return rot_branch(self.R)

    def __repr__(self):
        return "Case(%s, gap=%.2e)" % (self.label, self.gap)


def rot_branch(R):
    R = np.asarray(R, np.float64).reshape(3, 3)
    if (R[0, 0] + R[1, 1]) + R[2, 2] > 0:
        return "w"
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def solver_input(P, Q, c):
    """S[11], means[8] in float64 (rounded to float32 by the caller's Case)."""
    pb, qb = P.mean(0), Q.mean(0)
    dP, dQ = c * (P - pb), c * (Q - qb)
    S = np.concatenate([(dQ.T @ dP).ravel(), [(dP ** 2).sum(), (dQ ** 2).sum()]])
    means = np.concatenate([pb, [0.0], qb, [0.0]])
    return S, means


def _plane_basis(tilt):
    e1 = np.array([1.0, 0.0, tilt]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(np.array([0.2, 1.0, 0.1]), e1); e2 /= np.linalg.norm(e2)
    return e1, e2


def point_sets():
    """(name, P) in float64, millimetres: the families of the module docstring."""
    r = np.random.default_rng(0x5EED0)
    n = N_POINTS
    out = [("box", r.uniform(-500, 500, (n, 3)) + [100.0, -40.0, 900.0])]
    for sig in ((800, 50, 5), (800, 20, 2), (800, 5, 5)):
        out.append(("rod%dx%dx%d" % sig, r.normal(0, 1, (n, 3)) * sig + [20.0, 10.0, 1500.0]))
    uv = r.uniform(-1, 1, (n, 2)) * [300.0, 200.0]
    out.append(("plane_z", np.c_[uv, np.zeros(n)] + [0.0, 0.0, 0.0]))
    e1, e2 = _plane_basis(0.3)
    out.append(("plane_tilt", uv[:, :1] * e1 + uv[:, 1:] * e2 + [50.0, 25.0, 1000.0]))
    out.append(("plane_jitter", np.c_[uv, r.normal(0, 0.5, n)] + [0.0, 0.0, 800.0]))
    s = r.uniform(-400, 400, (n, 1))
    out.append(("line_x", np.c_[s, np.zeros(n), np.zeros(n)] + [0.0, 0.0, 700.0]))
    d = np.array([0.36, -0.48, 0.8])
    out.append(("line_tilt", s * d + [10.0, 20.0, 900.0]))
    two = np.array([[120.0, -80.0, 950.0], [-60.0, 140.0, 1010.0]])
    out.append(("twopoint", two[np.arange(n) % 2]))
    return out


MIRROR = np.diag([1.0, 1.0, -1.0])


@functools.lru_cache(maxsize=None)
def cases():
    """The corpus (cached): a list of Case.  Asserts its own coverage of the solvers' branches."""
    out = []
    sets = point_sets()
    axes = [("x", (1, 0, 0)), ("y", (0, 1, 0)), ("z", (0, 0, 1))] + [("g%d" % i, a) for i, a in enumerate(GENERIC_AXES)]
    t = np.array([25.0, -10.0, 15.0])
    k = 0
    for name, P in sets:
        for deg in ANGLES:
            for an, axis in axes:
                if deg == 0.0 and an != "x":
                    continue
                R = rotation(axis, deg)
                c = C_VALUES[k % len(C_VALUES)]
                k += 1
                Q = (P - t) @ R                                             # P = R Q + t
                S, m = solver_input(P, Q, c)
                out.append(Case("%s/%s/%g/c%g" % (name, an, deg, c), S, m, R))
    # mirrored correspondences: Q = (P - t) R M with a reflection M — det S < 0, the SVD branch's det fix
    for name, P in sets[:3]:
        for deg in (1.0, 30.0, 150.0):
            for an, axis in axes[3:5]:
                R = rotation(axis, deg)
                Q = ((P - t) @ R) @ MIRROR
                S, m = solver_input(P, Q, 1e-3)
                out.append(Case("mirror_%s/%s/%g" % (name, an, deg), S, m, R))
    # S scaled by powers of two: max |N| at the top of the exponents the rescale handles and below the normal range
    P = sets[0][1]
    for deg in (1.0, 150.0):
        R = rotation(GENERIC_AXES[0], deg)
        S, m = solver_input(P, (P - t) @ R, 1.0)
        N = ref.horn_matrix(S[:9].reshape(3, 3))
        top = np.abs(N).max()
        for e in SCALE_EXPONENTS:                                          # max |N| in [2^e, 2^(e+1))
            f = 2.0 ** (e - np.floor(np.log2(top)))
            Ss = S * f
            out.append(Case("scaled2^%d/g0/%g" % (e, deg), Ss, m, R))
    _assert_coverage(out)
    return out


def _assert_coverage(cs):
    branches = {c.branch for c in cs if c.unique}
    assert branches >= {"w", 0, 1, 2}, branches
    det = [np.linalg.det(c.S[:9].astype(np.float64).reshape(3, 3)) for c in cs]
    assert any(d < 0 for d in det), "no case with det S < 0"
    labels = [c.label for c in cs]
    for fam in ("box", "rod", "plane_z", "plane_tilt", "plane_jitter", "line", "twopoint", "mirror", "scaled"):
        assert any(fam in l for l in labels), fam
    # exact zeros in the truth quaternion (rotations about a coordinate axis)
    assert any(np.count_nonzero(c.q == 0.0) >= 2 for c in cs) or any(np.count_nonzero(np.abs(c.q) < 1e-12) >= 2 for c in cs)
    tops = [np.abs(ref.horn_matrix(c.S[:9].astype(np.float64).reshape(3, 3))).max() for c in cs]
    assert max(tops) >= 2.0 ** 127 and min(t for t in tops if t > 0) < 2.0 ** -126


def quat_error(q, truth):
    """Sign-aligned |q - truth| (q and -q are the same rotation)."""
    q = np.asarray(q, np.float64)[:4]
    return min(np.linalg.norm(q - truth), np.linalg.norm(q + truth))


def quat_bound(case):
    """What float32 arithmetic allows for the top eigenvector: 64 ulps, divided by the relative gap."""
    return max(64 * EPS32, 64 * EPS32 / case.gap)


def literal_applies(case):
    """Where the reference's literal loop (icp_kernels.cl:1012-1041) can work: a dominant positive eigenvalue, a clear gap and a first
    component it can divide by (:1024)."""
    return (case.unique and case.lam[0] >= 1.5 * abs(case.lam[3]) and case.gap >= 0.1 and abs(case.q[0]) >= 0.05)


def planar_case(seed, tilt=0.3):
    """S[11], means[8] of an exactly planar pair: points on a tilted plane, the moving set rotated by 7 degrees about the plane's normal
    (S of rank 2: Horn's N has the eigenvalue pairs +-(s1 + s2), +-(s1 - s2))."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1, 1, (400, 2)) * np.array([300.0, 200.0])
    e1 = np.array([1.0, 0.0, tilt]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(np.array([0.2, 1.0, 0.1]), e1); e2 /= np.linalg.norm(e2)
    n = np.cross(e1, e2)
    f = uv[:, :1] * e1 + uv[:, 1:] * e2
    th = np.radians(7.0)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    q = f @ R.T                                            # moving = R fixed: the solver must find R^T
    c = 1e-3
    S9 = (c * q).T @ (c * f)                               # S_ab = sum m_a f_b
    S = np.concatenate([S9.ravel(), [((c * f) ** 2).sum(), ((c * q) ** 2).sum()]]).astype(np.float32)
    means = np.zeros(8, np.float32)
    return S, means, R.T
