"""The device's rotation solvers and composition (icp_amd/csrc/icp_device.h: icp_power_method_quad, icp_svd_rotation, icp_rot_to_quat,
icp_compose / icp_compose_pure) against the oracle bit for bit and against float64, on the corpus of tests/rotation_cases.py and on
registrations whose cumulative rotation is 120 - 180 degrees (each branch of rot_to_quat).  The float64 bounds are those of
tests/test_rotation_solvers_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ref as ref                                                 # noqa: E402
import rotation_cases as rc                                               # noqa: E402

pytestmark = pytest.mark.gpu
A, C_ = 2e2, 1e-6                                                         # the metric's a and the scale c of the registrations below


def same_bits(got, want):
    """Equal bit for bit, a NaN equal to any NaN (payloads are not compared)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %r want %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("solver", ["literal", "squared", "eigen"])
def test_corpus_equals_the_oracle_and_float64(engine, oracle, solver):
    bad, far = [], []
    for c in rc.cases():
        if solver == "eigen":
            T, R, _ = engine.power_method(c.S, c.means, rot=engine.ICPStepConfigT.EIGEN)
            oR, oT = oracle.svd_rotation(c.S, c.means)
            ok = same_bits(T, oT) and same_bits(R, oR)
        else:
            mode = engine.PowerMode.SQUARED if solver == "squared" else engine.PowerMode.LITERAL
            T, R, it = engine.power_method(c.S, c.means, mode=mode)
            oT, oit = oracle.power_method(c.S, c.means, fast=(solver == "squared"))
            ok = same_bits(T, oT) and same_bits(R, oracle.quat_to_rot(oT[:4])) and it == oit
        if not ok:
            bad.append(c.label)
        if solver != "literal" and c.unique and c.in_range(solver):
            e, b = rc.quat_error(T[:4], c.q), rc.quat_bound(c)
            if not e <= b:
                far.append("%s %.3g > %.3g" % (c.label, e, b))
    assert not bad, "%s: %d cases differ from the oracle, first: %s" % (solver, len(bad), bad[:8])
    assert not far, "%s: %d cases beyond the float64 bound: %s" % (solver, len(far), far[:8])


def _rotated_pair(engine, side, axis, deg, seed=0x1C9D5EED):
    """(F, M', T0): M' is the synthetic moving cloud turned by Rbig^T about the origin and T0 = [quat (Rbig) | 0, 0, 0 | 1], so a run
    that starts from T0 sees the ordinary 3-degree problem while its cumulative R stays near Rbig."""
    F, M = engine.synth_pair(side, seed=seed)
    Rb = rc.rotation(axis, deg)
    M = M.copy()
    M[:, 0:3] = (M[:, 0:3].astype(np.float64) @ Rb).astype(np.float32)          # rows: Rb^T m
    q = ref.rot_to_quat(Rb)
    T0 = np.r_[q, 0.0, 0.0, 0.0, 1.0].astype(np.float32)
    return F, M, T0


# cumulative rotations for each branch of rot_to_quat: trace > 0 ('w'), and the largest diagonal x, y, z of trace <= 0
BIG_TURNS = [("w", (0.3, 0.9, 0.1), 60.0), (0, (1.0, 0.1, -0.05), 150.0), (1, (0.05, 1.0, 0.1), 170.0), (2, (-0.1, 0.05, 1.0), 180.0)]
MODES = ["reference_order", "fused", "eigen"]


def _handle(engine, oracle, mode, side, nr, batch=1):
    CR = engine.ICPStepConfigT.EIGEN if mode == "eigen" else engine.ICPStepConfigT.POWER_METHOD
    g = engine.ICP(0, CR=CR)
    g.init(side * side, nr, A, C_, batch=batch)
    fused = mode != "reference_order"
    g.setReduceMode(engine.ReduceMode.FUSED if fused else engine.ReduceMode.REFERENCE_ORDER)
    g.setPowerMode(engine.PowerMode.SQUARED)
    mk = lambda: oracle.OracleICP(side * side, nr, A, C_, rot=oracle.ROT_SVD if mode == "eigen" else oracle.ROT_POWER,
                                  threads=8, power_fast=True, fused=fused)
    return g, mk


def _check_final(engine, g, o, b, what, eigen):
    assert g.state(b).k == o.k, (what, g.state(b).k, o.k)
    assert_bits(g.read(engine.Memory.T, b), o.T, what + ": T")
    assert_bits(g.read(engine.Memory.R, b).reshape(3, 3), o.R, what + ": R")
    assert_bits(g.read(engine.Memory.TK, b), o.Tk, what + ": Tk")
    # q is re-derived from R in every composition.  The SVD's Rk is orthonormal to a few ulps only, and R drifts by that much over a
    # run: 1.4e-6 on these runs, hence 4e-6 for EIGEN (1e-6 for the power method, whose Rk is the rotation of a unit quaternion)
    T, R = g.read(engine.Memory.T, b), g.read(engine.Memory.R, b).reshape(3, 3).astype(np.float64)
    assert np.abs(ref.quat_to_rot(T[:4]) - R).max() < (4e-6 if eigen else 1e-6), (what, T, R)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("branch,axis,deg", BIG_TURNS, ids=[str(t[0]) for t in BIG_TURNS])
def test_composition_at_large_angles(engine, oracle, mode, branch, axis, deg):
    side, nr = 64, 64
    F, M, T0 = _rotated_pair(engine, side, axis, deg)
    assert rc.rot_branch(ref.quat_to_rot(T0[:4])) == branch
    g, mk = _handle(engine, oracle, mode, side, nr)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T0)
    o = mk()
    o.write_f(F); o.write_m(M); o.build_rbc(); o.write_t(T0)
    k = g.run()
    assert k == o.run() and o.converged, (mode, branch, k, o.k)
    _check_final(engine, g, o, 0, "%s, branch %s" % (mode, branch), mode == "eigen")
    assert rc.rot_branch(g.read(engine.Memory.R)) == branch
    g.close()


@pytest.mark.parametrize("mode", ["fused", "eigen"])
def test_composition_at_large_angles_batched(engine, oracle, mode):
    """Batch 3: each registration starts from a turn of its own (branches x, y, z) and equals its own oracle."""
    side, nr = 64, 64
    g, mk = _handle(engine, oracle, mode, side, nr, batch=3)
    oracles = []
    for b, (_, axis, deg) in enumerate(BIG_TURNS[1:]):
        F, M, T0 = _rotated_pair(engine, side, axis, deg, seed=0x1C9D5EED + b)
        g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
        o = mk()
        o.write_f(F); o.write_m(M); o.build_rbc(); o.write_t(T0)
        oracles.append((o, T0))
    g.buildRBC()
    for b, (o, T0) in enumerate(oracles):
        g.write(engine.Memory.T, T0, batch_index=b)
    g.run()
    for b, (o, _) in enumerate(oracles):
        o.run()
        _check_final(engine, g, o, b, "%s, registration %d" % (mode, b), mode == "eigen")
    g.close()


def test_eigen_run_on_an_exactly_planar_scene(engine, oracle):
    """z = 0 for every point of both clouds: S has a zero column and a zero row in every iteration, and the SVD branch completes U.
    The iteration's R stays a rotation and the run converges to the exact transform (noise-free, the correspondences end exact)."""
    side, nr = 64, 64
    F, M = engine.synth_pair(side)
    F = F.copy()
    F[:, 2] = 0.0
    Rt, tt = rc.rotation((0.0, 0.0, 1.0), 1.0), np.array([2.0, -1.0, 0.0])
    M = F.copy()
    M[:, 0:3] = ((F[:, 0:3].astype(np.float64) - tt) @ Rt).astype(np.float32)                   # F = Rt M + t, z = 0 on both
    g, mk = _handle(engine, oracle, "eigen", side, nr)
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    o = mk()
    o.write_f(F); o.write_m(M); o.build_rbc()
    k = g.run()
    assert k == o.run() and o.converged and k < 20, k
    _check_final(engine, g, o, 0, "planar, EIGEN", True)
    R = g.read(engine.Memory.R).astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-5
    assert np.abs(R - Rt).max() < 1e-6, (R, Rt)
    T = g.read(engine.Memory.T)
    assert np.abs(T[4:7] - tt).max() < 1e-4 and abs(T[7] - 1.0) < 1e-6, T
    g.close()
