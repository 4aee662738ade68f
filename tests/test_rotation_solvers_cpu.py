"""The oracle's rotation solvers (oracle/icp_oracle.c: power_literal, power_fast, orc_svd_rotation, orc_rot_to_quat) against float64 on
the corpus of tests/rotation_cases.py.  The device code is held to these functions bit for bit (tests/test_gpu_rotation_solvers.py), so
a misfit here is a misfit of the engine.  No GPU.

Bounds: the top eigenvector of a float32 N is determined to about 2^-23 |N| / gap; the squared start and the SVD branch must be within
64 ulps of that (sign-aligned |q - q64| <= max (64, 64 / gap) 2^-23) wherever the optimum is unique, and every rotation they return is
proper (R R^T = I, det R = +1, within 1e-5) also where it is not.  t_k and s_k are the float64 formulas of the solver's own rotation to
float32 rounding, relative to the size of the means.  The reference's literal loop is held to the same bound only where it can work
(literal_applies); elsewhere its failures are recorded, not asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ref as ref                                                 # noqa: E402
import rotation_cases as rc                                               # noqa: E402

EPS32 = rc.EPS32


def _report(bad, what):
    bad.sort(key=lambda b: -b[1])
    return "%s: %d cases, worst: %s" % (what, len(bad), "; ".join("%s %.3g (bound %.3g)" % b for b in bad[:6]))


def _solve(oracle, case, solver):
    """(q[4], R[3,3] float64, Tk[8], trips) of one solver on a case."""
    if solver == "eigen":
        R, Tk = oracle.svd_rotation(case.S, case.means)
        return Tk[:4], R.astype(np.float64), Tk, 0
    Tk, it = oracle.power_method(case.S, case.means, fast=(solver == "squared"))
    return Tk[:4], oracle.quat_to_rot(Tk[:4]).astype(np.float64), Tk, it


def test_corpus_covers_the_branches():
    cs = rc.cases()
    assert len(cs) > 500
    n = {b: sum(1 for c in cs if c.unique and c.branch == b) for b in ("w", 0, 1, 2)}
    assert min(n.values()) >= 10, n
    assert sum(1 for c in cs if not c.unique) >= 100
    assert sum(1 for c in cs if c.unique and c.gap < 2e-3 and c.in_range("power")) >= 50        # rods: small gaps, no +-lambda pairs


@pytest.mark.parametrize("solver", ["squared", "eigen"])
def test_quaternion_against_float64(oracle, solver):
    bad = []
    for c in rc.cases():
        if not (c.unique and c.in_range(solver)):
            continue
        q, _, _, it = _solve(oracle, c, solver)
        e, b = rc.quat_error(q, c.q), rc.quat_bound(c)
        if not e <= b:
            bad.append((c.label + " trips %d" % it, e, b))
    assert not bad, _report(bad, solver + " |q - q64|")


@pytest.mark.parametrize("solver", ["squared", "eigen"])
def test_every_rotation_is_proper(oracle, solver):
    """Also where the optimum is not unique (lines, two points): the step is composed into R, which must stay a rotation."""
    bad = []
    for c in rc.cases():
        if not c.in_range(solver):
            continue
        _, R, _, _ = _solve(oracle, c, solver)
        e = max(np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0)) if np.all(np.isfinite(R)) else np.inf
        if not e <= 1e-5:
            bad.append((c.label, e, 1e-5))
    assert not bad, _report(bad, solver + " |R R^T - I|, |det R - 1|")


@pytest.mark.parametrize("solver", ["squared", "eigen", "literal"])
def test_translation_and_scale_against_float64(oracle, solver):
    bad = []
    for c in rc.cases():
        if not c.in_range(solver) or (solver == "literal" and not rc.literal_applies(c)):
            continue
        q, R, Tk, _ = _solve(oracle, c, solver)
        if not np.all(np.isfinite(Tk)):
            bad.append((c.label + " (not finite)", np.inf, 0.0))
            continue
        es = abs(Tk[7] - c.sk) / c.sk
        if not es <= 4 * EPS32:
            bad.append((c.label + " sk", es, 4 * EPS32))
        et = np.abs(Tk[4:7] - c.tk_of(R)).max()
        bt = 32 * EPS32 * c.mean_scale
        if not et <= bt:
            bad.append((c.label + " tk", et, bt))
    assert not bad, _report(bad, solver + " tk, sk")


def test_literal_loop_where_it_applies(oracle, record_property):
    """icp_kernels.cl:1012-1041 as written: only a dominant positive eigenvalue (lambda1 >= 1.5 |lambda4|), a clear gap (>= 0.1) and a
    first component to divide by (|q64_0| >= 0.05) are in its reach.  On the rest its misses are data (record_property), not a pass."""
    bad, applies, missed = [], 0, []
    for c in rc.cases():
        if not c.unique or not c.in_range("literal"):
            continue
        q, _, _, it = _solve(oracle, c, "literal")
        e, b = rc.quat_error(q, c.q), rc.quat_bound(c)
        if rc.literal_applies(c):
            applies += 1
            if not e <= b:
                bad.append((c.label + " trips %d" % it, e, b))
        elif not e <= b:
            missed.append(c.label)
    assert applies >= 20 and not bad, _report(bad, "literal |q - q64|")
    record_property("literal_misses_outside_its_reach", len(missed))


def test_rot_to_quat_on_all_four_branches(oracle):
    """orc_rot_to_quat (Eigen's matrix -> quaternion) on float32 rotations against the float64 quaternion of the same matrix: both
    branches, and each largest diagonal of the trace <= 0 branch, many times each.  Both branches take a root of at least 1, so the
    result is good to a few ulps."""
    r = np.random.default_rng(0xA7)
    qs = r.normal(size=(4000, 4))
    qs = np.r_[qs, np.eye(4), np.c_[r.normal(size=(200, 3)), np.zeros(200)]]            # (180 degree turns: w = 0)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    seen, bad = {}, []
    for q in qs:
        R = ref.quat_to_rot(q).astype(np.float32)
        b = rc.rot_branch(R)
        seen[b] = seen.get(b, 0) + 1
        got = oracle.rot_to_quat(R).astype(np.float64)
        want = ref.rot_to_quat(R.astype(np.float64))
        e = min(np.linalg.norm(got - want), np.linalg.norm(got + want))
        if not e <= 16 * EPS32:
            bad.append((str(b), e, 16 * EPS32))
    assert min(seen.get(b, 0) for b in ("w", 0, 1, 2)) >= 300, seen
    assert not bad, _report(bad, "rot_to_quat")
