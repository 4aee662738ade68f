"""One-to-one correspondences without a device: the header, the Python mirror, the command lines, argument validation on no handle,
the numpy rule of tests/unique_ref.py against a per-group loop, and the compiler's resources of the new kernels.
(tests/test_gpu_unique.py checks what the option does.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unique_ref as ref                                        # noqa: E402
from kernel_resources import kernel_resources                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_order():
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    a, b, c = hdr.index("ICP_MEM_NORMALS_M = 24,"), hdr.index("ICP_MEM_UNIQUE = 25,"), hdr.index("ICP_MEM_COUNT_")
    assert a < b < c


def test_functions_are_declared():
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    for decl in ("int icp_set_unique (icp_handle h, int on);", "int icp_get_unique (icp_handle h, int *on);",
                 "int icp_batch_set_unique (icp_batch_handle b, int on);"):
        assert decl in hdr, decl


def test_python_mirror(engine):
    assert engine.Memory.UNIQUE == 25
    assert engine._MEM_DTYPE[engine.Memory.UNIQUE] == (np.uint32, None)
    for cls in (engine.ICPStep, engine.ICPBatch):
        assert callable(cls.set_unique) and callable(cls.unique)


def test_arguments_on_no_handle(engine):
    L = engine.lib()
    for on in (2, -1, 7):
        assert L.icp_set_unique(None, on) == 1, on                            # ICP_EINVAL
        assert "0 or 1" in L.icp_last_error(None).decode(), on
    for on in (0, 1):                                                         # valid on no handle: still EINVAL (nothing to set)
        assert L.icp_set_unique(None, on) == 1
        assert "null handle" in L.icp_last_error(None).decode()
    v = C.c_int32()
    assert L.icp_get_unique(None, C.byref(v)) == 1
    assert L.icp_batch_set_unique(None, 1) == 1


def test_header_compiles_as_c_and_the_facades_expose_the_setting(tmp_path):
    c = tmp_path / "unique.c"
    c.write_text('#include "icp_amd.h"\n'
                 'int f (icp_handle h, icp_batch_handle b) {\n'
                 '    int on; uint32_t u[2];\n'
                 '    if (icp_set_unique (h, 1)) return 1;\n'
                 '    if (icp_get_unique (h, &on)) return 1;\n'
                 '    if (icp_read (h, ICP_MEM_UNIQUE, u, sizeof u)) return 1;\n'
                 '    return icp_batch_set_unique (b, on);\n'
                 '}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude", str(c)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "unique.cpp"
    cpp.write_text('#include <ocl_icp_reg.hpp>\n'
                   'using namespace cl_algo::ICP;\n'
                   'bool f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
                   '        ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
                   '    reg.setUnique (true); app.setUnique (false);\n'
                   '    return reg.getUnique () || app.getUnique ();\n'
                   '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude", str(cpp)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--one-to-one" in r.stdout


def test_example_command_line_accepts_the_option():
    """examples/registration (built by build()): --one-to-one is an option of its own; a bad value behind it is refused before
    anything touches a device."""
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    r = subprocess.run([exe, "--one-to-one", "--trim", "1.5"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "--trim" in r.stderr, r.stderr


def _brute(ids, g, cand):
    """The rule as a loop over the groups of equal id: the candidate with the smallest (geo bits, index) wins."""
    bits = np.ascontiguousarray(g, np.float32).view(np.uint32)
    win = np.zeros(len(ids), bool)
    for j in set(int(x) for x in ids):
        best = None
        for i in range(len(ids)):
            if ids[i] == j and cand[i] and (best is None or (int(bits[i]), i) < best):
                best = (int(bits[i]), i)
        if best is not None:
            win[best[1]] = True
    return win


@pytest.mark.parametrize("seed", range(6))
def test_rule_against_a_loop_over_the_groups(seed):
    rng = np.random.default_rng(1000 + seed)
    m = 97 + 31 * seed
    ids = rng.integers(0, max(m // 4, 3), m).astype(np.uint32)
    g = rng.choice(np.array([0.0, 0.25, 1.0, 1.0000001, 3.5, 1e-42, 7.0], np.float32), m)     # (few values: equal geo inside groups)
    cand = rng.random(m) > 0.25
    dead = int(ids[0])                                # a group whose only members are non-candidates
    cand[ids == dead] = False
    win, counts = ref.unique_from_keys(ids, g, cand)
    want = _brute(ids, g, cand)
    assert np.array_equal(win, want)
    assert counts[0] == np.count_nonzero(cand) and counts[1] == np.count_nonzero(want)
    assert not win[ids == dead].any() and not win[~cand].any()
    groups = set(int(x) for x in ids[cand])
    assert counts[1] == len(groups)                  # one winner per claimed fixed point
    tied = [j for j in groups if np.count_nonzero((ids == j) & cand & (g == g[(ids == j) & cand].min())) > 1]
    assert tied, "the draw has groups with equal geo"
    for j in tied:                                    # a tie goes to the lowest query index
        grp = np.flatnonzero((ids == j) & cand)
        assert np.flatnonzero(win & (ids == j))[0] == grp[g[grp] == g[grp].min()][0]


def test_rule_from_engine_style_outputs():
    """unique_rule: candidates are the pairs of weight != 0 with a finite geo; a pair of weight 0 or with a NaN / inf geo claims nothing."""
    PF = np.zeros((6, 4), np.float32); PM = np.zeros((6, 4), np.float32)
    PM[:, 0] = [1, 2, 0.5, np.inf, np.nan, 0.5]
    ids = np.array([3, 3, 3, 3, 3, 3], np.uint32)
    W0 = np.array([1, 1, 0, 1, 1, 1], np.float32)
    win, cand, counts = ref.unique_rule(ids, PF, PM, W0)
    assert cand.tolist() == [True, True, False, False, False, True]
    assert win.tolist() == [False, False, False, False, False, True] and counts.tolist() == [3, 1]
    W = ref.weights_after(W0, win, cand)
    assert W.tolist() == [0, 0, 0, 1, 1, 1]           # (non-candidates do not change)


def test_unique_kernels_have_zero_scratch():
    res = dict(kernel_resources("icp_amd/csrc/icp_unique.hip"))
    names = sorted(n for n in res if n.startswith("k_unique_"))
    assert names == ["k_unique_claim", "k_unique_resolve"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])
