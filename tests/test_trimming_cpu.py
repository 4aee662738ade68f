"""Trimmed ICP without a device: argument validation of the C-ABI, the header as C, the C++ facade's and ICPReg's setters, both
command lines, and the compiler's resources of the new kernels.  (tests/test_gpu_trimming.py checks what the option does.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

from kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


def test_invalid_fractions_are_refused_with_a_message(L):
    for keep in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert L.icp_set_trimming(None, keep) == 1, keep                      # ICP_EINVAL
        assert "keep_fraction" in L.icp_last_error(None).decode(), keep
    for keep in (1e-6, 0.5, 0.8, 1.0):                                        # valid on no handle: still EINVAL (nothing to set)
        assert L.icp_set_trimming(None, keep) == 1
        assert "null handle" in L.icp_last_error(None).decode()
    f = C.c_float()
    assert L.icp_get_trimming(None, C.byref(f)) == 1
    assert L.icp_batch_set_trimming(None, 0.8) == 1


def test_memory_enum(engine):
    assert engine.Memory.TRIM == 20
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert "ICP_MEM_TRIM = 20," in hdr and hdr.index("ICP_MEM_TRIM = 20,") < hdr.index("ICP_MEM_COUNT_")


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b) {\n'
           '    float keep; uint32_t trim[4];\n'
           '    if (icp_set_trimming (h, 0.8f)) return 1;\n'
           '    if (icp_get_trimming (h, &keep)) return 1;\n'
           '    if (icp_read (h, ICP_MEM_TRIM, trim, sizeof trim)) return 1;\n'
           '    return icp_batch_set_trimming (b, keep);\n'
           '}\n')
    _compile(tmp_path, "trim.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'float f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
           '         ICPReg<ICPStepConfigT::EIGEN, ICPStepConfigW::REGULAR> &app) {\n'
           '    reg.setTrimming (0.8f); app.setTrimming (0.7f);\n'
           '    return reg.getTrimming () + app.getTrimming ();\n'
           '}\n')
    _compile(tmp_path, "trim.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_option():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--trim" in r.stdout
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--trim", "1.5"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--trim" in r.stderr, r.stderr


def test_example_command_line_accepts_the_option():
    """examples/registration (built by build()): --trim is an option of its own (not 'unknown option'), its value is checked before
    anything touches a device."""
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    r = subprocess.run([exe, "--trim", "1.5"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--trim: FRACTION must be in (0, 1]" in r.stderr, r.stderr
    r = subprocess.run([exe, "--trim", "0"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--trim" in r.stderr, r.stderr
    r = subprocess.run([exe, "--bogus"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "unknown option" in r.stderr


def test_trim_kernels_have_zero_scratch():
    res = dict(kernel_resources("icp_amd/csrc/icp_trim.hip"))
    names = sorted(n for n in res if n.startswith("k_trim_"))
    assert names == ["k_trim_apply<false>", "k_trim_apply<true>", "k_trim_select", "k_trim_select_pass<0>", "k_trim_select_pass<1>",
                     "k_trim_select_pass<2>"], names
    for n in names:
        assert res[n]["scratch"] == 0 and res[n]["dynamic_stack"] == "False", (n, res[n])
