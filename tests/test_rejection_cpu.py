"""Correspondence rejection without a device: argument validation of the C-ABI, the header as C, the C++ facade's and ICPReg's
setters, the command line.  (tests/test_gpu_rejection.py checks what the option does.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(engine):
    return engine.lib()


def test_invalid_arguments_are_refused_with_a_message(L):
    for flags, md, what in [(2, 0.0, "unknown flag bits"), (-1, 0.0, "unknown flag bits"), (1, -1.0, "max_dist"),
                            (0, float("nan"), "max_dist"), (0, -float("inf"), "max_dist")]:
        assert L.icp_set_rejection(None, flags, md) == 1, (flags, md)          # ICP_EINVAL
        assert what in L.icp_last_error(None).decode(), (flags, md)
    # valid arguments on no handle: still EINVAL (nothing to set)
    for flags, md in [(0, 0.0), (1, 0.0), (1, 60.0), (0, float("inf"))]:
        assert L.icp_set_rejection(None, flags, md) == 1
        assert "null handle" in L.icp_last_error(None).decode()
    f, d = C.c_int(), C.c_float()
    assert L.icp_get_rejection(None, C.byref(f), C.byref(d)) == 1
    assert L.icp_batch_set_rejection(None, 1, 60.0) == 1


def test_python_argument_mapping(engine):
    assert engine.REJECT_INVALID == 1
    assert engine._max_dist_arg(None) == 0.0 and engine._max_dist_arg(60) == 60.0


def _compile(tmp_path, name, src, cmd):
    p = tmp_path / name
    p.write_text(src)
    r = subprocess.run(cmd + [str(p)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_header_compiles_as_c(tmp_path):
    src = ('#include "icp_amd.h"\n'
           'int f (icp_handle h, icp_batch_handle b) {\n'
           '    int fl; float md;\n'
           '    if (icp_set_rejection (h, ICP_REJECT_INVALID, 60.0f)) return 1;\n'
           '    if (icp_get_rejection (h, &fl, &md)) return 1;\n'
           '    return icp_batch_set_rejection (b, fl, md);\n'
           '}\n')
    _compile(tmp_path, "rej.c", src, ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-Iinclude"])


def test_facade_and_icpreg_expose_the_setting(tmp_path):
    src = ('#include <ocl_icp_reg.hpp>\n'
           'using namespace cl_algo::ICP;\n'
           'void f (ICP<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::WEIGHTED> &reg,\n'
           '        ICPReg<ICPStepConfigT::POWER_METHOD, ICPStepConfigW::REGULAR> &app) {\n'
           '    int fl; float md;\n'
           '    reg.setRejection (ICP_REJECT_INVALID, 60.f); reg.getRejection (fl, md);\n'
           '    app.setRejection (ICP_REJECT_INVALID); app.getRejection (fl, md);\n'
           '}\n')
    _compile(tmp_path, "rej.cpp", src, ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-Iinclude"])


def test_register_command_line_has_the_options():
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--reject-invalid" in r.stdout and "--max-dist" in r.stdout
