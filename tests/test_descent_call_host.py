"""CPU test of what the direction calls share on the host (morbit.jl_amd/csrc/descent_call_host.hpp): the launch chunk rule, the
staging layout of the *_direction entries' outputs and the packed input block of the single-start calls, driven by
tools/descent_call_host_check.cpp -- a stand-alone program under AddressSanitizer and UBSan, run as a child process.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "morbit.jl_amd", "csrc")


def test_descent_call_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "descent_call_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "descent_call_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "descent_call_host_check: ok" in res.stdout


def test_host_header_includes_no_hip():
    text = open(os.path.join(CSRC, "descent_call_host.hpp")).read()
    assert not re.search(r"#include\s*[<\"](hip|rocblas|common\.hpp)", text)

