"""CPU tests of the Pascoletti-Serafini step's host part (morbit.jl_amd/csrc/ps_host.hpp): the refinement's state machine, the
proximal weights, the constraint violation, the sizes of a start's state and the budgets, driven on analytic functions by
tools/ps_host_check.cpp -- a stand-alone program under AddressSanitizer and UBSan, run as a child process.  No GPU, no library."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_ps_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "ps_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "ps_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "ps_host_check: ok" in res.stdout


def test_host_header_includes_no_hip_and_the_solver_uses_it():
    text = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ps_host.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower()
    src = open(os.path.join(ROOT, "morbit.jl_amd", "csrc", "ps_solver.hip")).read()
    assert '#include "ps_host.hpp"' in src
    # what moved lives in one place: the limits, the problem, the refinement and the sizes are the header's alone
    for moved in ("constexpr int MAXRUNS", "struct Problem {", "struct Descent {", "void prox_weights(", "struct Sizes {"):
        assert moved in text and moved not in src, moved
    assert src.count("ps::sizes(") == 1 and src.count(" sizes(d, k, with_ideal, with_ps)") == 1     # the chunk sizing and the arena
