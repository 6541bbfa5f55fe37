"""The one reader of a container's roles table (morbit.jl_amd/csrc/descent_problem.hpp) on the CPU: tools/descent_problem_check.cpp
enumerates the tables of up to 3 slots x 3 outputs with 0 .. 3 objectives and the slot defects, and judges every result by statements
made directly from the table as include/mrbf.h defines it (its header comment says which tables are enumerated in full).  The
header needs neither HIP nor the library: the program is compiled with the plain C++ compiler."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_descent_problem_reader(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "descent_problem_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tools", "descent_problem_check.cpp"),
                           "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "descent_problem_check: ok" in res.stdout
