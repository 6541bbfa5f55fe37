"""The host logic of the affine batch and of the round-4 batch (morbit.jl_amd/csrc/affine_host.hpp, round4_host.hpp) on the CPU:
tools/select_host_check.cpp enumerates small batches -- the validation of the jobs, the pick counts, the routing of every start and the
layout of each call's arena -- and judges every result by statements made directly from the headers' comments and include/mrbf.h.  The
headers need neither HIP nor the library: the program is a stand-alone executable built with the plain C++ compiler under
AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "select_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "select_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "select_host_check: ok" in res.stdout
