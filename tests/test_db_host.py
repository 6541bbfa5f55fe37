"""The host logic of the resident site database (morbit.jl_amd/csrc/db_host.hpp) on the CPU: tools/db_host_check.cpp enumerates small
cases of the capacity rule, the exclusion-mask builder, the validation of a batch's jobs and the layout of a batch's views, upload,
read-back and scratch, and judges every result by statements made directly from the header's text.  The header needs neither HIP nor
the library: the program is a stand-alone executable built with the plain C++ compiler under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_db_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "db_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "db_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "db_host_check: ok" in res.stdout
