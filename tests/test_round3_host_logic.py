"""The host logic of the batched round 3 (morbit.jl_amd/csrc/round3_host.hpp) on the CPU: tools/round3_host_check.cpp enumerates small
cases of a start's row counts, the validation of a batch's jobs, the reservation rule and the layout (no row offset outside its
reservation, no overlapping staging blocks) and judges every result by statements made from the header's text.  The header needs
neither HIP nor the library: the program is a stand-alone executable built with the plain C++ compiler under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round3_host_logic(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    exe = str(tmp_path / "round3_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tools", "round3_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "round3_host_check: ok" in res.stdout
