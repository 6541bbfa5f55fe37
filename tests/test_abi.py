"""CPU tests of the drop-in boundary: libmrbf.so loads, exports exactly what include/mrbf.h declares,
the ctypes table binds the same set, and without a GPU every compute path fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu


def header_symbols():
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mrbf_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    import morbit.jl_amd as pkg

    declared = header_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), "libmrbf.so does not export %s" % name
    assert sorted(pkg._lib.SIGNATURES) == declared
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH]).decode()
    for name in declared:
        assert re.search(r"\bT %s\b" % name, exported), name


def test_struct_layouts_match_header():
    from morbit.jl_amd import _lib

    assert ctypes.sizeof(_lib.FitInfo) == 4 * 4 + 3 * 8 + 6 * 4 + 2 * 4 + 2 * 4 == 80
    assert ctypes.sizeof(_lib.EvalInfo) == 16
    assert ctypes.sizeof(_lib.Problem) == 2 * 8 + 4 * 4 + 2 * 8 + 7 * 8 == 104
    assert _lib.Result.fit.offset == 8
    assert ctypes.sizeof(_lib.PsOptions) == 40 and ctypes.sizeof(_lib.PsInfo) == 32 and _lib.PsInfo.tau.offset == 24
    assert ctypes.sizeof(_lib.Result) == 8 + 80 + 8 + 16
    assert ctypes.sizeof(_lib.PsProblem) == 72 and _lib.PsProblem.eq_tol.offset == 64 and _lib.PsProblem.n_lin_eq.offset == 24


def test_version_and_no_cpu_fallback(lib):
    assert b"gfx950" in lib.mrbf_version()
    if has_gpu():
        pytest.skip("GPU present: the no-device error path is not reachable")
    import morbit.jl_amd as pkg

    with pytest.raises(pkg.MrbfError) as ei:
        pkg.Context()
    assert ei.value.code == pkg._lib.MRBF_ENODEVICE
    assert "no CPU path" in str(ei.value)
    with pytest.raises(pkg.MrbfError):
        pkg.update_model(pkg.RbfConfig(), np.zeros((4, 2)), np.zeros((4, 1)))
    res = (pkg._lib.Result * 1)()
    prob = (pkg._lib.Problem * 1)()
    assert lib.mrbf_batch_run(1, None, 1, prob, res) == pkg._lib.MRBF_ENODEVICE
    assert lib.mrbf_fit(None, 1, 1, 1, None, None, 0, 3.0, 0.0, 1, None, None, None, None) == -1


def test_product_package_never_imports_the_oracle():
    pkg_dir = os.path.join(ROOT, "morbit.jl_amd")
    for base, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".jl", ".cpp", ".h")):
                src = open(os.path.join(base, f), errors="ignore").read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
                assert "librbf_oracle" not in src, f


def test_no_lds_dma_inside_lane_dependent_control_flow():
    """Source rule of round 5 (csrc/mega_gemm.hpp, profiles/r05_ldsdma_hazard.txt): the LDS base of an LDS-DMA travels in M0 and must be
    wave-uniform; a half-wave LDS-DMA under `if (lane < 32)` was merged by the compiler with the full-wave ones behind a non-uniform
    base (v_readfirstlane into M0) and put rows 64..127 of the B operand at the wrong LDS address.  No line of the product issues an
    LDS-DMA under a condition on the lane index (wave-uniform conditions are fine)."""
    import glob
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "morbit.jl_amd", "csrc")
    dma = re.compile(r"\bglds16\s*(<[^>]*>)?\s*\(|__builtin_amdgcn_global_load_lds\s*\(")
    offenders = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            code = line.split("//")[0]
            if not dma.search(code) or "__device__" in code:
                continue
            # the statement itself, or the `if (...)` line right above it, must not test the lane index
            ctx = code + " " + (lines[i - 1].split("//")[0] if i > 0 and lines[i - 1].strip().startswith("if") else "")
            m = re.search(r"if\s*\(([^)]*)\)", ctx)
            if m and re.search(r"\blane\b|\btid\b|threadIdx", m.group(1)):
                offenders.append("%s:%d: %s" % (os.path.basename(path), i + 1, line.strip()))
    assert not offenders, "LDS-DMA under a lane-dependent condition:\n" + "\n".join(offenders)


def test_environment_switches_sit_behind_one_gate(lib):
    """VERDICT r5 hygiene: some seventy MRBF_* environment switches select schedule experiments and earlier kernel forms.  A drop-in
    library must not change algorithm on a stray variable: every read goes through mrbf_env() (csrc/common.hpp), which answers only
    while MRBF_EXPERIMENTS=1 is set.  Pinned: the gate's behaviour (host-only hook) and that no source file reads an MRBF_* variable
    any other way."""
    import glob

    keep = {k: os.environ.get(k) for k in ("MRBF_EXPERIMENTS", "MRBF_PS_MULTI")}
    try:
        os.environ["MRBF_PS_MULTI"] = "0"
        os.environ.pop("MRBF_EXPERIMENTS", None)
        assert lib.mrbf_debug_env(b"MRBF_PS_MULTI") == 0            # set, but the gate is closed: ignored
        os.environ["MRBF_EXPERIMENTS"] = "0"
        assert lib.mrbf_debug_env(b"MRBF_PS_MULTI") == 0
        os.environ["MRBF_EXPERIMENTS"] = "1"
        assert lib.mrbf_debug_env(b"MRBF_PS_MULTI") == 1            # gate open: honoured
        assert lib.mrbf_debug_env(b"MRBF_NO_SUCH_SWITCH") == 0
        assert lib.mrbf_debug_env(None) == -1
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    csrc = os.path.join(ROOT, "morbit.jl_amd", "csrc")
    raw, gated = [], 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        for i, line in enumerate(open(path).read().split("\n")):
            code = line.split("//")[0]
            gated += len(re.findall(r"\bmrbf_env\(\"MRBF_", code))
            for m in re.finditer(r"(?<![_\w])(?:std::)?getenv\(\s*\"?([A-Za-z_]*)", code):
                if not (os.path.basename(path) == "common.hpp" and m.group(1) in ("MRBF_EXPERIMENTS", "name")):
                    raw.append("%s:%d: %s" % (os.path.basename(path), i + 1, line.strip()))
    assert not raw, "environment read outside the gate:\n" + "\n".join(raw)
    assert gated >= 97  # (104 before the diagonal block's retired v4 core left with its seven reads)
    # every switch is listed in INTEGRATION.md's appendix (regenerate it when one is added: the list is what a maintainer greps)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = set()
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        names.update(re.findall(r"mrbf_env\(\"(MRBF_[A-Z0-9_]+)\"\)", open(path).read()))
    missing = sorted(n for n in names if ("`%s`" % n) not in doc)
    assert not missing, "switches missing from INTEGRATION.md's appendix: %s" % missing
    # ... and the appendix lists nothing that the sources no longer read (a switch that was retired leaves the list with its code)
    listed = set(re.findall(r"^\| `(MRBF_[A-Z0-9_]+)` \|", doc[doc.index("## Appendix: every environment switch"):], flags=re.M))
    stale = sorted(listed - names)
    assert not stale, "INTEGRATION.md's appendix lists switches that no source reads: %s" % stale
