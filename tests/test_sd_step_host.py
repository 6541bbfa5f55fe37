"""CPU tests of the steepest-descent step's host side (no GPU needed): the decision table mrbf_dispatch_sd_step with every limit edge,
mrbf_dispatch_after for MRBF_ENTRY_SD_STEP, the ctypes structs against include/mrbf.h, and the Julia binding at source level (Julia
is not installed here, so hip_compute_descent_step is pinned from its text)."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT

JL = os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl")
HDR = os.path.join(ROOT, "include", "mrbf.h")


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


# (d, k, n_models, n_nl, n_lin, n_foreign, max_loops) -> device?
ROWS = [
    ((2, 2, 1, 0, 0, 0, 10), 1),
    ((2, 2, 3, 1, 1, 0, 117), 1),
    ((2, 2, 1, 0, 0, 1, 10), 0),       # a foreign objective / modelled row
    ((2, 2, 2, 1, 0, 3, 10), 0),
    ((2, 2, 0, 0, 0, 0, 10), 0),       # no device model
    ((0, 2, 1, 0, 0, 0, 10), 0),
    ((1, 2, 1, 0, 0, 0, 10), 1),
    ((4096, 2, 1, 0, 0, 0, 10), 1),
    ((4097, 2, 1, 0, 0, 0, 10), 0),
    ((2, 0, 1, 0, 0, 0, 10), 0),
    ((2, 1, 1, 0, 0, 0, 10), 1),
    ((2, 64, 1, 0, 0, 0, 10), 1),
    ((2, 65, 1, 0, 0, 0, 10), 0),
    ((2, 2, 1, 256, 0, 0, 10), 1),
    ((2, 2, 1, 0, 256, 0, 10), 1),
    ((2, 2, 1, 128, 128, 0, 10), 1),
    ((2, 2, 1, 129, 128, 0, 10), 0),
    ((2, 2, 1, 0, 257, 0, 10), 0),
    ((2, 2, 1, -1, 0, 0, 10), 0),
    ((2, 2, 1, 0, -1, 0, 10), 0),
    ((2, 2, 1, 0, 0, 0, -1), 0),
    ((2, 2, 1, 0, 0, 0, 0), 1),
    ((2, 2, 1, 0, 0, 0, 1024), 1),
    ((2, 2, 1, 0, 0, 0, 1025), 0),
]


@pytest.mark.parametrize("args,want", ROWS)
def test_decision_table(lib, args, want):
    assert lib.mrbf_dispatch_sd_step(*args) == want, args


def test_dispatch_after(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_SD_STEP == 8
    assert lib.mrbf_dispatch_after(_lib.ENTRY_SD_STEP, -2) == 1
    for rc in (0, -1, -3, -8, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
        assert lib.mrbf_dispatch_after(_lib.ENTRY_SD_STEP, rc) == 0, rc
    # the other entries keep their rules
    assert lib.mrbf_dispatch_after(_lib.ENTRY_SD, -2) == 1 and lib.mrbf_dispatch_after(_lib.ENTRY_NORMAL, -2) == 1
    assert lib.mrbf_dispatch_after(_lib.ENTRY_BACKTRACK, -2) == 0


def test_no_context_is_an_error(lib):
    from morbit.jl_amd import _lib

    opts = _lib.SdStepOptions(strict=1, max_loops=3, const_rhs=1e-6, shrink=0.75, min_stepsize=1e-15)
    info = _lib.SdStepInfo()
    assert lib.mrbf_sd_step(None, None, None, None, 0.5, None, None, 0.1, None, ctypes.byref(opts), None, None, ctypes.byref(info)) == -1


_C_TYPES = {"int32_t": (4, ctypes.c_int32), "float": (4, ctypes.c_float), "double": (8, ctypes.c_double)}


def _header_struct(name):
    """fields (name, size, ctype) of a `typedef struct { ... } name;` of include/mrbf.h, comments stripped"""
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            fields.append((n.strip(), _C_TYPES[ctype][0], _C_TYPES[ctype][1]))
    return fields


@pytest.mark.parametrize("hname,pyname,size", [("mrbf_sd_step_options", "SdStepOptions", 32), ("mrbf_sd_step_info", "SdStepInfo", 40)])
def test_ctypes_structs_match_the_header(hname, pyname, size):
    from morbit.jl_amd import _lib

    ct = getattr(_lib, pyname)
    fields = _header_struct(hname)
    assert [f[0] for f in ct._fields_] == [f[0] for f in fields]
    off = 0
    for (fname, fsize, ctype), (cname, cct) in zip(fields, ct._fields_):
        off = (off + fsize - 1) // fsize * fsize
        assert getattr(ct, cname).offset == off, (hname, fname)
        assert ctypes.sizeof(cct) == fsize and cct == ctype, (hname, fname)
        off += fsize
    assert ctypes.sizeof(ct) == size == (off + 7) // 8 * 8


def test_julia_struct_mirrors():
    from morbit.jl_amd import _lib
    from tests.test_julia_binding import _jl_struct_layout

    src = open(JL, encoding="utf-8").read()
    for jl_name, ct in (("MrbfSdStepOptions", _lib.SdStepOptions), ("MrbfSdStepInfo", _lib.SdStepInfo)):
        layout, total = _jl_struct_layout(src, jl_name)
        assert total == ctypes.sizeof(ct), jl_name
        assert list(layout) == [f[0] for f in ct._fields_], jl_name
        for fname, _ in ct._fields_:
            assert layout[fname] == getattr(ct, fname).offset, (jl_name, fname)


def test_julia_binding_routes_the_step():
    src = open(JL, encoding="utf-8").read()
    assert "(:mrbf_sd_step, libmrbf)" in src and "(:mrbf_dispatch_sd_step, libmrbf)" in src
    assert len(re.findall(re.escape("_dispatch_sd_step("), src)) >= 2          # definition + use
    assert "_fallback_rc(8" in src
    m = re.search(r"^function hip_compute_descent_step\((.*?)^end", src, flags=re.S | re.M)
    assert m, "hip_compute_descent_step is missing"
    body = m.group(0)
    assert body.startswith("function hip_compute_descent_step(desc_cfg::SteepestDescentConfig, mop, scal, x_it, x_it_n, data_base, "
                           "sc::SurrogateContainer,")
    assert "error(" not in body
    assert re.search(r"reference\(\) = compute_descent_step\(desc_cfg, mop, scal, x_it, x_it_n, data_base, sc, algo_config, ω, d\)", body)
    # the guard comes first, then the plan, the table, the locked call and the fallback test, in this order
    order = [body.index(s) for s in ("_touches_device(sc) || return reference()", "_container_plan(sc)", "_dispatch_sd_step(",
                                     "_locked(ctx) do hctx", "ccall((:mrbf_sd_step, libmrbf)", "_fallback_rc(8, rc)")]
    assert order == sorted(order), order
    # a function of its own, not a method of Morbit's compute_descent_step
    assert not re.search(r"^(function\s+)?compute_descent_step\(", src, flags=re.M)
