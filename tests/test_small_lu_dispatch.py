"""CPU tests of the one-launch LU's switch (MRBF_OPT_SMALL_LU) and of its decision-table row: the option's key and values as the header,
the library source and the bindings state them; mrbf_dispatch_fit_batch_lu's refusals, its monotonicity in n_lu_starts and its admitted
cells pinned at what DESIGN.md section 12 records; header <-> export <-> ctypes for the new names; and `rbf_model.update_models_many`
counting the LU-path starts, asking the table and raising the option around its one mrbf_fit_batch call and putting it back, also when
the call raises.  No GPU needed: the device call is a test double."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu

# the committed rule (csrc/dispatch.hip, FIT_LU): from so many LU-path starts on, the batch is admitted up to so many sites and that
# dimension; DESIGN.md section 12 has the measurement.  Rows ascending in all three columns.
ROWS = [(8, 512, 128)]


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts), encoding="utf-8").read()


def _rule(ns, n_max, d):
    if not (1 <= ns <= 65535 and 1 <= n_max <= 512 and 1 <= d <= 128):
        return 0
    for lo, max_n, max_d in reversed(ROWS):
        if ns >= lo:
            return int(n_max <= max_n and d <= max_d)
    return 0


def test_option_key_values_and_names(lib):
    from morbit.jl_amd import _lib

    assert _lib.OPT_SMALL_LU == 16 and (_lib.SMALL_LU_MAX_N, _lib.SMALL_LU_MAX_D, _lib.SMALL_LU_MAX_K) == (512, 128, 16)
    hdr = _read("include", "mrbf.h")
    assert re.search(r"MRBF_OPT_SMALL_LU = 16\b", hdr)
    assert "int32_t mrbf_dispatch_fit_batch_lu(int64_t n_lu_starts, int64_t n_max, int32_t d);" in hdr
    assert re.search(r"\*   mrbf_dispatch_fit_batch_lu\b", hdr)
    assert re.search(r"int small_lu = 0;", _read("morbit.jl_amd", "csrc", "common.hpp"))
    src = _read("morbit.jl_amd", "csrc", "context.hip")
    case = re.search(r"case MRBF_OPT_SMALL_LU:(.*?)break;", src, flags=re.S).group(1)
    assert case.index("return fail(ctx, -2,") < case.index("ctx->small_lu = v")      # checked before anything is stored
    # the range the bindings count LU starts by is the one the library applies
    applies = re.search(r"bool small_lu_applies\(.*?\n}", _read("morbit.jl_amd", "csrc", "small_lu.hip"), flags=re.S).group(0)
    assert "n <= 512" in applies and "d <= 128" in applies and "k <= 16" in applies and "n >= q" in applies and "!kp_nonsmooth(kp)" in applies
    # export and ctypes
    assert _lib.SIGNATURES["mrbf_dispatch_fit_batch_lu"][0].__name__ == "c_int" or _lib.SIGNATURES["mrbf_dispatch_fit_batch_lu"][0].__name__ == "c_int32"
    assert len(_lib.SIGNATURES["mrbf_dispatch_fit_batch_lu"][1]) == 3
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT mrbf_dispatch_fit_batch_lu\b", exported)
    jl = _read("morbit.jl_amd", "julia", "HipRbf.jl")
    assert re.search(r"ccall\(\(:mrbf_dispatch_fit_batch_lu, libmrbf\), Int32, \(Int64, Int64, Int32\),", jl)
    # no context: the same answer as for every other key
    assert lib.mrbf_set_option(None, 16, 1.0) == -1
    if not has_gpu():
        return
    import morbit.jl_amd as pkg

    c = pkg.Context()
    try:
        assert c.get_option(16) == 0
        c.set_option(16, 1)
        for bad in (2.0, -1.0, 0.5):
            assert lib.mrbf_set_option(c.h, 16, bad) == -2 and c.get_option(16) == 1
    finally:
        c.close()


def test_decision_table_row(lib):
    f = lib.mrbf_dispatch_fit_batch_lu
    for ns in (0, -1, -(2 ** 40), 65536):
        assert f(ns, 33, 16) == 0
    for n_max in (0, -3, 513, 2 ** 40):
        assert f(64, n_max, 16) == 0
    for d in (0, -1, 129, 4096):
        assert f(64, 33, d) == 0
    shapes = [(1, 1), (33, 16), (33, 17), (34, 16), (257, 128), (512, 128), (512, 3), (100, 64)]
    for n_max, d in shapes:
        vals = [f(ns, n_max, d) for ns in list(range(1, 200)) + [1000, 32767, 65535]]
        assert all(v in (0, 1) for v in vals)
        assert all(a <= b for a, b in zip(vals, vals[1:])), (n_max, d)          # monotone in n_lu_starts
        for ns in (1, 7, 8, 15, 16, 63, 64, 65535):
            assert f(ns, n_max, d) == _rule(ns, n_max, d), (ns, n_max, d)
    # the admitted cells are the ones DESIGN.md section 12 records
    design = _read("DESIGN.md")
    row = re.search(r"Admitted \(`FIT_LU`\): (.*)", design).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"from (\d+) starts on up to n = (\d+), d = (\d+)", row)] == ROWS


def test_takes_small_lu_mirrors_fit_model():
    from morbit.jl_amd import rbf_model as rm

    t = rm._takes_small_lu
    assert t(3, 2.0, 0.0, 1, 40, 3, 2) and t(0, 5.0, 0.0, 1, 40, 3, 2) and t(0, 3.0, 0.0, 0, 40, 3, 2) and t(0, 3.0, 0.0, -1, 40, 3, 2)
    assert t(2, 1.0, 0.5, -1, 40, 3, 2) and t(0, 3.0, 0.0, 1, 4, 3, 1)               # ... and n == q
    assert not t(0, 3.0, 0.0, 1, 40, 3, 2) and not t(2, 1.0, 0.5, 0, 40, 3, 2) and not t(4, 1.0, 0.0, -1, 40, 3, 2)   # Cholesky paths
    assert not t(0, 1.0, 0.0, -1, 40, 3, 2) and not t(3, 1.0, 0.0, 0, 40, 3, 2)      # nonsmooth kernels
    assert not t(3, 2.0, 0.0, 1, 3, 3, 2)                                            # n < q: minimum norm
    assert not t(3, 2.0, 0.0, 1, 513, 3, 2) and not t(3, 2.0, 0.0, 1, 200, 129, 2) and not t(3, 2.0, 0.0, 1, 40, 3, 17)


class _Lib:
    """the real decision table, its LU row replaced by `admit`, around a device call that records the options it runs under"""

    def __init__(self, real, owner, admit, raises=False):
        self.real, self.owner, self.admit, self.raises = real, owner, admit, raises
        self.asked, self.ran_under = [], []

    def mrbf_dispatch_fit_batch(self, ns):
        return self.real.mrbf_dispatch_fit_batch(ns)

    def mrbf_dispatch_fit_batch_max_n(self, ns, d):
        return self.real.mrbf_dispatch_fit_batch_max_n(ns, d)

    def mrbf_dispatch_fit_batch_lu(self, ns, n_max, d):
        self.asked.append((ns, n_max, d))
        return self.admit if self.admit is not None else self.real.mrbf_dispatch_fit_batch_lu(ns, n_max, d)

    def mrbf_dispatch_after(self, entry, rc):
        return self.real.mrbf_dispatch_after(entry, rc)

    def mrbf_fit_batch(self, h, ns, jobs, ms):
        self.ran_under.append(dict(self.owner.options))
        if self.raises:
            raise RuntimeError("the device call raised")
        for p in range(ns):
            jobs[p].status, jobs[p].model = 0, 1000 + p
        return 0


class _Ctx:
    def __init__(self, real, admit, raises=False, lu_at=0):
        self.options, self.sets, self.h = {15: 512, 16: lu_at}, [], None
        self.lib = _Lib(real, self, admit, raises)

    def check(self, rc):
        assert rc == 0

    def get_option(self, key):
        return float(self.options[key])

    def set_option(self, key, value):
        self.sets.append((key, value))
        self.options[key] = int(value)


def _starts(ns_and_d):
    rng = np.random.default_rng(0)
    sites = [rng.standard_normal((n, d)) for n, d in ns_and_d]
    return sites, [rng.standard_normal((s.shape[0], 2)) for s in sites]


def _release(mods):
    for m in mods:
        if m is not None:
            m.model = None      # (handles of the test double: nothing to release)


def test_update_models_many_raises_and_restores_the_option(lib):
    from morbit.jl_amd import rbf_model as rm

    tps, cub = rm.RbfConfig(kernel="thin_plate_spline"), rm.RbfConfig()
    sites, vals = _starts([(40, 3), (60, 3), (600, 3), (33, 3)])
    cfgs = [tps, tps, tps, cub]                   # two LU starts in range, one beyond it (n = 600), one Cholesky start
    ctx, stats = _Ctx(lib, 1), {}
    mods = rm.update_models_many(cfgs, sites, vals, 1.0, ctx=ctx, stats=stats)
    assert ctx.lib.asked == [(2, 60, 3)] * 2 and ctx.lib.ran_under == [{15: 512, 16: 1}] and ctx.sets == [(16, 1), (16, 0.0)]
    assert ctx.options[16] == 0 and stats["path"] == "batch" and stats["lu"] == 2 and stats["wide"] == 0 and len(mods) == 4
    _release(mods)
    # a context whose option the caller had set himself keeps HIS value
    ctx, stats = _Ctx(lib, 1, lu_at=1), {}
    _release(rm.update_models_many(cfgs, sites, vals, 1.0, ctx=ctx, stats=stats))
    assert ctx.options[16] == 1 and stats["lu"] == 2
    # the call raises: the option is back all the same
    ctx = _Ctx(lib, 1, raises=True)
    with pytest.raises(RuntimeError):
        rm.update_models_many(cfgs, sites, vals, 1.0, ctx=ctx)
    assert ctx.lib.ran_under == [{15: 512, 16: 1}] and ctx.options[16] == 0
    # the table refuses: nothing is set
    ctx, stats = _Ctx(lib, 0), {}
    _release(rm.update_models_many(cfgs, sites, vals, 1.0, ctx=ctx, stats=stats))
    assert ctx.sets == [] and ctx.lib.ran_under == [{15: 512, 16: 0}] and stats["lu"] == 0
    # no LU start: the table is not even asked
    ctx, stats = _Ctx(lib, 1), {}
    _release(rm.update_models_many(cub, sites, vals, 1.0, ctx=ctx, stats=stats))
    assert ctx.lib.asked == [] and ctx.sets == [] and stats["lu"] == 0
    # the committed rule through the binding
    for ns in (4, 8, 64):
        s2, v2 = _starts([(33, 16)] * ns)
        ctx, stats = _Ctx(lib, None), {}
        _release(rm.update_models_many(tps, s2, v2, 1.0, ctx=ctx, stats=stats))
        want = _rule(ns, 33, 16)
        assert ctx.lib.ran_under == [{15: 512, 16: want}] and ctx.options[16] == 0 and stats["lu"] == (ns if want else 0)
