"""CPU tests of the one-launch fit's opt-in ceiling (MRBF_OPT_SMALL_FIT_MAX_N): the option's key, default and range as the header,
the library source and the two bindings state them (on a machine with a GPU: as a context answers), the decision-table row
mrbf_dispatch_fit_batch_max_n pinned at its committed thresholds, and `rbf_model.update_models_many` raising the option around its
one mrbf_fit_batch call and putting it back, also when the call raises.  No GPU needed: the device call is a test double."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, has_gpu

# the committed rule: from so many starts on, the one-launch fit takes up to so many sites (rows ascending in both columns);
# DESIGN.md section 12 has the measurement they come from
THRESHOLDS = [(1, 512), (8, 1684), (16, 2048)]
MEASURED_D = (65, 100, 128)      # the padded dimension of the measurement; d <= 64 keeps the loop


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts), encoding="utf-8").read()


def test_option_key_default_and_range(lib):
    from morbit.jl_amd import _lib

    assert _lib.OPT_SMALL_FIT_MAX_N == 15 and _lib.SMALL_FIT_DEFAULT_MAX_N == 512
    assert re.search(r"MRBF_OPT_SMALL_FIT_MAX_N = 15\b", _read("include", "mrbf.h"))
    assert re.search(r"int small_fit_max_n = 512;", _read("morbit.jl_amd", "csrc", "common.hpp"))
    src = _read("morbit.jl_amd", "csrc", "context.hip")
    case = re.search(r"case MRBF_OPT_SMALL_FIT_MAX_N:(.*?)break;", src, flags=re.S).group(1)
    assert re.search(r"if \(!\(value >= 512\.0 && value <= 2048\.0\)\) return fail\(ctx, -2,", case)   # checked before anything is stored
    assert case.index("return fail") < case.index("ctx->small_fit_max_n = v")
    assert "n <= ctx->small_fit_max_n" in _read("morbit.jl_amd", "csrc", "small.hip")
    # no context: the same answer as for every other key
    assert lib.mrbf_set_option(None, 15, 1024.0) == -1
    if not has_gpu():
        return
    import morbit.jl_amd as pkg

    c = pkg.Context()
    try:
        assert c.get_option(15) == 512
        c.set_option(15, 2048)
        assert c.get_option(15) == 2048
        for bad in (511.0, 2049.0, 0.0, -5.0):
            assert lib.mrbf_set_option(c.h, 15, bad) == -2 and c.get_option(15) == 2048
    finally:
        c.close()


def test_decision_table_row_is_pinned(lib):
    f = lib.mrbf_dispatch_fit_batch_max_n
    for ns in (0, -1, -(2 ** 40), 65536):
        assert f(ns, 128) == 512
    for d in (0, -1, 1, 3, 64, 129, 4096):
        assert f(64, d) == 512
    for i, (lo, max_n) in enumerate(THRESHOLDS):
        hi = THRESHOLDS[i + 1][0] - 1 if i + 1 < len(THRESHOLDS) else 65535
        for d in MEASURED_D:
            assert f(lo, d) == max_n and f(hi, d) == max_n, (lo, hi, d)
    # monotone in n_starts, never outside the option's range
    for d in (3, 64, 65, 128):
        vals = [f(ns, d) for ns in range(1, 300)] + [f(ns, d) for ns in (1000, 32767, 65535)]
        assert all(512 <= v <= 2048 for v in vals)
        assert all(a <= b for a, b in zip(vals, vals[1:]))
    # the header documents the row and declares the function; the Julia binding calls it with the header's types
    hdr = _read("include", "mrbf.h")
    assert "int64_t mrbf_dispatch_fit_batch_max_n(int64_t n_starts, int32_t d);" in hdr
    assert re.search(r"\*   mrbf_dispatch_fit_batch_max_n\b", hdr)
    jl = _read("morbit.jl_amd", "julia", "HipRbf.jl")
    assert re.search(r"ccall\(\(:mrbf_dispatch_fit_batch_max_n, libmrbf\), Int64, \(Int64, Int32\),", jl)


class _Lib:
    """the real decision table, its wide row replaced by `max_n`, around a device call that records the option it runs under"""

    def __init__(self, real, owner, max_n, raises=False):
        self.real, self.owner, self.max_n, self.raises = real, owner, max_n, raises
        self.asked, self.ran_under = [], []

    def mrbf_dispatch_fit_batch(self, ns):
        return self.real.mrbf_dispatch_fit_batch(ns)

    def mrbf_dispatch_fit_batch_max_n(self, ns, d):
        self.asked.append((ns, d))
        return self.max_n if self.max_n is not None else self.real.mrbf_dispatch_fit_batch_max_n(ns, d)

    def mrbf_dispatch_after(self, entry, rc):
        return self.real.mrbf_dispatch_after(entry, rc)

    def mrbf_fit_batch(self, h, ns, jobs, ms):
        self.ran_under.append(self.owner.option)
        if self.raises:
            raise RuntimeError("the device call raised")
        for p in range(ns):
            jobs[p].status, jobs[p].model = 0, 1000 + p
        return 0


class _Ctx:
    def __init__(self, real, max_n, raises=False, start_at=512):
        self.option, self.sets, self.h = start_at, [], None
        self.lib = _Lib(real, self, max_n, raises)

    def check(self, rc):
        assert rc == 0

    def get_option(self, key):
        assert key == 15
        return float(self.option)

    def set_option(self, key, value):
        assert key == 15
        self.sets.append(value)
        self.option = int(value)


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

    cfg = rm.RbfConfig()
    sites, vals = _starts([(40, 3), (513, 3), (900, 3), (1200, 3)])
    # the table names 1024: two of the three starts beyond 512 share the launch, the option is 1024 during the call and 512 after
    ctx, stats = _Ctx(lib, 1024), {}
    mods = rm.update_models_many(cfg, sites, vals, 1.0, ctx=ctx, stats=stats)
    assert ctx.lib.asked == [(3, 3)] * 3 and ctx.lib.ran_under == [1024] and ctx.sets == [1024, 512.0] and ctx.option == 512
    assert stats["path"] == "batch" and stats["wide"] == 2 and len(mods) == 4
    _release(mods)
    # a context whose option the caller had raised himself gets HIS value back
    ctx, stats = _Ctx(lib, 2048, start_at=600), {}
    _release(rm.update_models_many(cfg, sites, vals, 1.0, ctx=ctx, stats=stats))
    assert ctx.lib.ran_under == [2048] and ctx.option == 600 and stats["wide"] == 3
    # the call raises: the option is back all the same
    ctx = _Ctx(lib, 2048, raises=True)
    with pytest.raises(RuntimeError):
        rm.update_models_many(cfg, sites, vals, 1.0, ctx=ctx)
    assert ctx.lib.ran_under == [2048] and ctx.sets == [2048, 512.0] and ctx.option == 512
    # the table keeps the loop (512): nothing is set
    ctx, stats = _Ctx(lib, 512), {}
    _release(rm.update_models_many(cfg, sites, vals, 1.0, ctx=ctx, stats=stats))
    assert ctx.sets == [] and ctx.lib.ran_under == [512] and stats["wide"] == 0
    # no start beyond 512: the table is not even asked
    ctx, stats = _Ctx(lib, 2048), {}
    s2, v2 = _starts([(40, 3), (512, 3)])
    _release(rm.update_models_many(cfg, s2, v2, 1.0, ctx=ctx, stats=stats))
    assert ctx.lib.asked == [] and ctx.sets == [] and stats["wide"] == 0
    # mixed dimensions: the smallest answer of the table holds for the call
    ctx = _Ctx(lib, None)
    s3, v3 = _starts([(600, 3), (600, 128)])
    _release(rm.update_models_many(cfg, s3, v3, 1.0, ctx=ctx, stats={}))
    assert sorted(ctx.lib.asked) == [(2, 3), (2, 128)] and ctx.sets == []        # (d = 3 keeps the loop: 512 for the call)


def test_the_committed_rule_through_the_binding(lib):
    """the real table: a batch the rule admits is raised to the rule's n, one it does not admit runs at the default"""
    from morbit.jl_amd import rbf_model as rm

    cfg = rm.RbfConfig()
    for ns in (8, 64, 4):
        want = lib.mrbf_dispatch_fit_batch_max_n(ns, 65)
        assert (want > 512) == (ns >= 8)
        sites, vals = _starts([(513, 65)] * ns)
        ctx, stats = _Ctx(lib, None), {}
        _release(rm.update_models_many(cfg, sites, vals, 1.0, ctx=ctx, stats=stats))
        assert ctx.lib.ran_under == [want] and ctx.option == 512 and stats["wide"] == (ns if want >= 513 else 0)
