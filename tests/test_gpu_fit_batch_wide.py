"""The one-launch fit beyond 512 sites (run with -m gpu): MRBF_OPT_SMALL_FIT_MAX_N raised on a context, mrbf_fit_batch against
mrbf_fit under the same option value.  Bit identity is the contract, as in tests/test_gpu_fit_batch.py (whose helpers these tests
use): weights, tail coefficients, values and Jacobians of mrbf_eval with np.array_equal, path / fallbacks / n / q with ==.
Shapes: (n, d) = (513, 3) the first size beyond the old limit, (641, 65) the crossing of npad 640 -> 768, (1100, 128) a size of
the C4 rehearsal, (2048, 3) the ceiling.  Accuracy is stated against the oracle's LU, not against the code under test."""
import numpy as np
import pytest

from tests.conftest import has_gpu
from tests.test_gpu_fit_batch import INFO_EQUAL, KERNELS, _free, _queries, _spec, assert_same_model, batch, single

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg

SHAPES = [(513, 3), (641, 65), (1100, 128), (2048, 3)]
CEILING = 2048


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


class raised:
    """the option at `value` on `ctx` inside the block, its previous value behind it"""

    def __init__(self, ctx, value=CEILING):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        self.previous = self.ctx.get_option(_lib.OPT_SMALL_FIT_MAX_N)
        self.ctx.set_option(_lib.OPT_SMALL_FIT_MAX_N, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(_lib.OPT_SMALL_FIT_MAX_N, self.previous)


def _same_bits(a, b, tag):
    """two (status, model) pairs: weights, tail, values and Jacobians at the 70 queries"""
    assert a[0] == b[0] == 0, (tag, a[0], b[0])
    assert np.array_equal(a[1].weights, b[1].weights) and np.array_equal(a[1].poly, b[1].poly), tag
    X = _queries(a[1].d)
    aV, aJ = a[1].eval_sites(X, want_values=True, want_jac=True)
    bV, bJ = b[1].eval_sites(X, want_values=True, want_jac=True)
    assert np.array_equal(aV, bV) and np.array_equal(aJ, bJ), tag


def test_option_default_range_and_rejection():
    c = pkg.Context()
    try:
        assert c.get_option(_lib.OPT_SMALL_FIT_MAX_N) == 512
        for good in (512, 513, 1100, 2048):
            c.set_option(_lib.OPT_SMALL_FIT_MAX_N, good)
            assert c.get_option(_lib.OPT_SMALL_FIT_MAX_N) == good
        c.set_option(_lib.OPT_SMALL_FIT_MAX_N, 1024)
        for bad in (511, 0, -1, 2049, 1e9, float("nan")):
            assert c.lib.mrbf_set_option(c.h, _lib.OPT_SMALL_FIT_MAX_N, float(bad)) == -2
            assert c.get_option(_lib.OPT_SMALL_FIT_MAX_N) == 1024
    finally:
        c.close()


# (a) the batch against the single call under the same option value
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("kernel,deg", KERNELS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_bit_identity_with_mrbf_fit_beyond_512(ctx, n, d, kernel, deg, k):
    specs = [_spec(kernel, deg, n, d, k, seed=1000 * n + 10 * d + p) for p in range(3)]
    with raised(ctx):
        refs = [single(ctx, s) for s in specs]
        assert all(rc == 0 for rc, _ in refs)
        for members in (range(3), [1]):
            got = batch(ctx, [specs[p] for p in members])
            for g, p in zip(got, members):
                assert_same_model(g, refs[p], (n, d, kernel, k, len(got), p))
            _free(got)
    _free(refs)


# (b) batches of 1, 9 and 40 starts select clusters of 16, 16 and 4 workgroups per start
def test_cluster_size_does_not_change_the_bits(ctx):
    n, d = 513, 3
    specs = [_spec("cubic", 1, n, d, 2, seed=77 + p) for p in range(40)]
    with raised(ctx):
        one = batch(ctx, specs[:1])
        nine = batch(ctx, specs[:9])
        forty = batch(ctx, specs)
        _same_bits(nine[0], one[0], "9 against 1")
        _same_bits(forty[0], one[0], "40 against 1")
        for p in range(9):
            _same_bits(forty[p], nine[p], ("40 against 9", p))
    _free(one), _free(nine), _free(forty)


def _mixed_specs():
    return [_spec("cubic", 1, 300, 3, 2, 11), _spec("cubic", 1, 513, 3, 2, 12), _spec("multiquadric", 0, 1100, 3, 1, 13),
            _spec("cubic", 1, 1100, 65, 2, 14), _spec("gaussian", -1, 300, 65, 1, 15), _spec("multiquadric", 1, 513, 65, 2, 16)]


# (c) position and company
def test_position_independence_beyond_512(ctx):
    specs = _mixed_specs()
    perm = [3, 0, 5, 2, 4, 1]
    with raised(ctx):
        a = batch(ctx, specs)
        b = batch(ctx, [specs[i] for i in perm])
        c = batch(ctx, [specs[i] for i in (2, 3)])
        for j, i in enumerate(perm):
            assert_same_model(b[j], a[i], ("permuted", j, i), well_conditioned=False)
        for j, i in enumerate((2, 3)):
            assert_same_model(c[j], a[i], ("other company", j, i), well_conditioned=False)
    _free(a), _free(b), _free(c)


# (d) today's contract, next to the new one: at the default the starts beyond 512 take mrbf_fit inside the call
def test_default_option_is_the_single_call(ctx):
    assert ctx.get_option(_lib.OPT_SMALL_FIT_MAX_N) == 512
    specs = _mixed_specs()
    refs = [single(ctx, s) for s in specs]
    got = batch(ctx, specs)
    for p, (g, r) in enumerate(zip(got, refs)):
        assert_same_model(g, r, ("default", p))
        assert g[1].info["path"] == r[1].info["path"]
    _free(got), _free(refs)


# (f) a raised option never changes a start with n <= 512
@pytest.mark.parametrize("n,d", [(300, 3), (512, 65), (257, 128)])
def test_raised_option_leaves_small_starts_alone(ctx, n, d):
    specs = [_spec("cubic", 1, n, d, 2, seed=5 * n + d + p) for p in range(2)] + [_spec("cubic", 1, 700, d, 2, seed=9)]
    refs = [single(ctx, s) for s in specs[:2]]
    with raised(ctx):
        again = [single(ctx, s) for s in specs[:2]]
        got = batch(ctx, specs)          # (a start beyond 512 shares the launch)
    for p in range(2):
        _same_bits(again[p], refs[p], ("single", n, d, p))
        _same_bits(got[p], refs[p], ("batch", n, d, p))
        assert all(got[p][1].info[f] == refs[p][1].info[f] for f in INFO_EQUAL)
    _free(refs), _free(again), _free(got)


# (e) accuracy against the oracle's LU.  Sites uniform in [-2, 2]^d, the package's default shape parameters (section 12's setting).
# Relative weight error err(w) = max |w - w_oracle| / max |w_oracle|.  The one-launch fit and the launch chain are two backward-stable
# Cholesky variants that sum in different orders: the wide fit may be up to 4 x the chain's error on the same case, or 1e-10.
# Measured (MI355X), wide / chain: 7e-14 .. 1.1e-13 / 5e-14 .. 1.1e-13 at d = 65 and 128 (gaussian: 0 / 0, its matrix is the identity
# to working precision there); (513, 3) cubic 1.2e-10 / 1.8e-10, multiquadric 4.6e-10 / 7.6e-10; (2048, 3) cubic 2.7e-9 / 2.7e-9,
# multiquadric 7.4e-7 / 1.1e-6; (513, 3) gaussian 3.5e-9 / 1.4e-9.  The d = 3 shapes, which the contract's size range asks for, are
# ill-conditioned (condition number of the saddle matrix, computed on the CPU: 5e7 .. 3e8 at n = 513; 2e9 cubic, 1e12 multiquadric at
# n = 2048), so the chain alone is above 1e-10 there and the bound that holds is the relative one.  Dropped: gaussian / degree -1 at
# (2048, 3): condition number 2e16, the oracle's LU reports rcond = 1e-17 and the chain's "error" against it is 0.2 -- the reference
# cannot judge either fit; tests (a) - (d) keep that case for bit identity.
ACCURACY_CASES = [(n, d, kernel, deg) for n, d in SHAPES for kernel, deg in KERNELS if not (kernel == "gaussian" and (n, d) == (2048, 3))]


@pytest.mark.parametrize("n,d,kernel,deg", ACCURACY_CASES)
def test_accuracy_against_the_oracle(ctx, n, d, kernel, deg):
    from oracle import rbf_oracle as orc

    for k in (1, 2):
        s = _spec(kernel, deg, n, d, k, seed=1000 * n + 10 * d)
        ref = orc.fit(s["C"], s["Y"], s["kid"], s["a"], s["b"], s["deg"])
        scale = np.abs(ref.w).max()
        rc_c, chain = single(ctx, s)
        with raised(ctx):
            rc_w, wide = single(ctx, s)
        assert rc_c == 0 and rc_w == 0
        e_chain, e_wide = np.abs(chain.weights - ref.w).max() / scale, np.abs(wide.weights - ref.w).max() / scale
        print("n=%d d=%d %s deg %d k=%d: weight error wide %.3e chain %.3e | rel_residual wide %.3e chain %.3e | path wide %d chain %d"
              % (n, d, kernel, deg, k, e_wide, e_chain, wide.info["rel_residual"], chain.info["rel_residual"], wide.info["path"],
                 chain.info["path"]))
        assert e_wide <= max(1e-10, 4.0 * e_chain), (n, d, kernel, k, e_wide, e_chain)
        if chain.info["rel_residual"] <= 1e-11:
            assert wide.info["rel_residual"] <= 1e-11, (n, d, kernel, k, wide.info, chain.info)
        chain.free(), wide.free()


# (g) the models of a wide batch hand on to the batched descent
def test_wide_models_hand_on_to_the_batched_descent(ctx):
    d, ns = 65, 5
    specs = [_spec("multiquadric", 1, 513 + 3 * p, d, 2, seed=300 + 7 * d + p) for p in range(ns)]
    with raised(ctx):
        refs = [single(ctx, s) for s in specs]
        got = batch(ctx, specs)
    rng = np.random.default_rng(55 + d)
    X = rng.uniform(-1.0, 1.0, (ns, d))
    X_n = X + rng.uniform(-0.02, 0.02, (ns, d))
    deltas = np.array([0.3, 0.25, 0.4, 0.35, 0.3])
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    cfg = descent.SteepestDescentConfig()
    out = []
    for pairs in (refs, got):
        plans = [sg.container_plan(sg.SurrogateContainer(objectives=[sg.RefSurrogate(m, [0, 1])])) for _, m in pairs]
        rc, D, XP, MXP, recs, ms = descent.sd_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, None)
        assert rc == 0 and all(r["sd_status"] == _lib.SD_OK for r in recs), (rc, recs)
        out.append((D, XP, MXP, recs))
    for u, v in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(u, v)
    for p, (ra, rb) in enumerate(zip(out[0][3], out[1][3])):
        assert ra.keys() == rb.keys()
        for f in ra:
            assert ra[f] == rb[f] or (isinstance(ra[f], float) and np.isnan(ra[f]) and np.isnan(rb[f])), (p, f, ra[f], rb[f])
    _free(got), _free(refs)


def test_a_batch_beyond_the_arena_budget_is_worked_off_in_halves(monkeypatch):
    """four starts of n = 1100 ask for ~14 MB of scratch each; with the launch group's budget at 40 MB the call must fit them two by
    two -- the same bits, and an arena that never held all four"""
    specs = [_spec("cubic", 1, 1100, 3, 2, seed=40 + p) for p in range(4)]
    whole, halved = pkg.Context(), pkg.Context()
    try:
        with raised(whole):
            a = batch(whole, specs)
        arena_whole = whole.get_option(_lib.OPT_ARENA_BYTES)
        monkeypatch.setenv("MRBF_EXPERIMENTS", "1")
        monkeypatch.setenv("MRBF_BATCH_ARENA_MB", "40")
        with raised(halved):
            b = batch(halved, specs)
        monkeypatch.undo()
        arena_halved = halved.get_option(_lib.OPT_ARENA_BYTES)
        print("arena bytes: one group %.1f MB, halves %.1f MB" % (arena_whole / 2**20, arena_halved / 2**20))
        assert arena_whole > 4 * 13.0 * 2**20 and arena_halved < 0.7 * arena_whole
        for p in range(4):
            assert_same_model(b[p], a[p], ("halves", p), well_conditioned=False)
        _free(a), _free(b)
    finally:
        whole.close(), halved.close()


def test_binding_raises_the_option_for_the_call_only(ctx):
    """update_models_many with the table's answer replaced by the ceiling: the starts beyond 512 share the launch (stats["wide"]),
    each is what update_model gives under that option value, and the option is back at 512 behind the call"""
    d, ns = 3, 4
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)
    data = [(s["C"], s["Y"]) for s in (_spec("cubic", 1, n, d, 2, seed=60 + n) for n in (300, 513, 700, 600))]
    real = ctx.lib.mrbf_dispatch_fit_batch_max_n
    stats = {}
    mods = pkg.update_models_many(cfg, [C for C, _ in data], [Y for _, Y in data], 1.0, ctx=ctx, stats=stats)
    assert stats["path"] == "batch" and stats["wide"] == sum(1 for C, _ in data if 512 < C.shape[0] <= real(3, d))
    for m in mods:
        m.free()

    class Lib:
        def __getattr__(self, name):
            return getattr(ctx.lib, name) if name != "mrbf_dispatch_fit_batch_max_n" else (lambda ns_, d_: CEILING)

    class Ctx:
        lib, h = Lib(), ctx.h
        check, set_option, get_option = ctx.check, ctx.set_option, ctx.get_option

    stats = {}
    mods = pkg.update_models_many(cfg, [C for C, _ in data], [Y for _, Y in data], 1.0, ctx=Ctx(), stats=stats)
    assert stats["path"] == "batch" and stats["wide"] == 3 and stats["status"] == [0] * ns
    assert ctx.get_option(_lib.OPT_SMALL_FIT_MAX_N) == 512
    with raised(ctx):
        for m, (C, Y) in zip(mods, data):
            ref = pkg.update_model(cfg, C, Y, ctx=ctx)
            assert np.array_equal(m.weights, ref.weights) and np.array_equal(m.poly, ref.poly)
            ref.free()
    for m in mods:
        m.free()
