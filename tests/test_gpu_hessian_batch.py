"""Many-start model Hessians on the device (mrbf_eval_hessian_batch; run with -m gpu).  The contract under test: for every job the
result is bit for bit what mrbf_eval_hessian writes for it on the same context, whatever its position, its company and the limit of
the chunk rule -- and, independently of the single call, inside the derived bound of tests/hessian_util.py against the
extended-precision reference.  Output buffers start as NaN; bits are compared as uint64."""
import ctypes

import numpy as np
import pytest

from tests import hessian_util as hu
from tests.conftest import has_gpu
from tests.test_gpu_hessian import ALL_KERNELS

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, rbf_model as rm, surrogates as sg

NSPLIT = {"one": 1, "d3_n3": 1, "d15_n4": 1, "d16_n5": 1, "d17_n63": 2, "d64_n257": 9, "d65_n65": 3, "d65_unsplit": 1, "d140_n64": 2,
          "d300_n300": 10, "d300_n5": 1}


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def make_model(ctx, C, W, kid, a, b):
    n, d = C.shape
    h = _lib.c_vp()
    ctx.check(ctx.lib.mrbf_model_from_coeffs(ctx.h, n, d, W.shape[1], _lib.as_ptr(C), _lib.as_ptr(W), None, kid, a, b, -1, ctypes.byref(h)))
    return rm.RbfModel(ctx, h, n, d, W.shape[1], 0, False, W, None, None)


def nan_out(m, r, d):
    return np.full((m, r, d, d), np.nan)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def inside_bound(tag, H, case_or_ref, S=None, n=None, d=None):
    if S is None:
        H_ref, S, n, d = case_or_ref.H_ref, case_or_ref.S, case_or_ref.n, case_or_ref.d
    else:
        H_ref = case_or_ref
    worst = float(hu.errors_over_bound(H, H_ref, S, n, d).max())
    print(tag, "worst error / bound %.3e" % worst)
    assert np.isfinite(H).all(), tag
    assert worst < 1.0, (tag, worst)


class Spec:
    """one job: a model handle (or None), the sites, the rows and the output buffer -- NumPy arrays, torch device tensors or None"""

    def __init__(self, mod, X, rows=None, out=None, m=None, n_rows=None):
        self.mod, self.X, self.out = mod, X, out
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        self.m = (0 if X is None else int(X.shape[0])) if m is None else m
        self.n_rows = (0 if self.rows is None else int(self.rows.size)) if n_rows is None else n_rows


def run_batch(ctx, specs, limit=None, h=None, n=None):
    jobs = (_lib.HessJob * max(1, len(specs)))()
    for J, s in zip(jobs, specs):
        J.model = None if s.mod is None else (s.mod.model.value if hasattr(s.mod.model, "value") else s.mod.model)
        J.m, J.n_rows = s.m, s.n_rows
        J.X = None if s.X is None else _lib.as_ptr(s.X).value
        J.rows = None if s.rows is None else _lib.as_ptr(s.rows).value
        J.hess_out = None if s.out is None else _lib.as_ptr(s.out).value
        J.status, J.nsplit = 99, 99
    info = _lib.HessBatchInfo()
    n = len(specs) if n is None else n
    h = ctx.h if h is None else h
    if limit is None:
        rc = ctx.lib.mrbf_eval_hessian_batch(h, n, jobs, ctypes.byref(info))
    else:
        rc = ctx.lib.mrbf_eval_hessian_batch_limited(h, n, jobs, ctypes.byref(info), limit)
    return rc, jobs, info


# ---- the eleven variants: models, the single call's results (computed once, read-only) -------------------------------------------------
@pytest.fixture(scope="module")
def variants(ctx):
    names = sorted(hu.VARIANTS)
    cases = [hu.variant_case(v) for v in names]
    mods = [make_model(ctx, c.C, c.W, c.kid, c.a, c.b) for c in cases]
    single = []
    for c, mod in zip(cases, mods):
        r = c.k if c.rows is None else len(c.rows)
        H = mod.hessian_sites(c.X, rows=c.rows, out=nan_out(c.m, r, c.d))
        H.setflags(write=False)
        single.append(H)
    yield names, cases, mods, single
    for mod in mods:
        mod.free()


def variant_specs(variants, order=None):
    names, cases, mods, single = variants
    order = range(len(names)) if order is None else order
    return [Spec(mods[i], cases[i].X, cases[i].rows, np.full(single[i].shape, np.nan)) for i in order]


# ---- 1. every variant of the kernels in one call ----------------------------------------------------------------------------------------
def test_all_variants_as_one_call(ctx, variants):
    names, cases, mods, single = variants
    specs = variant_specs(variants)
    rc, jobs, info = run_batch(ctx, specs)
    assert rc == 0
    print("info", info.asdict(), "nsplit", [jobs[i].nsplit for i in range(len(names))])
    for i, name in enumerate(names):
        assert jobs[i].status == 0
        assert jobs[i].nsplit == NSPLIT[name], (name, jobs[i].nsplit)
        assert same_bits(specs[i].out, single[i]), name                  # the bits of the single call
        inside_bound(name, specs[i].out, cases[i])                       # ... and, independently of it, the reference
        assert same_bits(specs[i].out, np.swapaxes(specs[i].out, 2, 3)), name   # both triangles the same bits
    # multiquadric, fast form, RB = 1, 2, 4: three main groups; one round, nothing inside
    assert info.chunks == 1 and info.single_inside == 0 and info.groups == 3


# ---- 2. every radial function, jobs of several groups interleaved ---------------------------------------------------------------------
def test_every_radial_function_in_one_call(ctx):
    cases = [hu.variant_case(v, kernel) for kernel in ALL_KERNELS for v in ("d16_n5", "d17_n63")]
    mods = [make_model(ctx, c.C, c.W, c.kid, c.a, c.b) for c in cases]
    try:
        singles = [mod.hessian_sites(c.X, rows=c.rows, out=nan_out(c.m, 3, c.d)) for c, mod in zip(cases, mods)]
        specs = [Spec(mod, c.X, c.rows, nan_out(c.m, 3, c.d)) for c, mod in zip(cases, mods)]
        rc, jobs, info = run_batch(ctx, specs)
        assert rc == 0
        print("info", info.asdict())
        for c, s, H, J in zip(cases, specs, singles, jobs):
            tag = "%s %s" % (c.kernel, c.name)
            assert J.status == 0 and J.nsplit == NSPLIT[c.name]
            assert same_bits(s.out, H), tag
            inside_bound(tag, s.out, c)
        # every job has r = 3 (RB = 4): the groups are the instantiations by radial function and fast form alone
        assert 5 <= info.groups <= len(ALL_KERNELS) and info.chunks == 1 and info.single_inside == 0
    finally:
        for mod in mods:
            mod.free()


# ---- 3. position and company ---------------------------------------------------------------------------------------------------------------
def test_position_and_company_do_not_change_the_bits(ctx, variants):
    names, cases, mods, single = variants
    nv = len(names)
    rng = np.random.default_rng(7)
    for order in (list(rng.permutation(nv)), list(range(nv))[::-1], [0], [0, 1, 2], list(range(nv))):
        specs = variant_specs(variants, order)
        rc, jobs, info = run_batch(ctx, specs)
        assert rc == 0
        for pos, i in enumerate(order):
            assert same_bits(specs[pos].out, single[i]), (order, names[i])
            assert jobs[pos].nsplit == NSPLIT[names[i]]
    # one model in two jobs with different rows and sites, an m = 0 job between two others
    i = names.index("d17_n63")
    mod, c = mods[i], cases[i]
    Xa, Xb = np.ascontiguousarray(c.X[:5]), np.ascontiguousarray(c.X[40:])
    Ha = mod.hessian_sites(Xa, rows=[0], out=nan_out(5, 1, c.d))
    Hb = mod.hessian_sites(Xb, rows=[1, 1, 0, 1, 0], out=nan_out(24, 5, c.d))
    empty_out = nan_out(3, 2, c.d)
    specs = [Spec(mod, Xa, [0], nan_out(5, 1, c.d)), Spec(mod, c.X[:3], None, empty_out, m=0), Spec(mod, Xb, [1, 1, 0, 1, 0], nan_out(24, 5, c.d)),
             Spec(mod, None, None, None, m=0)]
    rc, jobs, info = run_batch(ctx, specs)
    assert rc == 0 and [jobs[j].status for j in range(4)] == [0, 0, 0, 0]
    assert same_bits(specs[0].out, Ha) and same_bits(specs[2].out, Hb)
    assert np.isnan(empty_out).all() and jobs[1].nsplit == 0 and jobs[3].nsplit == 0     # an m = 0 job writes nothing
    assert jobs[0].nsplit == 2 and jobs[2].nsplit == 2                                    # each splits as its own single call does


# ---- 4. the many-start shape: one radial function, one r, any mix of n ---------------------------------------------------------------------
def test_many_start_shape_is_one_group(ctx):
    d, k = 65, 2
    mods, Xs, singles = [], [], []
    try:
        for t, n in enumerate((65, 66, 97, 129, 257)):
            C, W, rng = hu.random_model(d, n, k, 900 + t)
            mods.append(make_model(ctx, C, W, 0, 3.0, 0.0))                                 # cubic
            Xs.append(np.ascontiguousarray(rng.random((1, d))))
            infos = {}
            singles.append(mods[-1].hessian_sites(Xs[-1], out=nan_out(1, k, d), info=infos))
            assert infos["nsplit"] > 1
        specs = [Spec(mod, X, None, nan_out(1, k, d)) for mod, X in zip(mods, Xs)]
        rc, jobs, info = run_batch(ctx, specs)
        assert rc == 0
        assert info.groups == 1 and info.single_inside == 0 and info.chunks == 1
        for s, H in zip(specs, singles):
            assert same_bits(s.out, H)
    finally:
        for mod in mods:
            mod.free()


# ---- 5. host and device pointers mixed, per job and per buffer ------------------------------------------------------------------------------
def test_host_and_device_buffers_mixed(ctx, variants):
    names, cases, mods, single = variants
    pick = [names.index(v) for v in ("d17_n63", "d16_n5", "d65_n65", "d3_n3")]
    specs, guards = [], []
    for t, i in enumerate(pick):
        c = cases[i]
        x_dev, out_dev = bool(t & 1), bool(t & 2)                        # (host, host), (device, host), (host, device), (device, device)
        X, out, obuf = c.X, np.full(single[i].shape, np.nan), None
        if x_dev:
            xbuf = torch.full((c.m * c.d + 1,), float("nan"), dtype=torch.float64, device="cuda")
            X = xbuf[1:].view(c.m, c.d)                                   # a device buffer on an odd double
            X.copy_(torch.from_numpy(np.array(c.X)))
            guards.append(xbuf)
        if out_dev:
            obuf = torch.full((single[i].size + 1,), float("nan"), dtype=torch.float64, device="cuda")
            out = obuf[1:].view(*single[i].shape)
            assert out.data_ptr() % 16 == 8
            guards.append(obuf)
        specs.append((Spec(mods[i], X, c.rows, out), out_dev, obuf))
    rc, jobs, info = run_batch(ctx, [s for s, _, _ in specs])
    assert rc == 0 and info.chunks == 1
    for (s, out_dev, obuf), i in zip(specs, pick):
        got = s.out.cpu().numpy() if out_dev else s.out
        assert same_bits(got, single[i]), names[i]
        if out_dev:
            assert np.isnan(obuf[:1].cpu().numpy()).all()                # the double in front of the buffer is still NaN


# ---- 6. chunks ---------------------------------------------------------------------------------------------------------------------------
def test_chunks_do_not_change_the_bits_and_nothing_grows(ctx, variants):
    names, cases, mods, single = variants
    nv = len(names)
    counts = {}
    for limit in (None, 1, 24 << 20):
        specs = variant_specs(variants)
        rc, jobs, info = run_batch(ctx, specs, limit=limit)
        assert rc == 0
        print("limit", limit, info.asdict())
        counts[limit] = (info.chunks, info.single_inside)
        for i in range(nv):
            assert same_bits(specs[i].out, single[i]), (limit, names[i])
            assert jobs[i].nsplit == NSPLIT[names[i]]
    assert counts[None] == (1, 0)
    assert counts[1] == (nv, nv)                    # every active job beyond the limit on its own: the single call's chain inside
    assert 1 < counts[24 << 20][0] < nv
    arena = ctx.get_option(_lib.OPT_ARENA_BYTES)
    specs = variant_specs(variants)
    rc, jobs, info = run_batch(ctx, specs)
    assert rc == 0 and ctx.get_option(_lib.OPT_ARENA_BYTES) == arena
    assert all(same_bits(specs[i].out, single[i]) for i in range(nv))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(ctx, variants):
    names, cases, mods, single = variants
    i = names.index("d3_n3")
    mod, c = mods[i], cases[i]                        # d = 3, n = 3, m = 2, k = 2
    good = lambda: Spec(mod, c.X, None, nan_out(2, 2, 3))
    # -1 and -2
    rc, _, _ = run_batch(ctx, [good()], h=ctypes.c_void_p(None))
    assert rc == -1
    for n in (0, 65536):
        s = good()
        rc, jobs, _ = run_batch(ctx, [s], n=n)
        assert rc == -2 and np.isnan(s.out).all()
        assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_HESSIAN_BATCH, rc) == 1
    assert ctx.lib.mrbf_eval_hessian_batch(ctx.h, 2, None, None) == -3          # `jobs` NULL
    # -3: each kind of invalid job, between two valid ones; every job's own status; every buffer of every job still NaN
    rows_high = np.array([0, 2], dtype=np.int32)
    rows_neg = np.array([-1], dtype=np.int32)
    kinds = [
        (-2, lambda: Spec(None, c.X, None, nan_out(2, 2, 3))),
        (-3, lambda: Spec(mod, c.X, None, nan_out(2, 2, 3), m=-1)),
        (-5, lambda: Spec(mod, c.X, None, nan_out(2, 2, 3), n_rows=-1)),
        (-5, lambda: Spec(mod, c.X, None, nan_out(2, 2, 3), n_rows=2)),            # n_rows > 0 with NULL rows
        (-6, lambda: Spec(mod, c.X, rows_high, nan_out(2, 2, 3))),
        (-6, lambda: Spec(mod, c.X, rows_neg, nan_out(2, 1, 3))),
        (-6, lambda: Spec(mod, None, rows_high, None, m=0)),                       # the rows are looked at whatever m is
        (-4, lambda: Spec(mod, None, None, nan_out(2, 2, 3), m=2)),                # NULL X with m > 0
        (-7, lambda: Spec(mod, c.X, None, None)),                                  # NULL hess_out with m > 0
    ]
    other = pkg.Context()
    try:
        C2, W2, _ = hu.random_model(3, 3, 2, 5)
        foreign = make_model(other, C2, W2, 2, 1.0, 0.5)
        for status, bad in kinds:
            specs = [good(), bad(), good()]
            rc, jobs, _ = run_batch(ctx, specs)
            assert rc == -3, (status, rc)
            assert [jobs[j].status for j in range(3)] == [0, status, 0]
            assert all(s.out is None or np.isnan(s.out).all() for s in specs), status
            # -3 in front of -4: a foreign model elsewhere in the batch changes neither the code nor the statuses
            specs = [Spec(foreign, c.X, None, nan_out(2, 2, 3)), bad(), good()]
            rc, jobs, _ = run_batch(ctx, specs)
            assert rc == -3 and [jobs[j].status for j in range(3)] == [0, status, 0]
            assert all(s.out is None or np.isnan(s.out).all() for s in specs), status
        # -4: a model of a second context
        specs = [good(), Spec(foreign, c.X, None, nan_out(2, 2, 3)), good()]
        rc, jobs, _ = run_batch(ctx, specs)
        assert rc == -4 and all(np.isnan(s.out).all() for s in specs)
        for limit in (1, 1 << 20):
            rc, jobs, _ = run_batch(ctx, specs, limit=limit)
            assert rc == -4 and all(np.isnan(s.out).all() for s in specs)
        foreign.free()
    finally:
        other.close()
    # the same jobs without a defect run
    specs = [good(), good()]
    rc, jobs, _ = run_batch(ctx, specs)
    assert rc == 0 and same_bits(specs[0].out, single[i]) and same_bits(specs[1].out, single[i])


# ---- 8. models of every origin in one call -----------------------------------------------------------------------------------------------
def test_models_of_every_origin_in_one_call(ctx):
    d, n, k, m = 5, 40, 2, 4
    a = hu.gaussian_shape(d)
    mods, refs, specs = [], [], []
    try:
        for deg in (-1, 0, 1):
            cfg = pkg.RbfConfig(kernel="gaussian", shape_parameter=a, polynomial_degree=deg)
            C, _, rng = hu.random_model(d, n, k, 5 + deg)
            Y = np.stack([np.sin(C.sum(axis=1)), np.cos(C @ np.arange(1.0, d + 1.0) / d)], axis=1)
            X = np.ascontiguousarray(rng.random((m, d)))
            fitted = pkg.update_model(cfg, C, Y, ctx=ctx)
            batch = pkg.update_models_many([cfg, cfg], [C, C], [Y, Y], 1.0, ctx=ctx)
            coeffs = pkg.model_from_coeffs(cfg, C, fitted.weights, fitted.poly if deg >= 0 else None, ctx=ctx)
            for mod in (fitted, batch[0], batch[1], coeffs):
                assert mod is not None
                mods.append(mod)
                refs.append(hu.reference_hessian(C, mod.weights, 4, a, 0.0, X))       # the tail has no second derivative
                specs.append(Spec(mod, X, None, nan_out(m, k, d)))
        rc, jobs, info = run_batch(ctx, specs)
        assert rc == 0 and info.groups == 1
        for t, (s, (H_ref, S)) in enumerate(zip(specs, refs)):
            inside_bound("origin %d" % t, s.out, H_ref, S, n, d)
            assert same_bits(s.out, mods[t].hessian_sites(s.X, out=nan_out(m, k, d)))
    finally:
        for mod in mods:
            mod.free()


# ---- 9. bindings ---------------------------------------------------------------------------------------------------------------------------
def test_get_hessians_many_takes_both_paths(ctx, variants):
    names, cases, mods, single = variants
    pick = [names.index(v) for v in ("d17_n63", "d16_n5", "d65_n65", "d3_n3", "d64_n257")]
    ms, Xs, rows = [mods[i] for i in pick], [cases[i].X for i in pick], [cases[i].rows for i in pick]
    stats = {}
    got = pkg.get_hessians_many(ms, Xs, rows=rows, min_jobs=2, stats=stats)
    assert stats["path"] == "batch" and stats["jobs"] == 5 and stats["chunks"] == 1 and stats["single_inside"] == 0
    assert stats["nsplit"] == [NSPLIT[names[i]] for i in pick] and stats["groups"] >= 1
    assert all(same_bits(g, single[i]) for g, i in zip(got, pick))
    stats = {}
    loop = pkg.get_hessians_many(ms, Xs, rows=rows, min_jobs=6, stats=stats)
    assert stats["path"] == "loop" and stats["nsplit"] == [NSPLIT[names[i]] for i in pick]
    assert all(same_bits(g, single[i]) for g, i in zip(loop, pick))
    # the table's own threshold decides when none is given
    stats = {}
    pkg.get_hessians_many(ms, Xs, rows=rows, stats=stats)
    assert stats["path"] == ("batch" if 5 >= ctx.lib.mrbf_dispatch_hessian_batch_min_jobs() else "loop")
    # the chunk path through the binding
    stats = {}
    cut = rm.get_hessians_many(ms, Xs, rows=rows, min_jobs=1, limit_bytes=1, stats=stats)
    assert stats["single_inside"] == 5 and stats["chunks"] == 5 and all(same_bits(g, single[i]) for g, i in zip(cut, pick))


def test_container_functions_match_get_hessian(ctx):
    d, n_starts = 6, 5
    starts, Xs = [], []
    mods = []
    try:
        for p in range(n_starts):
            CA, WA, rng = hu.random_model(d, 20 + p, 4, 300 + p)
            CB, WB, _ = hu.random_model(d, 33 + p, 2, 400 + p)
            A, B = make_model(ctx, CA, WA, 2, 1.0, 0.5), make_model(ctx, CB, WB, 0, 3.0, 0.0)
            mods += [A, B]
            sc = sg.SurrogateContainer(objectives=[sg.RefSurrogate(A, [3, 0]), sg.RefSurrogate(B, [1]), sg.RefSurrogate(A, [2])],
                                       nl_ineq_constraints=[sg.RefSurrogate(B, [0]), sg.RefSurrogate(A, [1, 3])])
            starts.append(sc)
            Xs.append(np.ascontiguousarray(rng.random((2, d))))
        for fn, kind in ((sg.eval_container_objectives_hessians_at_scaled_sites_many, "objective"),
                         (sg.eval_container_nl_ineq_constraints_hessians_at_scaled_sites_many, "nl_ineq_constraint")):
            for min_jobs, path in ((2, "batch"), (11, "loop")):
                stats = {}
                many = fn(starts, None, Xs, stats=stats, min_jobs=min_jobs)
                assert stats["path"] == path and (path == "loop" or stats["jobs"] == 2 * n_starts)
                for p, sc in enumerate(starts):
                    surs = sc.lists[kind]
                    row = 0
                    for s in surs:
                        for ell in range(s.num_outputs):
                            for q in range(2):
                                assert same_bits(many[p][q, row], sg.get_hessian(s, None, Xs[p][q], ell)), (kind, path, p, row, q)
                            row += 1
                    assert many[p].shape == (2, row, d, d)
        one = sg.eval_container_objectives_hessians_at_scaled_sites(starts[0], None, Xs[0])
        assert same_bits(one, sg.eval_container_objectives_hessians_at_scaled_sites_many(starts, None, Xs, min_jobs=1)[0])
        assert same_bits(sg.eval_container_objectives_hessians_at_scaled_site(starts[0], None, Xs[0][1]), one[1])
        assert sg.eval_container_nl_eq_constraints_hessians_at_scaled_site(starts[0], None, Xs[0][0]).shape == (0, d, d)
        bad = sg.SurrogateContainer(objectives=[sg.RefSurrogate(mods[0], [0]), sg.CompositeSurrogate(mods[1], None, [0, 1], num_outputs=1)])
        with pytest.raises(NotImplementedError):
            sg.eval_container_objectives_hessians_at_scaled_sites_many([starts[0], bad], None, Xs[:2], min_jobs=1)
        with pytest.raises(NotImplementedError):
            sg.eval_container_objectives_hessians_at_scaled_site(bad, None, Xs[0][0])
    finally:
        for mod in mods:
            mod.free()
