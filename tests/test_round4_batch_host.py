"""CPU tests of the many-start round 4 (mrbf_round4_batch): its decision-table row and return codes, the job struct's mirrors against
the header, the routing of `sampling.rbf_round4_many` -- which starts form the batch, which run `_rbf_round4`, what happens when the
library refuses the batch or one start -- and the margin helper the GPU tests rest on.  No GPU: the device calls are replaced by a
host stand-in that does the batched kernel's arithmetic in NumPy (tests/round4_batch_util.py::numpy_walk)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import round4_batch_util as u


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


@pytest.mark.parametrize("n_starts, d, device", [
    (1, 128, True), (64, 128, True), (65535, 128, True), (0, 128, False), (65536, 128, False), (-1, 3, False),
    (64, 1, True), (64, 1024, True), (64, 1025, False), (64, 0, False), (1, 129, True),   # d > 128: mrbf_round4 inside the call
])
def test_decision_table_row(lib, n_starts, d, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_round4_batch(n_starts, d) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_ROUND4_BATCH == 13
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_ROUND4_BATCH = 13\b", text)
    # the case mirrors MRBF_ENTRY_ROUND4's, code by code
    for rc in (-14, -10, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7):
        assert lib.mrbf_dispatch_after(13, rc) == lib.mrbf_dispatch_after(_lib.ENTRY_ROUND4, rc), rc
    assert lib.mrbf_dispatch_after(13, -2) == 1 and lib.mrbf_dispatch_after(13, _lib.MRBF_ESINGULAR) == 1
    assert lib.mrbf_dispatch_after(13, -4) == 0 and lib.mrbf_dispatch_after(13, 0) == 0 and lib.mrbf_dispatch_after(13, _lib.MRBF_EHIP) == 0
    doc = text[text.index("many-start round 4"):text.index("} mrbf_round4_job;")]
    assert "NO FACTOR STATE IS KEPT" in doc and "mrbf_fit_batch" in doc and "RbfModel.jl:352-499" in doc
    assert re.search(r"does not depend on its position in the batch or on which other starts share it", doc)
    for limit in ("d <= 128", "q <= n0 <= 256", "mc <= 4096", "<= 256"):
        assert limit in doc, limit
    # without a context nothing is touched
    assert lib.mrbf_round4_batch(None, 1, 3, None, None) == -1


def test_job_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_round4_job;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "double": 8, "float": 4, "int64_t": 8}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:                 # a pointer: the name follows the last star
            fields.append((decl.rsplit("*", 1)[1].strip(), 8, True))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), sizes[ctype], False) for n in names.split(",")]
    off, layout = 0, []
    for name, size, _ in fields:        # natural alignment
        off = (off + size - 1) // size * size
        layout.append((name, off, size))
        off += size
    total = (off + 7) // 8 * 8
    assert total == 88 == ctypes.sizeof(_lib.Round4Job)
    assert [f[0] for f in _lib.Round4Job._fields_] == [n for n, _, _ in layout]
    assert [n for n, _, _ in layout] == ["n0", "mc", "start_sites", "cand_sites", "kernel_id", "poly_deg", "a", "b", "max_points",
                                         "theta_pivot_cholesky", "accepted_out", "n_accepted", "rc"]
    for name, o, size in layout:
        fld = getattr(_lib.Round4Job, name)
        assert (fld.offset, fld.size) == (o, size), name
    assert _lib.Round4Job.theta_pivot_cholesky.offset == 64 and _lib.Round4Job.rc.offset == 84
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfRound4Job\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Int64|Float64|Ptr\{\w+\})", jbody)
    jsize = {"Int32": 4, "Int64": 8, "Float64": 8}
    assert [(n, 8 if t.startswith("Ptr{") else jsize[t], t.startswith("Ptr{")) for n, t in jfields] == fields
    assert re.search(r"ccall\(\(:mrbf_round4_batch, libmrbf\)", jl) and re.search(r"ccall\(\(:mrbf_dispatch_round4_batch, libmrbf\)", jl)
    assert re.search(r"function hip_round4_many\(", jl)
    # both bindings keep the single calls below the same, measured, number of starts
    from morbit.jl_amd import sampling
    assert int(re.search(r"const ROUND4_BATCH_MIN_STARTS = (\d+)", jl).group(1)) == sampling.ROUND4_BATCH_MIN_STARTS


# ---- routing of rbf_round4_many ----------------------------------------------------------------------------------------------

def _walk(cfg, C0, Xc, delta=1.0):
    import morbit.jl_amd as pkg

    kid, a, b = pkg.rbf_model._get_kernel_params(delta, cfg)
    return u.numpy_walk(C0, Xc, kid, a, b, cfg.polynomial_degree, cfg.θ_pivot_cholesky, cfg.max_model_points)


@pytest.fixture
def stand_ins(monkeypatch):
    from morbit.jl_amd import sampling

    log = {"batch": [], "single": [], "rc": 0, "start_rc": {}}

    def fake_batch(items, d, ctx=None):
        log["batch"].append([(np.asarray(C0).shape, np.asarray(Xc).shape) for _, C0, Xc, _ in items])
        if log["rc"] != 0:
            return log["rc"], None, 0.0
        return 0, [(log["start_rc"][k], []) if k in log["start_rc"] else (0, _walk(cfg, C0, Xc, delta))
                   for k, (cfg, C0, Xc, delta) in enumerate(items)], 0.5

    def fake_single(sites, lb_2, ub_2, x, delta, found, cfg, ctx=None, **kw):
        sites = np.asarray(sites, dtype=np.float64)
        cand = sampling.results_in_box_indices(sites, lb_2, ub_2, found)
        log["single"].append((len(found), len(cand)))
        if not cand or len(found) < u.poly_dim(sites.shape[1], cfg.polynomial_degree):
            return []                   # (a start set without the tail is the host mirror's business, not this stand-in's)
        return [cand[p] for p in _walk(cfg, sites[list(found)], sites[cand], delta)]

    monkeypatch.setattr(sampling, "rbf_round4_batch_device", fake_batch)
    monkeypatch.setattr(sampling, "_rbf_round4", fake_single)
    return log


def _starts(specs, seed=3):
    """specs: (d, n0, candidates in the box, sites outside it) -> databases, boxes, centres, found indices"""
    rng = np.random.default_rng(seed)
    dbs, lbs, ubs, xs, found = [], [], [], [], []
    for d, n0, mc, outside in specs:
        C0, Xc = u.clustered_case(int(rng.integers(1 << 30)), d, n0, mc, scale=10.0)
        far = 20.0 + rng.random((outside, d))
        order = rng.permutation(n0 + mc + outside)
        db = np.vstack([C0, Xc, far])[order]
        dbs.append(db)
        found.append([int(np.where(order == i)[0][0]) for i in range(n0)])
        lbs.append(np.full(d, -1.0)), ubs.append(np.full(d, 11.0)), xs.append(C0[0])
    return dbs, lbs, ubs, xs, found


def _cfg(**kw):
    import morbit.jl_amd as pkg

    return pkg.RbfConfig(**{"kernel": "cubic", "polynomial_degree": 1, "max_model_points": 10 ** 6, "θ_pivot_cholesky": 0.2, **kw})


def test_many_gives_what_the_single_function_gives(lib, stand_ins):
    from morbit.jl_amd import sampling

    # start 1: a start set that cannot carry the tail (n0 = 2 < q = 4): the single path, decided up front; start 3: no candidate in
    # the box; start 4: another d, alone in its group (below min_starts = 2); start 6: max_points reached
    dbs, lbs, ubs, xs, found = _starts([(3, 4, 30, 5), (3, 2, 20, 0), (3, 6, 41, 3), (3, 4, 0, 7), (5, 6, 25, 0), (3, 4, 12, 0), (3, 4, 9, 0)])
    cfgs = [_cfg(), _cfg(), _cfg(kernel="gaussian", θ_pivot_cholesky=0.1), _cfg(), _cfg(), _cfg(kernel="multiquadric", polynomial_degree=0), _cfg(max_model_points=4)]
    stats = {}
    got = sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, found, cfgs, stats=stats, min_starts=2)
    assert stand_ins["batch"][0] == [((4, 3), (30, 3)), ((6, 3), (41, 3)), ((4, 3), (12, 3))]
    alone = True
    assert len(stand_ins["batch"]) == (1 if alone else 2)
    assert stand_ins["single"] == [(2, 20)] + ([(6, 25)] if alone else [])
    assert stats == {"path": "batch", "batched": [0, 2, 5] + ([] if alone else [4]), "fallback": []}
    assert got[3] == [] and got[6] == []
    stand_ins["single"].clear()
    want = [sampling._rbf_round4(dbs[p], lbs[p], ubs[p], xs[p], 1.0, found[p], cfgs[p]) for p in range(7)]
    assert got == want and all(len(got[p]) > 3 for p in (0, 2, 4, 5))
    # database indices, not positions
    assert all(i not in found[0] and np.all(dbs[0][i] <= 11.0) for i in got[0])


def test_a_refused_batch_takes_the_loop(lib, stand_ins):
    from morbit.jl_amd import sampling

    dbs, lbs, ubs, xs, found = _starts([(3, 4, 30, 0), (3, 4, 22, 2), (3, 5, 17, 0)], seed=8)
    stand_ins["rc"] = -2
    stats = {}
    got = sampling.rbf_round4_many(dbs, lbs, ubs, xs, [1.0, 1.0, 1.0], found, _cfg(), stats=stats, min_starts=1)
    assert stats == {"path": "loop", "batched": [], "fallback": []}
    assert len(stand_ins["batch"]) == 1 and stand_ins["single"] == [(4, 30), (4, 22), (5, 17)]
    assert got == [sampling._rbf_round4(dbs[p], lbs[p], ubs[p], xs[p], 1.0, found[p], _cfg()) for p in range(3)]
    # a shape the decision table refuses: the batched entry is not even asked
    stand_ins["batch"].clear()
    real = lib.mrbf_dispatch_round4_batch
    try:
        lib.mrbf_dispatch_round4_batch = lambda n, d: 0
        assert sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, found, _cfg(), stats=stats, min_starts=1) == got
    finally:
        lib.mrbf_dispatch_round4_batch = real
    assert stand_ins["batch"] == [] and stats["path"] == "loop"


def test_a_start_s_own_rc_is_honoured(lib, stand_ins):
    from morbit.jl_amd import _lib, sampling

    dbs, lbs, ubs, xs, found = _starts([(3, 4, 30, 0), (3, 4, 22, 2), (3, 5, 17, 0)], seed=9)
    stand_ins["start_rc"] = {1: _lib.MRBF_ESINGULAR}         # what mrbf_round4 said for start 1: take the reference method for it
    stats = {}
    got = sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, found, _cfg(), stats=stats, min_starts=1)
    assert stats == {"path": "batch", "batched": [0, 2], "fallback": [1]} and stand_ins["single"] == [(4, 22)]
    assert got == [sampling._rbf_round4(dbs[p], lbs[p], ubs[p], xs[p], 1.0, found[p], _cfg()) for p in range(3)]
    # a code that is an error stays one
    stand_ins["start_rc"] = {2: _lib.MRBF_EHIP}

    class Ctx:
        def check(self, rc):
            raise _lib.MrbfError(rc, "stand-in")

    with pytest.raises(_lib.MrbfError) as ei:
        sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, found, _cfg(), ctx=Ctx(), min_starts=1)
    assert ei.value.code == _lib.MRBF_EHIP


def test_the_measured_rule_keeps_the_single_calls_where_the_batch_does_not_pay(lib, stand_ins):
    from morbit.jl_amd import sampling

    pays = sampling.round4_batch_pays
    assert [pays(10, 300), pays(8, 256), pays(8, 300), pays(7, 100), pays(8, 1400), pays(43, 1400), pays(44, 1400), pays(64, 1400), pays(64, 4096)] == \
        [True, True, False, False, False, False, True, True, False]
    # three starts: the loop, by the rule; nine starts of 30 candidates: the batch
    dbs, lbs, ubs, xs, found = _starts([(3, 4, 30, 0)] * 9, seed=12)
    stats = {}
    few = sampling.rbf_round4_many(dbs[:3], lbs[:3], ubs[:3], xs[:3], 1.0, found[:3], _cfg(), stats=stats)
    assert stats["path"] == "loop" and stand_ins["batch"] == [] and len(stand_ins["single"]) == 3
    got = sampling.rbf_round4_many(dbs, lbs, ubs, xs, 1.0, found, _cfg(), stats=stats)
    assert stats["path"] == "batch" and stats["batched"] == list(range(9)) and got[:3] == few
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    assert int(re.search(r"const ROUND4_BATCH_CANDIDATES_PER_START = (\d+)", jl).group(1)) == sampling.ROUND4_BATCH_CANDIDATES_PER_START


def test_nothing_to_do(lib, stand_ins):
    from morbit.jl_amd import sampling

    stats = {}
    assert sampling.rbf_round4_many([], [], [], [], [], [], [], stats=stats) == []
    assert stats == {"path": "loop", "batched": [], "fallback": []} and stand_ins["batch"] == [] and stand_ins["single"] == []


# ---- the margin helper ------------------------------------------------------------------------------------------------------

def test_margin_helper_flags_a_borderline_decision():
    kid, a, b = u.KERNELS["cubic"]
    C0, Xc = u.random_case(5, 3, 4, 8, scale=10.0)
    _, taus = u.margins(C0, Xc, kid, a, b, 1, 1e-7, 10 ** 6)
    assert len(taus) == 8 and all(t is not None and t > 1.0 for _, t in taus)
    t3 = taus[3][1]
    # the walk up to decision 3 does not depend on the threshold while everything before it is accepted: put the threshold next to t3
    for factor, flagged in ((1.5, True), (1.0 / 1.5, True), (99.0, True), (1.0 / 99.0, True), (101.0, False), (1.0 / 101.0, False)):
        theta = (t3 * factor) ** 0.25
        if any(t <= (theta ** 4) * 100.0 for _, t in taus[:3]):
            continue
        acc, tt = u.margins(C0, Xc, kid, a, b, 1, theta, 10 ** 6)
        assert tt[3][1] == pytest.approx(t3, rel=1e-9)
        assert (3 in [p for p, _ in u.margin_violations(tt, theta)]) == flagged, factor
        assert (3 in acc) == (factor < 1.0)
    # an exact copy of an accepted candidate: a clear rejection at theta = 0.2, undecidable at the default theta (threshold 1e-28)
    Xd = Xc.copy()
    Xd[5] = Xd[2]
    noise = 1000.0 * np.finfo(float).eps * u.kernel_scale(C0, Xd, kid, a, b)
    acc, tt = u.margins(C0, Xd, kid, a, b, 1, 0.2, 10 ** 6)
    assert 5 not in acc and u.margin_violations(tt, 0.2, noise=noise) == []
    acc, tt = u.margins(C0, Xd, kid, a, b, 1, 1e-7, 10 ** 6)
    assert 5 in [p for p, _ in u.margin_violations(tt, 1e-7, noise=noise)]
    with pytest.raises(AssertionError, match="unfit test input"):
        u.oracle_case(("host", "unfit"), C0, Xd, "cubic", 1, 1e-7, 10 ** 6)


def test_margin_walk_is_the_oracle_s_and_the_kernel_s_arithmetic_agrees():
    """the helper's list equals oracle/sampling_oracle.py::rbf_round4's (asserted inside oracle_case), the share of rejections is what the
    clusters give, and the NumPy restatement of the batched kernel's arithmetic gives the same list on a fit input"""
    for kernel, deg, theta in (("cubic", 1, 0.2), ("gaussian", 0, 0.1), ("multiquadric", 1, 0.2), ("inv_multiquadric", -1, 0.1)):
        C0, Xc = u.clustered_case(17, 3, 5, 36, scale=10.0)
        acc, share = u.oracle_case(("host", kernel), C0, Xc, kernel, deg, theta, 10 ** 6)
        assert 0.25 <= share <= 0.75 and len(acc) == 18
        kid, a, b = u.KERNELS[kernel]
        assert u.numpy_walk(C0, Xc, kid, a, b, deg, theta, 10 ** 6) == acc
        assert u.numpy_walk(C0, Xc, kid, a, b, deg, theta, 5 + 7) == acc[:7]
