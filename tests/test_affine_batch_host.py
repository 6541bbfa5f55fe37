"""CPU tests of the many-start site selection (mrbf_affine_select_batch): its decision-table row, the job struct's mirrors against the
header, and the routing of `sampling.affine_collect_many` -- which filters form the batch, which run `collect()`, and what happens
when the library refuses the batch.  No GPU: the device calls are replaced by host stand-ins that do what the kernels do (scan plus
one reflector per pick)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


@pytest.mark.parametrize("n_starts, d, p_is_inf, device", [
    (1, 128, 1, True),
    (64, 128, 1, True),
    (65535, 128, 1, True),
    (0, 128, 1, False),
    (65536, 128, 1, False),
    (64, 1, 1, True),
    (64, 1023, 1, True),            # 8 * 1024 coordinates of 8 bytes = 64 KiB
    (64, 1024, 1, False),
    (64, 0, 1, False),
    (64, 128, 0, False),            # the 2-norm's column sums would depend on the order of arrival
    (1, 1023, 0, False),
    (65535, 1023, 1, True),
])
def test_decision_table_row(lib, n_starts, d, p_is_inf, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_affine_batch(n_starts, d, p_is_inf) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)


def test_return_codes_that_mean_reference(lib):
    from morbit.jl_amd import _lib

    assert _lib.ENTRY_AFFINE_BATCH == 10
    assert lib.mrbf_dispatch_after(10, -2) == 1
    assert lib.mrbf_dispatch_after(10, -5) == 0 and lib.mrbf_dispatch_after(10, 0) == 0 and lib.mrbf_dispatch_after(10, _lib.MRBF_EHIP) == 0
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert re.search(r"MRBF_ENTRY_AFFINE_BATCH = 10\b", text)
    # the contract sits next to the reference lines the call replaces
    doc = text[text.index("The pick loop for a batch of starts"):text.index("} mrbf_affine_job;")]
    assert "bit for bit" in doc and "AffinelyIndependentPoints.jl:71-106" in doc
    assert re.search(r"do not depend on the start's position in the batch\s+\*?\s*or on which other starts share it", doc)
    # without a context nothing is touched
    assert lib.mrbf_affine_select_batch(None, 1, 3, 1, None, None) == -1


def test_job_mirror_matches_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mrbf_affine_job;", text).group(1)
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
    assert total == 64 == ctypes.sizeof(_lib.AffineJob)
    assert [f[0] for f in _lib.AffineJob._fields_] == [n for n, _, _ in layout]
    assert [n for n, _, _ in layout] == ["mc", "j0", "max_picks", "pivot_val", "shifted", "Q0", "picked_out", "Z_out", "n_picked", "reserved"]
    for name, o, size in layout:
        fld = getattr(_lib.AffineJob, name)
        assert (fld.offset, fld.size) == (o, size), name
    # the Julia mirror carries the same fields in the same order
    jl = open(os.path.join(ROOT, "morbit.jl_amd", "julia", "HipRbf.jl"), encoding="utf-8").read()
    jbody = re.search(r"^struct MrbfAffineJob\b[^\n]*\n(.*?)^end", jl, flags=re.S | re.M).group(1)
    jfields = re.findall(r"(\w+)::(Int32|Int64|Float64|Ptr\{\w+\})", jbody)
    jsize = {"Int32": 4, "Int64": 8, "Float64": 8}
    assert [(n, 8 if t.startswith("Ptr{") else jsize[t], t.startswith("Ptr{")) for n, t in jfields] == fields
    assert re.search(r"ccall\(\(:mrbf_affine_select_batch, libmrbf\)", jl) and re.search(r"ccall\(\(:mrbf_dispatch_affine_batch, libmrbf\)", jl)


def _host_pick_loop(Sd, qr, want, pivot, p=np.inf):
    """what the pick kernels do, on the host: scan + one reflector per pick (as tests/test_dispatch.py's stand-in for the single call)"""
    Sd = Sd.copy()
    got = []
    Z = qr.complement(p)
    while len(got) < want:
        v = np.abs((Sd @ Z) @ Z.T).max(axis=1) if Z.shape[1] else np.zeros(Sd.shape[0])
        b = int(np.argmax(v))
        if not v[b] > pivot:
            break
        qr.append(Sd[b].copy())
        Sd[b] = 0.0
        Z = qr.complement(p)
        got.append(b)
    return got, Z


@pytest.fixture
def stand_ins(monkeypatch):
    from morbit.jl_amd import sampling

    log = {"batch": [], "single": [], "rc": 0}

    def fake_batch(items, d, p=np.inf, ctx=None):
        log["batch"].append([(Sd.shape, qr.j, want) for Sd, qr, want, _ in items])
        if log["rc"] != 0:
            return log["rc"], None, 0.0
        return 0, [_host_pick_loop(Sd, qr, want, pivot, p) for Sd, qr, want, pivot in items], 0.5

    def fake_select(self, Sd, qr, want):
        log["single"].append(Sd.shape)
        return _host_pick_loop(Sd, qr, want, self.pivot_val, self.p)

    monkeypatch.setattr(sampling, "affine_select_batch_device", fake_batch)
    monkeypatch.setattr(sampling.AffinelyIndependentPointFilter, "_select_device", fake_select)
    return log


def _filters(specs, seed=5):
    """specs: (d, candidates, n or None) -> two equal lists of filters"""
    from morbit.jl_amd import sampling

    rng = np.random.default_rng(seed)
    a, b = [], []
    for d, n, want in specs:
        x = rng.random(d)
        seeds = [x + 0.1 * rng.standard_normal(d) for _ in range(n)]
        for lst in (a, b):
            lst.append(sampling.AffinelyIndependentPointFilter(x, seeds, n=want, pivot_val=1e-3))
    return a, b


def test_collect_many_gives_what_collect_gives(lib, stand_ins):
    from morbit.jl_amd import sampling

    # d = 4 needs 8192 candidates for the device; d = 64 only as many as directions (mrbf_dispatch_affine)
    specs = [(4, 9000, None), (4, 50, None), (64, 70, None), (4, 8500, 3), (64, 40, None), (4, 0, None), (64, 200, 5)]
    many, single = _filters(specs)
    stats = {}
    got = sampling.affine_collect_many(many, stats=stats)
    assert stats == {"path": "batch", "batched": [0, 2, 3, 6]}
    # one batched call per dimension, with the first pick already taken on the host
    assert sorted(stand_ins["batch"], key=lambda c: c[0][0][1]) == [[((9000, 4), 1, 3), ((8500, 4), 1, 2)], [((70, 64), 1, 63), ((200, 64), 1, 4)]]
    assert stand_ins["single"] == []
    want = [f.collect() for f in single]
    assert stand_ins["single"] == [(9000, 4), (70, 64), (8500, 4), (200, 64)]
    assert got == want and got[5] == [] and len(got[3]) == 3 and len(got[6]) == 5
    for f, g in zip(many, single):
        assert np.array_equal(f.Y, g.Y) and np.array_equal(f.Z, g.Z)


def test_a_refused_batch_takes_the_loop(lib, stand_ins):
    from morbit.jl_amd import sampling

    many, single = _filters([(4, 9000, None), (4, 30, None), (4, 8300, 2)], seed=9)
    stand_ins["rc"] = -2
    stats = {}
    got = sampling.affine_collect_many(many, stats=stats)
    assert stats == {"path": "loop", "batched": []}
    assert len(stand_ins["batch"]) == 1 and stand_ins["single"] == [(9000, 4), (8300, 4)]
    assert got == [f.collect() for f in single]
    for f, g in zip(many, single):
        assert np.array_equal(f.Y, g.Y) and np.array_equal(f.Z, g.Z)
    # a shape the decision table refuses (the 2-norm): the batched entry is not even asked
    stand_ins["batch"].clear()
    a, b = _filters([(4, 9000, None), (4, 9000, None)], seed=3)
    for f in a + b:
        f.p = 2
    stats = {}
    assert sampling.affine_collect_many(a, stats=stats) == [f.collect() for f in b]
    assert stand_ins["batch"] == [] and stats["path"] == "loop"


def test_nothing_to_do(lib, stand_ins):
    from morbit.jl_amd import sampling

    stats = {}
    assert sampling.affine_collect_many([], stats=stats) == [] and stats == {"path": "loop", "batched": []}
    assert sampling.find_suitable_points_many([], [], [], [], [], 1e-3) == []
    assert stand_ins["batch"] == [] and stand_ins["single"] == []


def test_find_suitable_points_many_through_two_rounds(lib, stand_ins):
    """round 1 in the box, round 2 continued from each start's own Y / Z with its own n_missing in a larger box"""
    from morbit.jl_amd import sampling

    rng = np.random.default_rng(11)
    d, ns = 64, 3
    dbs = []
    for p, rank in enumerate((20, 25, 30)):     # the small box's sites span `rank` directions only: round 1 stops at the pivot test
        w = np.full(d, 1e-5)
        w[:rank] = 0.1
        dbs.append(np.vstack([np.full(d, 0.5), 0.5 + w * (2 * rng.random((150 + 10 * p, d)) - 1), 0.5 + 0.3 * (2 * rng.random((150, d)) - 1)]))
    xs = [db[0] for db in dbs]
    lb1, ub1 = [x - 0.1 for x in xs], [x + 0.1 for x in xs]
    lb2, ub2 = [x - 0.3 for x in xs], [x + 0.3 for x in xs]
    piv1, piv2 = 0.02, 0.02
    stats = {}
    r1 = sampling.find_suitable_points_many(dbs, lb1, ub1, xs, [0] * ns, piv1, stats=stats)
    w1 = [sampling._find_suitable_points(dbs[p], lb1[p], ub1[p], xs[p], 0, piv1) for p in range(ns)]
    assert stats["path"] == "batch"
    missing = [d - len(r[0]) for r in r1]
    assert missing == [44, 39, 34]                                # round 2 has something to continue from and something to find
    r2 = sampling.find_suitable_points_many(dbs, lb2, ub2, xs, [0] * ns, piv2, already_inspected_indices=[r[2] for r in r1],
                                            Ys=[r[3] for r in r1], Zs=[r[4] for r in r1], n_missing=missing, stats=stats)
    w2 = [sampling._find_suitable_points(dbs[p], lb2[p], ub2[p], xs[p], 0, piv2, already_inspected_indices=w1[p][2], Y=w1[p][3], Z=w1[p][4],
                                         n_missing=missing[p]) for p in range(ns)]
    for got, want in ((r1, w1), (r2, w2)):
        for g, w in zip(got, want):
            assert g[0] == w[0] and g[2] == w[2] and np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4])
            assert len(g[1]) == len(w[1]) and all(np.array_equal(a, b) for a, b in zip(g[1], w[1]))
    assert [len(r[0]) for r in r2] == missing and stats["path"] == "batch"
