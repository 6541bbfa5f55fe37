"""A start's evaluation database kept resident on the device (include/mrbf.h "resident site database", csrc/db.hip).

`DeviceDatabase` mirrors the reference's ArrayDB (src/Databases.jl): sites and values in insertion order, a row's position being its
id, appended to as the run goes.  `box_many` is results_in_box_indices (Databases.jl:324-327) with the filter's shifted rows and first
pick (AffinelyIndependentPoints.jl:25, :53) for a batch of starts in one call, `gather_many` the row gathers of round 4 and the fit
(RbfModel.jl:372, :747-757).  Their outputs are `DeviceView`s -- a device pointer with a shape -- which `_lib.as_ptr` and
`rbf_model._as_fit_input` take like a device tensor, so the batched calls read them in place.

A database keeps a host copy of its sites and values, as the caller's own database does: the small host-side steps (the filter's Y,
the fall-backs to the host filter or to the single calls) need no read-back, and when the decision table (mrbf_dispatch_db_batch) sends a
call to the host, the scan and the copies run on that copy.  `HostDatabase` is that copy alone; the batched functions take lists of
either kind (one kind per call) and serve host databases by their host branch, without a context.
"""
import ctypes

import numpy as np

from . import _lib

_NAN = np.float64(np.nan)


class DeviceView:
    """`shape` doubles, row-major, at device address `ptr`, owned by the library (its lifetime is the view's, include/mrbf.h).
    `host` (optional): a callable that returns the same rows from the host copy, for the code paths that want a NumPy array."""

    def __init__(self, ptr, shape, host=None):
        self.ptr, self.shape, self._host = int(ptr or 0), tuple(int(v) for v in shape), host

    @property
    def ndim(self):
        return len(self.shape)

    def data_ptr(self):
        return self.ptr

    def contiguous(self):
        return self

    def reshape(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        total = int(np.prod(self.shape, dtype=np.int64))
        known = int(np.prod([v for v in shape if v != -1], dtype=np.int64))
        shape = tuple((total // known if known else 0) if v == -1 else int(v) for v in shape)
        assert int(np.prod(shape, dtype=np.int64)) == total, "reshape of %r to %r" % (self.shape, shape)
        host = self._host
        return DeviceView(self.ptr, shape, None if host is None else (lambda: host().reshape(shape)))

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            raise TypeError("this DeviceView has no host copy")
        a = np.asarray(self._host(), dtype=np.float64).reshape(self.shape)
        return a if dtype is None else a.astype(dtype, copy=False)


def _host_rows(a):
    if hasattr(a, "data_ptr"):          # a torch tensor, host or device
        return a.detach().cpu().numpy()
    return a


class HostDatabase:
    """the sites (d) and values (k) of one start on the host, rows in insertion order: the database of a start where the device is not
    asked, and the host copy a `DeviceDatabase` keeps.  The many-start drivers (`sampling.prepare_update_models`) take either kind."""

    def __init__(self, d, k, capacity=0):
        self.d, self.k, self._n = int(d), int(k), 0
        self._S, self._V = np.empty((max(int(capacity), 16), self.d)), np.empty((max(int(capacity), 16), self.k))

    @classmethod
    def of_sites(cls, sites, d):
        """a plain (N, d) array or list of sites as a database without values; the caller's array is read, never written"""
        db = cls.__new__(cls)
        S = np.asarray(sites, dtype=np.float64).reshape(-1, int(d)).view()
        S.flags.writeable = False
        db.d, db.k, db._n, db._S, db._V = int(d), 0, S.shape[0], S, np.empty((S.shape[0], 0))
        return db

    def __len__(self):
        return self._n

    @property
    def sites(self):
        return self._S[: self._n]

    @property
    def values(self):
        return self._V[: self._n]

    def _adopt_rows(self, S, V=None):
        """m new rows on the host: `S` m x d, `V` m x k or None (NaN); the capacity doubles when they do not fit"""
        n, m = self._n, int(S.shape[0])
        if m == 0:
            return
        if n + m > self._S.shape[0]:
            cap = max(2 * self._S.shape[0], n + m)
            self._S = np.concatenate([self._S[:n], np.empty((cap - n, self.d))])
            self._V = np.concatenate([self._V[:n], np.empty((cap - n, self.k))])
        self._S[n: n + m] = S
        self._V[n: n + m] = _NAN if V is None else V
        self._n += m

    def append(self, sites, values=None):
        """new_result! for m rows: `sites` m x d, `values` m x k or None (unevaluated rows, stored as NaN: round 3, RbfModel.jl:303).
        Returns the position of the first new row."""
        S = np.asarray(_host_rows(sites), dtype=np.float64).reshape(-1, self.d)
        first = self._n
        self._adopt_rows(S, None if values is None else np.asarray(_host_rows(values), dtype=np.float64).reshape(S.shape[0], self.k))
        return first

    def set_values(self, indices, values):
        """eval_missing! (Databases.jl:258-277): the values of the rows `indices` (distinct positions)"""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size:
            self._V[idx] = np.asarray(_host_rows(values), dtype=np.float64).reshape(idx.size, self.k)


class DeviceDatabase(HostDatabase):
    """mrbf_db: the sites (d) and values (k) of one start resident on the device, with the host copy (`sites`, `values`) it inherits"""

    def __init__(self, d, k, ctx=None, capacity=0):
        super().__init__(d, k, capacity)
        self.ctx = ctx or _lib.default_context()
        h = _lib.c_vp()
        self.ctx.check(self.ctx.lib.mrbf_db_create(self.ctx.h, self.d, self.k, int(capacity), ctypes.byref(h)))
        self.h = h

    def append(self, sites, values=None):
        """`HostDatabase.append` on the device and on the host copy; NumPy arrays or torch tensors (a device tensor is read in place)"""
        S = sites.contiguous() if hasattr(sites, "data_ptr") else _lib.host_f64(sites).reshape(-1, self.d)
        m = int(S.shape[0]) if S.ndim == 2 else int(S.numel() // self.d)
        V = None
        if values is not None:
            V = values.contiguous() if hasattr(values, "data_ptr") else _lib.host_f64(values).reshape(m, self.k)
        first = ctypes.c_int64(-1)
        self.ctx.check(self.ctx.lib.mrbf_db_append(self.ctx.h, self.h, m, _lib.as_ptr(S), _lib.as_ptr(V), ctypes.byref(first)))
        at = super().append(S, V)
        assert first.value == at
        return at

    def set_values(self, indices, values):
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        V = values.contiguous() if hasattr(values, "data_ptr") else _lib.host_f64(values).reshape(idx.size, self.k)
        self.ctx.check(self.ctx.lib.mrbf_db_set_values(self.ctx.h, self.h, idx.size, _lib.as_ptr(idx), _lib.as_ptr(V)))
        super().set_values(idx, V)

    def read(self, first=0, m=None):
        """rows first .. first + m - 1 as the device holds them -> (sites, values)"""
        m = self._n - first if m is None else int(m)
        S, V = np.empty((m, self.d)), np.empty((m, self.k))
        self.ctx.check(self.ctx.lib.mrbf_db_read(self.ctx.h, self.h, int(first), m, _lib.as_ptr(S), _lib.as_ptr(V)))
        return S, V

    def dims(self):
        n, d, k = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        self.ctx.check(self.ctx.lib.mrbf_db_dims(self.h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(k)))
        return int(n.value), int(d.value), int(k.value)

    def free(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.mrbf_db_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def as_databases(dbs, xs):
    """the databases of one call of a many-start driver -> (list of databases, resident): every entry is a `DeviceDatabase`, a
    `HostDatabase`, or a plain (N, d) array or list of sites (d that of the start's centre `xs[p]`), which is wrapped; all of one kind"""
    dbs = [db if isinstance(db, HostDatabase) else HostDatabase.of_sites(db, np.size(xs[p])) for p, db in enumerate(dbs)]
    return dbs, _resident(dbs)


def _resident(dbs):
    kinds = {isinstance(db, DeviceDatabase) for db in dbs}
    assert len(kinds) <= 1, "the databases of a call are all resident or all on the host"
    return kinds == {True}


class BoxResult:
    """one start of `box_many`: `indices` (database positions of the candidates, ascending), `mc`, `first_pick` (position among the
    candidates, -1 without candidates), `first_row` (its shifted row), `sites` / `shifted` (mc x d: DeviceViews, or NumPy arrays when
    the call ran on the host copy), `rc`"""
    __slots__ = ("indices", "mc", "first_pick", "first_row", "sites", "shifted", "rc")


def _box_host(db, lb, ub, x0, exclude, p, zero_first_pick):
    from .sampling import results_in_box_indices

    r = BoxResult()
    r.indices = [int(i) for i in results_in_box_indices(db.sites, lb, ub, exclude)]
    r.mc, r.rc = len(r.indices), 0
    r.sites = db.sites[r.indices].copy() if r.mc else np.empty((0, db.d))
    r.shifted = r.sites - x0
    r.first_pick, r.first_row = -1, None
    if r.mc:
        r.first_pick = int(np.argmax(np.linalg.norm(r.shifted, ord=p, axis=1)))
        r.first_row = r.shifted[r.first_pick].copy()
        if zero_first_pick:
            r.shifted[r.first_pick] = 0.0
    return r


def box_many(dbs, lbs, ubs, x0s, excludes, p=np.inf, zero_first_pick=True, ctx=None, stats=None):
    """results_in_box_indices + shifted rows + the filter's first pick for a list of databases of one d in ONE call
    (mrbf_db_box_batch) -> list of BoxResult.  `excludes[p]`: positions to leave out (duplicates and positions outside the database
    allowed).  On host databases, and where mrbf_dispatch_db_batch sends the call to the host (or it returns -2), the same runs on the
    host copies, without a context; stats["path"] = "device" or "host".  The views stay valid until the next `box_many` on the context."""
    ns = len(dbs)
    stats = stats if stats is not None else {}
    resident = _resident(dbs)
    d = dbs[0].d if ns else 1
    assert all(db.d == d for db in dbs), "the databases of a call share d"
    x0s = [_lib.host_f64(x).reshape(d) for x in x0s]

    def host():
        stats["path"] = "host"
        return [_box_host(dbs[q], np.asarray(lbs[q], dtype=np.float64), np.asarray(ubs[q], dtype=np.float64), x0s[q], excludes[q], p,
                          zero_first_pick) for q in range(ns)]

    if not resident or _lib.load().mrbf_dispatch_db_batch(ns, d) != _lib.DISPATCH_DEVICE:
        return host()
    ctx = ctx or dbs[0].ctx
    jobs = (_lib.DbBoxJob * ns)()
    keep = []
    for q, db in enumerate(dbs):
        lb, ub = _lib.host_f64(lbs[q]).reshape(d), _lib.host_f64(ubs[q]).reshape(d)
        ex = np.ascontiguousarray(list(excludes[q]), dtype=np.int64).reshape(-1)
        idx, row = np.empty(max(len(db), 1), dtype=np.int64), np.empty(d)
        keep.append((lb, ub, ex, idx, row))
        J = jobs[q]
        J.db, J.lb, J.ub, J.x0 = db.h, lb.ctypes.data, ub.ctypes.data, x0s[q].ctypes.data
        J.n_exclude, J.exclude = ex.size, ex.ctypes.data if ex.size else None
        J.zero_first_pick, J.indices_out, J.first_row = 1 if zero_first_pick else 0, idx.ctypes.data, row.ctypes.data
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_db_box_batch(ctx.h, ns, d, 1 if np.isinf(p) else 0, jobs, ctypes.byref(ms))
    if rc != 0:
        if ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_BOX, rc):
            return host()
        ctx.check(rc)
    out = []
    for q, db in enumerate(dbs):
        J, (_, _, _, idx, row) = jobs[q], keep[q]
        if J.rc != 0:
            raise _lib.MrbfError(J.rc, "mrbf_db_box_batch: start %d" % q)
        r = BoxResult()
        r.mc, r.first_pick, r.rc = int(J.mc), int(J.first_pick), 0
        r.indices = [int(v) for v in idx[: r.mc]]
        r.first_row = row if r.mc else None
        x0, cand, zero = x0s[q], r.indices, bool(zero_first_pick)

        def host_shifted(db=db, cand=cand, x0=x0, pick=r.first_pick, zero=zero):
            S = db.sites[cand] - x0
            if zero and pick >= 0:
                S[pick] = 0.0
            return S

        r.sites = DeviceView(J.cand_sites_dev, (r.mc, d), lambda db=db, cand=cand: db.sites[cand])
        r.shifted = DeviceView(J.shifted_dev, (r.mc, d), host_shifted)
        out.append(r)
    stats.update(path="device", ms_total=float(ms.value))
    return out


class GatherResult:
    """one start of `gather_many`: `sites` (n_idx x d) and `values` (n_idx x k) in the order of the index list -- DeviceViews, or
    NumPy arrays when the call ran on the host copy -- and `rc` (-3: an index outside the database; sites and values are None)"""
    __slots__ = ("sites", "values", "rc")


def gather_many(dbs, index_lists, ctx=None, stats=None):
    """the rows `index_lists[p]` (any order, repeats allowed) of every database of one d in ONE call (mrbf_db_gather_batch) -> list of
    GatherResult.  Host databases, and the fall-backs, as in `box_many`.  The views stay valid until the next `gather_many` on the context."""
    ns = len(dbs)
    stats = stats if stats is not None else {}
    resident = _resident(dbs)
    d = dbs[0].d if ns else 1
    assert all(db.d == d for db in dbs), "the databases of a call share d"
    lists = [np.ascontiguousarray(list(l), dtype=np.int64).reshape(-1) for l in index_lists]

    def host():
        stats["path"] = "host"
        out = []
        for db, idx in zip(dbs, lists):
            r = GatherResult()
            ok = bool(np.all((idx >= 0) & (idx < len(db))))
            r.rc = 0 if ok else -3
            r.sites, r.values = (db.sites[idx].copy(), db.values[idx].copy()) if ok else (None, None)
            out.append(r)
        return out

    if not resident or _lib.load().mrbf_dispatch_db_batch(ns, d) != _lib.DISPATCH_DEVICE:
        return host()
    ctx = ctx or dbs[0].ctx
    jobs = (_lib.DbGatherJob * ns)()
    for q, db in enumerate(dbs):
        jobs[q].db, jobs[q].n_idx, jobs[q].indices = db.h, lists[q].size, lists[q].ctypes.data if lists[q].size else None
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_db_gather_batch(ctx.h, ns, d, jobs, ctypes.byref(ms))
    if rc != 0:
        if ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_GATHER, rc):
            return host()
        ctx.check(rc)
    out = []
    for q, db in enumerate(dbs):
        r, idx = GatherResult(), lists[q]
        r.rc = int(jobs[q].rc)
        r.sites = r.values = None
        if r.rc == 0:
            r.sites = DeviceView(jobs[q].sites_dev, (idx.size, d), lambda db=db, idx=idx: db.sites[idx])
            r.values = DeviceView(jobs[q].values_dev, (idx.size, db.k), lambda db=db, idx=idx: db.values[idx])
        out.append(r)
    stats.update(path="device", ms_total=float(ms.value))
    return out


def append_many(dbs, sites_list, values_list=None, ctx=None, stats=None):
    """`DeviceDatabase.append` for every database of the list in ONE call (mrbf_db_append_batch: one packed upload, one launch, one
    synchronisation) -- the trial points of an iteration.  `sites_list[p]`: m_p x d_p, `values_list[p]`: m_p x k_p or None (unevaluated
    rows); NumPy arrays or torch tensors.  Returns the position of the first new row per database; the host copies are kept in step.
    On host databases, and where mrbf_dispatch_db_batch sends the call to the host, it is the loop of single appends; stats["path"]
    says which."""
    ns = len(dbs)
    stats = stats if stats is not None else {}
    if ns == 0:
        return []
    resident = _resident(dbs)
    values_list = [None] * ns if values_list is None else values_list

    def loop():
        stats["path"] = "loop"
        return [db.append(sites_list[q], values_list[q]) for q, db in enumerate(dbs)]

    if not resident or _lib.load().mrbf_dispatch_db_batch(ns, 1) != _lib.DISPATCH_DEVICE:
        return loop()
    ctx = ctx or dbs[0].ctx
    jobs = (_lib.DbAppendJob * ns)()
    keep = []
    for q, db in enumerate(dbs):
        S = sites_list[q]
        S = S.contiguous() if hasattr(S, "data_ptr") else _lib.host_f64(S).reshape(-1, db.d)
        m = int(S.shape[0]) if S.ndim == 2 else int(S.numel() // db.d)
        V = values_list[q]
        if V is not None:
            V = V.contiguous() if hasattr(V, "data_ptr") else _lib.host_f64(V).reshape(m, db.k)
        keep.append((S, V, m))
        J = jobs[q]
        J.db, J.m = db.h, m
        J.sites, J.values = (_lib.as_ptr(S) if m else None), (_lib.as_ptr(V) if (V is not None and m) else None)
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_db_append_batch(ctx.h, ns, jobs, ctypes.byref(ms))
    if rc != 0:
        if ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_APPEND_BATCH, rc):
            return loop()
        ctx.check(rc)
    out = []
    for q, db in enumerate(dbs):
        S, V, m = keep[q]
        if jobs[q].rc != 0:
            raise _lib.MrbfError(jobs[q].rc, "mrbf_db_append_batch: start %d" % q)
        assert int(jobs[q].first_index) == len(db)
        out.append(len(db))
        HostDatabase.append(db, S, V)
    stats.update(path="device", ms_total=float(ms.value))
    return out


def set_values_many(dbs, index_lists, values_list, ctx=None, stats=None, strict=True):
    """`DeviceDatabase.set_values` (eval_missing!, Databases.jl:258-277) for every database of the list in ONE call
    (mrbf_db_set_values_batch).  Returns the rc of every start: 0, or -4 for an index list with a position outside the database --
    nothing of that start is written; with `strict` that raises after the other starts are done.  The host copies are kept in step.
    Host databases take the loop of single calls."""
    ns = len(dbs)
    stats = stats if stats is not None else {}
    if ns == 0:
        return []
    resident = _resident(dbs)
    idxs = [np.ascontiguousarray(list(l) if not isinstance(l, np.ndarray) else l, dtype=np.int64).reshape(-1) for l in index_lists]

    def loop():
        stats["path"] = "loop"
        rcs = []
        for q, db in enumerate(dbs):
            try:
                db.set_values(idxs[q], values_list[q])
                rcs.append(0)
            except _lib.MrbfError as e:
                if strict or e.code != -4:
                    raise
                rcs.append(e.code)
        return rcs

    if not resident or _lib.load().mrbf_dispatch_db_batch(ns, 1) != _lib.DISPATCH_DEVICE:
        return loop()
    ctx = ctx or dbs[0].ctx
    jobs = (_lib.DbSetValuesJob * ns)()
    keep = []
    for q, db in enumerate(dbs):
        m = idxs[q].size
        V = values_list[q]
        V = V.contiguous() if hasattr(V, "data_ptr") else _lib.host_f64(V).reshape(m, db.k)
        keep.append(V)
        J = jobs[q]
        J.db, J.m = db.h, m
        J.indices, J.values = (idxs[q].ctypes.data if m else None), (_lib.as_ptr(V) if m else None)
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_db_set_values_batch(ctx.h, ns, jobs, ctypes.byref(ms))
    if rc != 0:
        if ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DB_SET_VALUES_BATCH, rc):
            return loop()
        ctx.check(rc)
    rcs = []
    for q, db in enumerate(dbs):
        rcs.append(int(jobs[q].rc))
        if rcs[q] == 0:
            HostDatabase.set_values(db, idxs[q], keep[q])
    stats.update(path="device", ms_total=float(ms.value))
    bad = [q for q, r in enumerate(rcs) if r != 0]
    if strict and bad:
        raise _lib.MrbfError(rcs[bad[0]], "mrbf_db_set_values_batch: start %d has an index outside its database" % bad[0])
    return rcs
