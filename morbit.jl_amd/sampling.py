"""Host-side mirror of Morbit's RBF training-site selection around the device kernels.

Mirrors AffinelyIndependentPointFilter / _find_suitable_points (src/models/AffinelyIndependentPoints.jl:14-106,
src/models/RbfModel.jl:205-238) -- small d x d QRs that stay on the host, SURVEY.md section 8 row a12 -- and _rbf_round4
(src/models/RbfModel.jl:352-499, row a11).  Round 4's per-candidate kernel vectors `kernels(xi)` (:421) and the second
Gram assembly `RBF.get_matrices` (:374) are taken from the device in two batched calls (mrbf_gram for the start set,
mrbf_cross_gram for every candidate against every start site and every other candidate); the Givens / Cholesky
bookkeeping of Wild's test is sequential O(N^2) host work exactly as in the reference, including its acceptance rule
tau^2 > (theta_pivot_cholesky^2)^2 and its empty initial Z (RbfModel.jl:370, :391, :452).
"""
import ctypes
import math

import numpy as np

from . import _lib
from . import rbf_model as rm


def _orthogonal_complement_matrix(Y, p=np.inf):
    Q, _ = np.linalg.qr(Y, mode="complete")
    Z = Q[:, Y.shape[1]:]
    if Z.shape[1] > 0:
        Z = Z / np.linalg.norm(Z, ord=p, axis=0)[None, :]
    return Z


class _GrowingQR:
    """Householder QR of Y = [y_1 .. y_j] kept up to date as columns are appended, with the FULL orthogonal factor Q (d x d)
    explicit: appending y_{j+1} is one reflector H on the trailing rows, Q <- Q diag(I_j, H), i.e. a rank-1 update of Q's trailing
    columns -- O(d^2) per pick.  The reference re-factors Y from scratch after every pick (`_orthogonal_complement_matrix`,
    AffinelyIndependentPoints.jl:4-11: qr(Y), O(d^3) per pick, O(d^4) per filter -- 140-280 ms per model update at d = 128 in the
    iteration rehearsal, more than round 4, the fit and the Pascoletti-Serafini step together).  Same reflectors as LAPACK's dgeqrf
    (dlarfg: beta = -sign(alpha) ||x||, v_1 = 1), so Q agrees with qr(Y)'s to rounding and the picks are the reference's."""

    def __init__(self, d, Y=None):
        self.d = d
        if Y is None or Y.shape[1] == 0:
            self.Q, self.j = np.eye(d), 0
        else:
            self.Q, _ = np.linalg.qr(Y, mode="complete")
            self.j = Y.shape[1]

    def append(self, y):
        j, Q = self.j, self.Q
        if j >= self.d:
            return
        x = Q[:, j:].T @ y                      # the new column in the current basis, trailing part
        alpha, xn = x[0], np.linalg.norm(x[1:])
        if xn != 0.0:                           # dlarfg
            beta = -math.copysign(math.hypot(alpha, xn), alpha)
            tau = (beta - alpha) / beta
            v = x / (alpha - beta)
            v[0] = 1.0
            Qt = Q[:, j:]
            Qt -= np.outer(Qt @ v, tau * v)     # Q[:, j:] H
        self.j = j + 1

    def complement(self, p=np.inf):
        Z = self.Q[:, self.j:].copy()
        if Z.shape[1] > 0:
            Z /= np.linalg.norm(Z, ord=p, axis=0)[None, :]
        return Z


class AffinelyIndependentPointFilter:
    """Greedy filter: repeatedly the candidate maximising ||Z Z'(xi - x0)||_p, accepted while it exceeds pivot_val."""

    def __init__(self, x_0, seeds, n=None, Y=None, Z=None, p=np.inf, pivot_val=1e-3, ctx=None):
        self.x_0 = np.asarray(x_0, dtype=np.float64)
        self.shifted = [np.asarray(s, dtype=np.float64) - self.x_0 for s in seeds]
        d = self.x_0.size
        self.n = d if n is None else n
        assert self.n > 0, "`x_0` must not be empty and `n` must be positive."
        self.Y = np.empty((d, 0)) if Y is None else np.array(Y, dtype=np.float64)
        self.Z = np.eye(d) if Z is None else np.array(Z, dtype=np.float64)
        self.p, self.pivot_val = p, pivot_val
        # databases with many sites in the box: the candidate scan (two tall products + a reduction per pick) runs on the device
        # (mrbf_affine_scores) when the decision table says so (mrbf_dispatch_affine, as in HipRbf.jl's iterate method); a given
        # `ctx` forces the device scan (tests)
        self.ctx = ctx

    def _scores_device(self, S):
        ctx = self.ctx or _lib.default_context()
        Z = np.asfortranarray(self.Z)
        best, val = ctypes.c_int64(-1), ctypes.c_double()
        ctx.check(ctx.lib.mrbf_affine_scores(ctx.h, S.shape[0], S.shape[1], Z.shape[1], _lib.as_ptr(S), _lib.as_ptr(Z) if Z.shape[1] else None,
                                             1 if np.isinf(self.p) else 0, None, ctypes.byref(best), ctypes.byref(val)))
        return int(best.value), float(val.value)

    def _select_device(self, Sd, qr, want):
        """up to `want` further picks from the rows of Sd (picked rows zeroed) after the directions in `qr`: (positions, final Z)"""
        ctx = self.ctx or _lib.default_context()
        d = self.x_0.size
        picks = np.empty(max(want, 1), dtype=np.int64)
        npick = ctypes.c_int32(0)
        Zbuf = np.empty((max(d - qr.j, 1), d))                          # (column-major d x dz)
        Q0 = np.asfortranarray(qr.Q)
        ctx.check(ctx.lib.mrbf_affine_select(ctx.h, Sd.shape[0], d, _lib.as_ptr(Sd), qr.j, _lib.as_ptr(Q0), want, float(self.pivot_val),
                                             1 if np.isinf(self.p) else 0, picks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                             ctypes.byref(npick), _lib.as_ptr(Zbuf)))
        got = [int(v) for v in picks[: npick.value]]
        return got, Zbuf[: d - qr.j - len(got)].T.copy()

    def _take(self, qr, i):
        self.Y = np.hstack([self.Y, self.shifted[i][:, None]])
        qr.append(self.shifted[i])
        self.Z = qr.complement(self.p)

    def _begin(self):
        """the first pick (the largest shifted seed) and the factorisation it starts, on the host: (out, qr, S, i, cand)"""
        i = int(np.argmax([np.linalg.norm(s, ord=self.p) for s in self.shifted]))
        cand = [c for c in range(len(self.shifted)) if c != i]
        qr = _GrowingQR(self.x_0.size, self.Y)
        self._take(qr, i)
        S = np.array(self.shifted) if self.shifted else np.empty((0, self.x_0.size))
        return [i], qr, S, i, cand

    def _device_job(self, out, qr, S, i):
        """what the device pick loop needs after `_begin`: the candidates with the chosen site zeroed and the picks still wanted"""
        Sd = np.ascontiguousarray(S, dtype=np.float64)
        Sd[i] = 0.0   # chosen sites score 0 (the reference removes them from the candidate list)
        return Sd, min(self.n - len(out), self.x_0.size - qr.j)

    def _accept_device(self, out, S, got, Z):
        if got:
            self.Y = np.hstack([self.Y, S[got].T])
            self.Z = Z
            out.extend(got)
        return out

    def collect(self):
        if not self.shifted:
            return []
        out, qr, S, i, cand = self._begin()
        on_device = self.ctx is not None or \
            _lib.load().mrbf_dispatch_affine(len(cand), self.x_0.size) == _lib.DISPATCH_DEVICE
        if on_device:
            # the whole pick loop in ONE device call (mrbf_affine_select): the factorisation grows by a reflector per pick on the
            # device, no host round trip between picks (until round 6: one mrbf_affine_scores call + a host QR update per pick)
            Sd, want = self._device_job(out, qr, S, i)
            got, Z = self._select_device(Sd, qr, want)
            return self._accept_device(out, S, got, Z)
        while len(out) < self.n and cand:
            if self.Z.shape[1]:
                P = (S[cand] @ self.Z) @ self.Z.T                     # all candidates at once: rows Z Z'(xi - x0)
                vals = np.linalg.norm(P, ord=self.p, axis=1)
            else:
                vals = np.zeros(len(cand))
            b = int(np.argmax(vals))                                   # first maximiser, like the `>` scan of the reference
            if not vals[b] > self.pivot_val:
                break
            best = cand[b]
            self._take(qr, best)
            cand.remove(best)
            out.append(best)
        return out


def _per(v, ns):
    return list(v) if isinstance(v, (list, tuple)) else [v] * ns


def _by_d(dbs):
    """the positions of the databases of a call, grouped by d (one d per batched library call)"""
    groups = {}
    for p, db in enumerate(dbs):
        groups.setdefault(db.d, []).append(p)
    return groups


def _job_rows(a, d):
    """a job's block of sites: a device view or tensor is read in place, anything else becomes a contiguous float64 (m, d) array"""
    return a if hasattr(a, "data_ptr") else _lib.host_f64(a).reshape(-1, d)


def affine_select_batch_device(items, d, p=np.inf, ctx=None, device_Z=None):
    """mrbf_affine_select_batch: `items` = one (Sd, qr, want, pivot_val) per start -- the rows of Sd are the start's candidates
    (picked rows zeroed; a NumPy array, or a DeviceView or tensor, which is read in place), `qr` the `_GrowingQR` of the directions
    chosen so far -> (rc, [(positions, final Z)] or None, ms).  `device_Z[k]` (optional): start k's Z_out is a device buffer and its
    final Z comes back as a (dz, d) device tensor whose ROWS are the columns of Z (the memory of the column-major d x dz matrix), for
    mrbf_db_round3_batch to read in place.  Raises nothing for an rc that `mrbf_dispatch_after` reads as "take the single calls"."""
    ctx = ctx or _lib.default_context()
    n = len(items)
    jobs = (_lib.AffineJob * max(n, 1))()
    keep = []
    for k, (Sd, qr, want, pivot) in enumerate(items):
        Sd = _job_rows(Sd, d)
        Q0 = np.asfortranarray(qr.Q)
        picks = np.empty(max(want, 1), dtype=np.int64)
        if device_Z is not None and device_Z[k]:
            import torch

            Zbuf = torch.empty((max(d - qr.j, 1), d), dtype=torch.float64, device="cuda")
        else:
            Zbuf = np.empty((max(d - qr.j, 1), d))                      # (column-major d x dz)
        keep.append((Sd, Q0, picks, Zbuf))
        jobs[k].mc, jobs[k].j0, jobs[k].max_picks, jobs[k].pivot_val = int(Sd.shape[0]), qr.j, want, float(pivot)
        jobs[k].shifted, jobs[k].Q0 = _lib.as_ptr(Sd), Q0.ctypes.data
        jobs[k].picked_out, jobs[k].Z_out = picks.ctypes.data, _lib.as_ptr(Zbuf)
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_affine_select_batch(ctx.h, n, d, 1 if np.isinf(p) else 0, jobs, ctypes.byref(ms))
    if rc != 0:
        if not ctx.lib.mrbf_dispatch_after(_lib.ENTRY_AFFINE_BATCH, rc):
            ctx.check(rc)
        return rc, None, 0.0
    res = []
    for k, (Sd, qr, want, pivot) in enumerate(items):
        _, _, picks, Zbuf = keep[k]
        got = [int(v) for v in picks[: jobs[k].n_picked]]
        Zk = Zbuf[: d - qr.j - len(got)]
        res.append((got, Zk if hasattr(Zk, "data_ptr") else Zk.T.copy()))
    return 0, res, float(ms.value)


def _pick_loops(begun, d, p, ctx=None, device_Z=None):
    """the device pick loops of one (d, norm) group of filters past their first pick -- `begun` = one (filter, Sd, qr, want) each -- in
    ONE call (mrbf_affine_select_batch) when mrbf_dispatch_affine_batch takes the group; a group it does not take, and a batch the
    library refuses (rc -2, mrbf_dispatch_after), run the single call per filter on the same Sd, from the same state
    -> ([(positions, final Z)], whether the batched call served them)"""
    rc = -2
    if _lib.load().mrbf_dispatch_affine_batch(len(begun), d, 1 if np.isinf(p) else 0) == _lib.DISPATCH_DEVICE:
        kw = {} if device_Z is None else {"device_Z": device_Z}
        rc, res, _ = affine_select_batch_device([(Sd, qr, want, f.pivot_val) for f, Sd, qr, want in begun], d, p, ctx=ctx, **kw)
    if rc != 0:
        res = [f._select_device(Sd, qr, want) for f, Sd, qr, want in begun]
    return res, rc == 0


def affine_collect_many(filters, stats=None, ctx=None):
    """`collect()` for a list of AffinelyIndependentPointFilters -- the filters of the starts of a many-start run -- with the device
    pick loops of all of them in ONE call (mrbf_affine_select_batch): the first pick and the start of the factorisation stay on the
    host exactly as in `collect()`; the filters the decision table sends to the device (mrbf_dispatch_affine, per filter) form the
    batch when mrbf_dispatch_affine_batch takes it (one d and one norm per call: filters are grouped by them), every other filter
    runs `collect()`; a batch the library refuses (rc -2, mrbf_dispatch_after) continues with the single call per filter.  Sets every
    filter's Y and Z as `collect()` would and returns the lists of picks; stats["path"] = "batch" when a batched call ran, else
    "loop", stats["batched"] = the positions of the filters it served."""
    filters = list(filters)
    out = [None] * len(filters)
    lib = _lib.load() if filters else None
    groups = {}
    for k, f in enumerate(filters):
        if not f.shifted:
            out[k] = []
        elif f.ctx is not None or lib.mrbf_dispatch_affine(len(f.shifted) - 1, f.x_0.size) == _lib.DISPATCH_DEVICE:
            groups.setdefault((f.x_0.size, bool(np.isinf(f.p)), id(f.ctx or ctx)), []).append(k)
        else:
            out[k] = f.collect()
    batched = []
    for (d, _, _), members in groups.items():
        begun = []
        for k in members:
            f = filters[k]
            out[k], qr, S, i, _ = f._begin()
            Sd, want = f._device_job(out[k], qr, S, i)
            begun.append((f, Sd, qr, want, S))
        f0 = filters[members[0]]
        res, served = _pick_loops([b[:4] for b in begun], d, f0.p, ctx=f0.ctx or ctx)
        for k, (f, _, _, _, S), (got, Z) in zip(members, begun, res):
            f._accept_device(out[k], S, got, Z)
        if served:
            batched.extend(members)
    if stats is not None:
        stats["path"] = "batch" if batched else "loop"
        stats["batched"] = sorted(batched)
    return out


def results_in_box_indices(sites, lb, ub, exclude_indices=()):
    """indices of database sites inside the box (Databases.jl:324-327); `sites` is an (N, d) array or list"""
    ex = set(exclude_indices)
    lb, ub = np.asarray(lb), np.asarray(ub)
    return [i for i, s in enumerate(sites) if i not in ex and np.all(lb <= s) and np.all(s <= ub)]


def _find_suitable_points(sites, lb, ub, x, x_index, piv_val, already_inspected_indices=(), Y=None, Z=None, n_missing=None,
                          collect_improving_directions=True):
    """RbfModel.jl:205-238 -> (filtered_indices, improving_directions, candidate_indices, Y, Z)"""
    x = np.asarray(x, dtype=np.float64)
    cand = results_in_box_indices(sites, lb, ub, [x_index, *already_inspected_indices])
    flt = AffinelyIndependentPointFilter(x, [sites[i] for i in cand], n=x.size if n_missing is None else n_missing, Y=Y, Z=Z,
                                         p=np.inf, pivot_val=piv_val)
    picked = [cand[i] for i in flt.collect()]
    dirs = [flt.Z[:, j].copy() for j in range(flt.Z.shape[1])][::-1] if collect_improving_directions else None
    return picked, dirs, cand, flt.Y, flt.Z


def find_suitable_points_many(dbs, lbs, ubs, xs, x_indices, piv_val, already_inspected_indices=None, Ys=None, Zs=None, n_missing=None,
                              collect_improving_directions=True, stats=None, ctx=None, keep_Z_on_device=None):
    """`_find_suitable_points` (RbfModel.jl:205-238) for a list of starts -- start p has its own database `dbs[p]` (resident, host, or a
    plain array of sites: `database.as_databases`), box, centre and, for a second round, its own Y / Z and `n_missing[p]` (entries may
    be None).  Returns the list of `_find_suitable_points`' tuples.  The box scan, the shifted rows and the first pick of every start
    come from `database.box_many` (resident: ONE mrbf_db_box_batch per d, first pick's row zeroed: the state the pick loop expects);
    the first reflector starts on the host from the returned row; the pick loops of the starts the decision table sends to the device
    (mrbf_dispatch_affine per start, mrbf_dispatch_affine_batch per group) read the shifted rows in place, in ONE
    mrbf_affine_select_batch per d; a start the table keeps on the host runs the host filter on the host copy.
    `keep_Z_on_device[p]` (optional, resident databases): the caller will not run a second round from start p's Y and Z (its round 2 is
    skipped), so where the batched pick loop served the start and picked something its final Z stays on the device: the tuple's
    directions AND its Z are then one (dz, d) device tensor whose rows are the columns of Z -- the improving directions are its rows
    from the last to the first (`rbf_round3_append(..., reversed_order=True)` reads them in place)."""
    from . import database

    ns = len(dbs)
    opt = lambda seq, p: None if seq is None else seq[p]
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    dbs, _ = database.as_databases(dbs, xs)
    lib = _lib.load() if ns else None
    res, batched = [None] * ns, []
    for d, members in _by_d(dbs).items():
        sub = lambda seq: [seq[p] for p in members]
        excl = [[x_indices[p], *(opt(already_inspected_indices, p) or ())] for p in members]
        boxes = database.box_many(sub(dbs), sub(lbs), sub(ubs), sub(xs), excl, p=np.inf, zero_first_pick=True, ctx=ctx)
        begun, served = [], []
        for p, B in zip(members, boxes):
            nm = opt(n_missing, p)
            flt = AffinelyIndependentPointFilter(xs[p], [], n=d if nm is None else nm, Y=opt(Ys, p), Z=opt(Zs, p), p=np.inf, pivot_val=piv_val)
            res[p] = ([], flt, B.indices)
            if B.mc == 0:
                continue
            if lib.mrbf_dispatch_affine(B.mc - 1, d) != _lib.DISPATCH_DEVICE:
                flt.shifted = list(dbs[p].sites[B.indices] - xs[p])
                res[p] = ([B.indices[i] for i in flt.collect()], flt, B.indices)
                continue
            qr = _GrowingQR(d, flt.Y)         # `_begin` with the scan's first pick: Y gains its row, the factorisation its first reflector
            flt.Y = np.hstack([flt.Y, B.first_row[:, None]])
            qr.append(B.first_row)
            flt.Z = qr.complement(flt.p)
            flt.ctx = ctx
            begun.append((flt, B.shifted, qr, min(flt.n - 1, d - qr.j)))
            served.append((p, B))
        if not begun:
            continue
        in_place = keep_Z_on_device is not None and hasattr(begun[0][1], "data_ptr")
        got_all, ok = _pick_loops(begun, d, np.inf, ctx=ctx, device_Z=[bool(keep_Z_on_device[p]) for p, _ in served] if in_place else None)
        for (p, B), (flt, *_), (got, Z) in zip(served, begun, got_all):
            picked = [B.indices[i] for i in [B.first_pick, *got]]
            if got:
                flt.Y, flt.Z = np.hstack([flt.Y, (dbs[p].sites[picked[1:]] - xs[p]).T]), Z
            res[p] = (picked, flt, B.indices)
        if ok:
            batched.extend(p for p, _ in served)
    if stats is not None:
        stats["path"] = "batch" if batched else "loop"
        stats["batched"] = sorted(batched)
    final = []
    for picked, flt, cand in res:
        dirs = None
        if collect_improving_directions:     # (a Z left on the device: its rows are the directions, last to first)
            dirs = flt.Z if hasattr(flt.Z, "data_ptr") else [flt.Z[:, j].copy() for j in range(flt.Z.shape[1])][::-1]
        final.append((picked, dirs, cand, flt.Y, flt.Z))
    return final


def _nullify_last_row(R):
    """Givens rotations that zero the appended last row of an upper-triangular R (utilities.jl:437-448)."""
    R = np.array(R, dtype=np.float64)
    m, n = R.shape
    G = np.eye(m)
    for j in range(min(m - 1, n)):
        a, b = R[j, j], R[m - 1, j]
        r = math.hypot(a, b)
        if r == 0.0:
            continue
        c, s = a / r, b / r
        rj, rm_ = R[j].copy(), R[m - 1].copy()
        R[j], R[m - 1] = c * rj + s * rm_, -s * rj + c * rm_
        gj, gm = G[j].copy(), G[m - 1].copy()
        G[j], G[m - 1] = c * gj + s * gm, -s * gj + c * gm
    return R, G


def cross_gram(cfg, X, C, delta=1.0, ctx=None):
    """phi(||x_i - c_j||) for all pairs on the device (mrbf_cross_gram)."""
    ctx = ctx or _lib.default_context()
    X, C = _lib.host_f64(X), _lib.host_f64(C)
    m, d = X.shape
    n = C.shape[0]
    kid, a, b = rm._get_kernel_params(delta, cfg)
    K = np.empty((m, n))
    ctx.check(ctx.lib.mrbf_cross_gram(ctx.h, m, n, d, _lib.as_ptr(X), _lib.as_ptr(C), kid, a, b, _lib.as_ptr(K)))
    return K


def _rand_box_point(lb, ub, rng):
    """utilities.jl:303: uniform point of the box"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    return lb + (ub - lb) * rng.random(lb.size)


class Round4State:
    """the factors mrbf_round4 left on the device (start sites, candidates, accepted positions, kappa-factor): hand it to
    `fit_from_round4` to get the model on (start sites + accepted sites) without a new factorisation"""

    def __init__(self, ctx, handle, cfg, delta, start_sites, cand_sites, accepted):
        self.ctx, self.handle, self.cfg, self.delta = ctx, handle, cfg, delta
        self.start_sites, self.cand_sites, self.accepted = start_sites, cand_sites, list(accepted)

    @property
    def training_sites(self):
        return np.vstack([self.start_sites, self.cand_sites[self.accepted]]) if self.accepted else self.start_sites.copy()

    def free(self):
        if self.handle is not None and self.ctx.h:
            self.ctx.lib.mrbf_free_round4(self.ctx.h, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def rbf_round4_device(cfg, start_sites, cand_sites, delta=1.0, ctx=None, keep_state=False, rc_only=False):
    """_rbf_round4's selection (RbfModel.jl:352-499) as ONE device call: positions (into cand_sites) of the accepted sites in
    acceptance order [, Round4State].  Raises MrbfError(-2 / ESINGULAR) when the start set does not carry the polynomial tail;
    with `rc_only` returns (rc, accepted, state) and raises nothing (what the routed `_rbf_round4` uses)."""
    ctx = ctx or _lib.default_context()
    C0, Xc = _lib.host_f64(start_sites), _lib.host_f64(cand_sites)
    n0, d = C0.shape
    mc = Xc.shape[0]
    kid, a, b = rm._get_kernel_params(delta, cfg)
    acc = np.zeros(max(mc, 1), dtype=np.int32)
    nacc = ctypes.c_int32()
    h = _lib.c_vp()
    rc = ctx.lib.mrbf_round4(ctx.h, n0, d, _lib.as_ptr(C0), mc, _lib.as_ptr(Xc) if mc else None, kid, a, b, cfg.polynomial_degree,
                             int(cfg.max_model_points), float(cfg.θ_pivot_cholesky), _lib.as_ptr(acc), ctypes.byref(nacc),
                             ctypes.byref(h) if keep_state else None)
    if rc != 0:
        if rc_only:
            return rc, [], None
        ctx.check(rc)
    accepted = [int(v) for v in acc[: nacc.value]]
    state = Round4State(ctx, h if h.value else None, cfg, delta, C0, Xc.reshape(mc, d), accepted) if keep_state else None
    if rc_only:
        return rc, accepted, state
    return (accepted, state) if keep_state else accepted


# Where the batched call pays: measured (tools/round4_batch_bench.py, DESIGN.md section 14, next to the decision-table row), not chosen
# in advance.  One workgroup walks one start, so a batch call takes about 0.022 ms per candidate of its largest start whatever the
# number of starts, against 0.9 - 1.2 ms per start for the loop of single calls: the batch and the loop tie at 8 starts of 300
# candidates, and the batch wins from about 10 starts on there and from about 44 on at 1400 candidates.  HipRbf.jl carries the same two numbers.
ROUND4_BATCH_MIN_STARTS = 8
ROUND4_BATCH_CANDIDATES_PER_START = 32


def round4_batch_pays(n_starts, max_candidates):
    """the measured rule: at least 8 starts, and at least one start per 32 candidates of the largest start"""
    return n_starts >= ROUND4_BATCH_MIN_STARTS and n_starts * ROUND4_BATCH_CANDIDATES_PER_START >= max_candidates


def rbf_round4_batch_device(items, d, ctx=None):
    """mrbf_round4_batch: `items` = one (cfg, start_sites, cand_sites, delta) per start -> (rc, [(rc_p, positions)] or None, ms): per
    start the return code of its own selection (0, or what mrbf_round4 returned for a start that took it inside the call) and the
    positions (into its cand_sites) of the accepted sites in acceptance order.  The sites are NumPy arrays, or DeviceViews or tensors,
    which are read in place.  No factor state is kept: the fits of a batch go through `update_models_many`.  Raises nothing for an rc
    that `mrbf_dispatch_after` reads as "take the single calls"."""
    ctx = ctx or _lib.default_context()
    n = len(items)
    jobs = (_lib.Round4Job * max(n, 1))()
    keep = []
    for k, (cfg, C0, Xc, delta) in enumerate(items):
        C0, Xc = _job_rows(C0, d), _job_rows(Xc, d)
        kid, a, b = rm._get_kernel_params(delta, cfg)
        mc = int(Xc.shape[0])
        acc = np.zeros(max(mc, 1), dtype=np.int32)
        keep.append((C0, Xc, acc))
        J = jobs[k]
        J.n0, J.mc, J.start_sites, J.cand_sites = int(C0.shape[0]), mc, _lib.as_ptr(C0), _lib.as_ptr(Xc) if mc else None
        J.kernel_id, J.poly_deg, J.a, J.b = kid, cfg.polynomial_degree, a, b
        J.max_points, J.theta_pivot_cholesky, J.accepted_out = int(cfg.max_model_points), float(cfg.θ_pivot_cholesky), acc.ctypes.data
    ms = ctypes.c_float(0.0)
    rc = ctx.lib.mrbf_round4_batch(ctx.h, n, d, jobs, ctypes.byref(ms))
    if rc != 0:
        if not ctx.lib.mrbf_dispatch_after(_lib.ENTRY_ROUND4_BATCH, rc):
            ctx.check(rc)
        return rc, None, 0.0
    return 0, [(int(jobs[k].rc), [int(v) for v in keep[k][2][: jobs[k].n_accepted]]) for k in range(n)], float(ms.value)


def rbf_round4_many(dbs, lb2s, ub2s, xs, deltas, indices_found_list, cfgs, ctx=None, stats=None, min_starts=None):
    """`_rbf_round4` (RbfModel.jl:352-499) for a list of starts -- start p has its own database `dbs[p]` (resident, host, or a plain
    array of sites: `database.as_databases`), box, centre, radius, indices found so far and (one per start, or one for all) config --
    with the selections of all starts the decision table sends to the device (mrbf_dispatch_round4, per start) in ONE call
    (mrbf_round4_batch) when mrbf_dispatch_round4_batch takes the group (one d per call) and the batch pays (`round4_batch_pays`,
    measured; `min_starts` replaces the rule by a plain count: tests).  The candidates of every start come from `database.box_many`
    (the box of round 4 without the sites found so far; resident: ONE mrbf_db_box_batch per d), the start sites of the starts that form
    a batch from `database.gather_many` (ONE mrbf_db_gather_batch); mrbf_round4_batch reads both in place (a box view and a gather view
    are alive at once).  Every other start runs `_rbf_round4` on the database's host copy: start sets that cannot carry
    the tail, starts with `use_max_points` (their random box points need the caller's generator and site list, as for the single
    call), a batch the library refuses (rc -2: every start of it), and a start whose own rc `mrbf_dispatch_after` reads as "take the
    reference method".  Returns, per start, what `_rbf_round4` returns: database indices in acceptance order.  stats["path"] =
    "batch" when a batched call ran, else "loop"; stats["batched"] = the starts it served; stats["fallback"] = starts of a batch
    that went back to `_rbf_round4`."""
    from . import database

    ns = len(dbs)
    cfgs, deltas = _per(cfgs, ns), _per(deltas, ns)
    dbs, _ = database.as_databases(dbs, xs)
    out = [None] * ns
    lib = _lib.load() if ns else None
    single = lambda p: _rbf_round4(dbs[p].sites, lb2s[p], ub2s[p], xs[p], deltas[p], indices_found_list[p], cfgs[p], ctx=ctx)
    batched, fallback = [], []
    for d, all_members in _by_d(dbs).items():
        sub = lambda seq: [seq[p] for p in all_members]
        boxes = database.box_many(sub(dbs), sub(lb2s), sub(ub2s), sub(xs), [list(indices_found_list[p]) for p in all_members], p=np.inf,
                                  zero_first_pick=False, ctx=ctx)
        members, prepared = [], {}
        for p, B in zip(all_members, boxes):
            cfg, found = cfgs[p], list(indices_found_list[p])
            max_points = (d + 1) * (d + 2) // 2 if cfg.max_model_points <= 0 else cfg.max_model_points
            if cfg.use_max_points:
                out[p] = single(p)
            elif not (len(found) < max_points and B.mc):
                out[p] = []
            elif lib.mrbf_dispatch_round4(len(found), d, cfg.polynomial_degree, B.mc) != _lib.DISPATCH_DEVICE:
                out[p] = single(p)
            else:
                prepared[p] = (found, B)
                members.append(p)
        if not members:
            continue
        pays = len(members) >= min_starts if min_starts is not None else round4_batch_pays(len(members), max(prepared[p][1].mc for p in members))
        if not pays or lib.mrbf_dispatch_round4_batch(len(members), d) != _lib.DISPATCH_DEVICE:
            for p in members:
                out[p] = single(p)
            continue
        starts = database.gather_many([dbs[p] for p in members], [prepared[p][0] for p in members], ctx=ctx)
        for p, g in zip(members, starts):
            if g.rc != 0:
                raise _lib.MrbfError(g.rc, "rbf_round4_many: start %d has a found index outside its database" % p)
        rc, res, _ = rbf_round4_batch_device([(cfgs[p], g.sites, prepared[p][1].sites, deltas[p]) for p, g in zip(members, starts)], d, ctx=ctx)
        for pos, p in enumerate(members):
            if rc != 0:                                   # refused: the single call per start
                out[p] = single(p)
                continue
            rc_p, accepted = res[pos]
            if rc_p == 0:
                out[p] = [prepared[p][1].indices[a] for a in accepted]
                batched.append(p)
            elif lib.mrbf_dispatch_after(_lib.ENTRY_ROUND4_BATCH, rc_p):
                out[p] = single(p)
                fallback.append(p)
            else:
                (ctx or _lib.default_context()).check(rc_p)
    if stats is not None:
        stats["path"] = "batch" if batched else "loop"
        stats["batched"] = sorted(batched)
        stats["fallback"] = sorted(fallback)
    return out


def fit_from_round4(state, training_values, fully_linear=False, rc_only=False):
    """update_model (RbfModel.jl:743-767) for the training set (start sites + sites accepted by round 4) from the factor round 4
    left on the device -- the reference's TODO at RbfModel.jl:657-660.  `training_values`: (n0 + n_accepted) x k in that order.
    With `rc_only` returns (rc, model or None) and raises nothing."""
    ctx = state.ctx
    S = state.training_sites
    n, d = S.shape
    Y = _lib.host_f64(training_values).reshape(n, -1)
    k = Y.shape[1]
    q = 0 if state.cfg.polynomial_degree < 0 else (1 if state.cfg.polynomial_degree == 0 else d + 1)
    W, L = np.empty((n, k)), np.empty((max(q, 1), k))
    h, info = _lib.c_vp(), _lib.FitInfo()
    if state.handle is None:  # nothing was selected / no state kept: the ordinary fit
        mod = rm.update_model(state.cfg, S, Y, state.delta, fully_linear, ctx=ctx)
        return (0, mod) if rc_only else mod
    rc = ctx.lib.mrbf_fit_from_round4(ctx.h, state.handle, k, _lib.as_ptr(Y), ctypes.byref(h), _lib.as_ptr(W), _lib.as_ptr(L), ctypes.byref(info))
    if rc != 0:
        if rc_only:
            return rc, None
        ctx.check(rc)
    mod = rm.RbfModel(ctx, h, n, d, k, q, fully_linear, W, L[:q], info.asdict())
    return (0, mod) if rc_only else mod


class Round4Keeper:
    """HipRbf.jl's `_ROUND4_KEPT`: the factor round 4 left behind, per (sub-)database, together with the training indices it
    describes (start indices, then accepted indices, in factor order); `update_model_from_selection` consumes it."""

    def __init__(self):
        self.kept = {}

    def put(self, db_key, state, training_indices):
        self.drop(db_key)
        self.kept[db_key] = (state, list(training_indices))

    def pop(self, db_key):
        return self.kept.pop(db_key, None)

    def drop(self, db_key):
        old = self.kept.pop(db_key, None)
        if old is not None and old[0] is not None:
            old[0].free()


def update_model_from_selection(cfg, sites, values, training_indices, delta=1.0, fully_linear=False, keeper=None, db_key=None, ctx=None,
                                stats=None):
    """`update_model(mod, meta, cfg::HipRbfConfig, ...)` of HipRbf.jl (RbfModel.jl:743-767): the model on the training set
    `_collect_indices(meta)` -- from the kept round-4 factor when the decision table (mrbf_dispatch_fit / mrbf_dispatch_after) says
    it describes exactly this training set, else Gram + factorisation + solve (`mrbf_fit`).  `sites` / `values`: the database."""
    lib = _lib.load()
    idx = list(training_indices)
    S, Y = np.asarray(sites, dtype=np.float64)[idx], np.asarray(values, dtype=np.float64)[idx]
    kept = keeper.pop(db_key) if keeper is not None else None
    if kept is not None:
        state, ids = kept
        d = S.shape[1]
        q = 0 if cfg.polynomial_degree < 0 else (1 if cfg.polynomial_degree == 0 else d + 1)
        n0, nacc = (state.start_sites.shape[0], len(state.accepted)) if state is not None and state.handle is not None else (0, 0)
        if lib.mrbf_dispatch_fit(len(idx), n0, q, nacc, int(ids == idx)) == _lib.FIT_FROM_ROUND4:
            rc, mod = fit_from_round4(state, Y, fully_linear, rc_only=True)
            if rc == 0:
                if stats is not None:
                    stats["fit"] = "from_round4"
                state.free()
                return mod
            if not lib.mrbf_dispatch_after(_lib.ENTRY_FIT_FROM_ROUND4, rc):
                state.ctx.check(rc)
        if state is not None:
            state.free()
    if stats is not None:
        stats["fit"] = "full"
    return rm.update_model(cfg, S, Y, delta, fully_linear, ctx=ctx)


def _rbf_round4(sites, lb_2, ub_2, x, delta, indices_found_so_far, cfg, ctx=None, kernel_block=None, rng=None, new_sites=None,
                keeper=None, db_key=None, stats=None):
    """Wild's second selection round (RbfModel.jl:352-499): database indices of additional training sites that keep the
    Cholesky factors of Z'Phi Z bounded.  `sites` is the database as an (N_db, d) array; candidates are the box members
    not yet chosen, in database order.  With `cfg.use_max_points` random box points are tried once the database candidates
    are used up (RbfModel.jl:405-416, at most 10 max_points + 1 of them); an accepted one is appended to the list `new_sites`
    (the caller's `new_result!`, :455-457) and gets the index len(sites) + its position there."""
    sites = np.asarray(sites, dtype=np.float64)
    d = sites.shape[1]
    max_points = (d + 1) * (d + 2) // 2 if cfg.max_model_points <= 0 else cfg.max_model_points
    N = len(indices_found_so_far)
    cand = results_in_box_indices(sites, lb_2, ub_2, indices_found_so_far)
    round4 = []
    if not (N < max_points and (cand or cfg.use_max_points)):
        return round4
    if cfg.use_max_points:
        # the random points the loop may need, drawn up front so that their kernel values ride in the same batched device call
        # (the reference draws them one by one from the global RNG; the sequence of box points is the same)
        rng = np.random.default_rng() if rng is None else rng
        max_tries = 10 * max_points
        fresh = np.array([_rand_box_point(lb_2, ub_2, rng) for _ in range(max_tries + 1)])
        new_sites = [] if new_sites is None else new_sites
    else:
        fresh = np.empty((0, d))
    chol_pivot = cfg.θ_pivot_cholesky ** 2
    deg = cfg.polynomial_degree
    C0 = sites[list(indices_found_so_far)]
    Xc = np.vstack([sites[cand], fresh]) if len(cand) else fresh
    ids = list(cand) + [-1] * fresh.shape[0]
    if keeper is not None:
        keeper.drop(db_key)          # whatever was kept belongs to an older training set
    if kernel_block is None and _lib.load().mrbf_dispatch_round4(N, d, deg, Xc.shape[0]) == _lib.DISPATCH_DEVICE:
        # the whole selection as one device call (round4.hip), routed like `_rbf_round4(..., cfg::HipRbfConfig)` in HipRbf.jl; the
        # incremental host bookkeeping below is Morbit's own method: start sets that cannot carry the polynomial tail (n0 < q, decided
        # up front) or turn out rank deficient (the device call says so: mrbf_dispatch_after)
        rc, accepted, state = rbf_round4_device(cfg, C0, Xc, delta, ctx=ctx, keep_state=keeper is not None, rc_only=True)
        if rc == 0:
            for pos in accepted:
                id_ = ids[pos]
                if id_ < 0:
                    new_sites.append(Xc[pos].copy())
                    id_ = sites.shape[0] + len(new_sites) - 1
                round4.append(id_)
            if keeper is not None and state is not None:
                keeper.put(db_key, state, list(indices_found_so_far) + round4)
            if stats is not None:
                stats["round4"] = "device"
            return round4
        if not _lib.load().mrbf_dispatch_after(_lib.ENTRY_ROUND4, rc):
            (ctx or _lib.default_context()).check(rc)
    if stats is not None:
        stats["round4"] = "reference"
    if kernel_block is None:
        # two device calls replace one kernels(xi) call per candidate plus RBF.get_matrices
        Phi, Pi, _ = rm.get_matrices(cfg, C0, delta, ctx=ctx)
        Phi = np.array(Phi)
        K_all = cross_gram(cfg, Xc, np.vstack([C0, Xc]), delta, ctx=ctx)      # candidates x (start set + candidates)
    else:
        Phi = kernel_block(C0, C0)
        Pi = np.hstack([np.ones((N, 1)), C0])[:, : (0 if deg < 0 else (1 if deg == 0 else d + 1))]
        K_all = kernel_block(Xc, np.vstack([C0, Xc]))
    q = Pi.shape[1]
    Q, Rr = (np.linalg.qr(Pi, mode="complete") if q > 0 else (np.eye(N), np.zeros((N, 0))))
    R = np.vstack([Rr[: min(N, q)], np.zeros((N - min(N, q), q))]) if q > 0 else np.zeros((N, 0))
    Z = Q[:, N:]                     # empty, as in the reference (RbfModel.jl:391)
    L = np.zeros((0, 0))
    Linv = np.zeros((0, 0))
    phi0 = float(Phi[0, 0])
    cols = list(range(N))            # columns of K_all that are current centres
    n0 = N
    for pos, id_ in enumerate(ids):
        if N >= max_points:
            break
        xi = Xc[pos]
        phixi = K_all[pos, cols]
        pixi = np.concatenate([[1.0], xi])[:q]
        Rxi, G = _nullify_last_row(np.vstack([R, pixi[None, :]]))
        if deg >= 0 and N < math.comb(d + deg, d):
            if np.linalg.norm(Rxi[-1, :]) <= np.finfo(float).eps * 10:
                continue             # the rank of R is not augmented by adding xi
        gt, gh = G[-1, :-1], G[-1, -1]      # last column of G' without / with its last entry
        Qg = Q @ gt
        v = Z.T @ (Phi @ Qg + phixi * gh)
        sigma = Qg @ Phi @ Qg + 2.0 * gh * (phixi @ Qg) + gh * gh * phi0
        tau2 = sigma - (np.linalg.norm(Linv @ v) ** 2 if v.size else 0.0)
        if tau2 > chol_pivot ** 2:
            if id_ < 0:  # a fresh random site: stored by the caller (new_result!, RbfModel.jl:455-457)
                new_sites.append(xi.copy())
                id_ = sites.shape[0] + len(new_sites) - 1
            round4.append(id_)
            tau = math.sqrt(tau2)
            Qn = np.zeros((N + 1, N + 1))
            Qn[:N, :N] = Q
            Qn[N, N] = 1.0
            Q = Qn @ G.T
            Z = np.block([[Z, Qg[:, None]], [np.zeros((1, Z.shape[1])), np.array([[gh]])]])
            row = (v @ Linv.T) if v.size else np.zeros(0)
            L = np.block([[L, np.zeros((L.shape[0], 1))], [row[None, :], np.array([[tau]])]])
            Linv = np.block([[Linv, np.zeros((Linv.shape[0], 1))], [-(row @ Linv)[None, :] / tau, np.array([[1.0 / tau]])]])
            R = Rxi
            Phi = np.block([[Phi, phixi[:, None]], [phixi[None, :], np.array([[phi0]])]])
            cols.append(n0 + pos)
            N += 1
    return round4


# ---- round 3 (RbfModel.jl:269-307), the improvement step (:699-732) and phase I as one driver (:518-655) -------------------------------

def _rbf_round3(sites, lb_1, ub_1, x, piv_val_1, improving_directions, max_new, n_missing, ensure_fully_linear, force_rebuild):
    """RbfModel.jl:269-307 on `descent.intersect_box` -> (new_points, fully_linear, remaining_directions), or (None, None, None) when a
    direction fails the pivot test and the caller has to rebuild along the coordinate axes (:286-289).  new_points: n_new x d, to be
    appended to the database as unevaluated rows by the caller (:299-305; `sites` itself is not consulted, as in the reference)."""
    from .descent import intersect_box

    x = np.asarray(x, dtype=np.float64)
    n_new = max(0, min(int(n_missing), int(max_new)))
    fully_linear = n_new >= n_missing
    assert len(improving_directions) >= n_new, "There must be more improving directions than points missing."
    new_points = np.empty((n_new, x.size))
    for i in range(n_new):
        direction = np.asarray(improving_directions[i], dtype=np.float64)
        length = intersect_box(x, direction, lb_1, ub_1, return_vals="absmax")
        with np.errstate(invalid="ignore"):
            offset = length * direction
        if np.max(np.abs(offset)) <= piv_val_1:          # (the maximum propagates NaN: a NaN norm does not fail)
            if ensure_fully_linear and not force_rebuild:
                return None, None, None
            fully_linear = False
        with np.errstate(invalid="ignore"):
            new_points[i] = x + offset
    return new_points, bool(fully_linear), list(improving_directions[n_new:])


def _axes(d):
    return [row for row in np.eye(d)]


class Round3Result:
    """one start of round 3: `new_points` (n_new x d), `indices` (their database positions, or None where nothing was appended for the
    caller), `fully_linear`, `remaining_directions`, `rebuilt` (the start was redone along the coordinate axes, RbfModel.jl:633-637)"""
    __slots__ = ("new_points", "indices", "fully_linear", "remaining_directions", "rebuilt")

    def __init__(self, new_points, fully_linear, remaining, rebuilt, indices=None):
        self.new_points, self.fully_linear, self.remaining_directions, self.rebuilt, self.indices = new_points, fully_linear, remaining, rebuilt, indices


def _direction_rows(dirs, d, reverse):
    """the directions of one start in the order round 3 takes them: a list of vectors, a (n_dirs, d) array (rows are directions; the
    memory of a column-major d x n_dirs Z), or None for the coordinate axes"""
    if dirs is None:
        return _axes(d)
    rows = [np.asarray(v, dtype=np.float64) for v in (np.asarray(dirs, dtype=np.float64).reshape(-1, d) if not isinstance(dirs, list) else dirs)]
    return rows[::-1] if reverse else rows


def rbf_round3_many(lb1s, ub1s, xs, piv_vals, directions, max_news, n_missings, ensure_fully_linear=False, force_rebuild=False,
                    reversed_order=None):
    """`_rbf_round3` for a list of starts, with the rebuild done in place: a start whose round 3 returns nothing is redone along the
    coordinate axes with the arguments of the recursive call at RbfModel.jl:634-637 (n_missing = d, ensure_fully_linear and force_rebuild
    set).  -> list of Round3Result (`indices` None: nothing is appended here)."""
    ns = len(xs)
    piv_vals, max_news, n_missings = _per(piv_vals, ns), _per(max_news, ns), _per(n_missings, ns)
    efl, force, rev = _per(ensure_fully_linear, ns), _per(force_rebuild, ns), _per(False if reversed_order is None else reversed_order, ns)
    out = []
    for p in range(ns):
        x = np.asarray(xs[p], dtype=np.float64)
        rows = _direction_rows(directions[p], x.size, rev[p])
        pts, fl, rem = _rbf_round3(None, lb1s[p], ub1s[p], x, piv_vals[p], rows, max_news[p], n_missings[p], efl[p], force[p])
        rebuilt = pts is None
        if rebuilt:
            pts, fl, rem = _rbf_round3(None, lb1s[p], ub1s[p], x, piv_vals[p], _axes(x.size), max_news[p], x.size, True, True)
        out.append(Round3Result(pts, fl, rem, rebuilt))
    return out


def _improve_host(lb1, ub1, x, piv, rows):
    """prepare_improve_model's geometry (RbfModel.jl:715-728) -> Round3Result with 0 or 1 new point"""
    from .descent import intersect_box

    x = np.asarray(x, dtype=np.float64)
    if not rows:
        return Round3Result(np.empty((0, x.size)), False, [], False)
    direction = np.asarray(rows[0], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        offset = intersect_box(x, direction, lb1, ub1, return_vals="absmax") * direction
        ok = bool(np.max(np.abs(offset)) > piv)
        pts = (x + offset)[None, :] if ok else np.empty((0, x.size))
    return Round3Result(pts, ok and len(rows) == 1, list(rows[1:]), False)


def rbf_round3_append(dbs, lb1s, ub1s, xs, piv_vals, directions, max_news, n_missings, ensure_fully_linear=False, force_rebuild=False,
                      reversed_order=None, improve=False, ctx=None, stats=None):
    """`rbf_round3_many` with the new points appended to the databases `dbs` (`database.as_databases`) as unevaluated rows; on
    resident databases ONE mrbf_db_round3_batch per d (rebuild included).  `directions[p]`: a list of vectors, a (n_dirs, d) NumPy array or device tensor (rows are directions: the
    memory of a column-major d x n_dirs Z, read in place), or None for the coordinate axes; `reversed_order[p]`: take the rows from the
    last to the first.  `improve`: the improvement step (prepare_improve_model) instead.  On host databases, and where the decision
    table says host, the host loop runs and its points are appended through `database.append_many`.  -> list of Round3Result with
    `indices`."""
    from . import database

    ns = len(dbs)
    dbs, resident = database.as_databases(dbs, xs)
    stats = stats if stats is not None else {}
    piv_vals, max_news, n_missings = _per(piv_vals, ns), _per(max_news, ns), _per(n_missings, ns)
    efl, force, rev = _per(ensure_fully_linear, ns), _per(force_rebuild, ns), _per(False if reversed_order is None else reversed_order, ns)
    out = [None] * ns
    lib = _lib.load() if ns else None
    stats["path"] = "device"
    for d, members in _by_d(dbs).items():
        def host(members=members, d=d):
            stats["path"] = "host"
            host_rows = lambda p: _direction_rows(directions[p] if not hasattr(directions[p], "data_ptr") else directions[p].detach().cpu().numpy(),
                                                  d, rev[p])
            if improve:
                res = [_improve_host(lb1s[p], ub1s[p], xs[p], piv_vals[p], host_rows(p)) for p in members]
            else:
                res = rbf_round3_many([lb1s[p] for p in members], [ub1s[p] for p in members], [xs[p] for p in members],
                                      [piv_vals[p] for p in members], [host_rows(p) for p in members], [max_news[p] for p in members],
                                      [n_missings[p] for p in members], [efl[p] for p in members], [force[p] for p in members])
            firsts = database.append_many([dbs[p] for p in members], [r.new_points for r in res], ctx=ctx)
            for p, r, f in zip(members, res, firsts):
                r.indices = list(range(f, f + r.new_points.shape[0]))
                out[p] = r

        if not resident or lib.mrbf_dispatch_db_batch(len(members), d) != _lib.DISPATCH_DEVICE:
            host()
            continue
        c = ctx or dbs[members[0]].ctx
        jobs = (_lib.Round3Job * len(members))()
        keep = []
        for q, p in enumerate(members):
            x, lb, ub = (_lib.host_f64(v).reshape(d) for v in (xs[p], lb1s[p], ub1s[p]))
            D = directions[p]
            if D is None:
                n_dirs, ptr = d, None
            elif hasattr(D, "data_ptr"):
                D = D.contiguous()
                n_dirs, ptr = int(D.shape[0]), D.data_ptr()
            else:
                D = _lib.host_f64(np.asarray(D, dtype=np.float64).reshape(-1, d))
                n_dirs, ptr = int(D.shape[0]), (D.ctypes.data if D.size else None)
                if ptr is None:                              # an empty list is not the axes
                    D = np.zeros((1, d))
                    ptr = D.ctypes.data
            rows_out = max(min(int(n_missings[p]), int(max_news[p])), min(d, int(max_news[p])), 1)
            buf = np.empty((rows_out, d))
            keep.append((x, lb, ub, D, buf, n_dirs))
            J = jobs[q]
            J.db, J.x, J.lb, J.ub, J.pivot_val = dbs[p].h, x.ctypes.data, lb.ctypes.data, ub.ctypes.data, float(piv_vals[p])
            J.dirs, J.n_dirs, J.reversed = ptr, n_dirs, 1 if rev[p] else 0
            clamp = lambda v: int(max(-2 ** 31, min(2 ** 31 - 1, int(v))))
            J.n_missing, J.max_new = clamp(n_missings[p]), clamp(max_news[p])
            J.ensure_fully_linear, J.force_rebuild, J.mode = int(bool(efl[p])), int(bool(force[p])), _lib.R3_IMPROVE if improve else _lib.R3_UPDATE
            J.new_sites_out = buf.ctypes.data
        ms = ctypes.c_float(0.0)
        rc = c.lib.mrbf_db_round3_batch(c.h, len(members), d, jobs, ctypes.byref(ms))
        if rc != 0:
            if c.lib.mrbf_dispatch_after(_lib.ENTRY_DB_ROUND3, rc):
                host()
                continue
            c.check(rc)
        stats["ms_total"] = stats.get("ms_total", 0.0) + float(ms.value)
        failed = None
        for q, p in enumerate(members):
            J, (x, lb, ub, D, buf, n_dirs) = jobs[q], keep[q]
            if J.rc != 0:                                    # its database is untouched; the others are served before it is reported
                failed = failed or (p, int(J.rc))
                continue
            n_new, first = int(J.n_new), int(J.first_index)
            pts = buf[:n_new].copy()
            dbs[p]._adopt_rows(pts)
            rebuilt = J.status == _lib.R3_REBUILT
            if rebuilt:
                rem = _axes(d)[int(J.n_dirs_used):]
            else:
                Dh = directions[p]
                if int(J.n_dirs_used) >= n_dirs:
                    rem = []                                 # (no read-back of a device-side block for nothing)
                else:
                    if hasattr(Dh, "data_ptr"):
                        Dh = Dh.detach().cpu().numpy()
                    rem = _direction_rows(Dh, d, rev[p])[int(J.n_dirs_used):]
            out[p] = Round3Result(pts, bool(J.fully_linear), rem, rebuilt, list(range(first, first + n_new)))
        if failed is not None and failed[1] == -3:
            raise AssertionError("There must be more improving directions than points missing (start %d)." % failed[0])
        if failed is not None:
            raise _lib.MrbfError(failed[1], "mrbf_db_round3_batch: start %d" % failed[0])
    return out


def prepare_improve_models(dbs, metas, cfgs, xs, deltas, lb, ub, ctx=None, stats=None):
    """prepare_improve_model (RbfModel.jl:699-732) for a batch of starts: every meta that is not fully linear and has improving
    directions takes one improvement step, all of them through one `rbf_round3_append` (resident databases: ONE mrbf_db_round3_batch,
    MRBF_R3_IMPROVE, per d).  The metas (dicts as `prepare_update_models` returns them) are updated in place and returned."""
    from .descent import _local_bounds

    ns = len(dbs)
    cfgs, deltas = _per(cfgs, ns), _per(deltas, ns)
    act = [p for p in range(ns) if not metas[p]["fully_linear"] and len(metas[p]["improving_directions"]) > 0]
    if not act:
        return metas
    lb1s, ub1s, pivs = [], [], []
    for p in act:
        d1 = cfgs[p].θ_enlarge_1 * deltas[p]
        l1, u1 = _local_bounds(xs[p], d1, lb, ub)
        lb1s.append(l1), ub1s.append(u1), pivs.append(d1 * cfgs[p].θ_pivot)
    res = rbf_round3_append([dbs[p] for p in act], lb1s, ub1s, [xs[p] for p in act], pivs, [list(metas[p]["improving_directions"]) for p in act],
                            1, 1, improve=True, ctx=ctx, stats=stats)
    for p, r in zip(act, res):
        metas[p]["improving_directions"] = r.remaining_directions
        metas[p]["round1_indices"] = list(metas[p]["round1_indices"]) + list(r.indices)
        if r.fully_linear:
            metas[p]["fully_linear"] = True
    return metas


def _num_unevaluated(values):
    """length(_missing_ids(db)): rows whose values are NaN"""
    V = np.asarray(values, dtype=np.float64)
    return int(np.count_nonzero(np.isnan(V).any(axis=1))) if V.size else 0


def prepare_update_models(cfgs, dbs, xs, x_indices, deltas, delta_max, lb, ub, ensure_fully_linear=False, max_evals=2 ** 63 - 1,
                          num_evals=0, force_rebuild=False, ctx=None):
    """prepare_update_model (RbfModel.jl:518-655) for a list of starts on their databases `dbs` (`database.as_databases`: resident or
    host), phase by phase through `find_suitable_points_many`, `rbf_round3_append` (rebuild included, the new sites appended as
    unevaluated rows) and `rbf_round4_many`.  Round 1 is told which starts skip round 2 whatever it finds: on resident databases
    their Z stays on the device for round 3.  -> one meta (dict) per start: center_index, round1..4_indices, fully_linear,
    improving_directions, rebuilt.  One RBF config per start (_exploit_other_rbf_metas! is not mirrored)."""
    from . import database
    from .descent import _isapprox, _local_bounds

    ns = len(dbs)
    dbs, _ = database.as_databases(dbs, xs)
    cfgs, deltas, efl, force, num_evals = _per(cfgs, ns), _per(deltas, ns), _per(ensure_fully_linear, ns), _per(force_rebuild, ns), _per(num_evals, ns)
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    metas = [dict(center_index=int(x_indices[p]), round1_indices=[], round2_indices=[], round3_indices=[], round4_indices=[],
                  fully_linear=False, improving_directions=[], rebuilt=False) for p in range(ns)]
    lb1, ub1, piv1, lb2, ub2 = [None] * ns, [None] * ns, [None] * ns, [None] * ns, [None] * ns
    for p in range(ns):
        d1 = cfgs[p].θ_enlarge_1 * deltas[p]
        lb1[p], ub1[p] = _local_bounds(xs[p], d1, lb, ub)
        piv1[p] = cfgs[p].θ_pivot * d1
        lb2[p], ub2[p] = _local_bounds(xs[p], cfgs[p].θ_enlarge_2 * delta_max, lb, ub)
    sub = lambda seq, which: [seq[p] for p in which]
    # ---- round 1 (:564-579)
    searching = [p for p in range(ns) if not (force[p] or not cfgs[p].optimized_sampling)]
    cand1, Y1, Z1, dirs = {}, {}, {}, {p: None for p in range(ns)}       # (None: the coordinate axes, :568)
    # (the filter takes one pivot value per call: starts are grouped by theirs)
    groups = {}
    for p in searching:
        groups.setdefault(float(piv1[p]), []).append(p)
    # (:588 without its first clause: known before round 1; such a start never continues from its Y and Z)
    skips2 = [bool(force[p] or not cfgs[p].optimized_sampling or efl[p] or
                   (_isapprox(deltas[p], delta_max) and cfgs[p].θ_enlarge_1 == cfgs[p].θ_enlarge_2)) for p in range(ns)]
    for piv, which in groups.items():
        res = find_suitable_points_many(sub(dbs, which), sub(lb1, which), sub(ub1, which), sub(xs, which), sub(x_indices, which), piv, ctx=ctx,
                                        keep_Z_on_device=sub(skips2, which))
        for p, (picked, drs, cand, Y, Z) in zip(which, res):
            metas[p]["round1_indices"], dirs[p], cand1[p], Y1[p], Z1[p] = list(picked), drs, cand, Y, Z
    # ---- round 2 (:586-603)
    n_missing = [xs[p].size - len(metas[p]["round1_indices"]) for p in range(ns)]
    second = {}
    for p in range(ns):
        c = cfgs[p]
        if n_missing[p] == 0 or force[p] or not c.optimized_sampling or efl[p] or \
                (_isapprox(deltas[p], delta_max) and c.θ_enlarge_1 == c.θ_enlarge_2):
            metas[p]["fully_linear"] = True
        else:
            second.setdefault(float(piv1[p]), []).append(p)
    for piv, which in second.items():
        res = find_suitable_points_many(sub(dbs, which), sub(lb2, which), sub(ub2, which), sub(xs, which), sub(x_indices, which), piv,
                                        already_inspected_indices=[cand1[p] for p in which], Ys=[Y1[p] for p in which], Zs=[Z1[p] for p in which],
                                        n_missing=[n_missing[p] for p in which], collect_improving_directions=False, ctx=ctx)
        for p, r in zip(which, res):
            metas[p]["round2_indices"] = list(r[0])
    # ---- round 3 (:609-639), the rebuild inside the call
    third = []
    for p in range(ns):
        n_missing[p] -= len(metas[p]["round2_indices"])
        on_device = hasattr(dirs[p], "data_ptr")            # (d - |round 1| rows: with any row left, round 3 below replaces the list)
        metas[p]["improving_directions"] = _axes(xs[p].size) if dirs[p] is None else ([] if on_device else list(dirs[p]))
        if n_missing[p] > 0:
            third.append(p)
    if third:
        max_new = [max(0, min(max_evals, cfgs[p].max_evals) - 1 - num_evals[p] - _num_unevaluated(dbs[p].values)) for p in third]
        res = rbf_round3_append(sub(dbs, third), sub(lb1, third), sub(ub1, third), sub(xs, third), sub(piv1, third), [dirs[p] for p in third], max_new,
                                [n_missing[p] for p in third], [efl[p] for p in third], [force[p] for p in third],
                                reversed_order=[hasattr(dirs[p], "data_ptr") for p in third], ctx=ctx)
        for p, r in zip(third, res):
            m = metas[p]
            if r.rebuilt:   # the recursive call with force_rebuild: rounds 1 and 2 are empty, round 2 is skipped (fully linear so far)
                m["round1_indices"], m["round2_indices"], m["rebuilt"] = [], [], True
                m["fully_linear"] = bool(r.fully_linear)
            else:
                m["fully_linear"] = bool(r.fully_linear) and len(m["round2_indices"]) == 0     # :631
            m["round3_indices"], m["improving_directions"] = list(r.indices), r.remaining_directions
    # ---- round 4 (:645-652)
    fourth = [p for p in range(ns) if cfgs[p].optimized_sampling]
    if fourth:
        found = [[metas[p]["center_index"], *metas[p]["round1_indices"], *metas[p]["round2_indices"], *metas[p]["round3_indices"]] for p in fourth]
        for p, r4 in zip(fourth, rbf_round4_many(sub(dbs, fourth), sub(lb2, fourth), sub(ub2, fourth), sub(xs, fourth), sub(deltas, fourth), found,
                                                 sub(cfgs, fourth), ctx=ctx)):
            metas[p]["round4_indices"] = list(r4)
    return metas
