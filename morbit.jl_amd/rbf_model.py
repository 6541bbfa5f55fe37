"""Host-side mirror of Morbit's RBF surrogate interface for the hot path.

Mirrors names, argument meaning and error behaviour of /root/reference/src/models/RbfModel.jl
(RbfConfig :66-112, RbfModel :33-46, _get_kernel_params :665-690, update_model :743-767,
eval_models / get_gradient / get_jacobian :783-800) on top of the C ABI in include/mrbf.h.
All arithmetic runs in libmrbf's HIP kernels; nothing here computes a surrogate on the CPU.
`scal` arguments are accepted and ignored exactly like the reference (models live in scaled space).
"""
import ast
import ctypes
import math
import operator
from dataclasses import dataclass, fields

import numpy as np

from . import _lib

# Morbit.RbfKernels (RbfModel.jl:48-54); index = C-ABI kernel id
RbfKernels = ["cubic", "inv_multiquadric", "multiquadric", "thin_plate_spline", "gaussian"]


@dataclass(frozen=True)
class RbfConfig:
    """Configuration type for local RBF surrogate models (RbfModel.jl:58-112). Same fields and defaults."""

    kernel: str = "cubic"
    shape_parameter: object = float("nan")  # Union{String, Float64}
    polynomial_degree: int = 1
    θ_enlarge_1: float = 2.0
    θ_enlarge_2: float = 2.0
    θ_pivot: float = None  # 1 / (2 θ_enlarge_1)
    θ_pivot_cholesky: float = 1e-7
    require_linear: bool = True
    max_model_points: int = -1
    use_max_points: bool = False
    optimized_sampling: bool = True
    max_evals: int = 2 ** 63 - 1  # typemax(Int64)

    def __post_init__(self):
        if self.θ_pivot is None:
            object.__setattr__(self, "θ_pivot", 1.0 / (2.0 * self.θ_enlarge_1))
        sp = self.shape_parameter
        is_str = isinstance(sp, str)
        if not is_str:
            sp = float(sp)
            object.__setattr__(self, "shape_parameter", sp)
        nan = (not is_str) and math.isnan(sp)
        # the @assert block, RbfModel.jl:102-111
        assert self.θ_enlarge_1 * self.θ_pivot <= 1, "θ_pivot must be <= θ_enlarge_1^(-1)."
        assert self.kernel in RbfKernels, "`kernel` not supported. See `RbfKernels` for available symbols."
        if not is_str:
            assert self.kernel != "thin_plate_spline" or nan or (sp % 1 == 0 and sp >= 1), \
                "Invalid shape_parameter for :thin_plate_spline."
            assert self.kernel != "cubic" or nan or (sp % 1 == 0 and sp % 2 == 1), "Invalid shape_parameter for :cubic."
            assert nan or sp > 0, "Shape parameter must be strictly positive."
        assert self.θ_enlarge_1 >= 1 and self.θ_enlarge_2 >= 1, "θ's must be >= 1."
        assert self.polynomial_degree in (-1, 0, 1), "polynomial_degree must be -1, 0 or 1 (RbfModel.jl:21)"

    # isequal / hash over all fields so configs are combinable (RbfModel.jl:125-130); NaN == NaN like isequal
    def _key(self):
        out = []
        for f in fields(self):
            v = getattr(self, f.name)
            out.append("NaN" if isinstance(v, float) and math.isnan(v) else v)
        return tuple(out)

    def __eq__(self, other):
        return isinstance(other, RbfConfig) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


def max_evals(cfg):
    return cfg.max_evals  # RbfModel.jl:120


def combinable(cfg):
    return True  # RbfModel.jl:121


_BINOPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.Div: operator.truediv,
           ast.Pow: operator.pow}
_FUNCS = {"sqrt": math.sqrt, "exp": math.exp, "log": math.log, "abs": abs, "min": min, "max": max}


def parse_shape_param_string(delta, expr_str):
    """Evaluate a shape-parameter string such as "1/Δ" with Δ bound (RbfModel.jl:135-143).
    The reference Meta.parse + @eval's the string; here a small arithmetic evaluator is used instead."""
    src = expr_str.replace("^", "**")
    tree = ast.parse(src, mode="eval")

    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return float(node.value)
        if isinstance(node, ast.Name) and node.id in ("Δ", "delta", "Delta"):
            return float(delta)
        if isinstance(node, ast.BinOp) and type(node.op) in _BINOPS:
            return _BINOPS[type(node.op)](ev(node.left), ev(node.right))
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = ev(node.operand)
            return -v if isinstance(node.op, ast.USub) else v
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in _FUNCS:
            return float(_FUNCS[node.func.id](*[ev(a) for a in node.args]))
        raise ValueError("unsupported expression in shape parameter string: %r" % expr_str)

    return float(ev(tree))


def _get_kernel_params(delta, cfg):
    """(kernel_id, a, b) for the C ABI; follows _get_kernel_params (RbfModel.jl:665-690) with the package
    defaults substituted where the reference returns `nothing` (NaN shape parameter, :673)."""
    sp = cfg.shape_parameter
    if isinstance(sp, str):
        sp = parse_shape_param_string(delta, sp)
    kid = RbfKernels.index(cfg.kernel)
    nan = math.isnan(sp)
    if cfg.kernel == "gaussian":
        return kid, (1.0 if nan else sp), 0.0
    if cfg.kernel in ("inv_multiquadric", "multiquadric"):
        return kid, (1.0 if nan else sp), 0.5
    if cfg.kernel == "cubic":
        return kid, (3.0 if nan else float(int(sp))), 0.0
    return kid, (2.0 if nan else float(int(sp))), 0.0  # thin_plate_spline


class RbfModel:
    """Wraps a device-resident interpolation model (RbfModel.jl:33-38): `model` is the mrbf_model handle."""

    def __init__(self, ctx, handle, n, d, k, q, fully_linear=False, weights=None, poly=None, info=None):
        self.ctx, self.model = ctx, handle
        self.n, self.d, self.k, self.q = n, d, k, q
        self.fully_linear = bool(fully_linear)
        self.weights, self.poly, self.info = weights, poly, info

    @property
    def num_outputs(self):
        return self.k

    def free(self):
        if self.model is not None and self.ctx.h:
            self.ctx.lib.mrbf_free_model(self.ctx.h, self.model)
        self.model = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # ---- batched entry points (what SURVEY.md section 8f rank 2 adds to the container API)
    def eval_sites(self, X, want_values=True, want_jac=False, out_vals=None, out_jac=None, info=None):
        """values (m x k) and/or Jacobians (m x k x d) at m scaled sites in one mrbf_eval call.
        X / outputs may be NumPy arrays (host) or torch CUDA tensors (used in place)."""
        lib, ctx = self.ctx.lib, self.ctx
        is_np = not hasattr(X, "data_ptr")
        if is_np:
            X = _lib.host_f64(X).reshape(-1, self.d)
        m = int(X.shape[0])
        vals = jac = None
        if want_values:
            vals = out_vals if out_vals is not None else (np.empty((m, self.k)) if is_np else None)
            assert vals is not None, "pass out_vals for device tensors"
        if want_jac:
            jac = out_jac if out_jac is not None else (np.empty((m, self.d, self.k)) if is_np else None)
            assert jac is not None, "pass out_jac for device tensors"
        ei = _lib.EvalInfo()
        ctx.check(lib.mrbf_eval(ctx.h, self.model, m, _lib.as_ptr(X), _lib.as_ptr(vals), _lib.as_ptr(jac), ctypes.byref(ei)))
        if info is not None:
            info.update(ei.asdict())
        if want_jac and isinstance(jac, np.ndarray) and out_jac is None:
            jac = np.transpose(jac, (0, 2, 1))  # per-point k x d column-major block -> (m, k, d) view
        return vals, jac

    def hessian_sites(self, X, rows=None, out=None, info=None, stage_bytes=None):
        """model Hessians (m x r x d x d) at m scaled sites in one mrbf_eval_hessian call: per site and selected output the second
        derivative of that output with respect to the scaled site.  rows: 0-based output indices, any order, repeats allowed
        (None: all k).  X / out may be NumPy arrays (host) or torch CUDA tensors (used in place; pass `out` for those).
        stage_bytes: the staging limit of a host-side result, for tests (mrbf_eval_hessian_limited)."""
        lib, ctx = self.ctx.lib, self.ctx
        is_np = not hasattr(X, "data_ptr")
        if is_np:
            X = _lib.host_f64(X).reshape(-1, self.d)
        m = int(X.shape[0])
        rows_a = None if rows is None else np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
        r = self.k if rows_a is None else int(rows_a.size)
        if rows_a is not None and r == 0:
            return out if out is not None else np.empty((m, 0, self.d, self.d))
        if out is None:
            assert is_np, "pass out for device tensors"
            out = np.empty((m, r, self.d, self.d))
        hi = _lib.HessInfo()
        args = (ctx.h, self.model, m, _lib.as_ptr(X), 0 if rows_a is None else r, _lib.as_ptr(rows_a), _lib.as_ptr(out), ctypes.byref(hi))
        if stage_bytes is None:
            ctx.check(lib.mrbf_eval_hessian(*args))
        else:
            ctx.check(lib.mrbf_eval_hessian_limited(*args, int(stage_bytes)))
        if info is not None:
            info.update(hi.asdict())
        return out


def fully_linear(rbf):
    return rbf.fully_linear  # RbfModel.jl:40


def num_outputs(rbf):
    return rbf.num_outputs  # RbfModel.jl:41


def set_fully_linear(rbf, val):
    rbf.fully_linear = bool(val)  # RbfModel.jl:43-46
    return None


def update_model(cfg, training_sites, training_values, delta=1.0, fully_linear=False, ctx=None):
    """The arithmetic half of update_model (RbfModel.jl:743-767): given the training sites and values that
    `_collect_indices(meta)` selected from the database, assemble + factorise + solve on the GPU.
    Returns an RbfModel (the reference returns `(RbfModel(inner_model, meta.fully_linear), meta)`)."""
    ctx = ctx or _lib.default_context()
    C = _lib.host_f64(training_sites)
    assert C.ndim == 2, "training_sites: n sites of dimension d"
    n, d = C.shape
    Y = _lib.host_f64(training_values).reshape(n, -1)
    k = Y.shape[1]
    kid, a, b = _get_kernel_params(delta, cfg)
    q = 0 if cfg.polynomial_degree < 0 else (1 if cfg.polynomial_degree == 0 else d + 1)
    W = np.empty((n, k))
    L = np.empty((max(q, 1), k))
    h = _lib.c_vp()
    info = _lib.FitInfo()
    ctx.check(ctx.lib.mrbf_fit(ctx.h, n, d, k, _lib.as_ptr(C), _lib.as_ptr(Y), kid, a, b, cfg.polynomial_degree,
                               ctypes.byref(h), _lib.as_ptr(W), _lib.as_ptr(L), ctypes.byref(info)))
    return RbfModel(ctx, h, n, d, k, q, fully_linear, W, L[:q], info.asdict())


def _as_fit_input(a, rows=None):
    """a host array (made contiguous float64) or a device tensor (used in place) as a 2-d array of `rows` rows"""
    if hasattr(a, "data_ptr"):
        a = a.contiguous()
        return a.reshape(rows, -1) if rows is not None else a
    a = _lib.host_f64(a)
    return a.reshape(rows, -1) if rows is not None else a


def _takes_small_lu(kid, a, b, deg, n, d, k):
    """Is a start on the LU path (fit_model, solve.hip: the kernel's order exceeds what the tail covers, or n == q) and inside the range
    of MRBF_OPT_SMALL_LU (n <= 512, d <= 128, k <= 16, n >= q, a smooth kernel)?  (kid, a, b) as _get_kernel_params gives them."""
    q = 0 if deg < 0 else (1 if deg == 0 else d + 1)
    order = math.ceil(a / 2.0) if kid == 0 else (math.ceil(b) if kid == 2 else (int(a) + 1 if kid == 3 else 0))
    nonsmooth = kid in (0, 3) and a == 1.0
    chol = order <= deg + 1 and n > q
    return (not chol) and q <= n <= _lib.SMALL_LU_MAX_N and d <= _lib.SMALL_LU_MAX_D and k <= _lib.SMALL_LU_MAX_K and not nonsmooth


def update_models_many(cfgs, sites_list, values_list, deltas, fully_linear=False, ctx=None, stats=None):
    """update_model for a batch of starts (the Threads.@threads loop over starts of examples/large_scale_benchmarks.jl:102-109 around
    RbfModel.jl:743-767) in ONE mrbf_fit_batch call where mrbf_dispatch_fit_batch says so; otherwise, or when the call returns -2, the
    loop over update_model.  cfgs / deltas / fully_linear: one per start, or one for all.  Sites and values may be NumPy arrays or torch
    device tensors (used in place).  Returns a list of RbfModel -- for every start bit for bit the model update_model gives -- with None
    for a start whose fit failed; stats (optional dict) receives "path" ("batch" or "loop"), "status" (return code per start),
    "ms_total" and "wide": how many starts with more than 512 sites shared the batch's launch, the context's
    MRBF_OPT_SMALL_FIT_MAX_N raised to mrbf_dispatch_fit_batch_max_n's answer for the one call and put back behind it, also on error
    (such a start is, bit for bit, what mrbf_fit gives under that option value, not under the default); "lu": how many starts on the LU
    path shared the one-launch LU (MRBF_OPT_SMALL_LU set to 1 for the one call where mrbf_dispatch_fit_batch_lu admits them, and put back
    behind it, also on error; such a start is what mrbf_fit gives under that option)."""
    ctx = ctx or _lib.default_context()
    ns = len(sites_list)
    per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * ns
    cfgs, deltas, fls = per(cfgs), per(deltas), per(fully_linear)
    stats = stats if stats is not None else {}

    def loop():
        mods, status = [], []
        for p in range(ns):
            try:
                mods.append(update_model(cfgs[p], sites_list[p], values_list[p], deltas[p], fls[p], ctx=ctx))
                status.append(0)
            except _lib.MrbfError as e:
                mods.append(None)
                status.append(e.code)
        stats.update(path="loop", status=status, ms_total=float(sum(m.info["ms_total"] for m in mods if m is not None)), wide=0, lu=0)
        return mods

    if ctx.lib.mrbf_dispatch_fit_batch(ns) != _lib.DISPATCH_DEVICE:
        return loop()
    jobs = (_lib.FitJob * ns)()
    keep, lu = [], []
    for p in range(ns):
        C = _as_fit_input(sites_list[p])
        assert C.ndim == 2, "training_sites: n sites of dimension d"
        n, d = (int(v) for v in C.shape)
        Y = _as_fit_input(values_list[p], n)
        k = int(Y.shape[1])
        kid, a, b = _get_kernel_params(deltas[p], cfgs[p])
        deg = cfgs[p].polynomial_degree
        q = 0 if deg < 0 else (1 if deg == 0 else d + 1)
        W, L = np.empty((n, k)), np.empty((max(q, 1), k))
        keep.append((C, Y, W, L, n, d, k, q))
        if _takes_small_lu(kid, a, b, deg, n, d, k):
            lu.append((n, d))
        J = jobs[p]
        J.n, J.d, J.k, J.kernel_id, J.poly_deg, J.a, J.b = n, d, k, kid, deg, a, b
        J.centres, J.values = _lib.as_ptr(C), _lib.as_ptr(Y)
        J.weights_out, J.poly_out = _lib.as_ptr(W), _lib.as_ptr(L)
    ms = ctypes.c_float()
    # starts beyond the one-launch fit's default range: the table says up to which n they share the batch's launch
    # (MRBF_OPT_SMALL_FIT_MAX_N, raised for this one call); with none, nothing is asked and nothing is set
    beyond = [(n, d) for (_, _, _, _, n, d, _, _) in keep if n > _lib.SMALL_FIT_DEFAULT_MAX_N]
    wide_n = min((int(ctx.lib.mrbf_dispatch_fit_batch_max_n(len(beyond), d)) for _, d in beyond), default=_lib.SMALL_FIT_DEFAULT_MAX_N)
    n_wide = sum(1 for n, _ in beyond if n <= wide_n)
    # starts on the LU path inside the one-launch LU's range: the table says whether they share its launch (MRBF_OPT_SMALL_LU, likewise)
    n_lu = len(lu) if lu and all(ctx.lib.mrbf_dispatch_fit_batch_lu(len(lu), max(n for n, _ in lu), d) == 1 for _, d in lu) else 0
    stats["wide"], stats["lu"] = 0, 0
    options = ([(_lib.OPT_SMALL_FIT_MAX_N, wide_n)] if n_wide else []) + ([(_lib.OPT_SMALL_LU, 1)] if n_lu else [])
    previous = [(key, ctx.get_option(key)) for key, _ in options]
    try:
        for key, value in options:
            ctx.set_option(key, value)
        rc = ctx.lib.mrbf_fit_batch(ctx.h, ns, jobs, ctypes.byref(ms))
    finally:
        for key, value in previous:
            ctx.set_option(key, value)
    if rc != 0 and ctx.lib.mrbf_dispatch_after(_lib.ENTRY_FIT_BATCH, rc) == 1:
        return loop()
    ctx.check(rc)
    mods = []
    for p, (C, Y, W, L, n, d, k, q) in enumerate(keep):
        J = jobs[p]
        mods.append(RbfModel(ctx, _lib.c_vp(J.model), n, d, k, q, fls[p], W, L[:q], J.info.asdict()) if J.status == 0 else None)
    stats.update(path="batch", status=[int(J.status) for J in jobs], ms_total=float(ms.value), wide=n_wide, lu=n_lu)
    return mods


def update_models_resident(cfgs, dbs, index_lists, deltas, fully_linear=False, ctx=None, stats=None):
    """`update_models_many` on resident databases (database.DeviceDatabase): start p's training set is the rows `index_lists[p]` of
    `dbs[p]` (get_site / get_value over _collect_indices(meta), RbfModel.jl:747-757), gathered on the device for all starts in ONE call
    (mrbf_db_gather_batch) and handed to mrbf_fit_batch as device views: no site or value crosses PCIe.  Returns exactly what
    `update_models_many(cfgs, [db.sites[idx]], [db.values[idx]], ...)` returns, by the same decision-table answers; wherever that
    driver takes the loop of single fits, or the gather itself goes to the host (mrbf_dispatch_db_batch), the rows come from the
    databases' host copies."""
    from . import database

    ns = len(dbs)
    by_d = {}
    for p in range(ns):
        by_d.setdefault(dbs[p].d, []).append(p)
    per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * ns
    cfgs, deltas, fls = per(cfgs), per(deltas), per(fully_linear)
    mods, status, ms, paths, wide, lu = [None] * ns, [0] * ns, 0.0, [], 0, 0
    for members in by_d.values():   # one gather and one fit call per d (a gather's views last until the next gather)
        got = database.gather_many([dbs[p] for p in members], [index_lists[p] for p in members], ctx=ctx)
        for p, g in zip(members, got):
            if g.rc != 0:
                raise _lib.MrbfError(g.rc, "update_models_resident: start %d has a training index outside its database" % p)
        st = {}
        res = update_models_many([cfgs[p] for p in members], [g.sites for g in got], [g.values for g in got], [deltas[p] for p in members],
                                 [fls[p] for p in members], ctx=ctx, stats=st)
        for pos, p in enumerate(members):
            mods[p], status[p] = res[pos], st["status"][pos]
        ms += st["ms_total"]
        wide += st.get("wide", 0)
        lu += st.get("lu", 0)
        paths.append(st["path"])
    if stats is not None:
        stats.update(path="batch" if "batch" in paths else "loop", status=status, ms_total=ms, wide=wide, lu=lu)
    return mods


def eval_models_many(mods, Xs, want_values=True, want_jac=False, outs=None, ctx=None, stats=None, min_jobs=None):
    """`RbfModel.eval_sites` for a batch of (model, site block) pairs -- m(x) and m(x₊) of every start (src/algorithm.jl:766-767), the
    container sweeps of every start (src/SurrogateContainer.jl:234-269) -- in ONE mrbf_eval_batch call where mrbf_dispatch_eval_batch
    takes the job count and it reaches mrbf_dispatch_eval_batch_min_jobs (min_jobs: another threshold, for tests and measurements);
    otherwise, or when the call returns -2, the loop over eval_sites.  A model may appear several times.  Xs[i]: m_i x d, a NumPy array
    or a torch device tensor (used in place; then outs[i] = (out_vals, out_jac) device tensors must be given for what is wanted).
    want_values / want_jac: one for all, or one per pair.  Returns a list of (vals, jac) -- for every pair bit for bit what
    `mods[i].eval_sites(Xs[i], ...)` returns, in its shapes.  stats (optional dict) receives "path" ("batch" or "loop"), "jobs" (how
    many pairs the one call carried), "single_inside" (how many of them took the single call's chain inside it: d > 256, or
    MRBF_OPT_EVAL_IMPL = 1), "ms_total" (the batch call's, or the sum of the loop's) and "ms_jobs" (per pair: its own call's
    time in the loop, the one call's in the batch)."""
    n = len(mods)
    stats = stats if stats is not None else {}
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
    wv, wj = per(want_values), per(want_jac)
    outs = list(outs) if outs is not None else [(None, None)] * n
    if n == 0:
        stats.update(path="loop", jobs=0, single_inside=0, ms_total=0.0, ms_jobs=[])
        return []
    ctx = ctx or mods[0].ctx

    def loop():
        infos = [{} for _ in range(n)]
        res = [mods[i].eval_sites(Xs[i], want_values=wv[i], want_jac=wj[i], out_vals=outs[i][0], out_jac=outs[i][1], info=infos[i]) for i in range(n)]
        ms_jobs = [float(info.get("ms_total", 0.0)) for info in infos]
        stats.update(path="loop", jobs=0, single_inside=0, ms_total=float(sum(ms_jobs)), ms_jobs=ms_jobs)
        return res

    lib = ctx.lib
    floor = int(lib.mrbf_dispatch_eval_batch_min_jobs()) if min_jobs is None else int(min_jobs)
    if lib.mrbf_dispatch_eval_batch(n) != _lib.DISPATCH_DEVICE or n < floor or any(m.ctx is not ctx for m in mods):
        return loop()
    jobs = (_lib.EvalJob * n)()
    keep = []
    for i, mod in enumerate(mods):
        X = Xs[i]
        is_np = not hasattr(X, "data_ptr")
        X = _lib.host_f64(X).reshape(-1, mod.d) if is_np else X.contiguous()
        m = int(X.shape[0])
        vals = jac = None
        if wv[i]:
            vals = outs[i][0] if outs[i][0] is not None else (np.empty((m, mod.k)) if is_np else None)
            assert vals is not None, "pass out_vals for device tensors"
        if wj[i]:
            jac = outs[i][1] if outs[i][1] is not None else (np.empty((m, mod.d, mod.k)) if is_np else None)
            assert jac is not None, "pass out_jac for device tensors"
        keep.append((X, vals, jac))
        J = jobs[i]
        J.model, J.m = mod.model.value if hasattr(mod.model, "value") else mod.model, m
        J.X, J.vals_out, J.jac_out = (_lib.as_ptr(a).value if a is not None and m > 0 else None for a in (X, vals, jac))
    ms = ctypes.c_float()
    rc = lib.mrbf_eval_batch(ctx.h, n, jobs, ctypes.byref(ms))
    if rc != 0 and lib.mrbf_dispatch_after(_lib.ENTRY_EVAL_BATCH, rc) == 1:
        return loop()
    ctx.check(rc)
    res = []
    for i, (X, vals, jac) in enumerate(keep):
        if jac is not None and isinstance(jac, np.ndarray) and outs[i][1] is None:
            jac = np.transpose(jac, (0, 2, 1))  # per-point k x d column-major block -> (m, k, d) view, as eval_sites
        res.append((vals, jac))
    # the pairs that took the single call's chain inside the call: outside the fused kernels' range (d > 256), or all of them under
    # MRBF_OPT_EVAL_IMPL = 1 (pairs without rows or outputs launch nothing)
    active = [i for i, (X, vals, jac) in enumerate(keep) if int(X.shape[0]) > 0 and (vals is not None or jac is not None)]
    gemm = ctx.get_option(_lib.OPT_EVAL_IMPL) == 1
    stats.update(path="batch", jobs=n, single_inside=sum(1 for i in active if gemm or mods[i].d > 256), ms_total=float(ms.value),
                 ms_jobs=[float(ms.value)] * n)
    return res


def get_hessians_many(mods, Xs, rows=None, outs=None, ctx=None, stats=None, min_jobs=None, limit_bytes=None):
    """`RbfModel.hessian_sites` for a batch of (model, site block) pairs -- the second derivative of every start's model at its own
    iterate -- in ONE mrbf_eval_hessian_batch call where mrbf_dispatch_hessian_batch takes the job count and it reaches
    mrbf_dispatch_hessian_batch_min_jobs (min_jobs: another threshold, for tests and measurements); otherwise, or when the call
    returns -2, the loop over hessian_sites.  A model may appear several times.  Xs[i]: m_i x d, a NumPy array or a torch device
    tensor (used in place; then outs[i], a device tensor, must be given).  rows: None (all outputs), one list of 0-based output
    indices for all pairs, or one entry (a list or None) per pair.  limit_bytes: the limit of the chunk rule, for tests
    (mrbf_eval_hessian_batch_limited).  Returns a list with, for every pair, bit for bit what `mods[i].hessian_sites(Xs[i], rows=...)`
    returns, in its shape.  stats (optional dict) receives "path" ("batch" or "loop"), "jobs" (how many pairs the one call carried),
    "single_inside", "chunks", "groups", "ms_total" and "nsplit" (per pair)."""
    n = len(mods)
    stats = stats if stats is not None else {}
    outs = list(outs) if outs is not None else [None] * n
    one_for_all = rows is None or len(rows) == 0 or not (rows[0] is None or hasattr(rows[0], "__len__"))
    rows_l = [rows] * n if one_for_all else list(rows)
    assert len(rows_l) == n and len(Xs) == n and len(outs) == n
    if n == 0:
        stats.update(path="loop", jobs=0, single_inside=0, chunks=0, groups=0, ms_total=0.0, nsplit=[])
        return []
    ctx = ctx or mods[0].ctx

    def loop():
        infos = [{} for _ in range(n)]
        res = [mods[i].hessian_sites(Xs[i], rows=rows_l[i], out=outs[i], info=infos[i]) for i in range(n)]
        stats.update(path="loop", jobs=0, single_inside=0, chunks=0, groups=0,
                     ms_total=float(sum(info.get("ms_total", 0.0) for info in infos)), nsplit=[int(info.get("nsplit", 0)) for info in infos])
        return res

    lib = ctx.lib
    floor = int(lib.mrbf_dispatch_hessian_batch_min_jobs()) if min_jobs is None else int(min_jobs)
    if lib.mrbf_dispatch_hessian_batch(n) != _lib.DISPATCH_DEVICE or n < floor or any(m.ctx is not ctx for m in mods):
        return loop()
    jobs = (_lib.HessJob * n)()
    keep = []
    for i, mod in enumerate(mods):
        X = Xs[i]
        is_np = not hasattr(X, "data_ptr")
        X = _lib.host_f64(X).reshape(-1, mod.d) if is_np else X.contiguous()
        m = int(X.shape[0])
        rows_a = None if rows_l[i] is None else np.ascontiguousarray(np.atleast_1d(rows_l[i]), dtype=np.int32)
        r = mod.k if rows_a is None else int(rows_a.size)
        out = outs[i]
        empty = rows_a is not None and r == 0   # an empty selection is not "all": nothing to ask the library for
        if out is None:
            assert is_np, "pass outs for device tensors"
            out = np.empty((m, r, mod.d, mod.d))
        keep.append((X, rows_a, out))
        J = jobs[i]
        J.model, J.m = mod.model.value if hasattr(mod.model, "value") else mod.model, 0 if empty else m
        live = m > 0 and not empty
        J.X, J.hess_out = (_lib.as_ptr(a).value if live else None for a in (X, out))
        J.rows, J.n_rows = (None, 0) if rows_a is None or empty else (_lib.as_ptr(rows_a).value, r)
    bi = _lib.HessBatchInfo()
    if limit_bytes is None:
        rc = lib.mrbf_eval_hessian_batch(ctx.h, n, jobs, ctypes.byref(bi))
    else:
        rc = lib.mrbf_eval_hessian_batch_limited(ctx.h, n, jobs, ctypes.byref(bi), int(limit_bytes))
    if rc != 0 and lib.mrbf_dispatch_after(_lib.ENTRY_HESSIAN_BATCH, rc) == 1:
        return loop()
    ctx.check(rc)
    stats.update(path="batch", jobs=n, single_inside=int(bi.single_inside), chunks=int(bi.chunks), groups=int(bi.groups),
                 ms_total=float(bi.ms_total), nsplit=[int(jobs[i].nsplit) for i in range(n)])
    return [out for _, _, out in keep]


init_model = update_model      # RbfModel.jl:738-741 delegates
improve_model = update_model   # RbfModel.jl:770-776 delegates


def model_from_coeffs(cfg, sites, weights, poly, delta=1.0, fully_linear=False, ctx=None):
    ctx = ctx or _lib.default_context()
    C = _lib.host_f64(sites)
    n, d = C.shape
    W = _lib.host_f64(weights).reshape(n, -1)
    k = W.shape[1]
    kid, a, b = _get_kernel_params(delta, cfg)
    q = 0 if cfg.polynomial_degree < 0 else (1 if cfg.polynomial_degree == 0 else d + 1)
    L = _lib.host_f64(poly).reshape(q, k) if q else None
    h = _lib.c_vp()
    ctx.check(ctx.lib.mrbf_model_from_coeffs(ctx.h, n, d, k, _lib.as_ptr(C), _lib.as_ptr(W), _lib.as_ptr(L), kid, a, b,
                                             cfg.polynomial_degree, ctypes.byref(h)))
    return RbfModel(ctx, h, n, d, k, q, fully_linear, W, L, None)


def eval_models(mod, scal, x_hat, ell=None):
    """Evaluate `mod` at scaled site x̂; with `ell` (int or list of ints) only those outputs
    (RbfModel.jl:783-790; RefSurrogate passes index vectors, AbstractSurrogateInterface.jl:159-164)."""
    vals, _ = mod.eval_sites(np.asarray(x_hat, dtype=np.float64)[None, :])
    v = vals[0]
    return v if ell is None else v[ell]


def get_gradient(mod, scal, x_hat, ell):
    """Gradient vector of output `ell` at x̂ (RbfModel.jl:792-795). Bit-equal to the Jacobian row (same kernel)."""
    return get_jacobian(mod, scal, x_hat)[ell]


def get_jacobian(mod, scal, x_hat, rows=None):
    """k x d Jacobian (or selected rows) at x̂ (RbfModel.jl:797-800)."""
    _, jac = mod.eval_sites(np.asarray(x_hat, dtype=np.float64)[None, :], want_values=False, want_jac=True)
    J = np.ascontiguousarray(jac[0])
    return J if rows is None else J[rows]


def get_hessian(mod, scal, x_hat, ell):
    """d x d Hessian of output `ell` at x̂ with respect to the scaled site: the derivative of get_gradient (RbfModel.jl:792-795),
    which the reference leaves to the caller."""
    return mod.hessian_sites(np.asarray(x_hat, dtype=np.float64)[None, :], rows=[int(ell)])[0, 0]


# batched twins
def get_hessians_at_sites(mod, scal, X, rows=None):
    """(m, r, d, d): the Hessians of the selected outputs (None: all) at the rows of X"""
    return mod.hessian_sites(X, rows=rows)


def eval_models_at_sites(mod, scal, X):
    return mod.eval_sites(X)[0]


def get_jacobians_at_sites(mod, scal, X):
    return np.ascontiguousarray(mod.eval_sites(X, want_values=False, want_jac=True)[1])


def get_matrices(cfg, centers, delta=1.0, ctx=None, want_pi=True):
    """Phi (n x n) and Pi (n x q): RBF.get_matrices(phi, centers; poly_deg) as used by round 4 (RbfModel.jl:374-375)."""
    ctx = ctx or _lib.default_context()
    C = _lib.host_f64(centers)
    n, d = C.shape
    kid, a, b = _get_kernel_params(delta, cfg)
    q = 0 if cfg.polynomial_degree < 0 else (1 if cfg.polynomial_degree == 0 else d + 1)
    Phi = np.empty((n, n), order="F")
    Pi = np.empty((n, max(q, 1)), order="F")
    ms = ctypes.c_float()
    ctx.check(ctx.lib.mrbf_gram(ctx.h, n, d, _lib.as_ptr(C), kid, a, b, cfg.polynomial_degree, _lib.as_ptr(Phi),
                                _lib.as_ptr(Pi) if (want_pi and q) else None, ctypes.byref(ms)))
    return Phi, Pi[:, :q], ms.value
