"""Host-side mirror of the descent-step consumers of the surrogate path.

Mirrors /root/reference/src/descent.jl: SteepestDescentConfig backtracking fields (:55-66),
_armijo_condition (:137-143) and _backtrack (:150-185); and the steepest-descent criticality: the direction LP
_steepest_descent_direction (:91-135, HiGHS on the host), get_criticality (:187-241, routed to mrbf_sd_criticality) and
compute_descent_step (:243-320) with intersect_box / _intersect_bounds (utilities.jl:126-287).  The reference evaluates the <= max_loops
step sizes one after another; here all of them go to the device in one batch (mrbf_backtrack when the
objectives are one grouped RbfModel, else one batched container sweep) and the same loop logic picks
the step, so the returned (x_plus, mx_plus, step) are those of the sequential loop.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import surrogates as sg


@dataclass
class SteepestDescentConfig:
    strict_backtracking: bool = True
    armijo_const_rhs: float = 1e-6
    armijo_const_shrink: float = 0.75
    min_stepsize: float = 10 * np.finfo(np.float64).eps
    max_loops: int = None
    normalize: bool = True

    def __post_init__(self):
        if self.max_loops is None:  # descent.jl:61-66
            base = self.min_stepsize if self.min_stepsize > 0 else np.finfo(np.float64).eps
            self.max_loops = int(math.floor(math.log(base) / math.log(self.armijo_const_shrink)))
        assert self.armijo_const_rhs > 0


def _armijo_condition(strict, Mx, Mx_plus, step_size, omega, const_rhs):
    if strict:  # Val{true}, descent.jl:137-139
        return bool(np.all((Mx - Mx_plus) >= step_size * const_rhs * omega))
    return bool(np.max(Mx) - np.max(Mx_plus) >= step_size * const_rhs * omega)  # descent.jl:141-143


def _single_model(sc):
    """the inner RbfModel when the decision table (mrbf_dispatch_backtrack, the same call HipRbf.jl makes) sends `_backtrack` to
    mrbf_backtrack: every objective a RefSurrogate row of ONE grouped device model, outputs in order; else None"""
    plan = sg.container_plan(sc, objectives_only=True)
    lib = _lib.load()
    if lib.mrbf_dispatch_backtrack(len(plan["models"]), plan["n_foreign"], int(plan["in_order"])) == _lib.DISPATCH_DEVICE:
        return plan["models"][0]
    return None


def _backtrack(x, direction, step_size, omega, sc, cfg, scal=None):
    """Returns (x_plus, mx_plus, step) like descent.jl:150-185, plus the loop count as 4th value."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    direction = np.ascontiguousarray(direction, dtype=np.float64)
    min_step = cfg.min_stepsize if cfg.min_stepsize >= 0 else np.finfo(np.float64).eps
    inner = _single_model(sc)
    if inner is not None:
        ctx = inner.ctx
        xp = np.empty_like(x)
        mxp = np.empty(inner.num_outputs)
        step = np.empty_like(x)
        nl = ctypes.c_int32()
        ctx.check(ctx.lib.mrbf_backtrack(ctx.h, inner.model, _lib.as_ptr(x), _lib.as_ptr(direction), float(step_size),
                                         float(omega), int(cfg.strict_backtracking), cfg.armijo_const_rhs,
                                         cfg.armijo_const_shrink, min_step, cfg.max_loops, _lib.as_ptr(xp),
                                         _lib.as_ptr(mxp), _lib.as_ptr(step), ctypes.byref(nl)))
        return xp, mxp, step, nl.value
    # general container: one batched sweep over all trial points, then the reference's loop logic
    steps = [float(step_size)]
    for _ in range(cfg.max_loops):
        steps.append(steps[-1] * cfg.armijo_const_shrink)
    X = np.vstack([x[None, :]] + [x[None, :] + s * direction[None, :] for s in steps])
    M = sg.eval_container_objectives_at_scaled_sites(sc, scal, X)
    mx = M[0]
    i = 0
    while i < cfg.max_loops:
        if _armijo_condition(cfg.strict_backtracking, mx, M[i + 1], steps[i], omega, cfg.armijo_const_rhs):
            break
        if steps[i] <= min_step:
            break
        i += 1
    return X[i + 1], M[i + 1], steps[i] * direction, i


# ---- steepest-descent criticality (descent.jl:91-135, :187-320) --------------------------------------------------------------------
def _sd_box(x, lb, ub):
    """the direction's box of descent.jl:112-116, exactly as the device kernel forms it: [max(-1, lb - x), min(1, ub - x)]"""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(-1.0, np.asarray(lb, dtype=np.float64) - x), np.minimum(1.0, np.asarray(ub, dtype=np.float64) - x)


def _sd_omega(G, w, d):
    """omega = -max_i (g_i . d) / w_i over the rows with w_i > 0 (recomputed from d, as mrbf_sd_direction does)"""
    r = np.asarray(G, dtype=np.float64) @ np.asarray(d, dtype=np.float64)
    ok = w > 0
    return -float(np.max(r[ok] / w[ok])) if ok.any() else -np.inf


def _steepest_descent_direction(x, G, lb, ub, A_eq=None, b_eq=None, A_ineq=None, b_ineq=None, normalize=True, tol=1e-10,
                                want_status=False):
    """descent.jl:91-135 with HiGHS (scipy.optimize.linprog) in place of JuMP + OSQP: min alpha over (d, alpha) subject to
    G d <= alpha w (w = row norms with `normalize`, else 1), the box of `_sd_box`, A_eq d = b_eq, A_ineq d <= b_ineq.  Returns
    (d, omega) with omega = -alpha recomputed from d; (zeros, -inf) where the reference's catch branch fires (descent.jl:130-133:
    no objective row under `normalize`, an empty box, rows that cannot be met).  want_status: also the MRBF_SD_* status."""
    from scipy.optimize import linprog

    x = np.asarray(x, dtype=np.float64)
    n = x.size
    G = np.asarray(G, dtype=np.float64).reshape(-1, n)
    k = G.shape[0]
    w = np.sqrt(np.sum(G * G, axis=1)) if normalize else np.ones(k)
    lo, hi = _sd_box(x, lb, ub)

    def out(d, omega, status):
        return (d, omega, status) if want_status else (d, omega)

    if not np.all(lo <= hi):
        return out(np.zeros(n), -np.inf, _lib.SD_INFEASIBLE)
    if not np.any(w > 0):
        return out(np.zeros(n), -np.inf, _lib.SD_NO_OBJECTIVE)
    A_ub = [np.hstack([G, -w[:, None]])]
    b_ub = [np.zeros(k)]
    if b_ineq is not None and np.asarray(b_ineq).size:
        A_ub.append(np.hstack([np.asarray(A_ineq, dtype=np.float64).reshape(-1, n), np.zeros((np.asarray(b_ineq).size, 1))]))
        b_ub.append(np.asarray(b_ineq, dtype=np.float64).ravel())
    Ae = be = None
    if b_eq is not None and np.asarray(b_eq).size:
        Ae = np.hstack([np.asarray(A_eq, dtype=np.float64).reshape(-1, n), np.zeros((np.asarray(b_eq).size, 1))])
        be = np.asarray(b_eq, dtype=np.float64).ravel()
    c = np.zeros(n + 1)
    c[n] = 1.0
    res = linprog(c, A_ub=np.vstack(A_ub), b_ub=np.concatenate(b_ub), A_eq=Ae, b_eq=be,
                  bounds=list(zip(lo, hi)) + [(None, None)], method="highs",
                  options={"primal_feasibility_tolerance": tol, "dual_feasibility_tolerance": tol})
    if res.status != 0:
        return out(np.zeros(n), -np.inf, _lib.SD_INFEASIBLE if res.status == 2 else _lib.SD_NO_OBJECTIVE)
    d = np.clip(res.x[:n], lo, hi)
    return out(d, _sd_omega(G, w, d), _lib.SD_OK)


def _arr(a):
    """an input of a device call: a device tensor as it is, anything else as a contiguous float64 array"""
    return a if hasattr(a, "data_ptr") else np.ascontiguousarray(a, dtype=np.float64)


def _handles(plans):
    """the model handles of the plans, start-major (at least one entry, so that the array exists for a container without models)"""
    hs = [m.model.value if hasattr(m.model, "value") else m.model for p in plans for m in p["models"]]
    return (ctypes.c_void_p * max(len(hs), 1))(*hs)


def _step_options(cfg):
    """the mrbf_sd_step_options of a SteepestDescentConfig"""
    return _lib.SdStepOptions(strict=int(bool(cfg.strict_backtracking)), max_loops=int(cfg.max_loops), const_rhs=float(cfg.armijo_const_rhs),
                              shrink=float(cfg.armijo_const_shrink), min_stepsize=float(cfg.min_stepsize))


def _sd_problem(plan, lin):
    """the mrbf_ps_problem of a container plan (linear constraints lin = (A_eq, b_eq, A_ineq, b_ineq) in scaled variables), for the
    steepest-descent calls and for the normal step alike (which ignores the objective rows); the second value keeps the arrays alive"""
    A_eq, b_eq, A_in, b_in = [None if a is None or np.asarray(a).size == 0 else np.ascontiguousarray(a, dtype=np.float64) for a in lin]
    handles = _handles([plan])
    roles = (ctypes.c_int32 * max(len(plan["roles"]), 1))(*plan["roles"])
    prob = _lib.PsProblem(n_models=len(plan["models"]), n_objectives=plan["k"], models=handles, roles=roles,
                          n_lin_eq=0 if b_eq is None else b_eq.size, n_lin_ineq=0 if b_in is None else b_in.size,
                          A_eq=None if b_eq is None else A_eq.ctypes.data, b_eq=None if b_eq is None else b_eq.ctypes.data,
                          A_ineq=None if b_in is None else A_in.ctypes.data, b_ineq=None if b_in is None else b_in.ctypes.data, eq_tol=-1.0)
    return prob, (handles, roles, A_eq, b_eq, A_in, b_in)


def sd_criticality_device(plan, x, x_n, lb, ub, normalize=True, lin=None, want_duals=False):
    """one mrbf_sd_criticality call; returns (rc, omega, d, info dict[, duals])"""
    ctx = plan["models"][0].ctx
    x, x_n = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(x_n, dtype=np.float64)
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    prob, keep = _sd_problem(plan, lin or (None,) * 4)
    m = plan["k"] + plan["n_con"] + sum(0 if b is None else b.size for b in (keep[3], keep[5]))
    d = np.empty(x_n.size)
    y = np.empty(m) if want_duals else None
    info = _lib.SdInfo()
    rc = ctx.lib.mrbf_sd_criticality(ctx.h, ctypes.byref(prob), _lib.as_ptr(x), _lib.as_ptr(x_n), _lib.as_ptr(lb), _lib.as_ptr(ub),
                                     int(bool(normalize)), _lib.as_ptr(d), _lib.as_ptr(y), ctypes.byref(info))
    out = (rc, float(info.omega), d, info.asdict())
    return out + (y,) if want_duals else out


def _sd_host_rows(sc, scal, x, x_n, lin):
    """G, A_eq, b_eq, A_ineq, b_ineq of get_criticality (descent.jl:196-236) on container Jacobians"""
    x, x_n = np.asarray(x, dtype=np.float64), np.asarray(x_n, dtype=np.float64)
    n = x_n.size
    G = sg.eval_container_objectives_jacobian_at_scaled_site(sc, scal, x_n)
    lin = lin or (None,) * 4
    step = x_n - x
    A_eq, b_eq, A_in, b_in = [np.zeros((0, n))], [np.zeros(0)], [np.zeros((0, n))], [np.zeros(0)]
    if lin[1] is not None and np.asarray(lin[1]).size:
        A = np.asarray(lin[0], dtype=np.float64).reshape(-1, n)
        A_eq.append(A)
        b_eq.append(np.asarray(lin[1], dtype=np.float64) - A @ x_n)
    if lin[3] is not None and np.asarray(lin[3]).size:
        A = np.asarray(lin[2], dtype=np.float64).reshape(-1, n)
        A_in.append(A)
        b_in.append(np.asarray(lin[3], dtype=np.float64) - A @ x_n)
    if sc.lists["nl_eq_constraint"]:
        Dm = sg.eval_container_nl_eq_constraints_jacobian_at_scaled_site(sc, scal, x)
        A_eq.append(Dm)
        b_eq.append(-sg.eval_container_nl_eq_constraints_at_scaled_site(sc, scal, x_n) - Dm @ step)
    if sc.lists["nl_ineq_constraint"]:
        Dm = sg.eval_container_nl_ineq_constraints_jacobian_at_scaled_site(sc, scal, x)
        A_in.append(Dm)
        b_in.append(-sg.eval_container_nl_ineq_constraints_at_scaled_site(sc, scal, x_n) - Dm @ step)
    return G, np.vstack(A_eq), np.concatenate(b_eq), np.vstack(A_in), np.concatenate(b_in)


def get_criticality_sd(cfg, sc, scal, x, x_n, lb, ub, lin=None, stats=None):
    """`get_criticality(::SteepestDescentConfig, mop, scal, x_it, x_it_n, db, sc, ac)` (descent.jl:187-241) as HipRbf.jl routes it:
    mrbf_dispatch_sd decides, mrbf_sd_criticality solves on the device, and where the decision table or mrbf_dispatch_after say so
    the reference method runs -- the HiGHS direction LP on container Jacobians.  lb / ub: the global bounds in scaled variables
    (full_bounds_internal); lin = (A_eq, b_eq, A_ineq, b_ineq) in scaled variables.  Never raises on a size limit.  Returns (omega, d)."""
    lib = _lib.load()
    plan = sg.container_plan(sc)
    n = int(np.asarray(x_n).size)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))
    if lib.mrbf_dispatch_sd(n, plan["k"], len(plan["models"]), plan["n_con"], n_lin, plan["n_foreign"]) == _lib.DISPATCH_DEVICE:
        rc, omega, d, info = sd_criticality_device(plan, x, x_n, lb, ub, cfg.normalize, lin)
        if stats is not None:
            stats.update(info)
            stats["path"] = "device"
        if rc == 0:
            return omega, d
        if not lib.mrbf_dispatch_after(_lib.ENTRY_SD, rc):
            plan["models"][0].ctx.check(rc)
    if stats is not None:
        stats["path"] = "reference"
    G, A_eq, b_eq, A_in, b_in = _sd_host_rows(sc, scal, x, x_n, lin)
    d, omega = _steepest_descent_direction(x_n, G, lb, ub, A_eq, b_eq, A_in, b_in, cfg.normalize)
    return omega, d


# ---- the normal step (descent.jl:691-757): host reference, the dual bound of its certificate, the device call, the routing
def _ns_rows(n, A_eq, b_eq, A_ineq, b_ineq):
    """(C, b, m_eq) of the normal-step LP's rows in the step n: equalities first"""
    A = [np.zeros((0, n))]
    b = [np.zeros(0)]
    for M, v in ((A_eq, b_eq), (A_ineq, b_ineq)):
        if v is not None and np.asarray(v).size:
            A.append(np.asarray(M, dtype=np.float64).reshape(-1, n))
            b.append(np.asarray(v, dtype=np.float64).ravel())
        else:
            A.append(np.zeros((0, n)))
            b.append(np.zeros(0))
    return np.vstack(A), np.concatenate(b), A[1].shape[0]


def _normal_step_lp(x, lb, ub, A_eq=None, b_eq=None, A_ineq=None, b_ineq=None, tol=1e-10):
    """The LP of compute_normal_step (descent.jl:691-757) with HiGHS (scipy.optimize.linprog) in place of JuMP + OSQP, on the
    explicit LP with the 2d rows -alpha <= n_j <= alpha: min alpha over (n, alpha >= 0), lb - x <= n <= ub - x, A_eq n = b_eq,
    A_ineq n <= b_ineq (rows in the step n).  Returns (n, alpha, status, y): n projected into the box (_project_into_box),
    alpha = ||n||_inf, status MRBF_NS_*, y the row multipliers (equalities first, >= 0 on inequality rows); infeasible:
    (NaN, +Inf, NS_INFEASIBLE, None)."""
    from scipy.optimize import linprog

    x = np.asarray(x, dtype=np.float64)
    d = x.size
    lb, ub = np.broadcast_to(np.asarray(lb, dtype=np.float64), (d,)), np.broadcast_to(np.asarray(ub, dtype=np.float64), (d,))
    C, b, meq = _ns_rows(d, A_eq, b_eq, A_ineq, b_ineq)
    lo, hi = lb - x, ub - x
    bad = (np.full(d, np.nan), np.inf, _lib.NS_INFEASIBLE, None)
    if not np.all(lo <= hi):
        return bad
    eye, one = np.eye(d), np.ones((d, 1))
    A_ub = [np.hstack([eye, -one]), np.hstack([-eye, -one]), np.hstack([C[meq:], np.zeros((C.shape[0] - meq, 1))])]
    b_ub = [np.zeros(d), np.zeros(d), b[meq:]]
    Ae = np.hstack([C[:meq], np.zeros((meq, 1))]) if meq else None
    c = np.zeros(d + 1)
    c[d] = 1.0
    bnd = [(None if l == -np.inf else l, None if u == np.inf else u) for l, u in zip(lo, hi)] + [(0.0, None)]
    res = linprog(c, A_ub=np.vstack(A_ub), b_ub=np.concatenate(b_ub), A_eq=Ae, b_eq=b[:meq] if meq else None, bounds=bnd,
                  method="highs", options={"primal_feasibility_tolerance": tol, "dual_feasibility_tolerance": tol})
    if res.status != 0:
        return bad
    n = np.clip(x + res.x[:d], lb, ub) - x
    y = np.concatenate([-res.eqlin.marginals if meq else np.zeros(0), -res.ineqlin.marginals[2 * d:]])
    return n, float(np.max(np.abs(n))), _lib.NS_OK, y


def normal_lp_dual_bound(y, x, lb, ub, A_eq=None, b_eq=None, A_ineq=None, b_ineq=None):
    """phi(y) = -y.b + min over alpha >= alpha0 of [alpha + sum_j min over n_j in [max(l'_j, -alpha), min(u'_j, alpha)] of
    (C'y)_j n_j] (l' = lb - x, u' = ub - x, alpha0 = max(0, max l', max -u')): a lower bound on the normal-step LP's alpha* for
    every y with y >= 0 on the inequality rows (equal to alpha* at the optimal multipliers).  The inner function is convex and
    piecewise linear in alpha: evaluated at alpha0 and at every finite breakpoint above it; -inf where its slope at +inf is
    negative."""
    x = np.asarray(x, dtype=np.float64)
    d = x.size
    C, b, _ = _ns_rows(d, A_eq, b_eq, A_ineq, b_ineq)
    y = np.asarray(y, dtype=np.float64).ravel()
    lo = np.broadcast_to(np.asarray(lb, dtype=np.float64), (d,)) - x
    hi = np.broadcast_to(np.asarray(ub, dtype=np.float64), (d,)) - x
    r = C.T @ y
    a0 = max(0.0, float(np.max(lo)), float(np.max(-hi)))
    pos, neg = r > 0, r < 0
    if 1.0 - r[pos & (lo == -np.inf)].sum() + r[neg & (hi == np.inf)].sum() < 0:
        return -np.inf

    def f(al):
        L, U = np.maximum(lo, -al), np.minimum(hi, al)
        return al + float(np.sum(r[pos] * L[pos]) + np.sum(r[neg] * U[neg]))

    bps = np.concatenate([-lo, hi])
    bps = bps[np.isfinite(bps) & (bps > a0)]
    return float(-y @ b + min([f(a0)] + [f(v) for v in bps]))


def normal_step_device(plan, x, lb, ub, delta, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, want_duals=False):
    """one mrbf_normal_step call; returns (rc, n, delta, info dict[, duals])"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    prob, keep = _sd_problem(plan, lin or (None,) * 4)
    m = plan["n_con"] + sum(0 if b is None else b.size for b in (keep[3], keep[5]))
    ctx = plan["models"][0].ctx if plan["models"] else _lib.default_context()
    n = np.empty(x.size)
    y = np.empty(max(m, 1)) if want_duals else None
    info = _lib.NormalInfo()
    rc = ctx.lib.mrbf_normal_step(ctx.h, ctypes.byref(prob), x.size, _lib.as_ptr(x), _lib.as_ptr(lb), _lib.as_ptr(ub), float(delta),
                                  float(kappa_delta), float(delta_max), int(bool(variable_radius)), _lib.as_ptr(n), _lib.as_ptr(y),
                                  ctypes.byref(info))
    out = (rc, n, float(info.delta), info.asdict())
    return out + (y[:m],) if want_duals else out


def _ns_host_rows(sc, scal, x, lin):
    """A_eq, b_eq, A_ineq, b_ineq of compute_normal_step (descent.jl:700-735) in the step n, on container values / Jacobians at x"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    lin = lin or (None,) * 4
    A_eq, b_eq, A_in, b_in = [np.zeros((0, n))], [np.zeros(0)], [np.zeros((0, n))], [np.zeros(0)]
    if lin[1] is not None and np.asarray(lin[1]).size:
        A = np.asarray(lin[0], dtype=np.float64).reshape(-1, n)
        A_eq.append(A)
        b_eq.append(np.asarray(lin[1], dtype=np.float64) - A @ x)
    if sc.lists["nl_eq_constraint"]:
        A_eq.append(sg.eval_container_nl_eq_constraints_jacobian_at_scaled_site(sc, scal, x))
        b_eq.append(-sg.eval_container_nl_eq_constraints_at_scaled_site(sc, scal, x))
    if lin[3] is not None and np.asarray(lin[3]).size:
        A = np.asarray(lin[2], dtype=np.float64).reshape(-1, n)
        A_in.append(A)
        b_in.append(np.asarray(lin[3], dtype=np.float64) - A @ x)
    if sc.lists["nl_ineq_constraint"]:
        A_in.append(sg.eval_container_nl_ineq_constraints_jacobian_at_scaled_site(sc, scal, x))
        b_in.append(-sg.eval_container_nl_ineq_constraints_at_scaled_site(sc, scal, x))
    return np.vstack(A_eq), np.concatenate(b_eq), np.vstack(A_in), np.concatenate(b_in)


def _ns_radius(n, alpha, status, delta, kappa_delta, delta_max, variable_radius):
    """compute_normal_step's return value from the LP's result: (n, delta) or (NaN, -Inf) when infeasible"""
    if status == _lib.NS_OK:
        if not variable_radius:
            return n, float(delta)
        r = alpha / kappa_delta
        if r <= delta_max:
            return n, float(r)
    return np.full(np.asarray(n).size, np.nan), -np.inf


def compute_normal_step(sc, scal, x, delta, lb, ub, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, stats=None):
    """`compute_normal_step(mop, scal, x_it, data_base, sc, algo_config; variable_radius)` (descent.jl:691-757) as HipRbf.jl's
    `hip_compute_normal_step` routes it: mrbf_dispatch_normal decides, mrbf_normal_step solves on the device, and where the decision
    table or mrbf_dispatch_after say so the reference method runs -- the HiGHS LP on container values and Jacobians at x.  lb / ub:
    the global bounds in scaled variables (full_bounds_internal); lin = (A_eq, b_eq, A_ineq, b_ineq) in scaled variables.
    kappa_delta = filter_kappa_delta, delta_max the largest radius (variable radius only).  Returns (n, delta): n projected into
    the box, delta the given radius or alpha* / kappa_delta; (NaN, -Inf) when infeasible."""
    lib = _lib.load()
    plan = sg.container_plan(sc)
    n_foreign_con = plan["n_foreign"] - sg.container_plan(sc, objectives_only=True)["n_foreign"]
    d = int(np.asarray(x).size)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))
    if lib.mrbf_dispatch_normal(d, len(plan["models"]), plan["n_con"], n_lin, n_foreign_con) == _lib.DISPATCH_DEVICE:
        rc, n, dl, info = normal_step_device(plan, x, lb, ub, delta, lin, kappa_delta, delta_max, variable_radius)
        if stats is not None:
            stats.update(info)
            stats["path"] = "device"
        if rc == 0:
            return n, dl
        if not lib.mrbf_dispatch_after(_lib.ENTRY_NORMAL, rc):
            (plan["models"][0].ctx if plan["models"] else _lib.default_context()).check(rc)
    if stats is not None:
        stats["path"] = "reference"
    A_eq, b_eq, A_in, b_in = _ns_host_rows(sc, scal, x, lin)
    n, alpha, status, _ = _normal_step_lp(x, lb, ub, A_eq, b_eq, A_in, b_in)
    return _ns_radius(n, alpha, status, delta, kappa_delta, delta_max, variable_radius)


def _isapprox(a, b):
    """Julia's isapprox with its defaults (atol = 0, rtol = sqrt(eps)): norm(a - b) <= rtol max(norm(a), norm(b)), or a == b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if np.array_equal(a, b):
        return True
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return False
    return bool(np.linalg.norm(a - b) <= np.sqrt(np.finfo(np.float64).eps) * max(np.linalg.norm(a), np.linalg.norm(b)))


def _local_bounds(x, delta, lb, ub):
    """utilities.jl:290-294"""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(np.asarray(lb, dtype=np.float64), x - delta), np.minimum(np.asarray(ub, dtype=np.float64), x + delta)


def _intersect_bound_vec(x, b, direction, sense):
    """utilities.jl:126-152"""
    b = np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return np.zeros(0)
    nz = direction != 0
    dd = direction[nz]
    tmp = b[nz] - x[nz]
    tz = tmp == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = tmp[~tz] / dd[~tz]
    on = dd[tz]
    if on.size == 0:
        return s
    onb = np.where(on > 0, np.inf, 0.0) if sense == "lb" else np.where(on < 0, np.inf, 0.0)
    return np.concatenate([s, onb])


def _intersect_bounds(x, d, lb=(), ub=(), A_eq=None, b_eq=None, A_ineq=None, b_ineq=None, ret_mode="pos", impossible_val=0.0):
    """utilities.jl:156-282 (_eps = 0): the largest (ret_mode "pos") / smallest ("neg") step sigma with lb <= x + sigma d <= ub,
    A_eq (x + sigma d) = b_eq, A_ineq (x + sigma d) <= b_ineq"""
    x, d = np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.float64)
    if not np.any(d):
        return np.inf
    has_eq = A_eq is not None and np.asarray(A_eq).size > 0
    has_in = A_ineq is not None and np.asarray(A_ineq).size > 0
    if not has_eq:
        s = [_intersect_bound_vec(x, lb, d, "lb"), _intersect_bound_vec(x, ub, d, "ub")]
        if has_in:
            A = np.asarray(A_ineq, dtype=np.float64)
            bi = np.zeros(x.size) if b_ineq is None or np.asarray(b_ineq).size == 0 else np.asarray(b_ineq, dtype=np.float64)
            s.append(_intersect_bound_vec(A @ x, bi, A @ d, "ub"))
        s = np.concatenate(s)
        if s.size == 0:
            return -np.inf if ret_mode == "neg" else np.inf
        pos, neg = s[s >= 0], s[~(s >= 0)]
        s_pos = float(pos.min()) if pos.size else 0.0
        s_neg = float(neg.max()) if neg.size else 0.0
        if ret_mode == "pos":
            return s_pos
        if ret_mode == "neg":
            return s_neg
        if ret_mode == "absmax":
            return s_pos if abs(s_pos) >= abs(s_neg) else s_neg
        return s_neg, s_pos
    A = np.asarray(A_eq, dtype=np.float64)
    be = np.zeros(A.shape[0]) if b_eq is None or np.asarray(b_eq).size == 0 else np.asarray(b_eq, dtype=np.float64)
    sigma = None
    for i in range(A.shape[0]):
        ad = float(A[i] @ d)
        if ad != 0:
            s_i = -(float(A[i] @ x) - be[i]) / ad
        else:
            if abs(float(A[i] @ x) - be[i]) > np.finfo(np.float64).eps:
                return impossible_val
            continue
        if sigma is None:
            sigma = s_i
        elif not (s_i == sigma or abs(s_i - sigma) <= np.sqrt(np.finfo(np.float64).eps) * max(abs(s_i), abs(sigma))):
            return impossible_val
    if sigma is None:
        sigma = np.inf
    if np.isinf(sigma):
        return _intersect_bounds(x, d, lb, ub, None, None, A_ineq, b_ineq)
    xt = x + sigma * d
    bi = np.zeros(x.size) if b_ineq is None or np.asarray(b_ineq).size == 0 else np.asarray(b_ineq, dtype=np.float64)
    if (np.size(lb) and np.any(xt < np.asarray(lb))) or (np.size(ub) and np.any(xt > np.asarray(ub))) or \
            (has_in and np.any(np.asarray(A_ineq) @ xt - bi > 0)):
        return impossible_val
    if ret_mode == "pos" and sigma < 0:
        return impossible_val
    if ret_mode == "neg" and sigma >= 0:
        return impossible_val
    return sigma


def intersect_box(x, d, lb, ub, return_vals="absmax"):
    """utilities.jl:285-287"""
    return _intersect_bounds(x, d, lb, ub, ret_mode=return_vals)


def _blockdiag(A, B):
    A, B = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(B, dtype=np.float64))
    out = np.zeros((A.shape[0] + B.shape[0], A.shape[1] + B.shape[1]))
    out[:A.shape[0], :A.shape[1]] = A
    out[A.shape[0]:, A.shape[1]:] = B
    return out


def _sd_stepsize(x, x_n, delta, lb, ub, d, lin=None, constraints_at_x=None):
    """the initial step size sigma of compute_descent_step (descent.jl:251-303) and the branch that chose it ("delta" for
    Delta <= 1, "intersect" for ||d|| ~ 1 beyond, else "one").  constraints_at_x() -> (Dm_eq, m_eq, Dm_ineq, m_ineq) at x,
    asked for only on the "intersect" branch."""
    x, x_n, d = np.asarray(x, dtype=np.float64), np.asarray(x_n, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n = x.size
    lb_eff, ub_eff = _local_bounds(x, delta, lb, ub)
    Delta = delta if _isapprox(x, x_n) else intersect_box(x_n, d, lb_eff, ub_eff, return_vals="pos")
    norm_d = float(np.max(np.abs(d))) if n else 0.0
    if Delta <= 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float64(Delta) / np.float64(norm_d)
        return (r if np.isnan(r) else min(float(r), 1.0)), "delta"
    if not _isapprox(norm_d, 1.0):
        return 1.0, "one"
    lin = lin or (None,) * 4
    A_eq = np.zeros((0, n)) if lin[1] is None else np.asarray(lin[0], dtype=np.float64).reshape(-1, n)
    b_eq = np.zeros(0) if lin[1] is None else np.asarray(lin[1], dtype=np.float64).ravel()
    A_in = np.zeros((0, n)) if lin[3] is None else np.asarray(lin[2], dtype=np.float64).reshape(-1, n)
    b_in = np.zeros(0) if lin[3] is None else np.asarray(lin[3], dtype=np.float64).ravel()
    Dm_eq, m_eq, Dm_in, m_in = constraints_at_x() if constraints_at_x else (np.zeros((0, n)), np.zeros(0), np.zeros((0, n)), np.zeros(0))
    step_n = x_n - x
    sigma = _intersect_bounds(np.concatenate([x_n, step_n]), np.concatenate([d, d]), np.concatenate([lb_eff, lb_eff - x]),
                              np.concatenate([ub_eff, ub_eff - x]), _blockdiag(A_eq, np.reshape(Dm_eq, (-1, n))),
                              np.concatenate([b_eq, -np.ravel(m_eq)]), _blockdiag(A_in, np.reshape(Dm_in, (-1, n))),
                              np.concatenate([b_in, -np.ravel(m_in)]), ret_mode="pos")
    return sigma, "intersect"


def compute_descent_step_sd(cfg, sc, scal, x, x_n, delta, lb, ub, omega, d, lin=None):
    """compute_descent_step(::SteepestDescentConfig, ...) (descent.jl:243-320): the initial step size sigma, then the batched
    `_backtrack` from x_n along d.  lb / ub: global bounds in scaled variables.  Returns (omega, x_plus, mx_plus, ||step||_inf)."""
    x, x_n = np.asarray(x, dtype=np.float64), np.asarray(x_n, dtype=np.float64)

    def constraints_at_x():
        n = x.size
        out = []
        for kind in ("nl_eq_constraints", "nl_ineq_constraints"):
            if sc.lists[kind[:-1]]:
                out += [getattr(sg, "eval_container_%s_jacobian_at_scaled_site" % kind)(sc, scal, x),
                        getattr(sg, "eval_container_%s_at_scaled_site" % kind)(sc, scal, x)]
            else:
                out += [np.zeros((0, n)), np.zeros(0)]
        return tuple(out)

    sigma, _ = _sd_stepsize(x, x_n, delta, lb, ub, d, lin, constraints_at_x)
    if sigma > cfg.min_stepsize:
        xp, mxp, step, _ = _backtrack(x_n, d, sigma, omega, sc, cfg, scal)
        return omega, xp, mxp, float(np.max(np.abs(step))) if step.size else 0.0
    return 0, x_n.copy(), sg.eval_container_objectives_at_scaled_site(sc, scal, x_n), 0


# ---- the steepest-descent step on the device (descent.jl:243-318 with _backtrack :150-185): mrbf_sd_step and its routing -------------
_SD_BRANCHES = ("delta", "one", "intersect")


def sd_step_device(plan, cfg, x, x_n, delta, lb, ub, omega, d, lin=None, out=None):
    """one mrbf_sd_step call; returns (rc, x_plus, mx_plus, info dict with the branch name under "branch_name").  x, x_n, lb, ub, d
    may be NumPy arrays or device tensors; out = (x_plus, mx_plus) lets the caller pass its own output buffers (host or device)."""
    ctx = plan["models"][0].ctx
    x, x_n, lb, ub, d = _arr(x), _arr(x_n), _arr(lb), _arr(ub), _arr(d)
    prob, keep = _sd_problem(plan, lin or (None,) * 4)
    n = int(x_n.numel() if hasattr(x_n, "numel") else x_n.size)
    xp, mxp = out if out is not None else (np.empty(n), np.empty(plan["k"]))
    opts = _step_options(cfg)
    info = _lib.SdStepInfo()
    rc = ctx.lib.mrbf_sd_step(ctx.h, ctypes.byref(prob), _lib.as_ptr(x), _lib.as_ptr(x_n), float(delta), _lib.as_ptr(lb), _lib.as_ptr(ub),
                              float(omega), _lib.as_ptr(d), ctypes.byref(opts), _lib.as_ptr(xp), _lib.as_ptr(mxp), ctypes.byref(info))
    dd = info.asdict()
    dd["branch_name"] = _SD_BRANCHES[info.branch] if rc == 0 and 0 <= info.branch < 3 else None
    return rc, xp, mxp, dd


def compute_descent_step_sd_routed(cfg, sc, scal, x, x_n, delta, lb, ub, omega, d, lin=None, stats=None):
    """`compute_descent_step(::SteepestDescentConfig, ...)` (descent.jl:243-318) as HipRbf.jl's `hip_compute_descent_step` routes it:
    mrbf_dispatch_sd_step decides, mrbf_sd_step computes sigma, the trial points, their values and the Armijo stop in one call, and
    where the decision table or mrbf_dispatch_after say so `compute_descent_step_sd` runs.  Same arguments and result:
    (omega, x_plus, mx_plus, ||step||_inf)."""
    lib = _lib.load()
    plan = sg.container_plan(sc)
    n = int(np.asarray(x_n).size)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))
    if lib.mrbf_dispatch_sd_step(n, plan["k"], len(plan["models"]), plan["n_con"], n_lin, plan["n_foreign"], int(cfg.max_loops)) \
            == _lib.DISPATCH_DEVICE:
        rc, xp, mxp, info = sd_step_device(plan, cfg, x, x_n, delta, lb, ub, omega, d, lin)
        if stats is not None:
            stats.update(info)
            stats["path"] = "device"
        if rc == 0:
            if not info["sigma"] > cfg.min_stepsize:       # descent.jl:317: the reference returns integer zeros here
                return 0, xp, mxp, 0
            return omega, xp, mxp, info["step_norm"]
        if not lib.mrbf_dispatch_after(_lib.ENTRY_SD_STEP, rc):
            plan["models"][0].ctx.check(rc)
    if stats is not None:
        stats["path"] = "reference"
    return compute_descent_step_sd(cfg, sc, scal, x, x_n, delta, lb, ub, omega, d, lin)


# ---- many starts in one device call (mrbf_sd_iterate_batch): the reference's Threads.@threads loop over starts ---------------------
def sd_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, lin=None, out=None):
    """one mrbf_sd_iterate_batch call on the containers' plans (one shape, checked by the caller); X, X_n (n_starts x d), deltas,
    lb, ub may be NumPy arrays or device tensors; out = (d, x_plus, mx_plus) lets the caller pass its own output buffers (host or
    device).  Returns (rc, d, x_plus, mx_plus, list of record dicts with "branch_name", event ms)."""
    ctx = plans[0]["models"][0].ctx
    ns, k = len(plans), plans[0]["k"]
    X, X_n, deltas, lb, ub = _arr(X), _arr(X_n), _arr(deltas), _arr(lb), _arr(ub)
    n = int(lb.numel() if hasattr(lb, "numel") else lb.size)
    prob, keep = _sd_problem(plans[0], lin or (None,) * 4)
    handles = _handles(plans)
    dd, xp, mxp = out if out is not None else (np.empty((ns, n)), np.empty((ns, n)), np.empty((ns, k)))
    opts = _step_options(cfg)
    recs = (_lib.SdBatchRecord * ns)()
    ms = ctypes.c_float()
    rc = ctx.lib.mrbf_sd_iterate_batch(ctx.h, ns, ctypes.byref(prob), handles, _lib.as_ptr(X), _lib.as_ptr(X_n), _lib.as_ptr(deltas),
                                       _lib.as_ptr(lb), _lib.as_ptr(ub), int(bool(cfg.normalize)), ctypes.byref(opts), _lib.as_ptr(dd),
                                       _lib.as_ptr(xp), _lib.as_ptr(mxp), recs, ctypes.byref(ms))
    records = []
    for r in recs:
        rd = r.asdict()
        rd["branch_name"] = _SD_BRANCHES[r.branch] if rc == 0 and 0 <= r.branch < 3 else None
        records.append(rd)
    return rc, dd, xp, mxp, records, ms.value


def _same_plan_shape(plans):
    """do the containers share what mrbf_sd_iterate_batch requires: the model count, every slot's output count, the roles table and
    no foreign surrogate count that differs"""
    p0 = plans[0]
    sig0 = ([m.num_outputs for m in p0["models"]], p0["roles"], p0["k"], p0["n_con"], p0["n_foreign"])
    return all(([m.num_outputs for m in p["models"]], p["roles"], p["k"], p["n_con"], p["n_foreign"]) == sig0 for p in plans[1:])


def sd_iterate_many(cfg, containers, scal, X, X_n, deltas, lb, ub, lin=None, stats=None):
    """get_criticality then compute_descent_step (descent.jl:187-318) for many independent starts of one problem -- the reference's
    `Threads.@threads` loop over starts (examples/large_scale_benchmarks.jl:102-109): containers[p] is start p's surrogate container,
    X[p] / X_n[p] / deltas[p] its iterate, normal-step iterate and radius; lb / ub and lin belong to the one MOP.  Where the
    containers share one plan shape and mrbf_dispatch_sd_batch says so, ONE mrbf_sd_iterate_batch call serves all starts ("batch");
    otherwise, and for every start whose direction LP gave up, the routed single-start functions run (`get_criticality_sd`, then
    `compute_descent_step_sd_routed`).  Returns a list of (omega, d, x_plus, mx_plus, ||step||_inf); stats gets "path" ("batch" or
    "loop") and "rerouted", the starts that took the single-start functions after a batch call."""
    lib = _lib.load()
    X, X_n = np.asarray(X, dtype=np.float64), np.asarray(X_n, dtype=np.float64)
    deltas = np.asarray(deltas, dtype=np.float64).ravel()
    ns = len(containers)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))

    def single(p):
        omega, d = get_criticality_sd(cfg, containers[p], scal, X[p], X_n[p], lb, ub, lin)
        om, xp, mxp, nrm = compute_descent_step_sd_routed(cfg, containers[p], scal, X[p], X_n[p], float(deltas[p]), lb, ub, omega, d, lin)
        return om, d, xp, mxp, nrm

    if stats is not None:
        stats["path"], stats["rerouted"] = "loop", []
    if ns == 0:
        return []
    plans = [sg.container_plan(sc) for sc in containers]
    n = int(X_n.shape[1])
    p0 = plans[0]
    if _same_plan_shape(plans) and lib.mrbf_dispatch_sd_batch(ns, n, p0["k"], len(p0["models"]), p0["n_con"], n_lin, p0["n_foreign"],
                                                              int(cfg.max_loops)) == _lib.DISPATCH_DEVICE:
        rc, dd, xp, mxp, records, ms = sd_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, lin)
        if rc == 0:
            res, rerouted = [], []
            for p, r in enumerate(records):
                if r["sd_status"] == _lib.SD_GAVE_UP:          # this start's LP gave up: the reference method for it alone
                    rerouted.append(p)
                    res.append(single(p))
                elif not r["sigma"] > cfg.min_stepsize:        # descent.jl:317: the reference returns integer zeros here
                    res.append((0, dd[p].copy(), xp[p].copy(), mxp[p].copy(), 0))
                else:
                    res.append((r["omega"], dd[p].copy(), xp[p].copy(), mxp[p].copy(), r["step_norm"]))
            if stats is not None:
                stats.update(path="batch", rerouted=rerouted, records=records, ms_total=ms)
            return res
        if not lib.mrbf_dispatch_after(_lib.ENTRY_SD_BATCH, rc):
            p0["models"][0].ctx.check(rc)
    return [single(p) for p in range(ns)]


# ---- the normal steps of many starts in one device call (mrbf_normal_step_batch) ------------------------------------------------------
def normal_step_batch_device(plans, X, lb, ub, deltas, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, out=None,
                             want_duals=False):
    """one mrbf_normal_step_batch call on the containers' plans (one shape, checked by the caller); X (n_starts x d), lb, ub, deltas
    may be NumPy arrays or device tensors; out = (n, x_n) lets the caller pass its own output buffers (host or device).  Returns
    (rc, n, x_n, list of record dicts, event ms[, duals])."""
    ns, nm = len(plans), len(plans[0]["models"])
    ctx = plans[0]["models"][0].ctx if nm else _lib.default_context()
    X, lb, ub, deltas = _arr(X), _arr(lb), _arr(ub), _arr(deltas)
    d = int(lb.numel() if hasattr(lb, "numel") else lb.size)
    prob, keep = _sd_problem(plans[0], lin or (None,) * 4)
    m = plans[0]["n_con"] + sum(0 if b is None else b.size for b in (keep[3], keep[5]))
    handles = _handles(plans)
    n, x_n = out if out is not None else (np.empty((ns, d)), np.empty((ns, d)))
    y = np.empty((ns, max(m, 1))) if want_duals else None
    recs = (_lib.NormalBatchRecord * ns)()
    ms = ctypes.c_float()
    rc = ctx.lib.mrbf_normal_step_batch(ctx.h, ns, ctypes.byref(prob), handles if nm else None, d, _lib.as_ptr(X), _lib.as_ptr(lb),
                                        _lib.as_ptr(ub), _lib.as_ptr(deltas), float(kappa_delta), float(delta_max),
                                        int(bool(variable_radius)), _lib.as_ptr(n), _lib.as_ptr(x_n), _lib.as_ptr(y), recs, ctypes.byref(ms))
    res = (rc, n, x_n, [r.asdict() for r in recs], ms.value)
    return res + (y[:, :m],) if want_duals else res


def normal_steps_many(containers, scal, X, deltas, lb, ub, lin=None, kappa_delta=1.0, delta_max=np.inf, variable_radius=False, stats=None,
                      x_n_out=None):
    """compute_normal_step (descent.jl:691-757) for many independent starts of one problem -- the reference's `Threads.@threads` loop
    over starts (examples/large_scale_benchmarks.jl:102-109): containers[p] is start p's surrogate container, X[p] / deltas[p] its
    iterate and radius; lb / ub and lin belong to the one MOP.  Where the containers share one plan shape and
    mrbf_dispatch_normal_batch says so, ONE mrbf_normal_step_batch call serves all starts ("batch"); otherwise, and for every start
    whose LP gave up, the routed single-start function runs (`compute_normal_step`).  Returns a list of (n, delta); stats gets "path"
    ("batch" or "loop"), "rerouted" (the starts that took the single-start function after a batch call), and after a batch call
    "records" and "ms_total".  x_n_out (n_starts x d, a NumPy array or a device tensor) receives x + n of every start: given a device
    tensor the batch writes it on the device, ready to be the X_n of `sd_iterate_batch_device`."""
    lib = _lib.load()
    X = np.asarray(X, dtype=np.float64)
    deltas = np.asarray(deltas, dtype=np.float64).ravel()
    ns = len(containers)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))

    def single(p):
        n, dl = compute_normal_step(containers[p], scal, X[p], float(deltas[p]), lb, ub, lin, kappa_delta, delta_max, variable_radius)
        if x_n_out is not None:
            x_n_out[p] = x_n_out.new_tensor(X[p] + n) if hasattr(x_n_out, "new_tensor") else X[p] + n
        return n, dl

    if stats is not None:
        stats["path"], stats["rerouted"] = "loop", []
    if ns == 0:
        return []
    plans = [sg.container_plan(sc) for sc in containers]
    d = int(X.shape[1])
    p0 = plans[0]
    n_foreign_con = p0["n_foreign"] - sg.container_plan(containers[0], objectives_only=True)["n_foreign"]
    if _same_plan_shape(plans) and lib.mrbf_dispatch_normal_batch(ns, d, len(p0["models"]), p0["n_con"], n_lin, n_foreign_con) \
            == _lib.DISPATCH_DEVICE:
        out = None if x_n_out is None else (np.empty((ns, d)), x_n_out)
        rc, n, _, records, ms = normal_step_batch_device(plans, X, lb, ub, deltas, lin, kappa_delta, delta_max, variable_radius, out=out)
        if rc == 0:
            res, rerouted = [], []
            for p, r in enumerate(records):
                if r["status"] == _lib.NS_GAVE_UP:             # this start's LP gave up: the reference method for it alone
                    rerouted.append(p)
                    res.append(single(p))
                else:
                    res.append((n[p].copy(), float(r["delta"])))
            if stats is not None:
                stats.update(path="batch", rerouted=rerouted, records=records, ms_total=ms)
            return res
        if not lib.mrbf_dispatch_after(_lib.ENTRY_NORMAL_BATCH, rc):
            (p0["models"][0].ctx if p0["models"] else _lib.default_context()).check(rc)
    return [single(p) for p in range(ns)]
