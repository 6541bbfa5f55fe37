"""Host-side mirror of the descent-step consumers of the surrogate path.

Mirrors /root/reference/src/descent.jl: SteepestDescentConfig backtracking fields (:55-66),
_armijo_condition (:137-143) and _backtrack (:150-185); and the steepest-descent criticality: the direction LP
_steepest_descent_direction (:91-135, HiGHS on the host), get_criticality (:187-241, routed to mrbf_sd_criticality) and
compute_descent_step (:243-320) with intersect_box / _intersect_bounds (utilities.jl:126-287).  The reference evaluates the <= max_loops
step sizes one after another; here all of them go to the device in one batch (mrbf_backtrack when the
objectives are one grouped RbfModel, else one batched container sweep) and the same loop logic picks
the step, so the returned (x_plus, mx_plus, step) are those of the sequential loop.  Directed search (:583-664, parked in the
reference): DirectedSearchConfig, the direction QP's host method (_directed_search_direction: the active-set method of ds_qp.hip in
NumPy), get_criticality_ds (routed to mrbf_ds_criticality) and compute_descent_step_ds (the steepest-descent step on its direction).
"""
import ctypes
import math
from dataclasses import dataclass, field
from typing import Sequence

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


# ---- directed search (descent.jl:583-664): the direction QP, its host method, the device calls, the routing -------------------------
# The constants of the active-set method, shared in value with ds_qp.hip:
DS_RANK_TOL = 1e-12     # a row of M = G_N G_N' whose residual diagonal falls to DS_RANK_TOL M_ii depends on the rows pivoted before it
DS_VANISH_TOL = 1e-13   # a step with |dz_i| <= DS_VANISH_TOL (sum_j |G_ij| + |r_i|) in every row has vanished
DS_DUAL_TOL = 1e-11     # a multiplier violates its sign beyond DS_DUAL_TOL times the magnitudes it was formed from
DS_FEAS_TOL = 1e-13     # sd_lp.hip's FEAS_TOL: rows g_i . d <= DS_FEAS_TOL sum_j |G_ij|
DS_START_TOL = 1e-10    # ds_rows_host.hpp's START_TOL: a constraint row that d = 0 misses by DS_START_TOL sum_j |W_ij| is clamped (section 23)


@dataclass
class DirectedSearchConfig:
    """the configuration of the parked `compute_descent_step(::Val{:ds}, ...)` (descent.jl:583-664): the reference fields of
    PascolettiSerafiniConfig that choose the image direction (descent.jl:599-611) and the backtracking fields of
    SteepestDescentConfig for the step that follows"""
    reference_point: Sequence[float] = field(default_factory=list)
    reference_direction: Sequence[float] = field(default_factory=list)
    max_ideal_point_problem_evals: int = -1
    reference_algo: str = "GN_ISRES"
    reference_trust_region_factor: float = 1.1
    strict_backtracking: bool = True
    armijo_const_rhs: float = 1e-6
    armijo_const_shrink: float = 0.75
    min_stepsize: float = 10 * np.finfo(np.float64).eps
    max_loops: int = None
    normalize: bool = True
    constraint_rows: str = "host"     # "device": a container or problem with constraint rows takes mrbf_ds_criticality_rows
    ideal_point: str = "host"         # "device": the default image direction's ideal-point search takes mrbf_ideal_point_problem / _batch

    def __post_init__(self):
        assert all(v > 0 for v in self.reference_direction), "The components of the `reference_direction` cannot be negative."
        assert self.constraint_rows in ("host", "device")
        assert self.ideal_point in ("host", "device")
        if self.max_loops is None:  # descent.jl:61-66
            base = self.min_stepsize if self.min_stepsize > 0 else np.finfo(np.float64).eps
            self.max_loops = int(math.floor(math.log(base) / math.log(self.armijo_const_shrink)))
        assert self.armijo_const_rhs > 0


def _ds_factor(M, in_s, max_rank=None):
    """Cholesky of M with pivots taken from the row set S first (largest residual diagonal, lowest index on ties), then from the other
    rows; a row whose residual diagonal is within DS_RANK_TOL M_ii is left out (it depends on the pivoted rows).  A row of S that is
    left out leaves S (in place): the working set stays independent, and the row moves with the pivoted rows of S anyway.  Returns
    (piv, n_s, L): the pivot rows in order, how many of them lie in S, and L (k x rank) with M[piv, piv] = L[piv] L[piv]'.  max_rank
    (the rows method's count of free variables) ends the pivoting: the rank of W_N is at most |N|, whatever
    rounding leaves on a residual diagonal."""
    k = M.shape[0]
    dg = np.diag(M).copy()
    tol = DS_RANK_TOL * np.diag(M)
    L = np.zeros((k, k))
    piv, done, n_s = [], np.zeros(k, dtype=bool), 0
    for phase in (True, False):
        while True:
            best, bv = -1, 0.0
            for i in range(k):
                if not done[i] and bool(in_s[i]) == phase and dg[i] > tol[i] and dg[i] > bv:
                    best, bv = i, dg[i]
            if best < 0 or len(piv) == max_rank:
                break
            c = len(piv)
            L[best, c] = math.sqrt(dg[best])
            done[best] = True
            piv.append(best)
            for i in range(k):
                if done[i]:
                    continue
                acc = M[i, best]
                for q in range(c):
                    acc -= L[i, q] * L[best, q]
                L[i, c] = acc / L[best, c]
                dg[i] -= L[i, c] * L[i, c]
        if phase:
            n_s = len(piv)
            for i in range(k):
                in_s[i] = bool(done[i])
    return piv, n_s, L


def _ds_step_coeffs(M, in_s, z, rho, max_rank=None):
    """a (k) with the minimum-norm step p_N = G_N' a: dz = M a has dz_S = -z_S (the rows of S stay on zero) and is nearest to rho on
    the other rows.  Returns (a, factor) or (None, factor) where the small normal equations break down."""
    k = M.shape[0]
    piv, n_s, L = fac = _ds_factor(M, in_s, max_rank)
    rank = len(piv)
    c = np.zeros(rank)
    for a in range(n_s):
        p = piv[a]
        acc = -z[p]
        for q in range(a):
            acc -= L[p, q] * c[q]
        c[a] = acc / L[p, a]
    r2 = rank - n_s
    T = [i for i in range(k) if not in_s[i]]
    if r2:
        t = np.zeros(k)
        for i in T:
            acc = rho[i]
            for q in range(n_s):
                acc -= L[i, q] * c[q]
            t[i] = acc
        if len(T) == r2:      # every other row pivoted: a triangular solve in pivot order
            for b in range(r2):
                p = piv[n_s + b]
                acc = t[p]
                for q in range(b):
                    acc -= L[p, n_s + q] * c[n_s + q]
                c[n_s + b] = acc / L[p, n_s + b]
        else:                 # least squares over all other rows: normal equations of the r2 columns, Cholesky
            A = np.zeros((r2, r2))
            bv = np.zeros(r2)
            for a in range(r2):
                for b in range(a + 1):
                    acc = 0.0
                    for i in T:
                        acc += L[i, n_s + a] * L[i, n_s + b]
                    A[a, b] = acc
                acc = 0.0
                for i in T:
                    acc += L[i, n_s + a] * t[i]
                bv[a] = acc
            for a in range(r2):
                for b in range(a + 1):
                    acc = A[a, b]
                    for q in range(b):
                        acc -= A[a, q] * A[b, q]
                    if a == b:
                        if not acc > 0.0:
                            return None, fac
                        A[a, a] = math.sqrt(acc)
                    else:
                        A[a, b] = acc / A[b, b]
            for a in range(r2):
                acc = bv[a]
                for q in range(a):
                    acc -= A[a, q] * bv[q]
                bv[a] = acc / A[a, a]
            for a in range(r2 - 1, -1, -1):
                acc = bv[a]
                for q in range(a + 1, r2):
                    acc -= A[q, a] * bv[q]
                bv[a] = acc / A[a, a]
            c[n_s:] = bv
    av = np.zeros(k)
    for a in range(rank - 1, -1, -1):
        acc = c[a]
        for q in range(a + 1, rank):
            acc -= L[piv[q], a] * av[piv[q]]
        av[piv[a]] = acc / L[piv[a], a]
    return av, fac


def _ds_multipliers(M, fac, rho):
    """mu (k): M_PP mu_P = (M rho)_P on the pivoted rows P of S, zero elsewhere -- the multipliers of the rows held at zero"""
    piv, n_s, L = fac
    k = M.shape[0]
    mu = np.zeros(k)
    w = np.zeros(n_s)
    for a in range(n_s):
        p = piv[a]
        acc = 0.0
        for i in range(k):
            acc += M[p, i] * rho[i]
        for q in range(a):
            acc -= L[p, q] * w[q]
        w[a] = acc / L[p, a]
    for a in range(n_s - 1, -1, -1):
        acc = w[a]
        for q in range(a + 1, n_s):
            acc -= L[piv[q], a] * mu[piv[q]]
        mu[piv[a]] = acc / L[piv[a], a]
    return mu


def _ds_active_set(G, r, lo, hi, stats=None):
    """The direction QP of directed search, min 1/2 ||G d - r||^2 over lo <= d <= hi, G d <= 0 (descent.jl:635-640), by the primal
    active-set method with minimum-norm steps that ds_qp.hip runs: d starts at 0 with an empty row set S; a
    step is p_N = G_N' a on the free variables N, found from the k x k matrix M = G_N G_N' alone; the ratio test adds the bounds and
    rows that block; where the step vanishes the most violating multiplier is dropped.  After a step of length zero (a degenerate
    point: more constraints meet than the working set holds) the least index decides instead, rows before variables, for the one
    constraint that is added and for the one that is dropped (Bland's rule), until a step moves again.  Returns (d, z, omega, mu,
    status)."""
    G = np.asarray(G, dtype=np.float64)
    k, n = G.shape
    r = np.asarray(r, dtype=np.float64)
    nan_d = (np.full(n, np.nan), np.full(k, np.nan), np.nan, np.full(k, np.nan), _lib.DS_GAVE_UP)

    def gave_up(why):
        if stats is not None:
            stats["gave_up"] = why
        return nan_d

    if not np.all(r < 0):     # some r_i >= 0, or a NaN (descent.jl:615-617)
        return np.zeros(n), np.zeros(k), 0.0, np.zeros(k), _lib.DS_CRITICAL
    if not np.all(lo <= hi):
        return np.zeros(n), np.zeros(k), -np.inf, np.zeros(k), _lib.DS_INFEASIBLE
    if not (np.all(lo <= 0.0) and np.all(hi >= 0.0)):
        return gave_up("start")   # the start d = 0 is outside the box: x is outside [lb, ub] by less than one
    absG = np.abs(G)
    rowsum = absG.sum(axis=1)
    rscale = rowsum + np.abs(r)
    d = np.zeros(n)
    flag = np.where(lo == hi, 2, np.where(lo == 0.0, -1, np.where(hi == 0.0, 1, 0)))
    in_s = np.zeros(k, dtype=bool)
    degen = False
    free = flag == 0
    M = G[:, free] @ G[:, free].T
    cap = 8 * (n + k) + 16
    iters = dropped = full = 0
    mu = np.zeros(k)
    while True:
        if iters >= cap:
            return gave_up("cap")
        iters += 1
        z = G @ d
        rho = r - z
        av, fac = _ds_step_coeffs(M, in_s, z, rho)
        if av is None:
            return gave_up("normal equations")
        free = flag == 0
        p = np.where(free, G.T @ av, 0.0)
        dz = G @ p
        if full >= 2 or np.all(np.abs(dz) <= DS_VANISH_TOL * rscale):
            mu = _ds_multipliers(M, fac, rho)
            y = mu - rho
            s = G.T @ y
            sscale = absG.T @ (np.abs(r) + np.abs(z) + np.abs(mu))
            mscale = float(np.max(np.abs(r) + np.abs(z)))
            best, kind, idx = 0.0, 0, -1
            for i in range(k):
                v = -mu[i] / mscale if in_s[i] else 0.0
                if v > DS_DUAL_TOL and v > best and not (degen and kind):
                    best, kind, idx = v, 1, i
            viol = np.where(flag == -1, -s, np.where(flag == 1, s, 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(sscale > 0, viol / sscale, 0.0)
            if degen:             # the least index that violates; a row goes first
                cand = np.flatnonzero(ratio > DS_DUAL_TOL)
                j = int(cand[0]) if cand.size and not kind else -1
            else:
                j = int(np.argmax(ratio)) if n else -1
            if j >= 0 and ratio[j] > DS_DUAL_TOL and (degen or ratio[j] > best):
                best, kind, idx = float(ratio[j]), 2, j
            if kind == 0:
                break
            dropped += 1
            full = 0
            if kind == 1:
                in_s[idx] = False
            else:
                flag[idx] = 0
                fr = flag == 0
                M = G[:, fr] @ G[:, fr].T
            continue
        # ---- ratio test over the free variables' bounds and the rows outside S
        with np.errstate(divide="ignore", invalid="ignore"):
            av_j = np.where(free & (p < 0), (lo - d) / p, np.where(free & (p > 0), (hi - d) / p, np.inf))
        av_j = np.where(av_j < 0, 0.0, av_j)
        alpha = 1.0
        if n:
            alpha = min(alpha, float(av_j.min()))
        ar = np.full(k, np.inf)
        for i in range(k):
            if not in_s[i] and dz[i] > DS_VANISH_TOL * rscale[i]:
                ar[i] = max(0.0, -z[i] / dz[i])
        alpha = min(alpha, float(ar.min()))
        hit = free & (av_j <= alpha)
        rows_hit = ar <= alpha
        degen = not alpha > 0.0
        if degen:                 # a step of length zero adds one constraint: the least index that blocks, a row first
            first_row = np.flatnonzero(rows_hit)
            rows_hit = np.zeros(k, dtype=bool)
            if first_row.size:
                rows_hit[first_row[0]] = True
                hit = np.zeros(n, dtype=bool)
            else:
                first = int(np.argmax(hit))
                hit = np.zeros(n, dtype=bool)
                hit[first] = True
        d = np.where(free, np.minimum(np.maximum(d + alpha * p, lo), hi), d)
        d = np.where(hit, np.where(p < 0, lo, hi), d)
        flag = np.where(hit, np.where(p < 0, -1, 1), flag)
        in_s |= rows_hit
        nh = int(hit.sum())
        full = full + 1 if (nh == 0 and not rows_hit.any()) else 0
        if nh >= 1:           # M from G whenever N changes: a rank-one downdate would cancel against the columns that have left
            fr = flag == 0
            M = G[:, fr] @ G[:, fr].T
    z = G @ d
    if not np.all(z <= DS_FEAS_TOL * rowsum):
        return gave_up("rows")
    if stats is not None:
        stats["iterations"], stats["dropped"] = iters, dropped
    return d, z, max(0.0, -float(np.max(z))), mu, _lib.DS_OK


def _ds_rows_start(W, k, m_eq, h):
    """the start rule of the QP with constraint rows: d = 0 must satisfy the rows.  A residual of the start
    within DS_START_TOL sum_j |W_ij| -- |b_eq,i|, or -b_in,i where b_in,i < 0 -- is clamped to zero (in place); returns False where
    one is larger."""
    rowsum = np.abs(W).sum(axis=1)
    for i in range(k, W.shape[0]):
        miss = abs(h[i]) if i < k + m_eq else -h[i]
        if not miss <= 0.0:       # a miss, or a NaN
            if not miss <= DS_START_TOL * rowsum[i]:
                return False
            h[i] = 0.0
    return True


def _ds_active_set_rows(G, r, lo, hi, A_eq, b_eq, A_in, b_in, stats=None):
    """The direction QP of directed search with constraint rows, min 1/2 ||G d - r||^2 over lo <= d <= hi, G d <= 0, A_eq d = b_eq,
    A_in d <= b_in (descent.jl:196-236, :598-645), by the active-set method of `_ds_active_set` generalised as ds_qp_rows.hip runs it
    (DESIGN.md section 23).  W = [G; A_eq; A_in] (K rows), c = W d, h = (0, b_eq, b_in).  The step is p_N = W_N' a with a supported on
    the universe U = (objective rows) + S: the k x k work of `_ds_active_set` runs on M[U, U], the rows of S move to their right-hand
    side (dc_S = h_S - c_S), the objective rows outside S towards rho = r - z.  Equality rows start in S and are never dropped; one
    that the factorisation leaves out as dependent on the free variables blocks any step that would move it (either sign) and joins
    S again through the ratio test, as a row of the other kinds does, so that multipliers and steps always belong to one working set.
    Without constraint rows every operation is `_ds_active_set`'s: the same bits.  Returns (d, c, omega, mu, status); c and mu have K
    entries, objective rows first."""
    G = np.asarray(G, dtype=np.float64)
    k, n = G.shape
    r = np.asarray(r, dtype=np.float64)
    A_eq = np.zeros((0, n)) if A_eq is None or np.asarray(b_eq).size == 0 else np.asarray(A_eq, dtype=np.float64).reshape(-1, n)
    A_in = np.zeros((0, n)) if A_in is None or np.asarray(b_in).size == 0 else np.asarray(A_in, dtype=np.float64).reshape(-1, n)
    m_eq, m_in = A_eq.shape[0], A_in.shape[0]
    K = k + m_eq + m_in
    W = G if K == k else np.vstack([G, A_eq, A_in])
    h = np.zeros(K)
    if m_eq:
        h[k:k + m_eq] = np.asarray(b_eq, dtype=np.float64).ravel()
    if m_in:
        h[k + m_eq:] = np.asarray(b_in, dtype=np.float64).ravel()
    is_eq = np.zeros(K, dtype=bool)
    is_eq[k:k + m_eq] = True
    rext = np.zeros(K)
    rext[:k] = r

    def ended(status, why=None):
        if stats is not None and why is not None:
            stats["gave_up"] = why
        return np.full(n, np.nan), np.full(K, np.nan), np.nan, np.full(K, np.nan), status

    if not np.all(r < 0):     # some r_i >= 0, or a NaN (descent.jl:615-617)
        return np.zeros(n), np.zeros(K), 0.0, np.zeros(K), _lib.DS_CRITICAL
    if not np.all(lo <= hi):
        return np.zeros(n), np.zeros(K), -np.inf, np.zeros(K), _lib.DS_INFEASIBLE
    if not (np.all(lo <= 0.0) and np.all(hi >= 0.0)):
        return ended(_lib.DS_GAVE_UP, "start")   # the start d = 0 is outside the box: x is outside [lb, ub] by less than one
    if not _ds_rows_start(W, k, m_eq, h):
        return ended(_lib.DS_NO_START)           # the start d = 0 misses a constraint row: the method has no phase 1
    absW = np.abs(W)
    rowsum = absW.sum(axis=1)
    rscale = rowsum + np.abs(rext) + np.abs(h)
    d = np.zeros(n)
    flag = np.where(lo == hi, 2, np.where(lo == 0.0, -1, np.where(hi == 0.0, 1, 0)))
    in_s = is_eq.copy()
    degen = False
    free = flag == 0
    M = W[:, free] @ W[:, free].T
    cap = 8 * (n + K) + 16
    iters = dropped = full = 0
    mu = np.zeros(K)
    while True:
        if iters >= cap:
            return ended(_lib.DS_GAVE_UP, "cap")
        iters += 1
        c = W @ d
        rho = rext - c
        rho[k:] = 0.0
        U = np.flatnonzero(in_s | (np.arange(K) < k))
        MU = M if U.size == K else M[np.ix_(U, U)]
        s_u = in_s[U]
        av_u, fac = _ds_step_coeffs(MU, s_u, (c - h)[U], rho[U], int(np.count_nonzero(flag == 0)) if K > k else None)
        in_s[U] = s_u
        if av_u is None:
            return ended(_lib.DS_GAVE_UP, "normal equations")
        av = np.zeros(K)
        av[U] = av_u
        free = flag == 0
        p = np.where(free, W.T @ av, 0.0)
        dc = W @ p
        if full >= 2 or np.all(np.abs(dc) <= DS_VANISH_TOL * rscale):
            mu = np.zeros(K)
            mu[U] = _ds_multipliers(MU, fac, rho[U])
            y = mu - rho
            s = W.T @ y
            zext = np.where(np.arange(K) < k, c, 0.0)
            ysc = np.abs(rext) + np.abs(zext) + np.abs(mu)            # |r| + |z| + |mu| on objective rows, |mu| on the others
            sscale = absW.T @ ysc
            mscale = float(np.max(np.abs(r) + np.abs(c[:k])))
            best, kind, idx = 0.0, 0, -1
            for i in range(K):
                v = -mu[i] / mscale if in_s[i] and not is_eq[i] else 0.0
                if v > DS_DUAL_TOL and v > best and not (degen and kind):
                    best, kind, idx = v, 1, i
            viol = np.where(flag == -1, -s, np.where(flag == 1, s, 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(sscale > 0, viol / sscale, 0.0)
            if degen:             # the least index that violates; a row goes first
                cand = np.flatnonzero(ratio > DS_DUAL_TOL)
                j = int(cand[0]) if cand.size and not kind else -1
            else:
                j = int(np.argmax(ratio)) if n else -1
            if j >= 0 and ratio[j] > DS_DUAL_TOL and (degen or ratio[j] > best):
                best, kind, idx = float(ratio[j]), 2, j
            if kind == 0:
                break
            dropped += 1
            full = 0
            if kind == 1:
                in_s[idx] = False
            else:
                flag[idx] = 0
                fr = flag == 0
                M = W[:, fr] @ W[:, fr].T
            continue
        # ---- ratio test over the free variables' bounds and the rows outside S (an equality row there blocks on either side)
        with np.errstate(divide="ignore", invalid="ignore"):
            av_j = np.where(free & (p < 0), (lo - d) / p, np.where(free & (p > 0), (hi - d) / p, np.inf))
        av_j = np.where(av_j < 0, 0.0, av_j)
        alpha = 1.0
        if n:
            alpha = min(alpha, float(av_j.min()))
        ar = np.full(K, np.inf)
        for i in range(K):
            if not in_s[i] and (abs(dc[i]) if is_eq[i] else dc[i]) > DS_VANISH_TOL * rscale[i]:
                ar[i] = max(0.0, (h[i] - c[i]) / dc[i])
        alpha = min(alpha, float(ar.min()))
        hit = free & (av_j <= alpha)
        rows_hit = ar <= alpha
        degen = not alpha > 0.0
        if degen:                 # a step of length zero adds one constraint: the least index that blocks, a row first
            first_row = np.flatnonzero(rows_hit)
            rows_hit = np.zeros(K, dtype=bool)
            if first_row.size:
                rows_hit[first_row[0]] = True
                hit = np.zeros(n, dtype=bool)
            else:
                first = int(np.argmax(hit))
                hit = np.zeros(n, dtype=bool)
                hit[first] = True
        d = np.where(free, np.minimum(np.maximum(d + alpha * p, lo), hi), d)
        d = np.where(hit, np.where(p < 0, lo, hi), d)
        flag = np.where(hit, np.where(p < 0, -1, 1), flag)
        in_s |= rows_hit
        nh = int(hit.sum())
        full = full + 1 if (nh == 0 and not rows_hit.any()) else 0
        if nh >= 1:           # M from W whenever N changes: a rank-one downdate would cancel against the columns that have left
            fr = flag == 0
            M = W[:, fr] @ W[:, fr].T
    c = W @ d
    miss = np.where(is_eq, np.abs(c - h), c - h)
    if not np.all(miss <= DS_FEAS_TOL * (rowsum + np.abs(h))):
        return ended(_lib.DS_GAVE_UP, "rows")
    if stats is not None:
        stats["iterations"], stats["dropped"] = iters, dropped
    return d, c, max(0.0, -float(np.max(c[:k]))), mu, _lib.DS_OK


def _ds_slsqp(G, r, lo, hi, A_eq, b_eq, A_in, b_in):
    """the same QP, extended by rows A_eq d = b_eq and A_in d <= b_in, with SciPy's SLSQP from d = 0; None where it fails"""
    from scipy.optimize import minimize

    n = G.shape[1]
    cons = [{"type": "ineq", "fun": lambda v: -(G @ v), "jac": lambda v: -G}]
    if b_eq.size:
        cons.append({"type": "eq", "fun": lambda v: A_eq @ v - b_eq, "jac": lambda v: A_eq})
    if b_in.size:
        cons.append({"type": "ineq", "fun": lambda v: b_in - A_in @ v, "jac": lambda v: -A_in})
    res = minimize(lambda v: 0.5 * float(np.sum((G @ v - r) ** 2)), np.zeros(n), jac=lambda v: G.T @ (G @ v - r),
                   bounds=list(zip(lo, hi)), constraints=cons, method="SLSQP", options={"ftol": 1e-15, "maxiter": 1000})
    # status 8 ("positive directional derivative for linesearch") is SLSQP's usual end at a tight ftol: the point is judged by its rows
    if res.status not in (0, 8) or not np.all(np.isfinite(res.x)):
        return None
    d = np.clip(res.x, lo, hi)
    tol = 1e-9
    ok = np.all(G @ d <= tol * (1.0 + np.abs(G).sum(axis=1)))
    if b_eq.size:
        ok = ok and np.all(np.abs(A_eq @ d - b_eq) <= tol * (1.0 + np.abs(b_eq) + np.abs(A_eq).sum(axis=1)))
    if b_in.size:
        ok = ok and np.all(A_in @ d - b_in <= tol * (1.0 + np.abs(b_in) + np.abs(A_in).sum(axis=1)))
    return d if ok else None


def _directed_search_direction(x, G, r, lb, ub, A_eq=None, b_eq=None, A_ineq=None, b_ineq=None, stats=None):
    """The host method of the directed-search direction (descent.jl:598-645): min 1/2 ||G d - r||^2 over the box of `_sd_box`,
    G d <= 0.  Without further rows it runs the device kernel's active-set method in NumPy (`_ds_active_set`); with rows
    A_eq d = b_eq, A_ineq d <= b_ineq (those of `_sd_host_rows`) -- and where the active-set method gives up -- SciPy's SLSQP solves the
    extended QP.  Returns (d, z = G d, omega = max(0, -max z), mu, status MRBF_DS_*): mu are the multipliers of G d <= 0 from the
    active-set method, NaN from SLSQP; CRITICAL and INFEASIBLE as mrbf_ds_direction answers them.  stats["method"]: which one ran."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    G = np.asarray(G, dtype=np.float64).reshape(-1, n)
    k = G.shape[0]
    r = np.asarray(r, dtype=np.float64).ravel()
    lo, hi = _sd_box(x, lb, ub)
    A_eq = np.zeros((0, n)) if b_eq is None or np.asarray(b_eq).size == 0 else np.asarray(A_eq, dtype=np.float64).reshape(-1, n)
    b_eq = np.zeros(0) if b_eq is None else np.asarray(b_eq, dtype=np.float64).ravel()
    A_in = np.zeros((0, n)) if b_ineq is None or np.asarray(b_ineq).size == 0 else np.asarray(A_ineq, dtype=np.float64).reshape(-1, n)
    b_in = np.zeros(0) if b_ineq is None else np.asarray(b_ineq, dtype=np.float64).ravel()
    if not (b_eq.size or b_in.size):
        out = _ds_active_set(G, r, lo, hi, stats)
        if stats is not None:
            stats["method"] = "active_set"
        if out[4] != _lib.DS_GAVE_UP:
            return out
    elif not np.all(r < 0):
        return np.zeros(n), np.zeros(k), 0.0, np.zeros(k), _lib.DS_CRITICAL
    elif not np.all(lo <= hi):
        return np.zeros(n), np.zeros(k), -np.inf, np.zeros(k), _lib.DS_INFEASIBLE
    if stats is not None:
        stats["method"] = "slsqp"
    d = _ds_slsqp(G, r, lo, hi, A_eq, b_eq, A_in, b_in)
    if d is None:
        return np.full(n, np.nan), np.full(k, np.nan), np.nan, np.full(k, np.nan), _lib.DS_GAVE_UP
    z = G @ d
    return d, z, max(0.0, -float(np.max(z))), np.full(k, np.nan), _lib.DS_OK


def ds_directions_many(G, r, X, lb, ub, ctx=None, want_mult=True):
    """one mrbf_ds_direction call for a batch of starts: G (n_qp x k x d, the starts' objective Jacobians), r (n_qp x k), X (n_qp x d),
    lb / ub (d, or n_qp x d).  Returns (rc, d (n_qp x d), z (n_qp x k), omega (n_qp), mu (n_qp x k) or None, status (n_qp),
    iters (n_qp x 2: iterations, constraints dropped))."""
    ctx = ctx or _lib.default_context()
    G = np.asarray(G, dtype=np.float64)
    nq, k, n = G.shape
    Gl = np.ascontiguousarray(np.transpose(G, (0, 2, 1)))      # mrbf_eval's jac_out layout: k x d column-major per start
    r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(nq, k))
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(nq, n))
    lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, dtype=np.float64), (nq, n)))
    ub = np.ascontiguousarray(np.broadcast_to(np.asarray(ub, dtype=np.float64), (nq, n)))
    d, z, om = np.empty((nq, n)), np.empty((nq, k)), np.empty(nq)
    mu = np.empty((nq, k)) if want_mult else None
    status, iters = np.empty(nq, dtype=np.int32), np.empty((nq, 2), dtype=np.int32)
    rc = ctx.lib.mrbf_ds_direction(ctx.h, nq, n, k, _lib.as_ptr(Gl), _lib.as_ptr(r), _lib.as_ptr(X), _lib.as_ptr(lb), _lib.as_ptr(ub),
                                   _lib.as_ptr(d), _lib.as_ptr(z), _lib.as_ptr(om), _lib.as_ptr(mu), _lib.as_ptr(status), _lib.as_ptr(iters))
    return rc, d, z, om, mu, status, iters


def ds_criticality_device(plan, x_n, lb, ub, r, want_mult=False):
    """one mrbf_ds_criticality call; returns (rc, omega, d, info dict[, multipliers])"""
    ctx = plan["models"][0].ctx
    x_n = np.ascontiguousarray(x_n, dtype=np.float64)
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64)
    prob, keep = _sd_problem(plan, (None,) * 4)
    d = np.empty(x_n.size)
    mu = np.empty(plan["k"]) if want_mult else None
    info = _lib.DsInfo()
    rc = ctx.lib.mrbf_ds_criticality(ctx.h, ctypes.byref(prob), _lib.as_ptr(x_n), _lib.as_ptr(lb), _lib.as_ptr(ub), _lib.as_ptr(r),
                                     _lib.as_ptr(d), _lib.as_ptr(mu), ctypes.byref(info))
    out = (rc, float(info.omega), d, info.asdict())
    return out + (mu,) if want_mult else out


def ds_directions_rows_many(G, r, X, lb, ub, A_eq=None, b_eq=None, A_in=None, b_in=None, ctx=None, want_mult=True, want_iters=True):
    """one mrbf_ds_direction_rows call for a batch of starts: G (n_qp x k x d), r (n_qp x k), X (n_qp x d), lb / ub (d, or n_qp x d),
    A_eq (n_qp x m_eq x d) with b_eq (n_qp x m_eq), A_in (n_qp x m_in x d) with b_in (n_qp x m_in); None where there are no such rows.
    Returns (rc, d (n_qp x d), c (n_qp x K: W d, objective rows first), omega (n_qp), mu (n_qp x K) or None, status (n_qp),
    iters (n_qp x 2: iterations, constraints dropped) or None)."""
    ctx = ctx or _lib.default_context()
    G = np.asarray(G, dtype=np.float64)
    nq, k, n = G.shape
    Gl = np.ascontiguousarray(np.transpose(G, (0, 2, 1)))      # mrbf_eval's jac_out layout: k x d column-major per start
    r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(nq, k))
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(nq, n))
    lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, dtype=np.float64), (nq, n)))
    ub = np.ascontiguousarray(np.broadcast_to(np.asarray(ub, dtype=np.float64), (nq, n)))

    def rows(A, b):
        if b is None or np.asarray(b).size == 0:
            return 0, None, None
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(nq, -1))
        return b.shape[1], np.ascontiguousarray(np.asarray(A, dtype=np.float64).reshape(nq, b.shape[1], n)), b

    m_eq, A_eq, b_eq = rows(A_eq, b_eq)
    m_in, A_in, b_in = rows(A_in, b_in)
    K = k + m_eq + m_in
    d, c, om = np.empty((nq, n)), np.empty((nq, K)), np.empty(nq)
    mu = np.empty((nq, K)) if want_mult else None
    status = np.empty(nq, dtype=np.int32)
    iters = np.empty((nq, 2), dtype=np.int32) if want_iters else None
    rc = ctx.lib.mrbf_ds_direction_rows(ctx.h, nq, n, k, m_eq, m_in, _lib.as_ptr(Gl), _lib.as_ptr(r), _lib.as_ptr(X), _lib.as_ptr(lb),
                                        _lib.as_ptr(ub), _lib.as_ptr(A_eq), _lib.as_ptr(b_eq), _lib.as_ptr(A_in), _lib.as_ptr(b_in),
                                        _lib.as_ptr(d), _lib.as_ptr(c), _lib.as_ptr(om), _lib.as_ptr(mu), _lib.as_ptr(status),
                                        _lib.as_ptr(iters))
    return rc, d, c, om, mu, status, iters


def ds_criticality_rows_device(plan, x, x_n, lb, ub, r, lin=None, want_mult=False):
    """one mrbf_ds_criticality_rows call; returns (rc, omega, d, info dict[, multipliers of the K rows])"""
    ctx = plan["models"][0].ctx
    x, x_n = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(x_n, dtype=np.float64)
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64)
    prob, keep = _sd_problem(plan, lin or (None,) * 4)
    m = plan["k"] + plan["n_con"] + sum(0 if b is None else b.size for b in (keep[3], keep[5]))
    d = np.empty(x_n.size)
    mu = np.empty(m) if want_mult else None
    info = _lib.DsInfo()
    rc = ctx.lib.mrbf_ds_criticality_rows(ctx.h, ctypes.byref(prob), _lib.as_ptr(x), _lib.as_ptr(x_n), _lib.as_ptr(lb), _lib.as_ptr(ub),
                                          _lib.as_ptr(r), _lib.as_ptr(d), _lib.as_ptr(mu), ctypes.byref(info))
    out = (rc, float(info.omega), d, info.asdict())
    return out + (mu,) if want_mult else out


def _ds_image_direction(cfg, sc, scal, x, x_n, fx_n, delta, lb, ub, rng, stats, seed=0):
    """r of descent.jl:599-611, the target change of the model values: minus the reference direction, or the reference point minus
    f(x_n), or the local ideal point (descent.jl:404-412, over the trust region stretched by reference_trust_region_factor) minus f(x_n).
    The ideal point is the host search's, or with cfg.ideal_point == "device" the device call's (mrbf_ideal_point_problem with `seed`;
    the box only, as the host search: constraints are not carried); stats["ideal_point_path"] says which ("device" or "reference")."""
    from . import pascoletti_serafini as ps

    fx_n = np.asarray(fx_n, dtype=np.float64)
    g = ps._get_global_dir(cfg, fx_n)
    if g is not None:
        return -g
    n = int(np.asarray(x_n).size)
    lb_eff, ub_eff = _local_bounds(x, cfg.reference_trust_region_factor * delta, lb, ub)
    if cfg.ideal_point == "device":
        st = {}
        ideal = ps.compute_local_ideal_points_many(cfg, [sc], np.asarray(x_n, dtype=np.float64)[None, :], lb_eff[None, :], ub_eff[None, :],
                                                   seeds=[seed], carry_constraints=False, stats=st, scal=scal)[0]
        if stats is not None:
            stats["ideal_point_path"] = "reference" if st["path"] == "reference" else "device"
        return ideal - fx_n
    if stats is not None:
        stats["ideal_point_path"] = "reference"
    max_evals = 500 * (n + 1) if cfg.max_ideal_point_problem_evals < 0 else cfg.max_ideal_point_problem_evals
    rng = np.random.default_rng(0) if rng is None else rng
    ideal = ps.compute_local_ideal_point(np.asarray(x_n, dtype=np.float64), lb_eff, ub_eff,
                                         lambda X: sg.eval_container_objectives_at_scaled_sites(sc, scal, X), fx_n.size, max_evals, rng,
                                         stats=stats)
    return ideal - fx_n


def _ds_normalise(omega, d, status, n):
    """what the step is given of a direction QP's (omega, d, status) (descent.jl:647-660): (omega, d / ||d||_inf), or (0, zeros) when
    the status is not OK or ||d||_inf = 0 -- the rule ds_scale_kernel applies on the device for mrbf_ds_iterate_batch"""
    nrm = float(np.max(np.abs(d))) if status == _lib.DS_OK and d.size else 0.0
    if status != _lib.DS_OK or not nrm > 0:
        return 0.0, np.zeros(n)
    return float(omega), d / nrm


def get_criticality_ds(cfg, sc, scal, x, x_n, fx_n, delta, lb, ub, lin=None, stats=None, rng=None, r=None, seed=0):
    """The criticality of directed search (descent.jl:583-660 up to the backtracking) as HipRbf.jl's `hip_get_criticality_ds` routes it:
    the image direction r from the configuration (`_get_global_dir` / `compute_local_ideal_point`), then mrbf_dispatch_ds decides,
    mrbf_ds_criticality solves the direction QP on the device (with cfg.constraint_rows == "device" and constraint rows:
    mrbf_dispatch_ds_rows and mrbf_ds_criticality_rows), and where the decision table or mrbf_dispatch_after say so the host
    method runs (`_directed_search_direction` on container Jacobians, with the rows of `_sd_host_rows` where the container or the
    problem has constraints).  lb / ub: the global bounds in scaled variables; lin = (A_eq, b_eq, A_ineq, b_ineq) in scaled variables.
    Never raises on a size limit.  r: a precomputed image direction (ds_iterate_many computes it for all starts at once); seed keys
    the device ideal-point search (cfg.ideal_point == "device").  Returns (omega, d / ||d||_inf), or (0, zeros) when critical or
    ||d||_inf = 0 (descent.jl:647-660); stats["path"] is "device" or "reference"."""
    lib = _lib.load()
    plan = sg.container_plan(sc)
    x_n = np.asarray(x_n, dtype=np.float64)
    n = int(x_n.size)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))
    if r is None:
        r = _ds_image_direction(cfg, sc, scal, x, x_n, fx_n, delta, lb, ub, rng, stats, seed=seed)
    r = np.asarray(r, dtype=np.float64)

    def result(omega, d, status):
        return _ds_normalise(omega, d, status, n)

    if (cfg.constraint_rows == "device" and (n_lin or plan["n_con"]) and
            lib.mrbf_dispatch_ds_rows(n, plan["k"], len(plan["models"]), plan["n_con"], n_lin, plan["n_foreign"]) == _lib.DISPATCH_DEVICE):
        rc, omega, d, info = ds_criticality_rows_device(plan, x, x_n, lb, ub, r, lin)
        if stats is not None:
            stats.update(info)
            stats["path"] = "device"
        if rc == 0:
            return result(omega, d, info["status"])
        if not lib.mrbf_dispatch_after(_lib.ENTRY_DS_ROWS, rc):     # -2: the QP gave up, or d = 0 misses a row (stats["status"])
            plan["models"][0].ctx.check(rc)
    elif lib.mrbf_dispatch_ds(n, plan["k"], len(plan["models"]), plan["n_con"], n_lin, plan["n_foreign"]) == _lib.DISPATCH_DEVICE:
        rc, omega, d, info = ds_criticality_device(plan, x_n, lb, ub, r)
        if stats is not None:
            stats.update(info)
            stats["path"] = "device"
        if rc == 0:
            return result(omega, d, info["status"])
        if not lib.mrbf_dispatch_after(_lib.ENTRY_DS, rc):
            plan["models"][0].ctx.check(rc)
    if stats is not None:
        stats["path"] = "reference"
    if n_lin or plan["n_con"]:
        G, A_eq, b_eq, A_in, b_in = _sd_host_rows(sc, scal, x, x_n, lin)
    else:
        G, A_eq, b_eq, A_in, b_in = sg.eval_container_objectives_jacobian_at_scaled_site(sc, scal, x_n), None, None, None, None
    d, _, omega, _, status = _directed_search_direction(x_n, G, r, lb, ub, A_eq, b_eq, A_in, b_in, stats)
    return result(omega, d, status)


def compute_descent_step_ds(cfg, sc, scal, x, x_n, delta, lb, ub, omega, d, lin=None, stats=None):
    """the step of directed search (descent.jl:645-660): what the parked code does with its direction is `_intersect_bounds` and the
    Armijo sweep -- `compute_descent_step_sd_routed` on (omega, d) of `get_criticality_ds`, no step code of its own.  Returns
    (omega, x_plus, mx_plus, ||step||_inf)."""
    return compute_descent_step_sd_routed(cfg, sc, scal, x, x_n, delta, lb, ub, omega, d, lin, stats)


# ---- many starts in one device call (mrbf_ds_iterate_batch): the reference's Threads.@threads loop over starts ---------------------
def ds_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, R, out=None):
    """one mrbf_ds_iterate_batch call on the containers' plans (one shape, checked by the caller); X, X_n (n_starts x d), deltas, lb,
    ub, R (n_starts x k: the image direction per start) may be NumPy arrays or device tensors; out = (d, x_plus, mx_plus, mu) lets the
    caller pass its own output buffers (host or device).  Returns (rc, d, x_plus, mx_plus, mu, list of record dicts with "branch_name",
    event ms)."""
    ctx = plans[0]["models"][0].ctx
    ns, k = len(plans), plans[0]["k"]
    X, X_n, deltas, lb, ub, R = _arr(X), _arr(X_n), _arr(deltas), _arr(lb), _arr(ub), _arr(R)
    n = int(lb.numel() if hasattr(lb, "numel") else lb.size)
    prob, keep = _sd_problem(plans[0], (None,) * 4)
    handles = _handles(plans)
    dd, xp, mxp, mu = out if out is not None else (np.empty((ns, n)), np.empty((ns, n)), np.empty((ns, k)), np.empty((ns, k)))
    opts = _step_options(cfg)
    recs = (_lib.DsBatchRecord * ns)()
    ms = ctypes.c_float()
    rc = ctx.lib.mrbf_ds_iterate_batch(ctx.h, ns, ctypes.byref(prob), handles, _lib.as_ptr(X), _lib.as_ptr(X_n), _lib.as_ptr(deltas),
                                       _lib.as_ptr(lb), _lib.as_ptr(ub), _lib.as_ptr(R), ctypes.byref(opts), _lib.as_ptr(dd),
                                       _lib.as_ptr(xp), _lib.as_ptr(mxp), _lib.as_ptr(mu), recs, ctypes.byref(ms))
    records = []
    for r in recs:
        rd = r.asdict()
        rd["branch_name"] = _SD_BRANCHES[r.branch] if rc == 0 and 0 <= r.branch < 3 else None
        records.append(rd)
    return rc, dd, xp, mxp, mu, records, ms.value


def ds_iterate_many(cfg, containers, scal, X, X_n, FX_n, deltas, lb, ub, lin=None, stats=None, rng=None, seeds=None):
    """`get_criticality_ds` then `compute_descent_step_ds` (descent.jl:583-664) for many independent starts of one problem -- the
    reference's `Threads.@threads` loop over starts (examples/large_scale_benchmarks.jl:102-109): containers[p] is start p's surrogate
    container, X[p] / X_n[p] / FX_n[p] / deltas[p] its iterate, normal-step iterate, values there and radius; lb / ub and lin belong to
    the one MOP.  The image direction r comes per start from `_ds_image_direction`: arithmetic with a reference direction or point,
    else the per-start ideal-point search (stats["image_direction"] says which: "reference_direction", "reference_point" or
    "ideal_point").  With cfg.ideal_point == "device" and that last mode, the ideal points of ALL starts come from one
    `compute_local_ideal_points_many` call before anything else (seeds[p] keys start p's search, None: 0 for every start;
    stats["ideal_point_path"] is "device", or "reference" where that call took the host search), and every start is handed its r, the
    ones that take the single-start functions too: a homogeneous unconstrained batch of at least ps.IDEAL_BATCH_MIN_STARTS starts makes
    two device calls whatever the number of starts.  Where the containers share one plan shape and mrbf_dispatch_ds_batch says so,
    ONE mrbf_ds_iterate_batch call serves all starts ("batch"); otherwise (a refused shape, constraints, mixed shapes), and for every start whose direction QP gave up, the
    routed single-start functions run.  Returns a list of (omega, d, x_plus, mx_plus, ||step||_inf); stats gets "path" ("batch" or
    "loop"), "rerouted" (the starts that took the single-start functions after a batch call), "records" and "ms_total"."""
    lib = _lib.load()
    X, X_n = np.asarray(X, dtype=np.float64), np.asarray(X_n, dtype=np.float64)
    FX_n = np.asarray(FX_n, dtype=np.float64)
    deltas = np.asarray(deltas, dtype=np.float64).ravel()
    ns = len(containers)
    lin = lin or (None,) * 4
    n_lin = sum(0 if b is None else int(np.asarray(b).size) for b in (lin[1], lin[3]))

    R_dev = None  # the image directions of all starts, where the device finds the ideal points

    def single(p):
        if R_dev is None:
            omega, d = get_criticality_ds(cfg, containers[p], scal, X[p], X_n[p], FX_n[p], float(deltas[p]), lb, ub, lin, rng=rng)
        else:
            omega, d = get_criticality_ds(cfg, containers[p], scal, X[p], X_n[p], FX_n[p], float(deltas[p]), lb, ub, lin, rng=rng, r=R_dev[p])
        om, xp, mxp, nrm = compute_descent_step_ds(cfg, containers[p], scal, X[p], X_n[p], float(deltas[p]), lb, ub, omega, d, lin)
        return om, d, xp, mxp, nrm

    if stats is not None:
        stats["path"], stats["rerouted"] = "loop", []
        stats["image_direction"] = ("reference_direction" if len(cfg.reference_direction)        # the order of ps._get_global_dir
                                    else "reference_point" if len(cfg.reference_point) else "ideal_point")
    if ns == 0:
        return []
    if cfg.ideal_point == "device" and not len(cfg.reference_direction) and not len(cfg.reference_point):
        from . import pascoletti_serafini as ps

        boxes = [_local_bounds(X[p], cfg.reference_trust_region_factor * float(deltas[p]), lb, ub) for p in range(ns)]
        st = {}
        ideal = ps.compute_local_ideal_points_many(cfg, containers, X_n, np.stack([b[0] for b in boxes]), np.stack([b[1] for b in boxes]),
                                                   seeds=seeds, carry_constraints=False, stats=st, scal=scal)
        R_dev = ideal - FX_n
        if stats is not None:
            stats["ideal_point_path"] = "reference" if st["path"] == "reference" else "device"
            stats["ideal_point_stats"] = st
    elif stats is not None and not len(cfg.reference_direction) and not len(cfg.reference_point):
        stats["ideal_point_path"] = "reference"
    plans = [sg.container_plan(sc) for sc in containers]
    n = int(X_n.shape[1])
    p0 = plans[0]
    if _same_plan_shape(plans) and lib.mrbf_dispatch_ds_batch(ns, n, p0["k"], len(p0["models"]), p0["n_con"], n_lin, p0["n_foreign"],
                                                              int(cfg.max_loops)) == _lib.DISPATCH_DEVICE:
        R = R_dev if R_dev is not None else np.stack(
            [_ds_image_direction(cfg, containers[p], scal, X[p], X_n[p], FX_n[p], float(deltas[p]), lb, ub, rng, None) for p in range(ns)])
        rc, dd, xp, mxp, mu, records, ms = ds_iterate_batch_device(plans, cfg, X, X_n, deltas, lb, ub, R)
        if rc == 0:
            res, rerouted = [], []
            for p, r in enumerate(records):
                if r["ds_status"] == _lib.DS_GAVE_UP:          # this start's QP gave up: the host method for it alone
                    rerouted.append(p)
                    res.append(single(p))
                elif not r["sigma"] > cfg.min_stepsize:        # descent.jl:317: the reference returns integer zeros here
                    res.append((0, dd[p].copy(), xp[p].copy(), mxp[p].copy(), 0))
                else:
                    res.append((r["omega_step"], dd[p].copy(), xp[p].copy(), mxp[p].copy(), r["step_norm"]))
            if stats is not None:
                stats.update(path="batch", rerouted=rerouted, records=records, ms_total=ms)
            return res
        if not lib.mrbf_dispatch_after(_lib.ENTRY_DS_BATCH, rc):
            p0["models"][0].ctx.check(rc)
    return [single(p) for p in range(ns)]
