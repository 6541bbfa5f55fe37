"""The return codes of the six descent entry points on a malformed container (run with -m gpu): mrbf_ps_step_problem,
mrbf_sd_criticality, mrbf_sd_step, mrbf_sd_iterate_batch, mrbf_normal_step, mrbf_normal_step_batch each get one defect at a time.
They read the roles table through one reader (csrc/descent_problem.hpp) and map its defect classes to their own codes: the single
calls and the PS step answer -2 throughout, the batches -3 for the table and the linear rows and -4 for the models -- the codes of
the entry points before they shared the reader, written here as literals.  mrbf_last_error starts with the entry point's name.  Every
case is refused before any launch; the two normal-step entries ignore objective rows and must still run a table whose objective
entries are malformed."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib

NONE, EQ, INEQ = -1, -2, -3
ENTRIES = ("ps_step", "sd_criticality", "sd_step", "sd_iterate_batch", "normal_step", "normal_step_batch")
BATCHES = ("sd_iterate_batch", "normal_step_batch")
NORMAL = ("normal_step", "normal_step_batch")
# the name in front of the messages (the PS step's messages say mrbf_ps_step)
PREFIX = dict(ps_step="mrbf_ps_step:", sd_criticality="mrbf_sd_criticality:", sd_step="mrbf_sd_step:",
              sd_iterate_batch="mrbf_sd_iterate_batch:", normal_step="mrbf_normal_step:", normal_step_batch="mrbf_normal_step_batch:")
# defect -> (code of the single calls and the PS step, code of the batches)
DEFECTS = {
    "objective_twice": (-2, -3),
    "objective_missing": (-2, -3),
    "role_is_n_objectives": (-2, -3),
    "role_minus_7": (-2, -3),
    "null_slot": (-2, -4),
    "slot_other_d": (-2, -4),
    "lin_eq_without_matrix": (-2, -3),
    "negative_lin_eq": (-2, -3),
    "second_start_other_k": (None, -4),
}
OBJECTIVE_DEFECTS = ("objective_twice", "objective_missing", "role_is_n_objectives")  # entries the normal step does not read


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(11)
    cfg = pkg.RbfConfig(kernel="cubic", polynomial_degree=1)

    def fit(d, k):
        C = rng.uniform(-1.0, 1.0, (6, d))
        return pkg.update_model(cfg, C, np.stack([np.sum((C - 0.3 * i) ** 2, axis=1) for i in range(k)], axis=1))

    M = dict(a=fit(2, 2), b=fit(2, 2), d3=fit(3, 2), k1=fit(2, 1))
    yield M
    for m in M.values():
        m.free()


def _handle(m):
    return None if m is None else (m.model.value if hasattr(m.model, "value") else m.model)


def _case(models, defect, n_starts):
    """(slots of every start, roles, n_objectives, n_lin_eq -- A_eq and b_eq are always NULL) of a good container [a: two objectives, b: an equality
    and an inequality row] with the one defect"""
    a, b = models["a"], models["b"]
    starts = [[a, b] for _ in range(n_starts)]
    roles, n_lin_eq = [0, 1, EQ, INEQ], 0
    if defect == "objective_twice":
        roles = [0, 0, EQ, INEQ]
    elif defect == "objective_missing":
        roles = [0, NONE, EQ, INEQ]
    elif defect == "role_is_n_objectives":
        roles = [0, 1, 2, INEQ]
    elif defect == "role_minus_7":
        roles = [0, 1, -7, INEQ]
    elif defect == "null_slot":
        starts[0][1] = None
    elif defect == "slot_other_d":
        starts[0][1] = models["d3"]
    elif defect == "lin_eq_without_matrix":
        n_lin_eq = 1
    elif defect == "negative_lin_eq":
        n_lin_eq = -1
    elif defect == "second_start_other_k":
        starts[1][1] = models["k1"]
    elif defect == "normal_runs":       # a doubled objective position and one valid constraint row
        roles = [0, 0, INEQ, NONE]
    else:
        assert defect == "good"
    return starts, roles, 2, n_lin_eq


def _call(models, entry, defect):
    """one call of the entry point; returns (rc, mrbf_last_error)"""
    n_starts = 2 if entry in BATCHES else 1
    starts, roles, k, n_lin_eq = _case(models, defect, n_starts)
    ctx = models["a"].ctx
    lib = ctx.lib
    d = 2
    single = (ctypes.c_void_p * 2)(*[_handle(m) for m in starts[0]])
    every = (ctypes.c_void_p * (2 * n_starts))(*[_handle(m) for s in starts for m in s])
    roles_c = (ctypes.c_int32 * len(roles))(*roles)
    prob = _lib.PsProblem(n_models=2, n_objectives=k, models=single, roles=roles_c, n_lin_eq=n_lin_eq, n_lin_ineq=0, A_eq=None, b_eq=None,
                          A_ineq=None, b_ineq=None, eq_tol=-1.0)
    x, x_n = np.zeros((n_starts, d)), np.full((n_starts, d), 0.05)
    lb, ub = np.full(d, -1.0), np.full(d, 1.0)
    deltas = np.full(n_starts, 0.5)
    dirn = np.full(d, -0.5)
    out_d, out_x, out_m, out_y = np.empty((n_starts, d)), np.empty((n_starts, d)), np.empty((n_starts, k)), np.empty((n_starts, 8))
    step_opts = _lib.SdStepOptions(strict=1, max_loops=5, const_rhs=1e-6, shrink=0.75, min_stepsize=1e-12)
    p = _lib.as_ptr
    if entry == "ps_step":
        opts = _lib.PsOptions(max_ideal_evals=40, max_ps_evals=40, max_polish_evals=0, reserved=0, seed=1, t0=-0.5, xtol_rel=1e-3)
        fx, r_out, info = np.zeros(k), np.empty(k), _lib.PsInfo()
        rc = lib.mrbf_ps_step_problem(ctx.h, ctypes.byref(prob), p(x_n), p(lb), p(ub), p(fx), None, ctypes.byref(opts), p(out_x), p(out_m),
                                      p(r_out), ctypes.byref(info))
    elif entry == "sd_criticality":
        info = _lib.SdInfo()
        rc = lib.mrbf_sd_criticality(ctx.h, ctypes.byref(prob), p(x), p(x_n), p(lb), p(ub), 1, p(out_d), None, ctypes.byref(info))
    elif entry == "sd_step":
        info = _lib.SdStepInfo()
        rc = lib.mrbf_sd_step(ctx.h, ctypes.byref(prob), p(x), p(x_n), 0.5, p(lb), p(ub), 0.1, p(dirn), ctypes.byref(step_opts), p(out_x),
                              p(out_m), ctypes.byref(info))
    elif entry == "sd_iterate_batch":
        recs, ms = (_lib.SdBatchRecord * n_starts)(), ctypes.c_float()
        rc = lib.mrbf_sd_iterate_batch(ctx.h, n_starts, ctypes.byref(prob), every, p(x), p(x_n), p(deltas), p(lb), p(ub), 1,
                                       ctypes.byref(step_opts), p(out_d), p(out_x), p(out_m), recs, ctypes.byref(ms))
    elif entry == "normal_step":
        info = _lib.NormalInfo()
        rc = lib.mrbf_normal_step(ctx.h, ctypes.byref(prob), d, p(x), p(lb), p(ub), 0.5, 1.0, np.inf, 0, p(out_d), p(out_y), ctypes.byref(info))
    else:
        recs, ms = (_lib.NormalBatchRecord * n_starts)(), ctypes.c_float()
        rc = lib.mrbf_normal_step_batch(ctx.h, n_starts, ctypes.byref(prob), every, d, p(x), p(lb), p(ub), p(deltas), 1.0, np.inf, 0, p(out_d),
                                        p(out_x), p(out_y), recs, ctypes.byref(ms))
    return rc, (lib.mrbf_last_error(ctx.h) or b"").decode()


CASES = [(e, f) for e in ENTRIES for f in DEFECTS
         if not (f == "second_start_other_k" and e not in BATCHES) and not (e in NORMAL and f in OBJECTIVE_DEFECTS)]


@pytest.mark.parametrize("entry,defect", CASES)
def test_defect_is_refused_with_the_entry_points_own_code(models, entry, defect):
    rc, msg = _call(models, entry, defect)
    print(entry, defect, rc, msg)
    assert rc == DEFECTS[defect][1 if entry in BATCHES else 0]
    assert msg.startswith(PREFIX[entry]), msg


@pytest.mark.parametrize("entry", NORMAL)
def test_normal_step_ignores_the_objective_rows(models, entry):
    rc, msg = _call(models, entry, "normal_runs")
    assert rc == 0, msg
