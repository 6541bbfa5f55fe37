"""ctypes binding of libmrbf.so (include/mrbf.h).  No CPU fallback: a missing library or GPU is an error."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRBF_LIB") or os.path.join(_HERE, "libmrbf.so")  # MRBF_LIB: same override as HipRbf.jl (A/B runs of two builds)

c_dp = ctypes.POINTER(ctypes.c_double)
c_fp = ctypes.POINTER(ctypes.c_float)
c_ip = ctypes.POINTER(ctypes.c_int32)
c_vp = ctypes.c_void_p

# error codes (mrbf.h)
MRBF_OK, MRBF_ENOTPD, MRBF_ESINGULAR, MRBF_EHIP, MRBF_EBLAS, MRBF_ENOMEM, MRBF_ENODEVICE, MRBF_ENCCL = range(8)
PATH_CHOL, PATH_PROJ_CHOL, PATH_LU, PATH_MINNORM, PATH_ROUND4 = 1, 2, 3, 4, 5
OPT_GRAM_MODE, OPT_RESIDUAL, OPT_FORCE_PATH, OPT_CHOL_IMPL, OPT_EVAL_IMPL, OPT_TIMING, OPT_DIAG_IMPL, OPT_CHOL_WINDOW = 1, 2, 3, 4, 5, 6, 7, 8
OPT_SPIN_MS, OPT_DEBUG_FAULT, OPT_LAST_DEVICE_MS, OPT_SLOW_LAUNCHES = 9, 10, 11, 12
OPT_ARENA_BYTES, OPT_LIVE_HANDLES = 13, 14   # read only
OPT_SMALL_FIT_MAX_N = 15                     # most sites the one-launch fit takes: 512 (default) .. 2048
SMALL_FIT_DEFAULT_MAX_N = 512
OPT_SMALL_LU = 16                            # 1: LU-path fits with n <= 512, d <= 128, k <= 16 take the one-launch LU (default 0)
SMALL_LU_MAX_N, SMALL_LU_MAX_D, SMALL_LU_MAX_K = 512, 128, 16
FB_CHOL_HOST_DRIVEN, FB_BACKSOLVE_BLOCKED, FB_LU = 1, 2, 4


class FitInfo(ctypes.Structure):
    _fields_ = [("path", ctypes.c_int32), ("factor_info", ctypes.c_int32), ("n", ctypes.c_int32), ("q", ctypes.c_int32),
                ("rel_residual", ctypes.c_double), ("max_pitw", ctypes.c_double), ("mu", ctypes.c_double),
                ("ms_gram", ctypes.c_float), ("ms_project", ctypes.c_float), ("ms_factor", ctypes.c_float),
                ("ms_solve", ctypes.c_float), ("ms_check", ctypes.c_float), ("ms_total", ctypes.c_float),
                ("fallbacks", ctypes.c_int32), ("giveup_code", ctypes.c_int32), ("ms_factor_device", ctypes.c_float),
                ("slow_launches", ctypes.c_int32)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class EvalInfo(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_float), ("ms_dist", ctypes.c_float), ("ms_kernel", ctypes.c_float),
                ("ms_contract", ctypes.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class HessInfo(ctypes.Structure):
    """mrbf_hess_info: what mrbf_eval_hessian reports"""
    _fields_ = [("ms_total", ctypes.c_float), ("nsplit", ctypes.c_int32), ("chunks", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class HessJob(ctypes.Structure):
    """mrbf_hess_job: one (model, site block) pair of mrbf_eval_hessian_batch"""
    _fields_ = [("model", ctypes.c_void_p), ("m", ctypes.c_int64), ("X", ctypes.c_void_p), ("rows", ctypes.c_void_p),
                ("hess_out", ctypes.c_void_p), ("n_rows", ctypes.c_int32), ("status", ctypes.c_int32), ("nsplit", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class HessBatchInfo(ctypes.Structure):
    """mrbf_hess_batch_info: what mrbf_eval_hessian_batch reports"""
    _fields_ = [("ms_total", ctypes.c_float), ("chunks", ctypes.c_int32), ("groups", ctypes.c_int32), ("single_inside", ctypes.c_int32)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PsOptions(ctypes.Structure):
    _fields_ = [("max_ideal_evals", ctypes.c_int32), ("max_ps_evals", ctypes.c_int32), ("max_polish_evals", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64), ("t0", ctypes.c_double), ("xtol_rel", ctypes.c_double)]


class PsInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("generations", ctypes.c_int32), ("evals_ideal", ctypes.c_int32),
                ("evals_ps", ctypes.c_int32), ("evals_polish", ctypes.c_int32), ("ms_total", ctypes.c_float), ("tau", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


PS_OK, PS_CRITICAL, PS_FAILURE = 0, 1, 2
ROLE_NONE, ROLE_EQ, ROLE_INEQ = -1, -2, -3
DISPATCH_REFERENCE, DISPATCH_DEVICE = 0, 1
FIT_FULL, FIT_FROM_ROUND4 = 0, 1
ENTRY_ROUND4, ENTRY_FIT_FROM_ROUND4, ENTRY_PS_STEP, ENTRY_BACKTRACK, ENTRY_AFFINE, ENTRY_SD, ENTRY_NORMAL, ENTRY_SD_STEP = 1, 2, 3, 4, 5, 6, 7, 8
ENTRY_SD_BATCH = 9
ENTRY_AFFINE_BATCH = 10
ENTRY_FIT_BATCH = 11
ENTRY_NORMAL_BATCH = 12
ENTRY_ROUND4_BATCH = 13
ENTRY_PS_BATCH = 14
ENTRY_DB_BOX = 15
ENTRY_DB_GATHER = 16
ENTRY_DB_ROUND3 = 17
ENTRY_DB_APPEND_BATCH = 18
ENTRY_DB_SET_VALUES_BATCH = 19
ENTRY_EVAL_BATCH = 20
ENTRY_HESSIAN_BATCH = 21
ENTRY_DS = 22
ENTRY_DS_BATCH = 23
ENTRY_DS_ROWS = 24
ENTRY_IDEAL = 25
ENTRY_IDEAL_BATCH = 26
R3_UPDATE, R3_IMPROVE = 0, 1
R3_DONE, R3_REBUILT = 0, 1
SD_OK, SD_NO_OBJECTIVE, SD_INFEASIBLE, SD_GAVE_UP = 0, 1, 2, 3
NS_OK, NS_INFEASIBLE, NS_GAVE_UP = 0, 1, 2
DS_OK, DS_CRITICAL, DS_INFEASIBLE, DS_GAVE_UP = 0, 1, 2, 3
DS_NO_START = 4
DS_MAXD, DS_MAXK = 4096, 16
SD_BRANCH_DELTA, SD_BRANCH_ONE, SD_BRANCH_INTERSECT = 0, 1, 2


class IdealInfo(ctypes.Structure):
    """mrbf_ideal_info: one start of mrbf_ideal_point_problem / mrbf_ideal_point_batch"""
    _fields_ = [("evals_ideal", ctypes.c_int32), ("generations", ctypes.c_int32), ("found", ctypes.c_int32), ("refined", ctypes.c_int32),
                ("ms_total", ctypes.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PsProblem(ctypes.Structure):
    _fields_ = [("n_models", ctypes.c_int32), ("n_objectives", ctypes.c_int32), ("models", ctypes.POINTER(ctypes.c_void_p)),
                ("roles", ctypes.POINTER(ctypes.c_int32)), ("n_lin_eq", ctypes.c_int32), ("n_lin_ineq", ctypes.c_int32),
                ("A_eq", ctypes.c_void_p), ("b_eq", ctypes.c_void_p), ("A_ineq", ctypes.c_void_p), ("b_ineq", ctypes.c_void_p),
                ("eq_tol", ctypes.c_double)]


class SdInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("bound_flips", ctypes.c_int32), ("ms_total", ctypes.c_float),
                ("omega", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DsInfo(ctypes.Structure):
    """mrbf_ds_info: what mrbf_ds_criticality reports"""
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("dropped", ctypes.c_int32), ("ms_total", ctypes.c_float),
                ("omega", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NormalInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("bound_flips", ctypes.c_int32), ("ms_total", ctypes.c_float),
                ("alpha", ctypes.c_double), ("delta", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class SdStepOptions(ctypes.Structure):
    _fields_ = [("strict", ctypes.c_int32), ("max_loops", ctypes.c_int32), ("const_rhs", ctypes.c_double), ("shrink", ctypes.c_double),
                ("min_stepsize", ctypes.c_double)]


class SdStepInfo(ctypes.Structure):
    _fields_ = [("branch", ctypes.c_int32), ("loops", ctypes.c_int32), ("ms_total", ctypes.c_float), ("sigma", ctypes.c_double),
                ("omega", ctypes.c_double), ("step_norm", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class SdBatchRecord(ctypes.Structure):
    _fields_ = [("sd_status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("bound_flips", ctypes.c_int32), ("branch", ctypes.c_int32),
                ("loops", ctypes.c_int32), ("reserved", ctypes.c_int32), ("omega", ctypes.c_double), ("omega_step", ctypes.c_double),
                ("sigma", ctypes.c_double), ("step_norm", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class DsBatchRecord(ctypes.Structure):
    """mrbf_ds_batch_record: one start of mrbf_ds_iterate_batch"""
    _fields_ = [("ds_status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("dropped", ctypes.c_int32), ("branch", ctypes.c_int32),
                ("loops", ctypes.c_int32), ("reserved", ctypes.c_int32), ("omega", ctypes.c_double), ("omega_step", ctypes.c_double),
                ("sigma", ctypes.c_double), ("step_norm", ctypes.c_double), ("dnorm", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NormalBatchRecord(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("iterations", ctypes.c_int32), ("bound_flips", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("alpha", ctypes.c_double), ("delta", ctypes.c_double)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class AffineJob(ctypes.Structure):
    """mrbf_affine_job: one start of mrbf_affine_select_batch"""
    _fields_ = [("mc", ctypes.c_int64), ("j0", ctypes.c_int32), ("max_picks", ctypes.c_int32), ("pivot_val", ctypes.c_double),
                ("shifted", ctypes.c_void_p), ("Q0", ctypes.c_void_p), ("picked_out", ctypes.c_void_p), ("Z_out", ctypes.c_void_p),
                ("n_picked", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Round4Job(ctypes.Structure):
    """mrbf_round4_job: one start of mrbf_round4_batch"""
    _fields_ = [("n0", ctypes.c_int64), ("mc", ctypes.c_int64), ("start_sites", ctypes.c_void_p), ("cand_sites", ctypes.c_void_p),
                ("kernel_id", ctypes.c_int32), ("poly_deg", ctypes.c_int32), ("a", ctypes.c_double), ("b", ctypes.c_double),
                ("max_points", ctypes.c_int32), ("theta_pivot_cholesky", ctypes.c_double), ("accepted_out", ctypes.c_void_p),
                ("n_accepted", ctypes.c_int32), ("rc", ctypes.c_int32)]


class FitJob(ctypes.Structure):
    """mrbf_fit_job: one start of mrbf_fit_batch"""
    _fields_ = [("n", ctypes.c_int64), ("d", ctypes.c_int32), ("k", ctypes.c_int32), ("kernel_id", ctypes.c_int32),
                ("poly_deg", ctypes.c_int32), ("a", ctypes.c_double), ("b", ctypes.c_double), ("centres", ctypes.c_void_p),
                ("values", ctypes.c_void_p), ("weights_out", ctypes.c_void_p), ("poly_out", ctypes.c_void_p), ("model", ctypes.c_void_p),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32), ("info", FitInfo)]


class EvalJob(ctypes.Structure):
    """mrbf_eval_job: one (model, query block) pair of mrbf_eval_batch"""
    _fields_ = [("model", ctypes.c_void_p), ("m", ctypes.c_int64), ("X", ctypes.c_void_p), ("vals_out", ctypes.c_void_p),
                ("jac_out", ctypes.c_void_p), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DbBoxJob(ctypes.Structure):
    """mrbf_db_box_job: one start of mrbf_db_box_batch"""
    _fields_ = [("db", ctypes.c_void_p), ("lb", ctypes.c_void_p), ("ub", ctypes.c_void_p), ("x0", ctypes.c_void_p),
                ("n_exclude", ctypes.c_int64), ("exclude", ctypes.c_void_p), ("zero_first_pick", ctypes.c_int32), ("rc", ctypes.c_int32),
                ("indices_out", ctypes.c_void_p), ("sites_out", ctypes.c_void_p), ("shifted_out", ctypes.c_void_p),
                ("first_row", ctypes.c_void_p), ("mc", ctypes.c_int64), ("first_pick", ctypes.c_int64),
                ("cand_sites_dev", ctypes.c_void_p), ("shifted_dev", ctypes.c_void_p)]


class DbGatherJob(ctypes.Structure):
    """mrbf_db_gather_job: one start of mrbf_db_gather_batch"""
    _fields_ = [("db", ctypes.c_void_p), ("n_idx", ctypes.c_int64), ("indices", ctypes.c_void_p), ("sites_out", ctypes.c_void_p),
                ("values_out", ctypes.c_void_p), ("sites_dev", ctypes.c_void_p), ("values_dev", ctypes.c_void_p),
                ("rc", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DbAppendJob(ctypes.Structure):
    """mrbf_db_append_job: one start of mrbf_db_append_batch"""
    _fields_ = [("db", ctypes.c_void_p), ("m", ctypes.c_int64), ("sites", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("first_index", ctypes.c_int64), ("rc", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DbSetValuesJob(ctypes.Structure):
    """mrbf_db_set_values_job: one start of mrbf_db_set_values_batch"""
    _fields_ = [("db", ctypes.c_void_p), ("m", ctypes.c_int64), ("indices", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("rc", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Round3Job(ctypes.Structure):
    """mrbf_round3_job: one start of mrbf_db_round3_batch"""
    _fields_ = [("db", ctypes.c_void_p), ("x", ctypes.c_void_p), ("lb", ctypes.c_void_p), ("ub", ctypes.c_void_p),
                ("pivot_val", ctypes.c_double), ("dirs", ctypes.c_void_p), ("n_dirs", ctypes.c_int32), ("reversed", ctypes.c_int32),
                ("n_missing", ctypes.c_int32), ("max_new", ctypes.c_int32), ("ensure_fully_linear", ctypes.c_int32),
                ("force_rebuild", ctypes.c_int32), ("mode", ctypes.c_int32), ("rc", ctypes.c_int32), ("new_sites_out", ctypes.c_void_p),
                ("first_index", ctypes.c_int64), ("n_new", ctypes.c_int32), ("fully_linear", ctypes.c_int32), ("status", ctypes.c_int32),
                ("n_dirs_used", ctypes.c_int32)]


class Problem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("m", ctypes.c_int64), ("d", ctypes.c_int32), ("k", ctypes.c_int32),
                ("kernel_id", ctypes.c_int32), ("poly_deg", ctypes.c_int32), ("a", ctypes.c_double), ("b", ctypes.c_double),
                ("centres", c_dp), ("values", c_dp), ("X", c_dp), ("weights_out", c_dp), ("poly_out", c_dp),
                ("vals_out", c_dp), ("jac_out", c_dp)]


class Result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("device", ctypes.c_int32), ("fit", FitInfo), ("ms_eval", ctypes.c_float),
                ("checksum_w", ctypes.c_double), ("checksum_vals", ctypes.c_double)]


# every symbol include/mrbf.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mrbf_init": (ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(c_vp)]),
    "mrbf_shutdown": (ctypes.c_int32, [c_vp]),
    "mrbf_last_error": (ctypes.c_char_p, [c_vp]),
    "mrbf_version": (ctypes.c_char_p, []),
    "mrbf_set_option": (ctypes.c_int32, [c_vp, ctypes.c_int32, ctypes.c_double]),
    "mrbf_get_option": (ctypes.c_int32, [c_vp, ctypes.c_int32, c_dp]),
    "mrbf_set_stream": (ctypes.c_int32, [c_vp, c_vp]),
    "mrbf_sync": (ctypes.c_int32, [c_vp]),
    "mrbf_gram": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, c_vp, ctypes.c_int32, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_int32, c_vp, c_vp, c_fp]),
    "mrbf_cross_gram": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, c_vp, c_vp, ctypes.c_int32, ctypes.c_double,
                                         ctypes.c_double, c_vp]),
    "mrbf_fit": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, ctypes.c_int32,
                                  ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(c_vp), c_vp, c_vp,
                                  ctypes.POINTER(FitInfo)]),
    "mrbf_model_from_coeffs": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, c_vp,
                                                ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                                ctypes.POINTER(c_vp)]),
    "mrbf_eval": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, c_vp, ctypes.POINTER(EvalInfo)]),
    "mrbf_eval_hessian": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.POINTER(HessInfo)]),
    "mrbf_eval_hessian_limited": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.POINTER(HessInfo),
                                                   ctypes.c_int64]),
    "mrbf_backtrack": (ctypes.c_int32, [c_vp, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32, c_vp, c_vp,
                                        c_vp, c_ip]),
    "mrbf_affine_scores": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_vp, c_vp, ctypes.c_int32, c_vp,
                                            ctypes.POINTER(ctypes.c_int64), c_dp]),
    "mrbf_affine_select": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, c_vp, ctypes.c_int32, c_vp, ctypes.c_int32, ctypes.c_double,
                                            ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), c_ip, c_vp]),
    "mrbf_affine_select_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(AffineJob), c_fp]),
    "mrbf_round4": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, c_vp, ctypes.c_int64, c_vp, ctypes.c_int32, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, c_vp, c_ip, ctypes.POINTER(c_vp)]),
    "mrbf_fit_from_round4": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int32, c_vp, ctypes.POINTER(c_vp), c_vp, c_vp, ctypes.POINTER(FitInfo)]),
    "mrbf_round4_sites": (ctypes.c_int32, [c_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), c_ip]),
    "mrbf_free_round4": (ctypes.c_int32, [c_vp, c_vp]),
    "mrbf_round4_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(Round4Job), c_fp]),
    "mrbf_dispatch_round4_batch": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32]),
    "mrbf_model_dims": (ctypes.c_int32, [c_vp, ctypes.POINTER(ctypes.c_int64), c_ip, c_ip, c_ip]),
    "mrbf_free_model": (ctypes.c_int32, [c_vp, c_vp]),
    "mrbf_batch_run": (ctypes.c_int32, [ctypes.c_int32, c_ip, ctypes.c_int64, ctypes.POINTER(Problem),
                                        ctypes.POINTER(Result)]),
    "mrbf_fit_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(FitJob), c_fp]),
    "mrbf_dispatch_fit_batch": (ctypes.c_int32, [ctypes.c_int64]),
    "mrbf_dispatch_fit_batch_max_n": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "mrbf_dispatch_fit_batch_lu": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]),
    "mrbf_eval_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(EvalJob), c_fp]),
    "mrbf_eval_batch_limited": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(EvalJob), c_fp, ctypes.c_int64]),
    "mrbf_dispatch_eval_batch": (ctypes.c_int32, [ctypes.c_int64]),
    "mrbf_dispatch_eval_batch_min_jobs": (ctypes.c_int64, []),
    "mrbf_eval_hessian_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(HessJob), ctypes.POINTER(HessBatchInfo)]),
    "mrbf_eval_hessian_batch_limited": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(HessJob), ctypes.POINTER(HessBatchInfo),
                                                         ctypes.c_int64]),
    "mrbf_dispatch_hessian_batch": (ctypes.c_int32, [ctypes.c_int64]),
    "mrbf_dispatch_hessian_batch_min_jobs": (ctypes.c_int64, []),
    "mrbf_db_create": (ctypes.c_int32, [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(c_vp)]),
    "mrbf_db_append": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "mrbf_db_set_values": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp]),
    "mrbf_db_read": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp]),
    "mrbf_db_dims": (ctypes.c_int32, [c_vp, ctypes.POINTER(ctypes.c_int64), c_ip, c_ip]),
    "mrbf_db_free": (ctypes.c_int32, [c_vp, c_vp]),
    "mrbf_db_box_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(DbBoxJob), c_fp]),
    "mrbf_db_gather_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(DbGatherJob), c_fp]),
    "mrbf_db_append_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(DbAppendJob), c_fp]),
    "mrbf_db_set_values_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(DbSetValuesJob), c_fp]),
    "mrbf_db_round3_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(Round3Job), c_fp]),
    "mrbf_dispatch_db_batch": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32]),
    "mrbf_debug_mfma_layout": (ctypes.c_int32, [c_vp, c_vp, c_vp, c_vp]),
    "mrbf_debug_potrf": (ctypes.c_int32, [c_vp, ctypes.c_int64, c_vp, ctypes.c_int32, c_ip, c_fp]),
    "mrbf_debug_env": (ctypes.c_int32, [ctypes.c_char_p]),
    "mrbf_debug_diag": (ctypes.c_int32, [c_vp, c_vp, ctypes.c_int32, c_fp, c_dp, c_dp]),
    "mrbf_debug_ps_rank": (ctypes.c_int32, [c_vp, ctypes.c_int32, c_vp, c_vp, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, c_ip, c_ip]),
    "mrbf_debug_mfma_peak": (ctypes.c_int32, [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_fp, c_dp]),
    "mrbf_debug_mfma_asm": (ctypes.c_int32, [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_fp, c_dp, c_dp]),
    "mrbf_debug_dgemm": (ctypes.c_int32, [c_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_fp, c_dp]),
    "mrbf_debug_mega_tables": (ctypes.c_int32, [ctypes.c_int32] * 8 + [c_vp]),
    "mrbf_debug_mega_tables2": (ctypes.c_int32, [ctypes.c_int32] * 8 + [c_vp, c_vp]),
    "mrbf_debug_mega_plan": (ctypes.c_int32, [ctypes.c_int32] * 3 + [c_vp]),
    "mrbf_stochastic_rank": (ctypes.c_int32, [ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_double, c_vp]),
    "mrbf_ps_step": (ctypes.c_int32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(PsOptions), c_vp, c_vp, c_vp,
                                      ctypes.POINTER(PsInfo)]),
    "mrbf_ps_step_problem": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(PsOptions),
                                              c_vp, c_vp, c_vp, ctypes.POINTER(PsInfo)]),
    "mrbf_ps_step_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(PsProblem), ctypes.POINTER(ctypes.c_void_p), c_vp, c_vp, c_vp,
                                            c_vp, c_vp, ctypes.POINTER(PsOptions), ctypes.POINTER(ctypes.c_uint64), c_vp, c_vp, c_vp,
                                            ctypes.POINTER(PsInfo), c_fp]),
    "mrbf_dispatch_ps_batch": (ctypes.c_int32, [ctypes.c_int64] + [ctypes.c_int32] * 6),
    "mrbf_ideal_point_problem": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, c_vp, ctypes.POINTER(PsOptions), c_vp, c_vp,
                                                  c_vp, ctypes.POINTER(IdealInfo)]),
    "mrbf_ideal_point_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(PsProblem), ctypes.POINTER(ctypes.c_void_p), c_vp, c_vp,
                                                c_vp, ctypes.POINTER(PsOptions), ctypes.POINTER(ctypes.c_uint64), c_vp, c_vp, c_vp,
                                                ctypes.POINTER(IdealInfo), c_fp]),
    "mrbf_dispatch_ideal": (ctypes.c_int32, [ctypes.c_int32] * 6),
    "mrbf_dispatch_ideal_batch": (ctypes.c_int32, [ctypes.c_int64] + [ctypes.c_int32] * 6),
    "mrbf_sd_direction": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [c_vp] * 8
                          + [ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mrbf_sd_criticality": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, c_vp, c_vp, ctypes.c_int32, c_vp, c_vp,
                                             ctypes.POINTER(SdInfo)]),
    "mrbf_ds_direction": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] + [c_vp] * 11),
    "mrbf_ds_criticality": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(DsInfo)]),
    "mrbf_dispatch_ds": (ctypes.c_int32, [ctypes.c_int32] * 6),
    "mrbf_ds_direction_rows": (ctypes.c_int32, [c_vp, ctypes.c_int64] + [ctypes.c_int32] * 4 + [c_vp] * 15),
    "mrbf_ds_criticality_rows": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                  ctypes.POINTER(DsInfo)]),
    "mrbf_dispatch_ds_rows": (ctypes.c_int32, [ctypes.c_int32] * 6),
    "mrbf_normal_direction": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] + [c_vp] * 12),
    "mrbf_normal_step": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), ctypes.c_int32, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int32, c_vp, c_vp, ctypes.POINTER(NormalInfo)]),
    "mrbf_sd_step": (ctypes.c_int32, [c_vp, ctypes.POINTER(PsProblem), c_vp, c_vp, ctypes.c_double, c_vp, c_vp, ctypes.c_double, c_vp,
                                      ctypes.POINTER(SdStepOptions), c_vp, c_vp, ctypes.POINTER(SdStepInfo)]),
    "mrbf_sd_iterate_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(PsProblem), ctypes.POINTER(ctypes.c_void_p), c_vp, c_vp, c_vp,
                                               c_vp, c_vp, ctypes.c_int32, ctypes.POINTER(SdStepOptions), c_vp, c_vp, c_vp,
                                               ctypes.POINTER(SdBatchRecord), c_fp]),
    "mrbf_dispatch_sd_batch": (ctypes.c_int32, [ctypes.c_int64] + [ctypes.c_int32] * 7),
    "mrbf_ds_iterate_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(PsProblem), ctypes.POINTER(ctypes.c_void_p), c_vp, c_vp, c_vp,
                                               c_vp, c_vp, c_vp, ctypes.POINTER(SdStepOptions), c_vp, c_vp, c_vp, c_vp,
                                               ctypes.POINTER(DsBatchRecord), c_fp]),
    "mrbf_dispatch_ds_batch": (ctypes.c_int32, [ctypes.c_int64] + [ctypes.c_int32] * 7),
    "mrbf_normal_step_batch": (ctypes.c_int32, [c_vp, ctypes.c_int64, ctypes.POINTER(PsProblem), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
                                                c_vp, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, c_vp, c_vp, c_vp,
                                                ctypes.POINTER(NormalBatchRecord), c_fp]),
    "mrbf_dispatch_normal_batch": (ctypes.c_int32, [ctypes.c_int64] + [ctypes.c_int32] * 5),
    "mrbf_dispatch_ps": (ctypes.c_int32, [ctypes.c_int32] * 6),
    "mrbf_dispatch_sd_step": (ctypes.c_int32, [ctypes.c_int32] * 7),
    "mrbf_dispatch_sd": (ctypes.c_int32, [ctypes.c_int32] * 6),
    "mrbf_dispatch_normal": (ctypes.c_int32, [ctypes.c_int32] * 5),
    "mrbf_dispatch_backtrack": (ctypes.c_int32, [ctypes.c_int32] * 3),
    "mrbf_dispatch_affine": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32]),
    "mrbf_dispatch_affine_batch": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "mrbf_dispatch_round4": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "mrbf_dispatch_fit": (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "mrbf_dispatch_after": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
}

_LIB = None


class MrbfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmrbf error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load libmrbf.so and bind every exported symbol; raises if the extension has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmrbf.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C morbit.jl_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def as_ptr(a):
    """void* of a NumPy array (host) or of anything exposing data_ptr() (a torch tensor, host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    raise TypeError("expected numpy array or tensor, got %r" % type(a))


def host_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class Context:
    """One per host thread and GPU (mrbf_init / mrbf_shutdown)."""

    def __init__(self, device_id=-1):
        self.lib = load()
        h = c_vp()
        rc = self.lib.mrbf_init(device_id, ctypes.byref(h))
        if rc != 0:
            raise MrbfError(rc, (self.lib.mrbf_last_error(None) or b"").decode())
        self.h = h

    def check(self, rc):
        if rc != 0:
            raise MrbfError(rc, (self.lib.mrbf_last_error(self.h) or b"").decode())

    def set_option(self, key, value):
        self.check(self.lib.mrbf_set_option(self.h, key, float(value)))

    def get_option(self, key):
        v = ctypes.c_double()
        self.check(self.lib.mrbf_get_option(self.h, key, ctypes.byref(v)))
        return v.value

    def sync(self):
        self.check(self.lib.mrbf_sync(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mrbf_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX = {}


def default_context(device_id=-1):
    import threading

    key = (threading.get_ident(), device_id)
    if key not in _DEFAULT_CTX:
        _DEFAULT_CTX[key] = Context(device_id)
    return _DEFAULT_CTX[key]
