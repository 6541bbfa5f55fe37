// The decision table of the host bindings (include/mrbf.h, "decision table"): which call of Morbit's surrogate / descent interface
// goes to a device entry point and which to Morbit's own method.  Pure host code: HipRbf.jl and the Python mirror call these
// functions instead of each carrying a copy of the rules, and tests/test_dispatch.py pins them without a GPU.
#include "common.hpp"

namespace {
// limits of ps_solver.hip (MAXLAM, MAXOBJ, MAXMODELS, MAXCON); the population of the PS run is 20 (d + 2)
constexpr int PS_MAXLAM = 7168, PS_MAXOBJ = 8, PS_MAXMODELS = 8, PS_MAXCON = 32, PS_MAXLIN = 256;
// below this many candidate coordinates one host BLAS call beats a launch + two copies (tools/affine_bench.py)
constexpr int64_t AFFINE_MIN_WORK = 4096 * 8;
constexpr int64_t FIT_REUSE_MAX_N = 1024;
// mrbf_dispatch_fit_batch_max_n: from min_starts starts on, the one-launch fit takes up to max_n sites (rows ascending in both).
// Measured at d = 128 (tools/fit_batch_bench.py --wide, profiles/fit_batch_wide_bench.jsonl): batch / parent loop = 0.54 - 0.56 at (8 starts,
// n = 1684), 0.72 - 0.73 at (8, 2048) -- within a run-to-run spread of the 0.8 that admits a cell, so not admitted --, 0.41 at (16, 2048)
struct FitWideRow {
    int64_t min_starts, max_n;
};
constexpr FitWideRow FIT_WIDE[] = {{8, 1684}, {16, 2048}};
constexpr int FIT_WIDE_MIN_D = 65;  // the padded dimension the cells were measured at (dpad = 128); d <= 64 has another chain and no measurement
constexpr int FIT_WIDE_ROWS = (int)(sizeof(FIT_WIDE) / sizeof(FIT_WIDE[0]));
// mrbf_dispatch_fit_batch_lu: from min_starts LU-path starts on, the one-launch LU takes the batch up to max_n sites and dimension max_d
// (rows ascending in all three).  Measured (profiles/fit_batch_lu_bench.jsonl: thin plate spline k = 2, degree-1 tail, k = 2, 30 calls
// each): batch / loop of single calls = 0.87, 1.24, 1.96 with 1 start at (n, d) = (33, 16), (257, 128), (512, 128) -- not admitted --,
// 0.12, 0.16, 0.25 with 8 starts, 0.065, 0.082, 0.13 with 16 and 0.023, 0.023, 0.035 with 64; 2 .. 7 starts were not measured
struct FitLuRow {
    int64_t min_starts, max_n;
    int max_d;
};
constexpr FitLuRow FIT_LU[] = {{8, 512, 128}};
constexpr int FIT_LU_ROWS = (int)(sizeof(FIT_LU) / sizeof(FIT_LU[0]));
// mrbf_dispatch_eval_batch_min_jobs: from this many jobs on the bindings make one mrbf_eval_batch call instead of the loop of mrbf_eval.
// Measured at the C4 shape (tools/eval_batch_bench.py, profiles/eval_batch_bench.jsonl: d = 128, n = 257, k = 2, device-resident buffers,
// medians of 30 host-clock calls): batch / loop of single calls on the parent build = 0.48, 0.40, 0.36 at 8, 16, 64 jobs of m = 6450 with
// Jacobians, 0.16, 0.083, 0.033 at 8, 16, 64 jobs of m = 2 values only, 0.031 at 64 jobs of d = 3, n = 20; fewer than 8 jobs were not
// measured and keep the loop
constexpr int64_t EVAL_BATCH_MIN_JOBS = 8;
// mrbf_dispatch_hessian_batch_min_jobs: from this many jobs on the bindings make one mrbf_eval_hessian_batch call instead of the loop of
// mrbf_eval_hessian.  Measured (tools/hessian_batch_bench.py, profiles/hessian_batch_bench.jsonl: all outputs of k = 2, device-resident
// buffers, medians of 30 host-clock calls): batch / loop of single calls on the parent build = 0.54, 0.28, 0.15, 0.097, 0.054 at 2, 4, 8,
// 16, 64 jobs of the C4 model (d = 128, n = 257) with m = 1 and 0.68, 0.47, 0.37, 0.41, 0.37 with m = 16; 0.16, 0.094 at 8, 64 jobs of
// the C3 model (d = 64, n = 8192, m = 1); 0.33, 0.31 at 8, 64 jobs of d = 256, n = 1024 (m = 1): every measured cell is admitted; a
// single job was not measured and keeps the single call
constexpr int64_t HESSIAN_BATCH_MIN_JOBS = 2;
}  // namespace

extern "C" {

int32_t mrbf_dispatch_ps(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    if (n_foreign != 0) return MRBF_DISPATCH_REFERENCE;                       // outer functions / other model families live on the host
    if (d < 1 || 20 * (d + 2) > PS_MAXLAM) return MRBF_DISPATCH_REFERENCE;    // d <= 356
    if (k < 1 || k > PS_MAXOBJ) return MRBF_DISPATCH_REFERENCE;
    if (n_models < 1 || n_models > PS_MAXMODELS) return MRBF_DISPATCH_REFERENCE;
    if (n_nl_constraints < 0 || n_nl_constraints > PS_MAXCON) return MRBF_DISPATCH_REFERENCE;
    if (n_lin_constraints < 0 || n_lin_constraints > PS_MAXLIN) return MRBF_DISPATCH_REFERENCE;
    return MRBF_DISPATCH_DEVICE;
}

// the Pascoletti-Serafini steps of many starts in one call (ps_solver.hip, mrbf_ps_step_batch): what the single call takes, inside the
// fused evaluation kernels' range (dpad in {64, 128, 256}) and with the start on a grid dimension
int32_t mrbf_dispatch_ps_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                               int32_t n_foreign) {
    if (n_starts < 1 || n_starts > 65535 || d > 256) return MRBF_DISPATCH_REFERENCE;
    return mrbf_dispatch_ps(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign);
}

// the ideal-point phase of that step as calls of its own (ps_solver.hip, mrbf_ideal_point_problem / mrbf_ideal_point_batch): the
// step's kernels and limits, hence the step's rows
int32_t mrbf_dispatch_ideal(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    return mrbf_dispatch_ps(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign);
}
int32_t mrbf_dispatch_ideal_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints,
                                  int32_t n_lin_constraints, int32_t n_foreign) {
    return mrbf_dispatch_ps_batch(n_starts, d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign);
}

// the direction LP of steepest descent (sd_lp.hip): at most 64 rows (B^-1 lives in LDS), d within the library's limit
int32_t mrbf_dispatch_sd(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    if (n_foreign != 0 || n_models < 1) return MRBF_DISPATCH_REFERENCE;
    if (d < 1 || d > 4096 || k < 1 || n_nl_constraints < 0 || n_lin_constraints < 0) return MRBF_DISPATCH_REFERENCE;
    return (int64_t)k + n_nl_constraints + n_lin_constraints <= 64 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the direction QP of directed search (ds_qp.hip): the k x k objects are factorised by one thread in LDS (k <= 16), d within the library's
// limit; constraint rows are not on the device -- the reference's own formulation (descent.jl:635-640) has none
int32_t mrbf_dispatch_ds(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    if (n_foreign != 0 || n_models < 1) return MRBF_DISPATCH_REFERENCE;
    if (d < 1 || d > 4096 || k < 1 || k > 16) return MRBF_DISPATCH_REFERENCE;
    return n_nl_constraints == 0 && n_lin_constraints == 0 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the direction QP of directed search with constraint rows (ds_qp_rows.hip; descent.jl:196-236, :598-645): objective and constraint rows
// share the K x K objects in LDS (K = k + n_nl + n_lin <= 16); without a constraint row mrbf_dispatch_ds is the table to ask
int32_t mrbf_dispatch_ds_rows(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    if (n_foreign != 0 || n_models < 1) return MRBF_DISPATCH_REFERENCE;
    if (d < 1 || d > 4096 || k < 1 || n_nl_constraints < 0 || n_lin_constraints < 0) return MRBF_DISPATCH_REFERENCE;
    if ((int64_t)n_nl_constraints + n_lin_constraints < 1) return MRBF_DISPATCH_REFERENCE;
    return (int64_t)k + n_nl_constraints + n_lin_constraints <= 16 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the normal-step LP (normal_lp.hip): at most 64 rows (M^-1 lives in LDS), d within the library's limit; linear rows need no model
int32_t mrbf_dispatch_normal(int32_t d, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign) {
    if (n_foreign != 0 || n_models < 0 || d < 1 || d > 4096 || n_nl_constraints < 0 || n_lin_constraints < 0) return MRBF_DISPATCH_REFERENCE;
    const int64_t rows = (int64_t)n_nl_constraints + n_lin_constraints;
    return rows >= 1 && rows <= 64 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the steepest-descent step (sd_step.hip): the Armijo scan reads up to 64 objectives and max_loops + 2 trial rows, the step size
// kernel one workgroup's worth of stacked constraint rows
int32_t mrbf_dispatch_sd_step(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign,
                              int32_t max_loops) {
    if (n_foreign != 0 || n_models < 1) return MRBF_DISPATCH_REFERENCE;
    if (d < 1 || d > 4096 || k < 1 || k > 64 || n_nl_constraints < 0 || n_lin_constraints < 0) return MRBF_DISPATCH_REFERENCE;
    if (max_loops < 0 || max_loops > 1024) return MRBF_DISPATCH_REFERENCE;
    return (int64_t)n_nl_constraints + n_lin_constraints <= 256 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// many starts in one call (sd_batch.hip): what both single calls take, inside the fused evaluation kernels' range (dpad in {64, 128,
// 256}) and with the start on a grid dimension
int32_t mrbf_dispatch_sd_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                               int32_t n_foreign, int32_t max_loops) {
    if (n_starts < 1 || n_starts > 65535 || d > 256) return MRBF_DISPATCH_REFERENCE;
    if (mrbf_dispatch_sd(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign) != MRBF_DISPATCH_DEVICE) return MRBF_DISPATCH_REFERENCE;
    return mrbf_dispatch_sd_step(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign, max_loops);
}

// directed search for many starts in one call (ds_batch.hip): what both single calls take, inside the fused evaluation kernels' range
// (dpad in {64, 128, 256}) and with the start on a grid dimension
int32_t mrbf_dispatch_ds_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                               int32_t n_foreign, int32_t max_loops) {
    if (n_starts < 1 || n_starts > 65535 || d > 256) return MRBF_DISPATCH_REFERENCE;
    if (mrbf_dispatch_ds(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign) != MRBF_DISPATCH_DEVICE) return MRBF_DISPATCH_REFERENCE;
    return mrbf_dispatch_sd_step(d, k, n_models, n_nl_constraints, n_lin_constraints, n_foreign, max_loops);
}

// the normal steps of many starts in one call (normal_batch.hip): what the single call takes, with the start on a grid dimension;
// modelled rows are evaluated by the fused evaluation kernels (dpad in {64, 128, 256}), linear rows alone need no evaluation
int32_t mrbf_dispatch_normal_batch(int64_t n_starts, int32_t d, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                                   int32_t n_foreign) {
    if (n_starts < 1 || n_starts > 65535) return MRBF_DISPATCH_REFERENCE;
    if (n_nl_constraints != 0 && d > 256) return MRBF_DISPATCH_REFERENCE;
    return mrbf_dispatch_normal(d, n_models, n_nl_constraints, n_lin_constraints, n_foreign);
}

int32_t mrbf_dispatch_backtrack(int32_t n_objective_models, int32_t n_foreign, int32_t outputs_in_order) {
    return (n_objective_models == 1 && n_foreign == 0 && outputs_in_order != 0) ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

int32_t mrbf_dispatch_affine(int64_t n_candidates, int32_t d) {
    if (d < 1 || n_candidates < 1) return MRBF_DISPATCH_REFERENCE;
    // round 6: the device entry point is the whole pick loop (mrbf_affine_select, ~50 us per pick whatever the candidate count); on the host a
    // pick costs two products of d x (d - j) x candidates.  From d = 64 on the device wins as soon as there are more candidates than
    // directions (d = 128, 255 candidates: 6.5 against 22 ms per model update, profiles/r06_iteration_c4.txt); below, only for large boxes
    if (d >= 64 && n_candidates >= d) return MRBF_DISPATCH_DEVICE;
    return n_candidates * (int64_t)d >= AFFINE_MIN_WORK ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// many filters in one call (affine.hip, affsel_pick_batch_kernel): the start on a grid dimension, the filter's own norm, and the eight
// candidates' coordinates of a workgroup within 64 KiB of LDS -- the range of the one-launch-per-pick kernel
int32_t mrbf_dispatch_affine_batch(int64_t n_starts, int32_t d, int32_t p_is_inf) {
    if (n_starts < 1 || n_starts > 65535 || d < 1 || p_is_inf == 0) return MRBF_DISPATCH_REFERENCE;
    return (int64_t)8 * (d + 1) * 8 <= 64 * 1024 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the model updates of many starts in one call (batch.hip, mrbf_fit_batch): the start on a grid dimension; which starts the batched fit
// takes and which the single call inside it is decided start by start in the library
int32_t mrbf_dispatch_fit_batch(int64_t n_starts) { return n_starts >= 1 && n_starts <= 65535 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE; }

// the value of MRBF_OPT_SMALL_FIT_MAX_N the bindings set around mrbf_fit_batch: the largest n the one-launch fit should take for a batch
// of n_starts starts of dimension d (small.hip: beyond 512 sites the solves are dealt over the cluster as well).  The bindings keep the
// loop of single calls -- 512, the default: a start beyond it takes mrbf_fit inside the call -- where the batch does not pay: a cell
// (n_starts, n) is admitted only where the batch took at most 0.8 of the loop's median (tools/fit_batch_bench.py --wide,
// profiles/fit_batch_wide_bench.jsonl), and between measured cells the rule takes the smaller n of the smaller
// batch, so that it is monotone in n_starts.  Fewer than 8 starts, and d <= 64 (the launch chain has another front end there, small.hip:
// TailQ), were not measured: 512.
int64_t mrbf_dispatch_fit_batch_max_n(int64_t n_starts, int32_t d) {
    if (n_starts < 1 || n_starts > 65535 || d < FIT_WIDE_MIN_D || d > 128) return 512;
    for (int i = FIT_WIDE_ROWS - 1; i >= 0; --i)
        if (n_starts >= FIT_WIDE[i].min_starts) return FIT_WIDE[i].max_n;
    return 512;
}

// whether the bindings set MRBF_OPT_SMALL_LU around mrbf_fit_batch: n_lu_starts of the call's starts are on the LU path inside the
// option's range (small_lu.hip: n <= 512, d <= 128), the largest with n_max sites, of dimension d.  Modelled on the row above: measured
// cells only -- a row (min_starts, max_n, max_d) is admitted where the batch under the option took at most 0.8 of the median of the loop
// of single calls with the option off (tools/fit_batch_lu_bench.py, profiles/fit_batch_lu_bench.jsonl) --, rows
// ascending in all three columns, so that the answer is monotone in n_lu_starts; a shape beyond the largest measured one of its row: 0.
int32_t mrbf_dispatch_fit_batch_lu(int64_t n_lu_starts, int64_t n_max, int32_t d) {
    if (n_lu_starts < 1 || n_lu_starts > 65535 || n_max < 1 || n_max > 512 || d < 1 || d > 128) return 0;
    for (int i = FIT_LU_ROWS - 1; i >= 0; --i)
        if (n_lu_starts >= FIT_LU[i].min_starts) return n_max <= FIT_LU[i].max_n && d <= FIT_LU[i].max_d ? 1 : 0;
    return 0;
}

int32_t mrbf_dispatch_round4(int64_t n0, int32_t d, int32_t poly_deg, int64_t n_candidates) {
    const int q = mrbf::poly_dim(d, poly_deg);
    if (n_candidates < 1 || n0 < 1 || n0 > 8192) return MRBF_DISPATCH_REFERENCE;
    // the limits of mrbf_round4 itself (round4.hip: d <= 1024, at most 30 000 candidates -- four candidate x candidate matrices live on
    // the device): a database box beyond them takes the reference's loop, it does not raise
    if (d < 1 || d > 1024 || n_candidates > 30000) return MRBF_DISPATCH_REFERENCE;
    return n0 >= q ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// round 4 of many starts in one call (round4_small.hip, mrbf_round4_batch): the start on a grid dimension and mrbf_round4's own limit on
// d (a start outside the small kernel's range takes mrbf_round4 inside the call); which starts share the batched launches is decided
// inside the call, start by start
int32_t mrbf_dispatch_round4_batch(int64_t n_starts, int32_t d) {
    return n_starts >= 1 && n_starts <= 65535 && d >= 1 && d <= 1024 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the box scans and row gathers of many resident databases in one call (db.hip): the start on a grid dimension; the kernels walk a row
// with a wave whatever its length, so d only has the library's own limit
int32_t mrbf_dispatch_db_batch(int64_t n_starts, int32_t d) {
    return n_starts >= 1 && n_starts <= 65535 && d >= 1 && d <= 4096 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE;
}

// the evaluations of many kept models in one call (eval_batch.hip, mrbf_eval_batch): the job on a grid dimension; which jobs share the
// fused kernels' launches and which take the single call's chain inside the call is decided there, job by job
int32_t mrbf_dispatch_eval_batch(int64_t n_jobs) { return n_jobs >= 1 && n_jobs <= 65535 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE; }

// the fewest jobs from which the batch pays (admitted where the batch took at most 0.8 of the median of the loop of single calls on the
// parent build; monotone: every larger batch takes the call as well; a value above 65535 would mean: the bindings keep the loop)
int64_t mrbf_dispatch_eval_batch_min_jobs(void) { return EVAL_BATCH_MIN_JOBS; }

// the Hessians of many kept models in one call (hess.hip, mrbf_eval_hessian_batch): the family's limit on the job count; which jobs
// share a launch is decided there, by kernel instantiation alone
int32_t mrbf_dispatch_hessian_batch(int64_t n_jobs) { return n_jobs >= 1 && n_jobs <= 65535 ? MRBF_DISPATCH_DEVICE : MRBF_DISPATCH_REFERENCE; }

// the fewest jobs from which that call pays (the admission rule of mrbf_dispatch_eval_batch_min_jobs; a value above 65535 would mean: the
// bindings keep the loop)
int64_t mrbf_dispatch_hessian_batch_min_jobs(void) { return HESSIAN_BATCH_MIN_JOBS; }

int32_t mrbf_dispatch_fit(int64_t n_training, int64_t state_n0, int32_t state_q, int32_t state_n_accepted, int32_t same_sites) {
    if (state_n0 < 1 || state_n_accepted < 1 || !same_sites) return MRBF_FIT_FULL;
    if (state_n0 != state_q) return MRBF_FIT_FULL;  // the kept factor only covers the directions added by round 4
    // beyond ~1000 sites the ordinary fit (persistent Cholesky) is as fast as the two triangular solves with the kept factor (d = 64,
    // n = 2145: 1.6 ms both, tools/round4_bench.py) and more accurate (the kappa matrix is formed with cancellation: residual 2e-11
    // against 1e-15): reuse pays below that
    if (n_training > FIT_REUSE_MAX_N) return MRBF_FIT_FULL;
    return state_n0 + state_n_accepted == n_training ? MRBF_FIT_FROM_ROUND4 : MRBF_FIT_FULL;
}

int32_t mrbf_dispatch_after(int32_t entry, int32_t rc) {
    switch (entry) {
        // (-3 / -5: dimension / candidate count beyond the device path; MRBF_ENOMEM: the candidate matrices did not fit)
        case MRBF_ENTRY_ROUND4: return rc == -2 || rc == -3 || rc == -5 || rc == MRBF_ESINGULAR || rc == MRBF_ENOMEM;
        case MRBF_ENTRY_FIT_FROM_ROUND4: return rc == -2 || rc == MRBF_ESINGULAR || rc == MRBF_ENOTPD;
        case MRBF_ENTRY_PS_STEP: return rc == -2;
        case MRBF_ENTRY_PS_BATCH: return rc == -2;  // likewise: the callers run the single call per start; a start's own status is in its info
        case MRBF_ENTRY_IDEAL: return rc == -2;        // shape outside the device path: the host search
        case MRBF_ENTRY_IDEAL_BATCH: return rc == -2;  // likewise: the callers run the single call per start
        case MRBF_ENTRY_SD: return rc == -2;  // shape outside the device path, or the LP gave up (MRBF_SD_GAVE_UP)
        case MRBF_ENTRY_NORMAL: return rc == -2;  // likewise (MRBF_NS_GAVE_UP)
        case MRBF_ENTRY_SD_STEP: return rc == -2;  // shape outside the device path
        case MRBF_ENTRY_SD_BATCH: return rc == -2;  // likewise; a start whose LP gave up says so in its record, not in rc
        case MRBF_ENTRY_AFFINE_BATCH: return rc == -2;  // likewise: the callers run the single-start call (or the host filter) per start
        case MRBF_ENTRY_FIT_BATCH: return rc == -2;  // likewise: the callers run the single fit per start
        case MRBF_ENTRY_NORMAL_BATCH: return rc == -2;  // likewise; a start whose LP gave up says so in its record, not in rc
        // the call itself: -2 (the table refuses the shape: the single call, or the host mirror, per start); a start's own rc
        // (mrbf_round4_job.rc, what mrbf_round4 returned for it) reads as MRBF_ENTRY_ROUND4's
        case MRBF_ENTRY_ROUND4_BATCH: return rc == -2 || rc == -3 || rc == -5 || rc == MRBF_ESINGULAR || rc == MRBF_ENOMEM;
        // the table refuses the shape: results_in_box_indices / the row copies on the host copy of the database; a job's own rc is an error
        case MRBF_ENTRY_DB_BOX: return rc == -2;
        case MRBF_ENTRY_DB_GATHER: return rc == -2;
        // likewise: _rbf_round3 / the per-start appends and value updates on the host copy; a job's own rc is an error
        case MRBF_ENTRY_DB_ROUND3: return rc == -2;
        case MRBF_ENTRY_DB_APPEND_BATCH: return rc == -2;
        case MRBF_ENTRY_DB_SET_VALUES_BATCH: return rc == -2;
        case MRBF_ENTRY_EVAL_BATCH: return rc == -2;  // the table refuses the job count: mrbf_eval per job; a job's own status is an error
        case MRBF_ENTRY_HESSIAN_BATCH: return rc == -2;  // likewise: mrbf_eval_hessian per job; a job's own status is an error
        case MRBF_ENTRY_DS: return rc == -2;  // shape outside the device path, or the QP gave up (MRBF_DS_GAVE_UP)
        case MRBF_ENTRY_DS_ROWS: return rc == -2;  // likewise, or d = 0 misses a constraint row (MRBF_DS_NO_START)
        case MRBF_ENTRY_DS_BATCH: return rc == -2;  // shape outside the device path; a start whose QP gave up says so in its record, not in rc
        default: return 0;
    }
}

}  // extern "C"
