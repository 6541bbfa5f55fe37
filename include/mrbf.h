/* mrbf.h -- C ABI of the MI355X-native RBF surrogate engine (libmrbf.so).
 *
 * Drop-in boundary for Morbit.jl's RbfConfig hot path.  Morbit reaches this
 * arithmetic through Julia multiple dispatch into RadialBasisFunctionModels.jl;
 * each entry point below names the reference interface it replaces.  A Julia
 * maintainer binds these with `ccall` (see INTEGRATION.md and
 * morbit.jl_amd/julia/HipRbf.jl); tests and bench bind them with ctypes.
 *
 * Conventions
 *   - every call returns int32: 0 ok; <0 = -(1-based index of the invalid
 *     argument); >0 numerical / runtime error (MRBF_E*).  Nothing throws or
 *     aborts across the ABI.  mrbf_last_error(ctx) gives a static string.
 *   - all numbers are fp64.  Buffers may be HOST or DEVICE pointers (detected
 *     with hipPointerGetAttributes); host buffers are copied over PCIe inside
 *     the call, device buffers are used in place on the context's stream.
 *   - the caller owns in/out buffers for the duration of the call (Julia:
 *     GC.@preserve); the library owns ctx and model handles.
 *   - one ctx per host thread; a ctx is not thread-safe; ctxs are independent.
 *   - layouts (chosen so that Julia's native arrays are passed zero-copy):
 *       centres  n x d row-major  == Julia d x n column-major
 *                                 == reinterpret(reshape, Float64, Vector{SVector{d}})
 *       values   n x k row-major  == Julia k x n column-major (Vector{MVector{k}})
 *       weights  n x k row-major, poly q x k row-major, basis [1, x_1..x_d]
 *       X        m x d row-major;  vals m x k row-major
 *       jac      per point a k x d COLUMN-major block (unsafe_wrap as Matrix k x d)
 *       Phi n x n, Pi n x q column-major.
 */
#ifndef MRBF_H
#define MRBF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrbf_ctx mrbf_ctx;
typedef struct mrbf_model mrbf_model;

/* kernel ids in the order of Morbit.RbfKernels (src/models/RbfModel.jl:48-54).
 * (a, b) are what _get_kernel_params (RbfModel.jl:665-690) hands to the package:
 *   cubic: a = beta (odd, default 3)              inv_multiquadric / multiquadric: a = alpha, b = beta (default 1, 1/2)
 *   thin_plate_spline: a = k (default 2)          gaussian: a = alpha (default 1) */
enum {
    MRBF_CUBIC = 0,
    MRBF_INV_MULTIQUADRIC = 1,
    MRBF_MULTIQUADRIC = 2,
    MRBF_THIN_PLATE_SPLINE = 3,
    MRBF_GAUSSIAN = 4
};

enum {
    MRBF_OK = 0,
    MRBF_ENOTPD = 1,    /* Cholesky met a non-positive pivot and the LU retry was disabled */
    MRBF_ESINGULAR = 2, /* LU met an exactly zero pivot (info.factor_info = its 1-based index) */
    MRBF_EHIP = 3,      /* a HIP runtime call failed */
    MRBF_EBLAS = 4,     /* a rocBLAS / rocSOLVER call failed */
    MRBF_ENOMEM = 5,
    MRBF_ENODEVICE = 6, /* no usable GPU: the library never computes on the CPU */
    MRBF_ENCCL = 7
};

/* solve paths reported in mrbf_fit_info.path */
enum {
    MRBF_PATH_CHOL = 1,      /* Phi SPD, no tail: potrf(Phi) */
    MRBF_PATH_PROJ_CHOL = 2, /* tail + conditionally p.d. kernel: potrf(P Phi P + mu Q1 Q1') on null(Pi') */
    MRBF_PATH_LU = 3,        /* indefinite saddle system [Phi Pi; Pi' 0]: getrf */
    MRBF_PATH_MINNORM = 4,   /* n < q (fewer sites than tail terms): minimum-norm solution by SVD */
    MRBF_PATH_ROUND4 = 5     /* mrbf_fit_from_round4: two triangular solves with the factor the site selection left behind */
};

/* mrbf_set_option keys */
enum {
    MRBF_OPT_GRAM_MODE = 1,    /* 0 = MFMA GEMM-form (default), 1 = VALU difference-form (reference arithmetic) */
    MRBF_OPT_RESIDUAL = 2,     /* 1 = compute rel_residual / max|Pi'w| after a fit (default 1) */
    MRBF_OPT_FORCE_PATH = 3,   /* 0 = automatic, else one of MRBF_PATH_* */
    MRBF_OPT_CHOL_IMPL = 4,    /* 0 = library default (3 from 256 columns on, else 2), 1 = rocSOLVER potrf, 2 = built-in blocked MFMA Cholesky driven by
                                  host launches, 3 = the same factorisation as one persistent launch */
    MRBF_OPT_EVAL_IMPL = 5,    /* 0 = default, 1 = GEMM pipeline, 2 = fused MFMA kernel */
    MRBF_OPT_TIMING = 6,       /* 1 = record per-phase hipEvents (default 1) */
    MRBF_OPT_DIAG_IMPL = 7,    /* diagonal-block kernel of the built-in Cholesky: 0 = MFMA-tiled (default), 1 = column sweep (host-driven
                                  factorisation only) */
    MRBF_OPT_CHOL_WINDOW = 8,  /* panels aggregated per trailing update: 0 = size-dependent schedule (default), else 1, 2 or 4 */
    MRBF_OPT_SPIN_MS = 9,      /* wall-clock limit (ms) a persistent kernel waits on one dependency without progress before it gives up
                                  and the call falls back to the host-driven GPU path (default 1000) */
    MRBF_OPT_LAST_DEVICE_MS = 11, /* read only: time the last persistent factorisation spent on the device, by its own clock (first
                                  workgroup in -> last workgroup out); unlike the hipEvent phases it excludes whatever the host did
                                  between the events */
    MRBF_OPT_SLOW_LAUNCHES = 12,  /* read only: persistent factorisations of this context that took more than twice the shortest seen
                                  at their shape (cumulative) */
    MRBF_OPT_ARENA_BYTES = 13,   /* read only: bytes of device memory the context's grow-only arena (named work buffers) and its pool of released
                                  * model blocks hold: constant in steady state (a caller can watch it over its iterations) */
    MRBF_OPT_LIVE_HANDLES = 14,  /* read only: models + round-4 states created through this context and not yet released */
    MRBF_OPT_SMALL_FIT_MAX_N = 15, /* most sites the one-launch fit takes (mrbf_fit, mrbf_fit_batch): 512 (default) .. 2048; any other value
                                  is an invalid argument (-2) and the stored value stays.  With 512 every result is what it always
                                  was.  Above, a start with 512 < n <= the value takes the one-launch fit as well (same shape range
                                  otherwise): a batch of such starts is one launch instead of a launch chain per start -- the bindings
                                  raise it around mrbf_fit_batch where mrbf_dispatch_fit_batch_max_n says the batch pays.  A fit is
                                  reproducible bit for bit under ONE value; the one-launch fit and the chain sum in different orders.
                                  The context's grow-only arena keeps the scratch of the widest batch (46 MB per start at n = 2048,
                                  d = 128; MRBF_OPT_ARENA_BYTES shows it) */
    MRBF_OPT_SMALL_LU = 16,    /* 0 (default) or 1; any other value is an invalid argument (-2) and the stored value stays.  With 0 every
                                  result is, bit for bit, what it always was.  With 1 a fit on the LU path (the kernel's order exceeds
                                  what the tail covers -- thin plate spline k = 2 or cubic 5 with a linear tail, cubic 3 with a constant
                                  or no tail, multiquadric without a tail --, n == q, or a Cholesky that gave up) with n <= 512, d <= 128,
                                  k <= 16, n >= q and a smooth kernel takes ONE launch (small_lu.hip: getrf's arithmetic, one workgroup
                                  per start) instead of the rocSOLVER chain, and mrbf_fit_batch puts such starts into one launch; the
                                  bindings raise it around mrbf_fit_batch where mrbf_dispatch_fit_batch_lu says the batch pays.  Not
                                  honoured with MRBF_OPT_GRAM_MODE 1 or a forced path other than MRBF_PATH_LU.  A fit is reproducible
                                  bit for bit under ONE value.  Scratch: at most 3.5 MB per start in the context's arena */
    MRBF_OPT_DEBUG_FAULT = 10  /* test hook: bit 0 = one workgroup of the persistent factorisation skips a publish, bit 1 = one workgroup of
                                  the persistent backward substitution does (the next fit must fall back and still return the right weights), bit 2 = one
                                  member of a small fit's workgroup cluster leaves early (the fit is repeated with one workgroup per problem) */
};

/* bits of mrbf_fit_info.fallbacks: a GPU path that was abandoned for another GPU path inside the same call (rc stays 0) */
enum {
    MRBF_FB_CHOL_HOST_DRIVEN = 1, /* persistent Cholesky gave up on a dependency -> re-assembled, host-driven blocked Cholesky */
    MRBF_FB_BACKSOLVE_BLOCKED = 2, /* persistent backward substitution gave up -> one launch per block row */
    MRBF_FB_LU = 4                /* Cholesky met a non-positive pivot / rank-deficient tail -> LU of the saddle system */
};

typedef struct {
    int32_t path;         /* MRBF_PATH_* actually taken */
    int32_t factor_info;  /* potrf / getrf info (0 = clean) */
    int32_t n, q;         /* system sizes */
    double rel_residual;  /* ||Phi w + Pi lam - Y||_F / ||Y||_F recomputed through the eval kernels; NaN if disabled */
    double max_pitw;      /* max |Pi' w|; NaN if disabled */
    double mu;            /* shift used by the projected Cholesky (0 otherwise) */
    float ms_gram, ms_project, ms_factor, ms_solve, ms_check, ms_total; /* hipEvent times on the ctx stream */
    int32_t fallbacks;    /* MRBF_FB_* bits */
    int32_t giveup_code;  /* diagnostic code of the last give-up (0 if none) */
    float ms_factor_device; /* persistent factorisation: its time by the launch's own clock (0 on other paths); ms_factor - this =
                               host-side gaps inside the hipEvent bracket (descheduled launcher thread, job-table rebuild) */
    int32_t slow_launches;  /* MRBF_OPT_SLOW_LAUNCHES of the context after this fit */
} mrbf_fit_info;

typedef struct {
    float ms_total;
    float ms_dist, ms_kernel, ms_contract; /* phases of the evaluation (0 when fused) */
} mrbf_eval_info;

/* per-GPU context: stream, rocBLAS handle, grow-only workspace arena.
 * device_id < 0 selects the current device. */
int32_t mrbf_init(int32_t device_id, mrbf_ctx **ctx);
int32_t mrbf_shutdown(mrbf_ctx *ctx);
const char *mrbf_last_error(const mrbf_ctx *ctx); /* ctx may be NULL: last init error */
const char *mrbf_version(void);
int32_t mrbf_set_option(mrbf_ctx *ctx, int32_t key, double value);
int32_t mrbf_get_option(const mrbf_ctx *ctx, int32_t key, double *value);
/* run on the caller's hipStream_t (e.g. torch's current stream); NULL restores the ctx's own stream */
int32_t mrbf_set_stream(mrbf_ctx *ctx, void *hip_stream);
int32_t mrbf_sync(mrbf_ctx *ctx);

/* Phi (n x n) and Pi (n x q) -- replaces RBF.get_matrices(phi, centers; poly_deg)
 * (src/models/RbfModel.jl:374-375).  Pi_out may be NULL.  *ms (may be NULL)
 * receives the hipEvent time of the assembly kernels alone. */
int32_t mrbf_gram(mrbf_ctx *ctx, int64_t n, int32_t d, const double *centres, int32_t kernel_id, double a, double b,
                  int32_t poly_deg, double *Phi_out, double *Pi_out, float *ms);

/* rectangular kernel block K[i][j] = phi(||x_i - c_j||), m x n row-major -- replaces the per-candidate
 * kernels(xi) / RBF.make_kernel calls of the round-4 site selection (src/models/RbfModel.jl:421, :487): all candidates
 * against all current and prospective centres in one launch (difference-form arithmetic, like norm(x - c)). */
int32_t mrbf_cross_gram(mrbf_ctx *ctx, int64_t m, int64_t n, int32_t d, const double *X, const double *centres, int32_t kernel_id,
                        double a, double b, double *K_out);

/* Gram assembly + factorisation + solve for all k outputs -- replaces
 * RBF.RBFInterpolationModel(sites, values, kernel, params, poly_deg) in update_model
 * (src/models/RbfModel.jl:759-763).  Keeps centres / weights resident on the device in
 * *model.  weights_out (n x k), poly_out (q x k) and info may be NULL. */
int32_t mrbf_fit(mrbf_ctx *ctx, int64_t n, int32_t d, int32_t k, const double *centres, const double *values,
                 int32_t kernel_id, double a, double b, int32_t poly_deg, mrbf_model **model, double *weights_out,
                 double *poly_out, mrbf_fit_info *info);

/* build a model from known coefficients (no solve): lets a caller that kept the
 * round-4 factors (RbfModel.jl:657-660 note) or a checkpoint skip the fit */
int32_t mrbf_model_from_coeffs(mrbf_ctx *ctx, int64_t n, int32_t d, int32_t k, const double *centres,
                               const double *weights, const double *poly, int32_t kernel_id, double a, double b,
                               int32_t poly_deg, mrbf_model **model);

/* values and Jacobians at m points, all k outputs in one sweep -- replaces
 * model(x), model(x, l), RBF.grad(model, x, l), RBF.jac(model, x, rows)
 * (src/models/RbfModel.jl:783-800) and the per-output closures of
 * _get_optim_handle (src/AbstractSurrogateInterface.jl:98-106).
 * vals_out (m x k) or jac_out (m x [k x d col-major]) may be NULL. */
int32_t mrbf_eval(mrbf_ctx *ctx, const mrbf_model *model, int64_t m, const double *X, double *vals_out,
                  double *jac_out, mrbf_eval_info *info);

/* model Hessians at m points: the second derivative of model(x, l) with respect to the scaled site, for the selected outputs l --
 * what a caller of the reference obtains by differentiating RBF.grad(model, x, l) / get_gradient (src/models/RbfModel.jl:792-795)
 * once more; neither the reference nor its RBF package has a method for it, so there is no reference method to fall back to and
 * no decision-table row: the call takes every d the library takes.
 *     H_l(x) = sum_c w_cl [ psi(s_c) I + chi(s_c) (x - c)(x - c)' ],  s_c = |x - c|^2,  psi = phi'/rho,  chi = (phi'' - phi'/rho)/rho^2
 * in difference form for every radial function, on the coordinates as given (the polynomial tail has degree <= 1 and contributes
 * nothing).  A centre with s = 0 contributes w psi(0) I -- psi(0) as in mrbf_eval's Jacobian: the limit, or 0 where none exists --
 * and no rank-one term.
 * rows: n_rows 0-based output indices, any order, repeats allowed (repeated rows give identical blocks); NULL with n_rows = 0: all
 * k outputs (r = k).  hess_out: m x r x d x d doubles, per point and selected output one d x d block; both triangles are written,
 * the mirrored entry with the bits of its twin, so a block reads the same row-major and in Julia's column-major order.  X and
 * hess_out may each be host or device memory; a device hess_out may start on any double.  m = 0: nothing to do, 0.
 * Returns, and writes nothing: -1 no context; -2 NULL model; -4 a model of another context (mrbf_eval_batch's code); -3 m < 0;
 * -5 n_rows < 0, or n_rows > 0 with NULL rows; -6 a row outside [0, k); with m > 0 also -4 NULL X and -7 NULL hess_out.
 * The centre range is split over workgroups where the queries alone would not fill the device; the split count is a function of
 * (m, n, d, r) alone (info->nsplit), the pieces are added in a fixed order, and for a given split count a query's blocks do not
 * depend, bit for bit, on its position in X or on the other queries.  The same call twice gives the same bits.
 * A host hess_out is staged through one grow-only work buffer in chunks of whole query points of at most 256 MiB (one point beyond
 * that is a chunk of its own; info->chunks); results do not depend on the limit, and a second identical call allocates nothing.
 * mrbf_eval_hessian_limited is the same call with that limit as an argument (stage_bytes <= 0: 256 MiB): for tests. */
typedef struct {
    float ms_total;   /* hipEvent time of the launches and read-backs on the ctx stream */
    int32_t nsplit;   /* pieces the centre range was split into */
    int32_t chunks;   /* chunks of query points the result was staged in (1 for a device hess_out) */
    int32_t reserved;
} mrbf_hess_info;
int32_t mrbf_eval_hessian(mrbf_ctx *ctx, const mrbf_model *model, int64_t m, const double *X, int32_t n_rows, const int32_t *rows,
                          double *hess_out, mrbf_hess_info *info);
int32_t mrbf_eval_hessian_limited(mrbf_ctx *ctx, const mrbf_model *model, int64_t m, const double *X, int32_t n_rows,
                                  const int32_t *rows, double *hess_out, mrbf_hess_info *info, int64_t stage_bytes);

/* all step sizes of the Armijo backtracking loop in one batch -- replaces the
 * sequential loop of _backtrack (src/descent.jl:150-185) with condition
 * _armijo_condition (src/descent.jl:137-143).  Evaluates x + step0*shrink^i*dir,
 * i = 0..max_loops, and returns the first i that satisfies the condition (or the
 * index at which the reference loop would have stopped).  x_plus (d), mx_plus (k),
 * step (d) and n_loops are outputs (host or device). */
int32_t mrbf_backtrack(mrbf_ctx *ctx, const mrbf_model *model, const double *x, const double *dir, double step0,
                       double omega, int32_t strict, double const_rhs, double shrink, double min_stepsize,
                       int32_t max_loops, double *x_plus, double *mx_plus, double *step, int32_t *n_loops);

/* ---- rounds 1-2 of the training-site selection: the candidate scan of the affinely-independent-point filter ------------
 * val(xi) = || Z (Z' (xi - x0)) ||_p for all candidates at once and the first maximiser -- replaces the loop over
 * filter.candidate_indices in Base.iterate(::AffinelyIndependentPointFilter, n) (src/models/AffinelyIndependentPoints.jl:71-106).
 * shifted: mc x d row-major rows xi - x0 (host or device; already chosen sites: pass a zero row); Z: d x dz column-major, the
 * p-normalised complement basis of AffinelyIndependentPoints.jl:4-12 (the caller's d x d QR); p_is_inf: 1 = inf-norm (the
 * filter's default in _find_suitable_points, RbfModel.jl:226), 0 = 2-norm.  vals_out (mc) may be NULL. */
int32_t mrbf_affine_scores(mrbf_ctx *ctx, int64_t mc, int32_t d, int32_t dz, const double *shifted, const double *Z, int32_t p_is_inf,
                           double *vals_out, int64_t *argmax, double *maxval);
/* The whole pick loop of the filter in one call (round 6): from the directions chosen so far -- Q0, d x d column-major, an orthogonal
 * matrix whose first j0 columns span them (the Q of qr(Y), full; NULL with j0 = 0) -- pick up to max_picks further candidates, each
 * time the first maximiser of || Z (Z' (xi - x0)) ||_p while that exceeds pivot_val (AffinelyIndependentPoints.jl:71-106), with the
 * Householder factorisation of Y = [chosen directions] grown by one reflector per pick on the device instead of qr(Y) from scratch
 * after every pick (:59-60, :93-94): O(d^2 + d mc) per pick, no host round trip between picks.  shifted: mc x d row-major rows
 * xi - x0 (host or device; sites chosen already: zero rows).  picked_out[max_picks]: positions of the picked candidates in pick order;
 * Z_out (d x (d - j0 - *n_picked), column-major, host or device, may be NULL): the p-normalised complement basis afterwards -- the
 * filter's final Z (its improving directions, RbfModel.jl:231-235).
 * Which d takes which form (1 <= d <= 4096; d > 4096: -3, nothing written):
 *   inf-norm, d <= 1023          one launch per pick (affsel_pick_kernel; 8 (d + 1) + 8 * 1024 doubles of LDS, 128 KiB at d = 1023)
 *   2-norm d <= 1024; inf-norm d = 1024
 *                                three launches per pick (score / decide / update); the score kernel asks for 8 (d - j0) doubles of
 *                                dynamic LDS plus 2 KiB static: 66 KiB at d - j0 = 1024, which the runtime grants a launch as it stands
 *                                (it reports 160 KiB per workgroup on gfx950; tests/test_gpu_select_wide.py, cases C11 and C12)
 *   d >= 1025                    rocBLAS for the two products, the decide / update kernels unchanged */
int32_t mrbf_affine_select(mrbf_ctx *ctx, int64_t mc, int32_t d, const double *shifted, int32_t j0, const double *Q0, int32_t max_picks,
                           double pivot_val, int32_t p_is_inf, int64_t *picked_out, int32_t *n_picked, double *Z_out);

/* The pick loop for a batch of starts in one call (affine.hip): rounds 1-2 of the training-site selection of n_starts independent
 * starts -- the filter loops (src/models/AffinelyIndependentPoints.jl:71-106, called by _find_suitable_points, RbfModel.jl:205-238)
 * inside the reference's Threads.@threads loop over starts (examples/large_scale_benchmarks.jl:102-109, :253).  For every start p,
 * the values of picked_out, n_picked and Z_out are, bit for bit, those of mrbf_affine_select(ctx, mc_p, d, shifted_p, j0_p, Q0_p,
 * max_picks_p, pivot_p, p_is_inf, ...); they do not depend on the start's position in the batch or on which other starts share it.
 * One launch per pick serves all starts (start p works at j = j0_p + t in launch t and sits out once it is done or has its
 * max_picks picks), the host looks at the starts' "done" words every sixteen launches and reads counts and pick lists back once.
 * The starts share d and the norm.  Returns -2 (take mrbf_affine_select per start, or the host filter) and writes nothing when
 * mrbf_dispatch_affine_batch refuses the shape; an invalid field of a job is an invalid `jobs` (-5).  At most 2^26 candidates in
 * all.  ms_total (may be NULL): hipEvent time of the chain on the ctx stream, without the final copies of Z_out. */
typedef struct {
    int64_t mc;            /* candidates of this start; 0: nothing to pick */
    int32_t j0;            /* directions chosen so far, 0 .. d */
    int32_t max_picks;     /* clipped to d - j0 */
    double pivot_val;
    const double *shifted; /* mc x d row-major, host or device; chosen sites: zero rows */
    const double *Q0;      /* d x d column-major, host or device; NULL with j0 = 0 */
    int64_t *picked_out;   /* host, max_picks entries (may be NULL when max_picks = 0) */
    double *Z_out;         /* d x (d - j0 - n_picked) column-major, host or device, may be NULL */
    int32_t n_picked;      /* out */
    int32_t reserved;
} mrbf_affine_job;
int32_t mrbf_affine_select_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, int32_t p_is_inf, mrbf_affine_job *jobs,
                                 float *ms_total);

/* ---- round 4 of the training-site selection on the device, with factor reuse -------------------------------------------
 * mrbf_round4 replaces _rbf_round4 (src/models/RbfModel.jl:352-499): start_sites (n0 x d, the sites found so far -- centre and
 * rounds 1-3 -- which must carry the polynomial tail: n0 >= q, full rank) and cand_sites (mc x d, the database candidates in
 * database order; with use_max_points the caller appends the random box points of :405-416) -> positions (into cand_sites) of
 * the accepted sites in acceptance order.  Acceptance test as in the reference: tau^2 > (theta_pivot_cholesky^2)^2 (:370, :452),
 * at most max_points sites in total (<= 0: (d+1)(d+2)/2, :356).  The kernel vectors of ALL candidates, the reference's
 * kernels(xi) / get_matrices calls (:374, :421), are three batched launches; the selection is a left-looking Cholesky
 * factorisation that skips the rejected columns (round4.hip).  *state (may be NULL) keeps the factors.
 * mrbf_fit_from_round4: the model on (start sites, accepted sites) -- values ((n0 + n_accepted) x k row-major, in that order)
 * -- from the kept factor instead of a new factorisation (the reference's TODO at RbfModel.jl:657-660); needs n0 == q
 * (returns -2 otherwise: use mrbf_fit).  info.path = MRBF_PATH_ROUND4. */
typedef struct mrbf_round4_state mrbf_round4_state;
int32_t mrbf_round4(mrbf_ctx *ctx, int64_t n0, int32_t d, const double *start_sites, int64_t mc, const double *cand_sites,
                    int32_t kernel_id, double a, double b, int32_t poly_deg, int32_t max_points, double theta_pivot_cholesky,
                    int32_t *accepted_out, int32_t *n_accepted, mrbf_round4_state **state);
int32_t mrbf_fit_from_round4(mrbf_ctx *ctx, const mrbf_round4_state *state, int32_t k, const double *values, mrbf_model **model,
                             double *weights_out, double *poly_out, mrbf_fit_info *info);
int32_t mrbf_round4_sites(const mrbf_round4_state *state, int64_t *n0, int64_t *n_candidates, int32_t *n_accepted);
int32_t mrbf_free_round4(mrbf_ctx *ctx, mrbf_round4_state *state);

/* ---- many-start round 4: the site selection of a batch of small starts in one call (round4_small.hip) ------------------------
 * _rbf_round4 (src/models/RbfModel.jl:352-499) for n_starts independent starts -- the reference's Threads.@threads loop over starts
 * (examples/large_scale_benchmarks.jl:102-109, :253) -- on ONE context.  For every start p, accepted_out and n_accepted are the list
 * mrbf_round4(ctx, n0_p, d, start_sites_p, mc_p, cand_sites_p, ...) returns: the same acceptance test, tau^2 > (theta_pivot_cholesky^2)^2
 * with at most max_points sites in all (<= 0: (d+1)(d+2)/2), walked in candidate order by a kernel of its own for the small shape (one
 * workgroup per start, right-looking; the sums run in another order than the blocked walk's, so a decision that sits on the threshold
 * to within rounding may differ).  A start's list does not depend on its position in the batch or on which other starts share it.
 * NO FACTOR STATE IS KEPT: there is no mrbf_round4_state to hand to mrbf_fit_from_round4; the fits of a batch go through
 * mrbf_fit_batch.  Nothing of the call outlives it (MRBF_OPT_LIVE_HANDLES is unchanged; the workspace is the context's arena).
 * The small range -- starts that share six launches whose grids span all of them, one packed descriptor upload and one read-back:
 *   d <= 128,  q <= n0 <= 256,  1 <= mc <= 4096,  min(mc, max_points - n0) <= 256 (the resulting model is in mrbf_fit_batch's one-launch
 *   range), and at most 2 GiB of workspace for the batch.
 * Every other start of an otherwise valid batch (and a start whose start set the batched chain finds rank deficient) runs mrbf_round4
 * inside the call, after the batched chain, with state = NULL; what that returned is the start's rc (read it with
 * mrbf_dispatch_after(MRBF_ENTRY_ROUND4_BATCH, rc): -2 / MRBF_ESINGULAR = take the host mirror for this start).  One such start does
 * not fail the others.  The call returns 0 unless an argument is invalid (an invalid field of a job is an invalid `jobs`: -4) or
 * mrbf_dispatch_round4_batch refuses the shape (-2: take mrbf_round4 per start; nothing is written).  ms_total (may be NULL): hipEvent
 * time of the batched chain on the ctx stream, without the starts that took the single call. */
typedef struct {
    int64_t n0, mc;                 /* start sites, candidates (mc = 0: nothing to do) */
    const double *start_sites;      /* n0 x d row-major, host or device */
    const double *cand_sites;       /* mc x d row-major, host or device, database order */
    int32_t kernel_id, poly_deg;
    double a, b;
    int32_t max_points;
    double theta_pivot_cholesky;
    int32_t *accepted_out;          /* host, min(mc, max_points - n0) entries */
    int32_t n_accepted;             /* out */
    int32_t rc;                     /* out: 0, or what mrbf_round4 returned for a start that took it */
} mrbf_round4_job;                  /* 88 bytes */
int32_t mrbf_round4_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_round4_job *jobs, float *ms_total);

int32_t mrbf_model_dims(const mrbf_model *model, int64_t *n, int32_t *d, int32_t *k, int32_t *q);
int32_t mrbf_free_model(mrbf_ctx *ctx, mrbf_model *model);

/* many-problem mode (the reference's Threads.@threads loop over independent
 * problems, examples/large_scale_benchmarks.jl:253): problem p runs on device
 * device_ids[p % n_dev] (device_ids == NULL: devices 0 .. n_dev-1), one host
 * thread + pooled ctx per entry of device_ids inside this process (entries may
 * repeat: {0, 0} is two workers on GPU 0), fit + eval per problem, one
 * fixed-size result record per problem; a failing problem sets `status` on its
 * own record only, the call itself returns 0 unless an argument is invalid or
 * a device cannot be initialised.
 * Every buffer of a problem may be a HOST pointer or a DEVICE pointer (detected
 * per pointer, as in mrbf_fit / mrbf_eval; outputs given as device pointers are
 * written in place, without a host round trip).  With n_dev > 1 a DEVICE buffer
 * of problem p must live on device_ids[p % n_dev], the device that runs it --
 * the library does no peer access; host buffers have no such constraint. */
typedef struct {
    int64_t n, m;
    int32_t d, k, kernel_id, poly_deg;
    double a, b;
    const double *centres; /* host or device, n x d row-major */
    const double *values;  /* host or device, n x k row-major */
    const double *X;       /* host or device, m x d row-major (may be NULL when m == 0) */
    double *weights_out;   /* host or device n x k, or NULL */
    double *poly_out;      /* host or device q x k, or NULL */
    double *vals_out;      /* host or device m x k, or NULL */
    double *jac_out;       /* host or device m x (k x d column-major blocks), or NULL */
} mrbf_problem;

typedef struct {
    int32_t status;   /* return code of the failing call, 0 if ok */
    int32_t device;   /* GPU that ran it */
    mrbf_fit_info fit;
    float ms_eval;
    double checksum_w;    /* sum of weights: order-fixed reduction on the device for the problems of the batched small-problem path
                             (batch.hip), a host loop over the output buffer for problems on the per-problem chain */
    double checksum_vals; /* sum of values, likewise */
} mrbf_result;

int32_t mrbf_batch_run(int32_t n_dev, const int32_t *device_ids, int64_t n_problems, const mrbf_problem *problems,
                       mrbf_result *results);

/* ---- many-start model update: one call fits a batch of starts and keeps the models (batch.hip) -----------------------------
 * update_model (src/models/RbfModel.jl:743-767) for n_starts independent starts -- the reference's Threads.@threads loop over
 * starts (examples/large_scale_benchmarks.jl:102-109, :253) -- on ONE context.  For every start p, weights_out, poly_out and every
 * later result computed from jobs[p].model (mrbf_eval values and Jacobians, the start's outputs and record of
 * mrbf_sd_iterate_batch) are, bit for bit, those of mrbf_fit on that start's arguments on the same context; they do not depend on
 * the start's position in the batch or on which other starts share it.  info.path, fallbacks, n and q equal the single call's;
 * rel_residual and max_pitw come from the batch's own check kernel (same quantities, sums in another order).
 * Starts in the range of the one-launch fit (n <= the context's MRBF_OPT_SMALL_FIT_MAX_N, d <= 128, k <= 16, Cholesky paths) share a handful of launches whose grids
 * span all of them, one packed descriptor upload and one read-back; every other start, and a start whose batched fit raised a flag
 * (not positive definite, rank-deficient tail), takes mrbf_fit inside the same call.
 * With MRBF_OPT_SMALL_LU at 1 the starts on the LU path inside that option's range share launches of their own in the same way (one
 * descriptor upload, one LU launch, the residual evaluations and the check kernel, one read-back; their models live in the call's
 * allocation as well); a singular start among them gets status MRBF_ESINGULAR and no model, and does not disturb its neighbours.
 * mrbf_batch_run does not look at the option.
 * Lifetime: jobs[p].model is a handle like any other -- mrbf_eval, mrbf_sd_iterate_batch, mrbf_ps_step_problem, mrbf_model_dims
 * accept it, MRBF_OPT_LIVE_HANDLES counts it, and the caller releases it with mrbf_free_model, in any order.  The models of one
 * call that took the batched path are carved from one device allocation of that call; each holds a share, and the allocation goes
 * back to the context's pool of released model blocks (or to the device) when the last of them is freed: device memory of a batch
 * is reusable only once ALL its models are released.
 * A failing start sets its own status and leaves its model NULL; the call returns 0 unless an argument is invalid (an invalid field
 * of a job is an invalid `jobs`: -3) or mrbf_dispatch_fit_batch refuses n_starts (-2: take mrbf_fit per start; nothing is written).
 * ms_total (may be NULL): hipEvent time of the batched launches plus info.ms_total of the starts that took the single call. */
typedef struct {
    int64_t n;
    int32_t d, k, kernel_id, poly_deg;
    double a, b;
    const double *centres, *values;   /* n x d, n x k row-major; host or device (detected per pointer) */
    double *weights_out, *poly_out;   /* n x k, q x k; host or device; may be NULL */
    mrbf_model *model;                /* out: the resident model; NULL when status != 0 */
    int32_t status;                   /* out: what mrbf_fit would have returned for this start */
    int32_t reserved;
    mrbf_fit_info info;               /* out */
} mrbf_fit_job;                       /* 168 bytes */
int32_t mrbf_fit_batch(mrbf_ctx *ctx, int64_t n_starts, mrbf_fit_job *jobs, float *ms_total);

/* ---- many-start evaluation: one call evaluates a batch of kept models (eval_batch.hip, host logic in eval_batch_host.hpp) -----
 * mrbf_eval for n_jobs independent (model, query block) pairs on ONE context: m(x) and m(x_+) of every start for the acceptance
 * test of iterate! (src/algorithm.jl:766-767), the container sweeps eval_container_*_at_scaled_sites
 * (src/SurrogateContainer.jl:234-269) of every start, and plain evaluation of the models mrbf_fit_batch keeps for the reference's
 * Threads.@threads loop over starts (examples/large_scale_benchmarks.jl:102-109).  For every job, vals_out and jac_out are, bit for
 * bit, what mrbf_eval(ctx, model, m, X, vals_out, jac_out, NULL) writes on the same context; they do not depend on the job's
 * position or on which other jobs share the call.  No evaluation arithmetic of its own: the call fills the descriptor arrays of the
 * single call's kernels, every job with the centre-range split of the single call it stands for.
 * Models may come from mrbf_fit, mrbf_fit_batch, mrbf_fit_from_round4 or mrbf_model_from_coeffs, may appear in several jobs, and may
 * differ in n, d, k, kernel and parameters.  Jobs the fused kernels take (dpad in {64, 128, 256}, MRBF_OPT_EVAL_IMPL != 1) share
 * launches: one group per (kernel and parameters, k, dpad, with or without Jacobians, split or unsplit centre range), a non-smooth
 * group in the difference form; every other job runs the single call's chain on the same stream inside the call.
 * One packed upload (descriptors + all host-side query rows), one read-back (all host-side outputs), one synchronisation.  Device-side
 * X / vals_out / jac_out are read and written in place (the descriptors carry their addresses): no copy, no host round trip.  The
 * work buffer is one slot of the context's arena: a second identical call allocates nothing.  A call whose work buffer would exceed
 * 2 GiB is processed in chunks of consecutive jobs inside the call (then: one upload, read-back and synchronisation per chunk).
 * m == 0 jobs write nothing; a job with both outputs NULL does nothing.  Every job's status is set (0 on success).
 * Returns 0; -1 without a context; -3 for an invalid job (NULL model, m < 0, NULL X with m > 0; `jobs` NULL): nothing is launched or
 * written; -4 for a model of another context or device (likewise); -2, and only -2, when mrbf_dispatch_eval_batch refuses n_jobs:
 * take mrbf_eval per job.  ms_total (may be NULL): hipEvent time of the whole call.
 * mrbf_eval_batch_limited is the same call with the 2 GiB limit of the chunk rule as an argument (arena_limit_bytes <= 0: 2 GiB): for
 * tests of the chunk path; the results do not depend on it. */
typedef struct {
    const mrbf_model *model;
    int64_t m;
    const double *X;     /* m x d row-major, host or device (detected per pointer); may be NULL when m == 0 */
    double *vals_out;    /* m x k, host or device, or NULL */
    double *jac_out;     /* m x (k x d column-major blocks), host or device, or NULL */
    int32_t status;      /* out: what mrbf_eval would have returned for this job */
    int32_t reserved;
} mrbf_eval_job;         /* 48 bytes */
int32_t mrbf_eval_batch(mrbf_ctx *ctx, int64_t n_jobs, mrbf_eval_job *jobs, float *ms_total);
int32_t mrbf_eval_batch_limited(mrbf_ctx *ctx, int64_t n_jobs, mrbf_eval_job *jobs, float *ms_total, int64_t arena_limit_bytes);

/* ---- many-start model Hessians: one call for a batch of kept models (hess.hip, host logic in hess_batch_host.hpp) ------------
 * mrbf_eval_hessian for n_jobs independent (model, site block) pairs on ONE context: the second derivative of every start's model at
 * its own iterate, for the reference's Threads.@threads loop over starts (examples/large_scale_benchmarks.jl:102-109) around a
 * method the reference does not have (the derivative of get_gradient, src/models/RbfModel.jl:792-800, taken once more).
 * For every job, hess_out is, bit for bit, what mrbf_eval_hessian(ctx, model, m, X, n_rows, rows, hess_out, NULL) writes on the same
 * context; it does not depend on the job's position, on which other jobs share the call, or on the limit below.  Every job keeps the
 * split count of the single call it stands for (job.nsplit: a function of its own m, n, d, r), the same piece length and the same
 * order of adding the pieces: no arithmetic of its own, the single call's two kernel bodies behind a descriptor array and a table of
 * first block indices in which a workgroup finds its descriptor.  The price: every job splits as if it were alone on the device.
 * Models may come from mrbf_fit, mrbf_fit_batch, mrbf_fit_from_round4 or mrbf_model_from_coeffs, may appear in several jobs, and may
 * differ in n, d, k, kernel and parameters.  Jobs share launches by template instantiation alone -- (radial function, fast form,
 * outputs per pass) for the main kernel, outputs per pass for the combining kernel --, so starts of one radial function and one r
 * take one main launch and at most one combining launch whatever their n.  A job beyond 2^30 blocks is cut by points as the single
 * call cuts it.
 * One packed upload (descriptors, block tables, row lists, all host-side query rows), one read-back (all host-side results), one
 * synchronisation.  Device-side X / hess_out are read and written in place (the descriptors carry their addresses).  The work
 * buffer is one slot of the context's arena: a second identical call allocates nothing.  A call whose work buffer would exceed
 * 2 GiB is processed in chunks of consecutive jobs (then: one upload, read-back and synchronisation per chunk); a single job beyond
 * the limit runs the single call's chain, with its 256 MiB staging rule, inside the call (info->single_inside).
 * m == 0 jobs write nothing and have status 0.
 * Returns 0; -1 without a context; -2, and only -2, when mrbf_dispatch_hessian_batch refuses n_jobs: take mrbf_eval_hessian per
 * job; -3 for an invalid job (`jobs` NULL; NULL model; m < 0; n_rows < 0; n_rows > 0 with NULL rows; a row outside [0, k); with m > 0
 * NULL X or NULL hess_out): nothing is launched or written, and every job's status holds the single call's own code (-2, -3, -5, -6,
 * -4, -7; 0 for a valid job); -4 for a model of another context (likewise nothing launched or written); -3 goes in front of -4.
 * info may be NULL.  mrbf_eval_hessian_batch_limited is the same call with the 2 GiB limit of the chunk rule as an argument
 * (arena_limit_bytes <= 0: 2 GiB): for tests of the chunk path; the results do not depend on it. */
typedef struct {
    const mrbf_model *model;
    int64_t m;
    const double *X;        /* m x d row-major, host or device (detected per pointer); may be NULL when m == 0 */
    const int32_t *rows;    /* host memory: n_rows 0-based outputs, any order, repeats allowed; NULL with n_rows = 0: all k */
    double *hess_out;       /* m x r x d x d, host or device (a device buffer may start on any double); may be NULL when m == 0 */
    int32_t n_rows;
    int32_t status;         /* out: what mrbf_eval_hessian would have returned for this job */
    int32_t nsplit;         /* out: pieces of this job's centre range (0 when nothing ran) */
    int32_t reserved;
} mrbf_hess_job;            /* 56 bytes */
typedef struct {
    float ms_total;         /* hipEvent time of the whole call on the ctx stream */
    int32_t chunks;         /* upload / launch / read-back rounds the call took */
    int32_t groups;         /* kernel groups launched, summed over the chunks */
    int32_t single_inside;  /* jobs that ran the single call's chain inside the call */
} mrbf_hess_batch_info;     /* 16 bytes */
int32_t mrbf_eval_hessian_batch(mrbf_ctx *ctx, int64_t n_jobs, mrbf_hess_job *jobs, mrbf_hess_batch_info *info);
int32_t mrbf_eval_hessian_batch_limited(mrbf_ctx *ctx, int64_t n_jobs, mrbf_hess_job *jobs, mrbf_hess_batch_info *info,
                                        int64_t arena_limit_bytes);

/* ---- resident site database: box scan and gathers for many-start updates (db.hip, host logic in db_host.hpp) -----------------
 * A start's evaluation database -- the ArrayDB of src/Databases.jl: sites (d) and values (k), rows in insertion order, a row's
 * position being its id -- kept on the device and appended to as the run goes, so that the batched calls above read their inputs from
 * device memory instead of a fresh host array per start and call.  All indices are 0-based positions in database order, like
 * accepted_out and picked_out.  MRBF_OPT_LIVE_HANDLES counts databases; MRBF_OPT_ARENA_BYTES does not: a database owns its own
 * allocation, which grows geometrically (db_host.hpp: twice the capacity, at least what is needed, at least 64 rows).
 *   mrbf_db_create      an empty database (init_db, Databases.jl:41-54); capacity_hint rows are allocated at once (<= 0: on first use).
 *   mrbf_db_append      new_result!(db, x, y) (Databases.jl:174-186) for m rows: sites m x d, values m x k row-major, host or device;
 *                       values == NULL: the rows are unevaluated and stored as NaN -- new_result!(db, p, F[]) of round 3,
 *                       RbfModel.jl:303.  Grows the allocation when needed; earlier rows keep their bits.  *first_index (may be NULL):
 *                       the position of the first new row.
 *   mrbf_db_set_values  eval_missing! (Databases.jl:258-277): the values (m x k row-major, host or device) of the rows `indices`
 *                       (host, m distinct positions; one out of range: -4, nothing written).
 *   mrbf_db_read        rows first .. first + m - 1 to sites_out (m x d) / values_out (m x k), host or device, either may be NULL:
 *                       get_sites / get_values (Databases.jl:128-137).
 *   mrbf_db_dims        n_sites, d, k (any may be NULL).
 *   mrbf_db_free        releases the allocation; views into the database (below) end with it. */
typedef struct mrbf_db mrbf_db;   /* one start's database: sites (d) and values (k), rows in insertion order (ArrayDB ids) */
int32_t mrbf_db_create(mrbf_ctx *ctx, int32_t d, int32_t k, int64_t capacity_hint, mrbf_db **db);
int32_t mrbf_db_append(mrbf_ctx *ctx, mrbf_db *db, int64_t m, const double *sites, const double *values, int64_t *first_index);
int32_t mrbf_db_set_values(mrbf_ctx *ctx, mrbf_db *db, int64_t m, const int64_t *indices, const double *values);
int32_t mrbf_db_read(mrbf_ctx *ctx, const mrbf_db *db, int64_t first, int64_t m, double *sites_out, double *values_out);
int32_t mrbf_db_dims(const mrbf_db *db, int64_t *n_sites, int32_t *d, int32_t *k);
int32_t mrbf_db_free(mrbf_ctx *ctx, mrbf_db *db);

/* The box scan for a batch of starts: results_in_box_indices (src/Databases.jl:324-327) as called by _find_suitable_points
 * (src/models/RbfModel.jl:214) and _rbf_round4 (:360), the shifted seeds xi - x0 of the filter (AffinelyIndependentPoints.jl:25)
 * and its first pick, findmax(norm.(shifted_seeds, p)) (:53), for n_starts databases of one d in four launches whose grids span all
 * starts, with one packed descriptor upload and one read-back.
 * Candidate i is in the box iff i is not in `exclude` and lb[j] <= site[i][j] <= ub[j] for all j: inclusive comparisons, a NaN
 * coordinate fails them, infinite bounds work.  Candidates come out in ascending database order (a scan of per-block counts, no
 * atomics).  A shifted row is site - x0, one fp64 subtraction per element.  first_pick: the position among the candidates of the
 * first maximiser of ||xi - x0||_p (p_is_inf: 1 = inf-norm, 0 = 2-norm as sqrt of the sum of squares); the lowest position wins ties,
 * the pivot value is not consulted; -1 when mc = 0.  With zero_first_pick != 0 that row of shifted_dev (and of shifted_out) is zero
 * afterwards and first_row still holds it: the state mrbf_affine_select[_batch] expects ("chosen sites: zero rows").
 * Lifetime of the views: cand_sites_dev and shifted_dev point into memory of the context and stay valid until the next
 * mrbf_db_box_batch on the same context; sites_dev and values_dev of mrbf_db_gather_batch until the next mrbf_db_gather_batch on it;
 * box views and gather views do not disturb each other, and no other entry point writes to either (the batched calls copy their
 * inputs into their own arena).  A database's release or the context's shutdown also ends them.
 * A database may appear at most once per batch call.  Returns 0; -2 (do it on the host; nothing is written) when
 * mrbf_dispatch_db_batch refuses the shape; an invalid field of a job is an invalid `jobs` (-5; mrbf_db_gather_batch: -4).  A job
 * that fails sets its own rc, leaves its outputs untouched and does not fail the others.  ms_total (may be NULL): hipEvent time of
 * the launches and the read-back on the ctx stream, without the copies to sites_out / shifted_out. */
typedef struct {
    mrbf_db *db;
    const double *lb, *ub, *x0;     /* host, d doubles each */
    int64_t n_exclude;
    const int64_t *exclude;         /* host; duplicates allowed, entries outside [0, n_sites) ignored; NULL with n_exclude = 0 */
    int32_t zero_first_pick;
    int32_t rc;                     /* out */
    int64_t *indices_out;           /* host, room for n_sites entries; may be NULL */
    double *sites_out, *shifted_out; /* host or device, mc x d row-major (room for n_sites x d); may be NULL */
    double *first_row;              /* host, d doubles: the first pick's shifted row (untouched when mc = 0) */
    int64_t mc;                     /* out: candidates in the box */
    int64_t first_pick;             /* out */
    const double *cand_sites_dev;   /* out: device, mc x d row-major, database order */
    const double *shifted_dev;      /* out: device, mc x d row-major */
} mrbf_db_box_job;                  /* 120 bytes */
int32_t mrbf_db_box_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, int32_t p_is_inf, mrbf_db_box_job *jobs, float *ms_total);

/* Row gathers for a batch of starts: get_site.(db, indices_found_so_far) of round 4 (RbfModel.jl:372) and the training set of the
 * fit (get_site / get_value over _collect_indices(meta), RbfModel.jl:747-757) in one launch, with one packed upload of the index
 * lists.  indices: host, any order, repeats allowed; an index outside [0, n_sites) sets the job's rc to -3 and leaves its outputs
 * untouched.  sites_dev (n_idx x d) and values_dev (n_idx x k) come in the order of `indices`. */
typedef struct {
    mrbf_db *db;
    int64_t n_idx;
    const int64_t *indices;         /* host */
    double *sites_out, *values_out; /* host or device, n_idx x d / n_idx x k; may be NULL */
    const double *sites_dev;        /* out: device, n_idx x d row-major */
    const double *values_dev;       /* out: device, n_idx x k row-major */
    int32_t rc;                     /* out */
    int32_t reserved;
} mrbf_db_gather_job;               /* 64 bytes */
int32_t mrbf_db_gather_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_db_gather_job *jobs, float *ms_total);

/* mrbf_db_append and mrbf_db_set_values for a batch of starts (db.hip): one packed upload, one launch whose grid spans all starts and
 * one synchronisation per call, whatever n_starts -- the trial points of an iteration and eval_missing! of every start.  Every
 * database is left bit-identical to the per-start calls.  sites / values: host or device (detected per pointer; device rows are read
 * in place); indices: host, distinct positions.  A database may appear at most once per call; the databases may differ in d and k.
 * Returns 0; -2 (nothing written) when mrbf_dispatch_db_batch(n_starts, 1) refuses the batch; an invalid field of a job is an invalid
 * `jobs` (-3).  mrbf_db_set_values_batch: an index outside the database sets that job's rc to -4, nothing of that job is written and
 * the others are not disturbed. */
typedef struct {
    mrbf_db *db;
    int64_t m;
    const double *sites;            /* m x d row-major, host or device */
    const double *values;           /* m x k row-major, host or device; NULL: unevaluated rows, stored as NaN */
    int64_t first_index;            /* out: the position of the first new row */
    int32_t rc;                     /* out */
    int32_t reserved;
} mrbf_db_append_job;               /* 48 bytes */
int32_t mrbf_db_append_batch(mrbf_ctx *ctx, int64_t n_starts, mrbf_db_append_job *jobs, float *ms_total);
typedef struct {
    mrbf_db *db;
    int64_t m;
    const int64_t *indices;         /* host, m distinct positions */
    const double *values;           /* m x k row-major, host or device */
    int32_t rc;                     /* out */
    int32_t reserved;
} mrbf_db_set_values_job;           /* 40 bytes */
int32_t mrbf_db_set_values_batch(mrbf_ctx *ctx, int64_t n_starts, mrbf_db_set_values_job *jobs, float *ms_total);

/* Round 3 of the training-site selection for a batch of starts (round3.hip, host logic in round3_host.hpp): _rbf_round3
 * (src/models/RbfModel.jl:269-307) with the rebuild along the coordinate axes it falls back to (:286-289 -> :633-637), and the
 * improvement step prepare_improve_model (:699-732), written straight into the resident databases.
 * MRBF_R3_UPDATE, per start: n_new = max(0, min(n_missing, max_new)); for i < n_new, len = intersect_box(x, dir_i, lb, ub; :absmax)
 * (utilities.jl:126-221: zero components are skipped, an on-bound component gives Inf or 0 by sign and sense, sigma+ is the minimum
 * of the entries >= 0, sigma- the maximum of the others, NaN included, an empty set gives 0, |sigma+| >= |sigma-| picks; a zero
 * direction gives Inf), offset = len .* dir and the new point x .+ offset, each rounded once.  Direction i fails iff
 * norm(offset, Inf) <= pivot_val (the maximum propagates NaN: a NaN norm does not fail).  If a direction fails and
 * ensure_fully_linear && !force_rebuild, nothing of that attempt is kept and the start is redone inside the call along the
 * coordinate axes with n_new = max(0, min(d, max_new)): status = MRBF_R3_REBUILT, fully_linear = n_new >= d and no axis fails,
 * n_dirs_used = n_new (of the axes).  Otherwise fully_linear = n_new >= n_missing and no direction fails.  (Whether round 2 found
 * sites, RbfModel.jl:631, is the caller's business.)
 * MRBF_R3_IMPROVE: direction 0 alone; its point is appended iff norm(offset, Inf) > pivot_val (:718: a NaN norm appends nothing);
 * n_new is 0 or 1, fully_linear = n_new == 1 && n_dirs == 1, n_dirs_used = min(n_dirs, 1).
 * The n_new points are appended to the start's database in direction order as unevaluated rows (NaN values); first_index is the
 * position of the first; the same rows come back in new_sites_out.  The allocation grows by the rule of mrbf_db_append before the
 * first launch (room for the larger of the first attempt and the rebuild); earlier rows keep their bits.
 * One packed upload, at most four launches whose grids span all starts (two when no job can rebuild), one read-back.
 * Returns 0; -2 (nothing written) when mrbf_dispatch_db_batch refuses the shape; an invalid field, a database of another d or
 * context or one named twice is an invalid `jobs` (-4).  n_dirs < n_new (the reference's @assert, :278; with dirs == NULL n_dirs is
 * d) sets the job's own rc to -3, leaves its outputs and its database untouched and does not fail the others. */
enum { MRBF_R3_UPDATE = 0, MRBF_R3_IMPROVE = 1 };
enum { MRBF_R3_DONE = 0, MRBF_R3_REBUILT = 1 };
typedef struct {
    mrbf_db *db;
    const double *x, *lb, *ub;      /* host, d doubles each: x, lb_1, ub_1 (local_bounds of Delta_1) */
    double pivot_val;               /* piv_val_1 */
    const double *dirs;             /* d x n_dirs column-major, host or device (a Z_out of mrbf_affine_select[_batch] is read in place);
                                       NULL: the coordinate axes, n_dirs = d (force_rebuild, RbfModel.jl:568) */
    int32_t n_dirs, reversed;       /* reversed != 0: direction i is column n_dirs - 1 - i (reverse(eachcol(Z)), :232) */
    int32_t n_missing, max_new;
    int32_t ensure_fully_linear, force_rebuild, mode;
    int32_t rc;                     /* out */
    double *new_sites_out;          /* host, room for max(min(n_missing, max_new), min(d, max_new)) x d; may be NULL */
    int64_t first_index;            /* out: the database position of the first new row */
    int32_t n_new, fully_linear, status, n_dirs_used;   /* out */
} mrbf_round3_job;                  /* 112 bytes */
int32_t mrbf_db_round3_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_round3_job *jobs, float *ms_total);

/* debug / test hooks (exported so the parity tests can pin kernel-level behaviour) */
/* Environment switches.  The library reads a number of MRBF_* variables (schedule experiments of the persistent factorisation,
 * earlier forms of kernels kept selectable for A/B runs, diagnostics: INTEGRATION.md "Tuning knobs").  NONE of them is honoured
 * unless MRBF_EXPERIMENTS=1 is set in the same environment: a stray variable never changes the algorithm of a production run.
 * mrbf_debug_env (host only): 1 if switch `name` is set and the gate is open, else 0. */
int32_t mrbf_debug_env(const char *name);
int32_t mrbf_debug_mfma_layout(mrbf_ctx *ctx, double *out16x16_a_times_b, const double *A16x4, const double *B4x16);
int32_t mrbf_debug_potrf(mrbf_ctx *ctx, int64_t n, double *A_colmajor_inout, int32_t impl, int32_t *info, float *ms);
int32_t mrbf_debug_diag(mrbf_ctx *ctx, const double *A128, int32_t reps, float *ms_per_call, double *shader_cycles,
                        double *realtime_us);
/* micro-benchmarks (tools/microbench.py): sustained f64 MFMA issue rate and the rocBLAS dgemm reference */
int32_t mrbf_debug_mfma_peak(mrbf_ctx *ctx, int32_t blocks_per_cu, int32_t threads, int32_t iters, float *ms, double *tflops);
int32_t mrbf_debug_mfma_asm(mrbf_ctx *ctx, int32_t variant, int32_t blocks_per_cu, int32_t iters, float *ms, double *tflops,
                            double *cycles_per_mfma);
int32_t mrbf_debug_dgemm(mrbf_ctx *ctx, int32_t m, int32_t n, int32_t k, float *ms, double *tflops);
/* Host only (no GPU needed): the job tables of the persistent factorisation for nt block columns / mt block rows and the given
 * schedule parameters, checked against their invariants.  out[0..3] = panel jobs, bulk jobs, chain jobs, windows; out[4] = checksum;
 * out[5] = violated invariants (0 when the tables are consistent).  Returns 0, or -(argument index) for a parameter out of range. */
int32_t mrbf_debug_mega_tables(int32_t nt, int32_t mt, int32_t slack, int32_t slack_chain, int32_t first, int32_t win, int32_t srows,
                               int32_t half_cols, int64_t *out6);
/* The same with the round-4 schedule options: opt5 = { head columns, tail columns of the chain-bound edge regime, block columns at the
 * end whose bulk jobs are 64-row halves, only a tile's last so many windows as halves (0: all), chain tiles' window jobs in queues of
 * their own }.  The last option is a bit field: bit 0 chain tiles' queues; bit 1 streamed tiles of five-row block columns as two 64-row
 * jobs (bits 2..9 / 10..17: only the first / last so many block columns, 0 / 0 = all); bits 18..25 = t + 1: panel tiles more than t
 * block rows below the streamed ones as one 128-row job; bit 26: the block rows below the square hold at most 64 non-zero rows (one
 * job per tile and window on the upper half that publishes for both).  The invariants cover both queue classes, the per-column
 * number of streamed rows and every one of these job shapes (each tile finished / updated exactly once). */
int32_t mrbf_debug_mega_tables2(int32_t nt, int32_t mt, int32_t slack, int32_t slack_chain, int32_t first, int32_t win, int32_t srows,
                                int32_t half_cols, const int32_t *opt5, int64_t *out6);
/* Host only: the schedule the persistent factorisation picks by size alone (no option or switch set) for nt block columns / mt block
 * rows, with xreal > 0 when only so many of the rows below the square are non-zero (the fit's right-hand sides), and its job tables
 * checked.  out39[0..8] = slack, slack_chain, first window, window, streamed rows, half_cols, tail_half, tail_half_w, chain queues;
 * [9..17] = the edge regime: head, tail_c0, srows_edge, pstream_edge, shalf, sh_head, sh_tail_c0, tfull1, xhalf; [18..32] = nchain,
 * ndedicated, nreserve, head_job1, reserve_job0, xchain, quiet_tail, pstream, look, use_quiet, wbias, cboost, panel_dma, grid, srows_max;
 * [33..38] = the six words of mrbf_debug_mega_tables for these tables.  Returns 0, or -(argument index) for a parameter out of range. */
int32_t mrbf_debug_mega_plan(int32_t nt, int32_t mt, int32_t xreal, int64_t *out39);

/* ---- Pascoletti-Serafini descent step with the subproblem solver on the device ----------------------------------------
 * Replaces, for objectives that share ONE grouped RBF model and carry no modelled constraints, the NLopt runs inside
 * get_criticality(::PascolettiSerafiniConfig, ...) (src/descent.jl:512-581): compute_local_ideal_point (:404-412, k runs of
 * _min_component :369-387) when no direction is given, and _ps_optimization (:478-510) with the constraint functions of
 * :434-447 (chi = [t; x], t in [-1,0], x in [lb_eff, ub_eff], minimise t subject to m_l(x) - m_l(x_n) - t r_l <= 0).
 * Population state, ranking and breeding live on the device; one batched surrogate sweep evaluates a whole generation of
 * all runs.  x_n, lb_eff, ub_eff: d; fx_n (true objective values at x_n, used for r = fx_n - ideal) and r_or_null (the direction
 * of _get_global_dir, :360-368): k, host or device.  Outputs x_trial (d), mx_trial (k), r_out (k, may be NULL).
 * info.status: MRBF_PS_OK -> omega = |info.tau| (:573-579); MRBF_PS_CRITICAL -> some r_l <= 0 (:546-549): x_trial = x_n,
 * mx_trial = m(x_n), tau = 0; MRBF_PS_FAILURE -> no feasible point (:571-572), outputs as for CRITICAL. */
enum { MRBF_PS_OK = 0, MRBF_PS_CRITICAL = 1, MRBF_PS_FAILURE = 2 };
typedef struct {
    int32_t max_ideal_evals;  /* per objective; < 0: 500 (d + 1)   (descent.jl:527) */
    int32_t max_ps_evals;     /* < 0: 500 (d + 1); the caller applies _ps_max_evals' 3/4 split (descent.jl:414-432) */
    int32_t max_polish_evals; /* 0: no polish (ps_polish_algo = nothing) */
    int32_t reserved;
    uint64_t seed;            /* counter-based generator key: same seed, same step */
    double t0;                /* start value of t, -0.5 in the reference (descent.jl:555) */
    double xtol_rel;          /* <= 0: 1e-3 (descent.jl:379, :485) */
} mrbf_ps_options;
typedef struct {
    int32_t status;           /* MRBF_PS_* */
    int32_t generations;      /* batched generations over all runs */
    int32_t evals_ideal, evals_ps, evals_polish; /* surrogate evaluations spent */
    float ms_total;           /* hipEvent time of the whole step on the ctx stream */
    double tau;
} mrbf_ps_info;
int32_t mrbf_ps_step(mrbf_ctx *ctx, const mrbf_model *model, const double *x_n, const double *lb_eff, const double *ub_eff,
                     const double *fx_n, const double *r_or_null, const mrbf_ps_options *opts, double *x_trial, double *mx_trial,
                     double *r_out, mrbf_ps_info *info);

/* The same step for a whole SurrogateContainer: objectives and modelled constraints spread over several grouped RBF models
 * (src/SurrogateContainer.jl:48-64), the nonlinear (in)equality constraint handles of descent.jl:389-402 / :448-466 and the MOP's
 * linear constraints in scaled variables (transformed_linear_eq/ineq_constraints, src/AbstractMOPInterface.jl:463-495).
 * roles: one entry per output row of every model, concatenated in model order: l >= 0 -> this row is objective l of the
 * container's objective vector; MRBF_ROLE_EQ / MRBF_ROLE_INEQ -> modelled constraint h(x) = 0 / g(x) <= 0; MRBF_ROLE_NONE ->
 * not used.  A_eq (n_lin_eq x d row-major), b_eq: A x = b; A_ineq, b_ineq: A x <= b (host or device; may be NULL when the
 * count is 0).  An equality counts as satisfied when |h| <= eq_tol (< 0: 1e-8; NLopt's default tolerance 0 would make every
 * point infeasible).  The ideal-point runs (descent.jl:404-412) carry the same constraints.  fx_n, r, mx_trial, r_out have
 * n_objectives entries.  Limits of the device path: mrbf_dispatch_ps. */
enum { MRBF_ROLE_NONE = -1, MRBF_ROLE_EQ = -2, MRBF_ROLE_INEQ = -3 };
typedef struct {
    int32_t n_models, n_objectives;
    const mrbf_model *const *models;
    const int32_t *roles;
    int32_t n_lin_eq, n_lin_ineq;
    const double *A_eq, *b_eq, *A_ineq, *b_ineq;
    double eq_tol;
} mrbf_ps_problem;
int32_t mrbf_ps_step_problem(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x_n, const double *lb_eff,
                             const double *ub_eff, const double *fx_n, const double *r_or_null, const mrbf_ps_options *opts,
                             double *x_trial, double *mx_trial, double *r_out, mrbf_ps_info *info);
/* test hook: ONE stochastic ranking (the ISRES-style pairwise rule of the PS solver, descent.jl:478-510's optimiser) of a given
 * generation -- f[lam] objective values, phi[lam] constraint violations (0 feasible, inf outside the budget) -- by the kernels of
 * the step: impl 0 one workgroup, 1 several compute units (lam >= 1024: one wave per 64 individuals, the records in registers),
 * 2 the same giving up at once (the time-out path: the finishing launch of the one-workgroup kernel runs the phases, the fallback
 * of 1), 9 as 0 with the one-pair-per-thread loop through LDS
 * for populations below 1024 too (round 6 ranks those with a wave per 96 individuals inside the one workgroup),
 * 3 one workgroup with the plain sort of a feasible generation in its one-pair-per-thread form (the form before round 6),
 * 4 one workgroup with the step's own mu = ceil(lam / 7): only the parents are ranked (order_out[mu ..] = -1), 5 the same without
 * the parent selection (the whole population sorted).
 * Other values of impl (6 - 8 were experiments and round 5's sixteen-workgroup form): -7.
 * order_out[lam]: individuals in rank order; *gave_up: the several-compute-unit kernel's failure word. */
int32_t mrbf_debug_ps_rank(mrbf_ctx *ctx, int32_t lam, const double *f, const double *phi, uint64_t seed, int32_t gen, int32_t impl,
                           int32_t *order_out, int32_t *gave_up);

/* ---- steepest-descent criticality: the direction LP on the device (sd_lp.hip) -------------------------------------------
 * mrbf_sd_direction replaces the JuMP / OSQP model of _steepest_descent_direction (src/descent.jl:91-135) for n_lp LPs of one
 * shape in one launch (one workgroup per LP, exact fp64 dual simplex with the bound-flipping ratio test):
 *   minimise alpha over (d, alpha), d in [l, u] with l_j = max(-1, lb_j - x_j), u_j = min(1, ub_j - x_j), alpha free,
 *   g_i . d <= w_i alpha (i < k; w_i = ||g_i||_2 with normalize, else 1), A_eq d = b_eq, A_ineq d <= b_ineq;
 *   m = k + m_eq + m_ineq <= 64, 1 <= d <= 4096.
 * Per LP (consecutive blocks): G k x d in mrbf_eval's jac_out layout (k x d column-major: a Jacobian from mrbf_eval goes in as it
 * is), x / lb / ub d, A_eq m_eq x d and A_ineq m_ineq x d row-major, b_eq m_eq, b_ineq m_ineq (A / b may be NULL when the count
 * is 0).  Outputs: d_out (d, inside [l, u] exactly), omega_out (1): -max_i (g_i . d) / w_i over the rows with w_i > 0, recomputed
 * from the returned d; dual_out (m, may be NULL): the row multipliers (>= 0 on objective and inequality rows, sum_i<k w_i y_i = 1),
 * the optimality certificate; status_out (1): MRBF_SD_*; iters_out (2, may be NULL): simplex iterations, bound flips.
 * NO_OBJECTIVE (normalize and every g_i = 0) and INFEASIBLE (empty box or rows that cannot be met) return d = 0, omega = -Inf:
 * the reference's catch branch (descent.jl:130-133).  Every LP gets a status; the call fails only on invalid arguments.  The
 * result of an LP does not depend on its position in the batch. */
enum { MRBF_SD_OK = 0, MRBF_SD_NO_OBJECTIVE = 1, MRBF_SD_INFEASIBLE = 2, MRBF_SD_GAVE_UP = 3 };
int32_t mrbf_sd_direction(mrbf_ctx *ctx, int64_t n_lp, int32_t d, int32_t k, int32_t m_eq, int32_t m_ineq, const double *G,
                          const double *x, const double *lb, const double *ub, const double *A_eq, const double *b_eq,
                          const double *A_ineq, const double *b_ineq, int32_t normalize, double *d_out, double *omega_out,
                          double *dual_out, int32_t *status_out, int32_t *iters_out);
/* get_criticality(::SteepestDescentConfig, mop, scal, x_it, x_it_n, db, sc, ac) (src/descent.jl:187-241) for a container given as
 * an mrbf_ps_problem (models, roles, linear constraints in scaled variables; eq_tol is not used): objective Jacobians at x_n,
 * modelled-constraint Jacobians at x and values at x_n through the evaluation kernels, right-hand sides b - A x_n (linear rows)
 * and -m(x_n) - Dm(x) (x_n - x) (modelled rows, descent.jl:214-229), then ONE direction LP at x_n over the global bounds lb / ub
 * (full_bounds_internal, not the trust region) and one read-back.  Row order of dual_out: objectives, linear equalities, modelled
 * equalities, linear inequalities, modelled inequalities (modelled rows in model order, then output order).  Returns -2 (take
 * the reference method) when the decision table refuses the shape or the LP gave up (info->status = MRBF_SD_GAVE_UP). */
typedef struct {
    int32_t status;      /* MRBF_SD_* */
    int32_t iterations;  /* dual simplex iterations */
    int32_t bound_flips; /* bound flips of the ratio tests */
    float ms_total;      /* hipEvent time of the whole call on the ctx stream */
    double omega;        /* the criticality omega (-Inf for NO_OBJECTIVE / INFEASIBLE) */
} mrbf_sd_info;
int32_t mrbf_sd_criticality(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x, const double *x_n, const double *lb,
                            const double *ub, int32_t normalize, double *d_out, double *dual_out, mrbf_sd_info *info);

/* ---- directed search: its direction QP on the device (ds_qp.hip) ---------------------------------------------------------
 * mrbf_ds_direction solves the direction problem of the reference's parked directed-search step (src/descent.jl:583-664) for n_qp
 * QPs of one shape in one launch (one workgroup per QP, exact fp64 primal active-set method with minimum-norm steps; DESIGN.md
 * section 21):
 *   minimise 1/2 ||G d - r||_2^2 over d in [l, u] with l_j = max(-1, lb_j - x_j), u_j = min(1, ub_j - x_j) (mrbf_sd_direction's box),
 *   G d <= 0 (descent.jl:635-639: only non-ascent directions);  1 <= d <= 4096, 1 <= k <= 16, n_qp >= 1.
 * Per QP (consecutive blocks): G k x d in mrbf_eval's jac_out layout (k x d column-major: a Jacobian from mrbf_eval goes in as it
 * is), r k (the target change of the model values: minus the direction of _get_global_dir, descent.jl:599-611), x / lb / ub d.
 * Outputs: d_out (d, inside [l, u] exactly: a variable on a bound carries the bound's bits; not normalised), z_out (k): G d
 * recomputed from the returned d, omega_out (1): max(0, -max_i z_i) (descent.jl:645), mult_out (k, may be NULL): the multipliers
 * mu >= 0 of the rows G d <= 0 -- with y = z - r + mu and s = G' y the certificate is s_j = 0 on free variables, s_j >= 0 on the
 * lower and <= 0 on the upper bound, mu_i z_i = 0 --, status_out (1): MRBF_DS_*, iters_out (2, may be NULL): iterations,
 * constraints dropped.  CRITICAL (some r_i >= 0 or NaN, descent.jl:615-617): d = 0, z = 0, omega = 0.  INFEASIBLE (some l_j > u_j):
 * d = 0, omega = -Inf.  GAVE_UP (the iteration cap 8 (d + k) + 16, a failed consistency check, or x outside [lb, ub] so that d = 0
 * is no start): d = NaN, omega = NaN; the bindings take the host method.  z, omega and the optimal value are unique; d is not where
 * the free columns of G have a null space: it is defined by the method, does not depend on the QP's position in the batch, and the
 * same call gives the same bits.  Every array may be host or device memory.  Every QP gets a status; the call fails only on
 * invalid arguments: -1 no context, -3 n_qp < 1, -4 d outside 1 .. 4096, -5 k outside 1 .. 16, -6 .. -10 NULL G, r, x, lb, ub,
 * -11 .. -14 NULL d_out, z_out, omega_out, status_out; nothing is written then. */
enum { MRBF_DS_OK = 0, MRBF_DS_CRITICAL = 1, MRBF_DS_INFEASIBLE = 2, MRBF_DS_GAVE_UP = 3 };
enum { MRBF_DS_NO_START = 4 };  /* mrbf_ds_direction_rows alone: the start d = 0 misses a constraint row */
int32_t mrbf_ds_direction(mrbf_ctx *ctx, int64_t n_qp, int32_t d, int32_t k, const double *G, const double *r, const double *x,
                          const double *lb, const double *ub, double *d_out, double *z_out, double *omega_out, double *mult_out,
                          int32_t *status_out, int32_t *iters_out);
/* The criticality of directed search (src/descent.jl:583-664) for a container given as an mrbf_ps_problem (models, roles; no linear
 * and no modelled constraints: the formulation the reference wrote down): the objective Jacobians at x_n through the evaluation
 * kernels, gathered by the roles table, then ONE direction QP at x_n over the global bounds lb / ub (full_bounds_internal) and one
 * read-back.  r (k): the target change of the model values.  d_out (d) and info->omega are, bit for bit, those of mrbf_ds_direction
 * on the Jacobian mrbf_eval returns at x_n; mult_out (k, may be NULL).  Returns -2 (take the host method) when the decision table
 * refuses the shape or the QP gave up (info->status = MRBF_DS_GAVE_UP); -1 no context, -3 .. -8 NULL problem, x_n, lb, ub, r,
 * d_out, -10 NULL info. */
typedef struct {
    int32_t status;      /* MRBF_DS_* */
    int32_t iterations;  /* active-set iterations */
    int32_t dropped;     /* constraints dropped from the working set */
    float ms_total;      /* hipEvent time of the whole call on the ctx stream */
    double omega;        /* the criticality omega */
} mrbf_ds_info;
int32_t mrbf_ds_criticality(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x_n, const double *lb, const double *ub,
                            const double *r, double *d_out, double *mult_out, mrbf_ds_info *info);

/* ---- directed search with constraint rows: the extended direction QP on the device (ds_qp_rows.hip) ---------------------------
 * mrbf_ds_direction_rows solves mrbf_ds_direction's QP extended by the rows of get_criticality (src/descent.jl:196-236) -- what the
 * parked directed-search step (src/descent.jl:598-645) would be given for a constrained problem -- for n_qp QPs of one shape in one
 * launch (one workgroup per QP, the same exact fp64 active-set method, generalised):
 *   minimise 1/2 ||G d - r||_2^2 over d in [l, u] (mrbf_sd_direction's box),  G d <= 0,  A_eq d = b_eq,  A_in d <= b_in;
 *   1 <= d <= 4096, k >= 1, m_eq >= 0, m_in >= 0, K = k + m_eq + m_in <= 16, n_qp >= 1.
 * Per QP (consecutive blocks): G, r, x, lb, ub as mrbf_ds_direction takes them; A_eq m_eq x d and A_in m_in x d row-major with b_eq
 * m_eq and b_in m_in, as mrbf_sd_direction takes them (NULL where the count is 0).  The start d = 0 must satisfy the rows: a miss
 * |b_eq,i| (or -b_in,i where b_in,i < 0) of at most 1e-10 sum_j |A_ij| is clamped to zero before the solve and the returned d is
 * feasible for the clamped right-hand side; a larger one ends that QP with MRBF_DS_NO_START (there is no phase 1).  Outputs: d_out (d,
 * inside [l, u] exactly), c_out (K): W d for W = [G; A_eq; A_in] recomputed from the returned d, objective rows first; omega_out (1):
 * max(0, -max_i (G d)_i); mult_out (K, may be NULL): mu with mu_i >= 0 on objective and inequality rows and free sign on equality
 * rows -- with y_i = (G d - r + mu)_i on objective rows, y_i = mu_i on the others and s = W' y the certificate is s_j = 0 on free
 * variables, s_j >= 0 on the lower and <= 0 on the upper bound, mu_i (h_i - c_i) = 0 for h = (0, b_eq, b_in) --; status_out (1):
 * MRBF_DS_*; iters_out (2, may be NULL): iterations, constraints dropped.  CRITICAL and INFEASIBLE as mrbf_ds_direction answers
 * them (c = 0, mult = 0).  GAVE_UP (the iteration cap 8 (d + K) + 16, a failed consistency check -- every row of the returned d holds
 * within 1e-13 (sum_j |W_ij| + |h_i|) --, or x outside [lb, ub]) and NO_START: d, c, omega, mult = NaN; the bindings take the host
 * method.  G d, omega and the optimal value are unique; d and the constraint rows' values are not.  With m_eq = m_in = 0 the outputs
 * are mrbf_ds_direction's, bit for bit.  The same call gives the same bits, whatever the QP's position in the batch.  Every array may
 * be host or device memory.  The call fails only on invalid arguments: -1 no context, -3 n_qp < 1, -4 d outside 1 .. 4096, -5 k
 * outside 1 .. 16, -6 m_eq < 0, -7 m_in < 0, -8 k + m_eq + m_in > 16, -9 .. -13 NULL G, r, x, lb, ub, -14 / -15 NULL A_eq / b_eq
 * with m_eq > 0, -16 / -17 NULL A_in / b_in with m_in > 0, -18 .. -21 NULL d_out, c_out, omega_out, status_out; nothing is written
 * then. */
int32_t mrbf_ds_direction_rows(mrbf_ctx *ctx, int64_t n_qp, int32_t d, int32_t k, int32_t m_eq, int32_t m_in, const double *G,
                               const double *r, const double *x, const double *lb, const double *ub, const double *A_eq,
                               const double *b_eq, const double *A_in, const double *b_in, double *d_out, double *c_out,
                               double *omega_out, double *mult_out, int32_t *status_out, int32_t *iters_out);
/* The criticality of directed search for a container with modelled or linear constraints (src/descent.jl:196-236 for the rows,
 * :598-645 for the QP), given as an mrbf_ps_problem: values and Jacobians at [x_n; x] through the evaluation kernels, G, A_eq / b_eq
 * (linear rows, then modelled ones), A_ineq / b_ineq (likewise) by mrbf_sd_criticality's assembly kernel, then ONE
 * mrbf_ds_direction_rows QP at x_n over the global bounds and one read-back.  d_out (d), mult_out (k + m_eq + m_in, may be NULL, row
 * order as mrbf_sd_criticality's dual_out) and info are, bit for bit, those of mrbf_ds_direction_rows on these rows.  Returns -2 (take
 * the host method) when mrbf_dispatch_ds_rows refuses the shape, the QP gave up or d = 0 is no start (info->status = MRBF_DS_GAVE_UP /
 * MRBF_DS_NO_START: with a normal step n != 0 the modelled rows' right-hand side -m(x_n) - Dm(x) n is not small in general); -1 no
 * context, -3 .. -9 NULL problem, x, x_n, lb, ub, r, d_out, -11 NULL info. */
int32_t mrbf_ds_criticality_rows(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x, const double *x_n, const double *lb,
                                 const double *ub, const double *r, double *d_out, double *mult_out, mrbf_ds_info *info);

/* ---- the normal step: its LP on the device (normal_lp.hip) ----------------------------------------------------------------
 * mrbf_normal_direction replaces the JuMP / OSQP model of compute_normal_step (src/descent.jl:691-757) for n_lp LPs of one shape
 * in one launch (one workgroup per LP, exact fp64 active-set dual simplex):
 *   minimise alpha over (n, alpha >= 0), -alpha <= n_j <= alpha, lb_j - x_j <= n_j <= ub_j - x_j, A_eq n = b_eq, A_ineq n <= b_ineq;
 *   1 <= m_eq + m_ineq <= 64 rows, 1 <= d <= 4096; the box may be infinite either way and x may lie outside it.
 * The rows are in the step n: for Morbit's LP pass b_eq - A_eq x, b_ineq - A_ineq x (linear rows) and -m(x) with Dm(x) (modelled
 * rows).  Per LP (consecutive blocks): x / lb / ub d, A_eq m_eq x d and A_ineq m_ineq x d row-major, b_eq m_eq, b_ineq m_ineq
 * (A / b may be NULL when the count is 0).  Outputs: n_out (d): clamp(x + n, lb, ub) - x (_project_into_box); alpha_out (1):
 * ||n_out||_inf of the returned n; dual_out (m, may be NULL): the row multipliers y (equalities first; >= 0 on inequality rows),
 * the certificate: alpha* = -y.b + min over alpha >= alpha0 of [alpha + sum_j min over n_j of (C'y)_j n_j]; status_out (1):
 * MRBF_NS_*; iters_out (2, may be NULL): simplex iterations, pivots that swap one column's constraints.  x already satisfying
 * every row gives n = 0 after zero iterations.  INFEASIBLE (empty box or rows that cannot be met) and GAVE_UP (the iteration
 * cap 8 (m + d), a singular working set, or multipliers that fail the dual-feasibility check at the end) return n = NaN,
 * alpha = +Inf, y = 0.  Every LP gets a status; the call fails only on invalid arguments (-1 without a context).  The result of
 * an LP does not depend on its position in the batch. */
enum { MRBF_NS_OK = 0, MRBF_NS_INFEASIBLE = 1, MRBF_NS_GAVE_UP = 2 };
int32_t mrbf_normal_direction(mrbf_ctx *ctx, int64_t n_lp, int32_t d, int32_t m_eq, int32_t m_ineq, const double *x, const double *lb,
                              const double *ub, const double *A_eq, const double *b_eq, const double *A_ineq, const double *b_ineq,
                              double *n_out, double *alpha_out, double *dual_out, int32_t *status_out, int32_t *iters_out);
/* compute_normal_step(mop, scal, x_it, data_base, sc, algo_config; variable_radius) (src/descent.jl:691-757) for a container
 * given as an mrbf_ps_problem (only MRBF_ROLE_EQ / MRBF_ROLE_INEQ rows are used; objective rows are ignored; n_models may be 0
 * for linear rows only; n_objectives and eq_tol are not used) in d variables (the models' d): values and Jacobians of the
 * modelled constraints at x through the evaluation kernels (one site per model that carries constraint rows), right-hand sides
 * b - A x (linear rows) and -m(x) (modelled rows) assembled on the device, ONE LP over the global bounds lb / ub
 * (full_bounds_internal) and one read-back.  Radius: delta as given (fixed), or alpha / kappa_delta when variable_radius
 * (infeasible above delta_max).  Infeasible: n_out = NaN, info->delta = -Inf.  Row order of dual_out: linear equalities,
 * modelled equalities, linear inequalities, modelled inequalities (modelled rows in model order, then output order).  Returns
 * -2 (take the reference method) when the decision table refuses the shape or the LP gave up (info->status = MRBF_NS_GAVE_UP). */
typedef struct {
    int32_t status;      /* MRBF_NS_* */
    int32_t iterations;  /* dual simplex iterations */
    int32_t bound_flips; /* pivots that swap one column's constraints (n_j from one bound to another) */
    float ms_total;      /* hipEvent time of the whole call on the ctx stream */
    double alpha;        /* ||n||_inf of the returned step (+Inf when the LP is infeasible) */
    double delta;        /* the radius the reference returns (-Inf when infeasible) */
} mrbf_normal_info;
int32_t mrbf_normal_step(mrbf_ctx *ctx, const mrbf_ps_problem *problem, int32_t d, const double *x, const double *lb, const double *ub,
                         double delta, double kappa_delta, double delta_max, int32_t variable_radius, double *n_out, double *dual_out,
                         mrbf_normal_info *info);

/* ---- the steepest-descent step on the device (sd_step.hip) ------------------------------------------------------------------
 * compute_descent_step(::SteepestDescentConfig, mop, scal, x_it, x_it_n, db, sc, ac, omega, d) (src/descent.jl:243-318) for a
 * container given as an mrbf_ps_problem (models, roles, linear constraints in scaled variables; eq_tol is not used) in one call:
 * the initial step size sigma of descent.jl:251-310 -- _local_bounds(x, delta, lb, ub), isapprox(x, x_n), intersect_box(x_n, d,
 * lb_eff, ub_eff; :pos) and, for Delta > 1 and ||d||_inf ~ 1, _intersect_bounds (utilities.jl:126-287) on the stacked [x_n; x_n - x]
 * with the linear rows and the modelled constraints linearised at x (values and Jacobians through the evaluation kernels) --
 * then the Armijo loop of _backtrack (descent.jl:150-185, condition :137-143) over all max_loops + 1 step sizes at once: the
 * objective models evaluate x_n and the max_loops + 1 trial points x_n + sigma shrink^i d (step sizes formed one after another,
 * never as a power) in one sweep each, and the index the reference loop stops at is picked on the device; one read-back.
 * lb / ub: the global bounds in scaled variables (full_bounds_internal); omega / d: what mrbf_sd_criticality returned.  Every
 * array may be a host or a device pointer.  x_plus (d) and mx_plus (n_objectives, objective order) are x+ and m(x+); sigma <=
 * min_stepsize (NaN included) gives omega = 0, x+ = x_n, m(x_n) and a step norm of 0 (descent.jl:312-317).  The backtracking stop
 * uses min_stepsize when it is >= 0, else eps (descent.jl:152).  Modelled rows are taken in model order, then output order
 * (which only matters for the anchor of the equality test).  Returns -2 (take the reference method) when mrbf_dispatch_sd_step
 * refuses the shape.  Trial points and Armijo right-hand sides round as the host loop's (no FMA contraction); every reduction has
 * a fixed order, so the result does not depend on timing. */
typedef struct {
    int32_t strict;       /* strict_backtracking: every objective must decrease (1) or the maximum (0) */
    int32_t max_loops;    /* 0 .. 1024 */
    double const_rhs;     /* armijo_const_rhs */
    double shrink;        /* armijo_const_shrink, in (0, 1) */
    double min_stepsize;  /* cfg.min_stepsize as given (< 0: eps for the backtracking stop) */
} mrbf_sd_step_options;
typedef struct {
    int32_t branch;      /* how sigma was chosen: 0 "delta" (Delta <= 1), 1 "one", 2 "intersect" */
    int32_t loops;       /* the reference loop's counter i at its stop (0 for the sigma <= min_stepsize branch) */
    float ms_total;      /* hipEvent time of the whole call on the ctx stream */
    double sigma;        /* the initial step size */
    double omega;        /* omega as given, or 0 for the sigma <= min_stepsize branch */
    double step_norm;    /* ||sigma shrink^loops d||_inf (0 for the sigma <= min_stepsize branch) */
} mrbf_sd_step_info;
int32_t mrbf_sd_step(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x, const double *x_n, double delta, const double *lb,
                     const double *ub, double omega, const double *d, const mrbf_sd_step_options *opts, double *x_plus, double *mx_plus,
                     mrbf_sd_step_info *info);

/* ---- many-start steepest descent: one call for a batch of starts (sd_batch.hip) -----------------------------------------------
 * get_criticality(::SteepestDescentConfig, ...) (src/descent.jl:187-241) followed by compute_descent_step (descent.jl:243-318) for
 * n_starts independent starts of one problem -- the reference's Threads.@threads loop over starts
 * (examples/large_scale_benchmarks.jl:102-109) -- as one chain on the ctx stream with one read-back.  For start p the outputs are,
 * bit for bit, those of mrbf_sd_criticality(x_p, x_n_p, lb, ub, normalize) -> (omega_p, d_p) and mrbf_sd_step(x_p, x_n_p, delta_p,
 * lb, ub, omega_p, d_p, opts) chained on start p's container: the roles table and linear rows of `shape` with row p of `models`
 * (n_starts x shape->n_models handles, start-major; shape->models is ignored).  The starts share d, the model count, every model
 * slot's output count, the roles and the linear rows; the number of centres and the kernel parameters may differ between starts.
 * x, x_n: n_starts x d; delta: n_starts; lb / ub (d): the one MOP's global bounds; d_out, x_plus: n_starts x d; mx_plus: n_starts x
 * n_objectives; every array may be a host or a device pointer, records is host memory; ms_total may be NULL.  The step runs on
 * whatever the LP returned (NO_OBJECTIVE / INFEASIBLE: d = 0, omega = -Inf, x+ = x_n), except MRBF_SD_GAVE_UP: that start's record
 * carries the status and its d, x+ and mx+ are NaN (take the reference method for it).  Every start gets a record.  Returns 0 unless
 * an argument is invalid, -2 (take the reference method) when mrbf_dispatch_sd_batch refuses the shape. */
typedef struct {
    int32_t sd_status;              /* MRBF_SD_* of this start's direction LP */
    int32_t iterations, bound_flips;
    int32_t branch, loops;          /* as mrbf_sd_step_info */
    int32_t reserved;
    double omega;                   /* criticality from the LP (-Inf for NO_OBJECTIVE / INFEASIBLE) */
    double omega_step;              /* what the step returns: omega, or 0 on the sigma <= min_stepsize branch */
    double sigma, step_norm;
} mrbf_sd_batch_record;
int32_t mrbf_sd_iterate_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                              const double *x, const double *x_n, const double *delta, const double *lb, const double *ub,
                              int32_t normalize, const mrbf_sd_step_options *opts, double *d_out, double *x_plus, double *mx_plus,
                              mrbf_sd_batch_record *records, float *ms_total);

/* ---- many-start directed search: one call for a batch of starts (ds_batch.hip) -------------------------------------------------
 * The criticality of directed search (src/descent.jl:583-664) followed by its step (descent.jl:645-660: the steepest-descent step on
 * the normalised direction) for n_starts independent starts of one problem -- the reference's Threads.@threads loop over starts
 * (examples/large_scale_benchmarks.jl:102-109) -- as one chain on the ctx stream with one upload and one read-back.  For start p the
 * outputs are, bit for bit, those of this chain on start p's container (the roles table of `shape` with row p of `models`: n_starts
 * x shape->n_models handles, start-major; shape->models is ignored; no linear and no modelled constraints):
 *   mrbf_ds_criticality(x_n_p, lb, ub, r_p) -> (omega, d, status, mu);
 *   the bindings' rule: (omega, d / ||d||_inf) if status = MRBF_DS_OK and ||d||_inf > 0, else (0, zeros);
 *   mrbf_sd_step(x_p, x_n_p, delta_p, lb, ub, omega', d', opts) -> x+, m(x+) and the step info.
 * The starts share d, the model count, every model slot's output count and the roles; the number of centres and the kernel parameters
 * may differ between starts.  x, x_n: n_starts x d; delta: n_starts; lb / ub (d): the one MOP's global bounds; r: n_starts x
 * n_objectives, the target change of the model values per start; d_out (the normalised direction d'), x_plus: n_starts x d; mx_plus:
 * n_starts x n_objectives; mult_out (mu; may be NULL): n_starts x n_objectives.  Every array may be a host or a device pointer, records
 * is host memory; ms_total may be NULL.  CRITICAL / INFEASIBLE starts take the step on (0, zeros): x+ = x_n (the record's omega is 0 /
 * -Inf, the QP's).  MRBF_DS_GAVE_UP: that start's record carries the status, its d_out, x_plus, mx_plus and mult_out rows are NaN (take
 * the host method for it); the other starts are unaffected.  Every start gets a record.  Returns 0, or: -1 no context; -2 (take the
 * single calls per start) when mrbf_dispatch_ds_batch refuses the shape; -3 NULL shape, no models, no roles table or a defect of the
 * table; -4 NULL models or a defect of the handles; -5 .. -10 NULL x, x_n, delta, lb, ub, r; -11 NULL opts or shrink outside (0, 1);
 * -12 .. -15 NULL d_out, x_plus, mx_plus, records.  Nothing is written on a negative code. */
typedef struct {
    int32_t ds_status;           /* MRBF_DS_* of this start's direction QP */
    int32_t iterations, dropped; /* as mrbf_ds_info */
    int32_t branch, loops;       /* as mrbf_sd_step_info */
    int32_t reserved;
    double omega;                /* the QP's omega (what mrbf_ds_criticality reports) */
    double omega_step;           /* what the step returns */
    double sigma, step_norm;
    double dnorm;                /* ||d||_inf of the QP's d before normalisation (0 unless the status is MRBF_DS_OK) */
} mrbf_ds_batch_record;          /* 64 bytes */
int32_t mrbf_ds_iterate_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                              const double *x, const double *x_n, const double *delta, const double *lb, const double *ub,
                              const double *r, const mrbf_sd_step_options *opts, double *d_out, double *x_plus, double *mx_plus,
                              double *mult_out, mrbf_ds_batch_record *records, float *ms_total);

/* ---- many-start normal step: one call for a batch of starts (normal_batch.hip) -------------------------------------------------
 * compute_normal_step (src/descent.jl:691-757) for n_starts independent starts of one problem -- the reference's Threads.@threads loop
 * over starts (examples/large_scale_benchmarks.jl:102-109) -- as one chain on the ctx stream with one read-back.  For start p n_out,
 * dual_out and every record field are, bit for bit, what mrbf_normal_step(x_p, lb, ub, delta_p, kappa_delta, delta_max,
 * variable_radius) returns on start p's container: the roles table and linear rows of `shape` with row p of `models` (n_starts x
 * shape->n_models handles, start-major; shape->models is ignored; models may be NULL when shape->n_models == 0: linear rows only).
 * The starts share d, the model count, every model slot's output count, the roles and the linear rows; the number of centres and the
 * kernel parameters may differ between starts.  x: n_starts x d; delta: n_starts; lb / ub (d): the one MOP's global bounds; n_out:
 * n_starts x d; x_n_out (n_starts x d, may be NULL): x + n, one fp64 add per entry -- it can stay on the device and be passed as x_n
 * to mrbf_sd_iterate_batch; dual_out (n_starts x m, may be NULL): row order as mrbf_normal_step; every array may be a host or a
 * device pointer, records is host memory; ms_total may be NULL.  A start whose LP is infeasible, or whose radius alpha / kappa_delta
 * exceeds delta_max, gets n = NaN, x_n = NaN and delta = -Inf in its record, as the single call returns; a start whose LP gave up
 * (MRBF_NS_GAVE_UP) gets the same with that status in its record and does not fail the call (take the reference method for it).
 * Every start gets a record.  Returns 0 unless an argument is invalid, -2 (take the reference method) when
 * mrbf_dispatch_normal_batch refuses the shape (n_starts < 1 included).  -2 means nothing else here: an invalid argument (a NULL
 * pointer, a negative count, an unknown role, kappa_delta <= 0 with a variable radius, models that do not share the shape) returns
 * -1 or a code from -3 down, as in mrbf_sd_iterate_batch and unlike mrbf_normal_step, which answers -2 to those too. */
typedef struct {
    int32_t status;              /* MRBF_NS_* of this start's LP */
    int32_t iterations, bound_flips;
    int32_t reserved;
    double alpha;                /* as mrbf_normal_info.alpha */
    double delta;                /* as mrbf_normal_info.delta (-Inf: infeasible, or above delta_max) */
} mrbf_normal_batch_record;      /* 32 bytes */
int32_t mrbf_normal_step_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models, int32_t d,
                               const double *x, const double *lb, const double *ub, const double *delta, double kappa_delta,
                               double delta_max, int32_t variable_radius, double *n_out, double *x_n_out, double *dual_out,
                               mrbf_normal_batch_record *records, float *ms_total);

/* ---- many-start Pascoletti-Serafini step: one call for a batch of starts (ps_solver.hip) ----------------------------------------
 * get_criticality(::PascolettiSerafiniConfig, ...) (src/descent.jl:512-581) for n_starts independent starts of one problem -- the
 * reference's Threads.@threads loop over starts (examples/large_scale_benchmarks.jl:102-109) with descent_method = :ps (:70, budgets
 * :215-219).  For start p, x_trial, mx_trial, r_out and every field of infos[p] except ms_total are, bit for bit, what
 * mrbf_ps_step_problem returns for start p's container -- the roles table, the linear rows and eq_tol of `shape` with row p of `models`
 * (n_starts x shape->n_models handles, start-major; shape->models is ignored) -- called with row p of the arrays and the seed seeds[p]:
 * the kernels are that call's own with the start on a grid dimension, every run keeps its index within its own start and its start's
 * seed as the generator's key, and every evaluation keeps the query count of the single call it stands for.  The starts share d, the
 * model count, every model slot's output count, the roles and the linear rows; the number of centres and the kernel parameters may
 * differ between starts.  x_n, lb_eff, ub_eff, x_trial: n_starts x d (the effective box is a start's own: it follows its trust
 * region); fx_n, r_or_null, mx_trial, r_out: n_starts x n_objectives; r_or_null == NULL: the ideal-point phase runs for every start;
 * r_out may be NULL; every one of these arrays may be a host or a device pointer.  infos (n_starts) and seeds_or_null (n_starts; NULL:
 * opts->seed for every start) are host memory; ms_total may be NULL, and every infos[p].ms_total carries the whole call's event time.
 * Per generation there is one population sweep per launch group, the optional score launch, the ranking and the breeding for all
 * starts together; the refinements of all starts advance in lockstep with one host synchronisation per iteration.  The several-
 * compute-unit ranking is used while all runs of a launch can be resident together (16 compute units per run); beyond that count every
 * run is ranked by one workgroup.  A batch whose state exceeds 2 GiB is processed in chunks of starts inside the call.
 * A start's MRBF_PS_CRITICAL or MRBF_PS_FAILURE is that start's status and does not fail the call; a critical start takes no part in
 * the PS-run phase.  Returns 0; -1 or a code from -3 down for an invalid argument (the table and the linear rows -3, models that do
 * not share the shape -4); -2 (take mrbf_ps_step_problem, or the reference method, per start) only when mrbf_dispatch_ps_batch refuses
 * the shape (n_starts < 1 included). */
int32_t mrbf_ps_step_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                           const double *x_n, const double *lb_eff, const double *ub_eff, const double *fx_n, const double *r_or_null,
                           const mrbf_ps_options *opts, const uint64_t *seeds_or_null, double *x_trial, double *mx_trial, double *r_out,
                           mrbf_ps_info *infos, float *ms_total);

/* ---- local ideal points: the ideal-point phase of the step above as calls of its own (ps_solver.hip) ---------------------------
 * compute_local_ideal_point (src/descent.jl:404-412: k runs of _min_component, :369-387) for one start, or for n_starts starts in one
 * call: the k single-objective minimisations of every start side by side -- sweep, ranking and breeding on the device, the
 * refinements in lockstep -- and nothing else of the step.  It is the phase mrbf_ps_step_problem / mrbf_ps_step_batch run when
 * r_or_null == NULL, the same code with the same launches: for the same container, box, max_ideal_evals, xtol_rel and seed,
 * fx_n[l] - ideal_out[l] == r_out[l] of that call, bit for bit, and evals_ideal is equal; and every output of the batch call for
 * start p (ms_total aside) is, bit for bit, the single call's on start p's container with seeds[p].
 * problem / shape: roles, linear rows and eq_tol as in the PS calls (the runs carry the constraints); models: n_starts x n_models
 * handles, start-major (shape->models is ignored).  opts: only max_ideal_evals, seed and xtol_rel are read.  x_n, lb_eff, ub_eff:
 * (n_starts x) d.  ideal_out (n_starts x) k: the value the phase ends with for objective l, after its refinement; x_ideal_out
 * (n_starts x) k x d, may be NULL: where that value was found (inside [lb_eff, ub_eff]); mx_out (n_starts x) k, may be NULL: m(x_n).
 * A run that met no feasible point gives ideal = m_l(x_n) and x_ideal = x_n.  Every one of these arrays may be a host or a device
 * pointer; infos and seeds_or_null (NULL: opts->seed for every start) are host memory; ms_total may be NULL.
 * Returns 0; -1 no context; -3 NULL problem / shape, a bad roles table or bad linear rows; -4 NULL models, or models that do not
 * share the shape; -5 NULL x_n; -6 NULL lb_eff, or lb_eff > ub_eff somewhere; -7 NULL ub_eff; -8 NULL opts; -9 NULL ideal_out; -10
 * NULL info / infos; -2 (take the reference method, or the single call per start) only when mrbf_dispatch_ideal /
 * mrbf_dispatch_ideal_batch refuses the shape (n_starts < 1 included).  Nothing is written on a negative code. */
typedef struct {
    int32_t evals_ideal;      /* surrogate evaluations spent, all objectives, refinements included */
    int32_t generations;      /* generations, summed over the objectives' runs */
    int32_t found;            /* bit l: the run of objective l met a feasible point */
    int32_t refined;          /* bit l: a refinement of objective l's best point ran */
    float ms_total;           /* hipEvent time of the whole call on the ctx stream */
} mrbf_ideal_info;            /* 20 bytes */
int32_t mrbf_ideal_point_problem(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x_n, const double *lb_eff,
                                 const double *ub_eff, const mrbf_ps_options *opts, double *ideal_out, double *x_ideal_out,
                                 double *mx_out, mrbf_ideal_info *info);
int32_t mrbf_ideal_point_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                               const double *x_n, const double *lb_eff, const double *ub_eff, const mrbf_ps_options *opts,
                               const uint64_t *seeds_or_null, double *ideal_out, double *x_ideal_out, double *mx_out,
                               mrbf_ideal_info *infos, float *ms_total);

/* ---- the decision table of the host bindings ---------------------------------------------------------------------------
 * Which implementation a binding (morbit.jl_amd/julia/HipRbf.jl, the Python mirror) takes for one call of Morbit's interface:
 * the device entry point (MRBF_DISPATCH_DEVICE) or Morbit's own method on the same arguments (MRBF_DISPATCH_REFERENCE; Julia:
 * `invoke` of the generic method, Python: the host mirror).  Pure host code (no ctx, no GPU), so both bindings make exactly the
 * same decisions and the CPU tests pin them.  A binding never raises because a size limit was hit.
 *   mrbf_dispatch_ps         get_criticality(::PascolettiSerafiniConfig, ...) (src/descent.jl:512-581).  n_foreign = objectives or
 *                            modelled constraints that are not RefSurrogate rows of a device model (CompositeSurrogate,
 *                            ExactModel, Taylor / Lagrange models); n_nl_constraints = modelled constraint rows, n_lin_constraints =
 *                            linear constraint rows of the MOP.
 *   mrbf_dispatch_backtrack  _backtrack (src/descent.jl:150-185): device iff the objectives are the outputs, in order, of ONE
 *                            device model (then mrbf_backtrack applies); otherwise the reference loop (on batched container
 *                            sweeps where the binding has them).
 *   mrbf_dispatch_affine     candidate scan of the affinely-independent-point filter (AffinelyIndependentPoints.jl:71-106).
 *   mrbf_dispatch_affine_batch  the filters of n_starts starts in one call (mrbf_affine_select_batch): device iff
 *                            1 <= n_starts <= 65535 (a grid dimension), the inf-norm and 8 (d + 1) coordinates of 8 bytes within
 *                            64 KiB of LDS (d <= 1023) -- the range of the one-launch-per-pick kernel.  Whether a start's filter is
 *                            worth the device at all stays mrbf_dispatch_affine's decision, start by start.
 *   mrbf_dispatch_round4     _rbf_round4 (src/models/RbfModel.jl:352-499): device iff the start set can carry the tail (n0 >= q)
 *                            and there are candidates.
 *   mrbf_dispatch_fit        update_model (RbfModel.jl:743-767): MRBF_FIT_FROM_ROUND4 iff a kept round-4 state describes exactly
 *                            the training set (state_n0 + state_n_accepted == n_training, same sites in the same order:
 *                            same_sites != 0) with a unisolvent start set (state_n0 == q), at least one accepted site and at most
 *                            1024 training sites (beyond that the ordinary fit is as fast and more accurate).
 *   mrbf_dispatch_sd         get_criticality(::SteepestDescentConfig, ...) (src/descent.jl:187-241): device iff no foreign
 *                            surrogate, at least one device model, 1 <= d <= 4096, k >= 1 and k + n_nl + n_lin <= 64 LP rows.
 *   mrbf_dispatch_ds         the criticality of directed search (src/descent.jl:583-664, mrbf_ds_criticality): device iff no foreign
 *                            surrogate, at least one device model, 1 <= d <= 4096, 1 <= k <= 16 and neither modelled nor linear
 *                            constraints -- the formulation the reference wrote down; with constraint rows the host method runs.
 *   mrbf_dispatch_ds_rows    the criticality of directed search for a container with constraint rows (src/descent.jl:196-236,
 *                            :598-645, mrbf_ds_criticality_rows): device iff no foreign surrogate, at least one device model,
 *                            1 <= d <= 4096, k >= 1, at least one constraint row and k + n_nl + n_lin <= 16 rows.
 *   mrbf_dispatch_normal     compute_normal_step (src/descent.jl:691-757): device iff no modelled constraint row sits on a
 *                            foreign surrogate, 1 <= d <= 4096 and 1 <= n_nl + n_lin <= 64 LP rows (n_models may be 0).
 *   mrbf_dispatch_sd_step    compute_descent_step(::SteepestDescentConfig, ...) (src/descent.jl:243-318, _backtrack :150-185,
 *                            utilities.jl:126-294): device iff no objective or modelled-constraint row is foreign, at least one
 *                            device model, 1 <= d <= 4096, 1 <= k <= 64, n_nl + n_lin <= 256 rows and 0 <= max_loops <= 1024.
 *   mrbf_dispatch_sd_batch   the two calls above for n_starts starts in one (mrbf_sd_iterate_batch): device iff mrbf_dispatch_sd
 *                            and mrbf_dispatch_sd_step both say so, d <= 256 (the fused evaluation kernels' range) and
 *                            1 <= n_starts <= 65535 (a grid dimension).
 *   mrbf_dispatch_ds_batch   the criticality and the step of directed search for n_starts starts in one call (mrbf_ds_iterate_batch):
 *                            device iff mrbf_dispatch_ds and mrbf_dispatch_sd_step both say so, d <= 256 (the fused evaluation
 *                            kernels' range) and 1 <= n_starts <= 65535 (a grid dimension).
 *   mrbf_dispatch_normal_batch  compute_normal_step for n_starts starts in one call (mrbf_normal_step_batch): device iff
 *                            mrbf_dispatch_normal says so, 1 <= n_starts <= 65535 (a grid dimension) and, where modelled rows are
 *                            evaluated (n_nl > 0), d <= 256 (the fused evaluation kernels' range); linear rows alone keep d <= 4096.
 *   mrbf_dispatch_fit_batch  update_model of n_starts starts in one call (mrbf_fit_batch): device iff 1 <= n_starts <= 65535 (a grid
 *                            dimension).  Which starts share the batched launches is decided inside the call, start by start.
 *   mrbf_dispatch_fit_batch_max_n  the value of MRBF_OPT_SMALL_FIT_MAX_N the bindings set around mrbf_fit_batch for n_starts starts
 *                            of dimension d: the largest n the one-launch fit should take.  The bindings keep the loop of single
 *                            calls (512: the option's default, starts beyond it take mrbf_fit inside the call) where the batch does
 *                            not pay (measured, DESIGN.md section 12: 1684 from 8 starts on, 2048 from 16 on, at 65 <= d <= 128);
 *                            n_starts < 1 or > 65535, or d outside 1 .. 128: 512.
 *   mrbf_dispatch_fit_batch_lu  1 where the bindings set MRBF_OPT_SMALL_LU around mrbf_fit_batch: n_lu_starts of the call's starts are
 *                            on the LU path inside that option's range, the largest of them has n_max sites, their dimension is d.
 *                            Measured cells only (tools/fit_batch_lu_bench.py; admitted where the batch took at
 *                            most 0.8 of the loop of single calls), monotone in n_lu_starts; anything else: 0, the option stays off.
 *   mrbf_dispatch_round4_batch  _rbf_round4 of n_starts starts in one call (mrbf_round4_batch): device iff 1 <= n_starts <= 65535 (a grid
 *                            dimension) and 1 <= d <= 1024 (mrbf_round4's own limit).  Which starts share the batched launches (the small
 *                            range: d <= 128, q <= n0 <= 256, mc <= 4096, at most 256 sites to accept) is decided inside the call.
 *                            The bindings keep the loop of single calls where the batch does not pay (measured, DESIGN.md section
 *                            14: fewer than 8 starts, or fewer than one start per 32 candidates of the largest start).
 *   mrbf_dispatch_ps_batch   get_criticality(::PascolettiSerafiniConfig, ...) for n_starts starts in one call (mrbf_ps_step_batch):
 *                            device iff mrbf_dispatch_ps says so, d <= 256 (the fused evaluation kernels' range) and
 *                            1 <= n_starts <= 65535 (a grid dimension).  The bindings keep the loop of single calls where the
 *                            batch does not pay.
 *   mrbf_dispatch_ideal      compute_local_ideal_point (src/descent.jl:404-412) as a call of its own (mrbf_ideal_point_problem): what
 *                            mrbf_dispatch_ps returns -- the kernels and the limits are that step's.
 *   mrbf_dispatch_ideal_batch  the same for n_starts starts in one call (mrbf_ideal_point_batch): what mrbf_dispatch_ps_batch
 *                            returns.  The bindings keep the loop of single calls where the batch does not pay (DESIGN.md
 *                            section 24).
 *   mrbf_dispatch_db_batch   results_in_box_indices (src/Databases.jl:324-327) and the row gathers of n_starts resident databases in one
 *                            call (mrbf_db_box_batch, mrbf_db_gather_batch): device iff 1 <= n_starts <= 65535 (a grid dimension) and
 *                            1 <= d <= 4096; otherwise the scan and the copies run on the caller's host copy of the database.
 *                            mrbf_db_round3_batch, mrbf_db_append_batch and mrbf_db_set_values_batch (MRBF_ENTRY_DB_ROUND3,
 *                            _DB_APPEND_BATCH, _DB_SET_VALUES_BATCH) are routed by the same rule.
 *   mrbf_dispatch_eval_batch mrbf_eval of n_jobs (model, query block) pairs in one call (mrbf_eval_batch): device iff
 *                            1 <= n_jobs <= 65535 (a grid dimension).  Which jobs share launches is decided inside the call.
 *   mrbf_dispatch_eval_batch_min_jobs  the fewest jobs from which the bindings make that one call instead of the loop of mrbf_eval
 *                            (measured cells only, tools/eval_batch_bench.py, DESIGN.md section 18: admitted where the batch took
 *                            at most 0.8 of the loop's median -- 0.48 at 8 C4 evaluations, 0.16 at 8 acceptance-test pairs --;
 *                            monotone: every job count from the answer, 8, on takes the batch; fewer were not measured).
 *   mrbf_dispatch_hessian_batch  mrbf_eval_hessian of n_jobs (model, site block) pairs in one call (mrbf_eval_hessian_batch): device
 *                            iff 1 <= n_jobs <= 65535, the family's limit.
 *   mrbf_dispatch_hessian_batch_min_jobs  the fewest jobs from which the bindings make that one call instead of the loop of
 *                            mrbf_eval_hessian (measured cells only, tools/hessian_batch_bench.py, DESIGN.md section 20: admitted where
 *                            the batch took at most 0.8 of the loop's median on the parent build -- 0.54 at 2 C4 models with one
 *                            site each, 0.68 with 16 sites each --; monotone: every job count from the answer, 2, on takes the
 *                            batch; a value above 65535 would mean: the bindings keep the loop).
 *   mrbf_dispatch_after      the return code rc of a device entry point (MRBF_ENTRY_*) that means "take the reference method
 *                            for this call" (start set without the tail or rank deficient, limits of the device path) rather
 *                            than an error: 1 = fall back, 0 = rc is what it says. */
enum { MRBF_DISPATCH_REFERENCE = 0, MRBF_DISPATCH_DEVICE = 1 };
enum { MRBF_FIT_FULL = 0, MRBF_FIT_FROM_ROUND4 = 1 };
enum { MRBF_ENTRY_ROUND4 = 1, MRBF_ENTRY_FIT_FROM_ROUND4 = 2, MRBF_ENTRY_PS_STEP = 3, MRBF_ENTRY_BACKTRACK = 4, MRBF_ENTRY_AFFINE = 5,
       MRBF_ENTRY_SD = 6, MRBF_ENTRY_NORMAL = 7, MRBF_ENTRY_SD_STEP = 8, MRBF_ENTRY_SD_BATCH = 9, MRBF_ENTRY_AFFINE_BATCH = 10,
       MRBF_ENTRY_FIT_BATCH = 11, MRBF_ENTRY_NORMAL_BATCH = 12, MRBF_ENTRY_ROUND4_BATCH = 13, MRBF_ENTRY_PS_BATCH = 14,
       MRBF_ENTRY_DB_BOX = 15, MRBF_ENTRY_DB_GATHER = 16, MRBF_ENTRY_DB_ROUND3 = 17, MRBF_ENTRY_DB_APPEND_BATCH = 18,
       MRBF_ENTRY_DB_SET_VALUES_BATCH = 19, MRBF_ENTRY_EVAL_BATCH = 20, MRBF_ENTRY_HESSIAN_BATCH = 21,
       MRBF_ENTRY_DS = 22, MRBF_ENTRY_DS_BATCH = 23 };
enum { MRBF_ENTRY_DS_ROWS = 24 };
enum { MRBF_ENTRY_IDEAL = 25, MRBF_ENTRY_IDEAL_BATCH = 26 };
int32_t mrbf_dispatch_ps(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_ps_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints,
                               int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_ideal(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_ideal_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints,
                                  int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_sd(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_ds(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_ds_rows(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                              int32_t n_foreign);
int32_t mrbf_dispatch_normal(int32_t d, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign);
int32_t mrbf_dispatch_sd_step(int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints, int32_t n_foreign,
                              int32_t max_loops);
int32_t mrbf_dispatch_sd_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints,
                               int32_t n_lin_constraints, int32_t n_foreign, int32_t max_loops);
int32_t mrbf_dispatch_ds_batch(int64_t n_starts, int32_t d, int32_t k, int32_t n_models, int32_t n_nl_constraints,
                               int32_t n_lin_constraints, int32_t n_foreign, int32_t max_loops);
int32_t mrbf_dispatch_normal_batch(int64_t n_starts, int32_t d, int32_t n_models, int32_t n_nl_constraints, int32_t n_lin_constraints,
                                   int32_t n_foreign);
int32_t mrbf_dispatch_backtrack(int32_t n_objective_models, int32_t n_foreign, int32_t outputs_in_order);
int32_t mrbf_dispatch_affine(int64_t n_candidates, int32_t d);
int32_t mrbf_dispatch_affine_batch(int64_t n_starts, int32_t d, int32_t p_is_inf);
int32_t mrbf_dispatch_round4(int64_t n0, int32_t d, int32_t poly_deg, int64_t n_candidates);
int32_t mrbf_dispatch_fit_batch(int64_t n_starts);
int64_t mrbf_dispatch_fit_batch_max_n(int64_t n_starts, int32_t d);
int32_t mrbf_dispatch_fit_batch_lu(int64_t n_lu_starts, int64_t n_max, int32_t d);
int32_t mrbf_dispatch_round4_batch(int64_t n_starts, int32_t d);
int32_t mrbf_dispatch_db_batch(int64_t n_starts, int32_t d);
int32_t mrbf_dispatch_eval_batch(int64_t n_jobs);
int64_t mrbf_dispatch_eval_batch_min_jobs(void);
int32_t mrbf_dispatch_hessian_batch(int64_t n_jobs);
int64_t mrbf_dispatch_hessian_batch_min_jobs(void);
int32_t mrbf_dispatch_fit(int64_t n_training, int64_t state_n0, int32_t state_q, int32_t state_n_accepted, int32_t same_sites);
int32_t mrbf_dispatch_after(int32_t entry, int32_t rc);

/* ---- host-side helper of the Pascoletti-Serafini subproblem solver -------------------------------------------------
 * Stochastic ranking of one ISRES generation (Runarsson & Yao): lam sweeps over adjacent individuals, compared by
 * objective f when both are feasible (phi == 0) or with probability pf, else by constraint violation phi; stops after a
 * sweep without a swap.  Replaces what NLopt's GN_ISRES does internally for `_ps_optimization` /
 * `compute_local_ideal_point` (src/descent.jl:369-387, :478-510); the generation itself is evaluated by ONE mrbf_eval.
 * u: lam * (lam - 1) uniform random numbers in [0,1) (sweep-major), idx_out: the ranked permutation (best first).
 * Pure host code (no ctx, no device). */
int32_t mrbf_stochastic_rank(int32_t lam, const double *f, const double *phi, const double *u, double pf, int32_t *idx_out);

#ifdef __cplusplus
}
#endif
#endif /* MRBF_H */
