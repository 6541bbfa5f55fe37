# HipRbf.jl -- drop-in surrogate family for Morbit.jl backed by libmrbf.so (MI355X).
#
# NOT EXECUTED IN THIS REPOSITORY'S BUILD CONTAINER (no Julia there): this is the binding a Morbit maintainer adds next to
# src/models/RbfModel.jl (`include("models/HipRbf.jl")` in src/Morbit.jl after :87).  It implements the surrogate interface of
# src/AbstractSurrogateInterface.jl for a new config type `HipRbfConfig` by replacing every call into
# RadialBasisFunctionModels.jl on the hot path, plus the batched twins the descent code needs:
#     RBF.RBFInterpolationModel(...)               RbfModel.jl:759-763              -> mrbf_fit / mrbf_fit_from_round4
#     mod.model(x̂[, ℓ]), RBF.grad, RBF.jac         RbfModel.jl:784-799              -> mrbf_eval
#     RBF.get_matrices, kernels(ξ), the whole loop  RbfModel.jl:352-499 (_rbf_round4) -> mrbf_round4
#     candidate scan of the affine filter           AffinelyIndependentPoints.jl:71-106 -> mrbf_affine_scores
#     eval_container_*_at_scaled_site[s]            SurrogateContainer.jl:234-269     -> one mrbf_eval per grouped model
#     _backtrack                                    descent.jl:150-185                -> mrbf_backtrack
#     get_criticality(::PascolettiSerafiniConfig)   descent.jl:512-581                -> mrbf_ps_step_problem
# Which of Morbit's calls go to the device and which to Morbit's own methods is decided by the mrbf_dispatch_* functions of the
# library (include/mrbf.h, "decision table"), the same ones the Python mirror calls; no method here raises because of a size limit.
# Every ccall below has a 1:1 ctypes twin in morbit.jl_amd/_lib.py, which is what tests/ execute; struct layouts are pinned by
# tests/test_abi.py; tests/test_julia_binding.py parses every ccall of this file against include/mrbf.h.
# Conventions: a context is owned by one Julia task at a time (one per thread, created under a lock) and is NOT thread-safe, while
# finalizers run on whichever thread triggers the GC -- so EVERY ccall that passes a context handle runs inside `_locked(ctx)`, i.e.
# holding `ctx.lock` (finalizers `trylock` and re-schedule themselves); models keep their context alive and are released through
# it; buffers passed to ccall are GC.@preserve'd.
# INERT FOR NON-USERS: nothing in this file changes a run that does not select `HipRbfConfig`.  The three methods that extend Morbit
# functions on Morbit's own types (`Base.iterate` of the affine filter, `_backtrack`, `get_criticality` of the PS step) first look
# for a HipRbf object -- the task-local scan state set by `prepare_update_model(..., ::HipRbfConfig, ...)`, a `HipRbfModel` in the
# container -- and hand over to Morbit's method by `invoke` before anything of libmrbf is touched when there is none.

const libmrbf = get(ENV, "MRBF_LIB", "libmrbf.so")

struct MrbfFitInfo          # mirrors mrbf_fit_info (include/mrbf.h), 80 bytes
    path::Int32; factor_info::Int32; n::Int32; q::Int32
    rel_residual::Float64; max_pitw::Float64; mu::Float64
    ms_gram::Float32; ms_project::Float32; ms_factor::Float32; ms_solve::Float32; ms_check::Float32; ms_total::Float32
    fallbacks::Int32; giveup_code::Int32
    ms_factor_device::Float32; slow_launches::Int32
end
struct MrbfPsOptions        # mirrors mrbf_ps_options, 40 bytes
    max_ideal_evals::Int32; max_ps_evals::Int32; max_polish_evals::Int32; reserved::Int32
    seed::UInt64; t0::Float64; xtol_rel::Float64
end
struct MrbfPsInfo           # mirrors mrbf_ps_info, 32 bytes
    status::Int32; generations::Int32; evals_ideal::Int32; evals_ps::Int32; evals_polish::Int32; ms_total::Float32
    tau::Float64
end
struct MrbfIdealInfo        # mirrors mrbf_ideal_info, 20 bytes
    evals_ideal::Int32; generations::Int32; found::Int32; refined::Int32; ms_total::Float32
end

struct MrbfSdInfo          # mirrors mrbf_sd_info, 24 bytes
    status::Int32; iterations::Int32; bound_flips::Int32; ms_total::Float32
    omega::Float64
end

struct MrbfDsInfo          # mirrors mrbf_ds_info, 24 bytes
    status::Int32; iterations::Int32; dropped::Int32; ms_total::Float32
    omega::Float64
end

struct MrbfNormalInfo      # mirrors mrbf_normal_info, 32 bytes
    status::Int32; iterations::Int32; bound_flips::Int32; ms_total::Float32
    alpha::Float64; delta::Float64
end

struct MrbfSdStepOptions    # mirrors mrbf_sd_step_options, 32 bytes
    strict::Int32; max_loops::Int32
    const_rhs::Float64; shrink::Float64; min_stepsize::Float64
end

struct MrbfSdStepInfo       # mirrors mrbf_sd_step_info, 40 bytes
    branch::Int32; loops::Int32; ms_total::Float32
    sigma::Float64; omega::Float64; step_norm::Float64
end

struct MrbfSdBatchRecord    # mirrors mrbf_sd_batch_record, 56 bytes
    sd_status::Int32; iterations::Int32; bound_flips::Int32; branch::Int32; loops::Int32; reserved::Int32
    omega::Float64; omega_step::Float64; sigma::Float64; step_norm::Float64
end

struct MrbfDsBatchRecord    # mirrors mrbf_ds_batch_record, 64 bytes
    ds_status::Int32; iterations::Int32; dropped::Int32; branch::Int32; loops::Int32; reserved::Int32
    omega::Float64; omega_step::Float64; sigma::Float64; step_norm::Float64; dnorm::Float64
end

struct MrbfNormalBatchRecord    # mirrors mrbf_normal_batch_record, 32 bytes
    status::Int32; iterations::Int32; bound_flips::Int32; reserved::Int32
    alpha::Float64; delta::Float64
end

struct MrbfAffineJob        # mirrors mrbf_affine_job, 64 bytes
    mc::Int64
    j0::Int32; max_picks::Int32
    pivot_val::Float64
    shifted::Ptr{Float64}; Q0::Ptr{Float64}; picked_out::Ptr{Int64}; Z_out::Ptr{Float64}
    n_picked::Int32; reserved::Int32
end

struct MrbfRound4Job        # mirrors mrbf_round4_job, 88 bytes
    n0::Int64; mc::Int64
    start_sites::Ptr{Float64}; cand_sites::Ptr{Float64}
    kernel_id::Int32; poly_deg::Int32
    a::Float64; b::Float64
    max_points::Int32
    theta_pivot_cholesky::Float64
    accepted_out::Ptr{Int32}
    n_accepted::Int32; rc::Int32
end

struct MrbfFitJob           # mirrors mrbf_fit_job, 168 bytes
    n::Int64
    d::Int32; k::Int32; kernel_id::Int32; poly_deg::Int32
    a::Float64; b::Float64
    centres::Ptr{Float64}; values::Ptr{Float64}; weights_out::Ptr{Float64}; poly_out::Ptr{Float64}
    model::Ptr{Cvoid}
    status::Int32; reserved::Int32
    info::MrbfFitInfo
end

struct MrbfEvalJob          # mirrors mrbf_eval_job, 48 bytes
    model::Ptr{Cvoid}
    m::Int64
    X::Ptr{Float64}; vals_out::Ptr{Float64}; jac_out::Ptr{Float64}
    status::Int32; reserved::Int32
end

struct MrbfHessInfo         # mirrors mrbf_hess_info, 16 bytes
    ms_total::Float32; nsplit::Int32; chunks::Int32; reserved::Int32
end

struct MrbfHessJob          # mirrors mrbf_hess_job, 56 bytes
    model::Ptr{Cvoid}
    m::Int64
    X::Ptr{Float64}; rows::Ptr{Int32}; hess_out::Ptr{Float64}
    n_rows::Int32; status::Int32; nsplit::Int32; reserved::Int32
end

struct MrbfHessBatchInfo    # mirrors mrbf_hess_batch_info, 16 bytes
    ms_total::Float32; chunks::Int32; groups::Int32; single_inside::Int32
end

struct MrbfPsProblem        # mirrors mrbf_ps_problem, 72 bytes
    n_models::Int32; n_objectives::Int32
    models::Ptr{Ptr{Cvoid}}; roles::Ptr{Int32}
    n_lin_eq::Int32; n_lin_ineq::Int32
    A_eq::Ptr{Float64}; b_eq::Ptr{Float64}; A_ineq::Ptr{Float64}; b_ineq::Ptr{Float64}
    eq_tol::Float64
end

const MRBF_KERNEL_ID = Dict(k => Int32(i - 1) for (i, k) in enumerate(RbfKernels))  # order of RbfModel.jl:48-54

# ---- context: one per thread, created under a lock; live models are registered so that shutdown never outruns them -------
mutable struct MrbfContext
    handle::Ptr{Cvoid}
    models::Set{Ptr{Cvoid}}        # handles of live models / round-4 states created through this context
    lock::ReentrantLock
    function MrbfContext(device::Integer = -1)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:mrbf_init, libmrbf), Int32, (Int32, Ref{Ptr{Cvoid}}), device, h)
        rc == 0 || error("mrbf_init failed ($rc): ", unsafe_string(ccall((:mrbf_last_error, libmrbf), Cstring, (Ptr{Cvoid},), C_NULL)))
        ctx = new(h[], Set{Ptr{Cvoid}}(), ReentrantLock())
        finalizer(_shutdown!, ctx)
        return ctx
    end
end
function _shutdown!(ctx::MrbfContext)
    # finalizers may run on any thread: never block in one -- hand the work to a task if the lock is busy
    if !trylock(ctx.lock)
        @async _shutdown!(ctx)
        return nothing
    end
    try
        if ctx.handle != C_NULL
            for m in ctx.models   # models first: mrbf_shutdown deletes the context they would be released through
                ccall((:mrbf_free_model, libmrbf), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.handle, m)
            end
            empty!(ctx.models)
            ccall((:mrbf_shutdown, libmrbf), Int32, (Ptr{Cvoid},), ctx.handle)
            ctx.handle = C_NULL   # later model finalizers see a closed context and do nothing
        end
    finally
        unlock(ctx.lock)
    end
    return nothing
end

const _CTX = Dict{Int,MrbfContext}()
const _CTX_LOCK = ReentrantLock()
"The calling thread's context (a ctx is not thread-safe; ctxs are independent)."
mrbf_context() = lock(_CTX_LOCK) do
    get!(() -> MrbfContext(), _CTX, Threads.threadid())
end

"""
Run `f(handle)` holding the context's lock.  A context is documented as not thread-safe (include/mrbf.h) and model / round-4
finalizers may run on any thread (whichever triggers the GC, e.g. under the `Threads.@threads` loop of
examples/large_scale_benchmarks.jl:253): they `trylock` this same lock and re-schedule themselves when it is busy, so a handle is
never released from thread B while thread A is inside a compute call of the same context.  Reentrant.
"""
function _locked(f, ctx::MrbfContext)
    lock(ctx.lock)
    try
        ctx.handle == C_NULL && error("libmrbf context was shut down")
        return f(ctx.handle)
    finally
        unlock(ctx.lock)
    end
end

function _check(ctx::MrbfContext, rc::Int32)
    rc == 0 && return nothing
    msg = _locked(ctx) do h
        unsafe_string(ccall((:mrbf_last_error, libmrbf), Cstring, (Ptr{Cvoid},), h))
    end
    # MRBF_ENOTPD = 1, MRBF_ESINGULAR = 2: numerical failures the algorithm can react to (rebuild / not fully linear)
    rc in (1, 2) ? throw(LinearAlgebra.SingularException(Int(rc))) : error("libmrbf error $rc: $msg")
end

# ---- config: every RbfConfig field, same defaults and the same six assertions (RbfModel.jl:66-112) ------------------------
@with_kw struct HipRbfConfig <: AbstractSurrogateConfig
    kernel::Symbol = :cubic
    shape_parameter::Union{String,Float64} = NaN
    polynomial_degree::Int64 = 1
    θ_enlarge_1::Float64 = 2
    θ_enlarge_2::Float64 = 2
    θ_pivot::Float64 = 1 / (2 * θ_enlarge_1)
    θ_pivot_cholesky::Float64 = 1e-7
    require_linear::Bool = true
    max_model_points::Int64 = -1
    use_max_points::Bool = false
    optimized_sampling = true
    max_evals::Int64 = typemax(Int64)
    @assert θ_enlarge_1 * θ_pivot ≤ 1 "θ_pivot must be <= θ_enlarge_1^(-1)."
    @assert kernel ∈ RbfKernels "`kernel` not supported. See `Morbit.RbfKernels` for available symbols."
    @assert kernel != :thin_plate_spline || shape_parameter isa String || isnan(shape_parameter) ||
            (shape_parameter % 1 == 0 && shape_parameter >= 1) "Invalid shape_parameter for :thin_plate_spline."
    @assert kernel != :cubic || shape_parameter isa String || isnan(shape_parameter) ||
            (shape_parameter % 1 == 0 && shape_parameter % 2 == 1) "Invalid shape_parameter for :cubic."
    @assert shape_parameter isa String || isnan(shape_parameter) || shape_parameter > 0 "Shape parameter must be strictly positive."
    @assert θ_enlarge_1 >= 1 && θ_enlarge_2 >= 1 "θ's must be >= 1."
    @assert -1 <= polynomial_degree <= 1
end
# the sampling code only reads fields, so it works on either config type
_as_rbf_config(cfg::HipRbfConfig) = RbfConfig(; (fn => getfield(cfg, fn) for fn in fieldnames(RbfConfig))...)

max_evals(cfg::HipRbfConfig)::Int = cfg.max_evals
combinable(cfg::HipRbfConfig)::Bool = true
Base.hash(cfg::HipRbfConfig, h::UInt) = hash(Tuple(getfield(cfg, fn) for fn in fieldnames(HipRbfConfig)), h)
Base.isequal(a::HipRbfConfig, b::HipRbfConfig) = all(isequal(getfield(a, fn), getfield(b, fn)) for fn in fieldnames(HipRbfConfig))
Base.:(==)(a::HipRbfConfig, b::HipRbfConfig) = isequal(a, b)
get_saveable_type(::HipRbfConfig, x::AbstractVector{F}, y) where {F<:AbstractFloat} = RbfMeta{F,Nothing}

# (kernel id, a, b) from _get_kernel_params (RbfModel.jl:665-690); NaN -> the package defaults
function _mrbf_kernel_params(Δ, cfg)
    p = _get_kernel_params(Δ, _as_rbf_config(cfg))
    kid = MRBF_KERNEL_ID[cfg.kernel]
    cfg.kernel == :gaussian && return kid, Float64(something(p, 1.0)), 0.0
    cfg.kernel in (:multiquadric, :inv_multiquadric) && return kid, Float64(p === nothing ? 1.0 : p[1]), 0.5
    cfg.kernel == :cubic && return kid, Float64(something(p, 3)), 0.0
    return kid, Float64(something(p, 2)), 0.0   # :thin_plate_spline
end

# ---- model ------------------------------------------------------------------------------------------------------------------
mutable struct HipRbfModel <: AbstractSurrogate
    ctx::MrbfContext            # keeps the context alive as long as the model is reachable
    handle::Ptr{Cvoid}          # mrbf_model*, device resident centres / weights
    n_vars::Int
    num_outputs::Int
    fully_linear::Bool
    info::MrbfFitInfo
    function HipRbfModel(ctx, handle, n_vars, k, fl, info)
        m = new(ctx, handle, n_vars, k, fl, info)
        lock(ctx.lock) do
            push!(ctx.models, handle)
        end
        finalizer(_free_model!, m)
        return m
    end
end
function _free_model!(m::HipRbfModel)
    ctx = m.ctx
    if !trylock(ctx.lock)
        @async _free_model!(m)
        return nothing
    end
    try
        if ctx.handle != C_NULL && m.handle in ctx.models   # not yet released by the context's own shutdown
            delete!(ctx.models, m.handle)
            ccall((:mrbf_free_model, libmrbf), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.handle, m.handle)
        end
        m.handle = C_NULL
    finally
        unlock(ctx.lock)
    end
    return nothing
end
fully_linear(m::HipRbfModel)::Bool = m.fully_linear
num_outputs(m::HipRbfModel) = m.num_outputs
set_fully_linear!(m::HipRbfModel, val) = (m.fully_linear = val; nothing)

# ---- the decision table (include/mrbf.h, "decision table"): pure host functions of libmrbf that the Python mirror calls as well,
#      so both bindings route every call the same way; 1 = device entry point, 0 = Morbit's own method
_dispatch_ps(d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ps, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32), d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_ps_batch(n_starts, d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ps_batch, libmrbf), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Int32),
          n_starts, d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_ideal(d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ideal, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32), d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_ideal_batch(n_starts, d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ideal_batch, libmrbf), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Int32),
          n_starts, d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_sd(d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_sd, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32), d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_ds(d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ds, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32), d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_normal(d, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_normal, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32), d, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_sd_step(d, k, n_models, n_nl, n_lin, n_foreign, max_loops) =
    ccall((:mrbf_dispatch_sd_step, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32, Int32),
          d, k, n_models, n_nl, n_lin, n_foreign, max_loops) == 1
_dispatch_sd_batch(n_starts, d, k, n_models, n_nl, n_lin, n_foreign, max_loops) =
    ccall((:mrbf_dispatch_sd_batch, libmrbf), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Int32, Int32),
          n_starts, d, k, n_models, n_nl, n_lin, n_foreign, max_loops) == 1
_dispatch_ds_rows(d, k, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_ds_rows, libmrbf), Int32, (Int32, Int32, Int32, Int32, Int32, Int32), d, k, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_ds_batch(n_starts, d, k, n_models, n_nl, n_lin, n_foreign, max_loops) =
    ccall((:mrbf_dispatch_ds_batch, libmrbf), Int32, (Int64, Int32, Int32, Int32, Int32, Int32, Int32, Int32),
          n_starts, d, k, n_models, n_nl, n_lin, n_foreign, max_loops) == 1
_dispatch_normal_batch(n_starts, d, n_models, n_nl, n_lin, n_foreign) =
    ccall((:mrbf_dispatch_normal_batch, libmrbf), Int32, (Int64, Int32, Int32, Int32, Int32, Int32),
          n_starts, d, n_models, n_nl, n_lin, n_foreign) == 1
_dispatch_backtrack(n_models, n_foreign, in_order::Bool) =
    ccall((:mrbf_dispatch_backtrack, libmrbf), Int32, (Int32, Int32, Int32), n_models, n_foreign, in_order) == 1
_dispatch_affine(n_candidates, d) = ccall((:mrbf_dispatch_affine, libmrbf), Int32, (Int64, Int32), n_candidates, d) == 1
_dispatch_affine_batch(n_starts, d, p) =
    ccall((:mrbf_dispatch_affine_batch, libmrbf), Int32, (Int64, Int32, Int32), n_starts, d, isinf(p) ? 1 : 0) == 1
_dispatch_fit_batch(n_starts) = ccall((:mrbf_dispatch_fit_batch, libmrbf), Int32, (Int64,), n_starts) == 1
_dispatch_fit_batch_max_n(n_starts, d) = Int(ccall((:mrbf_dispatch_fit_batch_max_n, libmrbf), Int64, (Int64, Int32), n_starts, d))
_dispatch_fit_batch_lu(n_lu_starts, n_max, d) = ccall((:mrbf_dispatch_fit_batch_lu, libmrbf), Int32, (Int64, Int64, Int32), n_lu_starts, n_max, d) == 1
# is a start on the LU path (fit_model, solve.hip: the kernel's order exceeds what the tail covers, or n == q) and inside the range of
# MRBF_OPT_SMALL_LU (n <= 512, d <= 128, k <= 16, n >= q, a smooth kernel)?  params = (kernel id, a, b) as _mrbf_kernel_params gives them
function _takes_small_lu(params, deg, n, d, k)
    kid, a, b = params
    q = deg < 0 ? 0 : (deg == 0 ? 1 : d + 1)
    order = kid == 0 ? ceil(Int, a / 2) : (kid == 2 ? ceil(Int, b) : (kid == 3 ? Int(a) + 1 : 0))
    nonsmooth = (kid == 0 || kid == 3) && a == 1
    return !(order <= deg + 1 && n > q) && n >= q && n <= 512 && d <= 128 && k <= 16 && !nonsmooth
end
_dispatch_eval_batch(n_jobs) = ccall((:mrbf_dispatch_eval_batch, libmrbf), Int32, (Int64,), n_jobs) == 1
# where `hip_eval_models_many` takes the one call: from the job count the table names on (measured, DESIGN.md section 18)
_eval_batch_pays(n_jobs) = n_jobs >= ccall((:mrbf_dispatch_eval_batch_min_jobs, libmrbf), Int64, ())
_dispatch_hessian_batch(n_jobs) = ccall((:mrbf_dispatch_hessian_batch, libmrbf), Int32, (Int64,), n_jobs) == 1
# where `hip_get_hessians_many` takes the one call: from the job count the table names on (measured, DESIGN.md section 20)
_hessian_batch_pays(n_jobs) = n_jobs >= ccall((:mrbf_dispatch_hessian_batch_min_jobs, libmrbf), Int64, ())
_dispatch_round4_batch(n_starts, d) = ccall((:mrbf_dispatch_round4_batch, libmrbf), Int32, (Int64, Int32), n_starts, d) == 1
_dispatch_round4(n0, d, deg, n_candidates) =
    ccall((:mrbf_dispatch_round4, libmrbf), Int32, (Int64, Int32, Int32, Int64), n0, d, deg, n_candidates) == 1
_dispatch_fit(n_training, n0, q, n_accepted, same_sites::Bool) =
    ccall((:mrbf_dispatch_fit, libmrbf), Int32, (Int64, Int64, Int32, Int32, Int32), n_training, n0, q, n_accepted, same_sites) == 1
"Does return code `rc` of device entry point `entry` (1 round4, 2 fit_from_round4, 3 ps_step) mean: take the reference method?"
# Where `hip_round4_many` takes the batched call (measured: tools/round4_batch_bench.py, DESIGN.md section 14): at least 8 starts, and at
# least one start per 32 candidates of the largest start; below that the loop of single calls is faster.
const ROUND4_BATCH_MIN_STARTS = 8
const ROUND4_BATCH_CANDIDATES_PER_START = 32
_round4_batch_pays(n_starts, max_candidates) = n_starts >= ROUND4_BATCH_MIN_STARTS && n_starts * ROUND4_BATCH_CANDIDATES_PER_START >= max_candidates
# Where `hip_ps_criticality_many` takes the batched call (tools/ps_batch_bench.py, DESIGN.md section 15): the batch of one is the single
# call itself, from two starts on the starts share every generation's launches and every refinement iteration's synchronisation.
const PS_BATCH_MIN_STARTS = 2
_ps_batch_pays(n_starts) = n_starts >= PS_BATCH_MIN_STARTS
# from this many starts on ONE mrbf_ideal_point_batch call, below the loop of mrbf_ideal_point_problem calls (measured, DESIGN.md
# section 24: batch / loop = 0.81 at 2 starts, above the 0.8 that admits a count; 0.40 at 8)
const IDEAL_BATCH_MIN_STARTS = 8
_fallback_rc(entry, rc) = ccall((:mrbf_dispatch_after, libmrbf), Int32, (Int32, Int32), entry, rc) == 1

# ---- two-phase construction: phase I (which sites) stays Morbit's control flow (RbfModel.jl:506-655 is generic in `cfg`); the
#      pieces of it that are arithmetic are re-routed by dispatch on the config / element type:
#        _rbf_round4(..., cfg::HipRbfConfig)                       -> mrbf_round4, factors kept for the fit
#        iterate(::AffinelyIndependentPointFilter{Float64}, n)    -> mrbf_affine_scores for large candidate sets, ONLY while the
#                                                                    task-local scan state of a HipRbfConfig's update is set
_get_signature(cfg::HipRbfConfig) = (cfg.θ_pivot, cfg.θ_enlarge_1, cfg.θ_enlarge_2, cfg.optimized_sampling)   # RbfModel.jl:114

function prepare_init_model(cfg::HipRbfConfig, func_indices, mop, scal, id, sdb, ac; ensure_fully_linear = true, kwargs...)
    F = eltype(get_x_scaled(id))                                                 # RbfModel.jl:506-513
    meta = RbfMeta{F,typeof(func_indices)}(; signature = _get_signature(cfg), func_indices)
    return prepare_update_model(nothing, meta, cfg, func_indices, mop, scal, id, sdb, ac; ensure_fully_linear, kwargs...)
end
# Morbit's generic method (first argument Union{Nothing,RbfModel}, `cfg` untyped); run with `nothing` as the model it never looks at.
# Two methods so that neither is ambiguous with the generic one for a `nothing` model.
const _GENERIC_PREPARE_SIG = Tuple{Union{Nothing,RbfModel},RbfMeta,Any,Any,Any,Any,Any,Any,Any}
# While Morbit's generic method runs FOR A HipRbfConfig, the task carries a scan state: that -- not the element type of the filter --
# is what routes the affine filter's candidate scan (rounds 1-2) to the device.  The filter is built without a config
# (RbfModel.jl:219), so the config cannot be dispatched on there; a plain `RbfConfig` run never sets the key, on any task.
const _HIP_AFFINE_KEY = :HipRbf_affine_scan
# Householder QR of Y = [y_1 .. y_j] kept up to date as the filter picks sites, with the FULL orthogonal factor explicit: appending a
# column is one reflector on the trailing rows, Q <- Q diag(I_j, H) -- a rank-1 update of Q's trailing columns, O(d^2) per pick.  Morbit
# re-factors Y after every pick (`_orthogonal_complement_matrix`, AffinelyIndependentPoints.jl:4-11: O(d^3) per pick, O(d^4) per filter;
# 140-280 ms per model update at d = 128, more than round 4, the fit and the descent step together -- profiles/r06_iteration_c4.txt).
# Same reflectors as LAPACK's geqrf (larfg: beta = -sign(alpha) |x|, v_1 = 1): Q equals qr(Y)'s to rounding, the picks are Morbit's.
# (1:1 twin of `_GrowingQR` in morbit.jl_amd/sampling.py, which tests/test_sampling.py holds against the from-scratch factorisation.)
mutable struct HipRbfGrowingQR
    Q::Matrix{Float64}
    j::Int
end
function HipRbfGrowingQR(Y::AbstractMatrix)
    d = size(Y, 1)
    Q = size(Y, 2) == 0 ? Matrix{Float64}(I, d, d) : qr(Matrix{Float64}(Y)).Q * Matrix{Float64}(I, d, d)
    return HipRbfGrowingQR(Q, size(Y, 2))
end
function _append!(g::HipRbfGrowingQR, y::AbstractVector)
    d = size(g.Q, 1); j = g.j
    j >= d && return g
    Qt = view(g.Q, :, j+1:d)
    x = Qt' * Vector{Float64}(y)                       # the new column in the current basis, trailing part
    α = x[1]; xn = norm(view(x, 2:length(x)))
    if xn != 0
        β = -copysign(hypot(α, xn), α)
        τ = (β - α) / β
        v = x ./ (α - β); v[1] = 1.0
        Qt .-= (Qt * v) * (τ .* v)'                    # Q[:, j+1:d] H
    end
    g.j = j + 1
    return g
end
function _complement(g::HipRbfGrowingQR, p)
    Z = g.Q[:, g.j+1:end]
    size(Z, 2) > 0 && (Z ./= norm.(eachcol(Z), p)')   # AffinelyIndependentPoints.jl:7-9
    return Z
end

mutable struct HipRbfPickQueue               # what ONE mrbf_affine_select call picked for a filter, handed out pick by pick
    picks::Vector{Int}
    pos::Int
    Z::Matrix{Float64}                      # the filter's final complement basis
end
mutable struct HipRbfAffineScan
    seeds::IdDict{Any,Matrix{Float64}}      # filter => d x mc matrix of shifted seeds, picked columns zeroed (task-local, no global)
    qrs::IdDict{Any,HipRbfGrowingQR}        # filter => the growing factorisation of its Y (host scan)
    queues::IdDict{Any,HipRbfPickQueue}     # filter => the device's picks (device scan)
end
HipRbfAffineScan() = HipRbfAffineScan(IdDict{Any,Matrix{Float64}}(), IdDict{Any,HipRbfGrowingQR}(), IdDict{Any,HipRbfPickQueue}())
_hip_affine_scan() = get(task_local_storage(), _HIP_AFFINE_KEY, nothing)
_prepare_with_device_scan(meta, cfg::HipRbfConfig, args...; kwargs...) =
    task_local_storage(_HIP_AFFINE_KEY, HipRbfAffineScan()) do
        invoke(prepare_update_model, _GENERIC_PREPARE_SIG, nothing, meta, cfg, args...; kwargs...)
    end
prepare_update_model(mod::Nothing, meta::RbfMeta, cfg::HipRbfConfig, func_indices, mop, scal, iter_data, sdb, ac; kwargs...) =
    _prepare_with_device_scan(meta, cfg, func_indices, mop, scal, iter_data, sdb, ac; kwargs...)
prepare_update_model(mod::HipRbfModel, meta::RbfMeta, cfg::HipRbfConfig, func_indices, mop, scal, iter_data, sdb, ac; kwargs...) =
    _prepare_with_device_scan(meta, cfg, func_indices, mop, scal, iter_data, sdb, ac; kwargs...)
# the improvement step only reads config fields (RbfModel.jl:699-732)
prepare_improve_model(mod::Union{Nothing,HipRbfModel}, meta::RbfMeta, cfg::HipRbfConfig, args...; kwargs...) =
    prepare_improve_model(nothing, meta, _as_rbf_config(cfg), args...; kwargs...)

init_model(meta::RbfMeta, cfg::HipRbfConfig, func_indices, mop, scal, iter_data, sdb, ac; kwargs...) =
    update_model(nothing, meta, cfg, func_indices, mop, scal, iter_data, sdb, ac; kwargs...)
improve_model(mod, meta::RbfMeta, cfg::HipRbfConfig, args...; kwargs...) = update_model(mod, meta, cfg, args...; kwargs...)

# sites / values in the ABI layouts: centres n x d row-major == the d x n column-major Matrix, values n x k row-major == k x n.
# A Vector{SVector{d,Float64}} / Vector{MVector{k,Float64}} already IS those bytes: reinterpret it (no copy); anything else
# (Float32 sites, plain Vectors) is materialised once.
_as_matrix(v::Vector{StaticArrays.SVector{N,Float64}}) where {N} = reshape(reinterpret(Float64, v), N, length(v))   # zero-copy view
_as_matrix(v) = Matrix{Float64}(reduce(hcat, v))      # MVectors (heap objects), Float32 sites, plain Vectors: one d x n copy
_dense(A::Matrix{Float64}) = A
_dense(A::Base.ReshapedArray{Float64,2,<:Base.ReinterpretArray{Float64}}) = A   # dense, stride 1: ccall takes its pointer as it is
_dense(A) = Matrix{Float64}(A)

# ---- round 4 (RbfModel.jl:352-499) inside Morbit's own prepare_update_model: same arguments, same return value (database indices
#      of the accepted sites in acceptance order); the whole selection is ONE device call and its factor is kept for update_model
const _ROUND4_KEPT = IdDict{Any,Any}()          # sub-database => (state, training indices in factor order)
const _ROUND4_LOCK = ReentrantLock()
function _rbf_round4(db, lb_2, ub_2, x::AbstractVector{F}, Δ, indices_found_so_far, cfg::HipRbfConfig) where {F}
    lock(_ROUND4_LOCK) do
        delete!(_ROUND4_KEPT, db)               # whatever was kept belongs to an older training set
    end
    n_vars = length(x)
    max_points = cfg.max_model_points <= 0 ? Int(((n_vars + 1) * (n_vars + 2)) / 2) : cfg.max_model_points   # :356
    N = length(indices_found_so_far)
    candidate_indices_4 = results_in_box_indices(db, lb_2, ub_2, indices_found_so_far)
    (N < max_points && (!isempty(candidate_indices_4) || cfg.use_max_points)) || return Int[]                  # :367
    # with use_max_points the reference draws random box points one by one once the database candidates are used up (:405-416, at
    # most 10 max_points + 1); here they are drawn up front so that they ride in the same device call
    fresh = cfg.use_max_points ? [_rand_box_point(lb_2, ub_2, F) for _ = 1:(10 * max_points + 1)] : Vector{Vector{F}}()
    cand_sites = [get_site.(db, candidate_indices_4); fresh]
    if _dispatch_round4(N, n_vars, cfg.polynomial_degree, length(cand_sites))
        rc, accepted, state = rbf_round4_device(cfg, Δ, get_site.(db, indices_found_so_far), cand_sites; keep_state = true, rc_only = true)
        if rc == 0
            round4_indices = Int[]
            for pos in accepted
                id = pos <= length(candidate_indices_4) ? candidate_indices_4[pos] : new_result!(db, cand_sites[pos], F[])   # :455-457
                push!(round4_indices, id)
            end
            if state !== nothing
                lock(_ROUND4_LOCK) do
                    _ROUND4_KEPT[db] = (state, [collect(Int, indices_found_so_far); round4_indices])
                end
            end
            return round4_indices
        end
        _fallback_rc(1, rc) || _check(mrbf_context(), rc)       # a start set without the tail / rank deficient: Morbit's own loop
    end
    return _rbf_round4(db, lb_2, ub_2, x, Δ, indices_found_so_far, _as_rbf_config(cfg))
end

# ---- rounds 1-2: the candidate scan of the affine filter (AffinelyIndependentPoints.jl:71-106) with many candidates; picks, order
#      and the Y / Z bookkeeping are the reference's.  Routed by the task-local scan state of a HipRbfConfig's model update: without
#      it (every plain RbfConfig run) the first statement hands over to Morbit's own method -- no ccall, no library needed.
function Base.iterate(filter::AffinelyIndependentPointFilter{Float64,VF,SV}, num_found::Int) where {VF,SV}
    scan = _hip_affine_scan()
    scan === nothing && return invoke(Base.iterate, Tuple{AffinelyIndependentPointFilter,Int}, filter, num_found)
    done() = (delete!(scan.seeds, filter); delete!(scan.qrs, filter); delete!(scan.queues, filter); nothing)
    num_found == filter.n && return done()
    isempty(filter.candidate_indices) && return done()
    S = get!(scan.seeds, filter) do
        M = Matrix{Float64}(_as_matrix(filter.shifted_seeds))    # a copy: picked columns are zeroed below
        for j in setdiff(eachindex(filter.shifted_seeds), filter.candidate_indices)
            M[:, j] .= 0                                   # chosen sites score 0 (the reference removes them from the list)
        end
        M
    end
    if haskey(scan.queues, filter) || _dispatch_affine(length(filter.candidate_indices), length(filter.x_0))
        # many candidates (decision table): the whole remaining selection is ONE device call (mrbf_affine_select: the factorisation of Y
        # grows by a reflector per pick on the device, no host round trip between picks); its picks are handed out one per call
        queue = get!(scan.queues, filter) do
            g = HipRbfGrowingQR(filter.Y)
            picks, Zf = affine_select(S, g.Q, g.j, filter.n - num_found, Float64(filter.pivot_val), filter.p)
            HipRbfPickQueue(picks, 0, Zf)
        end
        queue.pos >= length(queue.picks) && return done()
        queue.pos += 1
        i = queue.picks[queue.pos]
        filter.Y = hcat(filter.Y, filter.shifted_seeds[i])
        setdiff!(filter.candidate_indices, i)
        queue.pos == length(queue.picks) && (filter.Z = queue.Z)
        return (filter.return_indices ? i : filter.seeds[i]), num_found + 1
    end
    # few candidates: two host BLAS products per pick -- the same scores -- and the factorisation grown by a reflector per pick
    best_index, best_val = _affine_scores_host(S, filter.Z, filter.p)
    if best_index >= 1 && best_val > filter.pivot_val
        i = best_index
        g = get!(() -> HipRbfGrowingQR(filter.Y), scan.qrs, filter)     # (factor of the sites found so far, before this one joins)
        filter.Y = hcat(filter.Y, filter.shifted_seeds[i])
        _append!(g, filter.shifted_seeds[i])
        filter.Z = _complement(g, filter.p)
        setdiff!(filter.candidate_indices, i)
        S[:, i] .= 0
        return (filter.return_indices ? i : filter.seeds[i]), num_found + 1
    end
    return done()
end
"`‖Z (Zᵀ s)‖_p` of every column s of S on the host; first maximiser like the `>` scan of AffinelyIndependentPoints.jl:80-89"
function _affine_scores_host(S::Matrix{Float64}, Z::AbstractMatrix, p)
    size(Z, 2) == 0 && return 0, -Inf
    P = Z * (Z' * S)
    best_val, best = findmax([norm(view(P, :, c), p) for c in axes(P, 2)])
    return best, best_val
end

# ---- phase II: the fit.  With a kept round-4 factor that describes exactly this training set: two triangular solves
#      (mrbf_fit_from_round4, the reference's TODO at RbfModel.jl:657-660); otherwise Gram + factorisation + solve (mrbf_fit)
function update_model(mod::Union{Nothing,HipRbfModel}, meta::RbfMeta, cfg::HipRbfConfig,
                      func_indices, mop, scal, iter_data, sdb, ac; kwargs...)
    db = get_sub_db(sdb, func_indices)
    Δ = get_delta(iter_data)
    training_indices = _collect_indices(meta)                                  # RbfModel.jl:754-757
    training_results = get_result.(db, training_indices)
    sites = get_site.(training_results); values = get_value.(training_results)
    kept = lock(_ROUND4_LOCK) do
        pop!(_ROUND4_KEPT, db, nothing)
    end
    if kept !== nothing
        state, ids = kept
        n0, nacc, q = _round4_dims(state, cfg, length(first(sites)))
        if _dispatch_fit(length(training_indices), n0, q, nacc, ids == training_indices)
            rc, model = fit_from_round4(state, values, length(first(sites)), meta.fully_linear; rc_only = true)
            _free_round4!(state)                 # released here, not left to the finalizer (as sampling.py does)
            rc == 0 && return model, meta
            _fallback_rc(2, rc) || _check(state.ctx, rc)
        else
            _free_round4!(state)
        end
    end
    C = _dense(_as_matrix(sites))
    Y = _dense(_as_matrix(values))
    d, n = size(C)
    k = size(Y, 1)
    kid, a, b = _mrbf_kernel_params(Δ, cfg)
    ctx = mrbf_context()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    info = Ref{MrbfFitInfo}()
    rc = GC.@preserve C Y begin
        _locked(ctx) do hctx
            ccall((:mrbf_fit, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64, Int32,
                   Ref{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfFitInfo}),
                  hctx, n, d, k, C, Y, kid, a, b, cfg.polynomial_degree, h, C_NULL, C_NULL, info)
        end
    end
    _check(ctx, rc)
    @logmsg loglevel3 "The model is $(meta.fully_linear ? "" : "not ")fully linear (solve path $(info[].path), residual $(info[].rel_residual))."
    return HipRbfModel(ctx, h[], d, k, meta.fully_linear, info[]), meta
end

# ---- evaluation: single site (reference API) and batched twins -----------------------------------------------------------------
function _mrbf_eval(mod::HipRbfModel, X::Matrix{Float64}; values::Bool = true, jac::Bool = false)
    d, m, k = mod.n_vars, size(X, 2), mod.num_outputs            # X is d x m column-major == m x d row-major
    V = values ? Matrix{Float64}(undef, k, m) : nothing          # k x m column-major == m x k row-major
    J = jac ? Array{Float64,3}(undef, k, d, m) : nothing         # per point a k x d column-major block
    rc = GC.@preserve X V J begin
        _locked(mod.ctx) do hctx
            ccall((:mrbf_eval, libmrbf), Int32,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                  hctx, mod.handle, m, X, values ? pointer(V) : C_NULL, jac ? pointer(J) : C_NULL, C_NULL)
        end
    end
    _check(mod.ctx, rc)
    return V, J
end

"""
`_mrbf_eval` for a batch of (model, site block) pairs -- m(x) and m(x₊) of every start (algorithm.jl:766-767), the container sweeps of
every start (SurrogateContainer.jl:234-269) -- in one device call (`mrbf_eval_batch`) where the decision table takes the job count
(`mrbf_dispatch_eval_batch`) and it reaches `mrbf_dispatch_eval_batch_min_jobs`; otherwise, or when the library refuses the call
(rc -2), the loop of `mrbf_eval`.  `Xs[i]` is d x m_i, one site per column; the models share one context.  Returns a vector of
`(V, J)`, for every pair bit for bit what `_mrbf_eval(mods[i], Xs[i]; values, jac)` returns.
"""
function hip_eval_models_many(mods::AbstractVector{HipRbfModel}, Xs::AbstractVector{Matrix{Float64}}; values::Bool = true, jac::Bool = false,
                              min_jobs::Union{Nothing,Int} = nothing)
    nj = length(mods)
    loop() = [_mrbf_eval(mods[i], Xs[i]; values = values, jac = jac) for i in 1:nj]
    nj == 0 && return loop()
    ctx = mods[1].ctx
    pays = min_jobs === nothing ? _eval_batch_pays(nj) : nj >= min_jobs
    (_dispatch_eval_batch(nj) && pays && all(m -> m.ctx === ctx, mods)) || return loop()
    Vs = [values ? Matrix{Float64}(undef, mods[i].num_outputs, size(Xs[i], 2)) : nothing for i in 1:nj]
    Js = [jac ? Array{Float64,3}(undef, mods[i].num_outputs, mods[i].n_vars, size(Xs[i], 2)) : nothing for i in 1:nj]
    jobs = Vector{MrbfEvalJob}(undef, nj)
    ms = Ref{Float32}(0)
    rc = GC.@preserve Xs Vs Js jobs begin
        for i in 1:nj
            jobs[i] = MrbfEvalJob(mods[i].handle, size(Xs[i], 2), pointer(Xs[i]), values ? pointer(Vs[i]) : C_NULL, jac ? pointer(Js[i]) : C_NULL, 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_eval_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Ptr{MrbfEvalJob}, Ref{Float32}), hctx, nj, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(20, rc) && return loop()           # the library refuses the batch: the single call per pair
    _check(ctx, rc)
    return [(Vs[i], Js[i]) for i in 1:nj]
end

"Evaluate `mod` at scaled site `x̂` (RbfModel.jl:783-785)."
eval_models(mod::HipRbfModel, scal::AbstractVarScaler, x̂::Vec) = vec(_mrbf_eval(mod, reshape(Vector{Float64}(x̂), :, 1))[1])
"Evaluate output(s) `ℓ` (RbfModel.jl:788-790; RefSurrogate passes index vectors)."
eval_models(mod::HipRbfModel, scal::AbstractVarScaler, x̂::Vec, ℓ) = eval_models(mod, scal, x̂)[ℓ]
"k x d Jacobian (or rows) at `x̂` (RbfModel.jl:797-800)."
function get_jacobian(mod::HipRbfModel, scal::AbstractVarScaler, x̂::Vec, rows = nothing)
    J = _mrbf_eval(mod, reshape(Vector{Float64}(x̂), :, 1); values = false, jac = true)[2][:, :, 1]
    return isnothing(rows) ? J : J[rows, :]
end
"Gradient of output `ℓ` (RbfModel.jl:792-795): the Jacobian row, bit for bit (test/rbf_models.jl:105-109)."
get_gradient(mod::HipRbfModel, scal::AbstractVarScaler, x̂::Vec, ℓ) = vec(get_jacobian(mod, scal, x̂, ℓ))

"""
Model Hessians at the columns of `X` (d x m, one scaled site per column) in one device call (`mrbf_eval_hessian`): a d x d x r x m
array, `H[:, :, j, p]` the second derivative of output `rows[j]` with respect to the scaled site at site p (`rows`: 1-based output
indices, any order, repeats allowed; `nothing`: all outputs).  Both triangles are written with the same bits, so the row-major
blocks of the library read the same in column-major order.  The reference has no method for this (RbfModel.jl:792-800 stops at
gradients and Jacobians).  `with_info = true` returns `(H, info)` with the call's `MrbfHessInfo` (time, split count, chunks).
"""
function hip_get_hessians_at_sites(mod::HipRbfModel, scal, X::Matrix{Float64}, rows = nothing; with_info::Bool = false)
    d, m = mod.n_vars, size(X, 2)
    rows0 = isnothing(rows) ? Int32[] : Int32[Int32(ℓ - 1) for ℓ in rows]
    r = isnothing(rows) ? mod.num_outputs : length(rows0)
    H = Array{Float64,4}(undef, d, d, r, m)
    info = Ref(MrbfHessInfo(0.0f0, 0, 0, 0))
    (m == 0 || r == 0) && return with_info ? (H, info[]) : H
    rc = GC.@preserve X rows0 H begin
        _locked(mod.ctx) do hctx
            ccall((:mrbf_eval_hessian, libmrbf), Int32,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float64}, Ref{MrbfHessInfo}),
                  hctx, mod.handle, m, X, length(rows0), isempty(rows0) ? C_NULL : pointer(rows0), H, info)
        end
    end
    _check(mod.ctx, rc)
    return with_info ? (H, info[]) : H
end
"d x d Hessian of output `ℓ` at `x̂` with respect to the scaled site: the derivative of `get_gradient(mod, scal, x̂, ℓ)`."
hip_get_hessian(mod::HipRbfModel, scal, x̂::Vec, ℓ::Integer) =
    hip_get_hessians_at_sites(mod, scal, reshape(Vector{Float64}(x̂), :, 1), [ℓ])[:, :, 1, 1]

"""
`hip_get_hessians_at_sites` for a batch of (model, site block) pairs -- the second derivative of every start's model at its own
iterate -- in one device call (`mrbf_eval_hessian_batch`) where the decision table takes the job count
(`mrbf_dispatch_hessian_batch`) and it reaches `mrbf_dispatch_hessian_batch_min_jobs`; otherwise, or when the library refuses the
call (rc -2), the loop of `mrbf_eval_hessian`.  `Xs[i]` is d x m_i, one site per column; `rows`: `nothing` (all outputs), one vector
of 1-based output indices for all pairs, or one entry (a vector or `nothing`) per pair; the models share one context.  Returns a
vector of d x d x r x m_i arrays, for every pair bit for bit what `hip_get_hessians_at_sites(mods[i], scal, Xs[i], rows)` returns.
"""
function hip_get_hessians_many(mods::AbstractVector{HipRbfModel}, Xs::AbstractVector{Matrix{Float64}}, rows = nothing;
                               min_jobs::Union{Nothing,Int} = nothing)
    nj = length(mods)
    one_for_all = isnothing(rows) || isempty(rows) || first(rows) isa Integer
    rows_of(i) = one_for_all ? rows : rows[i]
    loop() = [hip_get_hessians_at_sites(mods[i], nothing, Xs[i], rows_of(i)) for i in 1:nj]
    nj == 0 && return loop()
    ctx = mods[1].ctx
    pays = min_jobs === nothing ? _hessian_batch_pays(nj) : nj >= min_jobs
    (_dispatch_hessian_batch(nj) && pays && all(m -> m.ctx === ctx, mods)) || return loop()
    rows0 = [isnothing(rows_of(i)) ? Int32[] : Int32[Int32(ℓ - 1) for ℓ in rows_of(i)] for i in 1:nj]
    rs = [isnothing(rows_of(i)) ? Int(mods[i].num_outputs) : length(rows0[i]) for i in 1:nj]
    Hs = [Array{Float64,4}(undef, mods[i].n_vars, mods[i].n_vars, rs[i], size(Xs[i], 2)) for i in 1:nj]
    jobs = Vector{MrbfHessJob}(undef, nj)
    info = Ref(MrbfHessBatchInfo(0.0f0, 0, 0, 0))
    rc = GC.@preserve Xs rows0 Hs jobs begin
        for i in 1:nj
            m = rs[i] == 0 ? 0 : size(Xs[i], 2)          # an empty selection is not "all": nothing to ask the library for
            jobs[i] = MrbfHessJob(mods[i].handle, m, m == 0 ? C_NULL : pointer(Xs[i]), isempty(rows0[i]) ? C_NULL : pointer(rows0[i]),
                                  m == 0 ? C_NULL : pointer(Hs[i]), length(rows0[i]), 0, 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_eval_hessian_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Ptr{MrbfHessJob}, Ref{MrbfHessBatchInfo}), hctx, nj, jobs, info)
        end
    end
    rc != 0 && _fallback_rc(21, rc) && return loop()           # the library refuses the batch: the single call per pair
    _check(ctx, rc)
    return Hs
end

# batched twins (m sites as the columns of X): one device sweep for all k outputs of all sites
eval_models_at_sites(mod::HipRbfModel, scal, X::AbstractMatrix) = _mrbf_eval(mod, Matrix{Float64}(X))[1]
get_jacobians_at_sites(mod::HipRbfModel, scal, X::AbstractMatrix) = _mrbf_eval(mod, Matrix{Float64}(X); values = false, jac = true)[2]

# ---- container twins: eval_container_{objectives,nl_eq_constraints,nl_ineq_constraints}[_jacobian]_at_scaled_sites ------------
# (SurrogateContainer.jl:234-269 does one inner-model call per function index; here every distinct grouped HipRbfModel is swept
#  ONCE for all sites, RefSurrogates select rows, CompositeSurrogates apply their outer function / chain rule per site,
#  AbstractSurrogateInterface.jl:136-154, :175-229.)  Sites are the columns of X_scaled (d x m).
_inner(s::RefSurrogate) = s.model_ref[]
_inner(s::CompositeSurrogate) = s.model_ref[]
_inner(s) = s
# the container keeps dictionaries function index => surrogate (SurrogateContainer.jl:111-113); order = key order, as in :248-267
_container_surrogates(sc::SurrogateContainer, ::Val{:objectives}) = [get_surrogates(sc, ind) for ind in get_objective_indices(sc)]
_container_surrogates(sc::SurrogateContainer, ::Val{:nl_eq_constraints}) = [get_surrogates(sc, ind) for ind in get_nl_eq_constraint_indices(sc)]
_container_surrogates(sc::SurrogateContainer, ::Val{:nl_ineq_constraints}) = [get_surrogates(sc, ind) for ind in get_nl_ineq_constraint_indices(sc)]
function _sweep_groups(surrogates, scal, X::Matrix{Float64}; jac::Bool)
    cache = IdDict{Any,Any}()
    for s in surrogates
        m = _inner(s)
        haskey(cache, m) && continue
        cache[m] = m isa HipRbfModel ? _mrbf_eval(m, X; values = true, jac = jac) : nothing
    end
    return cache
end
function _container_values_at_sites(surrogates, scal, X_scaled::AbstractMatrix)
    X = Matrix{Float64}(X_scaled)
    m = size(X, 2)
    isempty(surrogates) && return Matrix{MIN_PRECISION}(undef, 0, m)          # SurrogateContainer.jl:265
    cache = _sweep_groups(surrogates, scal, X; jac = false)
    rows = map(surrogates) do s
        sweep = cache[_inner(s)]
        if sweep === nothing                                                  # some other surrogate family: site by site
            reduce(hcat, [_eval_models_vec(s, scal, X[:, p]) for p = 1:m])
        elseif s isa RefSurrogate
            sweep[1][s.output_indices, :]
        else                                                                  # CompositeSurrogate: φ([T(x); g(x)]) per site
            reduce(hcat, [eval_vfun(s.outer_ref[], [untransform(X[:, p], scal); sweep[1][s.inner_output_indices, p]]) for p = 1:m])
        end
    end
    return reduce(vcat, rows)                                                 # Σk x m
end
function _container_jacobians_at_sites(surrogates, scal, X_scaled::AbstractMatrix)
    X = Matrix{Float64}(X_scaled)
    d, m = size(X)
    isempty(surrogates) && return Array{MIN_PRECISION,3}(undef, 0, d, m)      # SurrogateContainer.jl:259
    cache = _sweep_groups(surrogates, scal, X; jac = true)
    blocks = map(surrogates) do s
        sweep = cache[_inner(s)]
        if sweep === nothing
            cat([get_jacobian(s, scal, X[:, p]) for p = 1:m]...; dims = 3)
        elseif s isa RefSurrogate
            sweep[2][s.output_indices, :, :]
        else
            cat([begin
                     gx = [untransform(X[:, p], scal); sweep[1][s.inner_output_indices, p]]
                     _composite_jac(_get_jacobian(s.outer_ref[], gx), sweep[2][s.inner_output_indices, :, p], scal, X[:, p])
                 end for p = 1:m]...; dims = 3)
        end
    end
    return reduce(vcat, blocks)                                               # Σk x d x m
end
for plural in (:objectives, :nl_eq_constraints, :nl_ineq_constraints)
    vals = Symbol("eval_container_", plural, "_at_scaled_sites")
    jacs = Symbol("eval_container_", plural, "_jacobian_at_scaled_sites")
    @eval begin
        $vals(sc::SurrogateContainer, scal, X::AbstractMatrix) = _container_values_at_sites(_container_surrogates(sc, Val($(QuoteNode(plural)))), scal, X)
        $jacs(sc::SurrogateContainer, scal, X::AbstractMatrix) = _container_jacobians_at_sites(_container_surrogates(sc, Val($(QuoteNode(plural)))), scal, X)
    end
end

"Does the container hold a `HipRbfModel` at all?  Pure Julia: asked before anything of libmrbf is touched (inertness for non-users)."
function _touches_device(sc::SurrogateContainer; objectives_only::Bool = false)
    kinds = objectives_only ? (Val(:objectives),) : (Val(:objectives), Val(:nl_eq_constraints), Val(:nl_ineq_constraints))
    for kind in kinds
        for s in _container_surrogates(sc, kind)
            _inner(s) isa HipRbfModel && return true
        end
    end
    return false
end

# What the device entry points need to know about a container: its distinct grouped HipRbfModels, the role of every output row
# (objective position l >= 0, MRBF_ROLE_EQ = -2, MRBF_ROLE_INEQ = -3, MRBF_ROLE_NONE = -1) and how many surrogates are "foreign"
# (CompositeSurrogates, other model families, or a model row used twice): with a foreign one the reference methods run.
function _container_plan(sc::SurrogateContainer; objectives_only::Bool = false)
    models = HipRbfModel[]; roles = Vector{Vector{Int32}}()
    k = 0; n_con = 0; n_foreign = 0
    function slot(m)
        i = findfirst(x -> x === m, models)
        i === nothing || return i
        push!(models, m); push!(roles, fill(Int32(-1), num_outputs(m)))
        return length(models)
    end
    for (kind, role) in ((Val(:objectives), 0), (Val(:nl_eq_constraints), -2), (Val(:nl_ineq_constraints), -3))
        objectives_only && role != 0 && continue                              # _backtrack only evaluates the objectives (descent.jl:161-179)
        for s in _container_surrogates(sc, kind)
            # a bare HipRbfModel in a container list contributes all its rows in order (as surrogates.py container_plan does)
            inner = s isa RefSurrogate ? _inner(s) : s
            if !(s isa CompositeSurrogate) && inner isa HipRbfModel
                i = slot(inner)
                for oi in (s isa RefSurrogate ? s.output_indices : 1:num_outputs(inner))
                    roles[i][oi] == -1 || (n_foreign += 1)                    # one row in two roles: not expressible
                    roles[i][oi] = role == 0 ? Int32(k) : Int32(role)
                    role == 0 ? (k += 1) : (n_con += 1)
                end
            else
                n_foreign += 1
                role == 0 ? (k += num_outputs(s)) : (n_con += num_outputs(s))
            end
        end
    end
    in_order = length(models) == 1 && n_con == 0 && roles[1] == Int32.(0:num_outputs(models[1])-1)
    return (; models, roles = isempty(roles) ? Int32[] : reduce(vcat, roles), k, n_con, n_foreign, in_order)
end

# ---- descent consumers ------------------------------------------------------------------------------------------------------------
"All Armijo step sizes of `_backtrack` (descent.jl:150-185) in one batch; returns (x₊, mx₊, step) like the reference."
function _backtrack(x::AbstractVector{F}, dir, step_size, ω, sc::SurrogateContainer, cfg, scal) where {F<:AbstractFloat}
    # no HipRbfModel among the objectives (every run that does not use HipRbfConfig): Morbit's own loop, libmrbf is not touched
    _touches_device(sc; objectives_only = true) ||
        return invoke(_backtrack, Tuple{AbstractVector{F},Any,Any,Any,Any,Any,Any}, x, dir, step_size, ω, sc, cfg, scal)
    plan = _container_plan(sc; objectives_only = true)
    if !_dispatch_backtrack(length(plan.models), plan.n_foreign, plan.in_order)
        return invoke(_backtrack, Tuple{AbstractVector{F},Any,Any,Any,Any,Any,Any}, x, dir, step_size, ω, sc, cfg, scal)
    end
    model = plan.models[1]
    x64 = Vector{Float64}(x); dir64 = Vector{Float64}(dir)
    k = model.num_outputs
    x₊, mx₊, step, loops = similar(x64), Vector{Float64}(undef, k), similar(x64), Ref{Int32}(0)
    rc = GC.@preserve x64 dir64 x₊ mx₊ step begin
        _locked(model.ctx) do hctx
            ccall((:mrbf_backtrack, libmrbf), Int32,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Int32, Float64, Float64, Float64, Int32,
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
                  hctx, model.handle, x64, dir64, step_size, ω, cfg.strict_backtracking, cfg.armijo_const_rhs,
                  cfg.armijo_const_shrink, cfg.min_stepsize >= 0 ? cfg.min_stepsize : eps(F), cfg.max_loops,
                  x₊, mx₊, step, loops)
        end
    end
    _check(model.ctx, rc)
    return F.(x₊), F.(mx₊), F.(step)
end

"""
Pascoletti-Serafini descent step (descent.jl:512-581) with the subproblem solver on the device (`mrbf_ps_step_problem`): objectives
and modelled constraints may be spread over several grouped `HipRbfModel`s, the MOP may carry linear constraints.  Whenever the
decision table says so (a `CompositeSurrogate` or another model family in the container, sizes outside the device path) or the
device call asks for it, Morbit's own method runs on the same arguments -- this method never raises because of a size limit.
Same returns as the reference.
"""
function get_criticality(desc_cfg::PascolettiSerafiniConfig, mop, scal, x_it, x_it_n, data_base, sc::SurrogateContainer, algo_config;
                         seed::UInt64 = rand(UInt64))
    reference() = invoke(get_criticality, Tuple{PascolettiSerafiniConfig,Any,Any,Any,Any,Any,Any,Any}, desc_cfg, mop, scal, x_it, x_it_n, data_base, sc, algo_config)
    _touches_device(sc) || return reference()      # no HipRbfModel in the container: Morbit's own method, libmrbf is not touched
    plan = _container_plan(sc)
    x = Vector{Float64}(get_x_scaled(x_it)); x_n = Vector{Float64}(get_x_scaled(x_it_n)); fx_n = Vector{Float64}(get_fx(x_it_n))
    d, k = length(x_n), plan.k
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_ps(d, k, length(plan.models), plan.n_con, length(b_eq) + length(b_in), plan.n_foreign) || return reference()
    lb_eff, ub_eff = local_bounds(scal, x, get_delta(x_it))
    lb = Vector{Float64}(lb_eff); ub = Vector{Float64}(ub_eff)
    r = _get_global_dir(desc_cfg, fx_n)                                        # descent.jl:360-368
    rbuf = r === nothing ? nothing : Vector{Float64}(r)
    g_evals, l_evals = _ps_max_evals(desc_cfg, d)                              # descent.jl:414-432
    opts = Ref(MrbfPsOptions(desc_cfg.max_ideal_point_problem_evals, g_evals, l_evals, 0, seed, -0.5, 1e-3))
    info = Ref{MrbfPsInfo}()
    x_trial, mx_trial = Vector{Float64}(undef, d), Vector{Float64}(undef, k)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    roles = plan.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    ctx = plan.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin x_n lb ub fx_n rbuf x_trial mx_trial begin
        prob = Ref(MrbfPsProblem(length(handles), k, pointer(handles), pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ps_step_problem, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfPsOptions},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfPsInfo}),
                  hctx, prob, x_n, lb, ub, fx_n, rbuf === nothing ? C_NULL : pointer(rbuf), opts, x_trial, mx_trial, C_NULL, info)
        end
    end
    rc != 0 && _fallback_rc(3, rc) && return reference()
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_n))
    info[].status == 1 && return 0, copy(get_x_scaled(x_it_n)), mx_trial, 0    # critical: some r_l <= 0 (descent.jl:546-549)
    info[].status == 2 && return 0, copy(get_x_scaled(x_it)), mx_trial, 0      # failure (descent.jl:571-572)
    return Xet(abs(info[].tau)), (Xet.(x_trial), mx_trial, norm(x .- x_trial, Inf))
end

"""
Many starts in one device call (`mrbf_ps_step_batch`): `get_criticality(::PascolettiSerafiniConfig, ...)` (descent.jl:512-581) for
independent starts of one problem -- the `Threads.@threads` loop over starts of examples/large_scale_benchmarks.jl:102-109 with
`descent_method = :ps`.  `x_its[p]`, `x_it_ns[p]` and `scs[p]` are start p's iterate, normal-step iterate and surrogate container,
`seeds[p]` keys its generator; `mop`, `scal` and the configurations belong to the one problem.  For every start the result is, bit for
bit, what `get_criticality` returns on that start alone with `seed = seeds[p]`.  Where the containers do not share one plan shape, the
decision table refuses (`mrbf_dispatch_ps_batch`: a foreign surrogate, d > 256, more than 65535 starts, the limits of the single
call) or the batch does not pay (`_ps_batch_pays`), every start takes the single-start method.  Returns a vector of that method's results.
"""
function hip_ps_criticality_many(desc_cfg::PascolettiSerafiniConfig, mop, scal, x_its::AbstractVector, x_it_ns::AbstractVector, data_base,
                                 scs::AbstractVector{<:SurrogateContainer}, algo_config;
                                 seeds::AbstractVector{UInt64} = rand(UInt64, length(scs)))
    single(p) = get_criticality(desc_cfg, mop, scal, x_its[p], x_it_ns[p], data_base, scs[p], algo_config; seed = seeds[p])
    loop() = [single(p) for p in eachindex(scs)]
    ns = length(scs)
    (_ps_batch_pays(ns) && all(_touches_device, scs)) || return loop()
    plans = [_container_plan(sc) for sc in scs]
    p1 = plans[1]
    same = all(pl -> pl.roles == p1.roles && pl.k == p1.k && pl.n_con == p1.n_con && pl.n_foreign == p1.n_foreign &&
                     length(pl.models) == length(p1.models) &&
                     all(num_outputs(a) == num_outputs(b) for (a, b) in zip(pl.models, p1.models)), plans)
    same || return loop()
    d, k, nm = length(get_x_scaled(x_it_ns[1])), p1.k, length(p1.models)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_ps_batch(ns, d, k, nm, p1.n_con, length(b_eq) + length(b_in), p1.n_foreign) || return loop()
    X_n = Matrix{Float64}(undef, d, ns); LB = Matrix{Float64}(undef, d, ns); UB = Matrix{Float64}(undef, d, ns)   # column p = start p
    FX_n = Matrix{Float64}(undef, k, ns)
    for p in 1:ns
        X_n[:, p] .= get_x_scaled(x_it_ns[p]); FX_n[:, p] .= get_fx(x_it_ns[p])
        lb_eff, ub_eff = local_bounds(scal, Vector{Float64}(get_x_scaled(x_its[p])), get_delta(x_its[p]))
        LB[:, p] .= lb_eff; UB[:, p] .= ub_eff
    end
    rs = [_get_global_dir(desc_cfg, FX_n[:, p]) for p in 1:ns]                 # descent.jl:360-368
    R = rs[1] === nothing ? nothing : Matrix{Float64}(hcat(rs...))
    g_evals, l_evals = _ps_max_evals(desc_cfg, d)                              # descent.jl:414-432
    opts = Ref(MrbfPsOptions(desc_cfg.max_ideal_point_problem_evals, g_evals, l_evals, 0, UInt64(0), -0.5, 1e-3))
    infos = Vector{MrbfPsInfo}(undef, ns)
    X_t = Matrix{Float64}(undef, d, ns); MX_t = Matrix{Float64}(undef, k, ns)
    ms = Ref{Float32}(0)
    seedv = Vector{UInt64}(seeds)
    handles = Ptr{Cvoid}[m.handle for pl in plans for m in pl.models]          # start-major
    roles = p1.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    ctx = p1.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin X_n LB UB FX_n R seedv X_t MX_t infos begin
        prob = Ref(MrbfPsProblem(nm, k, C_NULL, pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ps_step_batch, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Ref{MrbfPsProblem}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ref{MrbfPsOptions}, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{MrbfPsInfo},
                   Ref{Float32}),
                  hctx, ns, prob, handles, X_n, LB, UB, FX_n, R === nothing ? C_NULL : pointer(R), opts, seedv, X_t, MX_t, C_NULL, infos, ms)
        end
    end
    rc != 0 && _fallback_rc(14, rc) && return loop()           # a shape outside the device path: the single-start method
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_ns[1]))
    return map(1:ns) do p
        info = infos[p]
        info.status == 1 && return 0, copy(get_x_scaled(x_it_ns[p])), MX_t[:, p], 0    # critical: some r_l <= 0 (descent.jl:546-549)
        info.status == 2 && return 0, copy(get_x_scaled(x_its[p])), MX_t[:, p], 0      # failure (descent.jl:571-572)
        x_trial = X_t[:, p]
        (Xet(abs(info.tau)), (Xet.(x_trial), MX_t[:, p], norm(Vector{Float64}(get_x_scaled(x_its[p])) .- x_trial, Inf)))
    end
end

"""
Steepest-descent criticality (descent.jl:187-241) on the device (`mrbf_sd_criticality`): objective Jacobians at x_n, modelled
constraint Jacobians at x and values at x_n by the evaluation kernels, the linearised right-hand sides of descent.jl:196-229, then the
direction LP of `_steepest_descent_direction` (descent.jl:91-135) solved exactly (dual simplex) instead of by JuMP + OSQP.  Whenever
the decision table says so (a `CompositeSurrogate` or another model family, more than 64 LP rows, d > 4096) or the LP gave up, Morbit's
own method runs on the same arguments.  Returns (ω, d) in the iterate's float type.  `compute_descent_step` stays Morbit's method:
its `_backtrack` reaches the device through the method above.
"""
function get_criticality(desc_cfg::SteepestDescentConfig, mop, scal, x_it, x_it_n, data_base, sc::SurrogateContainer, algo_config)
    reference() = invoke(get_criticality, Tuple{SteepestDescentConfig,Any,Any,Any,Any,Any,Any,Any}, desc_cfg, mop, scal, x_it, x_it_n, data_base, sc, algo_config)
    _touches_device(sc) || return reference()      # no HipRbfModel in the container: Morbit's own method, libmrbf is not touched
    plan = _container_plan(sc)
    x = Vector{Float64}(get_x_scaled(x_it)); x_n = Vector{Float64}(get_x_scaled(x_it_n))
    d, k = length(x_n), plan.k
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_sd(d, k, length(plan.models), plan.n_con, length(b_eq) + length(b_in), plan.n_foreign) || return reference()
    lb_g, ub_g = full_bounds_internal(scal)                                    # the global bounds, not the trust region (descent.jl:202)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    info = Ref{MrbfSdInfo}()
    dir = Vector{Float64}(undef, d)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    roles = plan.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    ctx = plan.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin x x_n lb ub dir begin
        prob = Ref(MrbfPsProblem(length(handles), k, pointer(handles), pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_sd_criticality, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64},
                   Ptr{Float64}, Ref{MrbfSdInfo}),
                  hctx, prob, x, x_n, lb, ub, desc_cfg.normalize, dir, C_NULL, info)
        end
    end
    rc != 0 && _fallback_rc(6, rc) && return reference()       # the LP gave up: Morbit's JuMP model on the same arguments
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_n))
    return Xet(info[].omega), Xet.(dir)                        # NO_OBJECTIVE / INFEASIBLE: zeros and -Inf, as descent.jl:130-133
end

"""
Directed search (descent.jl:583-664, parked in the reference behind "TODO Re-enable Directed Search").  The fields that choose the image
direction are those of `PascolettiSerafiniConfig` (descent.jl:324-350), the backtracking fields those of `SteepestDescentConfig`
(descent.jl:55-66): `hip_get_criticality_ds` gives (ω, d), `hip_compute_descent_step` -- typed on `SteepestDescentConfig`, which
`_ds_step_config` makes of this one -- does the step.
"""
struct HipDirectedSearchConfig <: AbstractDescentConfig
    reference_point::Vector{Float64}
    reference_direction::Vector{Float64}
    max_ideal_point_problem_evals::Int
    reference_algo::Symbol
    strict_backtracking::Bool
    armijo_const_rhs::Float64
    armijo_const_shrink::Float64
    min_stepsize::Float64
    max_loops::Int
    normalize::Bool
    constraint_rows::Symbol      # :host (the parked body's JuMP model) or :device (mrbf_ds_criticality_rows) for a problem with rows
    ideal_point::Symbol          # :host (compute_local_ideal_point, NLopt) or :device (mrbf_ideal_point_problem / _batch) for the default r
    function HipDirectedSearchConfig(; reference_point = Float64[], reference_direction = Float64[], max_ideal_point_problem_evals = -1,
                                     reference_algo = :GN_ISRES, strict_backtracking = true, armijo_const_rhs = 1e-6,
                                     armijo_const_shrink = 0.75, min_stepsize = 10 * eps(Float64),
                                     max_loops = floor(Int, log(min_stepsize > 0 ? min_stepsize : eps(Float64)) / log(armijo_const_shrink)),
                                     normalize = true, constraint_rows = :host, ideal_point = :host)
        @assert all(reference_direction .> 0) "The components of the `reference_direction` cannot be negative."
        @assert armijo_const_rhs > 0
        @assert constraint_rows in (:host, :device)
        @assert ideal_point in (:host, :device)
        return new(reference_point, reference_direction, max_ideal_point_problem_evals, reference_algo, strict_backtracking,
                   armijo_const_rhs, armijo_const_shrink, min_stepsize, max_loops, normalize, constraint_rows, ideal_point)
    end
end
_ds_step_config(cfg::HipDirectedSearchConfig) =
    SteepestDescentConfig(; strict_backtracking = cfg.strict_backtracking, armijo_const_rhs = cfg.armijo_const_rhs,
                          armijo_const_shrink = cfg.armijo_const_shrink, min_stepsize = cfg.min_stepsize, max_loops = cfg.max_loops,
                          normalize = cfg.normalize)

"""
The local ideal point (descent.jl:404-412) of one start on the device (`mrbf_ideal_point_problem`): the k single-objective minimisations
over [lb_eff, ub_eff] side by side -- the ideal-point phase of the Pascoletti-Serafini step as a call of its own.  `plan` is the
container's plan (`_container_plan`); `lin = (Aeq, beq, Ain, bin)` holds the linear rows in scaled variables, the matrices d × rows
(the rows × d row-major array); `carry_constraints = false` searches the box only: constraint roles read MRBF_ROLE_NONE (-1) and no
linear rows are passed.  Returns (ideal (k), x_ideal (d × k), m(x_n) (k), info), or `nothing` where the decision table refuses
(`mrbf_dispatch_ideal`): take the host search.
"""
function hip_local_ideal_point(plan, x_n::Vector{Float64}, lb_eff::Vector{Float64}, ub_eff::Vector{Float64}; max_evals::Integer = -1,
                               seed::UInt64 = UInt64(0), lin = nothing, carry_constraints::Bool = true)
    d, k, nm = length(x_n), plan.k, length(plan.models)
    carry = carry_constraints
    roles = carry ? plan.roles : Int32[r >= 0 ? r : Int32(-1) for r in plan.roles]
    Aeq, beq, Ain, bin = (carry && lin !== nothing) ? lin : (zeros(0, 0), Float64[], zeros(0, 0), Float64[])
    _dispatch_ideal(d, k, nm, carry ? plan.n_con : 0, length(beq) + length(bin), plan.n_foreign) || return nothing
    opts = Ref(MrbfPsOptions(max_evals, -1, 0, 0, seed, -0.5, 1e-3))
    info = Ref{MrbfIdealInfo}()
    ideal = Vector{Float64}(undef, k); x_ideal = Matrix{Float64}(undef, d, k); mx = Vector{Float64}(undef, k)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    ctx = plan.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin x_n lb_eff ub_eff ideal x_ideal mx begin
        prob = Ref(MrbfPsProblem(nm, k, pointer(handles), pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ideal_point_problem, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfPsOptions}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ref{MrbfIdealInfo}),
                  hctx, prob, x_n, lb_eff, ub_eff, opts, ideal, x_ideal, mx, info)
        end
    end
    rc != 0 && _fallback_rc(25, rc) && return nothing          # a shape outside the device path: the host search
    _check(ctx, rc)
    return ideal, x_ideal, mx, info[]
end

"""
The local ideal points of many starts in one device call (`mrbf_ideal_point_batch`): `plans[p]` is start p's container plan, column p
of `X_n`, `LB`, `UB` (d × n_starts) its start point and box, `seeds[p]` keys its generator.  For every start the outputs are, bit for
bit, what `hip_local_ideal_point` returns on that start alone.  Below `IDEAL_BATCH_MIN_STARTS` starts, or where only the single call's
row of the decision table admits the shape, the loop of single calls runs.  Returns (ideal (k × n_starts), x_ideal (d × k × n_starts),
m(x_n) (k × n_starts), infos), or `nothing` where the plans do not share one shape or the table refuses a start: take the host search.
"""
function hip_local_ideal_points_many(plans::AbstractVector, X_n::Matrix{Float64}, LB::Matrix{Float64}, UB::Matrix{Float64};
                                     max_evals::Integer = -1, seeds::AbstractVector{UInt64} = zeros(UInt64, length(plans)), lin = nothing,
                                     carry_constraints::Bool = true)
    ns = length(plans)
    ns >= 1 || return nothing
    p1 = plans[1]
    d, k, nm = size(X_n, 1), p1.k, length(p1.models)
    function loop()
        ideal = Matrix{Float64}(undef, k, ns); x_ideal = Array{Float64,3}(undef, d, k, ns); mx = Matrix{Float64}(undef, k, ns)
        infos = Vector{MrbfIdealInfo}(undef, ns)
        for p in 1:ns
            one = hip_local_ideal_point(plans[p], X_n[:, p], LB[:, p], UB[:, p]; max_evals = max_evals, seed = seeds[p], lin = lin,
                                        carry_constraints = carry_constraints)
            one === nothing && return nothing
            ideal[:, p] .= one[1]; x_ideal[:, :, p] .= one[2]; mx[:, p] .= one[3]; infos[p] = one[4]
        end
        return ideal, x_ideal, mx, infos
    end
    same = all(pl -> pl.roles == p1.roles && pl.k == p1.k && pl.n_con == p1.n_con && pl.n_foreign == p1.n_foreign &&
                     length(pl.models) == length(p1.models) &&
                     all(num_outputs(a) == num_outputs(b) for (a, b) in zip(pl.models, p1.models)), plans)
    same || return nothing
    carry = carry_constraints
    roles = carry ? p1.roles : Int32[r >= 0 ? r : Int32(-1) for r in p1.roles]
    Aeq, beq, Ain, bin = (carry && lin !== nothing) ? lin : (zeros(0, 0), Float64[], zeros(0, 0), Float64[])
    (ns >= IDEAL_BATCH_MIN_STARTS &&
     _dispatch_ideal_batch(ns, d, k, nm, carry ? p1.n_con : 0, length(beq) + length(bin), p1.n_foreign)) || return loop()
    opts = Ref(MrbfPsOptions(max_evals, -1, 0, 0, UInt64(0), -0.5, 1e-3))
    infos = Vector{MrbfIdealInfo}(undef, ns)
    ideal = Matrix{Float64}(undef, k, ns); x_ideal = Array{Float64,3}(undef, d, k, ns); mx = Matrix{Float64}(undef, k, ns)
    ms = Ref{Float32}(0)
    seedv = Vector{UInt64}(seeds)
    handles = Ptr{Cvoid}[m.handle for pl in plans for m in pl.models]          # start-major
    ctx = p1.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin X_n LB UB seedv ideal x_ideal mx infos begin
        prob = Ref(MrbfPsProblem(nm, k, C_NULL, pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ideal_point_batch, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Ref{MrbfPsProblem}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfPsOptions},
                   Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{MrbfIdealInfo}, Ref{Float32}),
                  hctx, ns, prob, handles, X_n, LB, UB, opts, seedv, ideal, x_ideal, mx, infos, ms)
        end
    end
    rc != 0 && _fallback_rc(26, rc) && return loop()           # a shape outside the batch's path: the single call per start
    _check(ctx, rc)
    return ideal, x_ideal, mx, infos
end

# r of descent.jl:599-611, the target change of the model values: minus the reference direction, or the reference point minus f(x_n),
# or the local ideal point (descent.jl:404-412) minus f(x_n) -- the host search's, or with `ideal_point = :device` the device call's
# (the runs carry the modelled and the linear constraints, as the host search's handles do; `seed` keys its generator), the host
# search where the decision table refuses
function _ideal_lin(scal, mop)      # the MOP's linear rows in scaled variables, the matrices d x rows (the rows x d row-major array)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    return (Matrix{Float64}(transpose(Matrix(A_eq))), Vector{Float64}(b_eq), Matrix{Float64}(transpose(Matrix(A_in))), Vector{Float64}(b_in))
end
function _ds_image_direction(cfg::HipDirectedSearchConfig, mop, scal, x_it, x_it_n, sc; seed::UInt64 = UInt64(0))
    fx_n = Vector{Float64}(get_fx(x_it_n))
    isempty(cfg.reference_direction) || return -Vector{Float64}(cfg.reference_direction)
    isempty(cfg.reference_point) || return Vector{Float64}(cfg.reference_point) .- fx_n
    n_vars = length(get_x_scaled(x_it_n))
    if cfg.ideal_point == :device && _touches_device(sc)
        lb_d, ub_d = local_bounds(scal, Vector{Float64}(get_x_scaled(x_it)), get_delta(x_it))
        one = hip_local_ideal_point(_container_plan(sc), Vector{Float64}(get_x_scaled(x_it_n)), Vector{Float64}(lb_d), Vector{Float64}(ub_d);
                                    max_evals = cfg.max_ideal_point_problem_evals, seed = seed, lin = _ideal_lin(scal, mop))
        one === nothing || return one[1] .- fx_n
    end
    max_evals = cfg.max_ideal_point_problem_evals < 0 ? 500 * (n_vars + 1) : cfg.max_ideal_point_problem_evals
    objf_handles, eq_handles, ineq_handles = get_raw_optim_handles(mop, sc, scal)
    lb_eff, ub_eff = local_bounds(scal, get_x_scaled(x_it), get_delta(x_it))
    return compute_local_ideal_point(x_it_n, lb_eff, ub_eff, objf_handles, eq_handles, ineq_handles, max_evals, cfg.reference_algo) .- fx_n
end

# the parked body's own route (descent.jl:619-643): the pseudo-inverse without constraints, else its JuMP model, extended by the rows of
# get_criticality(::SteepestDescentConfig, ...) where there are any -- the host method of this binding
function _ds_reference_direction(mop, scal, x_it, x_it_n, sc, r)
    x = get_x_scaled(x_it); x_n = get_x_scaled(x_it_n)
    n_vars = length(x_n)
    lb, ub = full_bounds_internal(scal)
    Dm = eval_container_objectives_jacobian_at_scaled_site(sc, scal, x_n)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    dir_prob = JuMP.Model(LP_OPTIMIZER)
    JuMP.set_silent(dir_prob)
    JuMP.@variable(dir_prob, d[1:n_vars])
    JuMP.@objective(dir_prob, Min, sum((Dm * d .- r) .^ 2))
    JuMP.@constraint(dir_prob, -1.0 .<= d .<= 1.0)
    JuMP.@constraint(dir_prob, Dm * d .<= 0)
    JuMP.@constraint(dir_prob, lb .<= x_n .+ d .<= ub)
    isempty(b_eq) || JuMP.@constraint(dir_prob, A_eq * (x_n .+ d) .== b_eq)
    isempty(b_in) || JuMP.@constraint(dir_prob, A_in * (x_n .+ d) .<= b_in)
    if num_nl_eq_constraints(mop) > 0
        Dc = eval_container_nl_eq_constraints_jacobian_at_scaled_site(sc, scal, x)
        JuMP.@constraint(dir_prob, eval_container_nl_eq_constraints_at_scaled_site(sc, scal, x_n) .+ Dc * (x_n .- x .+ d) .== 0)
    end
    if num_nl_ineq_constraints(mop) > 0
        Dc = eval_container_nl_ineq_constraints_jacobian_at_scaled_site(sc, scal, x)
        JuMP.@constraint(dir_prob, eval_container_nl_ineq_constraints_at_scaled_site(sc, scal, x_n) .+ Dc * (x_n .- x .+ d) .<= 0)
    end
    JuMP.optimize!(dir_prob)
    dir = JuMP.value.(d)
    return max(0.0, -maximum(Dm * dir)), dir
end

"""
The criticality of directed search (descent.jl:583-660 up to the backtracking) on the device (`mrbf_ds_criticality`): the image direction
r from the configuration, the objective Jacobians at x_n by the evaluation kernels, then the direction QP min ½‖∇m d − r‖², the box of
the steepest-descent LP, ∇m d ≤ 0 (descent.jl:635-640), solved exactly by an active-set method instead of by JuMP + OSQP.  Whenever the
decision table says so (`mrbf_dispatch_ds`: a `CompositeSurrogate` or another model family, more than 16 objectives, d > 4096, modelled
or linear constraints) or the QP gave up, the parked body's own JuMP model runs on the same arguments.  With
`constraint_rows = :device` a container or problem with constraint rows takes `mrbf_ds_criticality_rows` where `mrbf_dispatch_ds_rows`
agrees (at most 16 rows in all), and the JuMP model where that call answers -2 (the QP gave up, or d = 0 misses a row).  Returns (ω, d / ‖d‖∞) in the
iterate's float type, or (0, zeros) when critical or ‖d‖∞ = 0 (descent.jl:615-617, :647-660); `hip_compute_descent_step(
_ds_step_config(cfg), ..., ω, d)` does the step.
"""
function hip_get_criticality_ds(desc_cfg::HipDirectedSearchConfig, mop, scal, x_it, x_it_n, data_base, sc::SurrogateContainer, algo_config;
                                r = nothing, seed::UInt64 = UInt64(0))
    x_n = Vector{Float64}(get_x_scaled(x_it_n))
    Xet = eltype(get_x_scaled(x_it_n))
    n = length(x_n)
    # (r: an image direction computed beforehand -- hip_ds_iterate_many finds the ideal points of all starts in one call)
    r = Vector{Float64}(r === nothing ? _ds_image_direction(desc_cfg, mop, scal, x_it, x_it_n, sc; seed = seed) : r)
    (any(r .>= 0) || any(isnan, r)) && return Xet(0), zeros(Xet, n)           # descent.jl:615-617
    function result(ω, dir)
        nrm = norm(dir, Inf)
        (nrm > 0 && isfinite(nrm)) || return Xet(0), zeros(Xet, n)
        return Xet(ω), Xet.(dir ./ nrm)
    end
    reference() = result(_ds_reference_direction(mop, scal, x_it, x_it_n, sc, r)...)
    _touches_device(sc) || return reference()      # no HipRbfModel in the container: libmrbf is not touched
    plan = _container_plan(sc)
    k = plan.k
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    n_lin = length(b_eq) + length(b_in)
    lb_g, ub_g = full_bounds_internal(scal)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    info = Ref{MrbfDsInfo}()
    dir = Vector{Float64}(undef, n)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    roles = plan.roles
    ctx = plan.models[1].ctx
    if plan.n_con + n_lin > 0
        # constraint rows: the extended QP on the device where the configuration asks for it and mrbf_dispatch_ds_rows agrees
        (desc_cfg.constraint_rows == :device &&
         _dispatch_ds_rows(n, k, length(plan.models), plan.n_con, n_lin, plan.n_foreign)) || return reference()
        x = Vector{Float64}(get_x_scaled(x_it))
        Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)
        Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
        rc = GC.@preserve handles roles Aeq beq Ain bin x x_n lb ub r dir begin
            prob = Ref(MrbfPsProblem(length(handles), k, pointer(handles), pointer(roles), length(beq), length(bin),
                                     isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                     isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
            _locked(ctx) do hctx
                ccall((:mrbf_ds_criticality_rows, libmrbf), Int32,
                      (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                       Ptr{Float64}, Ref{MrbfDsInfo}),
                      hctx, prob, x, x_n, lb, ub, r, dir, C_NULL, info)
            end
        end
        rc != 0 && _fallback_rc(24, rc) && return reference()  # gave up, or d = 0 is no start: the JuMP model on the same arguments
        _check(ctx, rc)
        info[].status == 0 || return Xet(0), zeros(Xet, n)
        return result(info[].omega, dir)
    end
    _dispatch_ds(n, k, length(plan.models), plan.n_con, n_lin, plan.n_foreign) || return reference()
    rc = GC.@preserve handles roles x_n lb ub r dir begin
        prob = Ref(MrbfPsProblem(length(handles), k, pointer(handles), pointer(roles), 0, 0, C_NULL, C_NULL, C_NULL, C_NULL, -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ds_criticality, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ref{MrbfDsInfo}),
                  hctx, prob, x_n, lb, ub, r, dir, C_NULL, info)
        end
    end
    rc != 0 && _fallback_rc(22, rc) && return reference()      # the QP gave up: the JuMP model on the same arguments
    _check(ctx, rc)
    info[].status == 0 || return Xet(0), zeros(Xet, n)         # CRITICAL / INFEASIBLE: no direction
    return result(info[].omega, dir)
end

"""
The direction QPs of many starts in one device call (`mrbf_ds_direction`): `Gs[p]` (k × d) is start p's objective Jacobian at
`X_n[:, p]`, `R[:, p]` its image direction; `lb` / `ub` the global bounds in scaled variables.  Returns (D (d × n), Z (k × n), ω (n),
status (n)): for every start what `mrbf_ds_criticality` computes on that start alone, unnormalised; status 3 (gave up): take
`hip_get_criticality_ds` for that start.
"""
function hip_ds_directions_many(ctx::MrbfContext, Gs::AbstractVector{<:AbstractMatrix}, R::AbstractMatrix, X_n::AbstractMatrix,
                                lb::AbstractVector, ub::AbstractVector)
    ns = length(Gs)
    k, d = size(Gs[1])
    G = Array{Float64}(undef, k, d, ns)                          # per start k x d column-major: mrbf_eval's jac_out layout
    for p in 1:ns
        G[:, :, p] .= Gs[p]
    end
    Rm = Matrix{Float64}(R); Xm = Matrix{Float64}(X_n)
    LB = repeat(Vector{Float64}(lb), 1, ns); UB = repeat(Vector{Float64}(ub), 1, ns)
    D = Matrix{Float64}(undef, d, ns); Z = Matrix{Float64}(undef, k, ns); ω = Vector{Float64}(undef, ns)
    status = Vector{Int32}(undef, ns)
    rc = GC.@preserve G Rm Xm LB UB D Z ω status begin
        _locked(ctx) do hctx
            ccall((:mrbf_ds_direction, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                  hctx, ns, d, k, G, Rm, Xm, LB, UB, D, Z, ω, C_NULL, status, C_NULL)
        end
    end
    _check(ctx, rc)
    return D, Z, ω, status
end

"""
The normal step (descent.jl:691-757) on the device (`mrbf_normal_step`): values and Jacobians of the modelled constraints at x by the
evaluation kernels, the right-hand sides b - A x (linear rows) and -m(x) (modelled rows), then the LP min α, -α <= n <= α,
lb <= x + n <= ub, rows in n, solved exactly (active-set dual simplex) instead of by JuMP + OSQP.  Morbit's `compute_normal_step` is
typed on Morbit's own types, so this is a function of its own with the same arguments and result (n, Δ): `find_normal_step`
(algorithm.jl:421,423) calls it in place of `compute_normal_step` (INTEGRATION.md).  Whenever the decision table says so (a modelled
constraint row on a `CompositeSurrogate` or another model family, no row or more than 64 rows, d > 4096) or the LP gave up,
Morbit's own method runs on the same arguments.
"""
function hip_compute_normal_step(mop, scal, x_it, data_base, sc::SurrogateContainer, algo_config; variable_radius::Bool = false)
    reference() = compute_normal_step(mop, scal, x_it, data_base, sc, algo_config; variable_radius = variable_radius)
    _touches_device(sc) || return reference()      # no HipRbfModel in the container: Morbit's own method, libmrbf is not touched
    plan = _container_plan(sc)
    n_foreign_con = plan.n_foreign - _container_plan(sc; objectives_only = true).n_foreign   # foreign objectives do not matter here
    x = Vector{Float64}(get_x_scaled(x_it))
    d = length(x)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_normal(d, length(plan.models), plan.n_con, length(b_eq) + length(b_in), n_foreign_con) || return reference()
    lb_g, ub_g = full_bounds_internal(scal)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    info = Ref{MrbfNormalInfo}()
    n = Vector{Float64}(undef, d)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    roles = plan.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    Δ = Float64(get_delta(x_it)); κ_Δ = Float64(filter_kappa_delta(algo_config)); Δ_max = Float64(delta_max(algo_config))
    # the table admits linear rows only: the container's HipRbfModels may all sit in foreign surrogates (plan.models empty)
    ctx = isempty(plan.models) ? mrbf_context() : plan.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin x lb ub n begin
        prob = Ref(MrbfPsProblem(length(handles), plan.k, pointer(handles), pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_normal_step, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Int32,
                   Ptr{Float64}, Ptr{Float64}, Ref{MrbfNormalInfo}),
                  hctx, prob, d, x, lb, ub, Δ, κ_Δ, Δ_max, variable_radius, n, C_NULL, info)
        end
    end
    rc != 0 && _fallback_rc(7, rc) && return reference()       # the LP gave up: Morbit's JuMP model on the same arguments
    _check(ctx, rc)
    info[].delta == -Inf && return fill(MIN_PRECISION(NaN64), d), -MIN_PRECISION(Inf)      # infeasible (descent.jl:746-748)
    Xet = eltype(get_x_scaled(x_it))
    return Xet.(n), Xet(info[].delta)                          # n already projected into [lb, ub] (descent.jl:752-754)
end

"""
The steepest-descent step (descent.jl:243-318) on the device (`mrbf_sd_step`): the initial step size σ of descent.jl:251-310 (trust
region and global box, and for Δ > 1 with ‖d‖∞ ≈ 1 the linear rows and the modelled constraints linearised at x), then all
`max_loops + 1` Armijo step sizes of `_backtrack` (descent.jl:150-185) evaluated in one sweep per objective model and the stop of the
reference loop picked on the device -- one call for any container of `HipRbfModel`s (several models, objectives out of order,
objectives grouped with modelled constraints).  Morbit's `compute_descent_step` is typed on Morbit's own types, so this is a function
of its own with the same arguments and result (ω, x₊, mx₊, ‖step‖∞): `iterate!` (algorithm.jl:752) calls it in place of
`compute_descent_step` (INTEGRATION.md).  Whenever the decision table says so (a `CompositeSurrogate` or another model family, more
than 64 objectives or 256 constraint rows, d > 4096, max_loops > 1024) Morbit's own method runs on the same arguments.
"""
function hip_compute_descent_step(desc_cfg::SteepestDescentConfig, mop, scal, x_it, x_it_n, data_base, sc::SurrogateContainer,
                                  algo_config, ω, d)
    reference() = compute_descent_step(desc_cfg, mop, scal, x_it, x_it_n, data_base, sc, algo_config, ω, d)
    _touches_device(sc) || return reference()      # no HipRbfModel in the container: Morbit's own method, libmrbf is not touched
    plan = _container_plan(sc)
    x = Vector{Float64}(get_x_scaled(x_it)); x_n = Vector{Float64}(get_x_scaled(x_it_n)); dir = Vector{Float64}(d)
    n, k = length(x_n), plan.k
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_sd_step(n, k, length(plan.models), plan.n_con, length(b_eq) + length(b_in), plan.n_foreign, desc_cfg.max_loops) ||
        return reference()
    lb_g, ub_g = full_bounds_internal(scal)                                    # descent.jl:253
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    opts = Ref(MrbfSdStepOptions(desc_cfg.strict_backtracking, desc_cfg.max_loops, desc_cfg.armijo_const_rhs, desc_cfg.armijo_const_shrink,
                                 desc_cfg.min_stepsize))
    info = Ref{MrbfSdStepInfo}()
    x₊, mx₊ = Vector{Float64}(undef, n), Vector{Float64}(undef, k)
    handles = Ptr{Cvoid}[m.handle for m in plan.models]
    roles = plan.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    Δ = Float64(get_delta(x_it))
    ctx = plan.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin x x_n lb ub dir x₊ mx₊ begin
        prob = Ref(MrbfPsProblem(length(handles), k, pointer(handles), pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_sd_step, libmrbf), Int32,
                  (Ptr{Cvoid}, Ref{MrbfPsProblem}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64},
                   Ref{MrbfSdStepOptions}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfSdStepInfo}),
                  hctx, prob, x, x_n, Δ, lb, ub, Float64(ω), dir, opts, x₊, mx₊, info)
        end
    end
    rc != 0 && _fallback_rc(8, rc) && return reference()       # a shape outside the device path: Morbit's own method
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_n))
    info[].sigma > desc_cfg.min_stepsize ||
        return 0, copy(get_x_scaled(x_it_n)), Xet.(mx₊), 0      # σ too small: no step, m(x_n) (descent.jl:317)
    return ω, Xet.(x₊), Xet.(mx₊), Xet(info[].step_norm)
end

"""
Many starts in one device call (`mrbf_sd_iterate_batch`): `get_criticality` (descent.jl:187-241) followed by the steepest-descent
step (descent.jl:243-318) for independent starts of one problem -- the `Threads.@threads` loop over starts of
examples/large_scale_benchmarks.jl:102-109 -- as one chain of launches and one read-back.  `x_its[p]`, `x_it_ns[p]` and `scs[p]` are
start p's iterate, normal-step iterate and surrogate container; `mop`, `scal` and the configurations belong to the one problem.  For
every start the result is, bit for bit, what `get_criticality` and `hip_compute_descent_step` return on that start alone.  Where the
containers do not share one plan shape, the decision table refuses (`mrbf_dispatch_sd_batch`: a foreign surrogate, d > 256, more than
65535 starts, the limits of the two single calls) or a start's direction LP gave up, those starts take the two single-start functions.
Returns a vector of (ω, d, x₊, mx₊, ‖step‖∞).
"""
function hip_sd_iterate_many(desc_cfg::SteepestDescentConfig, mop, scal, x_its::AbstractVector, x_it_ns::AbstractVector, data_base,
                             scs::AbstractVector{<:SurrogateContainer}, algo_config)
    function single(p)
        ω, d = get_criticality(desc_cfg, mop, scal, x_its[p], x_it_ns[p], data_base, scs[p], algo_config)
        ω₊, x₊, mx₊, nrm = hip_compute_descent_step(desc_cfg, mop, scal, x_its[p], x_it_ns[p], data_base, scs[p], algo_config, ω, d)
        return ω₊, d, x₊, mx₊, nrm
    end
    loop() = [single(p) for p in eachindex(scs)]
    ns = length(scs)
    (ns >= 1 && all(_touches_device, scs)) || return loop()
    plans = [_container_plan(sc) for sc in scs]
    p1 = plans[1]
    same = all(pl -> pl.roles == p1.roles && pl.k == p1.k && pl.n_con == p1.n_con && pl.n_foreign == p1.n_foreign &&
                     length(pl.models) == length(p1.models), plans)
    same || return loop()
    n, k, nm = length(get_x_scaled(x_it_ns[1])), p1.k, length(p1.models)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_sd_batch(ns, n, k, nm, p1.n_con, length(b_eq) + length(b_in), p1.n_foreign, desc_cfg.max_loops) || return loop()
    lb_g, ub_g = full_bounds_internal(scal)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    X = Matrix{Float64}(undef, n, ns); X_n = Matrix{Float64}(undef, n, ns)     # column p = start p: the n_starts x d row-major array
    for p in 1:ns
        X[:, p] .= get_x_scaled(x_its[p]); X_n[:, p] .= get_x_scaled(x_it_ns[p])
    end
    Δ = Float64[get_delta(x_it) for x_it in x_its]
    opts = Ref(MrbfSdStepOptions(desc_cfg.strict_backtracking, desc_cfg.max_loops, desc_cfg.armijo_const_rhs, desc_cfg.armijo_const_shrink,
                                 desc_cfg.min_stepsize))
    dirs = Matrix{Float64}(undef, n, ns); X₊ = Matrix{Float64}(undef, n, ns); MX₊ = Matrix{Float64}(undef, k, ns)
    records = Vector{MrbfSdBatchRecord}(undef, ns)
    ms = Ref{Float32}(0)
    handles = Ptr{Cvoid}[m.handle for pl in plans for m in pl.models]          # start-major
    roles = p1.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    ctx = p1.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin X X_n Δ lb ub dirs X₊ MX₊ records begin
        prob = Ref(MrbfPsProblem(nm, k, C_NULL, pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_sd_iterate_batch, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Ref{MrbfPsProblem}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Int32, Ref{MrbfSdStepOptions}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{MrbfSdBatchRecord},
                   Ref{Float32}),
                  hctx, ns, prob, handles, X, X_n, Δ, lb, ub, desc_cfg.normalize, opts, dirs, X₊, MX₊, records, ms)
        end
    end
    rc != 0 && _fallback_rc(9, rc) && return loop()            # a shape outside the device path: the single-start functions
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_ns[1]))
    return map(1:ns) do p
        r = records[p]
        r.sd_status == 3 && return single(p)                   # MRBF_SD_GAVE_UP: Morbit's JuMP model for this start alone
        r.sigma > desc_cfg.min_stepsize ||
            return 0, Xet.(dirs[:, p]), copy(get_x_scaled(x_it_ns[p])), Xet.(MX₊[:, p]), 0    # descent.jl:317
        (Xet(r.omega), Xet.(dirs[:, p]), Xet.(X₊[:, p]), Xet.(MX₊[:, p]), Xet(r.step_norm))
    end
end

"""
Directed search for many starts in one device call (`mrbf_ds_iterate_batch`): `hip_get_criticality_ds` followed by
`hip_compute_descent_step` for independent starts of one problem -- the `Threads.@threads` loop over starts of
examples/large_scale_benchmarks.jl:102-109 -- as one chain of launches and one read-back.  `x_its[p]`, `x_it_ns[p]` and `scs[p]` are
start p's iterate, normal-step iterate and surrogate container; `mop`, `scal` and the configuration belong to the one problem.  The
image direction r is formed per start (`_ds_image_direction`); with `ideal_point = :device` and no reference point or direction the
ideal points of ALL starts come from one `hip_local_ideal_points_many` call before anything else (`seeds[p]` keys start p's search), and
every start is handed its r, the ones that take the single-start functions too.  For every start the result is, bit for bit, what the two single-start
functions return on that start alone.  Where the containers do not share one plan shape, the decision table refuses
(`mrbf_dispatch_ds_batch`: a foreign surrogate, constraints, d > 256, more than 16 objectives, more than 65535 starts) or a start's
direction QP gave up, those starts take the two single-start functions.  Returns a vector of (ω, d, x₊, mx₊, ‖step‖∞).
"""
function hip_ds_iterate_many(desc_cfg::HipDirectedSearchConfig, mop, scal, x_its::AbstractVector, x_it_ns::AbstractVector, data_base,
                             scs::AbstractVector{<:SurrogateContainer}, algo_config;
                             seeds::AbstractVector{UInt64} = zeros(UInt64, length(scs)))
    step_cfg = _ds_step_config(desc_cfg)
    R_dev = nothing                # k × n_starts: the image directions of all starts, where the device finds the ideal points
    if desc_cfg.ideal_point == :device && isempty(desc_cfg.reference_direction) && isempty(desc_cfg.reference_point) &&
       length(scs) >= 1 && all(_touches_device, scs)
        n0 = length(get_x_scaled(x_it_ns[1]))
        X0 = Matrix{Float64}(undef, n0, length(scs)); LB0 = similar(X0); UB0 = similar(X0)
        for p in eachindex(scs)
            X0[:, p] .= get_x_scaled(x_it_ns[p])
            lb_eff, ub_eff = local_bounds(scal, Vector{Float64}(get_x_scaled(x_its[p])), get_delta(x_its[p]))
            LB0[:, p] .= lb_eff; UB0[:, p] .= ub_eff
        end
        many = hip_local_ideal_points_many([_container_plan(sc) for sc in scs], X0, LB0, UB0;
                                           max_evals = desc_cfg.max_ideal_point_problem_evals, seeds = seeds, lin = _ideal_lin(scal, mop))
        many === nothing || (R_dev = many[1] .- hcat([Vector{Float64}(get_fx(x)) for x in x_it_ns]...))
    end
    function single(p)
        ω, d = hip_get_criticality_ds(desc_cfg, mop, scal, x_its[p], x_it_ns[p], data_base, scs[p], algo_config;
                                      r = R_dev === nothing ? nothing : R_dev[:, p], seed = seeds[p])
        ω₊, x₊, mx₊, nrm = hip_compute_descent_step(step_cfg, mop, scal, x_its[p], x_it_ns[p], data_base, scs[p], algo_config, ω, d)
        return ω₊, d, x₊, mx₊, nrm
    end
    loop() = [single(p) for p in eachindex(scs)]
    ns = length(scs)
    (ns >= 1 && all(_touches_device, scs)) || return loop()
    plans = [_container_plan(sc) for sc in scs]
    p1 = plans[1]
    same = all(pl -> pl.roles == p1.roles && pl.k == p1.k && pl.n_con == p1.n_con && pl.n_foreign == p1.n_foreign &&
                     length(pl.models) == length(p1.models), plans)
    same || return loop()
    n, k, nm = length(get_x_scaled(x_it_ns[1])), p1.k, length(p1.models)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_ds_batch(ns, n, k, nm, p1.n_con, length(b_eq) + length(b_in), p1.n_foreign, desc_cfg.max_loops) || return loop()
    lb_g, ub_g = full_bounds_internal(scal)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    X = Matrix{Float64}(undef, n, ns); X_n = Matrix{Float64}(undef, n, ns)     # column p = start p: the n_starts x d row-major array
    R = Matrix{Float64}(undef, k, ns)
    for p in 1:ns
        X[:, p] .= get_x_scaled(x_its[p]); X_n[:, p] .= get_x_scaled(x_it_ns[p])
        R[:, p] .= R_dev === nothing ? _ds_image_direction(desc_cfg, mop, scal, x_its[p], x_it_ns[p], scs[p]; seed = seeds[p]) : R_dev[:, p]
    end
    Δ = Float64[get_delta(x_it) for x_it in x_its]
    opts = Ref(MrbfSdStepOptions(desc_cfg.strict_backtracking, desc_cfg.max_loops, desc_cfg.armijo_const_rhs, desc_cfg.armijo_const_shrink,
                                 desc_cfg.min_stepsize))
    dirs = Matrix{Float64}(undef, n, ns); X₊ = Matrix{Float64}(undef, n, ns); MX₊ = Matrix{Float64}(undef, k, ns)
    records = Vector{MrbfDsBatchRecord}(undef, ns)
    ms = Ref{Float32}(0)
    handles = Ptr{Cvoid}[m.handle for pl in plans for m in pl.models]          # start-major
    roles = p1.roles
    ctx = p1.models[1].ctx
    rc = GC.@preserve handles roles X X_n Δ lb ub R dirs X₊ MX₊ records begin
        prob = Ref(MrbfPsProblem(nm, k, C_NULL, pointer(roles), 0, 0, C_NULL, C_NULL, C_NULL, C_NULL, -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_ds_iterate_batch, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Ref{MrbfPsProblem}, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Ptr{Float64}, Ref{MrbfSdStepOptions}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Ptr{MrbfDsBatchRecord}, Ref{Float32}),
                  hctx, ns, prob, handles, X, X_n, Δ, lb, ub, R, opts, dirs, X₊, MX₊, C_NULL, records, ms)
        end
    end
    rc != 0 && _fallback_rc(23, rc) && return loop()           # a shape outside the device path: the single-start functions
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_it_ns[1]))
    return map(1:ns) do p
        r = records[p]
        r.ds_status == 3 && return single(p)                   # MRBF_DS_GAVE_UP: the JuMP model for this start alone
        r.sigma > desc_cfg.min_stepsize ||
            return 0, Xet.(dirs[:, p]), copy(get_x_scaled(x_it_ns[p])), Xet.(MX₊[:, p]), 0    # descent.jl:317
        (Xet(r.omega_step), Xet.(dirs[:, p]), Xet.(X₊[:, p]), Xet.(MX₊[:, p]), Xet(r.step_norm))
    end
end

"""
The normal steps of many starts in one device call (`mrbf_normal_step_batch`): `compute_normal_step` (descent.jl:691-757) for
independent starts of one problem -- the `Threads.@threads` loop over starts of examples/large_scale_benchmarks.jl:102-109 -- as one
chain of launches and one read-back.  `x_its[p]` and `scs[p]` are start p's iterate and surrogate container; `mop`, `scal` and the
configuration belong to the one problem.  For every start the result is, bit for bit, what `hip_compute_normal_step` returns on that
start alone.  Where the containers do not share one plan shape, the decision table refuses (`mrbf_dispatch_normal_batch`: a modelled
constraint row on a foreign surrogate, modelled rows at d > 256, more than 65535 starts, the limits of the single call) or a start's LP
gave up, those starts take the single-start function.  Returns a vector of (n, Δ).
"""
function hip_normal_steps_many(mop, scal, x_its::AbstractVector, data_base, scs::AbstractVector{<:SurrogateContainer}, algo_config;
                               variable_radius::Bool = false)
    single(p) = hip_compute_normal_step(mop, scal, x_its[p], data_base, scs[p], algo_config; variable_radius = variable_radius)
    loop() = [single(p) for p in eachindex(scs)]
    ns = length(scs)
    (ns >= 1 && all(_touches_device, scs)) || return loop()
    plans = [_container_plan(sc) for sc in scs]
    p1 = plans[1]
    same = all(pl -> pl.roles == p1.roles && pl.k == p1.k && pl.n_con == p1.n_con && pl.n_foreign == p1.n_foreign &&
                     length(pl.models) == length(p1.models), plans)
    same || return loop()
    n_foreign_con = p1.n_foreign - _container_plan(scs[1]; objectives_only = true).n_foreign   # foreign objectives do not matter here
    d, nm = length(get_x_scaled(x_its[1])), length(p1.models)
    A_eq, b_eq = transformed_linear_eq_constraints(scal, mop)                  # AbstractMOPInterface.jl:463-481: A x_scaled (=, <=) b
    A_in, b_in = transformed_linear_ineq_constraints(scal, mop)
    _dispatch_normal_batch(ns, d, nm, p1.n_con, length(b_eq) + length(b_in), n_foreign_con) || return loop()
    lb_g, ub_g = full_bounds_internal(scal)
    lb = Vector{Float64}(lb_g); ub = Vector{Float64}(ub_g)
    X = Matrix{Float64}(undef, d, ns)                                          # column p = start p: the n_starts x d row-major array
    for p in 1:ns
        X[:, p] .= get_x_scaled(x_its[p])
    end
    Δ = Float64[get_delta(x_it) for x_it in x_its]
    κ_Δ = Float64(filter_kappa_delta(algo_config)); Δ_max = Float64(delta_max(algo_config))
    N = Matrix{Float64}(undef, d, ns)
    records = Vector{MrbfNormalBatchRecord}(undef, ns)
    ms = Ref{Float32}(0)
    handles = Ptr{Cvoid}[m.handle for pl in plans for m in pl.models]          # start-major
    roles = p1.roles
    Aeq = Matrix{Float64}(transpose(Matrix(A_eq))); beq = Vector{Float64}(b_eq)   # row-major rows x d == the d x rows column-major matrix
    Ain = Matrix{Float64}(transpose(Matrix(A_in))); bin = Vector{Float64}(b_in)
    # the table admits linear rows only: the containers' HipRbfModels may all sit in foreign surrogates (no model in the plans)
    ctx = isempty(p1.models) ? mrbf_context() : p1.models[1].ctx
    rc = GC.@preserve handles roles Aeq beq Ain bin X Δ lb ub N records begin
        prob = Ref(MrbfPsProblem(nm, p1.k, C_NULL, pointer(roles), length(beq), length(bin),
                                 isempty(beq) ? C_NULL : pointer(Aeq), isempty(beq) ? C_NULL : pointer(beq),
                                 isempty(bin) ? C_NULL : pointer(Ain), isempty(bin) ? C_NULL : pointer(bin), -1.0))
        _locked(ctx) do hctx
            ccall((:mrbf_normal_step_batch, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Ref{MrbfPsProblem}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                   Float64, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{MrbfNormalBatchRecord}, Ref{Float32}),
                  hctx, ns, prob, handles, d, X, lb, ub, Δ, κ_Δ, Δ_max, variable_radius, N, C_NULL, C_NULL, records, ms)
        end
    end
    rc != 0 && _fallback_rc(12, rc) && return loop()           # a shape outside the device path: the single-start function
    _check(ctx, rc)
    Xet = eltype(get_x_scaled(x_its[1]))
    return map(1:ns) do p
        r = records[p]
        r.status == 2 && return single(p)                      # MRBF_NS_GAVE_UP: Morbit's JuMP model for this start alone
        r.delta == -Inf && return fill(MIN_PRECISION(NaN64), d), -MIN_PRECISION(Inf)      # infeasible (descent.jl:746-748)
        (Xet.(N[:, p]), Xet(r.delta))                          # n already projected into [lb, ub] (descent.jl:752-754)
    end
end

# ---- site selection on the device -----------------------------------------------------------------------------------------------------
mutable struct HipRound4State
    ctx::MrbfContext
    handle::Ptr{Cvoid}
end
function _free_round4!(s::HipRound4State)
    ctx = s.ctx
    if !trylock(ctx.lock)                 # also a finalizer: never block, never release under a running call of the same context
        @async _free_round4!(s)
        return nothing
    end
    try
        if s.handle != C_NULL && ctx.handle != C_NULL
            ccall((:mrbf_free_round4, libmrbf), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.handle, s.handle)
        end
        s.handle = C_NULL
    finally
        unlock(ctx.lock)
    end
    return nothing
end
"(n0, accepted sites, q) of a kept round-4 factor"
function _round4_dims(state::HipRound4State, cfg, n_vars)
    n0 = Ref{Int64}(0); nc = Ref{Int64}(0); nacc = Ref{Int32}(0)
    ccall((:mrbf_round4_sites, libmrbf), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int32}), state.handle, n0, nc, nacc)
    q = cfg.polynomial_degree < 0 ? 0 : (cfg.polynomial_degree == 0 ? 1 : n_vars + 1)
    return n0[], Int(nacc[]), q
end
"""
`_rbf_round4` (RbfModel.jl:352-499) as one device call.  `start_sites` / `cand_sites`: vectors of sites (the sites found so far; the
box candidates in database order, followed -- with `use_max_points` -- by the random box points the caller drew).  Returns the
positions of the accepted candidates in acceptance order and, with `keep_state`, the factors for `fit_from_round4` (`nothing` when
there was nothing to select: the library then keeps no state).  With `rc_only` the return code comes first and nothing is raised.
"""
function rbf_round4_device(cfg::HipRbfConfig, Δ, start_sites, cand_sites; keep_state::Bool = false, rc_only::Bool = false)
    C0 = _dense(_as_matrix(start_sites)); Xc = isempty(cand_sites) ? Matrix{Float64}(undef, size(C0, 1), 0) : _dense(_as_matrix(cand_sites))
    d, n0 = size(C0); mc = size(Xc, 2)
    kid, a, b = _mrbf_kernel_params(Δ, cfg)
    ctx = mrbf_context()
    acc = Vector{Int32}(undef, max(mc, 1)); nacc = Ref{Int32}(0); st = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve C0 Xc acc begin
        _locked(ctx) do hctx
            ccall((:mrbf_round4, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Float64, Float64, Int32, Int32, Float64,
                   Ptr{Int32}, Ref{Int32}, Ptr{Ptr{Cvoid}}),
                  hctx, n0, d, C0, mc, Xc, kid, a, b, cfg.polynomial_degree, cfg.max_model_points, cfg.θ_pivot_cholesky,
                  acc, nacc, keep_state ? Base.unsafe_convert(Ptr{Ptr{Cvoid}}, st) : C_NULL)
        end
    end
    if rc != 0
        rc_only && return rc, Int[], nothing
        _check(ctx, rc)
    end
    accepted = Int.(acc[1:nacc[]]) .+ 1                                         # 1-based positions into cand_sites
    state = nothing
    if keep_state && st[] != C_NULL                                             # NULL: nothing to select, no state (mrbf.h)
        state = HipRound4State(ctx, st[])
        finalizer(_free_round4!, state)
    end
    rc_only && return rc, accepted, state
    return keep_state ? (accepted, state) : accepted
end
"""
Round 4 of many starts in one device call (`mrbf_round4_batch`): `_rbf_round4`'s selection (RbfModel.jl:352-499) for independent
starts of one problem -- the `Threads.@threads` loop over starts of examples/large_scale_benchmarks.jl:102-109 -- with small starts
(d <= 128, q <= n0 <= 256, at most 4096 candidates and 256 sites to accept) sharing six launches and one read-back; any other start
runs `mrbf_round4` inside the call.  `cfgs[p]`, `Δs[p]`, `start_sites[p]` and `cand_sites[p]` (vectors of sites; with `use_max_points`
the caller appends the random box points, as for `rbf_round4_device`) are start p's arguments of `rbf_round4_device`; the starts share
d.  No factor state is kept: the fits of a batch go through `hip_update_models_many`.  Returns, per start, `(rc, positions)`: rc 0 and the
1-based positions of the accepted candidates in acceptance order, or the return code `mrbf_round4` gave for that start (read it with
`_fallback_rc(13, rc)`: take Morbit's own loop for it).  Where the batch does not pay (`_round4_batch_pays`: measured, DESIGN.md section 14), where
the decision table refuses the batch (`mrbf_dispatch_round4_batch`) or the library does (rc -2), every start takes `rbf_round4_device`.
"""
function hip_round4_many(cfgs::AbstractVector{HipRbfConfig}, Δs::AbstractVector{<:Real}, start_sites::AbstractVector, cand_sites::AbstractVector)
    ns = length(cfgs)
    function loop()
        return map(1:ns) do p
            rc, accepted, _ = rbf_round4_device(cfgs[p], Δs[p], start_sites[p], cand_sites[p]; rc_only = true)
            (Int32(rc), accepted)
        end
    end
    (ns >= 1 && _round4_batch_pays(ns, maximum(length, cand_sites))) || return loop()
    C0s = [_dense(_as_matrix(start_sites[p])) for p in 1:ns]
    d = size(C0s[1], 1)
    (all(C -> size(C, 1) == d, C0s) && _dispatch_round4_batch(ns, d)) || return loop()
    Xcs = [isempty(cand_sites[p]) ? Matrix{Float64}(undef, d, 0) : _dense(_as_matrix(cand_sites[p])) for p in 1:ns]
    accs = [Vector{Int32}(undef, max(size(Xcs[p], 2), 1)) for p in 1:ns]
    ctx = mrbf_context()
    ms = Ref{Float32}(0)
    jobs = Vector{MrbfRound4Job}(undef, ns)
    rc = GC.@preserve C0s Xcs accs jobs begin
        for p in 1:ns
            kid, a, b = _mrbf_kernel_params(Δs[p], cfgs[p])
            jobs[p] = MrbfRound4Job(size(C0s[p], 2), size(Xcs[p], 2), pointer(C0s[p]), pointer(Xcs[p]), kid, cfgs[p].polynomial_degree, a, b,
                                    cfgs[p].max_model_points, cfgs[p].θ_pivot_cholesky, pointer(accs[p]), 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_round4_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{MrbfRound4Job}, Ref{Float32}), hctx, ns, d, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(13, rc) && return loop()           # the library refuses the batch: the single call per start
    _check(ctx, rc)
    return map(1:ns) do p
        (jobs[p].rc, Int.(accs[p][1:jobs[p].n_accepted]) .+ 1)
    end
end
"The model on (start sites, accepted sites) from the factor round 4 kept (RbfModel.jl:657-660): `values` in that order, k x n."
function fit_from_round4(state::HipRound4State, values, n_vars::Int, fully_linear::Bool; rc_only::Bool = false)
    Y = _dense(_as_matrix(values)); k = size(Y, 1)
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Ref{MrbfFitInfo}()
    rc = GC.@preserve Y begin
        _locked(state.ctx) do hctx
            ccall((:mrbf_fit_from_round4, libmrbf), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ref{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfFitInfo}),
                  hctx, state.handle, k, Y, h, C_NULL, C_NULL, info)
        end
    end
    if rc != 0
        rc_only && return rc, nothing
        _check(state.ctx, rc)
    end
    model = HipRbfModel(state.ctx, h[], n_vars, k, fully_linear, info[])
    return rc_only ? (rc, model) : model
end
"""
The filter's whole pick loop in one device call (`mrbf_affine_select`): `S` d x mc shifted seeds (picked columns zero), `Q0` the full
orthogonal factor of the directions chosen so far (first `j0` columns), up to `want` further picks above `pivot_val`.  Returns the
1-based positions in pick order and the final p-normalised complement basis.
"""
function affine_select(S::Matrix{Float64}, Q0::Matrix{Float64}, j0::Int, want::Int, pivot_val::Float64, p)
    d, mc = size(S)
    ctx = mrbf_context()
    picks = Vector{Int64}(undef, max(want, 1)); npick = Ref{Int32}(0)
    Zbuf = Matrix{Float64}(undef, d, max(d - j0, 1))
    rc = GC.@preserve S Q0 picks Zbuf begin
        _locked(ctx) do hctx
            ccall((:mrbf_affine_select, libmrbf), Int32,
                  (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Float64, Int32, Ptr{Int64}, Ref{Int32}, Ptr{Float64}),
                  hctx, mc, d, S, j0, Q0, want, pivot_val, isinf(p) ? 1 : 0, picks, npick, Zbuf)
        end
    end
    _check(ctx, rc)
    np = Int(npick[])
    return Int.(picks[1:np]) .+ 1, Zbuf[:, 1:(d - j0 - np)]
end
"""
Many filters in one device call (`mrbf_affine_select_batch`): the pick loops of rounds 1-2 of the training-site selection
(AffinelyIndependentPoints.jl:71-106, called by `_find_suitable_points`, RbfModel.jl:205-238) for independent starts of one problem --
the `Threads.@threads` loop over starts of examples/large_scale_benchmarks.jl:102-109 -- as one launch per pick for all starts and one
read-back.  `Ss[p]` (d x mc_p shifted seeds, picked columns zero), `Q0s[p]` (the full orthogonal factor of the directions chosen so
far, first `j0s[p]` columns), `wants[p]` and `pivot_vals[p]` are start p's arguments of `affine_select`; the starts share d and the
norm `p`.  For every start the result is, bit for bit, what `affine_select` returns on that start alone, whatever its position in the
batch.  Where the decision table refuses the batch (`mrbf_dispatch_affine_batch`: the 2-norm, d > 1023, more than 65535 starts) or the
library does (rc -2), every start takes `affine_select`.  Returns a vector of (1-based positions in pick order, final p-normalised
complement basis).
"""
function affine_select_batch(Ss::AbstractVector{Matrix{Float64}}, Q0s::AbstractVector{Matrix{Float64}}, j0s::AbstractVector{<:Integer},
                             wants::AbstractVector{<:Integer}, pivot_vals::AbstractVector{<:Real}, p)
    ns = length(Ss)
    loop() = [affine_select(Ss[q], Q0s[q], Int(j0s[q]), Int(wants[q]), Float64(pivot_vals[q]), p) for q in 1:ns]
    ns >= 1 || return loop()
    d = size(Ss[1], 1)
    (all(S -> size(S, 1) == d, Ss) && _dispatch_affine_batch(ns, d, p)) || return loop()
    ctx = mrbf_context()
    picks = [Vector{Int64}(undef, max(Int(wants[q]), 1)) for q in 1:ns]
    Zbufs = [Matrix{Float64}(undef, d, max(d - Int(j0s[q]), 1)) for q in 1:ns]
    ms = Ref{Float32}(0)
    jobs = Vector{MrbfAffineJob}(undef, ns)
    rc = GC.@preserve Ss Q0s picks Zbufs jobs begin
        for q in 1:ns
            jobs[q] = MrbfAffineJob(size(Ss[q], 2), j0s[q], wants[q], pivot_vals[q], pointer(Ss[q]), pointer(Q0s[q]), pointer(picks[q]),
                                    pointer(Zbufs[q]), 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_affine_select_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{MrbfAffineJob}, Ref{Float32}),
                  hctx, ns, d, isinf(p) ? 1 : 0, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(10, rc) && return loop()           # a shape outside the batched pick loop: the single call per start
    _check(ctx, rc)
    return map(1:ns) do q
        np = Int(jobs[q].n_picked)
        (Int.(picks[q][1:np]) .+ 1, Zbufs[q][:, 1:(d - Int(j0s[q]) - np)])
    end
end
# (the context's lock is reentrant: hip_update_models_many holds it around the option it sets for this call)
_fit_batch_locked(ctx, ns, jobs, ms) = _locked(ctx) do hctx
    ccall((:mrbf_fit_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Ptr{MrbfFitJob}, Ref{Float32}), hctx, ns, jobs, ms)
end
"""
The model updates of many starts in one device call (`mrbf_fit_batch`): the arithmetic half of `update_model` (RbfModel.jl:743-767) for
independent starts -- the `Threads.@threads` loop over starts of examples/large_scale_benchmarks.jl:102-109 -- with the models kept.
`Cs[p]` (d x n_p sites, one per column), `Ys[p]` (k x n_p values), `Δs[p]` and `cfgs[p]` are start p's training data, radius and
config; `fully_linear[p]` what its meta says.  For every start the model is, bit for bit, the one `mrbf_fit` gives on that start alone
(a start with more than 512 sites that `mrbf_dispatch_fit_batch_max_n` sends into the batch's launch: the one `mrbf_fit` gives with
`MRBF_OPT_SMALL_FIT_MAX_N` at that value).
Where the decision table refuses the batch (`mrbf_dispatch_fit_batch`) or the library does (rc -2), every start takes `mrbf_fit`.
Returns a vector of `HipRbfModel` (`nothing` for a start whose fit failed) and the vector of return codes.  The models of one call
share one device allocation: its memory is reusable once all of them are released (finalizers, or `_free_model!`).
"""
function hip_update_models_many(cfgs::AbstractVector{HipRbfConfig}, Cs::AbstractVector{Matrix{Float64}}, Ys::AbstractVector{Matrix{Float64}},
                                Δs::AbstractVector{<:Real}, fully_linear::AbstractVector{Bool} = fill(false, length(Cs)))
    ns = length(Cs)
    ctx = mrbf_context()
    params = [_mrbf_kernel_params(Δs[q], cfgs[q]) for q in 1:ns]
    function single(q)
        d, n = size(Cs[q]); k = size(Ys[q], 1); kid, a, b = params[q]
        h = Ref{Ptr{Cvoid}}(C_NULL); info = Ref{MrbfFitInfo}()
        rc = GC.@preserve Cs Ys begin
            _locked(ctx) do hctx
                ccall((:mrbf_fit, libmrbf), Int32,
                      (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Float64, Int32,
                       Ref{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Float64}, Ref{MrbfFitInfo}),
                      hctx, n, d, k, Cs[q], Ys[q], kid, a, b, cfgs[q].polynomial_degree, h, C_NULL, C_NULL, info)
            end
        end
        return rc == 0 ? HipRbfModel(ctx, h[], d, k, fully_linear[q], info[]) : nothing, rc
    end
    function loop()
        res = [single(q) for q in 1:ns]
        return [r[1] for r in res], Int32[r[2] for r in res]
    end
    _dispatch_fit_batch(ns) || return loop()
    jobs = Vector{MrbfFitJob}(undef, ns)
    ms = Ref{Float32}(0)
    zero_info = MrbfFitInfo(ntuple(i -> zero(fieldtype(MrbfFitInfo, i)), fieldcount(MrbfFitInfo))...)
    rc = GC.@preserve Cs Ys jobs begin
        for q in 1:ns
            kid, a, b = params[q]
            jobs[q] = MrbfFitJob(size(Cs[q], 2), size(Cs[q], 1), size(Ys[q], 1), kid, cfgs[q].polynomial_degree, a, b, pointer(Cs[q]),
                                 pointer(Ys[q]), C_NULL, C_NULL, C_NULL, 0, 0, zero_info)
        end
        # starts beyond the one-launch fit's default range share the batch's launch up to the n the table names: the context's
        # MRBF_OPT_SMALL_FIT_MAX_N (key 15) is raised for this one call and put back behind it, also on error, under the context's lock.
        # Likewise MRBF_OPT_SMALL_LU (key 16) where the table admits the call's LU-path starts (mrbf_dispatch_fit_batch_lu).
        beyond = [q for q in 1:ns if size(Cs[q], 2) > 512]
        wide_n = isempty(beyond) ? 512 : minimum(_dispatch_fit_batch_max_n(length(beyond), size(Cs[q], 1)) for q in beyond)
        lu = [q for q in 1:ns if _takes_small_lu(params[q], cfgs[q].polynomial_degree, size(Cs[q], 2), size(Cs[q], 1), size(Ys[q], 1))]
        lu_n = isempty(lu) ? 0 : maximum(size(Cs[q], 2) for q in lu)
        opts = Tuple{Int32,Float64}[]
        any(size(Cs[q], 2) <= wide_n for q in beyond) && push!(opts, (Int32(15), Float64(wide_n)))
        !isempty(lu) && all(_dispatch_fit_batch_lu(length(lu), lu_n, size(Cs[q], 1)) for q in lu) && push!(opts, (Int32(16), 1.0))
        if !isempty(opts)
            _locked(ctx) do hctx
                previous = map(opts) do (key, _)
                    v = Ref{Float64}(0.0)
                    _check(ctx, ccall((:mrbf_get_option, libmrbf), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}), hctx, key, v))
                    v[]
                end
                try
                    for (key, value) in opts
                        _check(ctx, ccall((:mrbf_set_option, libmrbf), Int32, (Ptr{Cvoid}, Int32, Float64), hctx, key, value))
                    end
                    _fit_batch_locked(ctx, ns, jobs, ms)
                finally
                    for ((key, _), old) in zip(opts, previous)
                        ccall((:mrbf_set_option, libmrbf), Int32, (Ptr{Cvoid}, Int32, Float64), hctx, key, old)
                    end
                end
            end
        else
            _fit_batch_locked(ctx, ns, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(11, rc) && return loop()           # the library refuses the batch: the single fit per start
    _check(ctx, rc)
    models = map(1:ns) do q
        J = jobs[q]
        J.status == 0 ? HipRbfModel(ctx, J.model, size(Cs[q], 1), size(Ys[q], 1), fully_linear[q], J.info) : nothing
    end
    return models, Int32[jobs[q].status for q in 1:ns]
end
"Scores `‖Z (Zᵀ(ξ - x₀))‖_p` of all filter candidates and the first maximiser (AffinelyIndependentPoints.jl:71-106)."
affine_scores(shifted_seeds::AbstractVector, Z::AbstractMatrix, p = Inf) = affine_scores(_dense(_as_matrix(shifted_seeds)), Z, p)
function affine_scores(S::AbstractMatrix{Float64}, Z::AbstractMatrix, p = Inf)     # S: d x mc, one shifted seed per column
    d, mc = size(S); Zm = Matrix{Float64}(Z)
    ctx = mrbf_context(); best = Ref{Int64}(-1); val = Ref{Float64}(-Inf)
    rc = GC.@preserve S Zm begin
        _locked(ctx) do hctx
            ccall((:mrbf_affine_scores, libmrbf), Int32, (Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{Int64}, Ref{Float64}),
                  hctx, mc, d, size(Zm, 2), S, Zm, isinf(p) ? 1 : 0, C_NULL, best, val)
        end
    end
    _check(ctx, rc)
    return Int(best[]) + 1, val[]
end

# ---- resident site databases: round 3, appends and value updates of many starts in one call each (include/mrbf.h) -------------------

struct MrbfRound3Job        # mirrors mrbf_round3_job, 112 bytes
    db::Ptr{Cvoid}
    x::Ptr{Float64}; lb::Ptr{Float64}; ub::Ptr{Float64}
    pivot_val::Float64
    dirs::Ptr{Float64}
    n_dirs::Int32; reversed::Int32; n_missing::Int32; max_new::Int32
    ensure_fully_linear::Int32; force_rebuild::Int32; mode::Int32; rc::Int32
    new_sites_out::Ptr{Float64}
    first_index::Int64
    n_new::Int32; fully_linear::Int32; status::Int32; n_dirs_used::Int32
end

struct MrbfDbAppendJob      # mirrors mrbf_db_append_job, 48 bytes
    db::Ptr{Cvoid}
    m::Int64
    sites::Ptr{Float64}; values::Ptr{Float64}
    first_index::Int64
    rc::Int32; reserved::Int32
end

struct MrbfDbSetValuesJob   # mirrors mrbf_db_set_values_job, 40 bytes
    db::Ptr{Cvoid}
    m::Int64
    indices::Ptr{Int64}; values::Ptr{Float64}
    rc::Int32; reserved::Int32
end

_dispatch_db_batch(n_starts, d) = ccall((:mrbf_dispatch_db_batch, libmrbf), Int32, (Int64, Int32), n_starts, d) == 1

"An empty resident database for sites of dimension `d` and values of dimension `k` (`mrbf_db_create`); release it with `hip_db_free`."
function hip_db_create(d::Integer, k::Integer; capacity::Integer = 0)
    ctx = mrbf_context(); h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = _locked(ctx) do hctx
        ccall((:mrbf_db_create, libmrbf), Int32, (Ptr{Cvoid}, Int32, Int32, Int64, Ref{Ptr{Cvoid}}), hctx, d, k, capacity, h)
    end
    _check(ctx, rc)
    return h[]
end
function hip_db_free(db::Ptr{Cvoid})
    ctx = mrbf_context()
    rc = _locked(ctx) do hctx
        ccall((:mrbf_db_free, libmrbf), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), hctx, db)
    end
    _check(ctx, rc)
    return nothing
end

"""
`new_result!(db, x, y)` for every start in one device call (`mrbf_db_append_batch`): `sites[p]` is d x m_p (a site per column), `values[p]`
k x m_p or `nothing` (unevaluated rows, stored as NaN).  Returns the 1-based id of the first new row of every database, or `nothing` where
the decision table keeps the call on the host (rc -2: append start by start).
"""
function hip_db_append_many(dbs::AbstractVector{Ptr{Cvoid}}, sites::AbstractVector{Matrix{Float64}}, values::AbstractVector)
    ns = length(dbs)
    (ns >= 1 && _dispatch_db_batch(ns, 1)) || return nothing
    Vs = [values[p] === nothing ? nothing : Matrix{Float64}(values[p]) for p in 1:ns]
    ctx = mrbf_context(); ms = Ref{Float32}(0)
    jobs = Vector{MrbfDbAppendJob}(undef, ns)
    rc = GC.@preserve sites Vs jobs begin
        for p in 1:ns
            jobs[p] = MrbfDbAppendJob(dbs[p], size(sites[p], 2), pointer(sites[p]), Vs[p] === nothing ? Ptr{Float64}(C_NULL) : pointer(Vs[p]), 0, 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_db_append_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Ptr{MrbfDbAppendJob}, Ref{Float32}), hctx, ns, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(18, rc) && return nothing
    _check(ctx, rc)
    return [Int(jobs[p].first_index) + 1 for p in 1:ns]
end

"""
`eval_missing!` for every start in one device call (`mrbf_db_set_values_batch`): `ids[p]` are 1-based row ids, `values[p]` is k x m_p.
Returns the return code of every start (0, or -4 for an id outside the database: nothing of that start is written), or `nothing` where
the decision table keeps the call on the host.
"""
function hip_db_set_values_many(dbs::AbstractVector{Ptr{Cvoid}}, ids::AbstractVector{<:AbstractVector{<:Integer}}, values::AbstractVector{Matrix{Float64}})
    ns = length(dbs)
    (ns >= 1 && _dispatch_db_batch(ns, 1)) || return nothing
    idx = [Int64.(ids[p]) .- 1 for p in 1:ns]
    ctx = mrbf_context(); ms = Ref{Float32}(0)
    jobs = Vector{MrbfDbSetValuesJob}(undef, ns)
    rc = GC.@preserve idx values jobs begin
        for p in 1:ns
            jobs[p] = MrbfDbSetValuesJob(dbs[p], length(idx[p]), pointer(idx[p]), pointer(values[p]), 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_db_set_values_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Ptr{MrbfDbSetValuesJob}, Ref{Float32}), hctx, ns, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(19, rc) && return nothing
    _check(ctx, rc)
    return Int32[jobs[p].rc for p in 1:ns]
end

"""
`_rbf_round3` (RbfModel.jl:269-307) for many starts in one device call (`mrbf_db_round3_batch`), the rebuild along the coordinate axes
(:633-637) done inside the call and the new sites written straight into the resident databases.  `dirs[p]` is a d x n_dirs matrix whose
columns are the improving directions in the order round 3 takes them, or `nothing` for the coordinate axes; `improve = true` is the
improvement step of `prepare_improve_model` (:699-732).  Returns, per start, `(rc, ids, new_sites, fully_linear, rebuilt, n_dirs_used)`
with 1-based ids, or `nothing` where the decision table keeps the call on the host (rc -2: Morbit's own `_rbf_round3` per start).
"""
function hip_db_round3_many(dbs::AbstractVector{Ptr{Cvoid}}, xs::AbstractVector{Vector{Float64}}, lbs::AbstractVector{Vector{Float64}},
        ubs::AbstractVector{Vector{Float64}}, piv_vals::AbstractVector{<:Real}, dirs::AbstractVector, max_news::AbstractVector{<:Integer},
        n_missings::AbstractVector{<:Integer}, ensure_fully_linear::AbstractVector{Bool}, force_rebuild::AbstractVector{Bool}; improve::Bool = false)
    ns = length(dbs)
    ns >= 1 || return nothing
    d = length(xs[1])
    (all(x -> length(x) == d, xs) && _dispatch_db_batch(ns, d)) || return nothing
    Ds = [dirs[p] === nothing ? nothing : Matrix{Float64}(dirs[p]) for p in 1:ns]
    clamp32(v) = Int32(clamp(v, typemin(Int32), typemax(Int32)))
    outs = [Matrix{Float64}(undef, d, max(min(n_missings[p], max_news[p]), min(d, max_news[p]), 1)) for p in 1:ns]
    ctx = mrbf_context(); ms = Ref{Float32}(0)
    jobs = Vector{MrbfRound3Job}(undef, ns)
    rc = GC.@preserve xs lbs ubs Ds outs jobs begin
        for p in 1:ns
            jobs[p] = MrbfRound3Job(dbs[p], pointer(xs[p]), pointer(lbs[p]), pointer(ubs[p]), Float64(piv_vals[p]),
                                    Ds[p] === nothing ? Ptr{Float64}(C_NULL) : pointer(Ds[p]), Ds[p] === nothing ? 0 : size(Ds[p], 2), 0,
                                    clamp32(n_missings[p]), clamp32(max_news[p]), ensure_fully_linear[p] ? 1 : 0, force_rebuild[p] ? 1 : 0,
                                    improve ? 1 : 0, 0, pointer(outs[p]), 0, 0, 0, 0, 0)
        end
        _locked(ctx) do hctx
            ccall((:mrbf_db_round3_batch, libmrbf), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{MrbfRound3Job}, Ref{Float32}), hctx, ns, d, jobs, ms)
        end
    end
    rc != 0 && _fallback_rc(17, rc) && return nothing
    _check(ctx, rc)
    return map(1:ns) do p
        J = jobs[p]
        n = J.rc == 0 ? Int(J.n_new) : 0
        (J.rc, collect(Int(J.first_index) + 1 : Int(J.first_index) + n), outs[p][:, 1:n], J.fully_linear != 0, J.status == 1, Int(J.n_dirs_used))
    end
end
