// Many-start evaluation: mrbf_eval for n_jobs independent (model, query block) pairs in one call -- m(x) and m(x_+) of every start for
// the acceptance test of iterate! (Morbit.jl src/algorithm.jl:766-767), the container sweeps of src/SurrogateContainer.jl:234-269 for
// every start of the reference's Threads.@threads loop (examples/large_scale_benchmarks.jl:102-109), the models mrbf_fit_batch keeps.
// For job i the outputs are, bit for bit, those of mrbf_eval on job i's arguments: there is no evaluation arithmetic here, only the
// descriptor arrays of the single call's kernels (eval_fused_batch, eval_diff's kernel for a non-smooth group), every job with the
// centre-range split of the single call it stands for and partial buffers of its own (batch_chain.hpp).
//
// One call (one chunk of it, where the arena would exceed 2 GiB: eval_batch_host.hpp) is one chain on the ctx stream:
//   one packed upload           the descriptors and every host-side query block
//   eval_fused_batch            one launch group per (kernel and parameters, k, dpad, with or without Jacobians, split or unsplit centre
//                               range); then eval_model for the jobs the fused kernels do not take (dpad > 256, MRBF_OPT_EVAL_IMPL = 1)
//   one read-back               every host-side output
//   one synchronisation
// A buffer the caller keeps on the device is read or written in place: the descriptor carries its address (chain::Member::ext), so
// device-resident Jacobians (C4: 64 x 6450 x 2 x 128 doubles) neither pass through the arena nor are copied.  DESIGN.md section 18.
#include "batch_chain.hpp"
#include "eval_batch_host.hpp"

using namespace mrbf;

namespace {

static_assert(sizeof(mrbf_eval_job) == 48, "mrbf_eval_job is 48 bytes");

// jobs first .. first + count - 1 (validated): plan, arena, upload, launches, read-back, synchronisation
int run_chunk(mrbf_ctx *ctx, mrbf_eval_job *jobs, const evalbatch::Job *shape, int64_t first, int64_t count, float *ms) {
    chain::Plan ev;
    for (int64_t i = 0; i < count; ++i)
        if (evalbatch::active(shape[first + i])) ev.add(ctx, 0, i, 0, jobs[first + i].model, jobs[first + i].m, jobs[first + i].jac_out != nullptr);
    if (ev.mem.empty()) return 0;
    ev.close();
    chain::Arena scratch;
    ev.carve(scratch);
    const evalbatch::Layout L = evalbatch::layout(shape, first, count, ev.desc_doubles(), scratch.total);
    PinGuard pin(ctx);
    double *base;
    MRBF_TRY(get_buf(ctx, S_EVAL_BATCH, L.total, &base));
    chain::Staging up(ctx, L.up_cnt);
    double *hup = up.p;
    for (chain::Member &mb : ev.mem) {
        const mrbf_eval_job &J = jobs[first + mb.p];
        const evalbatch::Place &at = L.at[(size_t)mb.p];
        if (mb.group >= 0) mb.Xq += L.scratch, mb.xsq += L.scratch, mb.vpart += L.scratch, mb.gpart += L.scratch;
        mb.ext = true;
        mb.X_at = at.X == evalbatch::NONE ? J.X : base + at.X;
        mb.vals_at = !J.vals_out ? nullptr : (at.vals == evalbatch::NONE ? J.vals_out : base + at.vals);
        mb.jac_at = !J.jac_out ? nullptr : (at.jac == evalbatch::NONE ? J.jac_out : base + at.jac);
        if (at.X != evalbatch::NONE) std::memcpy(hup + at.X, J.X, (size_t)J.m * mb.M->d * sizeof(double));
    }
    EvalDesc *hdesc = reinterpret_cast<EvalDesc *>(hup + L.desc);
    const EvalDesc *ddesc = reinterpret_cast<const EvalDesc *>(base + L.desc);
    ev.fill(base, hdesc);
    hipStream_t st = ctx->stream;
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, L.up_cnt * sizeof(double), hipMemcpyHostToDevice, st));
    MRBF_TRY(ev.launch(ctx, 0, base, hdesc, ddesc));
    // the read-back: one block into the pinned staging where it fits; beyond that straight into the caller's buffers (no second copy
    // of hundreds of megabytes on the host)
    const bool staged = L.out_cnt * sizeof(double) <= ((size_t)4 << 20);
    chain::Staging down;
    if (staged && L.out_cnt) {
        down = chain::Staging(ctx, L.out_cnt);
        MRBF_HIP(ctx, hipMemcpyAsync(down.p, base + L.out0, L.out_cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    auto each_output = [&](auto &&f) -> int {
        for (const chain::Member &mb : ev.mem) {
            const mrbf_eval_job &J = jobs[first + mb.p];
            const evalbatch::Place &at = L.at[(size_t)mb.p];
            if (at.vals != evalbatch::NONE) MRBF_TRY(f(J.vals_out, at.vals, (size_t)J.m * mb.M->k));
            if (at.jac != evalbatch::NONE) MRBF_TRY(f(J.jac_out, at.jac, (size_t)J.m * mb.M->k * mb.M->d));
        }
        return 0;
    };
    if (!staged)
        MRBF_TRY(each_output([&](double *user, size_t at, size_t cnt) -> int {
            MRBF_HIP(ctx, hipMemcpyAsync(user, base + at, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
            return 0;
        }));
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    if (staged && L.out_cnt)
        MRBF_TRY(each_output([&](double *user, size_t at, size_t cnt) -> int {
            std::memcpy(user, down.p + (at - L.out0), cnt * sizeof(double));
            return 0;
        }));
    float t = 0.f;
    MRBF_HIP(ctx, hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
    *ms += t;
    return 0;
}

}  // namespace

extern "C" int32_t mrbf_eval_batch_limited(mrbf_ctx *ctx, int64_t n_jobs, mrbf_eval_job *jobs, float *ms_total, int64_t arena_limit_bytes) {
    if (!ctx) return -1;
    if (ms_total) *ms_total = 0.f;
    if (mrbf_dispatch_eval_batch(n_jobs) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_eval_batch: %lld jobs outside the device path (ask mrbf_dispatch_eval_batch first)", (long long)n_jobs);
    if (!jobs) return fail(ctx, -3, "jobs is NULL");
    (void)hipSetDevice(ctx->device);
    // ---- what the host logic is told of the jobs; nothing is launched or written unless all of them are valid
    std::vector<evalbatch::Job> shape((size_t)n_jobs);
    for (int64_t i = 0; i < n_jobs; ++i) {
        const mrbf_eval_job &J = jobs[i];
        evalbatch::Job &S = shape[(size_t)i];
        S.has_model = J.model != nullptr, S.m = J.m;
        S.X = J.X != nullptr, S.vals = J.vals_out != nullptr, S.jac = J.jac_out != nullptr;
        if (!J.model) continue;
        S.foreign = J.model->owner != ctx;
        S.d = J.model->d, S.k = J.model->k;
    }
    int64_t bad = 0;
    if (const int rc = evalbatch::validate(shape.data(), n_jobs, &bad)) {
        if (rc == -3)  // every job's own status: mrbf_eval's argument checks
            for (int64_t i = 0; i < n_jobs; ++i) jobs[i].status = !jobs[i].model ? -2 : (jobs[i].m < 0 ? -3 : (jobs[i].m > 0 && !jobs[i].X ? -4 : 0));
        return fail(ctx, rc, rc == -3 ? "mrbf_eval_batch: job %lld is invalid (NULL model, m < 0, or NULL X with m > 0)"
                                      : "mrbf_eval_batch: the model of job %lld belongs to another context", (long long)bad);
    }
    for (int64_t i = 0; i < n_jobs; ++i) {
        evalbatch::Job &S = shape[(size_t)i];
        jobs[i].status = 0;
        if (!evalbatch::active(S)) continue;
        S.X_dev = is_device_ptr(jobs[i].X), S.vals_dev = S.vals && is_device_ptr(jobs[i].vals_out), S.jac_dev = S.jac && is_device_ptr(jobs[i].jac_out);
    }
    // ---- what every job adds to an arena: its descriptor, its host-side buffers, its scratch (what Plan::carve gives it)
    std::vector<size_t> need((size_t)n_jobs, 0);
    for (int64_t i = 0; i < n_jobs; ++i) {
        const evalbatch::Job &S = shape[(size_t)i];
        if (!evalbatch::active(S)) continue;
        chain::Plan one;
        one.add(ctx, 0, 0, 0, jobs[i].model, jobs[i].m, S.jac);
        chain::Arena sc;
        one.carve(sc);
        need[(size_t)i] = evalbatch::pad16(sizeof(EvalDesc) / sizeof(double) + 1) + evalbatch::upload_doubles(S) + evalbatch::vals_doubles(S) +
                          evalbatch::jac_doubles(S) + sc.total;
    }
    const size_t limit = arena_limit_bytes > 0 ? (size_t)arena_limit_bytes : evalbatch::ARENA_LIMIT_BYTES;
    float ms = 0.f;
    for (const auto &c : evalbatch::chunks(need, limit)) MRBF_TRY(run_chunk(ctx, jobs, shape.data(), c.first, c.second, &ms));
    if (ms_total) *ms_total = ms;
    return MRBF_OK;
}

extern "C" int32_t mrbf_eval_batch(mrbf_ctx *ctx, int64_t n_jobs, mrbf_eval_job *jobs, float *ms_total) {
    return mrbf_eval_batch_limited(ctx, n_jobs, jobs, ms_total, 0);
}
