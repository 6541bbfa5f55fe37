// One batched call of the site selection on ctx->stream (DESIGN.md section 16 "one upload, one read-back").  While the object lives
// the device is set and the pinned block armed; it owns the work buffer laid out by a ByteArena, the host blocks of the upload and of
// the read-back, the event bracket and the one synchronisation.  A return before finish() leaves the stream untouched, the block disarmed.
#pragma once
#include "batch_chain.hpp"
#include "db_host.hpp"

namespace mrbf {
namespace chain {

struct SelectCall {
    mrbf_ctx *ctx;
    hipStream_t s;
    float *ms;  // where finish() puts the time since begin(), or NULL
    PinGuard pin;
    ByteArena A;
    char *base = nullptr;  // the work buffer: A.total bytes of an arena slot
    Block<char> up, back;  // up.p stands for base + A.up_at, back.p for base + A.back_at
    SelectCall(mrbf_ctx *c, float *ms_total) : ctx(c), s(c->stream), ms(ms_total), pin(c) { (void)hipSetDevice(c->device); }
    // the work buffer and the upload block for the layout `L`; the first `zero` bytes of the block are cleared
    int open(Slot slot, const ByteArena &L, size_t zero) {
        A = L;
        MRBF_TRY(get_buf(ctx, slot, A.total, &base));
        up = Block<char>(ctx, A.upload_bytes());
        if (zero && up.own.empty()) std::memset(up.p, 0, zero);  // (the block's own memory comes zeroed: no second pass over megabytes)
        return 0;
    }
    // the piece at offset `off` of the layout: in the work buffer, and (pieces of the upload) in the host block
    template <class T> T *dev(size_t off) const { return reinterpret_cast<T *>(base + off); }
    template <class T> T *host(size_t off) const { return reinterpret_cast<T *>(up.p + (off - A.up_at)); }
    int begin() {
        if (ms) MRBF_HIP(ctx, hipEventRecord(ctx->ev[0], s));
        return 0;
    }
    int upload() {
        MRBF_HIP(ctx, hipMemcpyAsync(base + A.up_at, up.p, A.upload_bytes(), hipMemcpyHostToDevice, s));
        return 0;
    }
    // the first `bytes` of the read-back range to the host block, then the call's one synchronisation
    int finish(size_t bytes) {
        MRBF_HIP(ctx, hipGetLastError());  // of the entry's launches
        if (bytes) back = Block<char>(ctx, bytes);
        if (bytes) MRBF_HIP(ctx, hipMemcpyAsync(back.p, base + A.back_at, bytes, hipMemcpyDeviceToHost, s));
        if (ms) MRBF_HIP(ctx, hipEventRecord(ctx->ev[1], s));
        MRBF_HIP(ctx, hipStreamSynchronize(s));
        if (ms) MRBF_HIP(ctx, hipEventElapsedTime(ms, ctx->ev[0], ctx->ev[1]));
        return 0;
    }
};

}  // namespace chain

namespace db {
// the opening of the five batched calls on resident databases: context, decision table, `jobs` (argument `arg`), the handles, the validation
template <class Job, class Check>
int open_batch(mrbf_ctx *ctx, const char *name, int64_t n_starts, int d, const Job *jobs, int arg, std::vector<DbInfo> &info, Check check) {
    if (!ctx) return -1;
    if (mrbf_dispatch_db_batch(n_starts, d) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "%s: %lld starts, d = %d is outside the batched call (ask mrbf_dispatch_db_batch first)", name, (long long)n_starts, d);
    if (!jobs) return fail(ctx, -arg, "jobs is NULL");
    info.resize((size_t)n_starts);
    for (size_t p = 0; p < info.size(); ++p) info[p] = info_of(ctx, jobs[p].db);
    if (Defect df = check()) return fail(ctx, df.code, "%s: %s", name, df.msg.c_str());
    return 0;
}
}  // namespace db
}  // namespace mrbf
