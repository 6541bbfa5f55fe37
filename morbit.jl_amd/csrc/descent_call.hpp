// descent_call_host.hpp's arithmetic on the runtime: the outputs of a *_direction entry as device pointers and their copies back, the packed
// input block of a single-start call fetched, uploaded and viewed, the three int words behind such a call's output doubles
#pragma once
#include "common.hpp"
#include "descent_call_host.hpp"

namespace mrbf {
namespace dcall {

struct Outputs {
    std::vector<Out> o;
    char *stage = nullptr;
    int open(mrbf_ctx *ctx, Slot slot, std::initializer_list<Out> outs) {
        o = outs;
        for (Out &a : o) a.device = is_device_ptr(a.user);
        return get_buf(ctx, slot, out_layout(o.data(), o.size()) * sizeof(double), (void **)&stage);
    }
    // what the kernel writes: the staged piece, the caller's device buffer, or NULL for an output that was not given
    template <class T> T *at(int i) const { return reinterpret_cast<T *>(o[i].at != NONE ? stage + o[i].at : (o[i].device ? (char *)o[i].user : nullptr)); }
    int copy_back(mrbf_ctx *ctx) const {  // the staged pieces to the caller's host buffers, in list order, on the stream
        for (const Out &a : o)
            if (a.at != NONE) MRBF_HIP(ctx, hipMemcpyAsync(a.user, stage + a.at, a.count * (a.is_int ? sizeof(int32_t) : sizeof(double)), hipMemcpyDeviceToHost, ctx->stream));
        return 0;
    }
};

// pieces fetched into one host vector in the order they are asked for (host or device memory), one upload, device views by the same offsets
struct PackedIn : Pack {
    std::vector<double> h;
    const double *base = nullptr;
    int rc = 0;  // of the first fetch that failed; the later ones are skipped
    size_t room(size_t count) {
        h.resize(total + count);
        return add(count);
    }
    size_t fetch(mrbf_ctx *ctx, const double *src, size_t count) {
        const size_t at = room(count);
        if (!rc) rc = input_fetch(ctx, src, count, h.data() + at);
        return at;
    }
    std::pair<size_t, size_t> fetch_linear_rows(mrbf_ctx *ctx, const mrbf_ps_problem *prob, int d) {  // the container's linear rows (eq, then ineq), their b
        const size_t n_lin = (size_t)prob->n_lin_eq + (size_t)prob->n_lin_ineq, A = room(n_lin * d), b = room(n_lin);
        if (!rc) rc = mrbf::fetch_linear_rows(ctx, prob, d, h.data() + A, h.data() + b);
        return {A, b};
    }
    int upload(mrbf_ctx *ctx, double *arena) {
        base = arena;
        MRBF_HIP(ctx, hipMemcpyAsync(arena, h.data(), total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    const double *dev(size_t at) const { return base + at; }
};

// the three int words behind a single-start call's output doubles: status, iterations and the solver's own count
inline void read_status(const double *words, int32_t *status, int32_t *iterations, int32_t *count) {
    int32_t w[3];
    std::memcpy(w, words, sizeof(w));
    *status = w[0], *iterations = w[1], *count = w[2];
}

}  // namespace dcall
}  // namespace mrbf
