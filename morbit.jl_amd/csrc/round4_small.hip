// Round 4 of the training-site selection for a BATCH of small starts in one call (mrbf_round4_batch, include/mrbf.h) -- what small.hip
// is to the large fit: a kernel of its own for the small shape, not the blocked two-stream walk of round4.hip with a start index
// threaded through it.  A start of a many-start run (the Threads.@threads loop of examples/large_scale_benchmarks.jl:102-109, :253) has
// n0 = d + 1 start sites, at most 2 d + 1 model points and a few hundred candidates: a few million FMAs, for which mrbf_round4 is
// nothing but launch gaps and a host round trip per block of candidates, paid once per start.
//
// The arithmetic is that of round4.hip's header.  Per start, with X0 the start sites (n0 x d), Pi0 their
// polynomial matrix (n0 x q, n0 >= q, full column rank) and G0 = Pi0' Pi0:
//     lam(xi) = Pi0 G0^-1 pi(xi),   p(xi) = phi(X0, xi),   f(xi) = Phi00 lam(xi),   u(xi) = f(xi) / 2 - p(xi)
//     kappa(xi, eta) = phi(|xi - eta|) + lam(xi).u(eta) + lam(eta).u(xi)          (= phi - lam.p - lam.p + (lam.f + lam.f) / 2)
//     H(xi, eta)     = delta + pi(xi)' G0^-1 pi(eta)
// and tau^2(xi | accepted) = s_K / s_H, the ratio of the running Cholesky pivots of K = kappa(acc + xi, acc + xi) and of H -- the
// reference's sigma - ||L^-1 v||^2 (RbfModel.jl:449).  xi is accepted iff tau^2 > (theta^2)^2 (:370, :452) while n0 + accepted <
// max_points.  The reference's rank guard (:433-438) only acts while the sites do not carry the polynomial tail; here n0 >= q with
// full rank is a precondition (a start set that fails it is handed to mrbf_round4, which reports it), so the guard cannot fire and is
// not implemented.
//
// Launches of a call, whatever the number of starts or candidates (starts on a grid dimension, one packed descriptor upload from
// pinned memory, one read-back of counts and lists):
//   r4s_ginv_kernel    one workgroup per start: G0 in LDS, inverted in place by Gauss-Jordan steps (q <= 129: 133 KB of the CU's 160)
//   r4s_stage_kernel   Phi00 and the candidates transposed (coordinate-major: the walk's loads are then contiguous across candidates)
//   r4s_tail_kernel    T = G0^-1 P' (q x mc)
//   r4s_lam_kernel     Lam = Pi0 T and P = phi(X0, candidates) (n0 x mc, candidate index fastest)
//   r4s_u_kernel       U = Phi00 Lam / 2 - P
//   r4s_walk_kernel    one workgroup of 256 threads per start, right-looking: for every candidate still ahead its rows
//                      R(:, j) = L_acc^-1 kappa(acc, j) and the H counterpart live in the start's slice of global memory, the two running
//                      diagonals in LDS.  Every thread takes the decision from the same two LDS words (no broadcast round trip); on an
//                      accept one kappa column is evaluated on demand and one O(accepted x ahead) update follows, a thread per candidate
//                      ahead, every sum in index order.  No atomics: a start's list does not depend on its place in the grid or on the
//                      other starts of the launch.
// The polynomial rows follow poly_rows_kernel's convention (round4.hip: [1, x_1 .. x_d] cut to q terms), restated here so that
// round4.hip stays as it is.
#include "radial.hpp"
#include "round4_host.hpp"  // the small range; the validation, routing and arena of mrbf_round4_batch
#include "select_call.hpp"  // chain::SelectCall: the host scaffold of a batched call

namespace mrbf {
namespace r4s {

constexpr int NT = 256;

#define R4S_GLOBAL __attribute__((address_space(1)))
typedef R4S_GLOBAL double *gdp;
typedef const R4S_GLOBAL double *cgdp;

// one start, as the kernels see it (device memory; the pointers are slices of the context's arena)
struct Job {
    double *X0, *Xc, *XcT, *Ginv, *Phi00, *T, *Lam, *U, *RK, *RH;
    int *out;  // [0] accepted count, [1] 1: the start set's polynomial matrix is rank deficient, [2 ..] accepted positions in acceptance order
    KP kp;
    double thr;
    int n0, mc, q, cap;
};

__device__ __forceinline__ double phi_rt(double s, const KP &kp) {
    switch (kp.kid) {
        case MRBF_CUBIC: return rbf_phi<MRBF_CUBIC>(s, kp);
        case MRBF_INV_MULTIQUADRIC: return rbf_phi<MRBF_INV_MULTIQUADRIC>(s, kp);
        case MRBF_MULTIQUADRIC: return rbf_phi<MRBF_MULTIQUADRIC>(s, kp);
        case MRBF_THIN_PLATE_SPLINE: return rbf_phi<MRBF_THIN_PLATE_SPLINE>(s, kp);
        default: return rbf_phi<MRBF_GAUSSIAN>(s, kp);
    }
}
// term t of the polynomial row of the site x (d coordinates `stride` apart): [1, x_1 .. x_d][t]
__device__ __forceinline__ double poly_term(cgdp x, int64_t stride, int t) { return t == 0 ? 1.0 : x[(int64_t)(t - 1) * stride]; }

// G0 = Pi0' Pi0 and its inverse, in LDS.  In-place Gauss-Jordan without pivoting (G0 is s.p.d.: the pivots are its Schur complements);
// a pivot that is not above 64 eps of its own diagonal entry marks the start set as rank deficient -- the walk is skipped and the
// start goes to mrbf_round4, whose factorisation reports it.
__global__ __launch_bounds__(NT) void r4s_ginv_kernel(const Job *__restrict__ jobs, int d) {
    const Job jb = jobs[blockIdx.x];
    const int q = jb.q, n0 = jb.n0, tid = threadIdx.x;
    if (q == 0) return;
    extern __shared__ double sm[];
    double *A = sm, *col = A + q * q, *row = col + q, *dg = row + q;
    cgdp X0 = (cgdp)jb.X0;
    for (int e = tid; e < q * q; e += NT) {
        const int t = e / q, u = e % q;
        double s = 0.0;
        for (int i = 0; i < n0; ++i) s = fma(poly_term(X0 + (int64_t)i * d, 1, t), poly_term(X0 + (int64_t)i * d, 1, u), s);
        A[e] = s;
    }
    __syncthreads();
    for (int t = tid; t < q; t += NT) dg[t] = A[t * q + t];
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < q; ++k) {
        const double piv = A[k * q + k];  // (every thread reads the same word: the exit is uniform)
        if (!(piv > 64.0 * 2.220446049250313e-16 * dg[k]) || !(piv < 1e300)) {
            bad = 1;
            break;
        }
        const double p = 1.0 / piv;
        __syncthreads();  // piv has been read by everybody, col / row of the step before are free
        for (int t = tid; t < q; t += NT) {
            col[t] = A[t * q + k];
            row[t] = A[k * q + t] * p;
        }
        __syncthreads();
        for (int e = tid; e < q * q; e += NT) {
            const int i = e / q, j = e % q;
            if (i == k)
                A[e] = (j == k) ? p : row[j];
            else
                A[e] = (j == k) ? -col[i] * p : fma(-col[i], row[j], A[e]);
        }
        __syncthreads();
    }
    gdp Ginv = (gdp)jb.Ginv;
    for (int e = tid; e < q * q; e += NT) Ginv[e] = A[e];
    if (tid == 0) ((R4S_GLOBAL int *)jb.out)[1] = bad;
}

// Phi00[i][i2] = phi(|x_i - x_i2|) (difference form) and XcT[k][j] = Xc[j][k]
__global__ __launch_bounds__(NT) void r4s_stage_kernel(const Job *__restrict__ jobs, int d) {
    const Job jb = jobs[blockIdx.y];
    const int64_t n0 = jb.n0, mc = jb.mc, nphi = n0 * n0, nx = mc * d, tot = nphi > nx ? nphi : nx;
    cgdp X0 = (cgdp)jb.X0, Xc = (cgdp)jb.Xc;
    gdp Phi00 = (gdp)jb.Phi00, XcT = (gdp)jb.XcT;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * NT) {
        if (e < nphi) {
            const int64_t i = e / n0, i2 = e % n0;
            double s = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = X0[i * d + k] - X0[i2 * d + k];
                s = fma(df, df, s);
            }
            Phi00[e] = phi_rt(s, jb.kp);
        }
        if (e < nx) {
            const int64_t j = e / d, k = e % d;
            XcT[k * mc + j] = Xc[e];
        }
    }
}

// T[t][j] = sum_u Ginv[t][u] pi_j[u]
__global__ __launch_bounds__(NT) void r4s_tail_kernel(const Job *__restrict__ jobs, int d) {
    const Job jb = jobs[blockIdx.y];
    const int q = jb.q;
    const int64_t mc = jb.mc, tot = (int64_t)q * mc;
    cgdp Ginv = (cgdp)jb.Ginv, XcT = (cgdp)jb.XcT;
    gdp T = (gdp)jb.T;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * NT) {
        const int64_t t = e / mc, j = e % mc;
        double s = 0.0;
#pragma unroll 4
        for (int u = 0; u < q; ++u) s = fma(Ginv[t * q + u], poly_term(XcT + j, mc, u), s);
        T[e] = s;
    }
}

// Lam[i][j] = sum_t pi0_i[t] T[t][j];  U[i][j] = phi(|x0_i - xc_j|) for now (r4s_u_kernel finishes it)
__global__ __launch_bounds__(NT) void r4s_lam_kernel(const Job *__restrict__ jobs, int d) {
    const Job jb = jobs[blockIdx.y];
    const int q = jb.q;
    const int64_t mc = jb.mc, tot = (int64_t)jb.n0 * mc;
    cgdp X0 = (cgdp)jb.X0, XcT = (cgdp)jb.XcT, T = (cgdp)jb.T;
    gdp Lam = (gdp)jb.Lam, U = (gdp)jb.U;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / mc, j = e % mc;
        cgdp x0 = X0 + i * d;
        double s = 0.0;
#pragma unroll 4
        for (int t = 0; t < q; ++t) s = fma(poly_term(x0, 1, t), T[(int64_t)t * mc + j], s);
        Lam[e] = s;
        double r2 = 0.0;
#pragma unroll 4
        for (int k = 0; k < d; ++k) {
            const double df = x0[k] - XcT[(int64_t)k * mc + j];
            r2 = fma(df, df, r2);
        }
        U[e] = phi_rt(r2, jb.kp);
    }
}

// U[i][j] = (Phi00 Lam)[i][j] / 2 - P[i][j]   (in place: every thread replaces the one entry of P it reads)
__global__ __launch_bounds__(NT) void r4s_u_kernel(const Job *__restrict__ jobs) {
    const Job jb = jobs[blockIdx.y];
    const int n0 = jb.n0;
    const int64_t mc = jb.mc, tot = (int64_t)n0 * mc;
    cgdp Phi00 = (cgdp)jb.Phi00, Lam = (cgdp)jb.Lam;
    gdp U = (gdp)jb.U;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * NT) {
        const int64_t i = e / mc, j = e % mc;
        double s = 0.0;
        if (jb.q > 0) {
#pragma unroll 4
            for (int i2 = 0; i2 < n0; ++i2) s = fma(Phi00[i * n0 + i2], Lam[(int64_t)i2 * mc + j], s);
        }
        U[e] = 0.5 * s - U[e];
    }
}

// The walk of one start.  LDS: dK[mc] | dH[mc] | xa[d] | la[n0] | ua[n0] | ta[max(q, 1)] | ra[cap] | ha[cap]
__global__ __launch_bounds__(NT) void r4s_walk_kernel(const Job *__restrict__ jobs, int d) {
    const Job jb = jobs[blockIdx.x];
    const int n0 = jb.n0, q = jb.q, cap = jb.cap, tid = threadIdx.x;
    const int64_t mc = jb.mc;
    extern __shared__ double sm[];
    double *dK = sm, *dH = dK + mc, *xa = dH + mc, *la = xa + d, *ua = la + n0, *ta = ua + n0, *ra = ta + (q > 0 ? q : 1), *ha = ra + cap;
    cgdp XcT = (cgdp)jb.XcT, T = (cgdp)jb.T, Lam = (cgdp)jb.Lam, U = (cgdp)jb.U;
    gdp RK = (gdp)jb.RK, RH = (gdp)jb.RH;  // (written and read back by different threads of this workgroup, a barrier in between)
    R4S_GLOBAL int *out = (R4S_GLOBAL int *)jb.out;
    const KP kp = jb.kp;
    if (q > 0 && out[1] != 0) {  // rank-deficient start set (r4s_ginv_kernel): nothing is decided here
        if (tid == 0) out[0] = 0;
        return;
    }
    // the diagonals: kappa(xi, xi) = phi(0) + 2 lam(xi).u(xi),  H(xi, xi) = 1 + pi(xi).T(xi)
    for (int64_t j = tid; j < mc; j += NT) {
        double s = 0.0;
        for (int i = 0; i < n0; ++i) s = fma(Lam[(int64_t)i * mc + j], U[(int64_t)i * mc + j], s);
        dK[j] = fma(2.0, s, kp.phi0);
        double h = 0.0;
        for (int t = 0; t < q; ++t) h = fma(poly_term(XcT + j, mc, t), T[(int64_t)t * mc + j], h);
        dH[j] = 1.0 + h;
    }
    __syncthreads();
    int nacc = 0;
    for (int64_t j = 0; j < mc; ++j) {
        if (nacc >= cap) break;  // max_points reached (cap = min(mc, max_points - n0))
        // the decision: the same two words, the same operations in every thread.  A non-finite pivot or s_H <= 0 rejects (NaN fails
        // every comparison) and leaves the factors as they are.
        const double sK = dK[j], sH = dH[j];
        const double tau2 = sK / sH;
        if (!(sH > 0.0 && sK > 0.0 && tau2 > jb.thr && tau2 < 1e300)) continue;
        for (int k = tid; k < d; k += NT) xa[k] = XcT[(int64_t)k * mc + j];
        for (int i = tid; i < n0; i += NT) {
            la[i] = Lam[(int64_t)i * mc + j];
            ua[i] = U[(int64_t)i * mc + j];
        }
        for (int t = tid; t < q; t += NT) ta[t] = T[(int64_t)t * mc + j];
        for (int r = tid; r < nacc; r += NT) {
            ra[r] = RK[(int64_t)r * mc + j];
            if (q > 0) ha[r] = RH[(int64_t)r * mc + j];
        }
        __syncthreads();
        const double rsK = 1.0 / sqrt(sK), rsH = 1.0 / sqrt(sH);
        // the new factor row for every candidate ahead: one kappa column on demand, then the rows so far (sums in index order)
        for (int64_t c = j + 1 + tid; c < mc; c += NT) {
            double r2 = 0.0;
#pragma unroll 4
            for (int k = 0; k < d; ++k) {
                const double df = xa[k] - XcT[(int64_t)k * mc + c];
                r2 = fma(df, df, r2);
            }
            double tail = 0.0;
#pragma unroll 4
            for (int i = 0; i < n0; ++i) {
                tail = fma(la[i], U[(int64_t)i * mc + c], tail);
                tail = fma(ua[i], Lam[(int64_t)i * mc + c], tail);
            }
            double dot = 0.0;
#pragma unroll 4
            for (int r = 0; r < nacc; ++r) dot = fma(ra[r], RK[(int64_t)r * mc + c], dot);
            const double v = ((phi_rt(r2, kp) + tail) - dot) * rsK;
            RK[(int64_t)nacc * mc + c] = v;
            dK[c] = fma(-v, v, dK[c]);
            if (q > 0) {
                double h = 0.0;
#pragma unroll 4
                for (int t = 0; t < q; ++t) h = fma(ta[t], poly_term(XcT + c, mc, t), h);
                double hd = 0.0;
#pragma unroll 4
                for (int r = 0; r < nacc; ++r) hd = fma(ha[r], RH[(int64_t)r * mc + c], hd);
                const double w = (h - hd) * rsH;
                RH[(int64_t)nacc * mc + c] = w;
                dH[c] = fma(-w, w, dH[c]);
            }
        }
        if (tid == 0) out[2 + nacc] = (int)j;
        ++nacc;
        __syncthreads();  // the diagonals and rows of this step are visible, the staged vectors free
    }
    if (tid == 0) out[0] = nacc;
}

}  // namespace r4s
}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_round4_batch(mrbf_ctx *ctx, int64_t n_starts, int32_t d, mrbf_round4_job *jobs, float *ms_total) {
    using namespace r4s;
    if (!ctx) return -1;
    if (mrbf_dispatch_round4_batch(n_starts, d) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_round4_batch: %lld starts, d = %d is outside the batched call (ask mrbf_dispatch_round4_batch first)",
                    (long long)n_starts, d);
    if (!jobs) return fail(ctx, -4, "jobs is NULL");
    const size_t N = (size_t)n_starts, D = (size_t)d;
    const Plan P = plan(n_starts, d, jobs, sizeof(Job), 4);
    if (P.bad) return fail(ctx, P.bad.code, "%s", P.bad.msg.c_str());
    for (size_t p = 0; p < N; ++p) jobs[p].n_accepted = 0, jobs[p].rc = 0;
    if (ms_total) *ms_total = 0.f;
    std::vector<int> hback;
    if (P.nb > 0) {
        // (a scope of its own: guard released, read-back copied out of the pinned block before the single calls below arm it again)
        chain::SelectCall call(ctx, ms_total);
        hipStream_t s = call.s;
        // ---- the arena: output words | descriptors | the starts' slices
        MRBF_TRY(call.open(S_R4_BATCH, P.A, 0));
        int *dOut = call.dev<int>(P.oOut);
        const Job *dDesc = call.dev<const Job>(P.oDesc);
        Job *hdesc = call.host<Job>(P.oDesc);
        MRBF_TRY(call.begin());
        MRBF_HIP(ctx, hipMemsetAsync(dOut, 0, P.A.back_bytes(), s));
        size_t k = 0;
        for (size_t p = 0; p < N; ++p) {
            const Start &st = P.st[p];
            if (st.route != BATCHED) continue;
            const mrbf_round4_job &jb = jobs[p];
            const size_t n0 = (size_t)jb.n0, mc = (size_t)jb.mc;
            auto slice = [&](size_t off) { return call.dev<double>(P.oSlices + off); };
            Job &h = hdesc[k];
            h.X0 = slice(st.X0), h.Xc = slice(st.Xc), h.XcT = slice(st.XcT), h.Ginv = slice(st.Ginv), h.Phi00 = slice(st.Phi00);
            h.T = slice(st.T), h.Lam = slice(st.Lam), h.U = slice(st.U), h.RK = slice(st.RK), h.RH = slice(st.RH);
            h.out = dOut + k * P.ostride;
            h.kp = make_kp(jb.kernel_id, jb.a, jb.b);
            const double th = jb.theta_pivot_cholesky;
            h.thr = (th * th) * (th * th);
            h.n0 = (int)n0, h.mc = (int)mc, h.q = st.q, h.cap = st.cap;
            // the sites, straight from where they are (host or device)
            MRBF_HIP(ctx, hipMemcpyAsync(h.X0, jb.start_sites, n0 * D * 8, hipMemcpyDefault, s));
            MRBF_HIP(ctx, hipMemcpyAsync(h.Xc, jb.cand_sites, mc * D * 8, hipMemcpyDefault, s));
            ++k;
        }
        MRBF_TRY(call.upload());
        const unsigned NB = (unsigned)P.nb;
        auto gx = [](int64_t elems) { return (unsigned)std::min<int64_t>(std::max<int64_t>((elems + NT - 1) / NT, 1), 4096); };
        const size_t shm_g = ((size_t)P.q_max * P.q_max + 3 * (size_t)std::max(P.q_max, 1)) * sizeof(double);
        const size_t shm_w = (2 * (size_t)P.mc_max + D + 2 * (size_t)P.n0_max + (size_t)std::max(P.q_max, 1) + 2 * (size_t)P.cap_max) * sizeof(double);
        MRBF_HIP(ctx, hipFuncSetAttribute((const void *)r4s_ginv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_g));
        MRBF_HIP(ctx, hipFuncSetAttribute((const void *)r4s_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_w));
        hipLaunchKernelGGL(r4s_ginv_kernel, dim3(NB), dim3(NT), shm_g, s, dDesc, d);
        hipLaunchKernelGGL(r4s_stage_kernel, dim3(gx(std::max<int64_t>(P.n0_max * P.n0_max, P.mc_max * d)), NB), dim3(NT), 0, s, dDesc, d);
        hipLaunchKernelGGL(r4s_tail_kernel, dim3(gx((int64_t)P.q_max * P.mc_max), NB), dim3(NT), 0, s, dDesc, d);
        hipLaunchKernelGGL(r4s_lam_kernel, dim3(gx(P.n0_max * P.mc_max), NB), dim3(NT), 0, s, dDesc, d);
        hipLaunchKernelGGL(r4s_u_kernel, dim3(gx(P.n0_max * P.mc_max), NB), dim3(NT), 0, s, dDesc);
        hipLaunchKernelGGL(r4s_walk_kernel, dim3(NB), dim3(NT), shm_w, s, dDesc, d);
        // ---- one read-back: counts, flags and lists of every start
        MRBF_TRY(call.finish(P.nb * P.ostride * sizeof(int)));
        hback.assign(reinterpret_cast<const int *>(call.back.p), reinterpret_cast<const int *>(call.back.p) + P.nb * P.ostride);
    }
    // ---- results; starts outside the small range, and starts whose start set the batched chain found rank deficient, take the single
    // call here, after the chain, without a kept state: one such start does not fail the others
    size_t k = 0;
    for (size_t p = 0; p < N; ++p) {
        mrbf_round4_job &jb = jobs[p];
        if (P.st[p].route == BATCHED) {
            const int *o = hback.data() + k * P.ostride;
            ++k;
            if (o[1] == 0) {
                const int na = std::min(o[0], P.st[p].cap);
                for (int i = 0; i < na; ++i) jb.accepted_out[i] = o[2 + i];
                jb.n_accepted = na;
                continue;
            }
        } else if (P.st[p].route == DONE) {
            continue;
        }
        int32_t na = 0;
        jb.rc = mrbf_round4(ctx, jb.n0, d, jb.start_sites, jb.mc, jb.cand_sites, jb.kernel_id, jb.a, jb.b, jb.poly_deg, jb.max_points,
                            jb.theta_pivot_cholesky, jb.accepted_out, &na, nullptr);
        jb.n_accepted = jb.rc == 0 ? na : 0;
    }
    return MRBF_OK;
}
