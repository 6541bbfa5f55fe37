// Host logic of mrbf_round4_batch (round4_small.hip): the validation of the jobs, the route of every start and the arena with the
// starts' slices.  No HIP include, no context, a defect by value: tools/select_host_check.cpp drives it as a plain C++ program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mrbf.h"
#include "select_host.hpp"

namespace mrbf {
namespace r4s {

constexpr int R4S_MAX_D = 128, R4S_MAX_N0 = 256, R4S_MAX_MC = 4096, R4S_MAX_ACC = 256;  // the small range (include/mrbf.h)
constexpr size_t R4S_ARENA_MAX = (size_t)2 << 30;  // starts whose slices would take the batch beyond this take the single call

enum Route { DONE = 0, BATCHED = 1, SINGLE = 2 };

// one start: q terms of the tail; cap = min(mc, max_points - n0) sites it may accept (max_points <= 0: (d + 1)(d + 2) / 2); its route --
// SINGLE: n0 < q, or outside the small range, or no room left for its slices; DONE: mc == 0 or cap <= 0; BATCHED: inside the R4S_MAX_*
// limits while the slices of the batch fit R4S_ARENA_MAX -- and, BATCHED, its slices (bytes from Plan::oSlices, 256-byte multiples):
//   X0 (n0 x d) | Xc | XcT (mc x d each) | Ginv (q x q) | Phi00 (n0 x n0) | T (q x mc) | Lam | U (n0 x mc each) | RK | RH (cap x mc each),
//   doubles; Ginv and T at least one; without a tail (q = 0) RH is RK.
struct Start {
    int route = SINGLE, q = 0, cap = 0;
    size_t X0 = 0, Xc = 0, XcT = 0, Ginv = 0, Phi00 = 0, T = 0, Lam = 0, U = 0, RK = 0, RH = 0;
};
// the call: nb BATCHED starts in job order; `A` = output words (ostride = cap_max + 2 ints each: the read-back) | descriptors (the upload) | slices
struct Plan {
    Defect bad;
    std::vector<Start> st;
    size_t nb = 0, ostride = 2;
    int cap_max = 0, q_max = 0;  // over the BATCHED starts, as mc_max and n0_max
    int64_t mc_max = 0, n0_max = 0;
    ByteArena A;
    size_t oOut = 0, oDesc = 0, oSlices = 0;
};
// every defect reports as argument `arg` (4); the first in job order wins, within a job the first of the checks below
inline Plan plan(int64_t n_starts, int d, const mrbf_round4_job *jobs, size_t desc_bytes, int arg) {
    Plan P;
    const size_t N = (size_t)n_starts, D = (size_t)d;
    P.st.resize(N);
    ByteArena S;  // the slices
    for (size_t p = 0; p < N; ++p) {
        const mrbf_round4_job &jb = jobs[p];
        const int q = jb.poly_deg < 0 ? 0 : (jb.poly_deg == 0 ? 1 : d + 1);  // (poly_dim of common.hpp)
        const int64_t mp = jb.max_points <= 0 ? (int64_t)(d + 1) * (d + 2) / 2 : jb.max_points;
        const int64_t cap = std::min<int64_t>(jb.mc, mp - jb.n0);
        std::string what;
        if (jb.n0 < 1) what = ".n0 = " + std::to_string(jb.n0);
        else if (jb.mc < 0) what = ".mc = " + std::to_string(jb.mc);
        else if (!jb.start_sites) what = ".start_sites is NULL";
        else if (jb.mc > 0 && !jb.cand_sites) what = ".cand_sites is NULL";
        else if (jb.kernel_id < 0 || jb.kernel_id > 4) what = ".kernel_id out of range";
        else if (jb.poly_deg < -1 || jb.poly_deg > 1) what = ".poly_deg must be -1, 0 or 1";
        else if (cap > 0 && !jb.accepted_out) what = ".accepted_out is NULL";
        if (!what.empty()) {
            P.bad.code = -arg, P.bad.msg = "jobs[" + std::to_string(p) + "]" + what;
            return P;
        }
        Start &st = P.st[p];
        st.q = q;
        if (jb.n0 < q) continue;  // (mrbf_round4 refuses it with its own code)
        if (jb.mc == 0 || cap <= 0) st.route = DONE;  // nothing to select (RbfModel.jl:368)
        if (st.route == DONE || d > R4S_MAX_D || jb.n0 > R4S_MAX_N0 || jb.mc > R4S_MAX_MC || cap > R4S_MAX_ACC) continue;
        const size_t n0 = (size_t)jb.n0, mc = (size_t)jb.mc, Q = (size_t)q, C = (size_t)cap, w = sizeof(double);
        ByteArena T = S;  // with this start's slices
        st.X0 = T.take(n0 * D * w), st.Xc = T.take(mc * D * w), st.XcT = T.take(mc * D * w), st.Ginv = T.take(std::max<size_t>(Q * Q, 1) * w);
        st.Phi00 = T.take(n0 * n0 * w), st.T = T.take(std::max<size_t>(Q * mc, 1) * w), st.Lam = T.take(n0 * mc * w), st.U = T.take(n0 * mc * w);
        st.RK = T.take(C * mc * w), st.RH = Q > 0 ? T.take(C * mc * w) : st.RK;
        if (T.total > R4S_ARENA_MAX) continue;
        S = T;
        st.route = BATCHED, st.cap = (int)cap;
        ++P.nb;
        P.cap_max = std::max(P.cap_max, (int)cap), P.q_max = std::max(P.q_max, q);
        P.mc_max = std::max(P.mc_max, jb.mc), P.n0_max = std::max(P.n0_max, jb.n0);
    }
    P.ostride = (size_t)P.cap_max + 2;
    P.oOut = P.A.take(P.nb * P.ostride * sizeof(int)), P.oDesc = P.A.take(P.nb * desc_bytes), P.oSlices = P.A.take(S.total);
    P.A.back_end = P.A.up_at = P.oDesc, P.A.up_end = P.oSlices;
    return P;
}

}  // namespace r4s
}  // namespace mrbf
