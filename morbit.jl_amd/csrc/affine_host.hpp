// Host logic of mrbf_affine_select_batch (affine.hip): the validation of the jobs, the picks every start wants and the call's arena.
// No HIP include, no context, a defect by value: tools/select_host_check.cpp drives it as a plain C++ program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mrbf.h"
#include "select_host.hpp"

namespace mrbf {
namespace affine {

constexpr int AFF_G = 8;                      // candidates of one workgroup of the projection, score and pick kernels
constexpr int64_t MC_MAX = (int64_t)1 << 26;  // candidates of a start, and of a batch in all

// Every defect reports as argument `arg` (5); the first in job order wins, within a job the first of the checks below.
//   want[p] = mc > 0 ? min(max_picks, d - j0) : 0 picks start p may make; T = max want[p] launches of the pick loop;
//   ngrp_max = max ceil(mc / AFF_G) over the starts with want[p] > 0: the width of the grids.
// The arena (bytes, 256-byte multiples): state (4 ints per start) | picks (d int64 per start) | hv (hvn = 2 d + 8 doubles per start) |
//   descriptors | Q | Zs (d x d doubles per start each) | val (a double per candidate) | C | S (d doubles per candidate each; room
//   for one candidate when there is none).  State and picks come back in one copy, descriptors and start bases go up in one.
struct Plan {
    Defect bad;
    std::vector<int> want;
    int T = 0;
    int64_t ngrp_max = 0, mc_sum = 0;
    ByteArena A;
    size_t hvn = 0, oState = 0, oPicks = 0, oHv = 0, oDesc = 0, oQ = 0, oZs = 0, oVal = 0, oC = 0, oS = 0;
};
inline Plan plan(int64_t n_starts, int d, const mrbf_affine_job *jobs, size_t desc_bytes, int arg) {
    Plan P;
    const size_t N = (size_t)n_starts, D = (size_t)d;
    P.want.assign(N, 0);
    auto bad = [&](size_t p, const char *what) {
        P.bad.code = -arg, P.bad.msg = "jobs[" + std::to_string(p) + "]" + what;
        return P;
    };
    for (size_t p = 0; p < N; ++p) {
        const mrbf_affine_job &jb = jobs[p];
        if (jb.mc < 0 || jb.mc > MC_MAX) return bad(p, ".mc out of range");
        if (jb.j0 < 0 || jb.j0 > d) return bad(p, ".j0 must lie in [0, d]");
        if (jb.j0 > 0 && !jb.Q0) return bad(p, ".Q0 is NULL");
        if (jb.max_picks < 0) return bad(p, ".max_picks < 0");
        if (jb.mc > 0 && !jb.shifted) return bad(p, ".shifted is NULL");
        const int mp = std::min(jb.max_picks, d - jb.j0);
        if (mp > 0 && !jb.picked_out) return bad(p, ".picked_out is NULL");
        P.mc_sum += jb.mc;
        if (P.mc_sum > MC_MAX) {
            P.bad.code = -arg, P.bad.msg = "mrbf_affine_select_batch: more than 2^26 candidates in all";
            return P;
        }
        P.want[p] = jb.mc > 0 ? mp : 0;
        if (P.want[p] > 0) P.T = std::max(P.T, P.want[p]), P.ngrp_max = std::max(P.ngrp_max, (jb.mc + AFF_G - 1) / AFF_G);
    }
    const size_t mcs = (size_t)std::max<int64_t>(P.mc_sum, 1), w = sizeof(double);
    P.hvn = 2 * D + 8;
    P.oState = P.A.take(N * 4 * sizeof(int)), P.oPicks = P.A.take(N * D * sizeof(long long)), P.oHv = P.A.take(N * P.hvn * w);
    P.oDesc = P.A.take(N * desc_bytes), P.oQ = P.A.take(N * D * D * w), P.oZs = P.A.take(N * D * D * w);
    P.oVal = P.A.take(mcs * w), P.oC = P.A.take(mcs * D * w), P.oS = P.A.take(mcs * D * w);
    P.A.back_end = P.oHv, P.A.up_at = P.oDesc, P.A.up_end = P.oZs;
    return P;
}

}  // namespace affine
}  // namespace mrbf
