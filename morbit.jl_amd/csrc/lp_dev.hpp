// Device leaf functions of the direction solvers (sd_lp.hip, normal_lp.hip, ds_qp.hip): what all of them run in the same text.  Every
// thread of a workgroup of lp::THREADS calls them; none of them knows its caller.  Each solver states `THREADS == lp::THREADS`.
#pragma once
#include <hip/hip_runtime.h>

namespace mrbf {
namespace lp {

constexpr int THREADS = 256;

// out[i] = sum_{j < n} f(i, j) for rows i < rows: THREADS / rows strided segments per row, their partial sums added in order
template <class F>
__device__ void row_pass(int n, int rows, F f, double *part, double *out) {
    const int t = threadIdx.x, S = THREADS / rows;
    if (t < rows * S) {
        const int i = t / S, s = t % S;
        double acc = 0.0;
        for (int j = s; j < n; j += S) acc += f(i, j);
        part[t] = acc;
    }
    __syncthreads();
    if (t < rows) {
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc += part[t * S + s];
        out[t] = acc;
    }
    __syncthreads();
}

// M^-1 from scratch: Gauss-Jordan with partial pivoting on [M | I] (sz x 2 sz in aug, filled and published by the caller).  rowbuf: 2 sz
// doubles, fac and cmax: sz each, flag: one word of LDS.  false: M is singular.
__device__ inline bool invert(int sz, double *aug, double *Minv, double *rowbuf, double *fac, double *cmax, int *flag) {
    const int t = threadIdx.x, W = 2 * sz;
    for (int c = t; c < sz; c += THREADS) {
        double mx = 0.0;
        for (int r = 0; r < sz; ++r) mx = fmax(mx, fabs(aug[r * W + c]));
        cmax[c] = mx;
    }
    __syncthreads();
    for (int c = 0; c < sz; ++c) {
        if (t == 0) {
            int r = c;
            double best = fabs(aug[c * W + c]);
            for (int i = c + 1; i < sz; ++i)
                if (fabs(aug[i * W + c]) > best) best = fabs(aug[i * W + c]), r = i;
            *flag = (best > 1e-14 * cmax[c] && best > 0.0) ? r : -1;
        }
        __syncthreads();
        const int r = *flag;
        if (r < 0) return false;  // uniform: every thread read the same word
        const double inv = 1.0 / aug[r * W + c];
        for (int e = t; e < W; e += THREADS) rowbuf[e] = aug[r * W + e] * inv;
        for (int i = t; i < sz; i += THREADS) fac[i] = aug[i * W + c];
        __syncthreads();
        if (r != c)
            for (int e = t; e < W; e += THREADS) aug[r * W + e] = aug[c * W + e];  // row c moves to r (row r is in rowbuf)
        __syncthreads();
        if (r != c && t == 0) fac[r] = fac[c];
        __syncthreads();
        for (int e = t; e < sz * W; e += THREADS) {
            const int i = e / W, cc = e % W;
            aug[e] = i == c ? rowbuf[cc] : aug[e] - fac[i] * rowbuf[cc];
        }
        __syncthreads();
    }
    for (int e = t; e < sz * sz; e += THREADS) Minv[e] = aug[(e / sz) * W + sz + e % sz];  // Minv[v * sz + p]: column slot v, row slot p
    __syncthreads();
    return true;
}

}  // namespace lp
}  // namespace mrbf
