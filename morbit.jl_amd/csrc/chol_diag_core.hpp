// Device core of the 128 x 128 diagonal-block factorisation (Cholesky + inverse of the factor), shared by the
// stand-alone kernel (chol_diag.hip), the persistent factorisation kernel (chol_mega.hip) and the one-launch small fit (small.hip).
//
// The block is cut into 16 x 16 tiles (36 lower tiles).  Every tile lives TRANSPOSED in the f64 MFMA C/D register
// layout of one of the 4 waves (lane l, register r hold A[16i + (l&15)][16j + (l>>4) + 4r]): in that layout a tile
// is directly the B operand of the next MFMA (its register r IS k-slice r), so the panel solve
//        P_i' = inv(L_bb) * A_ib'                (4 MFMAs per tile, A operand = the 16 x 16 leaf inverse from LDS)
// and the trailing update
//        A_ij' -= P_j * P_i'                     (4 MFMAs per tile, operands = finished panel tiles from LDS)
// never move data between lanes.  Only the 16 x 16 leaves are sequential: wave 0 factors them one column at a time
// with the rows of the leaf in lanes 0..15 and an identity block in lanes 16..31 (the same elimination turns the
// identity into L_bb^-T, i.e. the leaf inverse is free); columns are broadcast with v_readlane, no LDS, no barrier.
// After the 8 panels the full 128 x 128 inverse is assembled block column by block column with MFMAs
//        X_jj = inv(L_jj),   X_ij = -inv(L_ii) * sum_{p=j..i-1} L_ip X_pj.
#pragma once
#include "common.hpp"

namespace mrbf {
namespace diagcore {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) double gf64;  // explicit global address space: global_ (not flat_) loads / stores

constexpr int DNB = 128;
constexpr int NT = 8;      // 16 x 16 tiles per side
constexpr int TILE = 256;  // doubles per tile
constexpr int ITLD = 17;   // row stride of a leaf inverse in LDS: the leaf wave writes rows, the panel waves read columns, both conflict-free
constexpr int ITS = 16 * ITLD;
// strictly-lower tile (i, j), j < i
#define MRBF_SIDX(i, j) ((i) * ((i)-1) / 2 + (j))
// lower tile incl. diagonal (register ownership map)
#define MRBF_TIDX(i, j) ((i) * ((i) + 1) / 2 + (j))

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// v_rsq_f64 is good to ~2^-26 relative; one Newton step leaves ~1.5 * 2^-52 (under 2 ulp), two reach the last bit.  The pivot's
// reciprocal square root sits on the sequential chain of the whole factorisation (128 dependent leaf columns per block): the
// second step costs ~3 dependent f64 operations per column there and buys less than the rounding of the updates that follow
// (a 2-ulp perturbation of one pivot is a backward error of 2 ulp in that diagonal entry).  MRBF_DIAG_NEWTON=2 restores it.
#ifndef MRBF_DIAG_NEWTON
#define MRBF_DIAG_NEWTON 1
#endif
__device__ __forceinline__ double fast_rsqrt_v4(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
#pragma unroll
    for (int it = 0; it < MRBF_DIAG_NEWTON; ++it) y = y * fma(-h, y * y, 1.5);
    return y;
}

// operand fetch: element [4s + (l>>4)][l&15] of a 16 x 16 tile stored row-major ([k][c]); conflict-free ds_read_b64
__device__ __forceinline__ double opnd(const double *tile, int s, int l15, int l4) { return tile[(4 * s + l4) * 16 + l15]; }

// SC1: write-through stores (visible to other workgroups of the same launch after a flag hand-off)
template <bool SC1>
__device__ __forceinline__ void gstore(double *p, double v) {
    if constexpr (SC1)
        __hip_atomic_store((gf64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *(gf64 *)p = v;
}

// leaf: rows of the 16 x 16 s.p.d. block in lanes 0..15 (a[c], c <= lane valid), identity rows in lanes 16..31
template <int K>
__device__ __forceinline__ void leaf_step(double (&a)[16], int &bad, int col0) {
    // branch-free so that the 16 unrolled steps form one basic block: the scheduler can then start step K+1's
    // pivot -> rsqrt chain under the remaining column updates of step K
    // The pivot test stays off the pivot -> rsqrt -> scale chain: a non-positive pivot just lets NaNs through this block (every
    // later test then fails too, the first failure is the one recorded) and the caller aborts on the flag.
    const double piv = readlane_f64(a[K], K);
    const double rinv = fast_rsqrt_v4(piv);
    bad = (!(piv > 0.0) && bad == 0) ? col0 + K + 1 : bad;
    a[K] *= rinv;
#pragma unroll
    for (int j = K + 1; j < 16; ++j) {
        const double ljk = readlane_f64(a[K], j);
        a[j] = fma(-a[K], ljk, a[j]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// The core (v6 of the round notes): ONE workgroup barrier per 16-column panel, M_b, and the leaf wave on a short leash.
//
// The leaf wave (wave 0) only ever holds three tiles -- D_b = (b,b), S_b = (b+1,b), D_{b+1} -- and computes what its next leaf
// needs itself:
//     leaf(D_b) | barrier M_b | take S_b, D_{b+1} over from their owners (through LDS; they carry the panels <= b-2), apply
//     panel b-1 to both, S_b <- inv(L_bb) S_b = L(b+1,b), D_{b+1} -= L(b+1,b) L(b+1,b)' from registers, next leaf.
// The update waves (1..3) own every other tile; between M_b and M_{b+1} they apply panel b-1 to their tiles (column b first),
// solve column b's panel tiles (i >= b+2) with the leaf inverse, hand (b+2,b+1) and (b+2,b+2) over, store.  Whatever the leaf
// wave needs from them is one panel old, so it never waits for this step's work: ~3.2 us per panel, 26 us per block.  (With
// all eight diagonal tiles in the leaf wave and two barriers per panel -- leaf inverse visible, panel tiles visible -- the leaf
// wave spent 1.8 us in the leaf and 2.8 us around it: 40 us per block.)
//
// diag_v6_core factors the 128 x 128 block at A (lower part, column-major, leading dimension lda) in place and writes the inverse
// of the factor to Linv (128 x 128 column-major, zeros above the diagonal).  256 threads; the caller hands the block in registers
// (diag_v6_load).  Returns 0 or the 1-based index (inside the block) of the first non-positive pivot; in that case A / Linv are
// only partly written.  Every store of L and inv(L) is write-through.  The 16 x 16 leaf inverses also go to itg (8 x 256 doubles of
// global memory, [b][k][j] = inv(L_bb)[j][k]) and *prog counts the 16-column panels whose entries of L (and leaf inverse) are
// visible to other workgroups -- a consumer can run the panel solve of the tiles below in step.  The leaf inverses stay in LDS for
// two panels only and the final inverse is assembled from itg, which makes room for the double-buffered hand-over tiles.  Used by
// the stand-alone launch (chol_diag.hip), the persistent factorisation (chol_mega.hip) and the one-launch small fit (small.hip).
__host__ __device__ constexpr bool v6_leafwave(int i, int j) { return i <= 1; }  // (0,0), (1,0), (1,1) start in the leaf wave
__host__ __device__ constexpr int v6_index(int i, int j) { return MRBF_TIDX(i, j) - 3; }  // the other 33 lower tiles, row-major
__host__ __device__ constexpr int v6_owner(int i, int j) { return v6_leafwave(i, j) ? 0 : 1 + v6_index(i, j) % 3; }
__host__ __device__ constexpr int v6_slot(int i, int j) { return v6_leafwave(i, j) ? MRBF_TIDX(i, j) : v6_index(i, j) / 3; }
constexpr int NSLOT6 = 11;

struct DiagV6Shared {
    double LT[28 * TILE];  // strictly-lower tiles, [tile][c][row] (c = column inside the tile: MFMA operand order): final L -- or, before
                           // that, the raw tile handed to the leaf wave
    double IT[2 * ITS];    // leaf inverses of the current and the previous panel, transposed: IT[b & 1][a2 * ITLD + a] = inv(L_bb)[a][a2]
    double Dt[2 * TILE];   // leaf hand-over: [col][32 rows], rows 16..31 the identity (written once): the leaf wave's 32 lanes load their
                           // rows of [A_bb ; I] with one unconditional read per column
    double Lb[2 * TILE];   // factored leaves (double-buffered: the storing wave reads one while the next is written)
    double DH[2 * TILE];   // diagonal tiles on their way to the leaf wave (double-buffered)
    int bad[2];            // failure word of leaf b in slot b & 1: the leaf wave may write leaf b + 1's word before a slower wave has
                           // read leaf b's behind M_b -- with one word that wave would leave the loop one barrier early
};

__device__ __forceinline__ void diag_v6_load(const double *__restrict__ A, int64_t lda, v4d (&acc)[NSLOT6]) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            if (v6_owner(i, j) == wave) {
                v4d v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = *(const gf64 *)&A[(16 * i + l15) + (int64_t)(16 * j + l4 + 4 * r) * lda];
                acc[v6_slot(i, j)] = v;
            }
        }
}

// tile (i,j) -= L(i,p) L(j,p)' with both operands from LT
__device__ __forceinline__ void v6_update(v4d &c, const double *LT, int i, int j, int p, int l15, int l4) {
    const double *ti_ = &LT[MRBF_SIDX(i, p) * TILE];
    const double *tj_ = &LT[MRBF_SIDX(j, p) * TILE];
#pragma unroll
    for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f64_16x16x4f64(-opnd(tj_, s, l15, l4), opnd(ti_, s, l15, l4), c, 0, 0, 0);
}

__device__ __forceinline__ int diag_v6_core(double *__restrict__ A, int64_t lda, double *__restrict__ Linv, DiagV6Shared &sh,
                                            v4d (&acc)[NSLOT6], double *__restrict__ itg, unsigned *prog,
                                            unsigned long long *pubstamp = nullptr) {
    const int tid = threadIdx.x, lane_ = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // No barrier on entry: the leaf wave prepares what only it uses (failure word, identity rows) and starts the first leaf while the
    // other waves may still be folding the caller's last panel into their tiles; they meet at M_0.  (The caller's LDS use ended
    // behind a barrier.)
    if (wave == 0) {
        if (tid == 0) sh.bad[0] = sh.bad[1] = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = lane_ + 64 * u;
            sh.Dt[(e >> 4) * 32 + 16 + (e & 15)] = ((e >> 4) == (e & 15)) ? 1.0 : 0.0;
        }
    }
    v4d Dc = acc[0], Sc = acc[1], Dn = acc[2];  // leaf wave: (0,0), (1,0), (1,1)

#pragma unroll 1
    for (int b = 0; b < NT; ++b) {
        int lane = lane_;
        asm volatile("" : "+v"(lane));  // nothing derived from the lane index is hoisted out of the loop (and spilled)
        const int l15 = lane & 15, l4 = lane >> 4;
        const int bb = b & 1;
        if (wave == 0) {
            // ---- leaf b
#pragma unroll
            for (int r = 0; r < 4; ++r) sh.Dt[(l4 + 4 * r) * 32 + l15] = Dc[r];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            double a[16];
            int bad = 0;
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = sh.Dt[c * 32 + (lane & 31)];
            leaf_step<0>(a, bad, 16 * b);
            leaf_step<1>(a, bad, 16 * b);
            leaf_step<2>(a, bad, 16 * b);
            leaf_step<3>(a, bad, 16 * b);
            leaf_step<4>(a, bad, 16 * b);
            leaf_step<5>(a, bad, 16 * b);
            leaf_step<6>(a, bad, 16 * b);
            leaf_step<7>(a, bad, 16 * b);
            leaf_step<8>(a, bad, 16 * b);
            leaf_step<9>(a, bad, 16 * b);
            leaf_step<10>(a, bad, 16 * b);
            leaf_step<11>(a, bad, 16 * b);
            leaf_step<12>(a, bad, 16 * b);
            leaf_step<13>(a, bad, 16 * b);
            leaf_step<14>(a, bad, 16 * b);
            leaf_step<15>(a, bad, 16 * b);
            if (bad && lane == 0) sh.bad[bb] = bad;
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; ++c) sh.Lb[bb * TILE + c * 16 + lane] = a[c];
            } else if (lane < 32) {
                const int r = lane - 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) sh.IT[bb * ITS + r * ITLD + c] = (c >= r) ? a[c] : 0.0;
            }
        }
        // every wave: its write-through stores of the previous panel (L tiles, leaf, inverse) are out before the panel is published
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // M_b
        if (sh.bad[bb]) break;
        if (b > 0 && tid == 64)
            __hip_atomic_store((__attribute__((address_space(1))) unsigned *)prog, (unsigned)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wave == 0) {
            if (b < NT - 1) {
                if (b > 0) {
                    // take (b+1,b) and (b+1,b+1) over (they carry the panels <= b-2) and apply panel b-1
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        Sc[r] = sh.LT[MRBF_SIDX(b + 1, b) * TILE + (l4 + 4 * r) * 16 + l15];
                        Dn[r] = sh.DH[((b - 1) & 1) * TILE + (l4 + 4 * r) * 16 + l15];
                    }
                    v6_update(Sc, sh.LT, b + 1, b, b - 1, l15, l4);
                    v6_update(Dn, sh.LT, b + 1, b + 1, b - 1, l15, l4);
                }
                // L(b+1,b) = tile * inv(L_bb)'  (transposed layout: P' = inv(L_bb) * tile')
                const double *itb = &sh.IT[bb * ITS];
                v4d p = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 4; ++s) p = __builtin_amdgcn_mfma_f64_16x16x4f64(itb[(4 * s + l4) * ITLD + l15], Sc[s], p, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sh.LT[MRBF_SIDX(b + 1, b) * TILE + (l4 + 4 * r) * 16 + l15] = p[r];
                    gstore<true>(&A[(16 * (b + 1) + l15) + (int64_t)(16 * b + l4 + 4 * r) * lda], p[r]);
                }
                // next diagonal tile -= L(b+1,b) L(b+1,b)': both operands are the registers just computed
#pragma unroll
                for (int s = 0; s < 4; ++s) Dn = __builtin_amdgcn_mfma_f64_16x16x4f64(-p[s], p[s], Dn, 0, 0, 0);
                Dc = Dn;
            }
        } else {
            // ---- update waves, phase b
            if (wave == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = l4 + 4 * r;
                    if (c <= l15) gstore<true>(&A[(16 * b + l15) + (int64_t)(16 * b + c) * lda], sh.Lb[bb * TILE + c * 16 + l15]);
                }
            } else if (wave == 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) gstore<true>(&itg[b * TILE + (l4 + 4 * r) * 16 + l15], sh.IT[bb * ITS + (l4 + 4 * r) * ITLD + l15]);
            }
            // panel b-1 on this wave's tiles of block column b, then their panel solve
            const double *itb = &sh.IT[bb * ITS];
            double ia[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) ia[s] = itb[(4 * s + l4) * ITLD + l15];
#pragma unroll
            for (int i = 2; i < NT; ++i)
#pragma unroll
                for (int j = 0; j <= i - 2; ++j) {
                    if (j == b && v6_owner(i, j) == wave) {
                        v4d m = acc[v6_slot(i, j)];
                        if (b > 0) v6_update(m, sh.LT, i, j, b - 1, l15, l4);
                        v4d p = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int s = 0; s < 4; ++s) p = __builtin_amdgcn_mfma_f64_16x16x4f64(ia[s], m[s], p, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            sh.LT[MRBF_SIDX(i, j) * TILE + (l4 + 4 * r) * 16 + l15] = p[r];
                            gstore<true>(&A[(16 * i + l15) + (int64_t)(16 * j + l4 + 4 * r) * lda], p[r]);
                        }
                    }
                }
            // panel b-1 on the two tiles the leaf wave takes over after the next barrier, and their hand-over
#pragma unroll
            for (int i = 2; i < NT; ++i) {
                if (i == b + 2) {
                    if (v6_owner(i, i - 1) == wave) {  // (b+2, b+1)
                        v4d m = acc[v6_slot(i, i - 1)];
                        if (b > 0) v6_update(m, sh.LT, i, i - 1, b - 1, l15, l4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) sh.LT[MRBF_SIDX(i, i - 1) * TILE + (l4 + 4 * r) * 16 + l15] = m[r];
                    }
                    if (v6_owner(i, i) == wave) {  // (b+2, b+2)
                        v4d m = acc[v6_slot(i, i)];
                        if (b > 0) v6_update(m, sh.LT, i, i, b - 1, l15, l4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) sh.DH[bb * TILE + (l4 + 4 * r) * 16 + l15] = m[r];
                    }
                }
            }
            // panel b-1 on everything else this wave still owns: tiles (i,j) with j >= b+1 that are not on their way to the leaf wave
            if (b > 0) {
#pragma unroll
                for (int i = 3; i < NT; ++i)
#pragma unroll
                    for (int j = 1; j <= i; ++j) {
                        if (j >= b + 1 && i >= b + 3 && v6_owner(i, j) == wave) v6_update(acc[v6_slot(i, j)], sh.LT, i, j, b - 1, l15, l4);
                    }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int lane = lane_, l15 = lane & 15, l4 = lane >> 4;
    const int bad_all = sh.bad[0] ? (sh.bad[1] && sh.bad[1] < sh.bad[0] ? sh.bad[1] : sh.bad[0]) : sh.bad[1];
    if (bad_all) return bad_all;
    if (tid == 64) {
        __hip_atomic_store((__attribute__((address_space(1))) unsigned *)prog, (unsigned)NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pubstamp) *pubstamp = wall_clock64();  // all eight panels published (diagnostic launches)
    }
    // ---- inverse: wave w assembles block columns w and 7 - w of X = L^-1 in registers (MFMA C/D layout), zeros above the diagonal
    //      included (the panel GEMM reads the full 128 x 128 inverse); the leaf inverses are read back from itg (this workgroup's
    //      own write-through stores, drained above)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = half == 0 ? wave : 7 - wave;
        v4d X[NT];
#pragma unroll
        for (int r = 0; r < 4; ++r) X[0][r] = *(const gf64 *)&itg[j * TILE + l15 * 16 + l4 + 4 * r];
#pragma unroll
        for (int r = 0; r < 4; ++r) gstore<true>(&Linv[(16 * j + l4 + 4 * r) + (16 * j + l15) * DNB], X[0][r]);
#pragma unroll
        for (int di = 1; di < NT; ++di) {
            const int i = j + di;
            if (i < NT) {
                v4d S = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int dp = 0; dp < di; ++dp) {
                    const int p = j + dp;
                    const double *lt = &sh.LT[MRBF_SIDX(i, p) * TILE];
#pragma unroll
                    for (int s = 0; s < 4; ++s) S = __builtin_amdgcn_mfma_f64_16x16x4f64(opnd(lt, s, l15, l4), X[dp][s], S, 0, 0, 0);
                }
                v4d Xi = {0.0, 0.0, 0.0, 0.0};
                const double *iti = itg + i * TILE;
#pragma unroll
                for (int s = 0; s < 4; ++s) Xi = __builtin_amdgcn_mfma_f64_16x16x4f64(-*(const gf64 *)&iti[(4 * s + l4) * 16 + l15], S[s], Xi, 0, 0, 0);
                X[di] = Xi;
#pragma unroll
                for (int r = 0; r < 4; ++r) gstore<true>(&Linv[(16 * i + l4 + 4 * r) + (16 * j + l15) * DNB], Xi[r]);
            }
        }
        for (int e = lane; e < 16 * j * 16; e += 64) {
            const int row = e % (16 * j), col = e / (16 * j);
            gstore<true>(&Linv[row + (16 * j + col) * DNB], 0.0);
        }
    }
    return 0;
}

}  // namespace diagcore
}  // namespace mrbf
