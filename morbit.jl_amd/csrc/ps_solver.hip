// Pascoletti-Serafini descent step with the whole subproblem solver on the device -- replaces the NLopt runs of
// compute_local_ideal_point / _ps_optimization inside get_criticality(::PascolettiSerafiniConfig, ...)
// (Morbit.jl src/descent.jl:369-412, :434-510, :512-581).
//
// The reference hands one-point closures to NLopt's GN_ISRES: every candidate costs one sweep over all n centres PER OUTPUT.
// Here the subproblems are solved by an ISRES-style (mu, lambda) evolution strategy (Runarsson & Yao; population 20 (dim + 1),
// mu = lambda / 7, as NLopt's defaults) whose state lives in device memory:
//   * the k single-objective runs of the local ideal point and the Pascoletti-Serafini run each own a population block; all
//     blocks of a generation are evaluated by ONE batched surrogate sweep per grouped model (eval_model, values only);
//   * per generation three more launches do everything else, for all runs at once:
//       ps_score_kernel  one wave per individual: objective and constraint violation -- the PS constraints of descent.jl:443,
//                        the modelled (in)equality constraints (:448-466) and the MOP's linear constraints
//                        (AbstractMOPInterface.jl:487-495) -- into per-run arrays;
//       ps_rank_kernel   one 1024-thread workgroup per run: best so far, stop tests, stochastic ranking with the records in LDS
//                        (odd-even transposition with the random comparison rule -- the parallel form of the bubble sweeps --
//                        or, when no individual violates a constraint, a bitonic network that ends in the same order);
//       ps_breed_kernel  one wave per offspring: differential variation, log-normal self-adaptive mutation with re-draws inside
//                        the box, from a counter-based generator (Philox 4x32-10, keyed by seed / run / generation / individual /
//                        component: no state, any launch order);
//   * the host enqueues generations back to back and reads the runs' status words every few generations only.
// Populations up to MAXLAM individuals (d <= 356): the C4 / C5 dimensions of BASELINE.json (d = 128, 256; examples/example_zdt.jl:39)
// run here, not in a host loop.
// Parity with the reference is the contract of get_criticality (problem solved, budgets, start values, critical / failure
// short cuts, returned tuple), not NLopt's random trajectory; the returned point is always feasible for the subproblem.
// Many starts of one problem -- the reference's Threads.@threads loop over starts, examples/large_scale_benchmarks.jl:102-109, with
// descent_method = :ps -- take the same kernels in ONE call (mrbf_ps_step_batch): every start has its block (ps::Args: runs, box,
// x_n, m(x_n), r, seed, result blocks) in device memory, the start is a grid dimension, a generation of all starts is one sweep per
// launch group (batch_chain.hpp), one ranking and one breeding launch, and the refinements advance in lockstep.  The single call is
// the batch of one (ps_open, ps_ideal_phase, ps_step_phase, ps_close over one PsCall).  DESIGN.md section 15.  The host arithmetic
// -- limits, sizes, budgets, the refinement's state machine -- is ps_host.hpp's.
#include "batch_chain.hpp"
#include "ideal_host.hpp"
#include "ps_host.hpp"
#include "radial.hpp"

namespace mrbf {

namespace ps {

// (MAXLAM, MAXRUNS, MAXMODELS, MAXOBJ, MAXCON: ps_host.hpp)
constexpr int RANK_THREADS = 1024;
// ranking of a large population on several compute units (ps_rank_wave_kernel): phases between two no-swap tests (the exit-rule
// period), smallest population that takes this path, compute units the device must have per run for it (the waves of a run wait for
// each other, so they have to be resident together)
constexpr int RS_B = 256, RS_MINLAM = 1024, RS_CUS_PER_RUN = 16;
constexpr int RS_SYNC = 64;  // sync words per run: [0] arrivals, [1] failure, [2] the run asks for the phases (1) / the counted sort (2), [3] free, [4 + c] chunk c moved something

struct RankWs {  // device work space of the several-compute-unit ranking, run r OF THE LAUNCH (Args::grun0 + the start's own run index) at offset r * MAXLAM (r * RS_SYNC)
    double *f[2];  // ps_rank_wave_kernel's two exchange buffers (64-bit records)
    int *idx;      // the order it found, for the finishing launch
    int *sync;
    int *cnt;      // its keys: per run MAXLAM counts for f, MAXLAM for phi
    int *sticky;   // one word behind the runs' sync words: a wait of ps_rank_wave_kernel timed out (the host stops using that kernel)
};

struct Run {  // one (mu, lambda) run; all pointers into device arenas
    int nvar;       // 1 + d for the PS run (chi = [t; x]), d for an ideal-point run
    int lam, mu;
    int kind;       // 0: minimise objective `obj` over the box; 1: Pascoletti-Serafini run
    int obj;
    int off;        // first row of this run's block in the evaluation batch
    int max_evals;
    double *X[2];   // lam x nvar, ping-pong
    double *S[2];   // lam x nvar step sizes
    double *best;   // nvar + 2: best_x, best_f, best_phi
    double *f, *phi;  // lam: objective / violation of the current generation
    int *order;     // lam: ranked individuals (best first); the first mu are the parents
    int *stat;      // [0] evals so far, [1] done, [2] generations run, [3] generation + 1 whose offspring are to be bred
};

// One start's block.  The blocks of a launch's starts lie side by side in device memory and every kernel takes the start from a grid
// dimension (mrbf_ps_step_problem: one block; mrbf_ps_step_batch: one per start that takes part in the phase).  A run's index -- the
// generator's key beside the start's own seed -- is its index within its start.
struct Args {
    Run runs[MAXRUNS];
    int nruns, d, nobj, rows;
    const double *lb, *ub;   // d
    const double *mx, *r;    // nobj (PS run)
    const double *xn;        // d: the start point of generation 0
    double t0;               //    and of t (PS run)
    int grun0;               // the launch-wide index of this start's first run (RankWs)
    // evaluation batch results: one rows x kf[j] block per grouped model
    const double *F[MAXMODELS];
    int kf[MAXMODELS];
    int nmodels;
    short obj_model[MAXOBJ], obj_col[MAXOBJ];   // where objective l lives
    int ncon;                                   // modelled constraints: (model, column, 1 = equality)
    short con_model[MAXCON], con_col[MAXCON], con_eq[MAXCON];
    int nlin_eq, nlin_ineq;                     // A x = b, A x <= b in scaled variables (row-major rows x d)
    const double *A_eq, *b_eq, *A_ineq, *b_ineq;
    double eq_tol;
    double *Xeval;           // evaluation batch, rows x d
    int score_fused;         // no linear constraints: ps_rank_kernel scores its own run's individuals (no ps_score_kernel launch)
    double *Xq, *xsq;        // non-null: the breeding kernel also writes the batch centred and padded (rows x xqD, squared norms) for the one model
    const double *xmean;     //           whose evaluation reads it (the arithmetic of center_pad_kernel, prep.hip)
    int xqD;
    unsigned long long seed;
    double xtol_rel;
    int dbg;  // Dbg bits (MRBF_PS_DBG, mrbf_debug_ps_rank)
};
// Args::dbg: each bit makes a population take a live path that its size or its values would not take by default, so that the tests
// can put the same generation through both and compare
enum Dbg : int {
    DBG_PHASES = 4,          // transposition phases also when no individual violates anything (default: the plain sort / the counted sort)
    DBG_GIVE_UP = 64,        // ps_rank_wave_kernel gives up at once, as after a counter time-out: the finishing launch runs the phases itself
    DBG_SORT_PAIRS = 128,    // plain sort as one pair per thread through LDS (default: a run much smaller than the launch's largest)
    DBG_NO_SELECT = 256,     // plain sort of the whole population (default below 8 elements per thread: no parent selection)
    DBG_SELECT = 512,        // parent selection also below 8 elements per thread
    DBG_PHASE_PAIRS = 2048,  // populations below RS_MINLAM: phases as one pair per thread through LDS (default: a generation with a NaN, the larger populations' fallback)
    DBG_ALL = DBG_PHASES | DBG_GIVE_UP | DBG_SORT_PAIRS | DBG_NO_SELECT | DBG_SELECT | DBG_PHASE_PAIRS
};

// ---- Philox 4x32-10 ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0;
        c[1] = n1;
        c[2] = n2;
        c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// two uniforms in (0,1) and two standard normals for (run, generation, individual, component, draw)
__device__ __forceinline__ void rng4(const Args &a, int run, int gen, int ind, int comp, int draw, double &u0, double &u1, double &z0, double &z1) {
    unsigned c[4] = {(unsigned)ind, (unsigned)comp, (unsigned)(gen * 16 + draw), (unsigned)run};
    philox(c, (unsigned)a.seed, (unsigned)(a.seed >> 32));
    u0 = ((double)c[0] + 0.5) * (1.0 / 4294967296.0);
    u1 = ((double)c[1] + 0.5) * (1.0 / 4294967296.0);
    // Box-Muller in single precision (hardware log / sin / cos): the draws only steer a random search
    const float v0 = ((float)(c[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), v1 = ((float)(c[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = __fsqrt_rn(-2.0f * __logf(v0));
    z0 = (double)(rad * __cosf(6.2831853f * v1));
    z1 = (double)(rad * __sinf(6.2831853f * v1));
}

__device__ __forceinline__ double lo_of(const Args &a, const Run &R, int j) { return R.kind == 1 ? (j == 0 ? -1.0 : a.lb[j - 1]) : a.lb[j]; }
__device__ __forceinline__ double hi_of(const Args &a, const Run &R, int j) { return R.kind == 1 ? (j == 0 ? 0.0 : a.ub[j - 1]) : a.ub[j]; }
__device__ __forceinline__ int run_of_row(const Args &a, int row) {  // runs are laid out in row order
    int run = 0;
    while (run + 1 < a.nruns && row >= a.runs[run + 1].off) ++run;
    return run;
}

// generation 0: uniform population in the box, individual 0 = the start point (PS: [t0; x_n]), PS individual 1 = [0; x_n]
// (feasible for the PS constraints: m(x_n) - m(x_n) - 0 r = 0); step sizes (ub - lb) / sqrt(n)
__global__ __launch_bounds__(256) void ps_init_kernel(const Args *__restrict__ A) {
    const Args &a = A[blockIdx.z];
    const double *xn = a.xn;
    const double t0 = a.t0;
    const Run &R = a.runs[blockIdx.y];
    const int n = R.nvar;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < R.lam * n) {
        const int i = e / n, j = e % n;
        const double lo = lo_of(a, R, j), hi = hi_of(a, R, j);
        double u0, u1, z0, z1;
        rng4(a, blockIdx.y, 0, i, j, 15, u0, u1, z0, z1);
        double v = lo + u0 * (hi - lo);
        double step = (hi - lo) / sqrt((double)n);
        if (i == 0 || (i == 1 && R.kind == 1)) {
            v = (R.kind == 1) ? (j == 0 ? (i == 0 ? t0 : 0.0) : xn[j - 1]) : xn[j];
            v = fmin(fmax(v, lo), hi);
        } else if (i & 1) {
            // every second individual is a mutation of the start point with a scale from 1/4 of the box down to 2^-11 of it (NLopt's
            // ISRES starts its whole population at x0 too): at d >= 64 a uniform population holds no point that improves every
            // objective at once, i.e. no feasible chi with t < 0, and the run ended where it began (omega = 0 at d = 64 .. 256)
            const double sigma = 0.25 * exp2(-(double)(((i >> 1) - 1) % 10));
            const double xs = (R.kind == 1) ? (j == 0 ? 0.0 : xn[j - 1]) : xn[j];
            v = (R.kind == 1 && j == 0) ? 0.0 : fmin(fmax(xs + sigma * z0 * (hi - lo), lo), hi);
            step *= sigma;
        }
        R.X[0][e] = v;
        R.S[0][e] = step;
        const int skip = R.kind == 1 ? 1 : 0;  // the evaluation batch holds the x part of every individual of every run
        if (j >= skip) a.Xeval[(size_t)(R.off + i) * a.d + (j - skip)] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        R.best[n] = INFINITY;
        R.best[n + 1] = INFINITY;
        R.stat[0] = 0;
        R.stat[1] = 0;
        R.stat[2] = 0;
        R.stat[3] = 0;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- objective and constraint violation of individual i (row `row` of the evaluation batch) of run R.  WAVE: the 64 lanes of a wave
// work on the row together (the linear constraints' dot products are summed over the lanes); otherwise one thread does the row --
// problems without linear constraints only (ps_rank_kernel scores its own run that way: a launch per generation less).
template <bool WAVE>
__device__ __forceinline__ void score_row(const Args &a, int gen, const Run &R, int i, int row, int lane, double &f_out, double &phi_out) {
    const int m = min(R.lam, R.max_evals - R.stat[0]);  // individuals of this generation inside the budget
    double f = INFINITY, phi = INFINITY;
    if (i < m) {
        if (R.kind == 0) {
            f = a.F[a.obj_model[R.obj]][(size_t)row * a.kf[a.obj_model[R.obj]] + a.obj_col[R.obj]];
            phi = 0.0;
        } else {
            double t = R.X[gen & 1][(size_t)i * R.nvar];
            // the subproblem is min_x max_l (m_l(x) - m_l(x_n)) / r_l in disguise: the best t an x admits is known once x has been
            // evaluated, so the individual carries THAT t (pulled a hair towards 0 so that rounding cannot make it infeasible);
            // an x that worsens some objective keeps t = 0 and is ranked by its violation
            double ts = -INFINITY;
            for (int l = 0; l < a.nobj; ++l)
                ts = fmax(ts, (a.F[a.obj_model[l]][(size_t)row * a.kf[a.obj_model[l]] + a.obj_col[l]] - a.mx[l]) / a.r[l]);
            if (ts == ts) {
                t = ts <= 0.0 ? fmax(ts * (1.0 - 1e-14), -1.0) : 0.0;
                if (lane == 0) R.X[gen & 1][(size_t)i * R.nvar] = t;
            }
            f = t;
            phi = 0.0;
            for (int l = 0; l < a.nobj; ++l) {
                const double g = a.F[a.obj_model[l]][(size_t)row * a.kf[a.obj_model[l]] + a.obj_col[l]] - a.mx[l] - t * a.r[l];
                phi += g > 0.0 ? g * g : 0.0;  // m_l(x) - m_l(x_n) - t r_l <= 0  (descent.jl:443)
            }
        }
        for (int c = 0; c < a.ncon; ++c) {  // modelled constraints (descent.jl:448-466): h(x) = 0, g(x) <= 0
            const double v = a.F[a.con_model[c]][(size_t)row * a.kf[a.con_model[c]] + a.con_col[c]];
            if (a.con_eq[c])
                phi += fabs(v) > a.eq_tol ? v * v : (v == v ? 0.0 : INFINITY);
            else
                phi += v > 0.0 ? v * v : (v == v ? 0.0 : INFINITY);
        }
        if constexpr (WAVE) {
            const double *x = a.Xeval + (size_t)row * a.d;
            for (int c = 0; c < a.nlin_eq + a.nlin_ineq; ++c) {  // linear constraints of the MOP in scaled variables
                const bool eq = c < a.nlin_eq;
                const double *Ar = eq ? a.A_eq + (size_t)c * a.d : a.A_ineq + (size_t)(c - a.nlin_eq) * a.d;
                double s = 0.0;
                for (int j = lane; j < a.d; j += 64) s = fma(Ar[j], x[j], s);
                s = wave_sum(s) - (eq ? a.b_eq[c] : a.b_ineq[c - a.nlin_eq]);
                if (eq)
                    phi += fabs(s) > a.eq_tol ? s * s : (s == s ? 0.0 : INFINITY);
                else
                    phi += s > 0.0 ? s * s : (s == s ? 0.0 : INFINITY);
            }
        }
        if (!(f == f) || !(phi == phi) || fabs(f) == INFINITY || fabs(phi) == INFINITY) {
            f = INFINITY;
            phi = INFINITY;
        }
    }
    f_out = f;
    phi_out = phi;
}

// one wave per row of the evaluation batch (problems with linear constraints; without, ps_rank_kernel scores its run itself)
__global__ __launch_bounds__(256) void ps_score_kernel(const Args *__restrict__ A, int gen) {
    const Args &a = A[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int run = run_of_row(a, row);
    const Run &R = a.runs[run];
    if (R.stat[1]) return;  // finished earlier
    const int i = row - R.off;
    double f, phi;
    score_row<true>(a, gen, R, i, row, lane, f, phi);
    if (lane == 0) {
        R.f[i] = f;
        R.phi[i] = phi;
    }
}

// record order of the best-so-far bookkeeping: feasible beats infeasible, then the objective (feasible) or the violation
// (infeasible), ties by index
struct Cand {
    double key;  // f when feasible, phi otherwise
    int feas;    // 1 feasible, 0 infeasible, -1 none
    int idx;
};
__device__ __forceinline__ bool cand_better(const Cand &x, const Cand &y) {
    if (y.feas < 0) return x.feas >= 0;
    if (x.feas < 0) return false;
    if (x.feas != y.feas) return x.feas > y.feas;
    if (x.key != y.key) return x.key < y.key;
    return x.idx < y.idx;
}

// ---- the bitonic network of the plain sort with E elements per thread in registers (position p = tid * E + e): compare-exchanges at
// distance j < E stay inside the thread, j < 64 E go through wave shuffles, only the rest through LDS with a barrier -- 10 of the 78
// stages at N = 4096 (the one-pair-per-thread form paid an LDS round trip and a sixteen-wave barrier per stage: 60-80 us per generation at
// d = 128, 2.4 ms per step).  Same network, same comparator (objective, ties by index): the same order.  On return sidx[p] holds the order.
__device__ __forceinline__ int npow2(int lam) {
    int N = 1;
    while (N < lam) N <<= 1;
    return N;
}
template <int J, int E>
__device__ __forceinline__ void bitonic_inthread(double (&f)[E], int (&ix)[E], int base, int kk) {
#pragma unroll
    for (int e = 0; e < E; ++e)
        if ((e & J) == 0) {
            const int l = e | J;
            const bool greater = f[e] > f[l] || (f[e] == f[l] && ix[e] > ix[l]);
            const bool up = ((base + e) & kk) == 0;
            if (greater == up) {
                const double tf = f[e];
                f[e] = f[l];
                f[l] = tf;
                const int ti = ix[e];
                ix[e] = ix[l];
                ix[l] = ti;
            }
        }
}
template <int E>
__device__ __forceinline__ void bitonic_regs(const double *__restrict__ fin, const int *__restrict__ iin, int lam, int N, double *sf, int *sidx) {
    const int tid = threadIdx.x, base = tid * E;
    double f[E];
    int ix[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int p = base + e;
        f[e] = p < lam ? fin[p] : INFINITY;
        ix[e] = p < lam ? (iin ? iin[p] : p) : 0x7fffffff;
    }
    if (iin) __syncthreads();  // (the inputs may live where the stages exchange their elements)
    for (int kk = 2; kk <= N; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j < E) {
                if constexpr (E > 1) {
                    if (j == 1) bitonic_inthread<1, E>(f, ix, base, kk);
                }
                if constexpr (E > 2) {
                    if (j == 2) bitonic_inthread<2, E>(f, ix, base, kk);
                }
                if constexpr (E > 4) {
                    if (j == 4) bitonic_inthread<4, E>(f, ix, base, kk);
                }
            } else if (j < 64 * E) {
                const int dl = j / E;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int p = base + e;
                    const double of = __shfl_xor(f[e], dl);
                    const int oi = __shfl_xor(ix[e], dl);
                    const bool keep_min = ((p & j) == 0) == ((p & kk) == 0);
                    const bool greater = f[e] > of || (f[e] == of && ix[e] > oi);
                    if (keep_min == greater) {
                        f[e] = of;
                        ix[e] = oi;
                    }
                }
            } else {
                __syncthreads();  // (the partners' reads of the stage before)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    sf[base + e] = f[e];
                    sidx[base + e] = ix[e];
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int p = base + e, q = p ^ j;
                    const double of = sf[q];
                    const int oi = sidx[q];
                    const bool keep_min = ((p & j) == 0) == ((p & kk) == 0);
                    const bool greater = f[e] > of || (f[e] == of && ix[e] > oi);
                    if (keep_min == greater) {
                        f[e] = of;
                        ix[e] = oi;
                    }
                }
            }
        }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) sidx[base + e] = ix[e];
    __syncthreads();
}

// ---- only the mu best individuals of a plain sort are ever read (the parents, and the spread test over them): find them without sorting
// the other six sevenths.  A threshold from blockDim evenly spaced samples (each sample ranks itself among the samples by counting:
// no sort), placed three standard deviations of the sample quantile above rank mu; one pass counts and compacts the individuals at or
// below it (ties included, so the compacted set always CONTAINS the mu best with their index order intact); if that set holds at least mu
// and at most blockDim individuals it is padded to blockDim and sorted one element per thread (shuffles up to distance 32, LDS beyond:
// 10 barrier stages of 55) -- else the caller sorts everything as before.  The parents and their order are those of the full sort.
// scratch: 2 blockDim doubles + 2 blockDim ints behind `sf` (the caller's N >= 2 blockDim doubles + N ints cover it).
__device__ __forceinline__ bool select_parents(const double *__restrict__ fin, int lam, int mu, double *sf, int *sidx_out) {
    __shared__ int s_cnt[32];
    __shared__ double s_thr;
    const int tid = threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
    double *ssamp = sf, *csf = sf + NT;
    int *cidx = reinterpret_cast<int *>(sf + 2 * NT);
    // target rank: mu plus three standard deviations of the S-sample quantile estimate (in ranks)
    const int S = NT;
    const double p0 = (double)mu / lam;
    const double sd = lam * sqrt(fmax(p0 * (1.0 - p0), 0.0) / S);
    const double T = mu + 3.0 * sd + 2.0 * lam / S;
    if (!(T <= 0.9 * NT) || lam <= NT) return false;
    const int rstar = min(S - 1, (int)ceil(T * S / lam));
    const double mine = fin[(int)(((long long)tid * lam) / S)];
    ssamp[tid] = mine;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < S; ++q) {
        const double o = ssamp[q];  // (broadcast read)
        rank += (o < mine || (o == mine && q < tid)) ? 1 : 0;
    }
    if (rank == rstar) s_thr = mine;
    __syncthreads();
    const double thr = s_thr;
    int cnt = 0;
    for (int i = tid; i < lam; i += NT) cnt += fin[i] <= thr ? 1 : 0;
    // exclusive scan of the per-thread counts: inside the wave by shuffles, across the waves through LDS
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_cnt[wave] = incl;
    __syncthreads();
    int wbase = 0, total = 0;
    for (int w2 = 0; w2 < nw; ++w2) {
        if (w2 < wave) wbase += s_cnt[w2];
        total += s_cnt[w2];
    }
    if (total < mu || total > NT) return false;  // (uniform: every thread sees the same counts)
    int pos = wbase + incl - cnt;
    for (int i = tid; i < lam; i += NT) {
        const double v = fin[i];
        if (v <= thr) {
            csf[pos] = v;
            cidx[pos] = i;
            ++pos;
        }
    }
    for (int i = total + tid; i < NT; i += NT) {
        csf[i] = INFINITY;
        cidx[i] = 0x7fffffff;
    }
    __syncthreads();
    // (a thread's compacted elements are not in index order across threads -- thread t holds i = t, t + NT, .. -- which is fine: the
    // sort's comparator is (objective, index))
    bitonic_regs<1>(csf, cidx, NT, NT, ssamp, sidx_out);
    return true;
}

// ---- one workgroup per run: best so far, stop tests, ranking
// mode 0: everything in this launch.  Large populations with infeasible individuals (mode 1 / 2): mode 1 does the bookkeeping and, when
// the transposition phases are due, hands them to ps_rank_wave_kernel (one wave per 64 individuals); mode 2 picks the order up (or runs the
// phases here after all if that kernel gave up: it never touches f / phi) and finishes the generation.
constexpr int RW_OWN = 64, RW_H = 32;
constexpr int RW_CNT_T = 256;  // individuals per counting workgroup
__host__ __device__ inline int rw_waves(int lam) { return (lam + RW_OWN - 1) / RW_OWN; }
__host__ __device__ inline int rw_pitch(int lam) { return ((lam / 2 + RW_OWN + 63) / 64) * 64; }  // pair slots of a group, plus the last window's overhang
__host__ __device__ inline int rw_jsplit(int lam) { return lam > 2048 ? 32 : 8; }                 // the counting's split of the "other individual" loop

typedef unsigned long long u64;
// lane mask in a scalar register pair ? a : b
__device__ __forceinline__ unsigned msel(u64 m, unsigned a, unsigned b) {
    unsigned d;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(d) : "v"(b), "v"(a), "s"(m));
    return d;
}
// 16-bit compares of the two halves of a key, straight into a lane mask
__device__ __forceinline__ u64 gt_hi16(unsigned a, unsigned b) {
    u64 m;
    asm("v_cmp_gt_u16_sdwa %0, %1, %2 src0_sel:WORD_1 src1_sel:WORD_1" : "=s"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ u64 gt_lo16(unsigned a, unsigned b) {
    u64 m;
    asm("v_cmp_gt_u16_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ u64 zero_lo16(unsigned a) {
    u64 m;
    asm("v_cmp_eq_u16_e64 %0, 0, %1" : "=s"(m) : "v"(a));
    return m;
}
// (bound_ctrl: the lane without a source reads 0 -- its pair is masked off -- and the move needs no initialised destination)
__device__ __forceinline__ unsigned dpp_from_next(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); }  // wave_shl:1 -- lane l reads lane l + 1
__device__ __forceinline__ unsigned dpp_from_prev(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true); }  // wave_shr:1 -- lane l reads lane l - 1

// 4 NG phases on a window (KA / KB the keys, IA / IB the individuals of this lane's two positions).  TAIL: the ranking's last, short
// block -- phases from nph on do nothing.
template <bool TAIL, int NG>
__device__ __forceinline__ void rw_block(unsigned &KA, unsigned &KB, unsigned &IA, unsigned &IB, u64 dbits, int nph, u64 mPairE, u64 mPairO, u64 mOwnE,
                                         u64 mOwnO, u64 &moved) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const unsigned dg = (unsigned)(dbits >> (8 * g));  // (g < 4: low word, else high word -- resolved at compile time)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u64 live = (!TAIL || 4 * g + q < nph) ? ~0ull : 0ull;
            const u64 mDraw = __builtin_amdgcn_ballot_w64((dg & (1u << q)) != 0u);
            if ((q & 1) == 0) {
                const u64 gtf = gt_hi16(KA, KB), gtp = gt_lo16(KA, KB);
                const u64 byf = zero_lo16(KA | KB) | mDraw;
                u64 worse = mPairE & (gtp ^ (byf & (gtf ^ gtp)));
                if (TAIL) worse &= live;
                const unsigned tk = KA, ti = IA;
                KA = msel(worse, KB, KA);
                IA = msel(worse, IB, IA);
                KB = msel(worse, tk, KB);
                IB = msel(worse, ti, IB);
                moved |= worse & mOwnE;
            } else {
                const unsigned KN = dpp_from_next(KA);
                const u64 gtf = gt_hi16(KB, KN), gtp = gt_lo16(KB, KN);
                const u64 byf = zero_lo16(KB | KN) | mDraw;
                u64 worse = mPairO & (gtp ^ (byf & (gtf ^ gtp)));
                if (TAIL) worse &= live;
                const u64 wprev = worse << 1;  // lane l + 1 takes lane l's second record when lane l's pair swaps
                const unsigned IN = dpp_from_next(IA), KP = dpp_from_prev(KB), IP = dpp_from_prev(IB);
                KB = msel(worse, KN, KB);
                IB = msel(worse, IN, IB);
                KA = msel(wprev, KP, KA);
                IA = msel(wprev, IP, IA);
                moved |= worse & mOwnO;
            }
        }
    }
}

// ---- populations below RS_MINLAM: the same phases inside ps_rank_kernel's ONE workgroup (round 6).  The one-pair-per-thread loop
// through LDS costs 0.35 us per phase (a barrier of the whole workgroup per phase: 99 us per ranking at lam = 280, the largest item of
// a generation at d = 12); here wave w < ceil(lam / 96) holds a window of 128 two-word records in registers (its own 96, 16 of either
// neighbour), runs sixteen phases on them without a barrier (rw_block), and the waves exchange their parts through LDS at ONE
// workgroup barrier per sixteen phases -- which is also where this population size tests for sixteen phases without a swap.  Keys by
// counting and draws (one chunk of 256 phases at a time) are made by all threads of the workgroup.  Same comparisons, same draws,
// same exit rule as the loop it replaces (DBG_PHASE_PAIRS keeps that loop; tests compare both with the NumPy oracle).
constexpr int RWS_OWN = 96, RWS_H = 16;
__host__ __device__ inline int rws_waves(int lam) { return (lam + RWS_OWN - 1) / RWS_OWN; }
__host__ __device__ inline int rws_pitch(int lam) { return ((lam / 2 + 64 + 7) / 8) * 8; }
__host__ __device__ inline size_t rws_smem_bytes(int lam) {  // f, phi | keys | two exchange buffers (key, index) | order | draws of a chunk | words
    const size_t lp = (size_t)((lam + 1) & ~1);
    return 16 * lp + 4 * lp + 16 * lp + 4 * lp + (size_t)64 * rws_pitch(lam) + 64;
}
// false: the generation holds a NaN (no rank): the caller's loop ranks it.  On success sidx_out[0 .. lam) is the order.
__device__ __forceinline__ bool rank_small_waves(const Args &a, int gen, const Run &R, int run, double *smem, int *&sidx_out) {
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int lam = R.lam, lp = (lam + 1) & ~1, nw = rws_waves(lam), pitch = rws_pitch(lam), nslots = lam / 2;
    double *sf = smem, *sphi = sf + lp;
    unsigned *skey = reinterpret_cast<unsigned *>(sphi + lp);
    unsigned *xk = skey + lp;        // [2][lp]
    unsigned *xi = xk + 2 * lp;      // [2][lp]
    int *sidx = reinterpret_cast<int *>(xi + 2 * lp);
    unsigned char *sdraw = reinterpret_cast<unsigned char *>(sidx + lp);
    int *s_moved = reinterpret_cast<int *>(sdraw + (size_t)64 * pitch);  // three words, used in turn
    bool nan = false;
    for (int i = tid; i < lam; i += NT) {
        const double fi = R.f[i], pi = R.phi[i];
        sf[i] = fi;
        sphi[i] = pi;
        nan = nan || fi != fi || pi != pi;
    }
    if (tid < 3) s_moved[tid] = 0;
    if (__syncthreads_or(nan ? 1 : 0)) return false;
    // keys: rank(f) << 16 | (0 if phi == 0, else 1 + rank(phi)), rank(x) = #{j : x_j < x}
    for (int i = tid; i < lam; i += NT) {
        const double fi = sf[i], pi = sphi[i];
        int cf = 0, cp = 0;
        for (int j = 0; j < lam; ++j) {
            cf += sf[j] < fi ? 1 : 0;
            cp += sphi[j] < pi ? 1 : 0;
        }
        skey[i] = ((unsigned)cf << 16) | (pi == 0.0 ? 0u : 1u + (unsigned)cp);
    }
    __syncthreads();
    const bool ranks = wave < nw;
    const int s0 = wave * RWS_OWN, e0 = min(lam, s0 + RWS_OWN), ws0 = s0 - RWS_H;
    const int gA = ws0 + 2 * lane, gB = gA + 1;
    const bool inA = ranks && gA >= 0 && gA < lam, inB = ranks && gB >= 0 && gB < lam;
    const bool ownA = ranks && gA >= s0 && gA < e0, ownB = ranks && gB >= s0 && gB < e0;
    const u64 mPairE = __builtin_amdgcn_ballot_w64(inA && inB), mPairO = __builtin_amdgcn_ballot_w64(inB && gB + 1 < lam && lane < 63);
    const u64 mOwnE = __builtin_amdgcn_ballot_w64(ownA), mOwnO = __builtin_amdgcn_ballot_w64(ownB);
    const int slot = max(0, gA >> 1);
    unsigned KA = inA ? skey[gA] : 0u, KB = inB ? skey[gB] : 0u, IA = (unsigned)gA, IB = (unsigned)gB;
    int blkno = 0;
    bool quiet_exit = false;
    for (int c = 0; c * 256 < lam && !quiet_exit; ++c) {
        // draws of this chunk: byte [group][pair slot], bit q = phase q of the group compares by objective
        const int ng = min(64, (lam - 256 * c + 3) / 4);
        for (int e = tid; e < ng * pitch; e += NT) {
            const int g = e / pitch, m = e % pitch;
            unsigned bits = 0;
            if (m < nslots) {
                unsigned c4[4] = {(unsigned)m, (unsigned)(256 * c + 4 * g), (unsigned)(gen * 16 + 1), (unsigned)run};
                philox(c4, (unsigned)a.seed, (unsigned)(a.seed >> 32));
#pragma unroll
                for (int q = 0; q < 4; ++q) bits |= (((double)c4[q] + 0.5) * (1.0 / 4294967296.0) < 0.45) ? (1u << q) : 0u;
            }
            sdraw[e] = (unsigned char)bits;
        }
        __syncthreads();
        for (int b = 0; b < 16; ++b, ++blkno) {
            const int phb = 256 * c + 16 * b;
            if (phb >= lam) break;
            const int par = blkno & 1;
            if (ranks) {
                u64 dbits = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (4 * b + g < ng) dbits |= (u64)sdraw[(size_t)(4 * b + g) * pitch + slot] << (8 * g);
                u64 moved = 0;
                if (phb + 16 <= lam)
                    rw_block<false, 4>(KA, KB, IA, IB, dbits, 16, mPairE, mPairO, mOwnE, mOwnO, moved);
                else
                    rw_block<true, 4>(KA, KB, IA, IB, dbits, lam - phb, mPairE, mPairO, mOwnE, mOwnO, moved);
                if (ownA) {
                    xk[par * lp + gA] = KA;
                    xi[par * lp + gA] = IA;
                }
                if (ownB) {
                    xk[par * lp + gB] = KB;
                    xi[par * lp + gB] = IB;
                }
                if (moved != 0 && lane == 0) s_moved[blkno % 3] = 1;
            }
            __syncthreads();
            const int any = s_moved[blkno % 3];
            if (tid == 0) s_moved[(blkno + 2) % 3] = 0;  // (its last readers passed this barrier's predecessor; its next writers come after this one)
            if (!any) {  // sixteen phases without a swap: ranked under the drawn rules
                quiet_exit = true;
                break;
            }
            if (inA && !ownA) {
                KA = xk[par * lp + gA];
                IA = xi[par * lp + gA];
            }
            if (inB && !ownB) {
                KB = xk[par * lp + gB];
                IB = xi[par * lp + gB];
            }
        }
    }
    if (ownA) sidx[gA] = (int)IA;
    if (ownB) sidx[gB] = (int)IB;
    __syncthreads();
    sidx_out = sidx;
    return true;
}

__global__ __launch_bounds__(RANK_THREADS) void ps_rank_kernel(const Args *__restrict__ A, int gen, int mode, RankWs ws) {
    const Args &a = A[blockIdx.y];
    extern __shared__ double smem[];
    __shared__ double s_red[2 * (RANK_THREADS / 64)];
    __shared__ int s_ired[2 * (RANK_THREADS / 64)];
    __shared__ int s_swapped, s_stop, s_best, s_infeas;
    const int run = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = (int)blockDim.x;  // 64 .. RANK_THREADS: a small population is ranked by as many waves as it has pairs (a barrier of three waves instead of sixteen)
    const Run &R = a.runs[run];
    if (R.stat[1]) return;
    const int grun = a.grun0 + run;
    int *const sy = ws.sync ? ws.sync + grun * RS_SYNC : nullptr;
    if (mode == 2 && sy[2] == 0) return;  // (this run's generation was finished in mode 1)
    const int n = R.nvar, lam = R.lam, mu = R.mu;
    const double *X = R.X[gen & 1];
    const int evals0 = R.stat[0];
    const int m = min(lam, R.max_evals - evals0);
    if (tid == 0) {
        s_infeas = mode == 2 ? 1 : 0;
        s_stop = 0;
    }
    __syncthreads();
    // ---- (no linear constraints: the run's individuals are scored here, a thread per individual -- ps_score_kernel's arithmetic)
    if (mode != 2 && a.score_fused) {
        for (int i = tid; i < lam; i += NT) {
            double fi, pi;
            score_row<false>(a, gen, R, i, R.off + i, 0, fi, pi);
            R.f[i] = fi;
            R.phi[i] = pi;
        }
        __syncthreads();  // f / phi of the run are read below (and by the launches that follow this one)
    }
    // ---- this generation's best individual and whether any individual inside the budget violates a constraint
    if (mode != 2) {
        Cand mine{0.0, -1, 0x7fffffff};
        bool infeas = false;
        for (int i = tid; i < m; i += NT) {
            const double fi = R.f[i], pi = R.phi[i];
            if (pi > 0.0 && pi < INFINITY) infeas = true;
            if (pi == INFINITY) continue;
            const Cand c{pi == 0.0 ? fi : pi, pi == 0.0 ? 1 : 0, i};
            if (cand_better(c, mine)) mine = c;
        }
        if (infeas) s_infeas = 1;
        for (int off = 32; off > 0; off >>= 1) {
            Cand o;
            o.key = __shfl_xor(mine.key, off);
            o.feas = __shfl_xor(mine.feas, off);
            o.idx = __shfl_xor(mine.idx, off);
            if (cand_better(o, mine)) mine = o;
        }
        if (lane == 0) {
            s_red[wave] = mine.key;
            s_ired[2 * wave] = mine.feas;
            s_ired[2 * wave + 1] = mine.idx;
        }
        __syncthreads();
        if (tid == 0) {
            Cand b{0.0, -1, 0x7fffffff};
            for (int w = 0; w < NT / 64; ++w) {
                const Cand c{s_red[w], s_ired[2 * w], s_ired[2 * w + 1]};
                if (cand_better(c, b)) b = c;
            }
            s_best = -1;
            if (b.feas >= 0) {
                const double bf = R.best[n], bphi = R.best[n + 1];
                if ((b.feas == 1 && (bphi > 0.0 || b.key < bf)) || (b.feas == 0 && b.key < bphi)) {
                    s_best = b.idx;
                    R.best[n] = b.feas == 1 ? b.key : R.f[b.idx];
                    R.best[n + 1] = b.feas == 1 ? 0.0 : b.key;
                }
            }
            R.stat[0] = evals0 + max(m, 0);
            R.stat[2] = gen + 1;
            s_stop = (evals0 + m >= R.max_evals || m < lam) ? 1 : 0;
        }
        __syncthreads();
        if (s_best >= 0)
            for (int c = tid; c < n; c += NT) R.best[c] = X[(size_t)s_best * n + c];
    }
    if (s_stop) {
        if (tid == 0) R.stat[1] = 1;
        return;
    }
    // ---- ranking.  If no individual inside the budget violates a constraint (always so for unconstrained ideal-point runs,
    // usually so late in a PS run) every comparison of the pairwise rule is decided by (violation, objective) whatever is drawn,
    // and lam phases of the stable transposition sort end in THE sorted order (ties by index): a bitonic network over the padded
    // array reaches the same order in log2(N) (log2(N) + 1) / 2 phases (91 instead of 5160 at lam = 5160).
    const bool plain_sort = s_infeas == 0 && !(a.dbg & DBG_PHASES);
    if (mode == 1) {
        // Populations of RS_MINLAM and more leave this workgroup here, either way:
        //   sy[2] = 1  violations inside the budget: the transposition phases on several compute units (ps_rank_wave_kernel)
        //   sy[2] = 2  none: the sorted order by COUNTING on the whole chip -- rank(i) = #{j : f_j < f_i, or f_j = f_i and j < i} is the
        //              position of i in the stable sort by f, lam^2 independent comparisons (ps_rank_prep_kernel, a few us) instead of
        //              a bitonic network in this one workgroup (34 / 61 / 71 us at lam = 1320 / 2600 / 5160, half of a generation of
        //              an ideal-point run at d = 128); the finishing launch (mode 2) turns the counts into the parents' list.
        // (a NaN has no rank, so a generation that holds one stays here)
        bool nan = false;
        if (lam >= RS_MINLAM)
            for (int i = tid; i < lam; i += NT) nan = nan || R.f[i] != R.f[i] || R.phi[i] != R.phi[i];
        const bool leave = lam >= RS_MINLAM && !__syncthreads_or(nan ? 1 : 0);
        const int kind = !leave ? 0 : (!plain_sort ? 1 : (!(a.dbg & (DBG_SORT_PAIRS | DBG_NO_SELECT | DBG_SELECT)) ? 2 : 0));
        for (int i = tid; i < RS_SYNC; i += NT) sy[i] = i == 2 ? kind : 0;
        if (kind) {
            int *cnt = ws.cnt + (size_t)grun * 2 * MAXLAM;
            for (int i = tid; i < lam; i += NT) cnt[i] = cnt[MAXLAM + i] = 0;
            return;
        }
    }
    int *sidx;
    if (mode == 2 && sy[2] == 2) {  // the positions found by counting (ps_rank_prep_kernel)
        sidx = (int *)smem;
        const int *cnt = ws.cnt + (size_t)grun * 2 * MAXLAM;
        for (int i = tid; i < lam; i += NT) sidx[cnt[i]] = i;
        __syncthreads();
    } else if (mode == 2 && sy[1] == 0) {  // the order found by ps_rank_wave_kernel
        sidx = (int *)smem;
        const int *src = ws.idx + (size_t)grun * MAXLAM;
        for (int i = tid; i < lam; i += NT) sidx[i] = src[i];
        __syncthreads();
    } else if (plain_sort && !(a.dbg & (DBG_SORT_PAIRS | DBG_NO_SELECT)) && NT >= 256 && mu * 4 <= lam && (npow2(lam) >= 8 * NT || (a.dbg & DBG_SELECT)) &&
               select_parents(R.f, lam, mu, smem, (int *)(smem + npow2(lam)))) {  // (measured: pays from lam > 4096 on -- 135 against 195 us per ranking at
                                                                                  // lam = 5160; below, its sampling pass costs what the shorter sort saves; DBG_SELECT forces it)
        sidx = (int *)(smem + npow2(lam));  // (parents found and ranked without sorting the rest: see select_parents)
    } else if (plain_sort && !(a.dbg & DBG_SORT_PAIRS) && (npow2(lam) == NT || npow2(lam) == 2 * NT || npow2(lam) == 4 * NT || npow2(lam) == 8 * NT)) {
        // (the launch's thread count follows the LARGEST population: N / 2 up to N = 2048, 1024 beyond; a run whose padded size is not
        // 2, 4 or 8 elements per thread -- a much smaller run in the same launch -- takes the one-pair-per-thread form below)
        const int N = npow2(lam);
        double *sf = smem;      // N keys: violation is 0 or inf here, and inf comes with f = inf
        sidx = (int *)(sf + N);
        if (N == NT)
            bitonic_regs<1>(R.f, nullptr, lam, N, sf, sidx);
        else if (N == 2 * NT)
            bitonic_regs<2>(R.f, nullptr, lam, N, sf, sidx);
        else if (N == 4 * NT)
            bitonic_regs<4>(R.f, nullptr, lam, N, sf, sidx);
        else
            bitonic_regs<8>(R.f, nullptr, lam, N, sf, sidx);
    } else if (plain_sort) {
        const int N = npow2(lam);
        double *sf = smem;      // N keys: violation is 0 or inf here, and inf comes with f = inf
        sidx = (int *)(sf + N);
        for (int i = tid; i < N; i += NT) {
            sf[i] = i < lam ? R.f[i] : INFINITY;
            sidx[i] = i < lam ? i : 0x7fffffff;
        }
        __syncthreads();
        for (int kk = 2; kk <= N; kk <<= 1)
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < N / 2; t += NT) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;  // the t-th pair of this stage
                    const double fa = sf[i], fb = sf[l];
                    const int ia = sidx[i], ib = sidx[l];
                    const bool greater = fa > fb || (fa == fb && ia > ib);
                    const bool up = (i & kk) == 0;
                    if (greater == up) {
                        sf[i] = fb;
                        sf[l] = fa;
                        sidx[i] = ib;
                        sidx[l] = ia;
                    }
                }
                __syncthreads();
            }
    } else {
        // lam phases of odd-even transposition; a pair is compared by f when both are feasible or with probability 0.45, else by
        // the constraint violation (Runarsson & Yao).  The records themselves are swapped; one Philox call feeds four phases of a
        // pair; one barrier per phase.
        if (lam < RS_MINLAM && !(a.dbg & DBG_PHASE_PAIRS) && NT >= 64 * rws_waves(lam) && rank_small_waves(a, gen, R, run, smem, sidx)) {
            // (the order is in sidx: the records stayed in registers -- see rank_small_waves)
        } else {
        double *sf = smem, *sphi = sf + lam;
        sidx = (int *)(sphi + lam);
        for (int i = tid; i < lam; i += NT) {
            sf[i] = R.f[i];
            sphi[i] = R.phi[i];
            sidx[i] = i;
        }
        if (tid == 0) s_swapped = 1;
        __syncthreads();
        constexpr int PSLOTS = (MAXLAM / 2 + RANK_THREADS - 1) / RANK_THREADS;  // pairs per thread and phase
        // ONE exit rule for a population size, whichever kernel ranks it: with stochastic comparisons a stretch of phases without a
        // swap is not a fixed point (a pair that disagrees on f and phi can still swap on a later draw), so WHERE the no-swap test
        // sits decides the order that comes out.  Populations of RS_MINLAM and more -- the ones ps_rank_wave_kernel takes, whose waves
        // meet only every RS_B phases -- are tested every RS_B phases here too (this code is also that kernel's fallback after
        // a time-out and the MRBF_PS_MULTI=0 path); smaller ones every sixteen.
        const int quiet = lam >= RS_MINLAM ? RS_B : 16;
        for (int ph0 = 0; ph0 < lam; ph0 += 4) {
            if (ph0 % quiet == 0) {
                const int sw = s_swapped;
                __syncthreads();
                if (!sw) break;  // `quiet` phases without a swap: ranked under the drawn rules
                if (tid == 0) s_swapped = 0;
                __syncthreads();
            }
            unsigned c4[PSLOTS][4];
            bool drawn[PSLOTS];
#pragma unroll
            for (int s = 0; s < PSLOTS; ++s) drawn[s] = false;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int ph = ph0 + q4;
                if (ph < lam) {
#pragma unroll
                    for (int s = 0; s < PSLOTS; ++s) {
                        const int p = tid + s * NT;
                        const int j = 2 * p + (ph & 1);
                        if (j + 1 < lam) {
                            const double fa = sf[j], fb = sf[j + 1], pa = sphi[j], pb = sphi[j + 1];
                            const int ia = sidx[j], ib = sidx[j + 1];  // (with the keys: a swap then costs no second LDS round trip)
                            bool by_f = pa == 0.0 && pb == 0.0;
                            if (!by_f) {
                                if (!drawn[s]) {
                                    c4[s][0] = (unsigned)p;
                                    c4[s][1] = (unsigned)ph0;
                                    c4[s][2] = (unsigned)(gen * 16 + 1);
                                    c4[s][3] = (unsigned)run;
                                    philox(c4[s], (unsigned)a.seed, (unsigned)(a.seed >> 32));
                                    drawn[s] = true;
                                }
                                by_f = ((double)c4[s][q4] + 0.5) * (1.0 / 4294967296.0) < 0.45;
                            }
                            const bool worse = by_f ? (fa > fb) : (pa > pb);
                            if (worse) {
                                sf[j] = fb;
                                sf[j + 1] = fa;
                                sphi[j] = pb;
                                sphi[j + 1] = pa;
                                sidx[j] = ib;
                                sidx[j + 1] = ia;
                                s_swapped = 1;
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();
        }
    }
    // the parents, in rank order
    for (int i = tid; i < mu; i += NT) R.order[i] = sidx[i];
    // ---- stop like NLopt's xtol_rel, on the survivors' spread: variable by variable, leaving at the first one that still spreads
    bool converged = true;
    for (int c = 0; c < n; ++c) {
        double lo = INFINITY, hi = -INFINITY;
        for (int s2 = tid; s2 < mu; s2 += NT) {
            const double v = X[(size_t)sidx[s2] * n + c];
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
        for (int off = 32; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, off));
            hi = fmax(hi, __shfl_xor(hi, off));
        }
        __syncthreads();  // s_red of the previous variable has been read
        if (lane == 0) {
            s_red[2 * wave] = lo;
            s_red[2 * wave + 1] = hi;
        }
        __syncthreads();
        for (int w = 0; w < NT / 64; ++w) {
            lo = fmin(lo, s_red[2 * w]);
            hi = fmax(hi, s_red[2 * w + 1]);
        }
        if (hi - lo > a.xtol_rel * fmax(fabs(X[(size_t)sidx[0] * n + c]), 1e-300)) {
            converged = false;
            break;  // uniform: every thread holds the same lo / hi
        }
    }
    if (tid == 0) {
        if (converged)
            R.stat[1] = 1;
        else
            R.stat[3] = gen + 1;  // breed the next generation
    }
}

// ---- the transposition phases of large populations on several compute units: one WAVE per part, the records in registers (round 6).
// A phase moves information by one position, so a wave that holds its part of the array plus RW_H positions on either side can run
// RW_H phases on its own and its part comes out exactly as if the whole array had been worked on (the halo positions go wrong from the
// window's edges inwards, one position per phase, and are thrown away); every comparison is a function of (pair, phase, values) --
// the Philox counter is the pair and the four-phase group, as in ps_rank_kernel -- so the redundant comparisons in the halos agree
// with the owner's.  A wave holds a window of 128 records, two per lane (its own RW_OWN = 64 in the middle, RW_H = 32 of either
// neighbour on each side), so an even phase is lane-local, an odd phase takes the neighbouring lane's record by DPP (wave_shl /
// wave_shr), and no phase needs a barrier (one workgroup per run pays an LDS round trip and a barrier per phase); after RW_H phases
// the waves publish their parts (write-through stores of self-describing records: see the kernel) and take the neighbours' halves --
// a wave waits for its two neighbours only.  Every RS_B phases all waves of the run meet at the arrival counter: a chunk in which no
// wave moved anything inside its own part ends the ranking (ps_rank_kernel applies the same test at the same phases for these
// population sizes: one exit rule, hence one order, whichever kernel runs).  The waits are bounded: on a time-out the failure word
// is set and ps_rank_kernel (mode 2) runs the phases itself -- this kernel never writes f / phi.
// A wave alone on its SIMD issues one instruction every four cycles whatever its kind, so the instruction count of a phase IS its
// time (measured 0.11 us with records of two doubles + index: 22 vector + 14 scalar instructions).  Two things are therefore taken
// out of the phases and done beforehand on the whole chip by ps_rank_prep_kernel, since neither depends on the order so far:
//   * the draws (Philox is 40 quarter-rate multiplies per four phases): one byte per (four-phase group, pair slot), bit q = "phase
//     q of the group compares by objective";
//   * the keys: the pairwise rule only ever asks fa > fb, pa > pb and pa == pb == 0, and rank(x) = #{j : x_j < x} answers the first
//     two exactly (ties stay ties), so a record is TWO words -- (rank of f) << 16 | (0 if phi == 0, else 1 + rank of phi), and the
//     index -- instead of five, compared by 16-bit integer compares.  (NaN has no rank: ps_rank_kernel does not hand such a
//     generation over.)
// grid.x = [draw workgroups | counting workgroups]; the counts (ws.cnt: lam objective counts, then lam violation counts per run) are
// zeroed by ps_rank_kernel (mode 1) when it hands the generation over
__global__ __launch_bounds__(256) void ps_rank_prep_kernel(const Args *__restrict__ A, int gen, RankWs ws, u64 *draws, size_t per_run, int draw_blocks) {
    __shared__ double sf[RW_CNT_T], sp[RW_CNT_T];
    const Args &a = A[blockIdx.z];
    const int run = blockIdx.y, grun = a.grun0 + run;
    const Run &R = a.runs[run];
    const int *sy = ws.sync + grun * RS_SYNC;
    const int kind = sy[2];  // 1: draws + keys for the transposition phases; 2: the sorted order of a generation without violations
    if (R.stat[1] || kind == 0) return;
    const int lam = R.lam;
    if ((int)blockIdx.x < draw_blocks) {
        if (kind != 1) return;
        const int pitch = rw_pitch(lam), nblk = (lam + RW_H - 1) / RW_H, npair = lam / 2;
        u64 *out = draws + (size_t)grun * per_run;  // [block of RW_H phases][pair slot]: byte g = the block's g-th group of four phases
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)nblk * pitch; e += (int64_t)draw_blocks * 256) {
            const int blk = (int)(e / pitch), m = (int)(e % pitch);
            u64 bits = 0;
            if (m < npair) {
#pragma unroll
                for (int g = 0; g < RW_H / 4; ++g) {
                    unsigned c4[4] = {(unsigned)m, (unsigned)(blk * RW_H + 4 * g), (unsigned)(gen * 16 + 1), (unsigned)run};
                    philox(c4, (unsigned)a.seed, (unsigned)(a.seed >> 32));
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        bits |= (((double)c4[q] + 0.5) * (1.0 / 4294967296.0) < 0.45) ? (1ull << (8 * g + q)) : 0ull;
                }
            }
            out[e] = bits;
        }
        return;
    }
    // counting: workgroup (ib, js) counts, for its 256 individuals i, the j of its share with f_j < f_i and with phi_j < phi_i
    const int cb = (int)blockIdx.x - draw_blocks, nib = (lam + RW_CNT_T - 1) / RW_CNT_T, js = cb / nib, ib = cb % nib, nsplit = rw_jsplit(lam);
    if (js >= nsplit) return;
    const int i = ib * RW_CNT_T + threadIdx.x;
    const double fi = i < lam ? R.f[i] : 0.0, pi = i < lam ? R.phi[i] : 0.0;
    const int per = (lam + nsplit - 1) / nsplit, j0 = js * per, j1 = min(lam, j0 + per);
    int cf = 0, cp = 0;
    for (int jb = j0; jb < j1; jb += RW_CNT_T) {
        const int nj = min(RW_CNT_T, j1 - jb);
        __syncthreads();
        if ((int)threadIdx.x < nj) {
            sf[threadIdx.x] = R.f[jb + threadIdx.x];
            sp[threadIdx.x] = R.phi[jb + threadIdx.x];
        }
        __syncthreads();
        if (kind == 1) {
            for (int j = 0; j < nj; ++j) {
                cf += sf[j] < fi ? 1 : 0;
                cp += sp[j] < pi ? 1 : 0;
            }
        } else {  // position in the stable sort by f: ties by index
            for (int j = 0; j < nj; ++j) cf += (sf[j] < fi || (sf[j] == fi && jb + j < i)) ? 1 : 0;
        }
    }
    if (i < lam) {
        int *cnt = ws.cnt + (size_t)grun * 2 * MAXLAM;
        atomicAdd(cnt + i, cf);
        atomicAdd(cnt + MAXLAM + i, cp);
    }
}

__device__ __forceinline__ unsigned long long rs_clock() { return __builtin_amdgcn_s_memrealtime(); }  // 100 MHz
__global__ __launch_bounds__(64) void ps_rank_wave_kernel(const Args *__restrict__ A, RankWs ws, const u64 *draws, size_t per_run, unsigned epoch) {
    const Args &a = A[blockIdx.z];
    const int run = a.grun0 + (int)blockIdx.y, w = blockIdx.x, lane = threadIdx.x;  // (the launch-wide index: this kernel draws nothing)
    const Run &R = a.runs[blockIdx.y];
    int *const sy = ws.sync + run * RS_SYNC;
    if (R.stat[1] || sy[2] != 1) return;
    const int lam = R.lam, nw = rw_waves(lam);
    if (w >= nw) return;
    if (a.dbg & DBG_GIVE_UP) {  // (test switch: give up at once, as after a counter time-out)
        if (lane == 0) __hip_atomic_store(sy + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const size_t ro = (size_t)run * MAXLAM;
    // exchange buffers (the words of ws.f): a record travels as ONE 64-bit word -- key << 32 | tag << 16 | individual, tag = (launch, block)
    // -- so the word itself says when it has arrived: the reader polls the records it needs, there is no flag to write after the data
    // and no wait for the stores to be acknowledged (one trip through memory per exchange instead of three).  A buffer is rewritten
    // every second block and neighbours are never more than one block apart (a wave publishes block b + 1 only after it has taken
    // its neighbours' block b), so a reader cannot miss a record; records of earlier launches carry another launch number.
    u64 *const xr[2] = {reinterpret_cast<u64 *>(ws.f[0]) + ro, reinterpret_cast<u64 *>(ws.f[1]) + ro};
    const int s0 = w * RW_OWN, e0 = min(lam, s0 + RW_OWN), ws0 = s0 - RW_H;  // (ws0 even; negative for the first wave)
    const int gA = ws0 + 2 * lane, gB = gA + 1;                              // this lane's two positions
    const bool inA = gA >= 0 && gA < lam, inB = gB >= 0 && gB < lam;
    const bool ownA = gA >= s0 && gA < e0, ownB = gB >= s0 && gB < e0;
    const bool needA = inA && !ownA, needB = inB && !ownB;
    // lane masks (scalar registers): the decisions of a phase are mask arithmetic on the scalar unit, the vector unit compares and selects
    const u64 mPairE = __builtin_amdgcn_ballot_w64(inA && inB);                          // even phases: (gA, gB), lane-local
    const u64 mPairO = __builtin_amdgcn_ballot_w64(inB && gB + 1 < lam && lane < 63);    // odd phases: (gB, next lane's gA)
    const u64 mOwnE = __builtin_amdgcn_ballot_w64(ownA), mOwnO = __builtin_amdgcn_ballot_w64(ownB);  // the pair's left position lies in this wave's part
    const int slot = max(0, gA >> 1);  // pair slot of both of this lane's pairs
    const int pitch = rw_pitch(lam);
    const u64 *dr = draws + (size_t)run * per_run + slot;
    const int *cnt = ws.cnt + (size_t)run * 2 * MAXLAM;
    unsigned KA = 0, KB = 0, IA = (unsigned)gA, IB = (unsigned)gB;
    if (inA) KA = ((unsigned)cnt[gA] << 16) | (R.phi[gA] == 0.0 ? 0u : 1u + (unsigned)cnt[MAXLAM + gA]);
    if (inB) KB = ((unsigned)cnt[gB] << 16) | (R.phi[gB] == 0.0 ? 0u : 1u + (unsigned)cnt[MAXLAM + gB]);
    const int nblk = (lam + RW_H - 1) / RW_H;
    u64 moved = 0;
    u64 dnext = dr[0];
    for (int blk = 0; blk < nblk; ++blk) {
        const int phb = blk * RW_H;
        const u64 dbits = dnext;
        if (blk + 1 < nblk) dnext = dr[(size_t)(blk + 1) * pitch];  // (next block's draws: in flight over this block)
        if (phb + RW_H <= lam)
            rw_block<false, RW_H / 4>(KA, KB, IA, IB, dbits, RW_H, mPairE, mPairO, mOwnE, mOwnO, moved);
        else
            rw_block<true, RW_H / 4>(KA, KB, IA, IB, dbits, lam - phb, mPairE, mPairO, mOwnE, mOwnO, moved);
        // ---- publish this wave's part
        const int db = blk & 1;
        const unsigned tag = ((epoch & 0xffu) << 8) | (unsigned)(blk + 1);
        if (ownA) __hip_atomic_store(xr[db] + gA, ((u64)KA << 32) | (tag << 16) | IA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ownB) __hip_atomic_store(xr[db] + gB, ((u64)KB << 32) | (tag << 16) | IB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool chunk_end = ((blk + 1) * RW_H) % RS_B == 0 || blk + 1 == nblk;
        const int c = (blk * RW_H) / RS_B;
        const unsigned long long t0 = rs_clock();
        int ok = 1, any = 1;
        if (chunk_end) {  // ---- every RS_B phases: all waves of the run meet for the exit rule
            if (lane == 0) {
                if (moved != 0) __hip_atomic_fetch_or(sy + 4 + c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(sy, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // (orders the "moved" flag before the count)
                int spins = 0;
                while (__hip_atomic_load(sy, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < nw * (c + 1)) {
                    if ((++spins & 15) == 0 && (__hip_atomic_load(sy + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || rs_clock() - t0 > 500000ull)) {  // 5 ms
                        ok = 0;
                        break;
                    }
                }
                if (ok) any = __hip_atomic_load(sy + 4 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            ok = __builtin_amdgcn_readfirstlane(ok);
            any = __builtin_amdgcn_readfirstlane(any);
            moved = 0;
            if (ok && (!any || blk + 1 == nblk)) {  // nothing moved in RS_B phases (ranked under the drawn rules), or all phases done
                int *out = ws.idx + ro;             // the order, for the finishing launch
                if (ownA) out[gA] = (int)IA;
                if (ownB) out[gB] = (int)IB;
                return;
            }
        }
        // ---- take the neighbours' halves: poll the records until they carry this block's tag
        if (ok) {
            int spins = 0;
            for (;;) {
                const u64 ra = needA ? __hip_atomic_load(xr[db] + gA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                const u64 rb = needB ? __hip_atomic_load(xr[db] + gB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                const bool okA = !needA || (((unsigned)ra >> 16) == tag), okB = !needB || (((unsigned)rb >> 16) == tag);
                if (okA && needA) {
                    KA = (unsigned)(ra >> 32);
                    IA = (unsigned)ra & 0xffffu;
                }
                if (okB && needB) {
                    KB = (unsigned)(rb >> 32);
                    IB = (unsigned)rb & 0xffffu;
                }
                if (__builtin_amdgcn_ballot_w64(!(okA && okB)) == 0) break;
                if ((++spins & 15) == 0 && (__hip_atomic_load(sy + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || rs_clock() - t0 > 500000ull)) {  // 5 ms
                    ok = 0;
                    break;
                }
            }
        }
        if (!ok) {
            if (lane == 0) {
                __hip_atomic_store(sy + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ws.sticky, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (sticky: the host stops using this kernel)
            }
            return;
        }
    }
}

// ---- next generation: one wave per offspring, lanes over the components
__global__ __launch_bounds__(256) void ps_breed_kernel(const Args *__restrict__ A, int gen) {
    const Args &a = A[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int run = run_of_row(a, row);
    const Run &R = a.runs[run];
    if (R.stat[3] != gen + 1) return;
    const int n = R.nvar, mu = R.mu, o = row - R.off;
    const double *X = R.X[gen & 1], *S = R.S[gen & 1];
    double *Xn = R.X[(gen + 1) & 1], *Sn = R.S[(gen + 1) & 1];
    const double tau = 1.0 / sqrt(2.0 * sqrt((double)n)), taup = 1.0 / sqrt(2.0 * (double)n), alpha = 0.2, gamma = 0.85;
    const int nd = mu - 1;
    const int par = R.order[o % mu];
    const double *xp = X + (size_t)par * n, *sp = S + (size_t)par * n;
    double *xo = Xn + (size_t)o * n, *so = Sn + (size_t)o * n;
    const int skip = R.kind == 1 ? 1 : 0;
    double *xe = a.Xeval + (size_t)row * a.d;  // next generation's row of the evaluation batch (x part)
    __shared__ double s_row[4][360];           // the wave's new x part (a.Xq: centred below with the centring kernel's lane mapping)
    double *const srow = s_row[threadIdx.x >> 6];
    const bool keep = a.Xq != nullptr;
    if (o < nd) {
        // differential variation towards the best individual; kept only if it stays inside the box
        const double *xb = X + (size_t)R.order[0] * n, *xq = X + (size_t)R.order[o + 1] * n;
        bool inside = true;
        for (int c = lane; c < n; c += 64) {
            const double v = xp[c] + gamma * (xb[c] - xq[c]);
            inside = inside && v >= lo_of(a, R, c) && v <= hi_of(a, R, c);
        }
        inside = __all(inside);
        for (int c = lane; c < n; c += 64) {
            const double v = inside ? xp[c] + gamma * (xb[c] - xq[c]) : xp[c];
            xo[c] = v;
            so[c] = sp[c];
            if (c >= skip) {
                xe[c - skip] = v;
                if (keep) srow[c - skip] = v;
            }
        }
    } else {
        double u0, u1, zg, z1;
        rng4(a, run, gen, o, n, 2, u0, u1, zg, z1);  // the individual's global factor (the same draw in every lane)
        for (int c = lane; c < n; c += 64) {
            const double lo = lo_of(a, R, c), hi = hi_of(a, R, c);
            double z0, zz;
            rng4(a, run, gen, o, c, 3, u0, u1, z0, zz);
            double s = sp[c] * (double)__expf((float)(taup * zg + tau * z0));
            s = fmin(s, (hi - lo) / sqrt((double)n));
            double v = xp[c] + s * zz;
            for (int tr = 0; tr < 10 && (v < lo || v > hi); ++tr) {  // re-draw components that leave the box
                double w0, w1;
                rng4(a, run, gen, o, c, 4 + tr, u0, u1, w0, w1);
                v = xp[c] + s * w0;
            }
            if (v < lo || v > hi) v = xp[c];
            xo[c] = v;
            if (c >= skip) {
                xe[c - skip] = v;
                if (keep) srow[c - skip] = v;
            }
            so[c] = sp[c] + alpha * (s - sp[c]);  // exponential smoothing
        }
    }
    if (keep) {  // Xq[row][t] = x[t] - mean[t] (zero in the padding), xsq[row] = |Xq[row]|^2: center_pad_kernel's arithmetic, lane for lane
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (the wave's own LDS writes above are read by other lanes below)
        double ss = 0.0;
        for (int t = lane; t < a.xqD; t += 64) {
            double v = 0.0;
            if (t < a.d) v = srow[t] - a.xmean[t];
            a.Xq[(size_t)row * a.xqD + t] = v;
            ss = fma(v, v, ss);
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        if (lane == 0) a.xsq[row] = ss;
    }
}


}  // namespace ps

// ---- how the ranking of the runs of one Args is launched: ps_rank_kernel's thread count and dynamic LDS and, on the
// several-compute-unit path, the work space and the draws.  The step and the test hook both go through these two functions.
struct RankLaunch {
    int maxlam = 0, threads = 0;
    size_t shm = 0;
    bool several = false;  // populations of RS_MINLAM and more leave ps_rank_kernel's one workgroup (modes 1 / 2 around ps_rank_wave_kernel)
    ps::RankWs ws{};
    unsigned long long *draws = nullptr;
    size_t draws_per_run = 0;
};
// once per phase, before the first generation: `a` is the block of one of the launch's `nstarts` starts (they share the runs' shapes);
// `allow_several`: the caller's say on the several-compute-unit path
static int rank_launch_setup(mrbf_ctx *ctx, const ps::Args &a, int nstarts, bool allow_several, RankLaunch &L) {
    using namespace ps;
    // (populations below RS_MINLAM: room and waves for rank_small_waves -- a wave per 96 individuals, a chunk of draws in LDS;
    //  over ALL runs of the launch: a small run beside a large one must find its room too)
    size_t small_need = 0;
    int small_waves = 0;
    for (int q = 0; q < a.nruns; ++q) {
        const int lam = a.runs[q].lam;
        L.maxlam = std::max(L.maxlam, lam);
        if (lam < RS_MINLAM) {
            small_need = std::max(small_need, rws_smem_bytes(lam));
            small_waves = std::max(small_waves, rws_waves(lam));
        }
    }
    int N = 1;
    while (N < L.maxlam) N <<= 1;
    L.shm = std::max(std::max((size_t)20 * L.maxlam, (size_t)12 * N), small_need);
    // one thread per pair of the largest population (the bitonic network's N / 2 pairs), whole waves, at most RANK_THREADS
    // (a small population that needs more waves than N / 2 threads hold takes N threads: the plain sort then runs as one element per thread)
    L.threads = (int)std::min<int64_t>(RANK_THREADS, std::max<int64_t>(64, round_up(N / 2, 64)));
    if (64 * small_waves > L.threads) L.threads = (int)std::min<int64_t>(RANK_THREADS, std::max<int64_t>(N, 64 * small_waves));
    MRBF_HIP(ctx, hipFuncSetAttribute((const void *)ps_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.shm));
    L.several = allow_several && L.maxlam >= RS_MINLAM;
    if (!L.several) return MRBF_OK;
    L.draws_per_run = (size_t)((L.maxlam + RW_H - 1) / RW_H) * rw_pitch(L.maxlam);
    RankWs &rw = L.ws;
    double *wsb;
    const size_t per_run = (size_t)MAXLAM * 7 / 2 + RS_SYNC / 2;  // two exchange buffers, the order and the two counts (as doubles: 3 x 1/2), sync words
    const size_t TR = (size_t)std::max(MAXRUNS, nstarts * a.nruns);  // runs of the launch (the residency rule keeps them few: the caller's allow_several)
    MRBF_TRY(get_buf(ctx, S_PS_RANK, per_run * TR + 64 + L.draws_per_run * TR, &wsb));
    rw.f[0] = wsb;
    rw.f[1] = rw.f[0] + (size_t)MAXLAM * TR;
    rw.idx = reinterpret_cast<int *>(rw.f[1] + (size_t)MAXLAM * TR);
    rw.cnt = rw.idx + (size_t)MAXLAM * TR;
    rw.sync = rw.cnt + (size_t)2 * MAXLAM * TR;
    rw.sticky = rw.sync + RS_SYNC * TR;
    L.draws = reinterpret_cast<unsigned long long *>(wsb + per_run * TR + 64);
    // ps_rank_wave_kernel's readers accept any word whose bits 16..31 equal the block's tag.  The arena is not cleared when it is
    // handed out, so a word left by earlier work (a double of another buffer, a record of an earlier call whose launch number
    // agrees modulo 256) could pass as a record and carry an individual index beyond lam into the parents' list.  A zero word has
    // tag 0, which no block uses: both exchange buffers start as zeros at every call.
    MRBF_HIP(ctx, hipMemsetAsync(rw.f[0], 0, (size_t)2 * MAXLAM * TR * sizeof(double), ctx->stream));
    MRBF_HIP(ctx, hipMemsetAsync(rw.sticky, 0, sizeof(int), ctx->stream));
    return MRBF_OK;
}
// one generation's ranking: ps_rank_kernel alone (mode 0) or, on the several-compute-unit path, its bookkeeping (mode 1), the draws /
// keys / counted sort on the whole chip, the transposition phases with one wave per part, and the finishing launch (mode 2)
// (dA: the `nstarts` blocks in device memory, `nruns` runs each)
static void rank_launch(mrbf_ctx *ctx, const ps::Args *dA, int nstarts, int nruns, int gen, const RankLaunch &L, bool phases_possible) {
    using namespace ps;
    const unsigned NS = (unsigned)nstarts, NR = (unsigned)nruns;
    hipLaunchKernelGGL(ps_rank_kernel, dim3(NR, NS), dim3(L.threads), L.shm, ctx->stream, dA, gen, L.several ? 1 : 0, L.ws);
    if (!L.several) return;
    const int draw_blocks = (int)std::min<size_t>(512, (L.draws_per_run + 255) / 256);
    const int count_blocks = ((L.maxlam + RW_CNT_T - 1) / RW_CNT_T) * rw_jsplit(L.maxlam);
    hipLaunchKernelGGL(ps_rank_prep_kernel, dim3((unsigned)(draw_blocks + count_blocks), NR, NS), dim3(256), 0, ctx->stream, dA, gen, L.ws, L.draws, L.draws_per_run, draw_blocks);
    if (phases_possible)  // (runs without modelled or linear constraints -- ideal-point runs of a box-constrained problem -- never violate anything)
        hipLaunchKernelGGL(ps_rank_wave_kernel, dim3((unsigned)rw_waves(L.maxlam), NR, NS), dim3(64), 0, ctx->stream, dA, L.ws, L.draws, L.draws_per_run, ++ctx->ps_rank_epoch);
    hipLaunchKernelGGL(ps_rank_kernel, dim3(NR, NS), dim3(L.threads), L.shm, ctx->stream, dA, gen, 2, L.ws);
}

// A downloaded evaluation of m points into allF (row-major m x nftot) and, where Jobj is given, the objectives' Jacobian rows
// ([point][objective][coordinate]).  blocks: model j's m x k_j values at m * foff[j]; Jm[j]: model j's Jacobians, per point k_j x d
// column-major (read for the objectives' models only).
static void ps_unpack_eval(const ps::Problem &P, int m, const double *blocks, const double *const *Jm, std::vector<double> &allF,
                           std::vector<double> *Jobj) {
    const int d = P.d;
    allF.resize((size_t)m * P.nftot);
    for (int j = 0; j < P.nmodels; ++j) {
        const int kj = P.models[j]->k;
        for (int p = 0; p < m; ++p)
            for (int c = 0; c < kj; ++c) allF[(size_t)p * P.nftot + P.foff[j] + c] = blocks[(size_t)m * P.foff[j] + (size_t)p * kj + c];
    }
    if (!Jobj) return;
    Jobj->resize((size_t)m * P.nobj * d);
    for (int p = 0; p < m; ++p)
        for (int l = 0; l < P.nobj; ++l) {
            const int j = P.obj_model[l], kj = P.models[j]->k;
            const double *Jp = Jm[j] + (size_t)p * kj * d;
            for (int t = 0; t < d; ++t) (*Jobj)[((size_t)p * P.nobj + l) * d + t] = Jp[(size_t)t * kj + P.obj_col[l]];
        }
}

// all model outputs at m points (row-major m x nftot) and, optionally (m == 1), the objectives' Jacobian rows
static int ps_eval_points(mrbf_ctx *ctx, const ps::Problem &P, const double *x_host, int m, std::vector<double> &allF, std::vector<double> *Jobj) {
    const int d = P.d;
    double *dX;
    size_t cnt = (size_t)m * d + (size_t)m * P.nftot;
    for (int j = 0; j < P.nmodels; ++j) cnt += (size_t)(Jobj ? m : 1) * P.models[j]->k * d;
    MRBF_TRY(get_buf(ctx, S_PS_POLISH, cnt, &dX));
    double *dV = dX + (size_t)m * d, *dJ = dV + (size_t)m * P.nftot;
    // The descent phase calls this some 140 times per step with a few KB each way.  Transfers from / to pageable memory are a
    // synchronous round trip of their own (round 6: 285 copies = a sixth of the d = 128 step): the points go up and the values /
    // Jacobians come down through the context's pinned block (free during a PS step: no entry point arms it here), enqueued
    // asynchronously in front of ONE stream synchronisation.
    const size_t up_cnt = (size_t)m * d, down_cnt = cnt - up_cnt;
    double *pin = (ctx->pin_base && !ctx->pin_armed && cnt * sizeof(double) <= ((size_t)1 << 20)) ? reinterpret_cast<double *>(ctx->pin_base) : nullptr;
    // Round 6, second half: no copies at all.  The pinned block is mapped into the device's address space, so the kernels read the
    // points from it and write values / Jacobians into it (a few KB over the link inside kernels that run anyway) -- two blit launches
    // and their gaps less per call, ~75 calls per step (MRBF_PS_ZEROCOPY=0: the staged copies).
    static const int zc_env = mrbf_env("MRBF_PS_ZEROCOPY") ? atoi(mrbf_env("MRBF_PS_ZEROCOPY")) : 1;
    const bool zero_copy = pin && zc_env;
    if (zero_copy) {
        std::memcpy(pin, x_host, up_cnt * sizeof(double));
        dX = pin;
        dV = pin + up_cnt;
        dJ = dV + (size_t)m * P.nftot;
    } else if (pin) {
        std::memcpy(pin, x_host, up_cnt * sizeof(double));
        MRBF_HIP(ctx, hipMemcpyAsync(dX, pin, up_cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    } else {
        MRBF_HIP(ctx, hipMemcpyAsync(dX, x_host, up_cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<double *> jp(P.nmodels, nullptr), vp(P.nmodels, nullptr);
    for (int j = 0; j < P.nmodels; ++j) {
        jp[j] = Jobj && P.model_has_objective(j) ? dJ : nullptr;
        vp[j] = dV + (size_t)m * P.foff[j];  // model j's m x k_j block
        MRBF_TRY(eval_model(ctx, P.models[j], m, dX, vp[j], jp[j], nullptr));
        dJ += (size_t)(Jobj ? m : 1) * P.models[j]->k * d;
    }
    std::vector<double> blocks_v;
    std::vector<std::vector<double>> Jm_v(P.nmodels);
    const double *blocks;
    std::vector<const double *> Jm(P.nmodels, nullptr);
    if (pin) {
        double *down = pin + up_cnt;  // the values, then every model's Jacobian block at its device offset: one download
        if (!zero_copy) MRBF_HIP(ctx, hipMemcpyAsync(down, dV, down_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        blocks = down;
        for (int j = 0; j < P.nmodels; ++j)
            if (jp[j]) Jm[j] = down + (jp[j] - dV);
    } else {
        blocks_v.resize((size_t)m * P.nftot);
        MRBF_HIP(ctx, hipMemcpyAsync(blocks_v.data(), dV, blocks_v.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        blocks = blocks_v.data();
        for (int j = 0; j < P.nmodels; ++j)
            if (jp[j]) {
                Jm_v[j].resize((size_t)m * P.models[j]->k * d);
                MRBF_HIP(ctx, hipMemcpyAsync(Jm_v[j].data(), jp[j], Jm_v[j].size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                Jm[j] = Jm_v[j].data();
            }
    }
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ps_unpack_eval(P, m, blocks, Jm.data(), allF, Jobj);
    return 0;
}

// one evaluation of the refinement: all model outputs of problem P at m points (and the objectives' Jacobian rows)
struct EvalReq {
    const ps::Problem *P;
    const double *x;
    int m;
    std::vector<double> *allF, *Jobj;  // Jobj may be null
};
// The evaluations of several starts' points as ONE chain: a packed upload (points, descriptors), one launch group per (kernel and
// parameters, k, dpad, Jacobians or not, split or unsplit centre range), one download, one synchronisation.  Every member keeps the
// query count -- hence the split of the centre range and the order of every sum -- of the ps_eval_points call it stands for.  A single
// request takes that call itself.
static int ps_eval_points_many(mrbf_ctx *ctx, std::vector<EvalReq> &reqs) {
    if (reqs.empty()) return 0;
    if (reqs.size() == 1) return ps_eval_points(ctx, *reqs[0].P, reqs[0].x, reqs[0].m, *reqs[0].allF, reqs[0].Jobj);
    const size_t R = reqs.size();
    chain::Plan ev;
    chain::Arena ar;
    std::vector<size_t> oX(R), oV(R), oJ(R * ps::MAXMODELS, 0);
    for (size_t i = 0; i < R; ++i) {
        const ps::Problem &P = *reqs[i].P;
        oX[i] = ar.take((size_t)reqs[i].m * P.d);
        for (int j = 0; j < P.nmodels; ++j) ev.add(ctx, 0, (int64_t)i, j, P.models[j], reqs[i].m, reqs[i].Jobj && P.model_has_objective(j));
    }
    ev.close();
    const size_t oDesc = ar.take(ev.desc_doubles());
    const size_t up_cnt = ar.total;
    for (size_t i = 0; i < R; ++i) oV[i] = ar.take((size_t)reqs[i].m * reqs[i].P->nftot);
    for (const chain::Member &mb : ev.mem)
        if (mb.jac) oJ[(size_t)mb.p * ps::MAXMODELS + mb.j] = ar.take((size_t)mb.mq * mb.M->k * mb.M->d);
    const size_t down_cnt = ar.total - up_cnt;
    ev.carve(ar);
    for (chain::Member &mb : ev.mem) {
        const ps::Problem &P = *reqs[mb.p].P;
        mb.X = oX[mb.p];
        mb.vals = oV[mb.p] + (size_t)mb.mq * P.foff[mb.j];  // model j's m x k_j block
        mb.jacs = oJ[(size_t)mb.p * ps::MAXMODELS + mb.j];
    }
    double *base;
    MRBF_TRY(get_buf(ctx, S_PS_POLISH, ar.total, &base));
    // (the context's pinned block is free during a PS step: no entry point arms it here)
    double *pin = (ctx->pin_base && !ctx->pin_armed && (up_cnt + down_cnt) * sizeof(double) <= ((size_t)6 << 20)) ? reinterpret_cast<double *>(ctx->pin_base) : nullptr;
    std::vector<double> own;
    if (!pin) own.resize(up_cnt + down_cnt);
    double *hup = pin ? pin : own.data(), *hdown = hup + up_cnt;
    for (size_t i = 0; i < R; ++i) std::memcpy(hup + oX[i], reqs[i].x, (size_t)reqs[i].m * reqs[i].P->d * sizeof(double));
    EvalDesc *hdesc = reinterpret_cast<EvalDesc *>(hup + oDesc);
    ev.fill(base, hdesc);
    MRBF_HIP(ctx, hipMemcpyAsync(base, hup, up_cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MRBF_TRY(ev.launch(ctx, 0, base, hdesc, reinterpret_cast<const EvalDesc *>(base + oDesc)));
    MRBF_HIP(ctx, hipMemcpyAsync(hdown, base + up_cnt, down_cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < R; ++i) {
        const ps::Problem &P = *reqs[i].P;
        const double *Jm[ps::MAXMODELS] = {};
        for (int j = 0; j < P.nmodels; ++j)
            if (reqs[i].Jobj && P.model_has_objective(j)) Jm[j] = hdown + (oJ[i * ps::MAXMODELS + j] - up_cnt);
        ps_unpack_eval(P, reqs[i].m, hdown + (oV[i] - up_cnt), Jm, *reqs[i].allF, reqs[i].Jobj);
    }
    return 0;
}

// the descents of one start: they advance in lockstep through one evaluation per iteration (12 points per active descent)
struct DescentGroup {
    const ps::Problem *P = nullptr;
    std::vector<Descent> ds;
    // per iteration
    std::vector<int> who;
    std::vector<double> X, allF, J;
};
// The descents of all groups in lockstep: per iteration ONE chain of evaluations and one host synchronisation for all groups together
// (ps_eval_points_many).  A group's own sequence of evaluations -- which descents are active, how many points -- is what it would be alone.
static int ps_descend_groups(mrbf_ctx *ctx, std::vector<DescentGroup> &gs) {
    constexpr int NSTEP = Descent::NSTEP;
    std::vector<EvalReq> reqs;
    // the start points (values + Jacobian rows)
    for (DescentGroup &G : gs) {
        const size_t d = (size_t)G.P->d;
        for (auto &D : G.ds) D.start();
        G.who.clear();
        for (size_t i = 0; i < G.ds.size(); ++i)
            if (G.ds[i].wants_start_eval()) G.who.push_back((int)i);
        if (G.who.empty()) continue;
        G.X.resize(G.who.size() * d);
        for (size_t w = 0; w < G.who.size(); ++w) std::copy(G.ds[G.who[w]].x.begin(), G.ds[G.who[w]].x.end(), G.X.begin() + w * d);
        reqs.push_back(EvalReq{G.P, G.X.data(), (int)G.who.size(), &G.allF, &G.J});
    }
    MRBF_TRY(ps_eval_points_many(ctx, reqs));
    for (DescentGroup &G : gs)
        for (size_t w = 0; w < G.who.size(); ++w)
            G.ds[G.who[w]].take_start(&G.allF[w * (size_t)G.P->nftot], &G.J[w * (size_t)G.P->nobj * G.P->d]);
    for (;;) {
        reqs.clear();
        for (DescentGroup &G : gs) {
            const size_t d = (size_t)G.P->d;
            G.who.clear();
            for (size_t i = 0; i < G.ds.size(); ++i)
                if (G.ds[i].trials()) G.who.push_back((int)i);
            if (G.who.empty()) continue;
            G.X.resize(G.who.size() * (size_t)NSTEP * d);
            for (size_t w = 0; w < G.who.size(); ++w) std::copy(G.ds[G.who[w]].XT.begin(), G.ds[G.who[w]].XT.end(), G.X.begin() + w * (size_t)NSTEP * d);
            reqs.push_back(EvalReq{G.P, G.X.data(), (int)G.who.size() * NSTEP, &G.allF, &G.J});
        }
        if (reqs.empty()) break;
        MRBF_TRY(ps_eval_points_many(ctx, reqs));
        for (DescentGroup &G : gs)
            for (size_t w = 0; w < G.who.size(); ++w)
                G.ds[G.who[w]].consume(&G.allF[w * (size_t)NSTEP * G.P->nftot], &G.J[w * (size_t)NSTEP * G.P->nobj * G.P->d]);
    }
    return 0;
}

static int fetch_host(mrbf_ctx *ctx, const double *src, size_t cnt, std::vector<double> &dst) {
    dst.resize(cnt);
    return input_fetch(ctx, src, cnt, dst.data());
}

// one start of a step: the host view of its container, its inputs and what the step returns for it
struct PsStart {
    ps::Problem P;
    std::vector<double> hlb, hub, hxn, hfx, r, mx, xt;
    std::vector<double> ideal, x_ideal;  // the ideal-point phase: its value per objective and (k x d) where that value was found
    std::vector<char> found, refined;    // per objective: the run met a feasible point; a refinement of its best point ran
    unsigned long long seed = 0;
    mrbf_ps_info info{};
    ps::Args a{};  // its block of the current phase
};

// the function table of a container from the roles table's layout and one start's handles
static void ps_problem_fill(ps::Problem &P, const descent::Layout &lay, const mrbf_ps_problem *prob, const mrbf_model *const *models) {
    P.nmodels = prob->n_models;
    P.nobj = prob->n_objectives;
    P.d = lay.d;
    for (int j = 0; j < P.nmodels; ++j) {
        P.models[j] = models[j];
        P.foff[j] = P.nftot;
        P.nftot += lay.k[j];
    }
    for (int l = 0; l < P.nobj; ++l) P.obj_model[l] = lay.obj[l].slot, P.obj_col[l] = lay.obj[l].col;
    for (const descent::Row &r : lay.rows) {
        P.con_model[P.ncon] = r.slot, P.con_col[P.ncon] = r.col, P.con_eq[P.ncon] = r.eq;
        ++P.ncon;
    }
    P.nlin_eq = prob->n_lin_eq;
    P.nlin_ineq = prob->n_lin_ineq;
    P.eq_tol = prob->eq_tol >= 0.0 ? prob->eq_tol : 1e-8;
}

// doubles of device memory a start of the step takes in the state slot (run state, evaluation batch, results and the sweeps' scratch):
// the chunk loop sizes its chunks of starts with it.  An estimate of "the state": the ranking's work space (S_PS_RANK: only while
// at most 16 runs share a launch) and the refinement's chain (S_PS_POLISH: a few points per start) are not counted.
static size_t ps_start_doubles(const mrbf_ctx *ctx, const mrbf_model *const *models, int nm, int d, int k, int nftot, bool need_ideal,
                               bool with_ps) {
    const ps::Sizes z = ps::sizes(d, k, need_ideal, with_ps);
    size_t scratch = 0;  // of the larger sweep: centred queries, their norms and the partial sums of a split centre range, per model slot
    for (size_t m : {(size_t)(need_ideal ? k * z.lam_ip : 0), (size_t)z.lam_ps}) {
        size_t s = 0;
        for (int j = 0; j < nm && m; ++j) {
            const size_t mpad = (size_t)round_up((int64_t)m, 64);
            const int nsplit = eval_nsplit(ctx, (int64_t)m, (int)((models[j]->n + 63) / 64), false, true);
            s += mpad * (models[j]->dpad + 1) + (nsplit > 1 ? (size_t)nsplit * mpad * 2 * 2 : 0) + 64;
        }
        scratch = std::max(scratch, s);
    }
    return (size_t)z.rows * (d + nftot) + z.state + scratch + 4096;
}

// ---- The step for the starts of S (the single calls: one; the batch calls: a batch, or a chunk of one): the phases of
// get_criticality(::PascolettiSerafiniConfig, ...) for all starts together, as functions over one PsCall -- ps_open, then
// ps_ideal_phase where no direction was given, then ps_step_phase, then ps_close; the ideal-point calls open without room for the PS
// run and leave ps_step_phase out.  Per generation ONE population sweep per launch group, the optional score launch, the ranking and
// the breeding for every run of every start that takes part in the phase; the refinements advance in lockstep.  Nothing a start
// computes depends on another start: its block, its runs' indices and its seed are its own, a finished run is inert in every kernel
// (R.stat[1], R.stat[3] != gen + 1), the evaluations keep the single call's query counts.  Where a piece lies in the arena changes
// nothing a kernel computes.
enum { SITE_IP = 0, SITE_PS = 1 };
struct PsCall {
    mrbf_ctx *ctx = nullptr;
    std::vector<PsStart> *S = nullptr;
    const mrbf_ps_options *opts = nullptr;
    size_t N = 0;
    bool single = false;  // the one start's evaluations are eval_model's own launches (its arena slots, its pinned block)
    int d = 0, k = 0, nm = 0, nftot = 0;
    ps::Sizes sz{};
    // device arena: linear constraints, the starts' blocks, boxes and start points, mx, r, the runs' best records, then per start the
    // evaluation batch, its results and the runs' state; in a batch also the sweeps' descriptors and scratch (batch_chain.hpp)
    size_t oLin = 0, oArgs = 0, oBox = 0, oMx = 0, oR = 0, oBest = 0, oDesc = 0;
    std::vector<size_t> oStart;
    double *base = nullptr;
    int *stat = nullptr;
    const ps::Args *dA = nullptr;
    const double *dlin[4] = {};  // A_eq, b_eq, A_ineq, b_ineq in the arena
    chain::Plan ev_ip, ev_ps_all, ev_ps;  // the sweeps of the two phases over all starts; the PS sweep of the starts that take part
    int max_ip = 0, max_ps = 0, res_ip = 0, res_ps = 0;
    double xtol = 0.0;
    int dbg = 0;
    // host staging: sources and targets of asynchronous copies, alive for the whole call
    std::vector<double> hbox, hmx, hr, hbest;
    std::vector<ps::Args> harr;
    std::vector<EvalDesc> hdesc;
    std::vector<int> hs;
    std::vector<std::vector<double>> allF;  // m(x_n), later m(x_trial), per start
};

// the part of start p's state behind the evaluation batch and its results: where the runs of a phase are laid out
static double *ps_runs_at(const PsCall &c, size_t p) { return c.base + c.oStart[p] + (size_t)c.sz.rows * c.d + (size_t)c.sz.rows * c.nftot; }

static void ps_make_run(ps::Run &R, int kind, int obj, int lam, int nvar, int off, int max_evals, double *&p, double *best, int *stp) {
    R.kind = kind, R.obj = obj, R.lam = lam, R.mu = (lam + 6) / 7, R.nvar = nvar, R.off = off, R.max_evals = max_evals;
    for (int b = 0; b < 2; ++b) {
        R.X[b] = p, p += (size_t)lam * nvar;
        R.S[b] = p, p += (size_t)lam * nvar;
    }
    R.f = p, p += lam;
    R.phi = p, p += lam;
    R.order = (int *)p, p += lam;
    R.best = best, R.stat = stp;
}

// the block of start p (everything but the runs)
static void ps_make_args(const PsCall &c, size_t p) {
    const int d = c.d, k = c.k;
    PsStart &s = (*c.S)[p];
    const ps::Problem &P = s.P;
    ps::Args &a = s.a;
    a = ps::Args{};
    a.d = d, a.nobj = k;
    a.lb = c.base + c.oBox + p * 3 * d, a.ub = a.lb + d, a.xn = a.ub + d;
    a.mx = c.base + c.oMx + p * k;
    a.r = c.base + c.oR + p * k;
    a.nmodels = c.nm;
    double *fp = c.base + c.oStart[p] + (size_t)c.sz.rows * d;
    for (int j = 0; j < c.nm; ++j) {
        a.F[j] = fp;
        a.kf[j] = P.models[j]->k;
        fp += (size_t)c.sz.rows * P.models[j]->k;
    }
    for (int l = 0; l < k; ++l) a.obj_model[l] = (short)P.obj_model[l], a.obj_col[l] = (short)P.obj_col[l];
    a.ncon = P.ncon;
    for (int q = 0; q < P.ncon; ++q) a.con_model[q] = (short)P.con_model[q], a.con_col[q] = (short)P.con_col[q], a.con_eq[q] = (short)P.con_eq[q];
    a.nlin_eq = P.nlin_eq, a.nlin_ineq = P.nlin_ineq;
    a.A_eq = c.dlin[0], a.b_eq = c.dlin[1], a.A_ineq = c.dlin[2], a.b_ineq = c.dlin[3];
    a.eq_tol = P.eq_tol;
    a.Xeval = c.base + c.oStart[p];
    a.seed = s.seed, a.dbg = c.dbg, a.xtol_rel = c.xtol;
}

// Opening: the arena for the phases that will run (with_ideal: the k single-objective runs; with_ps: the PS run), the uploads,
// mx = m(x_n), the budgets and the starts' blocks.
static int ps_open(PsCall &c, mrbf_ctx *ctx, std::vector<PsStart> &S, const mrbf_ps_options *opts, bool with_ideal, bool with_ps) {
    using namespace ps;
    c.ctx = ctx, c.S = &S, c.opts = opts;
    const size_t N = c.N = S.size();
    c.single = N == 1;
    const Problem &P0 = S[0].P;
    const int d = c.d = P0.d, k = c.k = P0.nobj, nm = c.nm = P0.nmodels;
    c.nftot = P0.nftot;
    hipStream_t st = ctx->stream;
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    const Sizes &z = c.sz = sizes(d, k, with_ideal, with_ps);
    const size_t nlin = (size_t)P0.nlin_eq + P0.nlin_ineq;
    const size_t args_dbl = (sizeof(Args) + sizeof(double) - 1) / sizeof(double);
    chain::Arena ar;
    c.oLin = ar.take(nlin * (d + 1)), c.oArgs = ar.take(N * args_dbl), c.oBox = ar.take(N * 3 * d), c.oMx = ar.take(N * k), c.oR = ar.take(N * k);
    c.oBest = ar.take(N * z.best_per);
    const size_t start_cnt = (size_t)z.rows * d + (size_t)z.rows * c.nftot + z.state;
    c.oStart.resize(N);
    for (size_t p = 0; p < N; ++p) c.oStart[p] = ar.take(start_cnt);
    if (!c.single) {
        for (size_t p = 0; p < N && with_ideal; ++p)
            for (int j = 0; j < nm; ++j) c.ev_ip.add(ctx, SITE_IP, (int64_t)p, j, S[p].P.models[j], (int64_t)k * z.lam_ip, false, true);
        for (size_t p = 0; p < N && with_ps; ++p)
            for (int j = 0; j < nm; ++j) c.ev_ps_all.add(ctx, SITE_PS, (int64_t)p, j, S[p].P.models[j], z.lam_ps, false, true);
        c.ev_ip.close();
        c.ev_ps_all.close();
        c.oDesc = ar.take(std::max(c.ev_ip.desc_doubles(), c.ev_ps_all.desc_doubles()));
        chain::Arena a0, a1;  // (the two phases follow each other: their scratch shares its place)
        a0.total = a1.total = ar.total;
        c.ev_ip.carve(a0);
        c.ev_ps_all.carve(a1);
        ar.total = std::max(a0.total, a1.total);
        for (chain::Plan *pl : {&c.ev_ip, &c.ev_ps_all})
            for (chain::Member &mb : pl->mem) {
                mb.X = c.oStart[mb.p];
                mb.vals = c.oStart[mb.p] + (size_t)z.rows * d + (size_t)z.rows * P0.foff[mb.j];
            }
    }
    MRBF_TRY(get_buf(ctx, S_PS_STATE, ar.total + 64, &c.base));
    MRBF_TRY(get_buf(ctx, S_PS_STAT, (size_t)4 * std::max((size_t)MAXRUNS, N * (size_t)k), &c.stat));
    double *base = c.base;
    c.dA = reinterpret_cast<const Args *>(base + c.oArgs);
    c.hbox.resize(N * 3 * d), c.hmx.resize(N * k), c.hr.resize(N * k);
    for (size_t p = 0; p < N; ++p) {
        std::copy(S[p].hlb.begin(), S[p].hlb.end(), c.hbox.begin() + p * 3 * d);
        std::copy(S[p].hub.begin(), S[p].hub.end(), c.hbox.begin() + p * 3 * d + d);
        std::copy(S[p].hxn.begin(), S[p].hxn.end(), c.hbox.begin() + p * 3 * d + 2 * d);
    }
    MRBF_HIP(ctx, hipMemcpyAsync(base + c.oBox, c.hbox.data(), c.hbox.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const std::vector<double> *lin[4] = {&P0.lin->A_eq, &P0.lin->b_eq, &P0.lin->A_ineq, &P0.lin->b_ineq};
    double *dl = base + c.oLin;
    for (int q = 0; q < 4; dl += lin[q++]->size()) {
        c.dlin[q] = dl;
        if (!lin[q]->empty()) MRBF_HIP(ctx, hipMemcpyAsync(dl, lin[q]->data(), lin[q]->size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // mx = m(x_n)  (descent.jl:543)
    c.allF.resize(N);
    std::vector<EvalReq> reqs;
    for (size_t p = 0; p < N; ++p) reqs.push_back(EvalReq{&S[p].P, S[p].hxn.data(), 1, &c.allF[p], nullptr});
    MRBF_TRY(ps_eval_points_many(ctx, reqs));
    for (size_t p = 0; p < N; ++p) {
        S[p].mx.resize(k);
        for (int l = 0; l < k; ++l) S[p].mx[l] = c.hmx[p * k + l] = S[p].P.objective(c.allF[p], l);
    }
    MRBF_HIP(ctx, hipMemcpyAsync(base + c.oMx, c.hmx.data(), c.hmx.size() * sizeof(double), hipMemcpyHostToDevice, st));
    c.max_ip = budget(opts->max_ideal_evals, d);  // descent.jl:527
    c.max_ps = budget(opts->max_ps_evals, d);     // descent.jl:416
    // (a polish with a budget of its own leaves the PS run its whole budget)
    c.res_ip = reserve(c.max_ip), c.res_ps = opts->max_polish_evals > 0 ? 0 : reserve(c.max_ps);
    c.xtol = opts->xtol_rel > 0.0 ? opts->xtol_rel : 1e-3;  // descent.jl:379, :485
    c.dbg = (mrbf_env("MRBF_PS_DBG") ? atoi(mrbf_env("MRBF_PS_DBG")) : 0) & DBG_ALL;
    for (size_t p = 0; p < N; ++p) ps_make_args(c, p);
    c.hbest.resize(N * z.best_per);
    c.hs.resize((size_t)4 * std::max((size_t)MAXRUNS, N * (size_t)k));
    return MRBF_OK;
}

// Generations of one phase: the runs of the starts `act` (their blocks' runs are set), generation by generation until every run of
// every start is done
static int ps_generations(PsCall &c, const std::vector<size_t> &act, const chain::Plan *plan, int site, double t0, int max_gens) {
    using namespace ps;
    mrbf_ctx *ctx = c.ctx;
    std::vector<PsStart> &S = *c.S;
    hipStream_t st = ctx->stream;
    double *base = c.base;
    const Args *dA = c.dA;
    const int nm = c.nm;
    const int NA = (int)act.size();
    const Args &a0 = S[act[0]].a;
    const int nruns = a0.nruns;
    int maxel = 0, nrows = 0;
    for (int q2 = 0; q2 < nruns; ++q2) {
        nrows = std::max(nrows, a0.runs[q2].off + a0.runs[q2].lam);
        maxel = std::max(maxel, a0.runs[q2].lam * a0.runs[q2].nvar);
    }
    // large populations: the transposition phases with one wave per 64 individuals (MRBF_PS_MULTI=0, read per call: one workgroup per
    // run as in rounds 3 / 4) while ALL runs of the launch can be resident together -- their waves wait for each other; beyond that
    // count every run takes the one-workgroup ranking, and the many runs are the parallelism.  A counter wait that times out -- a
    // device shared with other work -- costs 5 ms; the host sees the sticky failure word with the status words, every eight
    // generations, and keeps to one workgroup per run from then on.
    const bool multi_env = !(mrbf_env("MRBF_PS_MULTI") && atoi(mrbf_env("MRBF_PS_MULTI")) == 0);
    RankLaunch L;
    MRBF_TRY(rank_launch_setup(ctx, a0, NA, (int64_t)ctx->ncu >= (int64_t)RS_CUS_PER_RUN * nruns * NA && !ctx->ps_multi_off && multi_env, L));
    bool phases_possible = a0.ncon + a0.nlin_eq + a0.nlin_ineq > 0 || (a0.dbg & DBG_PHASES);
    for (int q2 = 0; q2 < nruns; ++q2) phases_possible = phases_possible || a0.runs[q2].kind == 1;
    // one model, fused evaluation: the breeding kernel writes the next population centred and padded into the evaluation's own query
    // buffers (a launch per generation less; MRBF_PS_FUSEPAD=0: the evaluation's centring launch).  The one start's buffers are the
    // arena slots the evaluation will ask for -- same size, same pointer; eval_fused checks that and centres itself otherwise; a
    // batch's are its members' own.
    const int fusepad = mrbf_env("MRBF_PS_FUSEPAD") ? atoi(mrbf_env("MRBF_PS_FUSEPAD")) : 1;  // (read per call: the tests switch it inside one process)
    const int score_fused = (a0.nlin_eq + a0.nlin_ineq == 0 && !(mrbf_env("MRBF_PS_FUSESCORE") && atoi(mrbf_env("MRBF_PS_FUSESCORE")) == 0)) ? 1 : 0;
    bool fused = fusepad && nm == 1 && ctx->eval_impl != 1 && c.d <= 360;
    for (int i = 0; i < NA && fused; ++i) {
        const int dp = S[act[i]].P.models[0]->dpad;
        fused = dp == 64 || dp == 128 || dp == 256;
    }
    double *xq1 = nullptr, *xsq1 = nullptr;
    if (fused && c.single) {
        const int64_t mpad = round_up((int64_t)nrows, 64);
        MRBF_TRY(get_buf(ctx, S_EVAL_XC, (size_t)mpad * S[0].P.models[0]->dpad, &xq1));
        MRBF_TRY(get_buf(ctx, S_EVAL_XSQ, (size_t)mpad, &xsq1));
    }
    c.harr.resize(NA);
    for (int i = 0; i < NA; ++i) {
        Args &a = S[act[i]].a;
        a.rows = nrows, a.t0 = t0, a.grun0 = i * nruns, a.score_fused = score_fused;
        a.Xq = a.xsq = nullptr, a.xmean = nullptr, a.xqD = 0;
        if (fused) {
            const mrbf_model *M0 = S[act[i]].P.models[0];
            a.Xq = c.single ? xq1 : base + plan->mem[(size_t)i * nm].Xq;
            a.xsq = c.single ? xsq1 : base + plan->mem[(size_t)i * nm].xsq;
            a.xmean = M0->mean;
            a.xqD = M0->dpad;
        }
        c.harr[i] = a;
    }
    MRBF_HIP(ctx, hipMemcpyAsync(base + c.oArgs, c.harr.data(), (size_t)NA * sizeof(Args), hipMemcpyHostToDevice, st));
    const EvalDesc *ddesc = reinterpret_cast<const EvalDesc *>(base + c.oDesc);
    if (!c.single) {
        c.hdesc.resize(plan->n_desc);
        plan->fill(base, c.hdesc.data());
        if (plan->n_desc) MRBF_HIP(ctx, hipMemcpyAsync(base + c.oDesc, c.hdesc.data(), plan->n_desc * sizeof(EvalDesc), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(ps_init_kernel, dim3((unsigned)((maxel + 255) / 256), (unsigned)nruns, (unsigned)NA), dim3(256), 0, st, dA);
    std::vector<int> hstat((size_t)4 * nruns * NA);
    const unsigned wave_blocks = (unsigned)((nrows + 3) / 4);
    for (int g = 0; g < max_gens; ++g) {
        // (generation 0 comes from ps_init_kernel: centred by the evaluation's own launch)
        if (c.single) {
            EvalHints hints;
            hints.population = true;
            hints.pre_xq = (g > 0 && fused) ? xq1 : nullptr;
            for (int j = 0; j < nm; ++j) MRBF_TRY(eval_model(ctx, S[0].P.models[j], nrows, a0.Xeval, const_cast<double *>(a0.F[j]), nullptr, nullptr, hints));
        } else {
            MRBF_TRY(plan->launch(ctx, site, base, c.hdesc.data(), ddesc, g > 0 && fused));
        }
        if (!score_fused) hipLaunchKernelGGL(ps_score_kernel, dim3(wave_blocks, (unsigned)NA), dim3(256), 0, st, dA, g);
        rank_launch(ctx, dA, NA, nruns, g, L, phases_possible);
        hipLaunchKernelGGL(ps_breed_kernel, dim3(wave_blocks, (unsigned)NA), dim3(256), 0, st, dA, g);
        if ((g & 7) == 7 || g + 1 == max_gens) {  // status words every 8 generations: stop when every run of every start is done
            MRBF_HIP(ctx, hipMemcpyAsync(hstat.data(), c.stat, hstat.size() * sizeof(int), hipMemcpyDeviceToHost, st));
            int hfail = 0;
            if (L.several) MRBF_HIP(ctx, hipMemcpyAsync(&hfail, L.ws.sticky, sizeof(int), hipMemcpyDeviceToHost, st));
            MRBF_HIP(ctx, hipStreamSynchronize(st));
            if (hfail && !(a0.dbg & DBG_GIVE_UP)) {
                L.several = false;
                ctx->ps_multi_off = 1;
            }
            bool all = true;
            for (size_t q2 = 0; q2 < hstat.size() / 4; ++q2) all = all && hstat[4 * q2 + 1] != 0;
            if (all) break;
        }
    }
    MRBF_HIP(ctx, hipGetLastError());
    return 0;
}

// Ideal phase -- the local ideal point: the k single-objective minimisations of every start side by side (descent.jl:404-412) and the
// refinement of their best points.  Every start's ideal, x_ideal, found, refined and info.evals_ideal / generations are set.
static int ps_ideal_phase(PsCall &c) {
    mrbf_ctx *ctx = c.ctx;
    std::vector<PsStart> &S = *c.S;
    hipStream_t st = ctx->stream;
    const size_t N = c.N, best_per = c.sz.best_per;
    const int d = c.d, k = c.k, lam_ip = c.sz.lam_ip;
    std::vector<size_t> act(N);
    for (size_t p = 0; p < N; ++p) {
        act[p] = p;
        ps::Args &a = S[p].a;
        double *pp = ps_runs_at(c, p);
        a.nruns = k;
        for (int l = 0; l < k; ++l)
            ps_make_run(a.runs[l], 0, l, lam_ip, d, l * lam_ip, c.max_ip - c.res_ip, pp, c.base + c.oBest + p * best_per + (size_t)l * (d + 2), c.stat + 4 * (p * k + l));
    }
    MRBF_TRY(ps_generations(c, act, &c.ev_ip, SITE_IP, 0.0, (c.max_ip - c.res_ip + lam_ip - 1) / lam_ip + 1));
    MRBF_HIP(ctx, hipMemcpyAsync(c.hbest.data(), c.base + c.oBest, c.hbest.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    MRBF_HIP(ctx, hipMemcpyAsync(c.hs.data(), c.stat, (size_t)4 * N * k * sizeof(int), hipMemcpyDeviceToHost, st));
    MRBF_HIP(ctx, hipStreamSynchronize(st));
    // A run that never met a feasible point contributes its start value.  The runs' best points are refined by gradient steps on
    // their objective -- all descents of all starts in lockstep, one chain of evaluations per iteration
    std::vector<DescentGroup> gs;
    std::vector<std::pair<size_t, int>> dl;  // (start, objective) of every descent, group by group
    for (size_t p = 0; p < N; ++p) {
        DescentGroup G;
        G.P = &S[p].P;
        S[p].ideal.assign(k, 0.0);
        S[p].x_ideal.assign((size_t)k * d, 0.0);
        S[p].found.assign(k, 0), S[p].refined.assign(k, 0);
        for (int l = 0; l < k; ++l) {
            const double *b = &c.hbest[p * best_per + (size_t)l * (d + 2)];
            const int *h = &c.hs[4 * (p * k + l)];
            const bool found = b[d + 1] == 0.0 && std::isfinite(b[d]);
            S[p].ideal[l] = found ? b[d] : S[p].mx[l];
            S[p].found[l] = found;
            std::copy_n(found ? b : S[p].hxn.data(), d, S[p].x_ideal.begin() + (size_t)l * d);
            S[p].info.evals_ideal += h[0];
            S[p].info.generations += h[2];
            const int left = c.max_ip - h[0];
            if (found && left >= 13) {
                G.ds.push_back(descent_of_objective(&S[p].P, &S[p].hlb, &S[p].hub, l, b, S[p].ideal[l], left, c.xtol));
                dl.emplace_back(p, l);
            }
        }
        if (!G.ds.empty()) gs.push_back(std::move(G));
    }
    MRBF_TRY(ps_descend_groups(ctx, gs));
    size_t at = 0;
    for (DescentGroup &G : gs)
        for (Descent &D : G.ds) {
            PsStart &s = S[dl[at].first];
            const int l = dl[at].second;
            s.ideal[l] = D.val;  // (D.x is where D.val was taken: they change together)
            std::copy(D.x.begin(), D.x.end(), s.x_ideal.begin() + (size_t)l * d);
            s.refined[l] = D.evals > 0;
            s.info.evals_ideal += D.evals;
            ++at;
        }
    return MRBF_OK;
}

// PS phase: the direction where the ideal phase ran (r = f(x_n) - ideal point, descent.jl:536-538), the criticality test, the
// Pascoletti-Serafini runs of the starts that are not critical, their polish, and mx_trial = m(x_trial).
static int ps_step_phase(PsCall &c, bool r_from_ideal) {
    mrbf_ctx *ctx = c.ctx;
    std::vector<PsStart> &S = *c.S;
    const mrbf_ps_options *opts = c.opts;
    hipStream_t st = ctx->stream;
    const size_t N = c.N, best_per = c.sz.best_per;
    const int d = c.d, k = c.k, nm = c.nm, lam_ps = c.sz.lam_ps;
    for (size_t p = 0; p < N && r_from_ideal; ++p)
        for (int l = 0; l < k; ++l) S[p].r[l] = S[p].hfx[l] - S[p].ideal[l];
    std::vector<size_t> act;
    for (size_t p = 0; p < N; ++p) {
        PsStart &s = S[p];
        s.info.tau = 0.0;
        s.xt = s.hxn;
        bool critical = false;
        for (int l = 0; l < k; ++l) {
            critical = critical || !(s.r[l] > 0.0);
            c.hr[p * k + l] = s.r[l];
        }
        if (critical)
            s.info.status = MRBF_PS_CRITICAL;  // any(r .<= 0): omega = 0, the point itself (descent.jl:546-549)
        else
            act.push_back(p);
    }
    if (!act.empty()) {
        MRBF_HIP(ctx, hipMemcpyAsync(c.base + c.oR, c.hr.data(), c.hr.size() * sizeof(double), hipMemcpyHostToDevice, st));
        for (size_t i = 0; i < act.size(); ++i) {
            const size_t p = act[i];
            ps::Args &a = S[p].a;
            double *pp = ps_runs_at(c, p);
            a.nruns = 1;
            ps_make_run(a.runs[0], 1, 0, lam_ps, d + 1, 0, c.max_ps - c.res_ps, pp, c.base + c.oBest + p * best_per, c.stat + 4 * i);
        }
        if (!c.single) {  // the sweep of the starts that take part, every member where the plan of all starts has it
            std::vector<size_t> which;
            for (size_t p : act)
                for (int j = 0; j < nm; ++j) which.push_back(p * nm + j);
            c.ev_ps = c.ev_ps_all.select(ctx, which);
        }
        MRBF_TRY(ps_generations(c, act, &c.ev_ps, SITE_PS, opts->t0, (c.max_ps - c.res_ps + lam_ps - 1) / lam_ps + 1));
        MRBF_HIP(ctx, hipMemcpyAsync(c.hbest.data(), c.base + c.oBest, c.hbest.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        MRBF_HIP(ctx, hipMemcpyAsync(c.hs.data(), c.stat, (size_t)4 * act.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        MRBF_HIP(ctx, hipStreamSynchronize(st));
        std::vector<DescentGroup> gs;
        std::vector<size_t> gp;
        const bool own = opts->max_polish_evals > 0;
        for (size_t i = 0; i < act.size(); ++i) {
            PsStart &s = S[act[i]];
            const double *best = &c.hbest[act[i] * best_per];
            const int *h = &c.hs[4 * i];
            s.info.evals_ps = h[0];
            s.info.generations += h[2];
            const double bf = best[d + 1], bphi = best[d + 2];
            if (!(bphi == 0.0) || !std::isfinite(bf)) {
                s.info.status = MRBF_PS_FAILURE;  // descent.jl:571-572
                continue;
            }
            s.info.tau = bf;
            s.info.status = MRBF_PS_OK;
            for (int t = 0; t < d; ++t) s.xt[t] = best[1 + t];
            // the polish the configuration asks for (its own budget, descent.jl:423-429); without one, the part of the global budget
            // that was kept back or left over
            const int pbudget = own ? opts->max_polish_evals : c.max_ps - h[0];
            if (pbudget < 13) continue;
            DescentGroup G;
            G.P = &s.P;
            G.ds.push_back(descent_of_ps(&s.P, &s.hlb, &s.hub, s.info.tau, s.xt, s.mx, s.r, pbudget, c.xtol));
            gs.push_back(std::move(G));
            gp.push_back(act[i]);
        }
        MRBF_TRY(ps_descend_groups(ctx, gs));
        for (size_t g = 0; g < gs.size(); ++g) {
            PsStart &s = S[gp[g]];
            const Descent &D = gs[g].ds[0];
            s.info.tau = D.val;
            s.xt = D.x;
            if (own)
                s.info.evals_polish = D.evals;
            else
                s.info.evals_ps += D.evals;
        }
    }
    // mx_trial = m(x_trial)
    std::vector<EvalReq> reqs;
    for (size_t p = 0; p < N; ++p)
        if (S[p].info.status == MRBF_PS_OK) reqs.push_back(EvalReq{&S[p].P, S[p].xt.data(), 1, &c.allF[p], nullptr});
    MRBF_TRY(ps_eval_points_many(ctx, reqs));
    for (size_t p = 0; p < N; ++p)
        if (S[p].info.status == MRBF_PS_OK)
            for (int l = 0; l < k; ++l) S[p].mx[l] = S[p].P.objective(c.allF[p], l);
    return MRBF_OK;
}

// Closing: the call's elapsed device time
static int ps_close(PsCall &c, float *ms_out) {
    mrbf_ctx *ctx = c.ctx;
    MRBF_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MRBF_HIP(ctx, hipEventElapsedTime(ms_out, ctx->ev[0], ctx->ev[1]));
    return MRBF_OK;
}

// ---- the entry points' scaffold.  What differs between them -- return codes, the front of the messages, which phases run -- is a
// small table per entry; each entry keeps its own NULL checks and reads its own layout.
struct PsEntry {
    const char *box_prefix;  // in front of the inverted-box message ("" or the call's name and ": ")
    bool box_names_start;    // that message names the start
    int rc_box;              // and the code it comes with
    bool with_ps;            // the PS phase runs (false: the ideal-point calls)
};
// the inputs of N starts as host copies (the pointers may be host or device memory), the box checked
struct PsInputs {
    std::vector<double> x, lb, ub, fx, r;  // N x d (x, lb, ub), N x k (fx, r: empty where not given)
    ps::LinRows lin;
};
static int ps_read_inputs(mrbf_ctx *ctx, const PsEntry &E, size_t SN, int d, int k, const mrbf_ps_problem *shape, const double *x_n,
                          const double *lb_eff, const double *ub_eff, const double *fx_n, const double *r_or_null, PsInputs &in) {
    MRBF_TRY(fetch_host(ctx, x_n, SN * d, in.x));
    MRBF_TRY(fetch_host(ctx, lb_eff, SN * d, in.lb));
    MRBF_TRY(fetch_host(ctx, ub_eff, SN * d, in.ub));
    if (fx_n) MRBF_TRY(fetch_host(ctx, fx_n, SN * k, in.fx));
    if (r_or_null) MRBF_TRY(fetch_host(ctx, r_or_null, SN * k, in.r));
    for (size_t t = 0; t < SN * d; ++t)
        if (!(in.lb[t] <= in.ub[t])) {
            const int j = (int)(t % d);
            if (E.box_names_start) return fail(ctx, E.rc_box, "%sstart %lld: lb_eff[%d] > ub_eff[%d]", E.box_prefix, (long long)(t / d), j, j);
            return fail(ctx, E.rc_box, "%slb_eff[%d] > ub_eff[%d]", E.box_prefix, j, j);
        }
    MRBF_TRY(fetch_host(ctx, shape->A_eq, (size_t)shape->n_lin_eq * d, in.lin.A_eq));
    MRBF_TRY(fetch_host(ctx, shape->b_eq, (size_t)shape->n_lin_eq, in.lin.b_eq));
    MRBF_TRY(fetch_host(ctx, shape->A_ineq, (size_t)shape->n_lin_ineq * d, in.lin.A_ineq));
    MRBF_TRY(fetch_host(ctx, shape->b_ineq, (size_t)shape->n_lin_ineq, in.lin.b_ineq));
    return MRBF_OK;
}

// The chunk loop: a batch whose state exceeds 2 GiB is processed in chunks of starts (MRBF_PS_CHUNK_KB: another limit, so that a test
// can split a small batch).  Per chunk the starts' records are filled from the inputs, the phases run, and `gather` takes what start p
// (its index in the whole call) came out with.  A given direction (in.r) means no ideal phase.
typedef void (*PsGather)(void *out, size_t p, const PsStart &s);
static int ps_run_chunks(mrbf_ctx *ctx, const PsEntry &E, size_t SN, const descent::Layout &lay, const mrbf_ps_problem *shape,
                         const mrbf_model *const *models, const PsInputs &in, const mrbf_ps_options *opts, const uint64_t *seeds_or_null,
                         PsGather gather, void *out, float *ms_sum) {
    const int d = lay.d, k = shape->n_objectives, nm = shape->n_models;
    const bool with_ideal = in.r.empty();
    int nftot = 0;
    for (int j = 0; j < nm; ++j) nftot += lay.k[j];
    size_t per_start = 0;
    for (size_t p = 0; p < SN; ++p)
        per_start = std::max(per_start, ps_start_doubles(ctx, models + p * nm, nm, d, k, nftot, with_ideal, E.with_ps) * sizeof(double));
    const size_t limit = mrbf_env("MRBF_PS_CHUNK_KB") ? (size_t)std::max(1, atoi(mrbf_env("MRBF_PS_CHUNK_KB"))) << 10 : (size_t)2 << 30;
    const size_t chunk = std::max<size_t>(1, limit / per_start);
    *ms_sum = 0.f;
    for (size_t p0 = 0; p0 < SN; p0 += chunk) {
        const size_t n = std::min(chunk, SN - p0);
        std::vector<PsStart> S(n);
        for (size_t i = 0; i < n; ++i) {
            const size_t p = p0 + i;
            PsStart &s = S[i];
            ps_problem_fill(s.P, lay, shape, models + p * nm);
            s.P.lin = &in.lin;
            s.hlb.assign(in.lb.begin() + p * d, in.lb.begin() + (p + 1) * d);
            s.hub.assign(in.ub.begin() + p * d, in.ub.begin() + (p + 1) * d);
            s.hxn.assign(in.x.begin() + p * d, in.x.begin() + (p + 1) * d);
            if (!in.fx.empty()) s.hfx.assign(in.fx.begin() + p * k, in.fx.begin() + (p + 1) * k);
            s.r.assign(k, 0.0);
            if (!in.r.empty()) s.r.assign(in.r.begin() + p * k, in.r.begin() + (p + 1) * k);
            s.seed = seeds_or_null ? seeds_or_null[p] : opts->seed;
        }
        PsCall c;
        float ms = 0.f;
        MRBF_TRY(ps_open(c, ctx, S, opts, with_ideal, E.with_ps));
        if (with_ideal) MRBF_TRY(ps_ideal_phase(c));
        if (E.with_ps) MRBF_TRY(ps_step_phase(c, with_ideal));
        MRBF_TRY(ps_close(c, &ms));
        *ms_sum += ms;
        for (size_t i = 0; i < n; ++i) gather(out, p0 + i, S[i]);
    }
    return MRBF_OK;
}

// what the step calls gather: the records where the caller wants them (the single call: a record of its own -- nothing reaches the
// caller before the step has succeeded), the arrays in host blocks that are put at the end
struct PsStepOut {
    int d, k;
    mrbf_ps_info *infos;
    std::vector<double> x, mx, r;
};
static void ps_gather_step(void *out, size_t p, const PsStart &s) {
    PsStepOut &o = *static_cast<PsStepOut *>(out);
    o.infos[p] = s.info;
    std::copy(s.xt.begin(), s.xt.end(), o.x.begin() + p * o.d);
    std::copy(s.mx.begin(), s.mx.end(), o.mx.begin() + p * o.k);
    std::copy(s.r.begin(), s.r.end(), o.r.begin() + p * o.k);
}
static int ps_put_step(mrbf_ctx *ctx, const PsStepOut &o, size_t SN, double *x_trial, double *mx_trial, double *r_out) {
    MRBF_TRY(output_put(ctx, x_trial, o.x.data(), SN * o.d));
    MRBF_TRY(output_put(ctx, mx_trial, o.mx.data(), SN * o.k));
    if (r_out) MRBF_TRY(output_put(ctx, r_out, o.r.data(), SN * o.k));
    return MRBF_OK;
}

}  // namespace mrbf

using namespace mrbf;

extern "C" int32_t mrbf_ps_step_problem(mrbf_ctx *ctx, const mrbf_ps_problem *prob, const double *x_n, const double *lb_eff, const double *ub_eff,
                                        const double *fx_n, const double *r_or_null, const mrbf_ps_options *opts, double *x_trial,
                                        double *mx_trial, double *r_out, mrbf_ps_info *info) {
    if (!ctx) return -1;
    if (!prob) return fail(ctx, -2, "problem is NULL");
    if (!x_n) return fail(ctx, -3, "x_n is NULL");
    if (!lb_eff) return fail(ctx, -4, "lb_eff is NULL");
    if (!ub_eff) return fail(ctx, -5, "ub_eff is NULL");
    if (!r_or_null && !fx_n) return fail(ctx, -6, "fx_n is NULL but no direction was given");
    if (!opts) return fail(ctx, -8, "opts is NULL");
    if (opts->t0 < -1.0 || opts->t0 > 0.0) return fail(ctx, -8, "opts.t0 must lie in [-1, 0]");
    if (!x_trial) return fail(ctx, -9, "x_trial is NULL");
    if (!mx_trial) return fail(ctx, -10, "mx_trial is NULL");
    if (!info) return fail(ctx, -12, "info is NULL");
    (void)hipSetDevice(ctx->device);
    using namespace ps;
    std::memset(info, 0, sizeof(*info));
    // ---- the function table
    if (prob->n_models < 1 || prob->n_models > MAXMODELS || !prob->models || !prob->roles)
        return fail(ctx, -2, "mrbf_ps_step: 1..%d grouped models with a roles table are required", MAXMODELS);
    if (prob->n_objectives < 1 || prob->n_objectives > MAXOBJ) return fail(ctx, -2, "mrbf_ps_step: %d objectives (device path: 1..%d)", prob->n_objectives, MAXOBJ);
    std::vector<descent::SlotShape> slots;
    descent::Layout lay;
    if (descent::Defect D = descent::read(descent_shape(prob, prob->models, 1, slots), {true, descent::Centres::UNCHECKED}, lay))
        return fail(ctx, -2, "mrbf_ps_step: %s", D.msg.c_str());
    if (lay.n_nl > MAXCON) return fail(ctx, -2, "mrbf_ps_step: more than %d modelled constraints", MAXCON);
    const int d = lay.d, k = prob->n_objectives;
    if (mrbf_dispatch_ps(d, k, prob->n_models, (int)lay.rows.size(), prob->n_lin_eq + prob->n_lin_ineq, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_ps_step: d = %d / k = %d / %d constraints outside the device path (ask mrbf_dispatch_ps first)", d, k, (int)lay.rows.size());
    const PsEntry E{"", false, -4, true};
    PsInputs in;
    MRBF_TRY(ps_read_inputs(ctx, E, 1, d, k, prob, x_n, lb_eff, ub_eff, fx_n, r_or_null, in));
    mrbf_ps_info rec{};
    PsStepOut o{d, k, &rec, std::vector<double>(d), std::vector<double>(k), std::vector<double>(k)};
    float ms = 0.f;
    MRBF_TRY(ps_run_chunks(ctx, E, 1, lay, prob, prob->models, in, opts, nullptr, ps_gather_step, &o, &ms));
    *info = rec;
    info->ms_total = ms;
    return ps_put_step(ctx, o, 1, x_trial, mx_trial, r_out);
}

// ---- many-start Pascoletti-Serafini step: get_criticality(::PascolettiSerafiniConfig, ...) (Morbit.jl src/descent.jl:512-581) for
// n_starts independent starts of one problem in one call -- the reference's Threads.@threads loop over starts
// (examples/large_scale_benchmarks.jl:102-109) with descent_method = :ps.  For start p the outputs are, bit for bit, those of
// mrbf_ps_step_problem on start p's container: the step above is that call's own, with the start on a grid dimension.
extern "C" int32_t mrbf_ps_step_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                                      const double *x_n, const double *lb_eff, const double *ub_eff, const double *fx_n, const double *r_or_null,
                                      const mrbf_ps_options *opts, const uint64_t *seeds_or_null, double *x_trial, double *mx_trial, double *r_out,
                                      mrbf_ps_info *infos, float *ms_total) {
    if (!ctx) return -1;
    if (ms_total) *ms_total = 0.f;
    if (!shape) return fail(ctx, -3, "shape is NULL");
    if (!models) return fail(ctx, -4, "models is NULL");
    if (!x_n) return fail(ctx, -5, "x_n is NULL");
    if (!lb_eff) return fail(ctx, -6, "lb_eff is NULL");
    if (!ub_eff) return fail(ctx, -7, "ub_eff is NULL");
    if (!r_or_null && !fx_n) return fail(ctx, -8, "fx_n is NULL but no direction was given");
    if (!opts) return fail(ctx, -10, "opts is NULL");
    if (opts->t0 < -1.0 || opts->t0 > 0.0) return fail(ctx, -10, "opts.t0 must lie in [-1, 0]");
    if (!x_trial) return fail(ctx, -12, "x_trial is NULL");
    if (!mx_trial) return fail(ctx, -13, "mx_trial is NULL");
    if (!infos) return fail(ctx, -15, "infos is NULL");
    if (shape->n_models < 1 || !shape->roles) return fail(ctx, -3, "mrbf_ps_step_batch: grouped models with a roles table are required");
    if (n_starts < 1) return fail(ctx, -2, "mrbf_ps_step_batch: %lld starts (ask mrbf_dispatch_ps_batch first)", (long long)n_starts);
    const int64_t N = n_starts;
    const int k = shape->n_objectives, nm = shape->n_models;
    std::vector<descent::SlotShape> slots;
    descent::Shape sh = descent_shape(shape, models, N, slots);
    sh.batch = true;
    descent::Layout lay;
    if (descent::Defect D = descent::read(sh, {true, descent::Centres::EVERY_SLOT}, lay))
        return fail(ctx, D.cls == descent::Defect::MODELS ? -4 : -3, "mrbf_ps_step_batch: %s", D.msg.c_str());
    const int d = lay.d, n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if (mrbf_dispatch_ps_batch(N, d, k, nm, lay.n_nl, n_lin, 0) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "mrbf_ps_step_batch: %lld starts / d = %d / k = %d / %d constraints outside the device path (ask mrbf_dispatch_ps_batch first)",
                    (long long)N, d, k, lay.n_nl + n_lin);
    (void)hipSetDevice(ctx->device);
    const size_t SN = (size_t)N;
    std::memset(infos, 0, SN * sizeof(*infos));
    const PsEntry E{"", true, -6, true};
    PsInputs in;
    MRBF_TRY(ps_read_inputs(ctx, E, SN, d, k, shape, x_n, lb_eff, ub_eff, fx_n, r_or_null, in));
    PsStepOut o{d, k, infos, std::vector<double>(SN * d), std::vector<double>(SN * k), std::vector<double>(SN * k)};
    float ms_sum = 0.f;
    MRBF_TRY(ps_run_chunks(ctx, E, SN, lay, shape, models, in, opts, seeds_or_null, ps_gather_step, &o, &ms_sum));
    for (size_t p = 0; p < SN; ++p) infos[p].ms_total = ms_sum;
    if (ms_total) *ms_total = ms_sum;
    return ps_put_step(ctx, o, SN, x_trial, mx_trial, r_out);
}

// ---- local ideal points: compute_local_ideal_point (Morbit.jl src/descent.jl:404-412, k runs of _min_component :369-387) as calls of
// their own -- the step's opening without room for the PS run, its ideal phase and its closing.  The validation, the block the
// outputs are gathered in and the records' packing are ideal_host.hpp's; nothing reaches the caller before the call has succeeded.
struct IdealOut {
    int k;
    ideal::Layout L;
    std::vector<double> out;
    std::vector<mrbf_ideal_info> info;
};
static void ideal_gather(void *out, size_t p, const PsStart &s) {
    IdealOut &o = *static_cast<IdealOut *>(out);
    ideal::pack(o.info[p], o.k, s.info.evals_ideal, s.info.generations, s.found.data(), s.refined.data());
    std::copy(s.ideal.begin(), s.ideal.end(), o.out.begin() + o.L.ideal_at(p, 0));
    std::copy(s.mx.begin(), s.mx.end(), o.out.begin() + o.L.mx_at(p, 0));
    std::copy(s.x_ideal.begin(), s.x_ideal.end(), o.out.begin() + o.L.x_ideal_at(p, 0));
}
static_assert(ideal::MAX_OBJECTIVES == ps::MAXOBJ, "a bit per objective in mrbf_ideal_info::found / refined");
static int32_t ideal_points(mrbf_ctx *ctx, bool batch, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                            const double *x_n, const double *lb_eff, const double *ub_eff, const mrbf_ps_options *opts,
                            const uint64_t *seeds_or_null, double *ideal_out, double *x_ideal_out, double *mx_out, mrbf_ideal_info *infos,
                            float *ms_total) {
    const char *name = batch ? "mrbf_ideal_point_batch" : "mrbf_ideal_point_problem";
    ideal::Call c;
    c.has_ctx = ctx != nullptr, c.batch = batch, c.n_starts = n_starts;
    c.problem = shape != nullptr, c.models = models != nullptr, c.x_n = x_n != nullptr, c.lb = lb_eff != nullptr, c.ub = ub_eff != nullptr;
    c.opts = opts != nullptr, c.ideal_out = ideal_out != nullptr, c.info = infos != nullptr;
    if (shape) c.n_models = shape->n_models, c.roles = shape->roles != nullptr;
    if (const int rc = ideal::validate(c)) {
        if (rc == -1) return -1;
        return fail(ctx, rc, rc == -2 ? "%s: %lld starts (ask mrbf_dispatch_ideal_batch first)" : "%s: an argument is NULL, or the problem has no models or no roles table",
                    name, (long long)n_starts);
    }
    const int64_t N = n_starts;
    const int k = shape->n_objectives, nm = shape->n_models;
    std::vector<descent::SlotShape> slots;
    descent::Shape sh = descent_shape(shape, models, N, slots);
    sh.batch = batch;
    descent::Layout lay;
    if (descent::Defect D = descent::read(sh, {true, batch ? descent::Centres::EVERY_SLOT : descent::Centres::UNCHECKED}, lay))
        return fail(ctx, D.cls == descent::Defect::MODELS ? -4 : -3, "%s: %s", name, D.msg.c_str());
    const int d = lay.d, n_lin = shape->n_lin_eq + shape->n_lin_ineq;
    if ((batch ? mrbf_dispatch_ideal_batch(N, d, k, nm, lay.n_nl, n_lin, 0) : mrbf_dispatch_ideal(d, k, nm, lay.n_nl, n_lin, 0)) != MRBF_DISPATCH_DEVICE)
        return fail(ctx, -2, "%s: %lld starts / d = %d / k = %d / %d constraints outside the device path (ask %s first)", name, (long long)N, d, k,
                    lay.n_nl + n_lin, batch ? "mrbf_dispatch_ideal_batch" : "mrbf_dispatch_ideal");
    (void)hipSetDevice(ctx->device);
    const size_t SN = (size_t)N;
    const std::string prefix = std::string(name) + ": ";
    const PsEntry E{prefix.c_str(), true, -6, false};
    PsInputs in;
    MRBF_TRY(ps_read_inputs(ctx, E, SN, d, k, shape, x_n, lb_eff, ub_eff, nullptr, nullptr, in));
    IdealOut o{k, ideal::layout(N, d, k), {}, std::vector<mrbf_ideal_info>(SN)};
    o.out.resize(o.L.total);
    float ms_sum = 0.f;
    MRBF_TRY(ps_run_chunks(ctx, E, SN, lay, shape, models, in, opts, seeds_or_null, ideal_gather, &o, &ms_sum));
    for (size_t p = 0; p < SN; ++p) o.info[p].ms_total = ms_sum;
    MRBF_TRY(output_put(ctx, ideal_out, o.out.data() + o.L.ideal, SN * k));
    if (mx_out) MRBF_TRY(output_put(ctx, mx_out, o.out.data() + o.L.mx, SN * k));
    if (x_ideal_out) MRBF_TRY(output_put(ctx, x_ideal_out, o.out.data() + o.L.x_ideal, SN * k * d));
    std::copy(o.info.begin(), o.info.end(), infos);
    if (ms_total) *ms_total = ms_sum;
    return MRBF_OK;
}

extern "C" int32_t mrbf_ideal_point_problem(mrbf_ctx *ctx, const mrbf_ps_problem *problem, const double *x_n, const double *lb_eff,
                                            const double *ub_eff, const mrbf_ps_options *opts, double *ideal_out, double *x_ideal_out,
                                            double *mx_out, mrbf_ideal_info *info) {
    return ideal_points(ctx, false, 1, problem, problem ? problem->models : nullptr, x_n, lb_eff, ub_eff, opts, nullptr, ideal_out, x_ideal_out,
                        mx_out, info, nullptr);
}

// For start p every output (ms_total aside) is, bit for bit, that of mrbf_ideal_point_problem on start p's container with seeds[p]: the
// phase is that call's own with the start on a grid dimension, as in mrbf_ps_step_batch.
extern "C" int32_t mrbf_ideal_point_batch(mrbf_ctx *ctx, int64_t n_starts, const mrbf_ps_problem *shape, const mrbf_model *const *models,
                                          const double *x_n, const double *lb_eff, const double *ub_eff, const mrbf_ps_options *opts,
                                          const uint64_t *seeds_or_null, double *ideal_out, double *x_ideal_out, double *mx_out,
                                          mrbf_ideal_info *infos, float *ms_total) {
    return ideal_points(ctx, true, n_starts, shape, models, x_n, lb_eff, ub_eff, opts, seeds_or_null, ideal_out, x_ideal_out, mx_out, infos,
                        ms_total);
}

// one grouped model whose outputs are the objectives in order, no constraints: the common case (and the round-2 entry point)
extern "C" int32_t mrbf_ps_step(mrbf_ctx *ctx, const mrbf_model *model, const double *x_n, const double *lb_eff, const double *ub_eff,
                                const double *fx_n, const double *r_or_null, const mrbf_ps_options *opts, double *x_trial, double *mx_trial,
                                double *r_out, mrbf_ps_info *info) {
    if (!ctx) return -1;
    if (!model) return fail(ctx, -2, "model is NULL");
    if (model->k > ps::MAXOBJ) return fail(ctx, -2, "mrbf_ps_step: k = %d objectives (device path: <= %d)", model->k, ps::MAXOBJ);
    int32_t roles[ps::MAXOBJ];
    for (int l = 0; l < model->k; ++l) roles[l] = l;
    const mrbf_model *models[1] = {model};
    mrbf_ps_problem prob;
    std::memset(&prob, 0, sizeof(prob));
    prob.n_models = 1;
    prob.n_objectives = model->k;
    prob.models = models;
    prob.roles = roles;
    prob.eq_tol = -1.0;
    return mrbf_ps_step_problem(ctx, &prob, x_n, lb_eff, ub_eff, fx_n, r_or_null, opts, x_trial, mx_trial, r_out, info);
}

// Test hook: ONE ranking of a given generation (objective values f, violations phi; inf = outside the budget) by the kernels of the
// step above, launched as the step launches them -- impl 0: ps_rank_kernel alone (one workgroup); 1: hand-over to ps_rank_wave_kernel
// (one wave per 64 individuals) and the finishing launch; 2: the same with the kernel giving up at once (what a counter time-out
// leaves behind); 3 - 5, 9: see include/mrbf.h.  order_out[lam] = the individuals in rank order.  Lets the tests put crafted
// populations (nearly ranked, a few infeasible individuals: the no-swap exit is taken early) through both kernels and compare the
// orders entry by entry.
extern "C" int32_t mrbf_debug_ps_rank(mrbf_ctx *ctx, int32_t lam, const double *f, const double *phi, uint64_t seed, int32_t gen,
                                      int32_t impl, int32_t *order_out, int32_t *gave_up) {
    if (!ctx) return -1;
    using namespace ps;
    if (lam < 2 || lam > MAXLAM) return fail(ctx, -2, "mrbf_debug_ps_rank: lam = %d outside 2..%d", lam, MAXLAM);
    if (!f || !phi) return fail(ctx, -3, "f / phi is NULL");
    if (gen < 0) return fail(ctx, -6, "gen < 0");
    if (impl < 0 || impl > 9 || (impl >= 6 && impl <= 8)) return fail(ctx, -7, "impl must be 0 .. 5 or 9");
    const bool several = impl == 1 || impl == 2;
    if (several && lam < RS_MINLAM) return fail(ctx, -7, "mrbf_debug_ps_rank: the several-workgroup ranking takes populations >= %d", RS_MINLAM);
    if (!order_out) return fail(ctx, -8, "order_out is NULL");
    (void)hipSetDevice(ctx->device);
    double *base;
    int *stat;
    const size_t args_at = ((size_t)4 * lam + 16 + 15) & ~(size_t)15;  // the one start's block behind the generation
    MRBF_TRY(get_buf(ctx, S_PS_STATE, args_at + (sizeof(Args) + sizeof(double) - 1) / sizeof(double), &base));
    MRBF_TRY(get_buf(ctx, S_PS_STAT, (size_t)4 * MAXRUNS, &stat));
    Args a{};
    Run &R = a.runs[0];
    a.nruns = 1;
    a.seed = seed;
    a.xtol_rel = 1e-3;
    a.dbg = impl == 2 ? DBG_GIVE_UP : (impl == 3 ? DBG_SORT_PAIRS : (impl == 5 ? DBG_NO_SELECT : (impl == 4 ? DBG_SELECT : (impl == 9 ? DBG_PHASE_PAIRS : 0))));
    R.nvar = 1;
    R.lam = lam;
    R.mu = (impl == 4 || impl == 5) ? (lam + 6) / 7 : lam;  // mu = lam: the whole order comes out; 4 / 5: the step's own mu (order_out beyond it: -1)
    R.max_evals = 1 << 30;
    R.X[0] = R.X[1] = base;      // one dummy variable per individual
    R.best = base + lam;         // [x, f, phi]
    R.f = base + lam + 4;
    R.phi = R.f + lam;
    R.order = reinterpret_cast<int *>(R.phi + lam);
    R.stat = stat;
    std::vector<double> h((size_t)lam + 4, 0.0);
    h[lam + 1] = h[lam + 2] = INFINITY;
    MRBF_HIP(ctx, hipMemcpyAsync(base, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MRBF_HIP(ctx, hipMemcpyAsync(R.f, f, (size_t)lam * sizeof(double), hipMemcpyDefault, ctx->stream));
    MRBF_HIP(ctx, hipMemcpyAsync(R.phi, phi, (size_t)lam * sizeof(double), hipMemcpyDefault, ctx->stream));
    MRBF_HIP(ctx, hipMemsetAsync(stat, 0, (size_t)4 * MAXRUNS * sizeof(int), ctx->stream));
    const Args *dA = reinterpret_cast<const Args *>(base + args_at);
    MRBF_HIP(ctx, hipMemcpyAsync(base + args_at, &a, sizeof(Args), hipMemcpyHostToDevice, ctx->stream));
    RankLaunch L;
    MRBF_TRY(rank_launch_setup(ctx, a, 1, several, L));
    rank_launch(ctx, dA, 1, 1, gen, L, true);
    MRBF_HIP(ctx, hipGetLastError());
    int hsync[2] = {0, 0};
    if (L.several) MRBF_HIP(ctx, hipMemcpyAsync(hsync, L.ws.sync, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipMemsetAsync(R.order + R.mu, 0xff, (size_t)(lam - R.mu) * sizeof(int), ctx->stream));
    MRBF_HIP(ctx, hipMemcpyAsync(order_out, R.order, (size_t)lam * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MRBF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (gave_up) *gave_up = hsync[1];
    return MRBF_OK;
}
