// Gaussian mixtures with full (cov_type 2) or tied (cov_type 3) covariances by EM, all arithmetic in f64, the products on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64); gmm_full.py and the p2 / p4 `--gmm_covariance_type full | tied` branches.  The definition stands in include/dic_hip.h.
//
// AN EM ITERATION is five launches per call, every restart a grid row / plane of its own:
//   gf_pass_kernel    E-step.  At most 256 workgroups per restart, each takes its rows 64 at a time (4 waves x 16 rows).  A wave keeps x' of its 16 rows in
//                     registers (lane (r, g) holds the columns 16 ib + 4 g .. + 3 of row r: the contraction index of an MFMA is (g, ks) <-> column 4 g + ks,
//                     so one float4 load serves 4 MFMAs).  Per component: diff = x' - mu'_k once, then P_k comes through LDS in column panels of 16 columns
//                     (rows 0 .. 16 (jb + 1) - 1: only block rows <= the block column of the upper-triangular factor), two buffers, the next panel fetched
//                     into registers under the MFMAs of the current one.  The y tile is never stored: its squares are added per lane in panel order, then
//                     over the 16 lanes of a row by an xor tree.  log-sum-exp: one thread per row, k in order.  Then thread d adds r_ik x'_id over the
//                     tile's rows in row order and adds the tile's sum to the workgroup's partial; thread k likewise for sum_i r_ik.
//   gf_scatter_kernel S_k = sum_i r_ik x'_i x'_i^T on and below the block diagonal: A = r x', B = x', 4 points per MFMA.  A wave owns one block row of 16 x 16
//                     output tiles; N is cut into gf_slabs(N, Kc) row slabs (a function of N and the matrix count alone), one partial matrix per slab.
//   gf_params_kernel  n_k, mu'_k, w_k from the workgroup partials in block order; component 0 appends the lower bound and decides whether the restart is done.
//   gf_cov_kernel     the slab matrices in slab order, the covariance formula, and the mirror image: C == C^T bit for bit.
//   gf_factor_kernel  one workgroup per (restart, matrix): thread i owns row i of L.  Column panels of 16: the panel's 16 rows of L (as columns of U = L^T, kept
//                     in the workspace) come through LDS, every thread subtracts L_it L_jt for t ascending, then the 16 columns are finished one after the
//                     other.  The inverse is solved by columns of P: thread j owns column j and reads only U and its own earlier results.
// No floating-point atomics, no dependence on a neighbouring restart, nothing synchronises the stream.  A done restart is skipped by every kernel: status[6],
// written by the pass alone, says whether the pass ran (the done flag itself is rewritten by gf_params_kernel and gf_factor_kernel).
#include "dic_gmm_common.h"

namespace dic {

typedef double gf_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GF_THREADS = 256;
constexpr int GF_TILE = 64;                       // rows of a tile: 4 waves x 16
constexpr int GF_MAX_BLOCKS = kNumCU;
constexpr int GF_MAX_DIM = 256;
static_assert(GF_MAX_DIM == 4 * kWave, "gmm_check_points admits 4 * kWave columns");
enum { GF_W_LOGR = 0, GF_W_LABELS = 1, GF_W_RESP = 2, GF_W_ONES = 3 };          // where the scatter kernel takes its weights from
enum { GF_C_FULL = 0, GF_C_TSUM = 1, GF_C_TIED = 2 };                           // what the covariance kernel does

__host__ __device__ inline size_t gf_part_words(int K, int D) { return (size_t)K * (1 + (size_t)D) + 1; }          // n_k, sum r x', sum lse
static int gf_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)GF_MAX_BLOCKS, (N + GF_TILE - 1) / GF_TILE)); }
static int gf_slabs(int64_t N, int n_mats) { return (int)max((int64_t)1, min((N + 255) / 256, (int64_t)((128 + n_mats - 1) / n_mats))); }
static int gf_slab_rows(int64_t N, int S) { return (int)(((N + S - 1) / S + 3) / 4 * 4); }

struct GfWs {
    double* logr; double* part; double* nk; double* slab; double* U;
    size_t bytes;
};
static GfWs gf_carve(void* base, int64_t N, int D, int K, int n_runs, int cov_type) {
    const int Kc = cov_type == 2 ? K : 1;
    const size_t mat = (size_t)D * D;
    size_t o = 0;
    auto take = [&](size_t words) { double* p = (double*)((char*)base + o); o += align_up(words * sizeof(double), 256); return p; };
    GfWs w{};
    w.logr = take((size_t)n_runs * N * K);
    w.part = take((size_t)n_runs * gf_blocks(N) * gf_part_words(K, D));
    w.nk = take((size_t)n_runs * K);
    w.slab = take(cov_type == 2 ? (size_t)n_runs * K * gf_slabs(N, K) * mat : (size_t)gf_slabs(N, 1) * mat);
    w.U = take((size_t)n_runs * Kc * mat);
    w.bytes = o;
    return w;
}

struct GfArgs {
    const float* X; long ldx;
    int n, d, d0, k, kc, rpb, em, accum;
    const double* shift;
    const double* w; const double* mu; const double* P; const double* logdet;          // (runs, K), (runs, K, D), (runs, Kc, D, D), (runs, Kc)
    double* status; double* part;
    double* logr;                                                  // (runs, N, K) or NULL
    double* lse; int32_t* labels;                                  // optional
    const int32_t* labels_in; const double* resp_in;               // gf_resp_kernel
};

// The accumulation of a tile: s_r (nt, K) responsibilities and s_lse (nt) in LDS -> the workgroup's partial.  Thread d owns column d.
__device__ __forceinline__ void gf_accumulate(const GfArgs& a, const double* s_r, const double* s_lse, long long t0, int nt, bool first, double* part, double& pn,
                                              double& pl) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, K = a.k, D = a.d;
    if (tid < D) {          // (component by component: the rows are read again per component, which hits, and no accumulator array is kept)
        const double cd = a.shift[tid];
        const float* xc = a.X + (size_t)t0 * a.ldx + tid;
        for (int j = 0; j < K; ++j) {
            double sx = 0.0;
#pragma unroll 8
            for (int i = 0; i < nt; ++i) {
                const double xv = (double)xc[(size_t)i * a.ldx] - cd;
                const double t = s_r[i * K + j] * xv;
                sx = sx + t;
            }
            double* p = part + K + (size_t)j * D + tid;
            *p = first ? sx : *p + sx;
        }
    }
    if (tid < K)
        for (int i = 0; i < nt; ++i) pn += s_r[i * K + tid];
    if (tid == 0)
        for (int i = 0; i < nt; ++i) pl += s_lse[i];
}

// One panel of P_kc (rows 0 .. 16 (jb + 1) - 1 of the columns 16 jb .. 16 jb + 15) into registers: thread (q = tid >> 4, c = tid & 15) takes the rows q + 16 u.
template <int NB>
__device__ __forceinline__ void gf_fetch(double (&stage)[NB], const double* Pk, int D, int jb) {
    const int q = threadIdx.x >> 4, col = 16 * jb + (threadIdx.x & 15);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = q + 16 * u;
        stage[u] = (u <= jb && t < D && col < D) ? Pk[(size_t)t * D + col] : 0.0;
    }
}
// .. and from the registers into LDS, in the order the MFMAs read: row 16 ib + 4 g + ks at ((4 ib + ks) 64 + 16 g + c)
template <int NB>
__device__ __forceinline__ void gf_commit(const double (&stage)[NB], double* buf, int jb) {
    const int q = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int u = 0; u < NB; ++u)
        if (u <= jb) buf[(4 * u + (q & 3)) * 64 + 16 * (q >> 2) + c] = stage[u];
}

template <int NB>
__global__ __launch_bounds__(GF_THREADS) void gf_pass_kernel(GfArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double gf_lds[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int run = blockIdx.y, K = a.k, D = a.d, n = a.n;
    const int nb = (D + 15) >> 4;
    if (a.em) {
        const bool done = a.status[(size_t)run * DIC_GMM_STATUS_WORDS] != 0.0;          // (written by the previous call's kernels, never in this launch)
        if (blockIdx.x == 0 && tid == 0) a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] = done ? 0.0 : 1.0;
        if (done) return;
    }
    double* s_pan = gf_lds;                                   // 2 panels of 16 NB x 16
    double* s_lp = s_pan + 2 * 256 * NB;                      // (64, K): log p, then r
    double* s_lse = s_lp + GF_TILE * K;                       // 64
    double* s_lc = s_lse + GF_TILE;                           // K: log w_k
    double* s_ld = s_lc + K;                                  // K: log_det_k
    const double* mu = a.mu + (size_t)run * K * D;
    const double* P = a.P + (size_t)run * a.kc * D * D;
    if (tid < K) {
        s_lc[tid] = log(a.w[(size_t)run * K + tid]);
        s_ld[tid] = a.logdet[(size_t)run * a.kc + (a.kc == 1 ? 0 : tid)];
    }
    const size_t mat = (size_t)D * D;
    const double d0_log2pi = (double)a.d0 * GMM_LOG_2PI;
    double* part = a.part + ((size_t)run * gridDim.x + blockIdx.x) * gf_part_words(K, D);
    double pn = 0.0, pl = 0.0;
    double stage[NB];

    const long long r0 = (long long)blockIdx.x * a.rpb;
    const long long r1 = min((long long)n, r0 + a.rpb);
    int buf = 0;
    if (r0 < r1) {
        gf_fetch<NB>(stage, P, D, 0);
        gf_commit<NB>(stage, s_pan, 0);
    }
    __syncthreads();
    for (long long t0 = r0; t0 < r1; t0 += GF_TILE) {
        const int nt = (int)min((long long)GF_TILE, r1 - t0);
        const long long row = t0 + min(16 * wv + r, nt - 1);          // (a row past the end repeats the last valid one; its result is dropped)
        float4 xf[NB];          // (f32, as loaded: x' = (double)x - c is redone per component, which costs loads that hit and halves the registers)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
            const int col = 16 * ib + 4 * g;
            xf[ib] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col < D) xf[ib] = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + col);
        }
        for (int k = 0; k < K; ++k) {
            double diff[NB][4];
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                const int col = 16 * ib + 4 * g;
                const float xv[4] = {xf[ib].x, xf[ib].y, xf[ib].z, xf[ib].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    diff[ib][j] = 0.0;
                    if (col < D) {
                        const double xs = (double)xv[j] - a.shift[col + j];
                        diff[ib][j] = xs - mu[(size_t)k * D + col + j];
                    }
                }
                if ((ib & 3) == 3) __builtin_amdgcn_sched_barrier(0);          // (at most 32 of the loads in flight: all 128 at once do not fit the registers)
            }
            double msum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                if (jb < nb) {
                    // the panel after this one: the next column block, the next component, or the first panel again for the next tile
                    int njb = jb + 1, nk = k;
                    if (njb == nb) { njb = 0; nk = k + 1 < K ? k + 1 : 0; }
                    const bool more = jb + 1 < nb || k + 1 < K || t0 + GF_TILE < r1;
                    if (more) gf_fetch<NB>(stage, P + (a.kc == 1 ? 0 : (size_t)nk * mat), D, njb);
                    const double* pan = s_pan + buf * 256 * NB;
                    gf_f64x4 acc = gf_f64x4{0.0, 0.0, 0.0, 0.0};
                    // (the B operands of block row ib + 1 are read under the MFMAs of block row ib; the scheduling barrier keeps the compiler from hoisting
                    // the whole panel's reads, which at 16 block rows would not fit the registers)
                    double bc[4], bn[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) bc[ks] = pan[ks * 64 + lane];
#pragma unroll
                    for (int ib = 0; ib <= jb; ++ib) {
                        if (ib < jb) {
#pragma unroll
                            for (int ks = 0; ks < 4; ++ks) bn[ks] = pan[(4 * (ib + 1) + ks) * 64 + lane];
                        }
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(diff[ib][ks], bc[ks], acc, 0, 0, 0);
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) bc[ks] = bn[ks];
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const double q = acc[reg] * acc[reg];
                        msum[reg] = msum[reg] + q;
                    }
                    if (more) gf_commit<NB>(stage, s_pan + (buf ^ 1) * 256 * NB, njb);
                    __syncthreads();
                    buf ^= 1;
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) msum[reg] += __shfl_xor(msum[reg], o);
                if (r == 0) s_lp[(16 * wv + g + 4 * reg) * K + k] = (s_lc[k] - 0.5 * (d0_log2pi + msum[reg])) + s_ld[k];
            }
        }
        __syncthreads();
        if (tid < nt) {          // log-sum-exp of row tid, k in order
            double* lp = s_lp + tid * K;
            double mx = lp[0];
            int best = 0;
            for (int k = 1; k < K; ++k)
                if (lp[k] > mx) { mx = lp[k]; best = k; }          // the first maximum
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += exp(lp[k] - mx);
            const double lse = mx + log(s);
            const size_t grow = (size_t)(t0 + tid);
            for (int k = 0; k < K; ++k) {
                const double lr = lp[k] - lse;
                if (a.logr) a.logr[((size_t)run * n + grow) * K + k] = lr;
                lp[k] = exp(lr);
            }
            s_lse[tid] = lse;
            if (a.lse) a.lse[grow] = lse;
            if (a.labels) a.labels[grow] = best;
        }
        __syncthreads();
        if (a.accum) gf_accumulate(a, s_lp, s_lse, t0, nt, t0 == r0, part, pn, pl);
        else if (tid == 0)
            for (int i = 0; i < nt; ++i) pl += s_lse[i];
        __syncthreads();          // (the tile is rewritten)
    }
    if (a.accum && r0 >= r1 && tid < D)          // (a workgroup without rows: N just above a multiple of the tile)
        for (int j = 0; j < K; ++j) part[K + (size_t)j * D + tid] = 0.0;
    if (a.accum && tid < K) part[tid] = pn;
    if (tid == 0) part[K + (size_t)K * D] = pl;
}

// The partials of given responsibilities (hard labels or a matrix): the accumulation of the pass without its E-step.
__global__ __launch_bounds__(GF_THREADS) void gf_resp_kernel(GfArgs a) {
    extern __shared__ double gf_lds[];
    const int tid = threadIdx.x, run = blockIdx.y, K = a.k, n = a.n;
    double* s_r = gf_lds;
    double* s_lse = s_r + GF_TILE * K;
    double* part = a.part + ((size_t)run * gridDim.x + blockIdx.x) * gf_part_words(K, a.d);
    double pn = 0.0, pl = 0.0;
    const long long r0 = (long long)blockIdx.x * a.rpb;
    const long long r1 = min((long long)n, r0 + a.rpb);
    if (tid < GF_TILE) s_lse[tid] = 0.0;
    for (long long t0 = r0; t0 < r1; t0 += GF_TILE) {
        const int nt = (int)min((long long)GF_TILE, r1 - t0);
        for (int i = tid; i < nt * K; i += GF_THREADS) {
            const int rr = i / K, k = i - rr * K;
            const size_t row = (size_t)run * n + (size_t)(t0 + rr);
            s_r[i] = a.labels_in ? (a.labels_in[row] == k ? 1.0 : 0.0) : a.resp_in[row * K + k];
        }
        __syncthreads();
        gf_accumulate(a, s_r, s_lse, t0, nt, t0 == r0, part, pn, pl);
        __syncthreads();
    }
    if (r0 >= r1 && tid < a.d)
        for (int j = 0; j < K; ++j) part[K + (size_t)j * a.d + tid] = 0.0;
    if (tid < K) part[tid] = pn;
    if (tid == 0) part[K + (size_t)K * a.d] = 0.0;
}

struct GfScatter {
    const float* X; long ldx;
    int n, d, k, kw, slabs, slab_rows, mode, em;          // k: matrices per restart; kw: row length of the weights (K)
    const double* shift;
    const double* logr; const int32_t* labels; const double* resp;
    const double* status;
    double* slab;                                         // (runs, k, slabs, D, D): only the tiles on and below the block diagonal are written
};

// grid (slabs x row groups, matrices, restarts); wave w of row group q owns the block row q + QG w.
__global__ __launch_bounds__(GF_THREADS) void gf_scatter_kernel(GfScatter a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = a.d, nb = (D + 15) >> 4, QG = (nb + 3) >> 2;
    const int s = blockIdx.x / QG, q = blockIdx.x - s * QG;
    const int kk = blockIdx.y, run = blockIdx.z;
    const int bi = q + QG * ((wv + s) & 3);          // (rotated by the slab: the long block rows of co-resident workgroups land on different SIMDs)
    if (a.em && a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] == 0.0) return;
    if (bi >= nb) return;
    double cc[16];
#pragma unroll
    for (int bj = 0; bj < 16; ++bj) cc[bj] = (bj <= bi && 16 * bj + r < D) ? a.shift[16 * bj + r] : 0.0;
    gf_f64x4 acc[16];
#pragma unroll
    for (int bj = 0; bj < 16; ++bj) acc[bj] = gf_f64x4{0.0, 0.0, 0.0, 0.0};
    const bool arow = 16 * bi + r < D;
    const double ca = arow ? a.shift[16 * bi + r] : 0.0;
    const long long i0 = (long long)s * a.slab_rows, i1 = min((long long)a.n, i0 + a.slab_rows);
    for (long long c0 = i0; c0 < i1; c0 += 64) {
        // the weights of the chunk's 64 points: lane L holds point c0 + L
        const long long pi = c0 + lane;
        double wl = 0.0;
        if (pi < i1) {
            const size_t row = (size_t)run * a.n + (size_t)pi;
            if (a.mode == GF_W_LOGR) wl = exp(a.logr[row * a.kw + kk]);
            else if (a.mode == GF_W_LABELS) wl = a.labels[row] == kk ? 1.0 : 0.0;
            else if (a.mode == GF_W_RESP) wl = a.resp[row * a.kw + kk];
            else wl = 1.0;
        }
        const int steps = (int)min((long long)16, (i1 - c0 + 3) / 4);
        // the values of step st + 1 are loaded under the MFMAs of step st
        float xv[16], xn[16];
        float xa, xan = 0.f;
        {
            // (a point past the slab's end has weight 0: its row only has to be readable)
            const float* xr = a.X + (size_t)min(c0 + g, (long long)a.n - 1) * a.ldx + r;
#pragma unroll
            for (int bj = 0; bj < 16; ++bj) xv[bj] = (bj <= bi && 16 * bj + r < D) ? xr[16 * bj] : 0.f;
            xa = arow ? xr[16 * bi] : 0.f;
        }
        for (int st = 0; st < steps; ++st) {
            const double wt = __shfl(wl, 4 * st + g);
            if (st + 1 < steps) {
                const float* xr = a.X + (size_t)min(c0 + 4 * (st + 1) + g, (long long)a.n - 1) * a.ldx + r;
#pragma unroll
                for (int bj = 0; bj < 16; ++bj) xn[bj] = (bj <= bi && 16 * bj + r < D) ? xr[16 * bj] : 0.f;
                xan = arow ? xr[16 * bi] : 0.f;
            }
            const double av = wt * ((double)xa - ca);
#pragma unroll
            for (int bj = 0; bj < 16; ++bj)
                if (bj <= bi) acc[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, (double)xv[bj] - cc[bj], acc[bj], 0, 0, 0);
#pragma unroll
            for (int bj = 0; bj < 16; ++bj) xv[bj] = xn[bj];
            xa = xan;
        }
    }
    double* out = a.slab + (((size_t)run * a.k + kk) * a.slabs + s) * (size_t)D * D;
#pragma unroll
    for (int bj = 0; bj < 16; ++bj) {
        if (bj <= bi) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int orow = 16 * bi + g + 4 * reg, ocol = 16 * bj + r;
                if (orow < D && ocol < D) out[(size_t)orow * D + ocol] = acc[bj][reg];
            }
        }
    }
}

constexpr int GF_BATCH = 16;          // loads in flight of gmm_sum_blocks

struct GfParams {
    const double* part; int nblk;
    int n, d, k, em, lb_stride;
    double* w; double* mu; double* nk; double* status; double* lower_bounds;
};

// one workgroup per (component, restart): n_k, mu'_k, w_k; component 0 also the lower bound and the stopping decision
__global__ __launch_bounds__(GF_THREADS) void gf_params_kernel(GfParams a) {
#pragma clang fp contract(off)
    __shared__ double s_n[DIC_MAX_CLUSTERS];
    __shared__ double s_lse;
    const int tid = threadIdx.x, k = blockIdx.x, run = blockIdx.y, K = a.k, D = a.d;
    double* st = a.status + (size_t)run * DIC_GMM_STATUS_WORDS;
    if (a.em && st[6] == 0.0) return;
    const size_t P = gf_part_words(K, D);
    const double* part = a.part + (size_t)run * a.nblk * P;
    if (tid < K) s_n[tid] = gmm_sum_blocks<GF_BATCH>(part + tid, P, a.nblk) + GMM_NK_EPS;
    if (a.em && k == 0 && tid == kWave) s_lse = gmm_sum_blocks<GF_BATCH>(part + K + (size_t)K * D, P, a.nblk);
    __syncthreads();
    const double nk = s_n[k];
    if (tid < D) a.mu[((size_t)run * K + k) * D + tid] = gmm_sum_blocks<GF_BATCH>(part + K + (size_t)k * D + tid, P, a.nblk) / nk;
    if (tid == 0) {
        const double fn = (double)a.n;
        double ws = 0.0;
        for (int j = 0; j < K; ++j) ws += s_n[j] / fn;
        a.w[(size_t)run * K + k] = (nk / fn) / ws;
        a.nk[(size_t)run * K + k] = nk;
        if (a.em && k == 0) gmm_end_iteration(st, s_lse, fn, a.lower_bounds, a.lb_stride, run);
    }
}

struct GfCov {
    const double* slab; int slabs;
    int d, d0, k, mode, em;
    double reg;
    const double* mu; const double* nk; const double* status;
    const double* T;           // GF_C_TIED: (D, D)
    double* C;                 // GF_C_FULL: (runs, K, D, D); GF_C_TIED: (runs, 1, D, D); GF_C_TSUM: (D, D)
};

// grid (D rows, matrices, restarts); thread j <= i writes C_ij and C_ji
__global__ __launch_bounds__(GF_THREADS) void gf_cov_kernel(GfCov a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, j = threadIdx.x, kk = blockIdx.y, run = blockIdx.z, D = a.d, K = a.k;
    if (a.em && a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] == 0.0) return;
    if (j > i || j >= D) return;
    const size_t mat = (size_t)D * D, e = (size_t)i * D + j;
    double c;
    if (a.mode == GF_C_TSUM) {
        c = gmm_sum_blocks<GF_BATCH>(a.slab + e, mat, a.slabs);
    } else if (i >= a.d0) {          // the padding: the identity
        c = i == j ? 1.0 : 0.0;
    } else if (a.mode == GF_C_FULL) {
        const double s = gmm_sum_blocks<GF_BATCH>(a.slab + ((size_t)run * K + kk) * a.slabs * mat + e, mat, a.slabs);
        const double* mu = a.mu + ((size_t)run * K + kk) * D;
        const double t = s / a.nk[(size_t)run * K + kk];
        const double m2 = mu[i] * mu[j];
        c = t - m2;
        if (i == j) c = c + a.reg;
    } else {
        double m2 = 0.0, ns = 0.0;
        for (int k = 0; k < K; ++k) {
            const double* mu = a.mu + ((size_t)run * K + k) * D;
            const double nk = a.nk[(size_t)run * K + k];
            const double t = nk * mu[i];
            const double u = t * mu[j];
            m2 = m2 + u;
            ns = ns + nk;
        }
        const double t = a.T[e] - m2;
        c = t / ns;
        if (i == j) c = c + a.reg;
    }
    double* C = a.C + (a.mode == GF_C_TSUM ? 0 : ((size_t)run * (a.mode == GF_C_FULL ? K : 1) + kk) * mat);
    C[e] = c;
    if (i != j) C[(size_t)j * D + i] = c;
}

struct GfFactor {
    const double* C; double* U; double* P; double* logdet; double* status;
    int d, d0, kc, em;
};

// one workgroup per (matrix, restart).  Thread i owns row i of L (stored as column i of U = L^T) and, afterwards, column i of P.
__global__ __launch_bounds__(GF_THREADS) void gf_factor_kernel(GfFactor a) {
#pragma clang fp contract(off)
    __shared__ double s_hist[(GF_MAX_DIM - 16) * 16];
    __shared__ double s_col[16];
    __shared__ double s_piv;
    __shared__ double s_ld[GF_MAX_DIM];
    const int i = threadIdx.x, kk = blockIdx.x, run = blockIdx.y, D = a.d, D0 = a.d0;
    double* st = a.status + (size_t)run * DIC_GMM_STATUS_WORDS;
    if (a.em && st[6] == 0.0) return;
    const size_t mat = (size_t)D * D, m0 = ((size_t)run * a.kc + kk) * mat;
    const double* C = a.C + m0;
    double* U = a.U + m0;
    double* P = a.P + m0;
    const int nb0 = (D0 + 15) >> 4;
    bool ok = true;
    for (int jb = 0; jb < nb0 && ok; ++jb) {
        const int j0 = 16 * jb;
        for (int idx = i; idx < j0 * 16; idx += GF_THREADS) {
            const int t = idx >> 4, c = idx & 15;
            s_hist[idx] = j0 + c < D0 ? U[(size_t)t * D + j0 + c] : 0.0;
        }
        __syncthreads();
        const bool mine = i >= j0 && i < D0;
        double s[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) s[c] = (mine && j0 + c < D0) ? C[(size_t)(j0 + c) * D + i] : 0.0;
        if (mine) {
            for (int t = 0; t < j0; ++t) {
                const double lit = U[(size_t)t * D + i];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const double m = lit * s_hist[t * 16 + c];
                    s[c] = s[c] - m;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int j = j0 + c;
            if (j < D0 && ok) {          // (uniform)
                if (i == j) s_piv = s[c];
                __syncthreads();
                const double piv = s_piv;
                ok = piv > 0.0 && piv < __builtin_inf();          // (false for NaN too)
                double l = 0.0;
                if (ok) {
                    const double dj = sqrt(piv);
                    if (mine && i >= j) {
                        l = i == j ? dj : s[c] / dj;
                        U[(size_t)j * D + i] = l;
                        if (i < j0 + 16) s_col[i - j0] = l;
                    }
                }
                __syncthreads();
                if (ok && mine && i > j) {
#pragma unroll
                    for (int c2 = 0; c2 < 16; ++c2) {
                        if (c2 > c) {
                            const double m = l * s_col[c2];
                            s[c2] = s[c2] - m;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!ok) {          // an ill-defined covariance: the restart is done; P = I keeps every later read finite
        if (i < D)
            for (int c = 0; c < D; ++c) P[(size_t)c * D + i] = c == i ? 1.0 : 0.0;
        if (i == 0) {
            a.logdet[(size_t)run * a.kc + kk] = 0.0;
            st[0] = 1.0;
            st[7] = 1.0;
        }
        return;
    }
    // P = U^-1 by columns: P_cj = -(sum_{t = c + 1 .. j} U_ct P_tj) / U_cc for c = j - 1 .. 0, P_jj = 1 / U_jj
    if (i < D) {
        for (int c = D - 1; c >= D0; --c) P[(size_t)c * D + i] = c == i ? 1.0 : 0.0;
        for (int c = D0 - 1; c >= 0; --c) {
            double v = 0.0;
            if (i < D0 && i >= c) {
                const double ucc = U[(size_t)c * D + c];
                if (i == c) {
                    v = 1.0 / ucc;
                    s_ld[i] = log(v);
                } else {
                    double sum = 0.0;
                    int t = c + 1;
                    for (; t + 3 <= i; t += 4) {          // (4 pairs of loads in flight; the additions in the order of the plain loop)
                        double u[4], p[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { u[q] = U[(size_t)c * D + t + q]; p[q] = P[(size_t)(t + q) * D + i]; }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double m = u[q] * p[q];
                            sum = sum + m;
                        }
                    }
                    for (; t <= i; ++t) {
                        const double m = U[(size_t)c * D + t] * P[(size_t)t * D + i];
                        sum = sum + m;
                    }
                    v = -sum / ucc;
                }
            }
            P[(size_t)c * D + i] = v;
        }
    }
    __syncthreads();
    if (i == 0) {
        double ld = 0.0;
        for (int dd = 0; dd < D0; ++dd) ld += s_ld[dd];
        a.logdet[(size_t)run * a.kc + kk] = ld;
    }
}

__global__ void gf_sum_kernel(const double* part, size_t stride, int nblk, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = gmm_sum_blocks<GF_BATCH>(part, stride, nblk);
}

static int gf_check_points(const char* what, const float* X, long ldx, int64_t N, int D, int D0, int K, int cov_type) {
    const int rc = gmm_check_points(what, X, ldx, N, D, D0, K);
    if (rc == DIC_ERR_INVALID_ARG) return rc;
    DIC_REQUIRE(cov_type == 2 || cov_type == 3, DIC_ERR_INVALID_ARG, "%s: cov_type=%d: 2 (full) or 3 (tied)", what, cov_type);          // (before the unsupported shapes)
    return rc;
}

static size_t gf_pass_lds(int NB, int K) { return ((size_t)2 * 256 * NB + (size_t)GF_TILE * K + GF_TILE + 2 * (size_t)K) * sizeof(double); }

template <int NB>
static int gf_launch_pass_nb(const char* what, const GfArgs& a, int nblk, int n_runs, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        const int most = (int)gf_pass_lds(NB, DIC_MAX_CLUSTERS);
        hipError_t e = hipFuncSetAttribute((const void*)gf_pass_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", what, most, hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(gf_pass_kernel<NB>, dim3((unsigned)nblk, (unsigned)n_runs), dim3(GF_THREADS), gf_pass_lds(NB, a.k), st, a);
    return DIC_OK;
}
static int gf_launch_pass(const char* what, const GfArgs& a, int nblk, int n_runs, hipStream_t st) {
    if (a.d <= 32) return gf_launch_pass_nb<2>(what, a, nblk, n_runs, st);
    if (a.d <= 64) return gf_launch_pass_nb<4>(what, a, nblk, n_runs, st);
    if (a.d <= 128) return gf_launch_pass_nb<8>(what, a, nblk, n_runs, st);
    return gf_launch_pass_nb<16>(what, a, nblk, n_runs, st);
}

static void gf_launch_scatter(const float* X, long ldx, int64_t N, int D, int n_mats, int kw, int n_runs, int mode, int em, const double* shift,
                              const double* logr, const int32_t* labels, const double* resp, const double* status, double* slab, hipStream_t st) {
    GfScatter s{};
    s.X = X; s.ldx = ldx; s.n = (int)N; s.d = D; s.k = n_mats; s.kw = kw; s.slabs = gf_slabs(N, n_mats); s.slab_rows = gf_slab_rows(N, s.slabs);
    s.mode = mode; s.em = em; s.shift = shift; s.logr = logr; s.labels = labels; s.resp = resp; s.status = status; s.slab = slab;
    const int QG = (((D + 15) >> 4) + 3) >> 2;
    hipLaunchKernelGGL(gf_scatter_kernel, dim3((unsigned)(s.slabs * QG), (unsigned)n_mats, (unsigned)n_runs), dim3(GF_THREADS), 0, st, s);
}

// n_k / mu' / w, the covariances and their factors from the partials (and, for full covariances, the slab matrices) in the workspace
static void gf_finish_mstep(const GfWs& w, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg, int em, double* weights, double* means,
                            double* covariances, double* prec_chol, double* log_det, const double* T, double* status, double* lower_bounds, int lb_stride,
                            hipStream_t st) {
    const int Kc = cov_type == 2 ? K : 1;
    GfParams p{};
    p.part = w.part; p.nblk = gf_blocks(N); p.n = (int)N; p.d = D; p.k = K; p.em = em; p.lb_stride = lb_stride;
    p.w = weights; p.mu = means; p.nk = w.nk; p.status = status; p.lower_bounds = lower_bounds;
    hipLaunchKernelGGL(gf_params_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(GF_THREADS), 0, st, p);
    GfCov c{};
    c.slab = w.slab; c.slabs = gf_slabs(N, K); c.d = D; c.d0 = D0; c.k = K; c.mode = cov_type == 2 ? GF_C_FULL : GF_C_TIED; c.em = em; c.reg = reg;
    c.mu = means; c.nk = w.nk; c.status = status; c.T = T; c.C = covariances;
    hipLaunchKernelGGL(gf_cov_kernel, dim3((unsigned)D, (unsigned)Kc, (unsigned)n_runs), dim3(GF_THREADS), 0, st, c);
    GfFactor f{};
    f.C = covariances; f.U = w.U; f.P = prec_chol; f.logdet = log_det; f.status = status; f.d = D; f.d0 = D0; f.kc = Kc; f.em = em;
    hipLaunchKernelGGL(gf_factor_kernel, dim3((unsigned)Kc, (unsigned)n_runs), dim3(GF_THREADS), 0, st, f);
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_gmm_full_workspace(int64_t N, int D, int K, int n_runs, int cov_type) {
    if (N < 2 || N >= (1LL << 30) || D <= 0 || D > GF_MAX_DIM || K < 1 || K > DIC_MAX_CLUSTERS || n_runs < 1 || (cov_type != 2 && cov_type != 3)) return 0;
    return gf_carve(nullptr, N, D, K, n_runs, cov_type).bytes;
}

int dic_gmm_full_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                         double* weights, double* means, double* covariances, double* prec_chol, double* log_det, const double* scatter_total, double* status,
                         double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gf_check_points("gmm_full_em_iter", X, ldx, N, D, D0, K, cov_type);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && covariances && prec_chol && log_det && status && lower_bounds && workspace, DIC_ERR_INVALID_ARG,
                "gmm_full_em_iter: NULL pointer");
    DIC_REQUIRE(cov_type == 2 || scatter_total, DIC_ERR_INVALID_ARG, "gmm_full_em_iter: NULL pointer (tied covariances need the total scatter matrix)");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && lb_stride >= 1 && reg_covar >= 0.0, DIC_ERR_INVALID_ARG, "gmm_full_em_iter: n_runs=%d lb_stride=%d reg_covar=%g",
                n_runs, lb_stride, reg_covar);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_full_em_iter: the workspace must be 16-B aligned");
    const GfWs w = gf_carve(workspace, N, D, K, n_runs, cov_type);
    DIC_REQUIRE(workspace_bytes >= w.bytes, DIC_ERR_WORKSPACE, "gmm_full_em_iter: workspace %zu < %zu", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gf_blocks(N), Kc = cov_type == 2 ? K : 1;
    GfArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.kc = Kc; a.rpb = (int)((N + nblk - 1) / nblk); a.em = 1; a.accum = 1;
    a.shift = shift; a.w = weights; a.mu = means; a.P = prec_chol; a.logdet = log_det; a.status = status; a.part = w.part;
    a.logr = cov_type == 2 ? w.logr : nullptr;
    const int rl = gf_launch_pass("gmm_full_em_iter", a, nblk, n_runs, st);
    if (rl) return rl;
    if (cov_type == 2) gf_launch_scatter(X, ldx, N, D, K, K, n_runs, GF_W_LOGR, 1, shift, w.logr, nullptr, nullptr, status, w.slab, st);
    gf_finish_mstep(w, N, D, D0, K, n_runs, cov_type, reg_covar, 1, weights, means, covariances, prec_chol, log_det, scatter_total, status, lower_bounds,
                    lb_stride, st);
    return check_launch("gmm_full_em_iter");
}

int dic_gmm_full_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, int cov_type, const double* shift, const double* weights, const double* means,
                       const double* prec_chol, const double* log_det, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace,
                       size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gf_check_points("gmm_full_estep", X, ldx, N, D, D0, K, cov_type);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && prec_chol && log_det && workspace, DIC_ERR_INVALID_ARG, "gmm_full_estep: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_full_estep: the workspace must be 16-B aligned");
    const GfWs w = gf_carve(workspace, N, D, K, 1, cov_type);
    DIC_REQUIRE(workspace_bytes >= w.bytes, DIC_ERR_WORKSPACE, "gmm_full_estep: workspace %zu < %zu", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gf_blocks(N);
    GfArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.kc = cov_type == 2 ? K : 1; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.w = weights; a.mu = means; a.P = prec_chol; a.logdet = log_det; a.part = w.part;
    a.logr = log_resp; a.lse = lse; a.labels = labels;
    const int rl = gf_launch_pass("gmm_full_estep", a, nblk, 1, st);
    if (rl) return rl;
    if (sum_lse) {
        const size_t P = gf_part_words(K, D);
        hipLaunchKernelGGL(gf_sum_kernel, dim3(1), dim3(kWave), 0, st, (const double*)w.part + K + (size_t)K * D, P, nblk, sum_lse);
    }
    return check_launch("gmm_full_estep");
}

int dic_gmm_full_mstep(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                       const int32_t* labels, const double* resp, double* scatter_total, int compute_total, double* weights, double* means, double* covariances,
                       double* prec_chol, double* log_det, double* status, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gf_check_points("gmm_full_mstep", X, ldx, N, D, D0, K, cov_type);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && covariances && prec_chol && log_det && status && workspace, DIC_ERR_INVALID_ARG, "gmm_full_mstep: NULL pointer");
    DIC_REQUIRE(cov_type == 2 || scatter_total, DIC_ERR_INVALID_ARG, "gmm_full_mstep: NULL pointer (tied covariances need the total scatter matrix)");
    DIC_REQUIRE((labels != nullptr) != (resp != nullptr), DIC_ERR_INVALID_ARG, "gmm_full_mstep: exactly one of labels and resp");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && reg_covar >= 0.0, DIC_ERR_INVALID_ARG, "gmm_full_mstep: n_runs=%d reg_covar=%g", n_runs, reg_covar);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_full_mstep: the workspace must be 16-B aligned");
    const GfWs w = gf_carve(workspace, N, D, K, n_runs, cov_type);
    DIC_REQUIRE(workspace_bytes >= w.bytes, DIC_ERR_WORKSPACE, "gmm_full_mstep: workspace %zu < %zu", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gf_blocks(N);
    GfArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.kc = cov_type == 2 ? K : 1; a.rpb = (int)((N + nblk - 1) / nblk); a.accum = 1;
    a.shift = shift; a.part = w.part; a.labels_in = labels; a.resp_in = resp;
    hipLaunchKernelGGL(gf_resp_kernel, dim3((unsigned)nblk, (unsigned)n_runs), dim3(GF_THREADS), ((size_t)GF_TILE * K + GF_TILE) * sizeof(double), st, a);
    if (cov_type == 2) {
        gf_launch_scatter(X, ldx, N, D, K, K, n_runs, labels ? GF_W_LABELS : GF_W_RESP, 0, shift, nullptr, labels, resp, status, w.slab, st);
    } else if (compute_total) {          // T = sum_i x'_i x'_i^T: the scatter kernel with every weight 1, once per fit
        gf_launch_scatter(X, ldx, N, D, 1, 1, 1, GF_W_ONES, 0, shift, nullptr, nullptr, nullptr, status, w.slab, st);
        GfCov c{};
        c.slab = w.slab; c.slabs = gf_slabs(N, 1); c.d = D; c.d0 = D0; c.k = 1; c.mode = GF_C_TSUM; c.C = scatter_total;
        hipLaunchKernelGGL(gf_cov_kernel, dim3((unsigned)D, 1, 1), dim3(GF_THREADS), 0, st, c);
    }
    gf_finish_mstep(w, N, D, D0, K, n_runs, cov_type, reg_covar, 0, weights, means, covariances, prec_chol, log_det, scatter_total, status, nullptr, 0, st);
    return check_launch("gmm_full_mstep");
}

int dic_gmm_full_factor(const double* covariances, int n_runs, int n_mats, int D, int D0, double* prec_chol, double* log_det, double* status, void* workspace,
                        size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(covariances && prec_chol && log_det && status && workspace, DIC_ERR_INVALID_ARG, "gmm_full_factor: NULL pointer");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && n_mats >= 1 && D > 0 && D0 >= 1 && D0 <= D, DIC_ERR_INVALID_ARG, "gmm_full_factor: n_runs=%d n_mats=%d D=%d D0=%d",
                n_runs, n_mats, D, D0);
    DIC_REQUIRE(D <= GF_MAX_DIM && D % 4 == 0, DIC_ERR_UNSUPPORTED, "gmm_full_factor: D=%d: at most %d, multiples of 4", D, GF_MAX_DIM);
    DIC_REQUIRE(n_mats <= DIC_MAX_CLUSTERS, DIC_ERR_UNSUPPORTED, "gmm_full_factor: n_mats=%d: at most %d components", n_mats, DIC_MAX_CLUSTERS);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_full_factor: the workspace must be 16-B aligned");
    const size_t need = (size_t)n_runs * n_mats * D * D * sizeof(double);
    DIC_REQUIRE(workspace_bytes >= need, DIC_ERR_WORKSPACE, "gmm_full_factor: workspace %zu < %zu", workspace_bytes, need);
    GfFactor f{};
    f.C = covariances; f.U = (double*)workspace; f.P = prec_chol; f.logdet = log_det; f.status = status; f.d = D; f.d0 = D0; f.kc = n_mats; f.em = 0;
    hipLaunchKernelGGL(gf_factor_kernel, dim3((unsigned)n_mats, (unsigned)n_runs), dim3(GF_THREADS), 0, (hipStream_t)stream, f);
    return check_launch("gmm_full_factor");
}

}  // extern "C"
