// Variational Bayesian Gaussian mixtures with diagonal or spherical covariances, all arithmetic in f64 (sklearn.mixture.BayesianGaussianMixture's model; bgmm.py
// and the p2 / p4 `--cluster_method bgmm` branches).  One iteration is one pass over the f32 points and two small launches; the restarts advance together
// (grid.y).  The structure and the guarantees are dic_gmm.hip's.
// THE DEFINITION (sklearn 1.7.2, mixture/_bayesian_mixture.py, and the loop of mixture/_base.py fit_predict).  c = `shift` (D doubles, the column means the
// Python layer computes).  Every x enters as x' = (double)x - c, one rounded subtraction; the means are kept shifted.  D0 is the true feature count (columns
// D0 .. D - 1 are zero padding: they add nothing to M, their m is 0 and their v is 1, and no sum over d reads them).
// Priors: gamma0 (weight concentration), kappa0 (mean precision), m0 (mean prior, shifted: m0 - c), nu0 (degrees of freedom, > D0 - 1), s0 (covariance prior:
//   D values for diag, one value repeated for spherical).
// Sufficient statistics of responsibilities r:  n_k = sum_i r_ik + 10 * 2^-52,  xbar_k = sum_i r_ik x'_i / n_k,  s_kd = sum_i r_ik x'_id^2 / n_k - xbar_kd^2 +
//   reg_covar  (spherical: s_k = the mean of s_kd over d < D0).
// M-step:  kappa_k = kappa0 + n_k,  m_k = (kappa0 m0 + n_k xbar_k) / kappa_k,  nu_k = nu0 + n_k,
//   diag:       v_kd = (s0_d + n_k (s_kd + (kappa0 / kappa_k) (xbar_kd - m0_d)^2)) / nu_k
//   spherical:  v_k  = (s0 + n_k (s_k + (kappa0 / kappa_k) mean_{d < D0} (xbar_kd - m0_d)^2)) / nu_k
//   dirichlet_process (prior_type 0):  a_k = 1 + n_k,  b_k = gamma0 + sum_{j > k} n_j, the sum accumulated from j = K - 1 downwards (np.cumsum(nk[::-1]))
//   dirichlet_distribution (1):        alpha_k = gamma0 + n_k
// E-step:  M_ik = sum_d (x'_id - m_kd)^2 / v_kd  (here: t = x' - m, q = t t, fma(q, 1 / v, .)),
//   log p_ik = lc_k - M_ik / 2,   lc_k = E[log pi_k] - (D0 log 2 pi) / 2 + l_k + (log_lambda_k - D0 / kappa_k) / 2,
//   l_k = -(sum_{d < D0} log v_kd) / 2 - (D0 log nu_k) / 2,   log_lambda_k = D0 log 2 + sum_{j < D0} psi((nu_k - j) / 2),
//   process:       E[log pi_k] = psi(a_k) - psi(a_k + b_k) + sum_{j < k} (psi(b_j) - psi(a_j + b_j))
//   distribution:  E[log pi_k] = psi(alpha_k) - psi(sum_k alpha_k)
//   lse_i = max_k log p_ik + log sum_k exp(log p_ik - max),   log r_ik = log p_ik - lse_i,   r_ik = exp(log r_ik).
// The lower bound of an iteration is a SUM, from the log r of the iteration's E-step and the parameters AFTER its M-step:
//   lb = -sum_i sum_k r_ik log r_ik - sum_k logW_k - log_norm_weight - (D0 / 2) sum_k log kappa_k,
//   logW_k = -(nu_k l_k + nu_k D0 (log 2) / 2 + sum_{j < D0} lgamma((nu_k - j) / 2)),
//   process:  log_norm_weight = -sum_k (lgamma(a_k) + lgamma(b_k) - lgamma(a_k + b_k));   distribution:  lgamma(sum_k alpha_k) - sum_k lgamma(alpha_k).
//   r log r is taken only where log r is finite (exp underflows to 0 first, as in numpy).
// A restart is done when |lb_t - lb_(t-1)| < tol (lb_0 = -inf) or max_iter is reached; the M-step of the converging iteration is kept.
// THE ORDER OF EVERY SUM IS FIXED, and none depends on a neighbour: sum_d is 4 coordinates per lane in order, then wave_sum's xor tree; sum_k of a row is the
// xor tree over the 64 lanes; sums over rows are sequential over a workgroup's rows, in row order, and then sequential over the workgroups in block order;
// the sums over d < D0 and j < D0 of the reduction and every sum over k of the finish step are sequential in index order, by one thread.  No floating-point
// atomics.  The rows a workgroup takes depend on N alone, and a restart is a grid row of its own: its bits do not depend on the restarts beside it.
//
// THREE LAUNCHES PER ITERATION.  bg_pass_kernel is dic_gmm.hip's gm_pass_kernel (at most 256 workgroups of 4 waves per restart, m and 1 / v in LDS, 2 x 8 K D
// bytes: 128 KiB at K = 32, D = 256; 16 rows at a time) with three changes: lc_k is read from a device array, the partials carry one more word (sum r log r
// over the workgroup's rows, in row order), and the modes for hard labels and given responsibilities serve the initial M-step.  bg_reduce_kernel, one
// workgroup per (component, restart), adds the partials in block order and writes kappa_k, m_k, nu_k, v_k, l_k, log_lambda_k and the lgamma sum: thread j forms
// the j-th psi / lgamma term, and three threads add the three sums in index order.  bg_finish_kernel, one wave per restart, forms the Dirichlet parameters (the
// process's sums sequential, in sklearn's order), E[log pi], the K constants of the next pass, the lower bound, the iteration count and the done decision.
// WHY A THIRD LAUNCH AND NO HAND-OFF: the finish step needs all K reductions of its restart.  Handing it to the last reduction workgroup to arrive would take
// an agent-scope counter with release / acquire fences per restart and a reset of it, for a step that is K <= 32 special-function evaluations long; the launch
// it saves is enqueued behind its predecessor without a host round trip (the host reads the done flags once per _POLL_EVERY iterations), so it costs the
// few microseconds of a dependent launch against an iteration of milliseconds.  A launch boundary keeps the file free of atomics and of workgroups that wait:
// the done flag is written by the finish step alone, after every reader of the iteration has ended.  status[6], which the pass writes, tells the two later
// launches whether the pass ran.
#include "dic_gmm_common.h"

namespace dic {

constexpr int BG_THREADS = 256;
constexpr int BG_WAVES = BG_THREADS / kWave;
constexpr int BG_RPW = 4;                         // rows a wave takes at once
constexpr int BG_TILE = BG_WAVES * BG_RPW;        // rows of a tile
constexpr int BG_MAX_BLOCKS = kNumCU;
constexpr int BG_SLOTS = DIC_MAX_CLUSTERS;        // components a thread of the M-phase can own
constexpr int BG_BATCH = 32;                      // loads in flight of gmm_sum_blocks
constexpr double BG_LOG_2 = 0.6931471805599453;
enum { BG_EM = 0, BG_ESTEP = 1, BG_LABELS = 2, BG_RESP = 3 };
// rows of `comp` (n_runs, DIC_BGMM_COMP_WORDS, K)
enum { BC_NK = 0, BC_KAPPA = 1, BC_NU = 2, BC_L = 3, BC_LOGLAMBDA = 4, BC_LGAMMA = 5, BC_A = 6, BC_B = 7, BC_ELOGPI = 8, BC_LC = 9 };
// status words (f64): 0 done, 1 iterations, 2 stopped by tol, 3 last lower bound, 4 tol, 5 max_iter, 6 (internal) the last pass ran

struct BgArgs {
    const float* X; long ldx;
    int n, d, d0, k, rpb;                         // rpb: rows per workgroup
    const double* shift;
    const double* lc; long lc_stride;             // lc of restart r at lc + r * lc_stride
    const double* mu; const double* var;          // (n_runs, K, D)
    double* status;                               // (n_runs, DIC_GMM_STATUS_WORDS) or NULL
    double* part;                                 // (n_runs, gridDim.x, P) workgroup partials
    const int32_t* labels_in; const double* resp_in;               // (n_runs, N), (n_runs, N, K)
    double* lse; double* log_resp; int32_t* labels;                // E-step outputs, each optional
};

__host__ __device__ inline size_t bg_part_words(int K, int D) { return (size_t)K * (1 + 2 * (size_t)D) + 2; }          // n_k, sum r x', sum r x'^2, sum lse, sum r log r
static int bg_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)BG_MAX_BLOCKS, (N + BG_TILE - 1) / BG_TILE)); }
static size_t bg_lds_bytes(int mode, int K, int D) {
    const size_t params = (mode == BG_EM || mode == BG_ESTEP) ? 2 * (size_t)K * D + K : 0;
    return (params + (size_t)BG_TILE * K + 2 * BG_TILE) * sizeof(double);
}

// psi(x) for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10 (the reciprocals in a compensated sum: near psi's root at 1.4616 the result
// is the small difference of two numbers near 2.3), then the asymptotic series through x^-14, whose first dropped term is below 5e-17 at x = 10.
__device__ inline double bg_digamma(double x) {
#pragma clang fp contract(off)
    if (!(x > 0.0)) return __builtin_nan("");
    double s = 0.0, c = 0.0;
    while (x < 10.0) {
        const double y = 1.0 / x - c;
        const double u = s + y;
        c = (u - s) - y;
        s = u;
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double ser = r2 * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0 - r2 * (691.0 / 32760.0 - r2 * (1.0 / 12.0)))))));
    return (((log(x) - 0.5 * r) - ser) - s) + c;
}

__device__ __forceinline__ double bg_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// The E-step of up to BG_RPW rows (row0 .., nvalid of them) by one wave: r into s_rt, lse into s_lse, sum_k r log r into s_ent, and the optional outputs.
__device__ __forceinline__ void bg_wave_rows(const BgArgs& a, const double* s_mu, const double* s_iv, const double* s_lc, double* s_rt, double* s_lse,
                                             double* s_ent, long long row0, int nvalid, int trow, const double (&c)[4]) {
#pragma clang fp contract(off)
    const int lane = lane_id(), col = 4 * lane, D = a.d, K = a.k;
    double x[BG_RPW][4];
#pragma unroll
    for (int u = 0; u < BG_RPW; ++u) {
        const long long row = row0 + min(u, nvalid - 1);          // (a row past the end repeats the last valid one; its result is dropped)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < D) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + col);
        x[u][0] = (double)v.x - c[0]; x[u][1] = (double)v.y - c[1]; x[u][2] = (double)v.z - c[2]; x[u][3] = (double)v.w - c[3];
    }
    double lp[BG_RPW];
#pragma unroll
    for (int u = 0; u < BG_RPW; ++u) lp[u] = -__builtin_inf();
    for (int k = 0; k < K; ++k) {
        double m[BG_RPW];
#pragma unroll
        for (int u = 0; u < BG_RPW; ++u) m[u] = 0.0;
        if (col < D) {
            const double* pm = s_mu + (size_t)k * D + col;
            const double* pv = s_iv + (size_t)k * D + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double mj = pm[j], vj = pv[j];
#pragma unroll
                for (int u = 0; u < BG_RPW; ++u) {
                    const double t = x[u][j] - mj;
                    const double q = t * t;
                    m[u] = fma(q, vj, m[u]);
                }
            }
        }
        const double lc = s_lc[k];
#pragma unroll
        for (int u = 0; u < BG_RPW; ++u) {
            const double mk = wave_sum(m[u]);
            const double v = lc - 0.5 * mk;
            if (lane == k) lp[u] = v;
        }
    }
#pragma unroll
    for (int u = 0; u < BG_RPW; ++u) {
        const double mx = bg_wave_max(lp[u]);
        const double e = exp(lp[u] - mx);          // (lanes K .. 63: exp(-inf) = 0)
        const double s = wave_sum(e);
        const double lse = mx + log(s);
        const double lr = lp[u] - lse;
        const double r = exp(lr);
        const double ent = wave_sum(isfinite(lr) ? r * lr : 0.0);
        const unsigned long long at_max = __ballot(lp[u] == mx);
        if (u < nvalid) {          // (wave-uniform)
            const long long row = row0 + u;
            if (lane < K) {
                s_rt[(trow + u) * K + lane] = r;
                if (a.log_resp) a.log_resp[(size_t)row * K + lane] = lr;
            }
            if (lane == 0) {
                s_lse[trow + u] = lse;
                s_ent[trow + u] = ent;
                if (a.lse) a.lse[row] = lse;
                if (a.labels) a.labels[row] = at_max ? (int)__builtin_ctzll(at_max) : 0;          // the first maximum
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(BG_THREADS) void bg_pass_kernel(BgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double bg_lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int run = blockIdx.y, K = a.k, D = a.d, n = a.n;
    constexpr bool kParams = MODE == BG_EM || MODE == BG_ESTEP;
    constexpr bool kAccum = MODE != BG_ESTEP;
    if (MODE == BG_EM) {
        const bool done = a.status[(size_t)run * DIC_GMM_STATUS_WORDS] != 0.0;          // (written by the previous finish step, never in this launch)
        if (blockIdx.x == 0 && tid == 0) a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] = done ? 0.0 : 1.0;
        if (done) return;
    }
    double* s_mu = bg_lds;
    double* s_iv = s_mu + (kParams ? (size_t)K * D : 0);
    double* s_lc = s_iv + (kParams ? (size_t)K * D : 0);
    double* s_rt = s_lc + (kParams ? K : 0);
    double* s_lse = s_rt + (size_t)BG_TILE * K;
    double* s_ent = s_lse + BG_TILE;
    if (kParams) {
        const double* mu = a.mu + (size_t)run * K * D;
        const double* var = a.var + (size_t)run * K * D;
        const double* lc = a.lc + (size_t)run * a.lc_stride;
        for (int i = tid; i < K * D; i += BG_THREADS) {
            s_mu[i] = mu[i];
            s_iv[i] = 1.0 / var[i];
        }
        if (tid < K) s_lc[tid] = lc[tid];
        __syncthreads();
    }
    // E-phase: this lane's 4 shifts.  M-phase: this thread's column d and its components g, g + G, ..
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
    if (kParams && 4 * lane < D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c4[j] = a.shift[4 * lane + j];
    }
    const int G = BG_THREADS / D, g = tid / D, d = tid - g * D;
    const bool owner = kAccum && g < G;
    const int nslots = kAccum ? (K + G - 1) / G : 0;          // the same in every thread: a slot past K - 1 repeats component K - 1 and is never stored
    const double cd = kAccum ? a.shift[d] : 0.0;
    double sx[BG_SLOTS], sxx[BG_SLOTS];
#pragma unroll
    for (int j = 0; j < BG_SLOTS; ++j) { sx[j] = 0.0; sxx[j] = 0.0; }
    double pn = 0.0, pl = 0.0, pe = 0.0;

    const long long r0 = (long long)blockIdx.x * a.rpb;
    const long long r1 = min((long long)n, r0 + a.rpb);
    for (long long t0 = r0; t0 < r1; t0 += BG_TILE) {
        const int nt = (int)min((long long)BG_TILE, r1 - t0);
        if (kParams) {
            const int nvalid = min(BG_RPW, nt - BG_RPW * w);
            if (nvalid > 0) bg_wave_rows(a, s_mu, s_iv, s_lc, s_rt, s_lse, s_ent, t0 + BG_RPW * w, nvalid, BG_RPW * w, c4);
        } else {
            for (int i = tid; i < nt * K; i += BG_THREADS) {
                const int r = i / K, k = i - r * K;
                const size_t row = (size_t)run * n + (size_t)(t0 + r);
                s_rt[i] = MODE == BG_LABELS ? (a.labels_in[row] == k ? 1.0 : 0.0) : a.resp_in[row * K + k];
            }
            if (tid < nt) { s_lse[tid] = 0.0; s_ent[tid] = 0.0; }
        }
        __syncthreads();
        if (kAccum) {
            for (int i = 0; i < nt; ++i) {          // (no thread-dependent branch: threads that own nothing add into slots they never store)
#pragma clang fp contract(off)
                const double xv = (double)a.X[(size_t)(t0 + i) * a.ldx + d] - cd;
                const double* rr = s_rt + i * K;
#pragma unroll
                for (int j = 0; j < BG_SLOTS; ++j) {
                    if (j < nslots) {
                        const double t = rr[min(g + j * G, K - 1)] * xv;
                        sx[j] = sx[j] + t;
                        sxx[j] = fma(t, xv, sxx[j]);
                    }
                }
            }
            if (tid < K)
                for (int i = 0; i < nt; ++i) pn += s_rt[i * K + tid];
            if (tid == kWave)
                for (int i = 0; i < nt; ++i) pe += s_ent[i];
        }
        if (tid == 0)
            for (int i = 0; i < nt; ++i) pl += s_lse[i];
        __syncthreads();          // (the tile is rewritten)
    }
    double* part = a.part + ((size_t)run * gridDim.x + blockIdx.x) * (kAccum ? bg_part_words(K, D) : 1);
    if (kAccum) {
        if (owner) {
#pragma unroll
            for (int j = 0; j < BG_SLOTS; ++j) {
                if (j < nslots && g + j * G < K) {
                    const size_t o = (size_t)(g + j * G) * D + d;
                    part[K + o] = sx[j];
                    part[K + (size_t)K * D + o] = sxx[j];
                }
            }
        }
        if (tid < K) part[tid] = pn;
        if (tid == 0) part[K + 2 * (size_t)K * D] = pl;
        if (tid == kWave) part[K + 2 * (size_t)K * D + 1] = pe;
    } else if (tid == 0) {
        part[0] = pl;
    }
}

struct BgReduce {
    const double* part; int nblk;
    int d, d0, k, cov_type, prior_type, em, lb_stride;
    double reg, gamma0, kappa0, nu0;
    const double* m0; const double* s0;          // (D) each, shared by the restarts
    double* mu; double* var; double* comp; double* status; double* lower_bounds;
};

__device__ __forceinline__ double* bg_comp(const BgReduce& a, int run, int word) { return a.comp + ((size_t)run * DIC_BGMM_COMP_WORDS + word) * a.k; }

// one workgroup per (component, restart): the partials of the pass in block order, then the Gaussian and Wishart parameters of the component
__global__ __launch_bounds__(BG_THREADS) void bg_reduce_kernel(BgReduce a) {
#pragma clang fp contract(off)
    __shared__ double s_v[BG_THREADS], s_psi[BG_THREADS], s_lg[BG_THREADS];
    __shared__ double s_one[2];
    const int tid = threadIdx.x, k = blockIdx.x, run = blockIdx.y, K = a.k, D = a.d, D0 = a.d0;
    if (a.em && a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] == 0.0) return;          // (the pass skipped this restart: it was done)
    const size_t P = bg_part_words(K, D);
    const double* part = a.part + (size_t)run * a.nblk * P;
    if (tid == 0) s_one[0] = gmm_sum_blocks<BG_BATCH>(part + k, P, a.nblk) + GMM_NK_EPS;
    __syncthreads();
    const double nk = s_one[0];
    const double kap = a.kappa0 + nk, nu = a.nu0 + nk;
    const double ratio = a.kappa0 / kap;
    double s = 0.0, dd = 0.0, m = 0.0, s0 = 0.0;
    if (tid < D0) {
        const size_t o = (size_t)k * D + tid;
        const double sx = gmm_sum_blocks<BG_BATCH>(part + K + o, P, a.nblk);
        const double sxx = gmm_sum_blocks<BG_BATCH>(part + K + (size_t)K * D + o, P, a.nblk);
        const double xb = sx / nk;
        const double e2 = sxx / nk;
        const double x2 = xb * xb;
        s = (e2 - x2) + a.reg;
        const double m0 = a.m0[tid];
        const double diff = xb - m0;
        dd = diff * diff;
        m = (a.kappa0 * m0 + nk * xb) / kap;
        s0 = a.s0[tid];
    }
    if (a.cov_type == 1) {          // spherical: the means over the true columns, in column order
        s_v[tid] = s;
        s_psi[tid] = dd;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int j = 0; j < D0; ++j) t += s_v[j];
            s_one[0] = t / (double)D0;
        }
        if (tid == kWave) {
            double t = 0.0;
            for (int j = 0; j < D0; ++j) t += s_psi[j];
            s_one[1] = t / (double)D0;
        }
        __syncthreads();
        s = s_one[0];
        dd = s_one[1];
        __syncthreads();          // (s_v and s_psi are rewritten below)
    }
    double v = 1.0;          // (the padding: m = 0, v = 1)
    if (tid < D0) v = (s0 + nk * (s + ratio * dd)) / nu;
    if (tid < D) {
        a.mu[((size_t)run * K + k) * D + tid] = m;
        a.var[((size_t)run * K + k) * D + tid] = v;
    }
    const bool term = tid < D0;
    const double half = 0.5 * (nu - (double)tid);
    s_v[tid] = term ? log(v) : 0.0;
    s_psi[tid] = term ? bg_digamma(half) : 0.0;
    s_lg[tid] = term ? lgamma(half) : 0.0;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int j = 0; j < D0; ++j) t += s_v[j];
        bg_comp(a, run, BC_NK)[k] = nk;
        bg_comp(a, run, BC_KAPPA)[k] = kap;
        bg_comp(a, run, BC_NU)[k] = nu;
        bg_comp(a, run, BC_L)[k] = -0.5 * t - (0.5 * (double)D0) * log(nu);
    }
    if (tid == kWave) {
        double t = 0.0;
        for (int j = 0; j < D0; ++j) t += s_psi[j];
        bg_comp(a, run, BC_LOGLAMBDA)[k] = (double)D0 * BG_LOG_2 + t;
    }
    if (tid == 2 * kWave) {
        double t = 0.0;
        for (int j = 0; j < D0; ++j) t += s_lg[j];
        bg_comp(a, run, BC_LGAMMA)[k] = t;
    }
}

// one wave per restart: the Dirichlet parameters, E[log pi], the constants of the next pass, and with `em` the lower bound and the end of the iteration
__global__ __launch_bounds__(kWave) void bg_finish_kernel(BgReduce a) {
#pragma clang fp contract(off)
    __shared__ double s_n[DIC_MAX_CLUSTERS], s_a[DIC_MAX_CLUSTERS], s_b[DIC_MAX_CLUSTERS], s_pa[DIC_MAX_CLUSTERS], s_pd[DIC_MAX_CLUSTERS],
        s_ln[DIC_MAX_CLUSTERS], s_e[DIC_MAX_CLUSTERS];
    __shared__ double s_one[2];
    const int tid = threadIdx.x, run = blockIdx.x, K = a.k;
    double* st = a.status ? a.status + (size_t)run * DIC_GMM_STATUS_WORDS : nullptr;
    if (a.em && st[6] == 0.0) return;
    const double d0 = (double)a.d0;
    if (tid < K) s_n[tid] = bg_comp(a, run, BC_NK)[tid];
    if (a.em && tid == K) {          // (K <= 32 < 64: a lane beside the components')
        const size_t P = bg_part_words(K, a.d);
        s_one[0] = gmm_sum_blocks<BG_BATCH>(a.part + (size_t)run * a.nblk * P + (P - 1), P, a.nblk);
    }
    __syncthreads();
    double log_norm = 0.0;
    if (a.prior_type == 0) {
        if (tid == 0) {          // b_k = gamma0 + (n_(K-1) + .. + n_(k+1)), accumulated downwards
            double c = 0.0;
            s_b[K - 1] = a.gamma0 + 0.0;
            for (int j = K - 2; j >= 0; --j) {
                c += s_n[j + 1];
                s_b[j] = a.gamma0 + c;
            }
        }
        __syncthreads();
        if (tid < K) {
            const double av = 1.0 + s_n[tid], bv = s_b[tid], ab = av + bv;
            const double pab = bg_digamma(ab);
            s_a[tid] = av;
            s_pa[tid] = bg_digamma(av) - pab;
            s_pd[tid] = bg_digamma(bv) - pab;
            s_ln[tid] = (lgamma(av) + lgamma(bv)) - lgamma(ab);          // betaln
        }
        __syncthreads();
        if (tid == 0) {
            double cum = 0.0, t = 0.0;
            for (int j = 0; j < K; ++j) {
                s_e[j] = s_pa[j] + cum;
                cum += s_pd[j];
                t += s_ln[j];
            }
            log_norm = -t;
        }
    } else {
        if (tid < K) {
            const double al = a.gamma0 + s_n[tid];
            s_a[tid] = al;
            s_b[tid] = 0.0;
            s_pa[tid] = bg_digamma(al);
            s_ln[tid] = lgamma(al);
        }
        __syncthreads();
        if (tid == 0) {
            double sa = 0.0, t = 0.0;
            for (int j = 0; j < K; ++j) { sa += s_a[j]; t += s_ln[j]; }
            const double ps = bg_digamma(sa);
            for (int j = 0; j < K; ++j) s_e[j] = s_pa[j] - ps;
            log_norm = lgamma(sa) - t;
        }
    }
    __syncthreads();
    if (tid < K) {
        const double kap = bg_comp(a, run, BC_KAPPA)[tid];
        const double lk = bg_comp(a, run, BC_L)[tid];
        const double ll = bg_comp(a, run, BC_LOGLAMBDA)[tid];
        bg_comp(a, run, BC_A)[tid] = s_a[tid];
        bg_comp(a, run, BC_B)[tid] = s_b[tid];
        bg_comp(a, run, BC_ELOGPI)[tid] = s_e[tid];
        bg_comp(a, run, BC_LC)[tid] = ((s_e[tid] - 0.5 * (d0 * GMM_LOG_2PI)) + lk) + 0.5 * (ll - d0 / kap);
        if (a.em) {
            const double nu = bg_comp(a, run, BC_NU)[tid];
            s_pa[tid] = -((nu * lk + nu * d0 * 0.5 * BG_LOG_2) + bg_comp(a, run, BC_LGAMMA)[tid]);          // logW_k
            s_pd[tid] = log(kap);
        }
    }
    __syncthreads();
    if (a.em && tid == 0) {
        double sw = 0.0, sk = 0.0;
        for (int j = 0; j < K; ++j) { sw += s_pa[j]; sk += s_pd[j]; }
        const double lb = ((-s_one[0] - sw) - log_norm) - (0.5 * d0) * sk;
        gmm_end_iteration(st, lb, 1.0, a.lower_bounds, a.lb_stride, run);          // (the bound is a sum: divided by 1)
    }
}

__global__ void bg_sum_kernel(const double* part, int nblk, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = gmm_sum_blocks<BG_BATCH>(part, 1, nblk);
}

__global__ void bg_probe_kernel(const double* x, long long n, double* digamma_out, double* lgamma_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (digamma_out) digamma_out[i] = bg_digamma(x[i]);
    if (lgamma_out) lgamma_out[i] = lgamma(x[i]);
}

template <int MODE>
static int bg_launch_pass(const char* what, const BgArgs& a, int nblk, int n_runs, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        const int most = (int)bg_lds_bytes(MODE, DIC_MAX_CLUSTERS, 4 * kWave);
        hipError_t e = hipFuncSetAttribute((const void*)bg_pass_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", what, most, hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(bg_pass_kernel<MODE>, dim3((unsigned)nblk, (unsigned)n_runs), dim3(BG_THREADS), bg_lds_bytes(MODE, a.k, a.d), st, a);
    return DIC_OK;
}

// the checks init and em_iter share, after the points'
static int bg_check_model(const char* what, int D0, int n_runs, int cov_type, int prior_type, double reg_covar, double gamma0, double kappa0, double nu0,
                          const void* workspace, size_t workspace_bytes, size_t need) {
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && (cov_type == 0 || cov_type == 1) && (prior_type == 0 || prior_type == 1) && reg_covar >= 0.0,
                DIC_ERR_INVALID_ARG, "%s: n_runs=%d cov_type=%d prior_type=%d reg_covar=%g", what, n_runs, cov_type, prior_type, reg_covar);
    const double big = 1.7976931348623157e308;          // (a > 0 && a <= big: positive and finite, false for NaN)
    DIC_REQUIRE(gamma0 > 0.0 && gamma0 <= big && kappa0 > 0.0 && kappa0 <= big && nu0 > (double)(D0 - 1) && nu0 <= big, DIC_ERR_INVALID_ARG,
                "%s: priors gamma0=%g kappa0=%g nu0=%g: expected positive values and nu0 > D0 - 1 = %d", what, gamma0, kappa0, nu0, D0 - 1);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "%s: the workspace must be 16-B aligned", what);
    DIC_REQUIRE(workspace_bytes >= need, DIC_ERR_WORKSPACE, "%s: workspace %zu < %zu", what, workspace_bytes, need);
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_bgmm_workspace(int64_t N, int D, int K, int n_runs) {
    if (N < 2 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave || K < 1 || K > DIC_MAX_CLUSTERS || n_runs < 1) return 0;
    return align_up((size_t)n_runs * bg_blocks(N) * bg_part_words(K, D) * sizeof(double), 256);
}

int dic_bgmm_init(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, int prior_type, double reg_covar, double gamma0,
                  double kappa0, double nu0, const double* shift, const double* mean_prior, const double* cov_prior, const int32_t* labels, const double* resp,
                  double* means, double* variances, double* comp, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gmm_check_points("bgmm_init", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && mean_prior && cov_prior && means && variances && comp && workspace, DIC_ERR_INVALID_ARG, "bgmm_init: NULL pointer");
    DIC_REQUIRE((labels != nullptr) != (resp != nullptr), DIC_ERR_INVALID_ARG, "bgmm_init: exactly one of labels and resp");
    const int rm = bg_check_model("bgmm_init", D0, n_runs, cov_type, prior_type, reg_covar, gamma0, kappa0, nu0, workspace, workspace_bytes,
                                  dic_bgmm_workspace(N, D, K, n_runs));
    if (rm) return rm;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bg_blocks(N);
    BgArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.part = (double*)workspace; a.labels_in = labels; a.resp_in = resp;
    const int rl = labels ? bg_launch_pass<BG_LABELS>("bgmm_init", a, nblk, n_runs, st) : bg_launch_pass<BG_RESP>("bgmm_init", a, nblk, n_runs, st);
    if (rl) return rl;
    BgReduce r{};
    r.part = a.part; r.nblk = nblk; r.d = D; r.d0 = D0; r.k = K; r.cov_type = cov_type; r.prior_type = prior_type; r.em = 0; r.lb_stride = 0;
    r.reg = reg_covar; r.gamma0 = gamma0; r.kappa0 = kappa0; r.nu0 = nu0; r.m0 = mean_prior; r.s0 = cov_prior;
    r.mu = means; r.var = variances; r.comp = comp;
    hipLaunchKernelGGL(bg_reduce_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(BG_THREADS), 0, st, r);
    hipLaunchKernelGGL(bg_finish_kernel, dim3((unsigned)n_runs), dim3(kWave), 0, st, r);
    return check_launch("bgmm_init");
}

int dic_bgmm_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, int prior_type, double reg_covar, double gamma0,
                     double kappa0, double nu0, const double* shift, const double* mean_prior, const double* cov_prior, double* means, double* variances,
                     double* comp, double* status, double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gmm_check_points("bgmm_em_iter", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && mean_prior && cov_prior && means && variances && comp && status && lower_bounds && workspace, DIC_ERR_INVALID_ARG,
                "bgmm_em_iter: NULL pointer");
    DIC_REQUIRE(lb_stride >= 1, DIC_ERR_INVALID_ARG, "bgmm_em_iter: lb_stride=%d", lb_stride);
    const int rm = bg_check_model("bgmm_em_iter", D0, n_runs, cov_type, prior_type, reg_covar, gamma0, kappa0, nu0, workspace, workspace_bytes,
                                  dic_bgmm_workspace(N, D, K, n_runs));
    if (rm) return rm;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bg_blocks(N);
    BgArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.lc = comp + (size_t)BC_LC * K; a.lc_stride = (long)DIC_BGMM_COMP_WORDS * K; a.mu = means; a.var = variances; a.status = status;
    a.part = (double*)workspace;
    const int rl = bg_launch_pass<BG_EM>("bgmm_em_iter", a, nblk, n_runs, st);
    if (rl) return rl;
    BgReduce r{};
    r.part = a.part; r.nblk = nblk; r.d = D; r.d0 = D0; r.k = K; r.cov_type = cov_type; r.prior_type = prior_type; r.em = 1; r.lb_stride = lb_stride;
    r.reg = reg_covar; r.gamma0 = gamma0; r.kappa0 = kappa0; r.nu0 = nu0; r.m0 = mean_prior; r.s0 = cov_prior;
    r.mu = means; r.var = variances; r.comp = comp; r.status = status; r.lower_bounds = lower_bounds;
    hipLaunchKernelGGL(bg_reduce_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(BG_THREADS), 0, st, r);
    hipLaunchKernelGGL(bg_finish_kernel, dim3((unsigned)n_runs), dim3(kWave), 0, st, r);
    return check_launch("bgmm_em_iter");
}

int dic_bgmm_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, const double* shift, const double* log_const, const double* means,
                   const double* variances, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace, size_t workspace_bytes,
                   dic_stream_t stream) {
    const int rc = gmm_check_points("bgmm_estep", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && log_const && means && variances && workspace, DIC_ERR_INVALID_ARG, "bgmm_estep: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "bgmm_estep: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_bgmm_workspace(N, D, K, 1), DIC_ERR_WORKSPACE, "bgmm_estep: workspace %zu < %zu", workspace_bytes,
                dic_bgmm_workspace(N, D, K, 1));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bg_blocks(N);
    BgArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.lc = log_const; a.lc_stride = 0; a.mu = means; a.var = variances; a.part = (double*)workspace;
    a.lse = lse; a.log_resp = log_resp; a.labels = labels;
    const int rl = bg_launch_pass<BG_ESTEP>("bgmm_estep", a, nblk, 1, st);
    if (rl) return rl;
    if (sum_lse) hipLaunchKernelGGL(bg_sum_kernel, dim3(1), dim3(kWave), 0, st, (const double*)a.part, nblk, sum_lse);
    return check_launch("bgmm_estep");
}

int dic_bgmm_special_probe(const double* x, int64_t n, double* digamma_out, double* lgamma_out) {
    DIC_REQUIRE(x && (digamma_out || lgamma_out), DIC_ERR_INVALID_ARG, "bgmm_special_probe: NULL pointer");
    DIC_REQUIRE(n >= 1 && n < (1LL << 30), DIC_ERR_INVALID_ARG, "bgmm_special_probe: n=%lld", (long long)n);
    hipLaunchKernelGGL(bg_probe_kernel, dim3((unsigned)((n + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, (hipStream_t) nullptr, x, (long long)n,
                       digamma_out, lgamma_out);
    return check_launch("bgmm_special_probe");
}

}  // extern "C"
