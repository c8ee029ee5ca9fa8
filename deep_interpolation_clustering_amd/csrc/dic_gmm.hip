// Gaussian mixtures with diagonal or spherical covariances by EM, all arithmetic in f64 (sklearn.mixture.GaussianMixture's model; gmm.py and the p2 / p4
// `--cluster_method gmm` branches).  One EM iteration is one pass over the f32 points and a small reduction; the restarts advance together (grid.y).
// THE DEFINITION.  c = `shift` (D doubles, the column means the Python layer computes).  Every x enters as x' = (double)x - c, one rounded subtraction; the means
// are kept as mu' = mu - c.  With D0 the true feature count (columns D0 .. D - 1 are zero padding: they add nothing to M, and their variances are skipped)
//   M_ik     = sum_d (x'_id - mu'_kd)^2 / v_kd                                  (here: t = x' - mu', q = t t, fma(q, 1 / v, .))
//   log p_ik = log w_k - (D0 log 2 pi) / 2 - (sum_{d < D0} log v_kd) / 2 - M_ik / 2
//   lse_i    = max_k log p_ik + log sum_k exp(log p_ik - max),   log r_ik = log p_ik - lse_i,   r_ik = exp(log r_ik)
//   n_k = sum_i r_ik + 10 * 2^-52,  mu'_k = sum_i r_ik x'_i / n_k,  v_kd = sum_i r_ik x'_id^2 / n_k - mu'_kd^2 + reg_covar  (spherical: the mean over d < D0),
//   w_k = (n_k / N) / sum_k (n_k / N);  the lower bound of an iteration is sum_i lse_i / N.
// THE ORDER OF EVERY SUM IS FIXED, and none depends on a neighbour: sum_d is 4 coordinates per lane in order, then wave_sum's xor tree; sum_k is the xor tree
// over the 64 lanes (lane k holds component k, the others exp(-inf) = 0); sums over rows are sequential over a workgroup's rows, in row order, by the one
// thread that owns (k, d), and then sequential over the workgroups in block order (gm_mstep_kernel).  No floating-point atomics.  The rows a workgroup takes
// depend on N alone, and a restart is a grid row of its own: its bits do not depend on the restarts beside it.
//
// A PASS (gm_pass_kernel) is at most 256 workgroups of 4 waves per restart.  A workgroup holds its restart's mu' and 1 / v in LDS (2 x 8 K D bytes: 128 KiB at
// K = 32, D = 256) and takes its rows 16 at a time.  E-phase: a wave takes 4 rows at once -- a lane holds 4 coordinates of each, so one read of mu' and 1 / v
// from LDS serves 4 rows -- and leaves r (16, K) and lse (16) in LDS.  M-phase: thread (d, g) owns the components k = g, g + G, .. (G = 256 / D groups) of
// column d, re-reads x_d of the 16 rows (cache hits) and adds r x' and r x'^2 into registers.  At the end the workgroup stores its partial sums.
// gm_mstep_kernel, one workgroup per (component, restart), adds the partials in block order and writes the new parameters; the workgroup of component 0
// appends the lower bound, counts the iteration and decides whether the restart is done: |lb_t - lb_(t-1)| < tol (lb_0 = -inf), or max_iter reached.  As in
// sklearn the M-step of the converging iteration is kept.  A done restart is skipped by both kernels: status[6], which the pass writes and the reduction
// reads, tells the reduction whether its pass ran -- the done flag itself is rewritten by the reduction's component-0 workgroup while the others may not have
// started.
#include "dic_gmm_common.h"

namespace dic {

constexpr int GM_THREADS = 256;
constexpr int GM_WAVES = GM_THREADS / kWave;
constexpr int GM_RPW = 4;                         // rows a wave takes at once
constexpr int GM_TILE = GM_WAVES * GM_RPW;        // rows of a tile
constexpr int GM_MAX_BLOCKS = kNumCU;
constexpr int GM_SLOTS = DIC_MAX_CLUSTERS;        // components a thread of the M-phase can own
enum { GM_EM = 0, GM_ESTEP = 1, GM_LABELS = 2, GM_RESP = 3 };
// status words (f64): 0 done, 1 iterations, 2 stopped by tol, 3 last lower bound, 4 tol, 5 max_iter, 6 (internal) the last pass ran

struct GmArgs {
    const float* X; long ldx;
    int n, d, d0, k, rpb;                         // rpb: rows per workgroup
    const double* shift;
    const double* w; const double* mu; const double* var;          // (n_runs, K), (n_runs, K, D), (n_runs, K, D)
    double* status;                               // (n_runs, DIC_GMM_STATUS_WORDS) or NULL
    double* part;                                 // (n_runs, gridDim.x, P) workgroup partials
    const int32_t* labels_in; const double* resp_in;               // (n_runs, N), (n_runs, N, K)
    double* lse; double* log_resp; int32_t* labels;                // E-step outputs, each optional
};

__host__ __device__ inline size_t gm_part_words(int K, int D) { return (size_t)K * (1 + 2 * (size_t)D) + 1; }          // n_k, sum r x', sum r x'^2, sum lse
static int gm_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)GM_MAX_BLOCKS, (N + GM_TILE - 1) / GM_TILE)); }
static size_t gm_lds_bytes(int mode, int K, int D) {
    const size_t params = (mode == GM_EM || mode == GM_ESTEP) ? 2 * (size_t)K * D + K : 0;
    return (params + (size_t)GM_TILE * K + GM_TILE) * sizeof(double);
}

__device__ __forceinline__ double gm_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// The E-step of up to GM_RPW rows (row0 .., nvalid of them) by one wave: r into s_rt, lse into s_lse, and the optional outputs.
__device__ __forceinline__ void gm_wave_rows(const GmArgs& a, const double* s_mu, const double* s_iv, const double* s_lc, double* s_rt, double* s_lse,
                                             long long row0, int nvalid, int trow, const double (&c)[4]) {
#pragma clang fp contract(off)
    const int lane = lane_id(), col = 4 * lane, D = a.d, K = a.k;
    double x[GM_RPW][4];
#pragma unroll
    for (int u = 0; u < GM_RPW; ++u) {
        const long long row = row0 + min(u, nvalid - 1);          // (a row past the end repeats the last valid one; its result is dropped)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < D) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + col);
        x[u][0] = (double)v.x - c[0]; x[u][1] = (double)v.y - c[1]; x[u][2] = (double)v.z - c[2]; x[u][3] = (double)v.w - c[3];
    }
    double lp[GM_RPW];
#pragma unroll
    for (int u = 0; u < GM_RPW; ++u) lp[u] = -__builtin_inf();
    for (int k = 0; k < K; ++k) {
        double m[GM_RPW];
#pragma unroll
        for (int u = 0; u < GM_RPW; ++u) m[u] = 0.0;
        if (col < D) {
            const double* pm = s_mu + (size_t)k * D + col;
            const double* pv = s_iv + (size_t)k * D + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double mj = pm[j], vj = pv[j];
#pragma unroll
                for (int u = 0; u < GM_RPW; ++u) {
                    const double t = x[u][j] - mj;
                    const double q = t * t;
                    m[u] = fma(q, vj, m[u]);
                }
            }
        }
        const double lc = s_lc[k];
#pragma unroll
        for (int u = 0; u < GM_RPW; ++u) {
            const double mk = wave_sum(m[u]);
            const double v = lc - 0.5 * mk;
            if (lane == k) lp[u] = v;
        }
    }
#pragma unroll
    for (int u = 0; u < GM_RPW; ++u) {
        const double mx = gm_wave_max(lp[u]);
        const double e = exp(lp[u] - mx);          // (lanes K .. 63: exp(-inf) = 0)
        const double s = wave_sum(e);
        const double lse = mx + log(s);
        const double lr = lp[u] - lse;
        const unsigned long long at_max = __ballot(lp[u] == mx);
        if (u < nvalid) {          // (wave-uniform)
            const long long row = row0 + u;
            if (lane < K) {
                s_rt[(trow + u) * K + lane] = exp(lr);
                if (a.log_resp) a.log_resp[(size_t)row * K + lane] = lr;
            }
            if (lane == 0) {
                s_lse[trow + u] = lse;
                if (a.lse) a.lse[row] = lse;
                if (a.labels) a.labels[row] = at_max ? (int)__builtin_ctzll(at_max) : 0;          // the first maximum
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(GM_THREADS) void gm_pass_kernel(GmArgs a) {
    extern __shared__ double gm_lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int run = blockIdx.y, K = a.k, D = a.d, n = a.n;
    constexpr bool kParams = MODE == GM_EM || MODE == GM_ESTEP;
    constexpr bool kAccum = MODE != GM_ESTEP;
    if (MODE == GM_EM) {
        const bool done = a.status[(size_t)run * DIC_GMM_STATUS_WORDS] != 0.0;          // (written by the previous reduction, never in this launch)
        if (blockIdx.x == 0 && tid == 0) a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] = done ? 0.0 : 1.0;
        if (done) return;
    }
    double* s_mu = gm_lds;
    double* s_iv = s_mu + (kParams ? (size_t)K * D : 0);
    double* s_lc = s_iv + (kParams ? (size_t)K * D : 0);
    double* s_rt = s_lc + (kParams ? K : 0);
    double* s_lse = s_rt + (size_t)GM_TILE * K;
    if (kParams) {
        const double* mu = a.mu + (size_t)run * K * D;
        const double* var = a.var + (size_t)run * K * D;
        const double* wt = a.w + (size_t)run * K;
        for (int i = tid; i < K * D; i += GM_THREADS) {
            s_mu[i] = mu[i];
            s_iv[i] = 1.0 / var[i];
        }
        for (int k = w; k < K; k += GM_WAVES) {
#pragma clang fp contract(off)
            double s = 0.0;
            for (int d = lane; d < a.d0; d += kWave) s += log(var[(size_t)k * D + d]);
            s = wave_sum(s);
            if (lane == 0) s_lc[k] = (log(wt[k]) - 0.5 * ((double)a.d0 * GMM_LOG_2PI)) - 0.5 * s;
        }
        __syncthreads();
    }
    // E-phase: this lane's 4 shifts.  M-phase: this thread's column d and its components g, g + G, ..
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
    if (kParams && 4 * lane < D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c4[j] = a.shift[4 * lane + j];
    }
    const int G = GM_THREADS / D, g = tid / D, d = tid - g * D;
    const bool owner = kAccum && g < G;
    const int nslots = kAccum ? (K + G - 1) / G : 0;          // the same in every thread: a slot past K - 1 repeats component K - 1 and is never stored
    const double cd = kAccum ? a.shift[d] : 0.0;
    double sx[GM_SLOTS], sxx[GM_SLOTS];
#pragma unroll
    for (int j = 0; j < GM_SLOTS; ++j) { sx[j] = 0.0; sxx[j] = 0.0; }
    double pn = 0.0, pl = 0.0;

    const long long r0 = (long long)blockIdx.x * a.rpb;
    const long long r1 = min((long long)n, r0 + a.rpb);
    for (long long t0 = r0; t0 < r1; t0 += GM_TILE) {
        const int nt = (int)min((long long)GM_TILE, r1 - t0);
        if (kParams) {
            const int nvalid = min(GM_RPW, nt - GM_RPW * w);
            if (nvalid > 0) gm_wave_rows(a, s_mu, s_iv, s_lc, s_rt, s_lse, t0 + GM_RPW * w, nvalid, GM_RPW * w, c4);
        } else {
            for (int i = tid; i < nt * K; i += GM_THREADS) {
                const int r = i / K, k = i - r * K;
                const size_t row = (size_t)run * n + (size_t)(t0 + r);
                s_rt[i] = MODE == GM_LABELS ? (a.labels_in[row] == k ? 1.0 : 0.0) : a.resp_in[row * K + k];
            }
            if (tid < nt) s_lse[tid] = 0.0;
        }
        __syncthreads();
        if (kAccum) {
            for (int i = 0; i < nt; ++i) {          // (no thread-dependent branch: threads that own nothing add into slots they never store)
#pragma clang fp contract(off)
                const double xv = (double)a.X[(size_t)(t0 + i) * a.ldx + d] - cd;
                const double* rr = s_rt + i * K;
#pragma unroll
                for (int j = 0; j < GM_SLOTS; ++j) {
                    if (j < nslots) {
                        const double t = rr[min(g + j * G, K - 1)] * xv;
                        sx[j] = sx[j] + t;
                        sxx[j] = fma(t, xv, sxx[j]);
                    }
                }
            }
            if (tid < K)
                for (int i = 0; i < nt; ++i) pn += s_rt[i * K + tid];
        }
        if (tid == 0)
            for (int i = 0; i < nt; ++i) pl += s_lse[i];
        __syncthreads();          // (the tile is rewritten)
    }
    double* part = a.part + ((size_t)run * gridDim.x + blockIdx.x) * (kAccum ? gm_part_words(K, D) : 1);
    if (kAccum) {
        if (owner) {
#pragma unroll
            for (int j = 0; j < GM_SLOTS; ++j) {
                if (j < nslots && g + j * G < K) {
                    const size_t o = (size_t)(g + j * G) * D + d;
                    part[K + o] = sx[j];
                    part[K + (size_t)K * D + o] = sxx[j];
                }
            }
        }
        if (tid < K) part[tid] = pn;
        if (tid == 0) part[K + 2 * (size_t)K * D] = pl;
    } else if (tid == 0) {
        part[0] = pl;
    }
}

constexpr int GM_BATCH = 32;          // loads in flight of gmm_sum_blocks

struct GmReduce {
    const double* part; int nblk;
    int n, d, d0, k, cov_type, em, lb_stride;
    double reg;
    double* w; double* mu; double* var; double* status; double* lower_bounds;
};

// one workgroup per (component, restart): the partials of the pass in block order, then the M-step
__global__ __launch_bounds__(GM_THREADS) void gm_mstep_kernel(GmReduce a) {
#pragma clang fp contract(off)
    __shared__ double s_n[DIC_MAX_CLUSTERS];
    __shared__ double s_v[4 * kWave];
    __shared__ double s_mean, s_lse;
    const int tid = threadIdx.x, k = blockIdx.x, run = blockIdx.y, K = a.k, D = a.d;
    double* st = a.status ? a.status + (size_t)run * DIC_GMM_STATUS_WORDS : nullptr;
    if (a.em && st[6] == 0.0) return;          // (the pass skipped this restart: it was done)
    const size_t P = gm_part_words(K, D);
    const double* part = a.part + (size_t)run * a.nblk * P;
    if (tid < K) s_n[tid] = gmm_sum_blocks<GM_BATCH>(part + tid, P, a.nblk) + GMM_NK_EPS;
    if (a.em && k == 0 && tid == kWave) s_lse = gmm_sum_blocks<GM_BATCH>(part + K + 2 * (size_t)K * D, P, a.nblk);          // (the second wave, beside the first's n_k)
    __syncthreads();
    const double nk = s_n[k];
    double v = 0.0;
    if (tid < D) {
        const size_t o = (size_t)k * D + tid;
        const double sx = gmm_sum_blocks<GM_BATCH>(part + K + o, P, a.nblk);
        const double sxx = gmm_sum_blocks<GM_BATCH>(part + K + (size_t)K * D + o, P, a.nblk);
        const double m = sx / nk;
        const double e2 = sxx / nk;
        const double m2 = m * m;
        v = (e2 - m2) + a.reg;
        a.mu[((size_t)run * K + k) * D + tid] = m;
    }
    if (a.cov_type == 1) {          // spherical: the mean over the true columns, in column order
        s_v[tid] = v;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int j = 0; j < a.d0; ++j) s += s_v[j];
            s_mean = s / (double)a.d0;
        }
        __syncthreads();
        v = s_mean;
    }
    if (tid < D) a.var[((size_t)run * K + k) * D + tid] = v;
    if (tid == 0) {
        const double fn = (double)a.n;
        double ws = 0.0;
        for (int j = 0; j < K; ++j) ws += s_n[j] / fn;
        a.w[(size_t)run * K + k] = (nk / fn) / ws;
        if (a.em && k == 0) gmm_end_iteration(st, s_lse, fn, a.lower_bounds, a.lb_stride, run);
    }
}

__global__ void gm_sum_kernel(const double* part, int nblk, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = gmm_sum_blocks<GM_BATCH>(part, 1, nblk);
}

template <int MODE>
static int gm_launch_pass(const char* what, const GmArgs& a, int nblk, int n_runs, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        const int most = (int)gm_lds_bytes(MODE, DIC_MAX_CLUSTERS, 4 * kWave);
        hipError_t e = hipFuncSetAttribute((const void*)gm_pass_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", what, most, hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(gm_pass_kernel<MODE>, dim3((unsigned)nblk, (unsigned)n_runs), dim3(GM_THREADS), gm_lds_bytes(MODE, a.k, a.d), st, a);
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_gmm_workspace(int64_t N, int D, int K, int n_runs) {
    if (N < 2 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave || K < 1 || K > DIC_MAX_CLUSTERS || n_runs < 1) return 0;
    return align_up((size_t)n_runs * gm_blocks(N) * gm_part_words(K, D) * sizeof(double), 256);
}

int dic_gmm_em_iter(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift, double* weights,
                    double* means, double* variances, double* status, double* lower_bounds, int lb_stride, void* workspace, size_t workspace_bytes,
                    dic_stream_t stream) {
    const int rc = gmm_check_points("gmm_em_iter", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && variances && status && lower_bounds && workspace, DIC_ERR_INVALID_ARG, "gmm_em_iter: NULL pointer");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && lb_stride >= 1 && (cov_type == 0 || cov_type == 1) && reg_covar >= 0.0, DIC_ERR_INVALID_ARG,
                "gmm_em_iter: n_runs=%d lb_stride=%d cov_type=%d reg_covar=%g", n_runs, lb_stride, cov_type, reg_covar);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_em_iter: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_gmm_workspace(N, D, K, n_runs), DIC_ERR_WORKSPACE, "gmm_em_iter: workspace %zu < %zu", workspace_bytes,
                dic_gmm_workspace(N, D, K, n_runs));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gm_blocks(N);
    GmArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.w = weights; a.mu = means; a.var = variances; a.status = status; a.part = (double*)workspace;
    const int rl = gm_launch_pass<GM_EM>("gmm_em_iter", a, nblk, n_runs, st);
    if (rl) return rl;
    GmReduce r{};
    r.part = a.part; r.nblk = nblk; r.n = (int)N; r.d = D; r.d0 = D0; r.k = K; r.cov_type = cov_type; r.em = 1; r.lb_stride = lb_stride; r.reg = reg_covar;
    r.w = weights; r.mu = means; r.var = variances; r.status = status; r.lower_bounds = lower_bounds;
    hipLaunchKernelGGL(gm_mstep_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(GM_THREADS), 0, st, r);
    return check_launch("gmm_em_iter");
}

int dic_gmm_estep(const float* X, long ldx, int64_t N, int D, int D0, int K, const double* shift, const double* weights, const double* means,
                  const double* variances, double* lse, double* log_resp, int32_t* labels, double* sum_lse, void* workspace, size_t workspace_bytes,
                  dic_stream_t stream) {
    const int rc = gmm_check_points("gmm_estep", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && variances && workspace, DIC_ERR_INVALID_ARG, "gmm_estep: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_estep: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_gmm_workspace(N, D, K, 1), DIC_ERR_WORKSPACE, "gmm_estep: workspace %zu < %zu", workspace_bytes,
                dic_gmm_workspace(N, D, K, 1));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gm_blocks(N);
    GmArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.w = weights; a.mu = means; a.var = variances; a.part = (double*)workspace;
    a.lse = lse; a.log_resp = log_resp; a.labels = labels;
    const int rl = gm_launch_pass<GM_ESTEP>("gmm_estep", a, nblk, 1, st);
    if (rl) return rl;
    if (sum_lse) hipLaunchKernelGGL(gm_sum_kernel, dim3(1), dim3(kWave), 0, st, (const double*)a.part, nblk, sum_lse);
    return check_launch("gmm_estep");
}

int dic_gmm_mstep_labels(const float* X, long ldx, int64_t N, int D, int D0, int K, int n_runs, int cov_type, double reg_covar, const double* shift,
                         const int32_t* labels, const double* resp, double* weights, double* means, double* variances, void* workspace,
                         size_t workspace_bytes, dic_stream_t stream) {
    const int rc = gmm_check_points("gmm_mstep_labels", X, ldx, N, D, D0, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && weights && means && variances && workspace, DIC_ERR_INVALID_ARG, "gmm_mstep_labels: NULL pointer");
    DIC_REQUIRE((labels != nullptr) != (resp != nullptr), DIC_ERR_INVALID_ARG, "gmm_mstep_labels: exactly one of labels and resp");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && (cov_type == 0 || cov_type == 1) && reg_covar >= 0.0, DIC_ERR_INVALID_ARG,
                "gmm_mstep_labels: n_runs=%d cov_type=%d reg_covar=%g", n_runs, cov_type, reg_covar);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "gmm_mstep_labels: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_gmm_workspace(N, D, K, n_runs), DIC_ERR_WORKSPACE, "gmm_mstep_labels: workspace %zu < %zu", workspace_bytes,
                dic_gmm_workspace(N, D, K, n_runs));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = gm_blocks(N);
    GmArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.d0 = D0; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.shift = shift; a.part = (double*)workspace; a.labels_in = labels; a.resp_in = resp;
    const int rl = labels ? gm_launch_pass<GM_LABELS>("gmm_mstep_labels", a, nblk, n_runs, st) : gm_launch_pass<GM_RESP>("gmm_mstep_labels", a, nblk, n_runs, st);
    if (rl) return rl;
    GmReduce r{};
    r.part = a.part; r.nblk = nblk; r.n = (int)N; r.d = D; r.d0 = D0; r.k = K; r.cov_type = cov_type; r.em = 0; r.lb_stride = 0; r.reg = reg_covar;
    r.w = weights; r.mu = means; r.var = variances;
    hipLaunchKernelGGL(gm_mstep_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(GM_THREADS), 0, st, r);
    return check_launch("gmm_mstep_labels");
}

}  // extern "C"
