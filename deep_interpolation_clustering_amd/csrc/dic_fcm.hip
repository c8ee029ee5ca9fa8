// Fuzzy c-means (Bezdek) with the fuzzifier m > 1, all arithmetic in f64 (fcm.py and the p2 / p4 `--cluster_method fcm` branches).  One iteration is one pass
// over the f32 points and a small reduction; the restarts advance together (grid.y).
// THE DEFINITION.  c = `shift` (D doubles, the column means the Python layer computes).  Every x enters as x' = (double)x - c, one rounded subtraction; the
// centres are kept as v' = v - c.  p = 1 / (m - 1).  Padding columns are zero in both operands and add nothing.
//   d2_ik = sum_{d < D} (x'_id - v'_kd)^2                                        (difference form; here: t = x' - v', fma(t, t, .))
//   dmin_i = min_k d2_ik
//   dmin_i > 0:   r_ik = dmin_i / d2_ik in (0, 1],  t_ik = r_ik when m == 2 exactly, else exp(p log r_ik),  u_ik = t_ik / sum_k t_ik
//   dmin_i == 0:  u_ik = [d2_ik == 0] / #{k : d2_ik == 0}
//       (the min-normalised form cannot overflow; a tiny ratio underflows to 0 harmlessly, however close m is to 1)
//   w_ik = u_ik^2 when m == 2, else exp(m log u_ik), and 0 where u_ik == 0
//   v'_k = sum_i w_ik x'_i / sum_i w_ik;  a component with sum_i w_ik == 0 keeps its centre
//   the sums of a pass, with the memberships from the centres that entered it:  J = sum_ik w_ik d2_ik,  S2 = sum_ik u_ik^2,  SE = sum_ik u_ik log u_ik
//   (0 log 0 = 0)
// THE STOPPING RULE.  A restart is done after iteration t >= 2 if |J_(t-1) - J_t| <= tol J_(t-1) (stopped by tol), or when t == max_iter; the first iteration
// never stops.  The update of the stopping iteration is kept, as the mixtures keep their last M-step (fcm_end_iteration, dic_gmm_common.h).
// THE ORDER OF EVERY SUM IS FIXED, and none depends on a neighbour: sum_d is 4 coordinates per lane in order, then wave_sum's xor tree; sum_k and min_k are
// the xor tree over the 64 lanes (lane k holds component k, the others +inf, 0 after the division); sums over rows are sequential over a workgroup's rows, in
// row order, by the one thread that owns them, and then sequential over the workgroups in block order (gmm_sum_blocks).  No floating-point atomics.  The rows a
// workgroup takes depend on N alone, and a restart is a grid row of its own: its bits do not depend on the restarts beside it.
//
// A PASS (fc_pass_kernel) is at most 256 workgroups of 4 waves per restart.  A workgroup holds its restart's v' in LDS (8 K D bytes: 64 KiB at K = 32,
// D = 256) and takes its rows 16 at a time.  First phase: a wave takes 4 rows at once -- a lane holds 4 coordinates of each, so one read of v' from LDS serves
// 4 rows -- and leaves w (16, K) and the three row sums in LDS.  Second phase, as gm_pass_kernel's: thread (d, g) owns the components k = g, g + G, ..
// (G = 256 / D groups) of column d, re-reads x_d of the 16 rows (cache hits) and adds w x' into registers; there is no second moment.  At the end the
// workgroup stores its partial sums: K + K D + 3 doubles.  fc_reduce_kernel, one workgroup per (component, restart), adds the partials in block order and
// writes the centre; the workgroup of component 0 appends J, counts the iteration and decides whether the restart is done.  A done restart is skipped by both
// kernels: status[6], which the pass writes and the reduction reads, tells the reduction whether its pass ran -- the done flag itself is rewritten by the
// reduction's component-0 workgroup while the others may not have started.
#include "dic_gmm_common.h"

namespace dic {

constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / kWave;
constexpr int FC_RPW = 4;                         // rows a wave takes at once
constexpr int FC_TILE = FC_WAVES * FC_RPW;        // rows of a tile
constexpr int FC_MAX_BLOCKS = kNumCU;
constexpr int FC_SLOTS = DIC_MAX_CLUSTERS;        // components a thread of the second phase can own
constexpr int FC_BATCH = 32;                      // loads in flight of gmm_sum_blocks
// status words (f64): 0 done, 1 iterations, 2 stopped by tol, 3 last J, 4 tol, 5 max_iter, 6 (internal) the last pass ran

struct FcArgs {
    const float* X; long ldx;
    int n, d, k, rpb;                             // rpb: rows per workgroup
    int m2;                                       // m == 2 exactly
    double m, p;                                  // p = 1 / (m - 1)
    const double* shift;
    const double* centers;                        // (n_runs, K, D)
    double* status;                               // (n_runs, DIC_GMM_STATUS_WORDS) or NULL
    double* part;                                 // (n_runs, gridDim.x, P) workgroup partials
    double* u; int32_t* labels; double* d2;       // outputs of dic_fcm_memberships, each optional
};

__host__ __device__ inline size_t fc_part_words(int K, int D) { return (size_t)K * (1 + (size_t)D) + 3; }          // sum w, sum w x', then J, S2, SE
static int fc_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)FC_MAX_BLOCKS, (N + FC_TILE - 1) / FC_TILE)); }
static size_t fc_lds_bytes(int K, int D) { return ((size_t)K * D + (size_t)FC_TILE * K + 3 * FC_TILE) * sizeof(double); }

__device__ __forceinline__ double fc_wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ double fc_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// The memberships of up to FC_RPW rows (row0 .., nvalid of them) by one wave: w into s_w, the rows' J, S2, SE into s_rows, and the optional outputs.
__device__ __forceinline__ void fc_wave_rows(const FcArgs& a, const double* s_v, double* s_w, double* s_rows, long long row0, int nvalid, int trow,
                                             const double (&c)[4]) {
#pragma clang fp contract(off)
    const int lane = lane_id(), col = 4 * lane, D = a.d, K = a.k;
    const bool in = lane < K;
    double x[FC_RPW][4];
#pragma unroll
    for (int u = 0; u < FC_RPW; ++u) {
        const long long row = row0 + min(u, nvalid - 1);          // (a row past the end repeats the last valid one; its result is dropped)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < D) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * a.ldx + col);
        x[u][0] = (double)v.x - c[0]; x[u][1] = (double)v.y - c[1]; x[u][2] = (double)v.z - c[2]; x[u][3] = (double)v.w - c[3];
    }
    double dk[FC_RPW];
#pragma unroll
    for (int u = 0; u < FC_RPW; ++u) dk[u] = __builtin_inf();
    for (int k = 0; k < K; ++k) {
        double s[FC_RPW];
#pragma unroll
        for (int u = 0; u < FC_RPW; ++u) s[u] = 0.0;
        if (col < D) {
            const double* pv = s_v + (size_t)k * D + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double vj = pv[j];
#pragma unroll
                for (int u = 0; u < FC_RPW; ++u) {
                    const double t = x[u][j] - vj;
                    s[u] = fma(t, t, s[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FC_RPW; ++u) {
            const double sk = wave_sum(s[u]);
            if (lane == k) dk[u] = sk;
        }
    }
#pragma unroll
    for (int u = 0; u < FC_RPW; ++u) {
        const double dmin = fc_wave_min(dk[u]);          // (lanes K .. 63 hold +inf)
        double mu;
        if (dmin > 0.0) {          // (wave-uniform)
            const double r = dmin / dk[u];
            const double t = in ? (a.m2 ? r : exp(a.p * log(r))) : 0.0;
            const double s = wave_sum(t);
            mu = t / s;
        } else {
            const bool zero = in && dk[u] == 0.0;
            const unsigned long long zeros = __ballot(zero);
            mu = zero ? 1.0 / (double)__popcll(zeros) : 0.0;
        }
        const double lg = mu > 0.0 ? log(mu) : 0.0;
        const double w = a.m2 ? mu * mu : (mu > 0.0 ? exp(a.m * lg) : 0.0);
        const double rj = wave_sum(in ? w * dk[u] : 0.0);
        const double r2 = wave_sum(mu * mu);
        const double re = wave_sum(mu * lg);
        const double mx = fc_wave_max(in ? mu : -__builtin_inf());
        const unsigned long long at_max = __ballot(in && mu == mx);
        if (u < nvalid) {          // (wave-uniform)
            const long long row = row0 + u;
            if (in) {
                s_w[(trow + u) * K + lane] = w;
                if (a.u) a.u[(size_t)row * K + lane] = mu;
                if (a.d2) a.d2[(size_t)row * K + lane] = dk[u];
            }
            if (lane == 0) {
                s_rows[trow + u] = rj;
                s_rows[FC_TILE + trow + u] = r2;
                s_rows[2 * FC_TILE + trow + u] = re;
                if (a.labels) a.labels[row] = at_max ? (int)__builtin_ctzll(at_max) : 0;          // the first maximum
            }
        }
    }
}

// ACCUM: an iteration (status, the second phase, K + K D + 3 partial words); else the memberships of one centre set (the outputs, 3 partial words).
template <bool ACCUM>
__global__ __launch_bounds__(FC_THREADS) void fc_pass_kernel(FcArgs a) {
    extern __shared__ double fc_lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int run = blockIdx.y, K = a.k, D = a.d, n = a.n;
    if (ACCUM) {
        const bool done = a.status[(size_t)run * DIC_GMM_STATUS_WORDS] != 0.0;          // (written by the previous reduction, never in this launch)
        if (blockIdx.x == 0 && tid == 0) a.status[(size_t)run * DIC_GMM_STATUS_WORDS + 6] = done ? 0.0 : 1.0;
        if (done) return;
    }
    double* s_v = fc_lds;
    double* s_w = s_v + (size_t)K * D;
    double* s_rows = s_w + (size_t)FC_TILE * K;
    {
        const double* v = a.centers + (size_t)run * K * D;
        for (int i = tid; i < K * D; i += FC_THREADS) s_v[i] = v[i];
        __syncthreads();
    }
    // first phase: this lane's 4 shifts.  Second phase: this thread's column d and its components g, g + G, ..
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
    if (4 * lane < D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c4[j] = a.shift[4 * lane + j];
    }
    const int G = FC_THREADS / D, g = tid / D, d = tid - g * D;
    const bool owner = ACCUM && g < G;
    const int nslots = ACCUM ? (K + G - 1) / G : 0;          // the same in every thread: a slot past K - 1 repeats component K - 1 and is never stored
    const double cd = ACCUM ? a.shift[d] : 0.0;
    double sx[FC_SLOTS];
#pragma unroll
    for (int j = 0; j < FC_SLOTS; ++j) sx[j] = 0.0;
    double pn = 0.0, ps = 0.0;

    const long long r0 = (long long)blockIdx.x * a.rpb;
    const long long r1 = min((long long)n, r0 + a.rpb);
    for (long long t0 = r0; t0 < r1; t0 += FC_TILE) {
        const int nt = (int)min((long long)FC_TILE, r1 - t0);
        const int nvalid = min(FC_RPW, nt - FC_RPW * w);
        if (nvalid > 0) fc_wave_rows(a, s_v, s_w, s_rows, t0 + FC_RPW * w, nvalid, FC_RPW * w, c4);
        __syncthreads();
        if (ACCUM) {
            for (int i = 0; i < nt; ++i) {          // (no thread-dependent branch: threads that own nothing add into slots they never store)
#pragma clang fp contract(off)
                const double xv = (double)a.X[(size_t)(t0 + i) * a.ldx + d] - cd;
                const double* ww = s_w + i * K;
#pragma unroll
                for (int j = 0; j < FC_SLOTS; ++j) {
                    if (j < nslots) {
                        const double t = ww[min(g + j * G, K - 1)] * xv;
                        sx[j] = sx[j] + t;
                    }
                }
            }
            if (tid < K)
                for (int i = 0; i < nt; ++i) pn += s_w[i * K + tid];
        }
        if (tid >= kWave && tid < kWave + 3)          // (the second wave: J, S2 and SE of the tile's rows, in row order)
            for (int i = 0; i < nt; ++i) ps += s_rows[(tid - kWave) * FC_TILE + i];
        __syncthreads();          // (the tile is rewritten)
    }
    double* part = a.part + ((size_t)run * gridDim.x + blockIdx.x) * (ACCUM ? fc_part_words(K, D) : 3);
    if (ACCUM) {
        if (owner) {
#pragma unroll
            for (int j = 0; j < FC_SLOTS; ++j) {
                if (j < nslots && g + j * G < K) part[K + (size_t)(g + j * G) * D + d] = sx[j];
            }
        }
        if (tid < K) part[tid] = pn;
    }
    if (tid >= kWave && tid < kWave + 3) part[(ACCUM ? K + (size_t)K * D : 0) + (tid - kWave)] = ps;
}

struct FcReduce {
    const double* part; int nblk;
    int d, k, obj_stride;
    double* centers; double* status; double* objectives;
};

// one workgroup per (component, restart): the partials of the pass in block order, then the centre
__global__ __launch_bounds__(FC_THREADS) void fc_reduce_kernel(FcReduce a) {
#pragma clang fp contract(off)
    __shared__ double s_nk;
    __shared__ double s_j;
    const int tid = threadIdx.x, k = blockIdx.x, run = blockIdx.y, K = a.k, D = a.d;
    double* st = a.status + (size_t)run * DIC_GMM_STATUS_WORDS;
    if (st[6] == 0.0) return;          // (the pass skipped this restart: it was done)
    const size_t P = fc_part_words(K, D);
    const double* part = a.part + (size_t)run * a.nblk * P;
    if (tid == 0) s_nk = gmm_sum_blocks<FC_BATCH>(part + k, P, a.nblk);
    if (k == 0 && tid == kWave) s_j = gmm_sum_blocks<FC_BATCH>(part + K + (size_t)K * D, P, a.nblk);          // (the second wave, beside the first's sum w)
    __syncthreads();
    const double nk = s_nk;
    if (tid < D && nk != 0.0) {          // (a component without weight keeps its centre)
        const size_t o = (size_t)k * D + tid;
        const double sx = gmm_sum_blocks<FC_BATCH>(part + K + o, P, a.nblk);
        a.centers[(size_t)run * K * D + o] = sx / nk;
    }
    if (k == 0 && tid == 0) fcm_end_iteration(st, s_j, a.objectives, a.obj_stride, run);
}

// J, S2, SE of dic_fcm_memberships: the three partial words of every workgroup, in block order
__global__ void fc_sums_kernel(const double* part, int nblk, double* out) {
    if (blockIdx.x == 0 && threadIdx.x < 3) out[threadIdx.x] = gmm_sum_blocks<FC_BATCH>(part + threadIdx.x, 3, nblk);
}

template <bool ACCUM>
static int fc_launch_pass(const char* what, const FcArgs& a, int nblk, int n_runs, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        const int most = (int)fc_lds_bytes(DIC_MAX_CLUSTERS, 4 * kWave);
        hipError_t e = hipFuncSetAttribute((const void*)fc_pass_kernel<ACCUM>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", what, most, hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(fc_pass_kernel<ACCUM>, dim3((unsigned)nblk, (unsigned)n_runs), dim3(FC_THREADS), fc_lds_bytes(a.k, a.d), st, a);
    return DIC_OK;
}

static FcArgs fc_args(const float* X, long ldx, int64_t N, int D, int K, double m, const double* shift, const double* centers, void* workspace, int nblk) {
    FcArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D; a.k = K; a.rpb = (int)((N + nblk - 1) / nblk);
    a.m2 = m == 2.0; a.m = m; a.p = 1.0 / (m - 1.0);
    a.shift = shift; a.centers = centers; a.part = (double*)workspace;
    return a;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_fcm_workspace(int64_t N, int D, int K, int n_runs) {
    if (N < 2 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave || K < 1 || K > DIC_MAX_CLUSTERS || n_runs < 1) return 0;
    return align_up((size_t)n_runs * fc_blocks(N) * fc_part_words(K, D) * sizeof(double), 256);
}

int dic_fcm_iter(const float* X, long ldx, int64_t N, int D, int K, int n_runs, double m, const double* shift, double* centers, double* status,
                 double* objectives, int obj_stride, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(m > 1.0 && m < __builtin_inf(), DIC_ERR_INVALID_ARG, "fcm_iter: m=%g: the fuzzifier must be finite and greater than 1", m);
    const int rc = gmm_check_points("fcm_iter", X, ldx, N, D, D, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && centers && status && objectives && workspace, DIC_ERR_INVALID_ARG, "fcm_iter: NULL pointer");
    DIC_REQUIRE(n_runs >= 1 && n_runs <= 65535 && obj_stride >= 1, DIC_ERR_INVALID_ARG, "fcm_iter: n_runs=%d obj_stride=%d", n_runs, obj_stride);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "fcm_iter: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_fcm_workspace(N, D, K, n_runs), DIC_ERR_WORKSPACE, "fcm_iter: workspace %zu < %zu", workspace_bytes,
                dic_fcm_workspace(N, D, K, n_runs));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = fc_blocks(N);
    FcArgs a = fc_args(X, ldx, N, D, K, m, shift, centers, workspace, nblk);
    a.status = status;
    const int rl = fc_launch_pass<true>("fcm_iter", a, nblk, n_runs, st);
    if (rl) return rl;
    FcReduce r{};
    r.part = a.part; r.nblk = nblk; r.d = D; r.k = K; r.obj_stride = obj_stride; r.centers = centers; r.status = status; r.objectives = objectives;
    hipLaunchKernelGGL(fc_reduce_kernel, dim3((unsigned)K, (unsigned)n_runs), dim3(FC_THREADS), 0, st, r);
    return check_launch("fcm_iter");
}

int dic_fcm_memberships(const float* X, long ldx, int64_t N, int D, int K, double m, const double* shift, const double* centers, double* u, int32_t* labels,
                        double* d2, double* sums, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(m > 1.0 && m < __builtin_inf(), DIC_ERR_INVALID_ARG, "fcm_memberships: m=%g: the fuzzifier must be finite and greater than 1", m);
    const int rc = gmm_check_points("fcm_memberships", X, ldx, N, D, D, K);
    if (rc) return rc;
    DIC_REQUIRE(shift && centers && workspace, DIC_ERR_INVALID_ARG, "fcm_memberships: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED, "fcm_memberships: the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_fcm_workspace(N, D, K, 1), DIC_ERR_WORKSPACE, "fcm_memberships: workspace %zu < %zu", workspace_bytes,
                dic_fcm_workspace(N, D, K, 1));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = fc_blocks(N);
    FcArgs a = fc_args(X, ldx, N, D, K, m, shift, centers, workspace, nblk);
    a.u = u; a.labels = labels; a.d2 = d2;
    const int rl = fc_launch_pass<false>("fcm_memberships", a, nblk, 1, st);
    if (rl) return rl;
    if (sums) hipLaunchKernelGGL(fc_sums_kernel, dim3(1), dim3(kWave), 0, st, (const double*)a.part, nblk, sums);
    return check_launch("fcm_memberships");
}

}  // extern "C"
