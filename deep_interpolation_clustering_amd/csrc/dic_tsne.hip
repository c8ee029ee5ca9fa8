// Exact t-SNE of the latents (sklearn.manifold.TSNE(method='exact') on neighbour-based affinities).  The definition is stated once, in include/dic_hip.h;
// this file holds to it.  Everything is f64: the early-exaggeration trajectory amplifies a relative gradient error of 1e-7 to O(1) within 50 iterations
// (scripts/tsne_probe.py), so f32 pair terms would make the map a function of the summation order.  No floating-point atomics; the order of every sum is a
// function of N and of the row's entries alone, so two calls give the same bits.
//
// (1) tsne_perplexity_kernel: one wave owns a row of k <= 1024 squared distances and keeps it in registers (R = ceil(k / 64) per lane) across the steps of
//     sklearn's bracket-and-bisect search for the precision beta; the two sums of a step go through wave_sum's xor tree, so every lane takes the same branch.
// (2) tsne_repulsion_kernel, the hot path: all N^2 pairs of the (N, 2) map.  A workgroup owns 256 rows and one of S column ranges; the column points go
//     through LDS 256 at a time; a wave takes 64 of them and every lane 4 rows (row = r0 + 64 r + lane), so one broadcast LDS read serves 4 pairs.  1 / (1 + d2)
//     is an f32 seed (v_rcp_f32 of an argument >= 1) and two f64 Newton steps.  The self pair is masked only in the 64-column pieces that meet the
//     workgroup's own rows (a wave-uniform branch); columns past the range are never iterated.  The four waves' sums are added in wave order through LDS and
//     stored per split; tsne_zrows_kernel / tsne_zsum_kernel add the q sums per row in split order, per 256 rows in a fixed tree, then over the blocks.
// (3) tsne_step_kernel: one wave owns a row of the symmetric CSR of P, a lane an entry (64 entries per wave step, a long row simply takes more steps), each
//     lane's terms in ascending order by fma and the lanes in the xor tree; lanes 0 and 1 then add the split partials of the repulsion in split order, form
//     the gradient and apply sklearn's update to their component.  Y is read from one buffer and written to another: other rows read it.
#include "dic_common.h"

namespace dic {

constexpr int TS_ROWS = 256;           // rows per workgroup of the repulsion kernel: 64 lanes x TS_RPT
constexpr int TS_RPT = 4;              // rows per thread
constexpr int TS_CHUNK = 256;          // column points staged in LDS at a time: 4 waves x 64
constexpr int TS_MAXSPLIT = 64;
constexpr int TS_TARGET_WG = 2048;     // workgroups wanted: 8 per CU of the 256
constexpr int TS_MIN_COLS = 512;       // a split is not shorter than this (unless N is)
constexpr int TS_MAXK = 1024;          // the list limit of dic_knn_neighbors
constexpr int TS_MAX_STEPS = 200;
constexpr double TS_ENTROPY_TOL = 1e-10;

// S and the columns per split: functions of N alone
static int tsne_splits(int64_t N, int* cols_per) {
    const int64_t rb = (N + TS_ROWS - 1) / TS_ROWS;
    int64_t s = (TS_TARGET_WG + rb - 1) / rb;
    const int64_t most = (N + TS_MIN_COLS - 1) / TS_MIN_COLS;
    if (s > most) s = most;
    if (s > TS_MAXSPLIT) s = TS_MAXSPLIT;
    if (s < 1) s = 1;
    const int64_t cp = (int64_t)align_up((size_t)((N + s - 1) / s), TS_CHUNK);
    *cols_per = (int)cp;
    return (int)((N + cp - 1) / cp);
}

template <int R>
__global__ __launch_bounds__(256) void tsne_perplexity_kernel(const double* __restrict__ d2, long long m, int k, double logu, double* __restrict__ beta,
                                                              double* __restrict__ p) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;          // wave-uniform
    const int lane = threadIdx.x & 63;
    double r[R], e[R];
#pragma unroll
    for (int t = 0; t < R; ++t) r[t] = t * 64 + lane < k ? d2[(size_t)row * k + t * 64 + lane] : 0.0;
    double b = 1.0, lo = -INFINITY, hi = INFINITY, s = 1.0;
    for (int step = 0;; ++step) {
        double ss = 0.0, tt = 0.0;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            e[t] = t * 64 + lane < k ? exp(-b * r[t]) : 0.0;
            ss += e[t];
            tt = fma(r[t], e[t], tt);
        }
        s = wave_sum(ss);
        tt = wave_sum(tt);
        const double diff = log(s) + b * tt / s - logu;          // the same bits in every lane
        if (fabs(diff) <= TS_ENTROPY_TOL || step == TS_MAX_STEPS - 1) break;
        if (diff > 0.0) {
            lo = b;
            b = hi == INFINITY ? b * 2.0 : 0.5 * (b + hi);
        } else {
            hi = b;
            b = lo == -INFINITY ? b * 0.5 : 0.5 * (b + lo);
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t)
        if (t * 64 + lane < k) p[(size_t)row * k + t * 64 + lane] = e[t] / s;
    if (lane == 0) beta[row] = b;
}

// 1 / a for a >= 1: v_rcp_f32 (1 ulp of f32) and two Newton steps q <- q + q (1 - a q), each squaring the relative error
__device__ __forceinline__ double tsne_rcp(double a) {
    double q = (double)__builtin_amdgcn_rcpf((float)a);
    q = fma(q, fma(-a, q, 1.0), q);
    return fma(q, fma(-a, q, 1.0), q);
}

template <bool DIAG>
__device__ __forceinline__ void tsne_pairs(const double2* sy, int a, int b, int jbase, int i0, const double (&yx)[TS_RPT], const double (&yy)[TS_RPT],
                                           double (&fx)[TS_RPT], double (&fy)[TS_RPT], double (&z)[TS_RPT]) {
    for (int jj = a; jj < b; ++jj) {
        const double2 yj = sy[jj];          // every lane reads the same point: one broadcast
#pragma unroll
        for (int r = 0; r < TS_RPT; ++r) {
            const double dx = yx[r] - yj.x, dy = yy[r] - yj.y;
            double q = tsne_rcp(fma(dx, dx, fma(dy, dy, 1.0)));
            if (DIAG && jbase + jj == i0 + 64 * r) q = 0.0;          // the pair (i, i)
            z[r] += q;
            const double q2 = q * q;
            fx[r] = fma(q2, dx, fx[r]);
            fy[r] = fma(q2, dy, fy[r]);
        }
    }
}

__global__ __launch_bounds__(256) void tsne_repulsion_kernel(const double* __restrict__ Y, int n, int cols_per, double* __restrict__ part) {
    __shared__ double2 sy[TS_CHUNK];
    __shared__ double red[4][3][TS_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * TS_ROWS, s = blockIdx.y;
    const int j0 = s * cols_per, j1 = j0 + cols_per < n ? j0 + cols_per : n;
    const int i0 = r0 + lane;
    double yx[TS_RPT], yy[TS_RPT], fx[TS_RPT], fy[TS_RPT], z[TS_RPT];
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        const int i = i0 + 64 * r;
        yx[r] = i < n ? Y[2 * (size_t)i] : 0.0;          // (a row past N is computed and not stored)
        yy[r] = i < n ? Y[2 * (size_t)i + 1] : 0.0;
        fx[r] = fy[r] = z[r] = 0.0;
    }
    for (int c = j0; c < j1; c += TS_CHUNK) {
        const int cnt = j1 - c < TS_CHUNK ? j1 - c : TS_CHUNK;
        __syncthreads();
        if (tid < cnt) sy[tid] = reinterpret_cast<const double2*>(Y)[c + tid];
        __syncthreads();
        const int a = w * 64, b = a + 64 < cnt ? a + 64 : cnt;
        if (c + a < r0 + TS_ROWS && c + b > r0) tsne_pairs<true>(sy, a, b, c, i0, yx, yy, fx, fy, z);          // wave-uniform
        else tsne_pairs<false>(sy, a, b, c, i0, yx, yy, fx, fy, z);
    }
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        red[w][0][64 * r + lane] = fx[r];
        red[w][1][64 * r + lane] = fy[r];
        red[w][2][64 * r + lane] = z[r];
    }
    __syncthreads();
    const int i = r0 + tid;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            part[((size_t)s * 3 + c) * n + i] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
    }
}

__global__ __launch_bounds__(256) void tsne_zrows_kernel(const double* __restrict__ part, int n, int S, double* __restrict__ zblk) {
    __shared__ double lds[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double v = 0.0;
    if (i < n)
        for (int s = 0; s < S; ++s) v += part[((size_t)s * 3 + 2) * n + i];
    lds[tid] = v;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m) lds[tid] += lds[tid + m];
        __syncthreads();
    }
    if (tid == 0) zblk[blockIdx.x] = lds[0];
}

__global__ __launch_bounds__(256) void tsne_zsum_kernel(const double* __restrict__ zblk, int nblk, double* __restrict__ Z) {
    __shared__ double lds[256];
    const double v = reduce_partials_32x8(zblk, nblk, 1, 0, lds);
    if (threadIdx.x == 0) Z[0] = v;
}

__global__ __launch_bounds__(256) void tsne_step_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const double* __restrict__ pval,
                                                        int n, long long nnz, const double* __restrict__ Y, const double* __restrict__ part, int S,
                                                        const double* __restrict__ Zp, double exaggeration, double momentum, double lr, double* update,
                                                        double* gains, double* Ynew, double* grad, double* __restrict__ partials) {
    __shared__ double sh[4][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long r = (long long)blockIdx.x * 4 + w;
    double gsq = 0.0, plog = 0.0;
    if (r < n) {          // wave-uniform
        long long p = indptr[r], p1 = indptr[r + 1];
        p = p < 0 ? 0 : (p > nnz ? nnz : p);          // a public input: never read outside the nnz entries
        p1 = p1 < p ? p : (p1 > nnz ? nnz : p1);
        const double yix = Y[2 * r], yiy = Y[2 * r + 1];
        double ax = 0.0, ay = 0.0;
        for (p += lane; p < p1; p += 64) {
            const int j = indices[p];
            const double pv = pval[p];
            if ((unsigned)j < (unsigned)n) {          // an entry outside [0, N) is absent from the row
                const double dx = yix - Y[2 * (size_t)j], dy = yiy - Y[2 * (size_t)j + 1];
                const double d2 = fma(dx, dx, dy * dy);
                const double wq = (exaggeration * pv) / (1.0 + d2);
                ax = fma(wq, dx, ax);
                ay = fma(wq, dy, ay);
                plog = fma(pv, log1p(d2), plog);
            }
        }
        ax = wave_sum(ax);
        ay = wave_sum(ay);
        plog = wave_sum(plog);
        double g2 = 0.0;
        if (lane < 2) {
            double rep = 0.0;
            for (int s = 0; s < S; ++s) rep += part[((size_t)s * 3 + lane) * n + r];
            const double g = 4.0 * ((lane ? ay : ax) - rep / Zp[0]);
            const size_t o = 2 * (size_t)r + lane;
            if (grad) grad[o] = g;
            if (update) {
                double u = update[o], gn = gains[o];
                gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
                gn = gn < 0.01 ? 0.01 : gn;
                u = momentum * u - lr * (g * gn);
                gains[o] = gn;
                update[o] = u;
                Ynew[o] = Y[o] + u;
            }
            g2 = g * g;
        }
        gsq = __shfl(g2, 0) + __shfl(g2, 1);
    }
    if (lane == 0) {
        sh[w][0] = gsq;
        sh[w][1] = plog;
    }
    __syncthreads();
    if (tid < 2) partials[2 * (size_t)blockIdx.x + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

static bool ts_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int tsne_check_n(const char* what, int64_t N) {
    DIC_REQUIRE(N >= 2, DIC_ERR_INVALID_ARG, "%s: N=%lld: expected N >= 2", what, (long long)N);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: N=%lld: below 2^30", what, (long long)N);
    return DIC_OK;
}

// workspace of the repulsion: Z, 7 spare doubles, the per-256-row q sums, then (256-B aligned) the split partials (S, 3, N)
static size_t tsne_part_offset(int64_t N) { return align_up((size_t)(8 + (N + 255) / 256) * sizeof(double), 256); }

}  // namespace dic

using namespace dic;

extern "C" {

int dic_tsne_perplexity(const double* d2, int64_t M, int k, double perplexity, double* beta, double* p, dic_stream_t stream) {
    DIC_REQUIRE(d2 && beta && p, DIC_ERR_INVALID_ARG, "tsne_perplexity: NULL pointer");
    DIC_REQUIRE(M >= 1 && k >= 1, DIC_ERR_INVALID_ARG, "tsne_perplexity: M=%lld k=%d: expected M >= 1, k >= 1", (long long)M, k);
    DIC_REQUIRE(k <= TS_MAXK, DIC_ERR_UNSUPPORTED, "tsne_perplexity: k=%d: at most %d entries per row", k, TS_MAXK);
    DIC_REQUIRE(M < (1LL << 30), DIC_ERR_UNSUPPORTED, "tsne_perplexity: M=%lld: below 2^30", (long long)M);
    DIC_REQUIRE(perplexity > 0.0 && perplexity < 1e300, DIC_ERR_INVALID_ARG, "tsne_perplexity: perplexity=%g: expected a positive finite number", perplexity);
    DIC_REQUIRE(ts_aligned(d2, 8) && ts_aligned(beta, 8) && ts_aligned(p, 8), DIC_ERR_UNSUPPORTED, "tsne_perplexity: operands must be 8-B aligned");
    const dim3 grid((unsigned)((M + 3) / 4)), block(256);
    const double logu = log(perplexity);
    hipStream_t st = (hipStream_t)stream;
#define TSNE_LAUNCH(R) hipLaunchKernelGGL(tsne_perplexity_kernel<R>, grid, block, 0, st, d2, (long long)M, k, logu, beta, p)
    if (k <= 64) TSNE_LAUNCH(1);
    else if (k <= 128) TSNE_LAUNCH(2);
    else if (k <= 256) TSNE_LAUNCH(4);
    else if (k <= 512) TSNE_LAUNCH(8);
    else TSNE_LAUNCH(16);
#undef TSNE_LAUNCH
    return check_launch("tsne_perplexity");
}

int dic_tsne_splits(int64_t N) {
    if (N < 2 || N >= (1LL << 30)) return 0;
    int cols_per;
    return tsne_splits(N, &cols_per);
}

size_t dic_tsne_repulsion_workspace(int64_t N) {
    if (N < 2 || N >= (1LL << 30)) return 0;
    int cols_per;
    const int S = tsne_splits(N, &cols_per);
    return tsne_part_offset(N) + align_up((size_t)S * 3 * N * sizeof(double), 256);
}

int dic_tsne_repulsion(const double* Y, int64_t N, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(Y && workspace, DIC_ERR_INVALID_ARG, "tsne_repulsion: NULL pointer");
    int rc = tsne_check_n("tsne_repulsion", N);
    if (rc) return rc;
    DIC_REQUIRE(ts_aligned(Y, 16) && ts_aligned(workspace, 16), DIC_ERR_UNSUPPORTED, "tsne_repulsion: Y and the workspace must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_tsne_repulsion_workspace(N), DIC_ERR_WORKSPACE, "tsne_repulsion: workspace of %zu bytes, %zu needed", workspace_bytes,
                dic_tsne_repulsion_workspace(N));
    int cols_per;
    const int S = tsne_splits(N, &cols_per);
    const int nblk = (int)((N + TS_ROWS - 1) / TS_ROWS);
    double* Z = (double*)workspace;
    double* zblk = Z + 8;
    double* part = (double*)((char*)workspace + tsne_part_offset(N));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3(nblk, S), dim3(256), 0, st, Y, (int)N, cols_per, part);
    hipLaunchKernelGGL(tsne_zrows_kernel, dim3(nblk), dim3(256), 0, st, part, (int)N, S, zblk);
    hipLaunchKernelGGL(tsne_zsum_kernel, dim3(1), dim3(256), 0, st, zblk, nblk, Z);
    return check_launch("tsne_repulsion");
}

int64_t dic_tsne_step_partials(int64_t N) { return N < 2 || N >= (1LL << 30) ? 0 : (N + 3) / 4; }

int dic_tsne_step(const int64_t* indptr, const int32_t* indices, const double* pval, int64_t N, int64_t nnz, const double* Y, const void* workspace,
                  size_t workspace_bytes, double exaggeration, double momentum, double learning_rate, double* update, double* gains, double* Ynew,
                  double* grad, double* partials, dic_stream_t stream) {
    DIC_REQUIRE(indptr && indices && pval && Y && workspace && partials, DIC_ERR_INVALID_ARG, "tsne_step: NULL pointer");
    int rc = tsne_check_n("tsne_step", N);
    if (rc) return rc;
    DIC_REQUIRE(nnz >= 0, DIC_ERR_INVALID_ARG, "tsne_step: nnz=%lld: expected nnz >= 0", (long long)nnz);
    DIC_REQUIRE((update && gains && Ynew) || (!update && !gains && !Ynew), DIC_ERR_INVALID_ARG,
                "tsne_step: update, gains and Ynew go together (all NULL: the gradient alone)");
    DIC_REQUIRE(update || grad, DIC_ERR_INVALID_ARG, "tsne_step: nothing to do (no update and no grad)");
    DIC_REQUIRE(Ynew != Y, DIC_ERR_INVALID_ARG, "tsne_step: Ynew must not be Y (other rows read it)");
    DIC_REQUIRE(exaggeration > 0.0 && exaggeration < 1e300, DIC_ERR_INVALID_ARG, "tsne_step: exaggeration=%g: expected a positive finite number", exaggeration);
    DIC_REQUIRE(ts_aligned(indptr, 8) && ts_aligned(indices, 4) && ts_aligned(pval, 8) && ts_aligned(Y, 8) && ts_aligned(workspace, 16) &&
                    ts_aligned(update, 8) && ts_aligned(gains, 8) && ts_aligned(Ynew, 8) && ts_aligned(grad, 8) && ts_aligned(partials, 8),
                DIC_ERR_UNSUPPORTED, "tsne_step: operands must be aligned to their element size (the workspace to 16 B)");
    DIC_REQUIRE(workspace_bytes >= dic_tsne_repulsion_workspace(N), DIC_ERR_WORKSPACE, "tsne_step: workspace of %zu bytes, %zu needed", workspace_bytes,
                dic_tsne_repulsion_workspace(N));
    int cols_per;
    const int S = tsne_splits(N, &cols_per);
    const double* Z = (const double*)workspace;
    const double* part = (const double*)((const char*)workspace + tsne_part_offset(N));
    hipLaunchKernelGGL(tsne_step_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, indptr, indices, pval, (int)N, (long long)nnz, Y,
                       part, S, Z, exaggeration, momentum, learning_rate, update, gains, Ynew, grad, partials);
    return check_launch("tsne_step");
}

}  // extern "C"
