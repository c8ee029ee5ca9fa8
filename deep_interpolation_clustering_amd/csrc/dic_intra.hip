// The cluster-distance sums of the K sweep, on the matrix cores: two epilogues of the pair-tile loop (dic_pairtile.h: the planes, the loop, the tile sources and
// the error bound of the approximate d^2) over host-built tile lists (cluster_stats.py: PtListTiles).
//
// TOTALS (dic_cluster_intra_totals).  The gap statistic's "inertia" of one clustering (p2_clustering_optK.py:334-351): for every cluster c the sum over its
// ordered point pairs of the Euclidean distance, T[c] = sum_{i, j in c} ||x_i - x_j|| (= np.sum(pairwise_distances(X[a == c]))) -- the ONLY thing the 10
// reference sets of every K need from the point pairs (190 of the 209 pair passes of a K = 2..20 sweep).  dic_cluster_intra_sums (dic_pairdist.hip: the
// difference form on the VALU, every ordered pair) stays for the per-point sums and for widths above 256.  Every point is taken RELATIVE TO ITS CLUSTER'S
// CENTROID: distances do not change, and the cancellation in the norm form d^2 = n_i + n_j - 2 v_i . v_j shrinks to the cluster's own spread.  Measured against
// the f64 sum on the golden clusterings: <= 2e-7 relative on T[c] (the VALU kernel: <= 1e-7); the reference itself works in f32 (tests: rtol 1e-5).  Only the
// tile pairs (I, J >= I) of one cluster are visited, an off-diagonal tile counts twice: sum_c n_c^2 / 2 of the N^2 pairs.  The list (first row of I, first row of
// J, end row of the cluster, cluster) is sorted by cluster and strided over the workgroups.  A tile's 128 accumulators per lane end as sqrt(max(d^2, 0)) summed
// in a fixed order in f32, tiles in f64 per lane; every wave writes ONE f64 partial per cluster it met and intra_finalize_kernel adds the waves' partials in
// order: no atomics, deterministic.
//
// ROW SUMS (dic_cluster_pair_rowsums).  The same distance tiles over ALL point pairs, S[i][c] = sum_{j in c} ||x_i - x_j|| (the silhouette's mean distances,
// internal_eval.py:112-123), every point relative to ONE centre (pairs cross clusters).  A tile is 256 rows of ANY cluster against 256 rows of one cluster c; a
// workgroup walks a CONTIGUOUS range of the list (first row of I, first row of J, end row of J's cluster, output slot), sorted by row block, then cluster, and
// every maximal run of one (row block, cluster) inside a range is an output "slot": the lane's two row sums (its two 32-row blocks, 64 columns each per tile: a
// tile's 64 terms first, then the running sum -- f32 throughout) are written once per slot, the two column halves (wn) side by side; rows_reduce_kernel adds a
// (row block, cluster)'s slots in order.  No atomics, no weights, i == j masked wherever the ranges meet.
//
// Both epilogues mask the padding rows by index and compare a_ij with nothing (PT_SUMS_ONLY).
#include "dic_pairtile.h"

namespace dic {

constexpr int INTRA_WAVES = 8;          // waves of a tile workgroup

struct IntraTotalsArgs {
    PtListArgs p;
    double* partial; int K;             // (workgroups x 8 waves, K), zeroed by the caller
};

struct IntraRowsArgs {
    PtListArgs p;
    float* rows_out; int n_rows;        // rows_out (slots, 2, 256)
};

// A finished tile: lane (i = PtLane::row(I0, mb), hh), register k of block nb -> j = PtLane::col(J0, nb, k).
struct IntraTotals {
    const IntraTotalsArgs& a;
    const PtLane ln;
    double dsum = 0.0;
    int cur_c = -1;
    __device__ __forceinline__ IntraTotals(const IntraTotalsArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {
        if (cur_c < 0) return;
        double v = dsum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
        if (ln.lane == 0) a.partial[((size_t)blockIdx.x * INTRA_WAVES + ln.wm + 4 * ln.wn) * a.K + cur_c] = v;
        dsum = 0.0;
    }
    __device__ __forceinline__ void finish(const pi32x4& e, const pf32x16 (&acc)[4][2]) {
        const int I0 = e[0], J0 = e[1], end = e[2];
        if (e[3] != cur_c) {
            flush();
            cur_c = e[3];
        }
        const bool diag = I0 == J0;
        float t = 0.f;
        if (!diag && I0 + PT_T <= end && J0 + PT_T <= end) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) t += __builtin_amdgcn_sqrtf(fmaxf(acc[nb][mb][k], 0.f));
        } else {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const int gi = I0 + 64 * ln.wm + 32 * mb + ln.l31;          // (global rows: a tile-relative i == j test is loop-invariant, and the compiler keeps all 128 of
                const bool iv = gi < end;                                     //  its lane masks in scalar registers across the whole slab loop)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const int jb = J0 + 128 * ln.wn + 32 * nb + 4 * ln.hh;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int gj = jb + (k & 3) + 8 * (k >> 2);
                        const bool ok = iv && gj < end && gi != gj;
                        t += ok ? __builtin_amdgcn_sqrtf(fmaxf(acc[nb][mb][k], 0.f)) : 0.f;
                    }
                }
            }
        }
        dsum += (double)t * (diag ? 1.0 : 2.0);
    }
};

struct IntraRows {
    const IntraRowsArgs& a;
    const PtLane ln;
    float rs[2] = {0.f, 0.f};
    int cur_c = -1;
    __device__ __forceinline__ IntraRows(const IntraRowsArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {
        if (cur_c < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const float v = rs[mb] + __shfl_xor(rs[mb], 32);
            if (ln.hh == 0) a.rows_out[((size_t)cur_c * 2 + ln.wn) * PT_T + 64 * ln.wm + 32 * mb + ln.l31] = v;
            rs[mb] = 0.f;
        }
    }
    __device__ __forceinline__ void finish(const pi32x4& e, const pf32x16 (&acc)[4][2]) {
        const int I0 = e[0], J0 = e[1], end = e[2];
        if (e[3] != cur_c) {
            flush();
            cur_c = e[3];
        }
        const bool apart = I0 + PT_T <= J0 || J0 + PT_T <= I0;
        if (apart && I0 + PT_T <= a.n_rows && J0 + PT_T <= end) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                float t = 0.f;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) t += __builtin_amdgcn_sqrtf(fmaxf(acc[nb][mb][k], 0.f));
                rs[mb] += t;
            }
        } else {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const int gi = I0 + 64 * ln.wm + 32 * mb + ln.l31;
                const bool iv = gi < a.n_rows;
                float t = 0.f;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const int jb = J0 + 128 * ln.wn + 32 * nb + 4 * ln.hh;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int gj = jb + (k & 3) + 8 * (k >> 2);
                        const bool ok = iv && gj < end && gi != gj;
                        t += ok ? __builtin_amdgcn_sqrtf(fmaxf(acc[nb][mb][k], 0.f)) : 0.f;
                    }
                }
                rs[mb] += t;
            }
        }
    }
};

__global__ __launch_bounds__(512, 1) void intra_totals_kernel(IntraTotalsArgs a) {
    IntraTotals epi(a);
    pt_pair_pass<PtListTiles<false>>(a.p, epi);          // strided over the workgroups
}

__global__ __launch_bounds__(512, 1) void intra_rows_kernel(IntraRowsArgs a) {
    IntraRows epi(a);
    pt_pair_pass<PtListTiles<true>>(a.p, epi);           // contiguous ranges
}

// S[i][c] = the sum of the slots of (row block of i, c), both column halves, in slot order.  grid (row blocks, K).
__global__ __launch_bounds__(PT_T) void rows_reduce_kernel(const float* rows_out, const int* group_start, int n_rows, int K, float* S) {
    const int g = blockIdx.x * K + blockIdx.y, i = blockIdx.x * PT_T + threadIdx.x;
    if (i >= n_rows) return;
    float s = 0.f;
    for (int slot = group_start[g]; slot < group_start[g + 1]; ++slot)
        s += rows_out[((size_t)slot * 2) * PT_T + threadIdx.x] + rows_out[((size_t)slot * 2 + 1) * PT_T + threadIdx.x];
    S[(size_t)i * K + blockIdx.y] = s;
}

// one wave per cluster: lane l adds rows l, l + 64, ... in order, then the 64 lane sums are added by a fixed butterfly
__global__ __launch_bounds__(64) void intra_finalize_kernel(const double* partial, int rows, int K, double* out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int r = lane; r < rows; r += 64) s += partial[(size_t)r * K + c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[c] = s;
}

static size_t intra_partial_bytes(int K) { return (size_t)kNumCU * INTRA_WAVES * K * sizeof(double); }

static int intra_reserve_lds(const char* who) {
    static bool reserved = false;
    return pt_reserve_lds(reserved, {(const void*)intra_totals_kernel, (const void*)intra_rows_kernel}, who);
}

}  // namespace dic

using namespace dic;

extern "C" {

// workspaces: the planes' pt_layout(N), then the slots / the partials

size_t dic_cluster_pair_rowsums_workspace(int64_t N, int n_slots) {
    if (N <= 0 || n_slots < 0) return 0;
    return pt_layout(N).total + (size_t)max(1, n_slots) * 2 * PT_T * sizeof(float);
}

int dic_cluster_pair_rowsums(const float* X, long ldx, const float* centre, int64_t N, int D, int K, const int32_t* tiles, int ntiles, const int32_t* group_start,
                             int n_slots, float* S, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && K > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "cluster_pair_rowsums: N=%lld D=%d K=%d ldx=%ld", (long long)N, D, K, ldx);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "cluster_pair_rowsums: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N < (1 << 30) && K <= 65535, DIC_ERR_UNSUPPORTED, "cluster_pair_rowsums: N=%lld K=%d", (long long)N, K);
    DIC_REQUIRE(X && centre && tiles && group_start && S && workspace && ntiles > 0 && n_slots > 0, DIC_ERR_INVALID_ARG, "cluster_pair_rowsums: NULL pointer / empty list");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tiles & 15) == 0, DIC_ERR_UNSUPPORTED,
                "cluster_pair_rowsums: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_cluster_pair_rowsums_workspace(N, n_slots), DIC_ERR_WORKSPACE, "cluster_pair_rowsums: workspace %zu < %zu", workspace_bytes,
                dic_cluster_pair_rowsums_workspace(N, n_slots));
    int rc = intra_reserve_lds("cluster_pair_rowsums");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    rc = pt_prepare_planes<PT_SUMS_ONLY>(X, ldx, centre, N, D, 0.f, ws, st, "cluster_pair_rowsums");
    if (rc) return rc;
    float* rows_out = (float*)(ws + pt_layout(N).total);
    IntraRowsArgs a{pt_list_args(ws, N, tiles, ntiles), rows_out, (int)N};
    hipLaunchKernelGGL(intra_rows_kernel, dim3(pt_grid(ntiles)), dim3(512), PT_LDS, st, a);
    hipLaunchKernelGGL(rows_reduce_kernel, dim3((unsigned)((N + PT_T - 1) / PT_T), K), dim3(PT_T), 0, st, (const float*)rows_out, group_start, (int)N, K, S);
    return check_launch("cluster_pair_rowsums");
}

size_t dic_cluster_intra_totals_workspace(int64_t N, int K) {
    if (N <= 0 || K <= 0) return 0;
    return pt_layout(N).total + intra_partial_bytes(K);
}

int dic_cluster_intra_totals(const float* X, long ldx, const int32_t* seg, const float* centres, int64_t N, int D, int K, const int32_t* tiles, int ntiles,
                             double* totals, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && K > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "cluster_intra_totals: N=%lld D=%d K=%d ldx=%ld", (long long)N, D, K, ldx);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "cluster_intra_totals: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N < (1 << 30), DIC_ERR_UNSUPPORTED, "cluster_intra_totals: N=%lld", (long long)N);
    DIC_REQUIRE(X && seg && centres && totals && workspace && (tiles || ntiles == 0) && ntiles >= 0, DIC_ERR_INVALID_ARG, "cluster_intra_totals: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centres & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tiles & 15) == 0, DIC_ERR_UNSUPPORTED,
                "cluster_intra_totals: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_cluster_intra_totals_workspace(N, K), DIC_ERR_WORKSPACE, "cluster_intra_totals: workspace %zu < %zu", workspace_bytes,
                dic_cluster_intra_totals_workspace(N, K));
    int rc = intra_reserve_lds("cluster_intra_totals");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    rc = pt_prepare_planes<PT_BY_SEGMENT | PT_SUMS_ONLY>(X, ldx, centres, N, D, 0.f, ws, st, "cluster_intra_totals", seg, K);
    if (rc) return rc;
    double* partial = (double*)(ws + pt_layout(N).total);
    hipError_t e = hipMemsetAsync(partial, 0, intra_partial_bytes(K), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "cluster_intra_totals: memset: %s", hipGetErrorString(e));
    if (ntiles > 0) {
        IntraTotalsArgs a{pt_list_args(ws, N, tiles, ntiles), partial, K};
        hipLaunchKernelGGL(intra_totals_kernel, dim3(pt_grid(ntiles)), dim3(512), PT_LDS, st, a);
    }
    hipLaunchKernelGGL(intra_finalize_kernel, dim3(K), dim3(64), 0, st, partial, kNumCU * INTRA_WAVES, K, totals);
    return check_launch("cluster_intra_totals");
}

}  // extern "C"
