// Local outlier factor (Breunig, Kriegel, Ng & Sander 2000; sklearn.neighbors.LocalOutlierFactor) on the neighbour lists of dic_knn_neighbors, for up to 64
// values of k from ONE set of lists.  The definition is stated once, in include/dic_hip.h; this file holds to it.  All arithmetic is f64.
//
// Both kernels are the same walk: a (row i, column t) pair adds, over the first ks[t] entries s of row i's list, a value gathered from a table at
// (idx[i, s], t) -- the neighbour's k-distance at ks[t] (lof_lrd_kernel: max'ed with dist[i, s], the reachability distance) or its lrd at ks[t]
// (lof_scores_kernel).  LAYOUT: the tables are (row, t), so the values of one neighbour for all k are one contiguous run of nk doubles.  A row is owned by
// G = the next power of two >= nk adjacent lanes, lane t of the group takes column t: the gather of a step is one coalesced read of nk doubles per row, and
// idx[i, s] / dist[i, s] are one address per group (a broadcast).  With nk = 1 a lane is a row and the reads are plain gathers.
// ORDER: every (i, t) sum runs over s = 0, 1, .., ks[t] - 1 in that order, alone in its lane: it depends on neither the launch geometry nor the other
// entries of ks, so a column of a sweep has the bits of its own call.  The loop is unrolled by LOF_U for the LOADS only (they do not depend on each other:
// LOF_U indices, then LOF_U gathers in flight); the adds stay in order.  No atomics, no LDS, no cross-lane sums.
// The contents of idx are the caller's to check (lof.py does, on the device): here an index is clamped into [0, n), which costs one v_med3 per entry and
// turns a wild read into a wrong value.
#include "dic_common.h"

namespace dic {

constexpr int LOF_MAXK = 64;          // values of k per call: one wave holds a row's columns
constexpr int LOF_U = 8;              // loads in flight per lane

struct LofKs {
    int v[LOF_MAXK];
};

// sum over s < kt of (REACH ? max(tab[idx[s], t], dist[s]) : tab[idx[s], t]), s ascending
template <bool REACH>
__device__ __forceinline__ double lof_row_sum(const int32_t* __restrict__ ri, const double* __restrict__ rd, const double* __restrict__ tab, int n, int nk,
                                              int t, int kt) {
    double sum = 0.0;
    for (int s0 = 0; s0 < kt; s0 += LOF_U) {
        int j[LOF_U];
        double d[LOF_U], v[LOF_U];
#pragma unroll
        for (int u = 0; u < LOF_U; ++u) {
            const int s = s0 + u < kt ? s0 + u : 0;          // (the tail re-reads entry 0 and drops it below)
            j[u] = min(max(ri[s], 0), n - 1);
            d[u] = REACH ? rd[s] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < LOF_U; ++u) v[u] = tab[(size_t)j[u] * nk + t];
#pragma unroll
        for (int u = 0; u < LOF_U; ++u)
            if (s0 + u < kt) sum += REACH ? fmax(v[u], d[u]) : v[u];
    }
    return sum;
}

__global__ __launch_bounds__(256) void lof_lrd_kernel(const double* __restrict__ dist, const int32_t* __restrict__ idx, long long M, int ld,
                                                      const double* __restrict__ kdist, int n, int nk, int lg, LofKs ks, double* __restrict__ lrd) {
    const long long i = (long long)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg);
    const int t = threadIdx.x & ((1 << lg) - 1);
    if (i >= M || t >= nk) return;
    const int kt = ks.v[t];
    const double sum = lof_row_sum<true>(idx + (size_t)i * ld, dist + (size_t)i * ld, kdist, n, nk, t, kt);
    lrd[(size_t)i * nk + t] = 1.0 / (sum / (double)kt + 1e-10);
}

__global__ __launch_bounds__(256) void lof_scores_kernel(const int32_t* __restrict__ idx, long long M, int ld, const double* __restrict__ lrd_fit, int n,
                                                         const double* __restrict__ lrd_rows, int nk, int lg, LofKs ks, double* __restrict__ nof) {
    const long long i = (long long)blockIdx.x * (256 >> lg) + (threadIdx.x >> lg);
    const int t = threadIdx.x & ((1 << lg) - 1);
    if (i >= M || t >= nk) return;
    const int kt = ks.v[t];
    const double sum = lof_row_sum<false>(idx + (size_t)i * ld, nullptr, lrd_fit, n, nk, t, kt);
    nof[(size_t)i * nk + t] = -sum / ((double)kt * lrd_rows[(size_t)i * nk + t]);
}

static int lof_check(const char* what, int64_t M, int ld, int64_t n, const int* ks, int nk, LofKs* out, int* lg) {
    DIC_REQUIRE(nk >= 1, DIC_ERR_INVALID_ARG, "%s: nk=%d: expected 1 <= nk <= %d", what, nk, LOF_MAXK);
    DIC_REQUIRE(nk <= LOF_MAXK, DIC_ERR_UNSUPPORTED, "%s: nk=%d: at most %d values of k per call", what, nk, LOF_MAXK);
    DIC_REQUIRE(M >= 1 && n >= 1 && ld >= 1, DIC_ERR_INVALID_ARG, "%s: M=%lld n=%lld ld=%d: expected positive sizes", what, (long long)M, (long long)n, ld);
    DIC_REQUIRE(M < (1LL << 30) && n < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: M=%lld n=%lld: fewer than 2^30 rows", what, (long long)M, (long long)n);
    for (int t = 0; t < LOF_MAXK; ++t) out->v[t] = 1;
    for (int t = 0; t < nk; ++t) {
        DIC_REQUIRE(ks[t] >= 1 && ks[t] <= ld && (t == 0 || ks[t] > ks[t - 1]), DIC_ERR_INVALID_ARG,
                    "%s: ks[%d]=%d: expected 1 <= ks ascending <= ld = %d", what, t, ks[t], ld);
        out->v[t] = ks[t];
    }
    *lg = 0;
    while ((1 << *lg) < nk) ++*lg;
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_lof_lrd(const double* dist, const int32_t* idx, int64_t M, int ld, const double* kdist, int64_t n, const int* ks, int nk, double* lrd,
                dic_stream_t stream) {
    DIC_REQUIRE(dist && idx && kdist && ks && lrd, DIC_ERR_INVALID_ARG, "lof_lrd: NULL pointer");
    LofKs k;
    int lg = 0;
    int rc = lof_check("lof_lrd", M, ld, n, ks, nk, &k, &lg);
    if (rc) return rc;
    DIC_REQUIRE(((uintptr_t)dist & 7) == 0 && ((uintptr_t)kdist & 7) == 0 && ((uintptr_t)lrd & 7) == 0 && ((uintptr_t)idx & 3) == 0, DIC_ERR_UNSUPPORTED,
                "lof_lrd: operands must be aligned to their element size");
    const int rows = 256 >> lg;
    hipLaunchKernelGGL(lof_lrd_kernel, dim3((unsigned)((M + rows - 1) / rows)), dim3(256), 0, (hipStream_t)stream, dist, idx, (long long)M, ld, kdist, (int)n,
                       nk, lg, k, lrd);
    return check_launch("lof_lrd");
}

int dic_lof_scores(const int32_t* idx, int64_t M, int ld, const double* lrd_fit, int64_t n, const double* lrd_rows, const int* ks, int nk, double* nof,
                   dic_stream_t stream) {
    DIC_REQUIRE(idx && lrd_fit && lrd_rows && ks && nof, DIC_ERR_INVALID_ARG, "lof_scores: NULL pointer");
    LofKs k;
    int lg = 0;
    int rc = lof_check("lof_scores", M, ld, n, ks, nk, &k, &lg);
    if (rc) return rc;
    DIC_REQUIRE(((uintptr_t)lrd_fit & 7) == 0 && ((uintptr_t)lrd_rows & 7) == 0 && ((uintptr_t)nof & 7) == 0 && ((uintptr_t)idx & 3) == 0,
                DIC_ERR_UNSUPPORTED, "lof_scores: operands must be aligned to their element size");
    const int rows = 256 >> lg;
    hipLaunchKernelGGL(lof_scores_kernel, dim3((unsigned)((M + rows - 1) / rows)), dim3(256), 0, (hipStream_t)stream, idx, (long long)M, ld, lrd_fit, (int)n,
                       lrd_rows, nk, lg, k, nof);
    return check_launch("lof_scores");
}

}  // extern "C"
