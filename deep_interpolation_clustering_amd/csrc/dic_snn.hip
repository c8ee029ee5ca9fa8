// Shared-nearest-neighbour clustering on the k-neighbour lists of dic_knn_neighbors (Jarvis & Patrick 1973; Ertoz, Steinbach & Kumar 2003).  The definition is
// stated once, in include/dic_hip.h; this file holds to it.  Nothing N x N exists: both kernels walk the (N, k) int32 lists.
//
// (1) snn_similarity_kernel, the hot path: N k^2 list entries are read (4.95e9 at 75 000 x 257).  One workgroup owns row i.  It copies L(i) into LDS sorted
//     by index -- a bitonic sort of P = the next power of two >= k entries, padded with INT_MAX, 4 KB at k = 1024; an entry outside [0, N) becomes padding,
//     so it is absent from the set.  The waves take the columns c = wave, wave + 4, ..: j = L(i)[c]; the wave reads L(j) with coalesced loads (k contiguous
//     int32), every lane binary-searches its entry in the LDS copy (log2 P probes, a uniform trip count), the wave adds the popcounts of the ballots, and the
//     same sweep notes whether i occurs in L(j).  Lane 0 stores sim[i, c] = the count for a mutual pair, 0 otherwise (and for j = i, and for a j outside
//     [0, N), which is never used as a row index).  Every sim[i, c] is stored exactly once; there are no atomics.
// (2) snn_label_kernel + snn_jump_kernel, one label pass (the form of dic_dbscan_components_pass): one wave owns row i.  A core i takes m = the minimum of
//     labels over itself and its strong core neighbours (sim >= eps, density >= min_samples), hooks labels[labels[i]] and labels[i] to m with atomicMin and
//     sets *changed; labels then jump to their roots.  Labels only decrease and every value is a member of i's component, so a label read that is stale
//     within a launch costs a pass, never correctness; a launch that changes nothing read only settled labels, and then every component is constant at its
//     smallest core index (labels[x] <= x).  A non-core i gets border[i] = the core j with the largest sim >= eps, the smaller j on equal sim -- two keys,
//     so it is computed row-locally by the wave that owns the row, not by an atomic; it does not depend on the labels, so every pass stores the same value.
#include <limits.h>
#include "dic_common.h"

namespace dic {

constexpr int SNN_MAXK = 1024;          // = KN_MAXK of dic_knn.hip: the longest list dic_knn_neighbors produces, and the LDS sort's size

__global__ __launch_bounds__(256) void snn_similarity_kernel(const int32_t* __restrict__ idx, int n, int k, int p2, int32_t* __restrict__ sim) {
    __shared__ int32_t own[SNN_MAXK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    const int32_t* row = idx + (size_t)i * k;
    for (int t = tid; t < p2; t += 256) {
        const int v = t < k ? row[t] : INT_MAX;
        own[t] = (v >= 0 && v < n) ? v : INT_MAX;
    }
    __syncthreads();
    for (int len = 2; len <= p2; len <<= 1)
        for (int s = len >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < p2; t += 256) {
                const int u = t ^ s;
                if (u > t) {
                    const int a = own[t], b = own[u];
                    if ((a > b) == ((t & len) == 0)) {
                        own[t] = b;
                        own[u] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int c = wave; c < k; c += 4) {
        const int j = row[c];
        int count = 0;
        bool mutual = false;
        if (j >= 0 && j < n && j != i) {          // wave-uniform
            const int32_t* other = idx + (size_t)j * k;
            for (int t0 = 0; t0 < k; t0 += 64) {
                const int t = t0 + lane;
                const int v = t < k ? other[t] : -1;
                bool hit = false;
                if (v >= 0 && v < n) {
                    int pos = 0;
                    for (int s = p2 >> 1; s > 0; s >>= 1)
                        if (own[pos + s] <= v) pos += s;
                    hit = own[pos] == v;
                }
                count += __popcll(__ballot(hit));
                mutual = mutual || __ballot(v == i) != 0;
            }
        }
        if (lane == 0) sim[(size_t)i * k + c] = mutual ? count : 0;
    }
}

constexpr int SNN_NONE = -1;

__global__ __launch_bounds__(256) void snn_label_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ sim, int n, int k, int eps,
                                                        const int32_t* __restrict__ density, int min_samples, int32_t* L, int32_t* __restrict__ border,
                                                        int32_t* changed) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;          // wave-uniform
    const int i = (int)r, lane = threadIdx.x & 63;
    const int32_t* ri = idx + (size_t)i * k;
    const int32_t* rs = sim + (size_t)i * k;
    const bool core = density[i] >= min_samples;
    const int li = core ? L[i] : 0;
    int m = INT_MAX;          // core: the smallest label among the strong core neighbours
    int bs = 0, bj = INT_MAX;          // non-core: the best (sim descending, j ascending) strong core neighbour
    for (int c = lane; c < k; c += 64) {
        const int s = rs[c], j = ri[c];
        if (s < eps || j < 0 || j >= n || j == i || density[j] < min_samples) continue;
        if (core) {
            m = min(m, L[j]);
        } else if (s > bs || (s == bs && j < bj)) {
            bs = s;
            bj = j;
        }
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        m = min(m, __shfl_xor(m, w));
        const int os = __shfl_xor(bs, w), oj = __shfl_xor(bj, w);
        if (os > bs || (os == bs && oj < bj)) {
            bs = os;
            bj = oj;
        }
    }
    if (lane != 0) return;
    if (core) {
        border[i] = SNN_NONE;
        if (m < li) {
            atomicMin(L + li, m);
            atomicMin(L + i, m);
            *changed = 1;
        }
    } else {
        border[i] = bs >= eps ? bj : SNN_NONE;
    }
}

// L[i] = its root (L[x] <= x, so every chain ends)
__global__ __launch_bounds__(256) void snn_jump_kernel(int32_t* L, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int l = L[i];
    int ll = L[l];
    while (ll != l) {
        l = ll;
        ll = L[l];
    }
    L[i] = l;
}

static int snn_check_lists(const char* what, const void* idx, const void* sim, int64_t N, int k) {
    DIC_REQUIRE(idx && sim, DIC_ERR_INVALID_ARG, "%s: NULL pointer", what);
    DIC_REQUIRE(N > 0 && k >= 2 && k <= N, DIC_ERR_INVALID_ARG, "%s: N=%lld k=%d: expected 2 <= k <= N", what, (long long)N, k);
    DIC_REQUIRE(k <= SNN_MAXK, DIC_ERR_UNSUPPORTED, "%s: k=%d: at most %d neighbours", what, k, SNN_MAXK);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: N=%lld: below 2^30", what, (long long)N);
    DIC_REQUIRE(((uintptr_t)idx & 3) == 0 && ((uintptr_t)sim & 3) == 0, DIC_ERR_UNSUPPORTED, "%s: operands must be 4-B aligned", what);
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_snn_similarity(const int32_t* idx, int64_t N, int k, int32_t* sim, dic_stream_t stream) {
    int rc = snn_check_lists("snn_similarity", idx, sim, N, k);
    if (rc) return rc;
    int p2 = 2;
    while (p2 < k) p2 <<= 1;
    hipLaunchKernelGGL(snn_similarity_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, idx, (int)N, k, p2, sim);
    return check_launch("snn_similarity");
}

int dic_snn_components_pass(const int32_t* idx, const int32_t* sim, int64_t N, int k, int eps, const int32_t* density, int min_samples, int32_t* labels,
                            int32_t* border, int32_t* changed, dic_stream_t stream) {
    int rc = snn_check_lists("snn_components_pass", idx, sim, N, k);
    if (rc) return rc;
    DIC_REQUIRE(density && labels && border && changed, DIC_ERR_INVALID_ARG, "snn_components_pass: NULL pointer");
    DIC_REQUIRE(eps >= 1 && eps <= k && min_samples >= 0, DIC_ERR_INVALID_ARG, "snn_components_pass: eps=%d min_samples=%d: expected 1 <= eps <= k = %d, "
                "min_samples >= 0", eps, min_samples, k);
    DIC_REQUIRE(((uintptr_t)density & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)border & 3) == 0 && ((uintptr_t)changed & 3) == 0,
                DIC_ERR_UNSUPPORTED, "snn_components_pass: operands must be 4-B aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(snn_label_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, idx, sim, (int)N, k, eps, density, min_samples, labels, border,
                       changed);
    hipLaunchKernelGGL(snn_jump_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, labels, (int)N);
    return check_launch("snn_components_pass");
}

}  // extern "C"
