// Spectral clustering on the symmetrised k-neighbour graph (sklearn.cluster.SpectralClustering(affinity='nearest_neighbors')).  The definition is stated
// once, in include/dic_hip.h; this file holds to it.  Three f64 kernels on (N, b) row-major blocks, b <= 64, that a block eigen-solver is made of
// (spectral.py); nothing N x N exists and M = D^-1/2 W D^-1/2 is never stored: an entry is formed from its weight byte and the two dd.
//
// (1) spectral_spmm_kernel, the hot path: Y = alpha (M X) + beta X + gamma Z, the fused step of a three-term recurrence.  One wave owns row i.  G = the
//     power of two >= b lanes share one entry of the row (lane = slot * G + column), so a wave takes 64 / G entries at a time -- 32 at b = 2, 4 at the
//     workload's b = 15, 1 at b = 64 -- and reads each neighbour's row of X as one contiguous piece.  Slot s sums the entries s, s + 64 / G, .. of the row in
//     ascending order, four loads in flight, and the slots are added in a fixed xor tree: a row's sum depends on its entries and on b alone.  Every Y[i, c]
//     is stored once; there are no atomics.
// (2) spectral_gram_kernel + spectral_gram_sum_kernel: G = A^T B.  A workgroup owns SG_ROWS consecutive rows -- a function of N, not of the device --
//     stages them through LDS SG_TILE rows at a time, every thread keeps up to 16 of the b^2 sums over the rows in ascending order, and the per-workgroup
//     partials are added in block order by the second kernel (reduce_partials_32x8, as csrc/dic_gmm.hip adds its sums).
// (3) spectral_rotate_kernel: Y = X C, one thread per entry of Y, C in LDS, the sum over p ascending.
#include "dic_common.h"

namespace dic {

constexpr int SP_MAXB = 64;          // the widest block: one lane per column
constexpr int SG_ROWS = 128;         // rows of A and B per workgroup of the gram kernel
constexpr int SG_TILE = 32;          // rows staged in LDS at a time: 2 x 16 KB at b = 64

template <int G>
__global__ __launch_bounds__(256) void spectral_spmm_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const unsigned char* __restrict__ weight, const double* __restrict__ dd, int n, long long nnz, int b,
                                                            const double* __restrict__ X, const double* Z, double alpha, double beta, double gamma, double* Y) {
    constexpr int E = 64 / G;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;          // wave-uniform
    const int lane = threadIdx.x & 63, col = lane & (G - 1), slot = lane / G;
    const bool active = col < b;
    long long p = indptr[r], p1 = indptr[r + 1];
    p = p < 0 ? 0 : (p > nnz ? nnz : p);          // a public input: never read outside the nnz entries
    p1 = p1 < p ? p : (p1 > nnz ? nnz : p1);
    const double di = dd[r];
    double acc = 0.0;
    // an entry outside [0, N) is absent from the row
#define SPECTRAL_TERM(J, W, XV) \
    if ((unsigned)(J) < (unsigned)n) acc = fma((0.5 * (double)(W)) / (di * dd[J]), (XV), acc)
    p += slot;
    for (; p + 3 * E < p1; p += 4 * E) {
        const int j0 = indices[p], j1 = indices[p + E], j2 = indices[p + 2 * E], j3 = indices[p + 3 * E];
        const unsigned w0 = weight[p], w1 = weight[p + E], w2 = weight[p + 2 * E], w3 = weight[p + 3 * E];
        const bool k0 = active && (unsigned)j0 < (unsigned)n, k1 = active && (unsigned)j1 < (unsigned)n;
        const bool k2 = active && (unsigned)j2 < (unsigned)n, k3 = active && (unsigned)j3 < (unsigned)n;
        const double x0 = k0 ? X[(size_t)j0 * b + col] : 0.0, x1 = k1 ? X[(size_t)j1 * b + col] : 0.0;
        const double x2 = k2 ? X[(size_t)j2 * b + col] : 0.0, x3 = k3 ? X[(size_t)j3 * b + col] : 0.0;
        if (active) {
            SPECTRAL_TERM(j0, w0, x0);
            SPECTRAL_TERM(j1, w1, x1);
            SPECTRAL_TERM(j2, w2, x2);
            SPECTRAL_TERM(j3, w3, x3);
        }
    }
    for (; p < p1; p += E) {
        const int j = indices[p];
        const unsigned w = weight[p];
        if (active && (unsigned)j < (unsigned)n) {
            const double x = X[(size_t)j * b + col];
            SPECTRAL_TERM(j, w, x);
        }
    }
#undef SPECTRAL_TERM
#pragma unroll
    for (int w = G; w < 64; w <<= 1) acc += __shfl_xor(acc, w);          // both partners add the same two values: the same bits in every slot
    if (slot == 0 && active) {
        const size_t o = (size_t)r * b + col;
        double y = alpha * acc + beta * X[o];
        if (Z) y += gamma * Z[o];
        Y[o] = y;
    }
}

template <int S>
__global__ __launch_bounds__(256) void spectral_gram_kernel(const double* __restrict__ A, const double* __restrict__ B, long long n, int b,
                                                            double* __restrict__ partial) {
    __shared__ double sa[SG_TILE * SP_MAXB], sb[SG_TILE * SP_MAXB];
    const int tid = threadIdx.x, bb = b * b;
    int pa[S], qb[S];
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int o = tid + 256 * s;
        pa[s] = o < bb ? o / b : 0;          // (a thread without an output sums entry (0, 0) and stores nothing)
        qb[s] = o < bb ? o % b : 0;
        acc[s] = 0.0;
    }
    const long long r0 = (long long)blockIdx.x * SG_ROWS, r1 = r0 + SG_ROWS < n ? r0 + SG_ROWS : n;
    for (long long t0 = r0; t0 < r1; t0 += SG_TILE) {
        const int rows = (int)(r1 - t0 < SG_TILE ? r1 - t0 : SG_TILE);
        __syncthreads();
        for (int e = tid; e < rows * b; e += 256) {          // whole rows of a row-major block: one contiguous piece
            sa[e] = A[(size_t)t0 * b + e];
            sb[e] = B[(size_t)t0 * b + e];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] = fma(sa[r * b + pa[s]], sb[r * b + qb[s]], acc[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int o = tid + 256 * s;
        if (o < bb) partial[(size_t)blockIdx.x * bb + o] = acc[s];
    }
}

__global__ __launch_bounds__(256) void spectral_gram_sum_kernel(const double* __restrict__ partial, int nblk, int bb, double* __restrict__ G) {
    __shared__ double lds[256];
    const int i0 = blockIdx.x * 32;
    const double v = reduce_partials_32x8(partial, nblk, bb, i0, lds);
    if (threadIdx.x < 32 && i0 + (int)threadIdx.x < bb) G[i0 + threadIdx.x] = v;
}

__global__ __launch_bounds__(256) void spectral_rotate_kernel(const double* __restrict__ X, const double* __restrict__ C, long long n, int b,
                                                              double* __restrict__ Y) {
    __shared__ double sc[SP_MAXB * SP_MAXB];
    for (int e = threadIdx.x; e < b * b; e += 256) sc[e] = C[e];
    __syncthreads();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * b) return;
    const long long i = t / b;
    const int col = (int)(t - i * b);
    const double* row = X + (size_t)i * b;
    double acc = 0.0;
    for (int p = 0; p < b; ++p) acc = fma(row[p], sc[p * b + col], acc);
    Y[t] = acc;
}

static int spectral_check_block(const char* what, int64_t N, int b) {
    DIC_REQUIRE(N > 0 && b >= 1, DIC_ERR_INVALID_ARG, "%s: N=%lld b=%d: expected N >= 1, b >= 1", what, (long long)N, b);
    DIC_REQUIRE(b <= SP_MAXB, DIC_ERR_UNSUPPORTED, "%s: b=%d: at most %d columns", what, b, SP_MAXB);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: N=%lld: below 2^30", what, (long long)N);
    return DIC_OK;
}

static bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace dic

using namespace dic;

extern "C" {

int dic_spectral_spmm(const int64_t* indptr, const int32_t* indices, const unsigned char* weight, const double* dd, int64_t N, int64_t nnz, int b,
                      const double* X, const double* Z, double alpha, double beta, double gamma, double* Y, dic_stream_t stream) {
    DIC_REQUIRE(indptr && indices && weight && dd && X && Y, DIC_ERR_INVALID_ARG, "spectral_spmm: NULL pointer");
    int rc = spectral_check_block("spectral_spmm", N, b);
    if (rc) return rc;
    DIC_REQUIRE(nnz >= 0, DIC_ERR_INVALID_ARG, "spectral_spmm: nnz=%lld: expected nnz >= 0", (long long)nnz);
    DIC_REQUIRE(Y != X, DIC_ERR_INVALID_ARG, "spectral_spmm: Y must not be X (other rows read it); Y may be Z");
    DIC_REQUIRE(aligned8(indptr) && aligned8(dd) && aligned8(X) && aligned8(Z) && aligned8(Y) && ((uintptr_t)indices & 3) == 0, DIC_ERR_UNSUPPORTED,
                "spectral_spmm: operands must be aligned to their element size");
    const dim3 grid((unsigned)((N + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define SPECTRAL_LAUNCH(G) \
    hipLaunchKernelGGL(spectral_spmm_kernel<G>, grid, block, 0, st, indptr, indices, weight, dd, (int)N, (long long)nnz, b, X, Z, alpha, beta, gamma, Y)
    if (b <= 2) SPECTRAL_LAUNCH(2);
    else if (b <= 4) SPECTRAL_LAUNCH(4);
    else if (b <= 8) SPECTRAL_LAUNCH(8);
    else if (b <= 16) SPECTRAL_LAUNCH(16);
    else if (b <= 32) SPECTRAL_LAUNCH(32);
    else SPECTRAL_LAUNCH(64);
#undef SPECTRAL_LAUNCH
    return check_launch("spectral_spmm");
}

size_t dic_spectral_gram_workspace(int64_t N, int b) {
    if (N < 1 || N >= (1LL << 30) || b < 1 || b > SP_MAXB) return 0;
    return align_up((size_t)((N + SG_ROWS - 1) / SG_ROWS) * b * b * sizeof(double), 256);
}

int dic_spectral_gram(const double* A, const double* B, int64_t N, int b, double* G, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(A && B && G && workspace, DIC_ERR_INVALID_ARG, "spectral_gram: NULL pointer");
    int rc = spectral_check_block("spectral_gram", N, b);
    if (rc) return rc;
    DIC_REQUIRE(aligned8(A) && aligned8(B) && aligned8(G) && aligned8(workspace), DIC_ERR_UNSUPPORTED, "spectral_gram: operands must be 8-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_spectral_gram_workspace(N, b), DIC_ERR_WORKSPACE, "spectral_gram: workspace of %zu bytes, %zu needed", workspace_bytes,
                dic_spectral_gram_workspace(N, b));
    const int nblk = (int)((N + SG_ROWS - 1) / SG_ROWS), bb = b * b;
    double* partial = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (bb <= 256) hipLaunchKernelGGL(spectral_gram_kernel<1>, dim3(nblk), dim3(256), 0, st, A, B, (long long)N, b, partial);
    else if (bb <= 1024) hipLaunchKernelGGL(spectral_gram_kernel<4>, dim3(nblk), dim3(256), 0, st, A, B, (long long)N, b, partial);
    else hipLaunchKernelGGL(spectral_gram_kernel<16>, dim3(nblk), dim3(256), 0, st, A, B, (long long)N, b, partial);
    hipLaunchKernelGGL(spectral_gram_sum_kernel, dim3((bb + 31) / 32), dim3(256), 0, st, partial, nblk, bb, G);
    return check_launch("spectral_gram");
}

int dic_spectral_rotate(const double* X, const double* C, int64_t N, int b, double* Y, dic_stream_t stream) {
    DIC_REQUIRE(X && C && Y, DIC_ERR_INVALID_ARG, "spectral_rotate: NULL pointer");
    int rc = spectral_check_block("spectral_rotate", N, b);
    if (rc) return rc;
    DIC_REQUIRE(Y != X, DIC_ERR_INVALID_ARG, "spectral_rotate: Y must not be X");
    DIC_REQUIRE(aligned8(X) && aligned8(C) && aligned8(Y), DIC_ERR_UNSUPPORTED, "spectral_rotate: operands must be 8-B aligned");
    hipLaunchKernelGGL(spectral_rotate_kernel, dim3((unsigned)((N * b + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, C, (long long)N, b, Y);
    return check_launch("spectral_rotate");
}

}  // extern "C"
