// Density-peaks clustering (Rodriguez and Laio, Science 2014; density_peaks.py; the definition stands in include/dic_hip.h): the masked nearest-neighbour
// join -- for every point the nearest among the DENSER points -- and the halo's border densities, without the N x N matrix.  The planes, the tile loop and the
// error bound B0 = 2^-12 (n_i + nmax_J) of its approximate d^2 (a_ij) are dic_pairtile.h's, the exact distance is dic_exactd2.h's; this file is three
// epilogues, the exact stage and the bookkeeping.  The densities themselves need no kernel of their own (dic_dbscan_counts / dic_knn_kth_distance).
//
// SORTED PLANES.  The host gathers X into density order: row r is the point of rank r (rank 0 the densest).  "j is denser than i" is then col < row, an index
// compare in registers: no per-column loads, and no mask for the padding columns either (col < row < N).  Tiles with J0 > I0 hold no eligible pair and their
// epilogue returns at once; walking only the lower-triangular tiles would halve the pass but needs another tile list in the shared header (the follow-up).
//
// BOUND PASS.  A lane forms bq = fl(fl(B0) (1 + 2^-8)) and y = max(fl(a + bq), 0) for every eligible pair; U_i = min_j y_ij, in registers while the row block
// stays, flushed with an integer atomicMin on the bits of the non-negative f32 (exact, order-free).
// CANDIDATE PASS.  z = fl(a - bq); every eligible (i, j) with z_ij <= U_i is appended to the caller's list (DBSCAN's band-list protocol: a global cursor, a
// capacity, the count read back).
// WHY THE MINIMISER IS ON THE LIST.  |a - d^2| < B0 (the header's bound).  Roundings: fl(B0) is one add (the factor 2^-12 is exact), the inflation one
// product, a +- bq one add each, of |a +- bq| <= 2 (n_i + n_j) + 2 B0 < 2^13.1 B0: together < (2^-23 + 2^-10.9) B0 < 2^-10 B0 per side, and the inflation
// alone is 2^-8 B0.  So y >= a + B0 > d^2 (clamping at 0 keeps it, d^2 >= 0) and z <= a - B0 < d^2 for every pair.  Let j* attain the row's exact minimum
// (any of them, when several pairs tie): z_ij* < d^2_ij* <= d^2_ij < y_ij for every eligible j, hence z_ij* <= U_i.  All pairs that tie at the exact minimum are
// on the list, so the tie rule (the denser one) is decided by the exact stage alone.
//
// EXACT STAGE.  One wave per entry: exact_d2, written into the entry, and a 64-bit atomicMin on the bits of the non-negative f64 into the row's minimum; a
// second kernel takes the atomicMin of the column (= rank_j) over the entries that attain it; delta = the f64 root.  The densest point's delta is the maximum
// of N exact distances (64-bit atomicMax of the bits).  The approximate products never supply a value and never decide a tie.
//
// HALO PASS (dic_dpeaks_border).  In the ORIGINAL row order, on the workspace dic_dbscan_counts filled and with the band list and exact masks it left: the
// epilogue, modelled on DbLabel, stages the columns' labels and rho per wave, takes the certain pairs y <= tl with DBSCAN's own tl (so the certain and band
// classes are those of the counting pass) and keeps per row the largest rho_j over the neighbours j of another label; the flush adds rho_i and does an
// integer atomicMax into border2[label_i].  One thread per band entry adds the band pairs' share.
//
// No workgroup waits for another inside a kernel; every atomic is an integer atomic: two calls give the same bits.
#include <type_traits>
#include "dic_pairtile.h"
#include "dic_exactd2.h"

namespace dic {

typedef pi32x4 dpi32x4;

constexpr unsigned DP_U_INIT = 0x7f7f7f7fu;            // the bytes memset leaves: 3.39e38 as f32, above every y
constexpr float DP_INFLATE = 1.f + 0x1p-8f;
constexpr float DP_MAX_THRESHOLD = 0x1p100f;           // dic_dbscan.hip's DB_MAX_THRESHOLD

// pt_layout(N) + U (N + 256) u32 + row minimum (N) u64 + candidates per row (N) i32.  Scratch words (pt_layout's count block): cursor u64, max d^2 of the
// densest point u64, longest row i32.
struct DpLayout { size_t u, rowmin, rowcnt, total; };

inline DpLayout dp_layout(int64_t N) {
    DpLayout o;
    o.u = pt_layout(N).total;
    o.rowmin = o.u + align_up((size_t)(N + PT_T) * sizeof(unsigned), 256);
    o.rowcnt = o.rowmin + align_up((size_t)N * sizeof(unsigned long long), 256);
    o.total = o.rowcnt + align_up((size_t)N * sizeof(int32_t), 256);
    return o;
}

struct DpTileArgs {
    PtPairArgs p;
    unsigned* U;
    dpi32x4* cand; long long cap; unsigned long long* cursor;
    // halo
    float tl; const int32_t* labels; const int32_t* rho; int n_clusters; int32_t* border2;
};

// Bound epilogue: U_i = min over col < row of y.
struct DpBound {
    const DpTileArgs& a;
    const PtLane ln;
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    float u[2];

    __device__ __forceinline__ DpBound(const DpTileArgs& args) : a(args), ln() { u[0] = u[1] = __uint_as_float(DP_U_INIT); }
    __device__ __forceinline__ void flush() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(cur_i, mb);
            const float m = fminf(u[mb], __shfl_xor(u[mb], 32));
            if (ln.hh == 0 && gi < a.p.n && __float_as_uint(m) < DP_U_INIT) atomicMin(a.U + gi, __float_as_uint(m));
            u[mb] = __uint_as_float(DP_U_INIT);
        }
    }
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i) {
            flush();
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) ni[mb] = a.p.nrm[ln.row(I0, mb)];          // (padding rows hold 0)
        }
        if (J0 > I0) return;
        const float bm = a.p.bmax[J0 / PT_T];
        auto rows = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
            const int gi = ln.row(I0, mb);
            const float bq = ((ni[mb] + bm) * 0x1p-12f) * DP_INFLATE;
            float m = u[mb];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float y = fmaxf(acc[nb][mb][k] + bq, 0.f);
                    m = ln.col(J0, nb, k) < gi ? fminf(m, y) : m;
                }
            u[mb] = m;
        };
        rows(std::integral_constant<int, 0>{});
        rows(std::integral_constant<int, 1>{});
    }
};

// Candidate epilogue: every (row, col < row) with z <= U_row goes to the list.
struct DpCand {
    const DpTileArgs& a;
    const PtLane ln;
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    float ui[2] = {0.f, 0.f};

    __device__ __forceinline__ DpCand(const DpTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i) {
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                ni[mb] = a.p.nrm[ln.row(I0, mb)];          // (padding rows hold 0)
                ui[mb] = __uint_as_float(a.U[ln.row(I0, mb)]);          // (U has the padding rows too)
            }
        }
        if (J0 > I0) return;
        const float bm = a.p.bmax[J0 / PT_T];
        auto rows = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
            const int gi = ln.row(I0, mb);
            const bool iv = gi < a.p.n;          // (a padding row must not reach the list)
            const float bq = ((ni[mb] + bm) * 0x1p-12f) * DP_INFLATE;
            unsigned bits[2] = {0u, 0u};
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float z = acc[nb][mb][k] - bq;
                    const bool c = iv & (ln.col(J0, nb, k) < gi) & (z <= ui[mb]);
                    bits[nb >> 1] |= c ? (1u << (16 * (nb & 1) + k)) : 0u;
                }
            const int nbits = __builtin_popcount(bits[0]) + __builtin_popcount(bits[1]);
            if (nbits) {
                unsigned long long base = atomicAdd(a.cursor, (unsigned long long)nbits);
                for (int h = 0; h < 2; ++h) {
                    unsigned b = bits[h];
                    while (b) {
                        const int p = __builtin_ctz(b);
                        b &= b - 1;
                        if (base < (unsigned long long)a.cap) {
                            dpi32x4 ent;
                            ent[0] = gi; ent[1] = ln.col(J0, 2 * h + (p >> 4), p & 15); ent[2] = 0; ent[3] = 0;
                            a.cand[base] = ent;
                        }
                        ++base;
                    }
                }
            }
        };
        rows(std::integral_constant<int, 0>{});
        rows(std::integral_constant<int, 1>{});
    }
};

// Halo epilogue: per row the largest rho_j over the certain neighbours j of another label; flush: atomicMax(border2[label_i], rho_i + that).
struct DpBorder {
    const DpTileArgs& a;
    const PtLane ln;
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    int li[2] = {-1, -1};
    int mx[2] = {-1, -1};

    __device__ __forceinline__ DpBorder(const DpTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(cur_i, mb);
            const int m = max(mx[mb], __shfl_xor(mx[mb], 32));
            if (ln.hh == 0 && gi < a.p.n && m >= 0 && (unsigned)li[mb] < (unsigned)a.n_clusters) atomicMax(a.border2 + li[mb], m + a.rho[gi]);
            mx[mb] = -1;
        }
    }
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i) {
            flush();
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const int gi = ln.row(I0, mb);
                ni[mb] = a.p.nrm[gi];          // (padding rows hold 0)
                li[mb] = gi < a.p.n ? a.labels[gi] : -1;
            }
        }
        const float bm = a.p.bmax[J0 / PT_T];
        // labels and rho of the 128 points j of this wave's half of the tile: lane l holds j = jw + l and jw + 64 + l (a padding point j presents
        // PT_PAD_NORM: its y lies above tl, its staged values are never used)
        const int jw = J0 + 128 * ln.wn;
        int lc[2], rc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = jw + 64 * h + ln.lane;
            lc[h] = j < a.p.n ? a.labels[j] : -1;
            rc[h] = j < a.p.n ? a.rho[j] : -1;
        }
        const float tl = a.tl;
        float b0[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) b0[mb] = (ni[mb] + bm) * 0x1p-12f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                // (two v_readlane and a select per value, or scheduling barriers between the groups of k, cost MORE registers here: 164 and 42 spilled VGPRs
                // against 16 this way; DbLabel, with one staged value, spills 10)
                const int jl = 32 * (nb & 1) + 4 * ln.hh + (k & 3) + 8 * (k >> 2);
                const int lj = __shfl(lc[nb >> 1], jl);
                const int rj = __shfl(rc[nb >> 1], jl);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const float y = acc[nb][mb][k] + b0[mb];
                    mx[mb] = max(mx[mb], ((y <= tl) & (lj != li[mb])) ? rj : -1);
                }
            }
    }
};

__global__ __launch_bounds__(512, 1) void dp_bound_kernel(DpTileArgs a) {
    DpBound epi(a);
    pt_pair_pass(a.p, epi);
}

__global__ __launch_bounds__(512, 1) void dp_cand_kernel(DpTileArgs a) {
    DpCand epi(a);
    pt_pair_pass(a.p, epi);
}

__global__ __launch_bounds__(512, 1) void dp_border_kernel(DpTileArgs a) {
    DpBorder epi(a);
    pt_pair_pass(a.p, epi);
}

// One wave per entry: the exact d^2 into the entry, its bits into the row's minimum, the row's entry count.
__global__ __launch_bounds__(256) void dp_exact_kernel(const float* X, long ldx, int d, dpi32x4* cand, long long ncand, unsigned long long* rowmin,
                                                       int32_t* rowcnt) {
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= ncand) return;
    dpi32x4 ent = cand[idx];
    const double s = exact_d2(exact_d2_load(X, ldx, (size_t)ent[0], d), exact_d2_load(X, ldx, (size_t)ent[1], d));
    if (lane_id() == 0) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(s);          // (s >= 0: the bits order as the values)
        ent[2] = (int)(unsigned)b; ent[3] = (int)(unsigned)(b >> 32);
        cand[idx] = ent;
        atomicMin(rowmin + ent[0], b);
        atomicAdd(rowcnt + ent[0], 1);
    }
}

// parent_i = the smallest column (rank) among the entries that attain the row's minimum (one thread per entry)
__global__ __launch_bounds__(256) void dp_parent_kernel(const dpi32x4* cand, long long ncand, const unsigned long long* rowmin, int32_t* parent) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= ncand) return;
    const dpi32x4 ent = cand[idx];
    const unsigned long long b = ((unsigned long long)(unsigned)ent[3] << 32) | (unsigned)ent[2];
    if (b == rowmin[ent[0]]) atomicMin(parent + ent[0], ent[1]);
}

// the densest point (row 0): the largest exact d^2 to any row, one wave per row
__global__ __launch_bounds__(256) void dp_far_kernel(const float* X, long ldx, int d, int n, unsigned long long* far) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const double s = exact_d2(exact_d2_load(X, ldx, 0, d), exact_d2_load(X, ldx, (size_t)j, d));
    if (lane_id() == 0) atomicMax(far, (unsigned long long)__double_as_longlong(s));
}

__global__ __launch_bounds__(256) void dp_finish_kernel(const unsigned long long* rowmin, const int32_t* rowcnt, const unsigned long long* far, int n,
                                                        double* delta, int32_t* parent, int32_t* longest) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) {
        delta[0] = sqrt(__longlong_as_double((long long)*far));
        parent[0] = -1;
        return;
    }
    delta[i] = sqrt(__longlong_as_double((long long)rowmin[i]));
    atomicMax(longest, rowcnt[i]);
}

// the band pairs' share of border2 (one thread per entry; .z bit 0 = the exact neighbour mask of the one eps)
__global__ __launch_bounds__(256) void dp_band_border_kernel(const dpi32x4* band, long long nband, const int32_t* labels, const int32_t* rho, int n,
                                                             int n_clusters, int32_t* border2) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nband) return;
    const dpi32x4 ent = band[idx];
    const int i = ent[0], j = ent[1];
    if (!(ent[2] & 1) || (unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) return;
    const int li = labels[i];
    if (li != labels[j] && (unsigned)li < (unsigned)n_clusters) atomicMax(border2 + li, rho[i] + rho[j]);
}

static int dp_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)dp_bound_kernel, (const void*)dp_cand_kernel, (const void*)dp_border_kernel}, "dpeaks");
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_dpeaks_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > PT_D) return 0;
    return dp_layout(N).total;
}

int dic_dpeaks_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && centre && workspace, DIC_ERR_INVALID_ARG, "dpeaks_prepare: NULL pointer");
    DIC_REQUIRE(N >= 1 && D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "dpeaks_prepare: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0 && N < (1LL << 30), DIC_ERR_UNSUPPORTED,
                "dpeaks_prepare: N=%lld D=%d (row stride %ld): D at most %d, multiples of 4", (long long)N, D, ldx, PT_D);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED,
                "dpeaks_prepare: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dpeaks_workspace(N, D), DIC_ERR_WORKSPACE, "dpeaks_prepare: workspace %zu < %zu", workspace_bytes,
                dic_dpeaks_workspace(N, D));
    int rc = pt_prepare_planes(X, ldx, centre, N, D, PT_PAD_NORM, (unsigned char*)workspace, (hipStream_t)stream, "dpeaks_prepare");
    if (rc) return rc;
    return check_launch("dpeaks_prepare");
}

int dic_dpeaks_delta(const float* X, long ldx, int64_t N, int D, int32_t* cand, int64_t capacity, double* delta, int32_t* parent, int64_t* n_cand,
                     int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && delta && parent && n_cand && stats && workspace && (cand || capacity == 0), DIC_ERR_INVALID_ARG, "dpeaks_delta: NULL pointer");
    DIC_REQUIRE(N >= 1 && D > 0 && ldx >= D && capacity >= 0, DIC_ERR_INVALID_ARG, "dpeaks_delta: N=%lld D=%d ldx=%ld capacity=%lld", (long long)N, D, ldx,
                (long long)capacity);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0 && N < (1LL << 30), DIC_ERR_UNSUPPORTED,
                "dpeaks_delta: N=%lld D=%d (row stride %ld): D at most %d, multiples of 4", (long long)N, D, ldx, PT_D);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)cand & 15) == 0, DIC_ERR_UNSUPPORTED,
                "dpeaks_delta: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dpeaks_workspace(N, D), DIC_ERR_WORKSPACE, "dpeaks_delta: workspace %zu < %zu", workspace_bytes,
                dic_dpeaks_workspace(N, D));
    *n_cand = 0;
    stats[0] = stats[1] = 0;
    int rc = dp_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const DpLayout o = dp_layout(N);
    unsigned long long* words = (unsigned long long*)(ws + pt_layout(N).count);          // cursor | far | longest
    unsigned long long* rowmin = (unsigned long long*)(ws + o.rowmin);
    int32_t* rowcnt = (int32_t*)(ws + o.rowcnt);
    int32_t* longest = (int32_t*)(words + 2);
    hipError_t e = hipMemsetAsync(words, 0, 32, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws + o.u, 0x7f, (size_t)(N + PT_T) * sizeof(unsigned), st);
    if (e == hipSuccess) e = hipMemsetAsync(rowmin, 0xff, (size_t)N * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(rowcnt, 0, (size_t)N * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(parent, 0x7f, (size_t)N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dpeaks_delta: memset: %s", hipGetErrorString(e));
    DpTileArgs t{};
    pt_fill_pair_args(t.p, ws, N);
    t.U = (unsigned*)(ws + o.u);
    t.cand = (dpi32x4*)cand;
    t.cap = capacity;
    t.cursor = words;
    const dim3 grid(pt_grid(t.p.ntiles)), blk(512);
    hipLaunchKernelGGL(dp_bound_kernel, grid, blk, PT_LDS, st, t);
    hipLaunchKernelGGL(dp_cand_kernel, grid, blk, PT_LDS, st, t);
    rc = check_launch("dpeaks_delta");
    if (rc) return rc;
    unsigned long long nc = 0;
    e = hipMemcpyAsync(&nc, words, sizeof(nc), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dpeaks_delta: reading the candidate count: %s", hipGetErrorString(e));
    *n_cand = (int64_t)nc;
    stats[0] = (int64_t)nc;
    DIC_REQUIRE((int64_t)nc <= capacity, DIC_ERR_WORKSPACE, "dpeaks_delta: %llu candidate pairs, list capacity %lld (nothing written: run again with "
                "capacity >= n_cand)", nc, (long long)capacity);
    if (nc > 0) {
        hipLaunchKernelGGL(dp_exact_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, X, ldx, D, (dpi32x4*)cand, (long long)nc, rowmin, rowcnt);
        hipLaunchKernelGGL(dp_parent_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, (const dpi32x4*)cand, (long long)nc,
                           (const unsigned long long*)rowmin, parent);
    }
    hipLaunchKernelGGL(dp_far_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, D, (int)N, words + 1);
    hipLaunchKernelGGL(dp_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)rowmin, (const int32_t*)rowcnt,
                       (const unsigned long long*)(words + 1), (int)N, delta, parent, longest);
    rc = check_launch("dpeaks_delta exact");
    if (rc) return rc;
    int32_t lg = 0;
    e = hipMemcpyAsync(&lg, longest, sizeof(lg), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dpeaks_delta: reading the longest row: %s", hipGetErrorString(e));
    stats[1] = lg;
    return DIC_OK;
}

int dic_dpeaks_border(int64_t N, int D, float threshold, const int32_t* labels, const int32_t* rho, int n_clusters, const int32_t* band, int64_t n_band,
                      int32_t* border2, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(labels && rho && border2 && workspace && (band || n_band == 0), DIC_ERR_INVALID_ARG, "dpeaks_border: NULL pointer");
    DIC_REQUIRE(N >= 1 && D > 0 && n_clusters >= 1 && n_band >= 0, DIC_ERR_INVALID_ARG, "dpeaks_border: N=%lld D=%d n_clusters=%d n_band=%lld", (long long)N, D,
                n_clusters, (long long)n_band);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && N < (1LL << 30), DIC_ERR_UNSUPPORTED, "dpeaks_border: N=%lld D=%d: D at most %d, a multiple of 4", (long long)N, D,
                PT_D);
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0, DIC_ERR_UNSUPPORTED, "dpeaks_border: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= pt_layout(N).total, DIC_ERR_WORKSPACE, "dpeaks_border: workspace %zu < %zu", workspace_bytes, pt_layout(N).total);
    DIC_REQUIRE(threshold >= 0.f, DIC_ERR_INVALID_ARG, "dpeaks_border: threshold %g", (double)threshold);
    DIC_REQUIRE(threshold < DP_MAX_THRESHOLD, DIC_ERR_UNSUPPORTED, "dpeaks_border: threshold %g: below 2^100", (double)threshold);
    int rc = dp_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(border2, 0, (size_t)n_clusters * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dpeaks_border: memset: %s", hipGetErrorString(e));
    DpTileArgs t{};
    pt_fill_pair_args(t.p, (unsigned char*)workspace, N);
    t.tl = threshold * (1.f - 0x1p-20f);          // dic_dbscan.hip's db_margins
    t.labels = labels;
    t.rho = rho;
    t.n_clusters = n_clusters;
    t.border2 = border2;
    hipLaunchKernelGGL(dp_border_kernel, dim3(pt_grid(t.p.ntiles)), dim3(512), PT_LDS, st, t);
    if (n_band > 0)
        hipLaunchKernelGGL(dp_band_border_kernel, dim3((unsigned)((n_band + 255) / 256)), dim3(256), 0, st, (const dpi32x4*)band, (long long)n_band, labels,
                           rho, (int)N, n_clusters, border2);
    return check_launch("dpeaks_border");
}

}  // extern "C"
