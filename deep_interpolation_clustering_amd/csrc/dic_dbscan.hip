// DBSCAN on the matrix cores (p2_clustering_optK.py:82-85,90-168, p4_clustering_final.py:181-236): upstream builds pairwise_distances(X) (N x N f32, 22.5 GB
// at 75 000 points) and runs DBSCAN(eps, min_samples, metric='precomputed') on it.  Here every pair pass recomputes the distances tile by tile, nothing N x N is
// ever stored: the planes, the tile loop and the error bound B0 = 2^-12 (n_i + nmax_J) of its approximate d^2 (call it a_ij) are dic_pairtile.h's; this file is
// the two epilogues that decide on it, the exact recheck and the label bookkeeping.
//
// NEIGHBOUR RULE (sklearn's, bit for bit): (i, j) are neighbours for eps e iff f32(d^2_ij) <= t_e, where d^2 is the exact squared distance of the f32 points and
// t_e (f32) is the largest float s with np.sqrt(np.float32(s)) <= eps under NumPy's promotion of the caller's eps object (dbscan.py finds it on the host).  The
// self pair counts (d = 0).
//
// A lane forms y = fl(a + B0) and z = fl(a - B0), u = 2^-24, and decides the pair itself when
//   y <= tl_e = t_e (1 - 2^-20)   =>  d^2 <= a + B0 <= y (1 + u) < t_e               (a neighbour), or
//   z >  th_e = t_e (1 + 2^-20)   =>  d^2 >= a - B0 >= z (1 - u) > t_e + ulp(t_e)    (not one: its f32 rounding stays above t_e).
// The margin 2^-20 t_e also covers the difference between the exact d^2 and sklearn's f64 norm form (~2^-52 of |x_i|^2 + |x_j|^2), for points with
// |x|^2 < 2^30 t_e.  Every other pair (a BAND pair, in the band of some e) is appended to a device list and rechecked exactly: f64 difference form over the f32
// coordinates (each term exact, 256 of them summed in f64), rounded to f32, compared with every t_e.
// The 256 padding points behind the last one present the norm PT_PAD_NORM = 2^120 as operand j: their y and z lie above every tl_e / th_e, so they are neither
// counted nor put in a band and no pair is masked by its column index.  That needs thresholds well below the norm: t_e < DB_MAX_THRESHOLD = 2^100 (eps < 2^50).
//
// COUNTS (one pass, all eps): counts[e][i] = |N_eps(i)|; a band pair contributes nothing in the tile (for no e) and its exact neighbour mask from the recheck.
// COMPONENTS of the core graph, per eps: label passes L (init L[i] = i), each ONE launch of the tile kernel + one of the band list + one pointer jump:
//   every core i takes m = min L[j] over its core neighbours j (certain pairs in the tiles with y <= tl_e, band pairs with bit e of their exact mask) and, when
//   m < L[i], hooks: atomicMin(&L[L[i]], m), atomicMin(&L[i], m), and sets the changed word; the pointer jump then sets L[i] = root.  L[x] <= x always and
//   every value is a member of x's component, so the passes end with L[i] = the smallest core index of i's component; the host reads the changed word once
//   per pass.  One eps per pass (one label array): all ten at once would hold ten label sets per lane on top of the 128 accumulators.
// BORDER points come out of the same pass: a non-core i takes m = min L[j] over its core neighbours (atomicMin into border[i]).  In the last pass -- the one
// that changes nothing -- no label is written while it runs, so those minima are over the final roots: the smallest cluster id among i's core neighbours
// (sklearn's _dbscan_inner labels a border point from the first cluster that reaches it, and clusters are numbered by their smallest core index).
// No workgroup waits for another inside a kernel: the kernel boundaries are the only barriers.
#include <type_traits>
#include "dic_pairtile.h"

namespace dic {

typedef pi32x4 di32x4;

constexpr int DB_MAX_EPS = 16;
constexpr int DB_NONE = 0x7fffffff;
constexpr float DB_MAX_THRESHOLD = 0x1p100f;           // thresholds stay this far below PT_PAD_NORM

struct DbThresholds { float tl[DB_MAX_EPS], th[DB_MAX_EPS], t[DB_MAX_EPS]; };

struct DbTileArgs {
    PtPairArgs p;
    DbThresholds thr; int n_eps;
    // counts
    int32_t* counts; di32x4* band; long long cap; unsigned long long* band_count;
    // components
    const int32_t* cnt_e; int min_samples; int32_t* L; int32_t* border; int32_t* changed;
};

// Counting epilogue: counts of every eps (NE thresholds, NE >= n_eps; unused ones never match) + the band list.
template <int NE>
struct DbCount {
    const DbTileArgs& a;
    const PtLane ln;
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    int cnt[2][NE];

    __device__ __forceinline__ DbCount(const DbTileArgs& args) : a(args), ln() {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int e = 0; e < NE; ++e) cnt[mb][e] = 0;
    }
    __device__ __forceinline__ void flush() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(cur_i, mb);
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int v = cnt[mb][e] + __shfl_xor(cnt[mb][e], 32);
                if (ln.hh == 0 && gi < a.p.n && e < a.n_eps && v) atomicAdd(a.counts + (size_t)e * a.p.n + gi, v);
                cnt[mb][e] = 0;
            }
        }
    }
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i) {
            flush();
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) ni[mb] = a.p.nrm[ln.row(I0, mb)];          // (padding rows hold 0)
        }
        const float bm = a.p.bmax[J0 / PT_T];
        // the two rows of the lane, the row index a compile-time constant: as a `#pragma unroll` loop over mb this body was left rolled at NE = 16, which
        // turned cnt[mb][q] into a run-time-indexed array in scratch (5 x the time of the pass)
        auto rows = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
            const int gi = ln.row(I0, mb);
            const bool iv = gi < a.p.n;          // (a padding row i counts what it likes: never flushed; but it must not reach the band list)
            const float b0 = (ni[mb] + bm) * 0x1p-12f;
            unsigned bits[2] = {0u, 0u};
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float d2 = acc[nb][mb][k];          // (a padding point j: PT_PAD_NORM, above every tl and th)
                    const float y = d2 + b0, z = d2 - b0;
                    bool inb = false;
#pragma unroll
                    for (int q = 0; q < NE; ++q) inb |= (y > a.thr.tl[q]) & (z <= a.thr.th[q]);
#pragma unroll
                    for (int q = 0; q < NE; ++q) cnt[mb][q] += (int)((y <= a.thr.tl[q]) & !inb);
                    bits[nb >> 1] |= (iv && inb) ? (1u << (16 * (nb & 1) + k)) : 0u;
                }
            const int nbits = __builtin_popcount(bits[0]) + __builtin_popcount(bits[1]);
            if (nbits) {
                unsigned long long base = atomicAdd(a.band_count, (unsigned long long)nbits);
                for (int h = 0; h < 2; ++h) {
                    unsigned b = bits[h];
                    while (b) {
                        const int p = __builtin_ctz(b);
                        b &= b - 1;
                        if (base < (unsigned long long)a.cap) {
                            di32x4 ent;
                            ent[0] = gi; ent[1] = ln.col(J0, 2 * h + (p >> 4), p & 15); ent[2] = 0; ent[3] = 0;
                            a.band[base] = ent;
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

// Label epilogue: one label pass of eps 0 of thr.
struct DbLabel {
    const DbTileArgs& a;
    const PtLane ln;
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    int mn[2] = {DB_NONE, DB_NONE};

    __device__ __forceinline__ DbLabel(const DbTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(cur_i, mb);
            const int m = min(mn[mb], __shfl_xor(mn[mb], 32));
            if (ln.hh == 0 && gi < a.p.n && m != DB_NONE) {
                if (a.cnt_e[gi] >= a.min_samples) {
                    const int li = a.L[gi];
                    if (m < li) {
                        atomicMin(a.L + li, m);
                        atomicMin(a.L + gi, m);
                        *a.changed = 1;
                    }
                } else {
                    atomicMin(a.border + gi, m);
                }
            }
            mn[mb] = DB_NONE;
        }
    }
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i) {
            flush();
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) ni[mb] = a.p.nrm[ln.row(I0, mb)];          // (padding rows hold 0)
        }
        const float bm = a.p.bmax[J0 / PT_T];
        // labels of the 128 points j of this wave's half of the tile (DB_NONE: not a core point, or past the end): lane l holds j = jw + l and jw + 64 + l
        const int jw = J0 + 128 * ln.wn;
        int lc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = jw + 64 * h + ln.lane;
            lc[h] = (j < a.p.n && a.cnt_e[j] >= a.min_samples) ? a.L[j] : DB_NONE;
        }
        const float tl = a.thr.tl[0];
        float b0[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) b0[mb] = (ni[mb] + bm) * 0x1p-12f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int jl = 32 * (nb & 1) + 4 * ln.hh + (k & 3) + 8 * (k >> 2);
                const int v = __shfl(lc[nb >> 1], jl);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const float y = acc[nb][mb][k] + b0[mb];
                    mn[mb] = min(mn[mb], y <= tl ? v : DB_NONE);
                }
            }
    }
};

template <int NE>
__global__ __launch_bounds__(512, 1) void db_count_kernel(DbTileArgs a) {
    DbCount<NE> epi(a);
    pt_pair_pass(a.p, epi);
}

__global__ __launch_bounds__(512, 1) void db_label_kernel(DbTileArgs a) {
    DbLabel epi(a);
    pt_pair_pass(a.p, epi);
}

// Band pairs, exactly: one wave per entry, f64 difference form over the f32 coordinates; entry .z = the neighbour mask over the eps; counts += it.
__global__ __launch_bounds__(256) void db_recheck_kernel(const float* X, long ldx, int d, int n, di32x4* band, long long nband, DbThresholds thr, int n_eps,
                                                         int32_t* counts) {
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx >= nband) return;
    di32x4 ent = band[idx];
    const float* xi = X + (size_t)ent[0] * ldx;
    const float* xj = X + (size_t)ent[1] * ldx;
    double s = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double t = (double)xi[c] - (double)xj[c];
        s = fma(t, t, s);
    }
    s = wave_sum(s);
    const float d2 = (float)s;
    int mask = 0;
    for (int e = 0; e < n_eps; ++e) mask |= (d2 <= thr.t[e]) ? (1 << e) : 0;
    if (lane == 0) {
        ent[2] = mask;
        band[idx] = ent;
    }
    if (lane < n_eps && ((mask >> lane) & 1)) atomicAdd(counts + (size_t)lane * n + ent[0], 1);
}

// The band pairs' share of a label pass for eps bit e (one thread per entry).
__global__ __launch_bounds__(256) void db_band_link_kernel(const di32x4* band, long long nband, int e, const int32_t* cnt_e, int min_samples, int32_t* L,
                                                           int32_t* border, int32_t* changed) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nband) return;
    const di32x4 ent = band[idx];
    const int i = ent[0], j = ent[1];
    if (!((ent[2] >> e) & 1) || cnt_e[j] < min_samples) return;
    const int m = L[j];
    if (cnt_e[i] >= min_samples) {
        const int li = L[i];
        if (m < li) {
            atomicMin(L + li, m);
            atomicMin(L + i, m);
            *changed = 1;
        }
    } else {
        atomicMin(border + i, m);
    }
}

// L[i] = its root (L[x] <= x, so every chain ends)
__global__ __launch_bounds__(256) void db_jump_kernel(int32_t* L, int n) {
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

static int db_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)db_count_kernel<1>, (const void*)db_count_kernel<4>, (const void*)db_count_kernel<10>,
                                 (const void*)db_count_kernel<16>, (const void*)db_label_kernel}, "dbscan");
}

static void db_margins(float t, float& tl, float& th) {
    tl = t * (1.f - 0x1p-20f);
    th = t * (1.f + 0x1p-20f);
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_dbscan_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > PT_D) return 0;
    return pt_layout(N).total;
}

int dic_dbscan_counts(const float* X, long ldx, const float* centre, int64_t N, int D, const float* thresholds, int n_eps, int32_t* counts, int32_t* band,
                      int64_t capacity, int64_t* n_band, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && n_eps > 0 && capacity >= 0, DIC_ERR_INVALID_ARG, "dbscan_counts: N=%lld D=%d ldx=%ld n_eps=%d capacity=%lld",
                (long long)N, D, ldx, n_eps, (long long)capacity);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "dbscan_counts: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N < (1LL << 30) && n_eps <= DB_MAX_EPS, DIC_ERR_UNSUPPORTED, "dbscan_counts: N=%lld n_eps=%d (at most %d)", (long long)N, n_eps, DB_MAX_EPS);
    DIC_REQUIRE(X && centre && thresholds && counts && n_band && workspace && (band || capacity == 0), DIC_ERR_INVALID_ARG, "dbscan_counts: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0,
                DIC_ERR_UNSUPPORTED, "dbscan_counts: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dbscan_workspace(N, D), DIC_ERR_WORKSPACE, "dbscan_counts: workspace %zu < %zu", workspace_bytes,
                dic_dbscan_workspace(N, D));
    for (int e = 0; e < n_eps; ++e) {
        DIC_REQUIRE(thresholds[e] >= 0.f, DIC_ERR_INVALID_ARG, "dbscan_counts: threshold %d = %g", e, (double)thresholds[e]);
        DIC_REQUIRE(thresholds[e] < DB_MAX_THRESHOLD, DIC_ERR_UNSUPPORTED, "dbscan_counts: threshold %d = %g: below 2^100 (eps < 2^50)", e, (double)thresholds[e]);
    }
    int rc = db_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    unsigned long long* cnt_dev = (unsigned long long*)(ws + pt_layout(N).count);
    hipError_t e = hipMemsetAsync(cnt_dev, 0, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, (size_t)n_eps * N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan_counts: memset: %s", hipGetErrorString(e));
    rc = pt_prepare_planes(X, ldx, centre, N, D, PT_PAD_NORM, ws, st, "dbscan_counts");
    if (rc) return rc;
    DbTileArgs t{};
    pt_fill_pair_args(t.p, ws, N);
    const int ne = n_eps <= 1 ? 1 : n_eps <= 4 ? 4 : n_eps <= 10 ? 10 : 16;
    for (int q = 0; q < DB_MAX_EPS; ++q) {
        if (q < n_eps) {
            t.thr.t[q] = thresholds[q];
            db_margins(thresholds[q], t.thr.tl[q], t.thr.th[q]);
        } else {                                        // never a neighbour, never in a band
            t.thr.t[q] = -1.f;
            t.thr.tl[q] = -__builtin_inff();
            t.thr.th[q] = -__builtin_inff();
        }
    }
    t.n_eps = n_eps;
    t.counts = counts;
    t.band = (di32x4*)band;
    t.cap = capacity;
    t.band_count = cnt_dev;
    const dim3 grid(pt_grid(t.p.ntiles)), blk(512);
    switch (ne) {
        case 1: hipLaunchKernelGGL(db_count_kernel<1>, grid, blk, PT_LDS, st, t); break;
        case 4: hipLaunchKernelGGL(db_count_kernel<4>, grid, blk, PT_LDS, st, t); break;
        case 10: hipLaunchKernelGGL(db_count_kernel<10>, grid, blk, PT_LDS, st, t); break;
        default: hipLaunchKernelGGL(db_count_kernel<16>, grid, blk, PT_LDS, st, t); break;
    }
    rc = check_launch("dbscan_counts");
    if (rc) return rc;
    unsigned long long nb = 0;
    e = hipMemcpyAsync(&nb, cnt_dev, sizeof(nb), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan_counts: reading the band count: %s", hipGetErrorString(e));
    *n_band = (int64_t)nb;
    DIC_REQUIRE((int64_t)nb <= capacity, DIC_ERR_WORKSPACE, "dbscan_counts: %llu band pairs, band list capacity %lld (counts incomplete: run again with "
                "capacity >= n_band)", nb, (long long)capacity);
    if (nb > 0)
        hipLaunchKernelGGL(db_recheck_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, X, ldx, D, (int)N, (di32x4*)band, (long long)nb, t.thr,
                           n_eps, counts);
    return check_launch("dbscan_counts recheck");
}

int dic_dbscan_components_pass(int64_t N, int D, float threshold, int eps_index, const int32_t* counts_e, int min_samples, const int32_t* band, int64_t n_band,
                               int32_t* labels, int32_t* border, int32_t* changed, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && eps_index >= 0 && n_band >= 0 && min_samples >= 1, DIC_ERR_INVALID_ARG,
                "dbscan_components_pass: N=%lld D=%d eps_index=%d n_band=%lld min_samples=%d", (long long)N, D, eps_index, (long long)n_band, min_samples);
    DIC_REQUIRE(D <= PT_D && N < (1LL << 30) && eps_index < DB_MAX_EPS, DIC_ERR_UNSUPPORTED, "dbscan_components_pass: N=%lld D=%d eps_index=%d", (long long)N,
                D, eps_index);
    DIC_REQUIRE(counts_e && labels && border && changed && workspace && (band || n_band == 0), DIC_ERR_INVALID_ARG, "dbscan_components_pass: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0, DIC_ERR_UNSUPPORTED, "dbscan_components_pass: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dbscan_workspace(N, D), DIC_ERR_WORKSPACE, "dbscan_components_pass: workspace %zu < %zu", workspace_bytes,
                dic_dbscan_workspace(N, D));
    DIC_REQUIRE(threshold >= 0.f, DIC_ERR_INVALID_ARG, "dbscan_components_pass: threshold %g", (double)threshold);
    DIC_REQUIRE(threshold < DB_MAX_THRESHOLD, DIC_ERR_UNSUPPORTED, "dbscan_components_pass: threshold %g: below 2^100 (eps < 2^50)", (double)threshold);
    int rc = db_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(border, 0x7f, (size_t)N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan_components_pass: memset: %s", hipGetErrorString(e));
    DbTileArgs t{};
    pt_fill_pair_args(t.p, (unsigned char*)workspace, N);
    for (int q = 0; q < DB_MAX_EPS; ++q) t.thr.t[q] = t.thr.tl[q] = t.thr.th[q] = -1.f;
    t.thr.t[0] = threshold;
    db_margins(threshold, t.thr.tl[0], t.thr.th[0]);
    t.n_eps = 1;
    t.cnt_e = counts_e;
    t.min_samples = min_samples;
    t.L = labels;
    t.border = border;
    t.changed = changed;
    hipLaunchKernelGGL(db_label_kernel, dim3(pt_grid(t.p.ntiles)), dim3(512), PT_LDS, st, t);
    if (n_band > 0)
        hipLaunchKernelGGL(db_band_link_kernel, dim3((unsigned)((n_band + 255) / 256)), dim3(256), 0, st, (const di32x4*)band, (long long)n_band, eps_index,
                           counts_e, min_samples, labels, border, changed);
    hipLaunchKernelGGL(db_jump_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, labels, (int)N);
    return check_launch("dbscan_components_pass");
}

}  // extern "C"
