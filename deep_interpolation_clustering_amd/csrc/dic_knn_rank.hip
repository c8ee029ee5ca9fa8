// Neighbour ranks (include/dic_hip.h, dic_knn_ranks): where does j stand among the neighbours of i, for a short list of targets j per row -- the counterpart
// of dic_knn.hip, which returns the value at a given rank.   rank(i, j) = 1 + #{ l != i : (d^2(i, l), l) < (d^2(i, j), j) },  d^2 the f64 difference-form
// squared distance of dic_exactd2.h; a target j == i or outside [0, N) has rank 0.  Nothing N x N is stored: the pairs are recomputed tile by tile on the
// matrix cores (dic_pairtile.h) and COUNTED against per-row thresholds, the epilogue dic_knn.hip selects with (dic_candlist.h).
//
// THE APPROXIMATE d^2 ONLY NARROWS.  a_il is the tile loop's split-bf16 value, a fixed function of (i, l), and |a_il - d^2_il| < B_i = 2^-12 (n_i + nmax) for
// every l (dic_pairtile.h, dic_knn.hip).
// (1) TARGET DISTANCES.  One wave per (row, target): t = d^2(i, j) exactly, and the two f32 thresholds
//         lo = fl(fl(t) - 1.01 b),   hi = fl(fl(t) + 1.01 b),   b = fl((n_i + nmax) 2^-12)   (the f32 value kr_bound_kernel stores).
//     MARGIN.  t <= (|v_i| + |v_j|)^2 (1 + 2^-20) < 2.01 (n_i + nmax), so fl(t) is off by < 2^-24 * 2.01 (n_i + nmax) < 2^-10.9 B, the f32 difference or sum by as
//     much again, and b by 2^-24 B: together < 2^-9.8 B, far inside the .01 B = 2^-6.6 B.  Hence lo + B <= t <= hi - B in exact arithmetic, and
//       - a_il <= lo  =>  d^2_il < a_il + B <= t:  l stands CERTAINLY BEFORE the target, whatever its index;
//       - a_il > hi   =>  d^2_il > a_il - B >= t:  certainly after;
//       - lo < a_il <= hi: the BAND of the target -- the pairs only the exact stage can place.  The target's own pair lies in it (|a_ij - t| < B).
// (2) COUNTING PASSES, one per 8 targets: KnCount<16> against the 16 thresholds (lo, hi) x 8 of every row; cnt[lo] = the pairs certainly before (the self pair
//     among them: below) and cnt[hi] - cnt[lo] = the band's size.  Absent targets and the padding behind the last carry lo = hi = -inf: nothing counted.
// (3) GATHER + EXACT over groups of rows sized by the candidate budget (dic_candlist.h has the protocol, what the budget can change and the guards).  A row's
//     list holds one (l, q) entry per band pair of each of its targets q: its length is the sum of the band sizes, known from (2).  One gather pass per 8
//     targets walks the tiles of the group's row blocks.  The exact kernel, one workgroup per row, recomputes t of every target (the same function: the
//     same bits), computes d^2(i, l) of every entry with l != i and adds 1 to the target's count where (d^2(i, l), l) < (t, j).
//         rank = 1 + cnt[lo] - [lo is finite] + #{band entries before the target}.
//     The approximate products never decide an order.  The order of a list cannot matter: every entry is judged alone.
// THE SELF PAIR l = i is no neighbour, and it is taken out by its index, never by its distance (a duplicate of i at distance 0 stays in).  In a band it is an
//     entry like any other and the exact kernel skips the entry with l == i.  Whether the counting pass took it for "certainly before" depends on a_ii, which no
//     kernel stores; but d^2_ii = 0 exactly, so |a_ii| < B_i <= b (1 + 2^-24) < 1.001 b.  A target whose lo is >= 1.001 b has therefore counted the self pair
//     for certain (a_ii <= lo) and exactly once, and the exact kernel subtracts it.  A target with lo below that -- a target within about 2 B of the point --
//     gets lo = -inf: nothing is certainly before it, the self pair is not counted, and its band is everything up to hi (the few pairs with a_il < 2.01 b
//     more than the band proper).  Either way no comparison of a_ii decides anything.
// No workgroup waits for another inside a kernel; the only atomics are integer adds (counts, cursors, LDS tallies).  Two calls give the same bits.
#include "dic_exactd2.h"
#include "dic_candlist.h"
#include "dic_pairtile.h"

namespace dic {

constexpr int KR_T = 16;                               // thresholds per row and pass: (lo, hi) of
constexpr int KR_Q = KR_T / 2;                         // 8 targets
constexpr int KR_MAXM = 1023;                          // targets per row
constexpr int KR_ENTRY = 8;                            // bytes per list entry: int32 l, int32 q

struct KrLayout { size_t thr, cnt, bnd, len, off, cursor, bounds, plan, list, total; long long entries; int passes; };

static KrLayout kr_layout(int64_t N, int m, int64_t budget) {
    KrLayout o;
    if (budget <= 0) budget = CL_DEFAULT_BUDGET;
    const size_t rows = (size_t)(N + PT_T);
    const long long all = N > 3000000 ? (1LL << 62) : (long long)N * N * m;          // every pair in every band: nothing larger is ever needed
    o.entries = max(1LL, min(min((long long)(budget / KR_ENTRY), all), (1LL << 31) - 1));          // (16 GiB of lists at the most)
    o.passes = (m + KR_Q - 1) / KR_Q;
    o.thr = align_up(pt_layout(N).total, 256);
    o.cnt = o.thr + align_up((size_t)o.passes * rows * KR_T * sizeof(float), 256);
    o.bnd = o.cnt + align_up((size_t)o.passes * rows * KR_T * sizeof(int32_t), 256);
    o.len = o.bnd + align_up(rows * sizeof(float), 256);
    o.off = o.len + align_up(rows * sizeof(long long), 256);
    o.cursor = o.off + align_up((rows + 1) * sizeof(long long), 256);
    o.bounds = o.cursor + align_up(rows * sizeof(int32_t), 256);
    o.plan = o.bounds + align_up((rows + 1) * sizeof(int32_t), 256);
    o.list = o.plan + 256;
    o.total = o.list + align_up((size_t)o.entries * KR_ENTRY, 256);
    return o;
}

// b_i of every row
__global__ __launch_bounds__(256) void kr_bound_kernel(const float* nrm, const float* gmax, int n, float* bnd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bnd[i] = (nrm[i] + *gmax) * 0x1p-12f;
}

__device__ __forceinline__ int kr_target(const int32_t* targets, int i, int q, int m, int n) {
    const int j = targets[(size_t)i * m + q];
    return ((unsigned)j < (unsigned)n && j != i) ? j : -1;
}

// (1): one wave per (row, slot); slot q of pass q / 8 holds target q, or nothing (q >= m, an absent target, the row itself)
__global__ __launch_bounds__(256) void kr_target_kernel(const float* X, long ldx, int d, int n, const int32_t* targets, int m, int passes, const float* bnd,
                                                        float* thr) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int mp = passes * KR_Q;
    if (w >= (long long)n * mp) return;
    const int i = (int)(w / mp), q = (int)(w - (long long)i * mp);
    const int j = q < m ? kr_target(targets, i, q, m, n) : -1;
    float lo = -__builtin_inff(), hi = -__builtin_inff();
    if (j >= 0) {          // (uniform over the wave)
        const double t = exact_d2(exact_d2_load(X, ldx, (size_t)i, d), exact_d2_load(X, ldx, (size_t)j, d));
        const float b = bnd[i], tf = (float)t, mg = fmaf(1.01f, b, 1e-30f);          // (the tiny term: b = 0, every point AT the centre, must still leave a band)
        lo = tf - mg;
        hi = tf + mg;
        if (!(lo >= fmaf(1.001f, b, 1e-30f))) lo = -__builtin_inff();          // THE SELF PAIR (header): lo is finite only where a_ii <= lo is certain
    }
    if (lane_id() == 0) {
        float* at = thr + ((size_t)(q / KR_Q) * (size_t)(n + PT_T) + (size_t)i) * KR_T + 2 * (q % KR_Q);
        at[0] = lo;
        at[1] = hi;
    }
}

__global__ __launch_bounds__(512, 1) void kr_count_kernel(KnTileArgs a) {
    KnCount<KR_T> epi(a);
    pt_pair_pass(a.p, epi);
}

// list length of every row: the band sizes of all its targets
__global__ __launch_bounds__(256) void kr_len_kernel(const int32_t* cnt, int n, int passes, long long* len) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long s = 0;
    for (int p = 0; p < passes; ++p) {
        const int32_t* c = cnt + ((size_t)p * (size_t)(n + PT_T) + (size_t)i) * KR_T;
#pragma unroll
        for (int q = 0; q < KR_Q; ++q) s += (long long)c[2 * q + 1] - c[2 * q];
    }
    len[i] = s;
}

struct KrEntry { int32_t l, q; };

struct KrGatherArgs {
    PtPairArgs p;
    const float* thr;                        // this pass's (rows, 16) thresholds
    const long long* off; int32_t* cursor; KrEntry* list;
    int r0, r1, q0, entries;                 // rows of the group, first target of the pass, entries of the buffer (< 2^31: kr_layout)
};

// Gather epilogue: rows r0 <= i < r1 append (l, q0 + q) for every l and every target q of the pass with lo_q < a_il <= hi_q -- the comparisons the counting
// pass made, on the same values.  Per row half and band a lane builds the 64-bit membership mask, reserves its entries with one cursor add and
// writes them.
struct KrGather {
    const KrGatherArgs& a;
    const PtLane ln;
    __device__ __forceinline__ KrGather(const KrGatherArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(I0, mb);
            const bool iv = gi >= a.r0 && gi < a.r1;
            // one band at a time, its two thresholds reloaded (8 B per row, from L2): eight bands' masks at once do not fit the registers the loop leaves
#pragma unroll 1
            for (int q = 0; q < KR_Q; ++q) {
                const float lo = a.thr[(size_t)gi * KR_T + 2 * q], hi = a.thr[(size_t)gi * KR_T + 2 * q + 1];          // (gi < n + 256: inside the array)
                unsigned bits[2] = {0u, 0u};
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const float d2 = acc[nb][mb][k];          // (a padding point l is beyond every band: PT_PAD_NORM)
                        const bool in = iv && d2 > lo && d2 <= hi;
                        bits[nb >> 1] |= in ? (1u << (16 * (nb & 1) + k)) : 0u;
                    }
                const int nbits = __builtin_popcount(bits[0]) + __builtin_popcount(bits[1]);
                if (nbits) {
                    const long long o = a.off[gi] - a.off[a.r0];
                    // the list's length (< 2^31: the host checks), cut at the end of the buffer: no write beyond either, whatever happens
                    const int len = (int)max(0LL, min(a.off[gi + 1] - a.off[gi], (long long)a.entries - o));
                    int pos = atomicAdd(a.cursor + gi, nbits);
                    unsigned long long b = ((unsigned long long)bits[1] << 32) | bits[0];
                    while (b) {
                        const int p = __builtin_ctzll(b);
                        b &= b - 1;
                        if (pos < len) a.list[o + pos] = KrEntry{ln.col(J0, p >> 4, p & 15), a.q0 + q};
                        ++pos;
                    }
                }
            }
        }
    }
};

__global__ __launch_bounds__(512, 1) void kr_gather_kernel(KrGatherArgs a) {
    KrGather epi(a);
    pt_pair_pass(a.p, epi);
}

// One workgroup per row r0 + blockIdx.x: the targets' exact distances again (one wave per target: dic_exactd2.h, the bits kr_target_kernel saw), then every
// list entry (one wave per entry) judged by (d^2, index) against its target, tallied in LDS (integer atomics), then the ranks.  plan->flag is set if the
// cursor disagrees with the counted length or an entry names no point or no target (the invariants say none can happen).
__global__ __launch_bounds__(256) void kr_exact_kernel(const float* X, long ldx, int d, int n, int r0, const int32_t* targets, int m, const float* thr,
                                                       const int32_t* cnt, const long long* off, const int32_t* cursor,
                                                       const KrEntry* list, long long entries, int32_t* ranks, ClPlan* plan) {
    __shared__ double st[KR_MAXM + 1];
    __shared__ int sj[KR_MAXM + 1], tally[KR_MAXM + 1];
    const int i = r0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long len = off[i + 1] - off[i], o = off[i] - off[r0];
    const ed_f32x4 xi = exact_d2_load(X, ldx, (size_t)i, d);
    for (int q = w; q < m; q += 4) {
        const int j = kr_target(targets, i, q, m, n);
        const double t = j >= 0 ? exact_d2(xi, exact_d2_load(X, ldx, (size_t)j, d)) : 0.0;
        if (lane == 0) { st[q] = t; sj[q] = j; tally[q] = 0; }
    }
    __syncthreads();
    const bool whole = len == (long long)cursor[i] && o + len <= entries;
    if (!whole && tid == 0) plan->flag = 1;
    for (long long e = w; whole && e < len; e += 4) {
        const KrEntry en = list[o + e];
        if ((unsigned)en.l >= (unsigned)n || (unsigned)en.q >= (unsigned)m || sj[en.q] < 0) {
            if (lane == 0) plan->flag = 1;
            continue;
        }
        if (en.l == i) continue;          // the self pair: no neighbour
        const double s = exact_d2(xi, exact_d2_load(X, ldx, (size_t)en.l, d));
        const double t = st[en.q];
        if (lane == 0 && (s < t || (s == t && en.l < sj[en.q]))) atomicAdd(&tally[en.q], 1);
    }
    __syncthreads();
    for (int q = tid; q < m; q += 256) {
        int r = 0;
        if (sj[q] >= 0) {
            const size_t at = ((size_t)(q / KR_Q) * (size_t)(n + PT_T) + (size_t)i) * KR_T + 2 * (q % KR_Q);
            r = 1 + cnt[at] - (thr[at] > -__builtin_inff() ? 1 : 0) + tally[q];          // (a finite lo has counted the self pair)
        }
        ranks[(size_t)i * m + q] = r;
    }
}

static int kr_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)kr_count_kernel, (const void*)kr_gather_kernel}, "knn_ranks");
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_knn_ranks_workspace(int64_t N, int D, int m, int64_t candidate_budget) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > PT_D || m < 1 || m > KR_MAXM) return 0;
    return kr_layout(N, m, candidate_budget).total;
}

int dic_knn_ranks(const float* X, long ldx, const float* centre, int64_t N, int D, const int32_t* targets, int m, int32_t* ranks, int64_t candidate_budget,
                  int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && centre && targets && ranks && workspace, DIC_ERR_INVALID_ARG, "knn_ranks: NULL pointer");
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && m >= 1, DIC_ERR_INVALID_ARG, "knn_ranks: N=%lld D=%d ldx=%ld m=%d", (long long)N, D, ldx, m);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "knn_ranks: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(m <= KR_MAXM, DIC_ERR_UNSUPPORTED, "knn_ranks: m=%d: at most %d targets per row", m, KR_MAXM);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "knn_ranks: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)targets & 3) == 0 &&
                    ((uintptr_t)ranks & 3) == 0,
                DIC_ERR_UNSUPPORTED, "knn_ranks: operands must be 16-B aligned");
    const KrLayout o = kr_layout(N, m, candidate_budget);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "knn_ranks: workspace %zu < %zu", workspace_bytes, o.total);
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = stats[4] = 0;
    int rc = kr_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    rc = pt_prepare_planes(X, ldx, centre, N, D, PT_PAD_NORM, ws, st, "knn_ranks");
    if (rc) return rc;
    KnTileArgs t{};
    pt_fill_pair_args(t.p, ws, N);
    const size_t rows = (size_t)(N + PT_T);
    float* thr = (float*)(ws + o.thr);
    int32_t* cnt = (int32_t*)(ws + o.cnt);
    float* bnd = (float*)(ws + o.bnd);
    long long* len = (long long*)(ws + o.len);
    long long* off = (long long*)(ws + o.off);
    int32_t* cursor = (int32_t*)(ws + o.cursor);
    int32_t* bounds = (int32_t*)(ws + o.bounds);
    ClPlan* plan = (ClPlan*)(ws + o.plan);
    KrEntry* list = (KrEntry*)(ws + o.list);
    float* gmax = (float*)(ws + pt_layout(N).count);
    const int n = (int)N, P = o.passes;
    const dim3 rgrid((unsigned)((N + 255) / 256)), tgrid(pt_grid(t.p.ntiles)), tblk(512);
    // the padding rows' thresholds are read (and their rows never flushed or gathered): defined values
    hipError_t e = hipMemsetAsync(thr, 0, (size_t)P * rows * KR_T * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)P * rows * KR_T * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, rows * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_ranks: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(cl_gmax_kernel, dim3(1), dim3(256), 0, st, t.p.bmax, t.p.nblk, gmax);
    hipLaunchKernelGGL(kr_bound_kernel, rgrid, dim3(256), 0, st, t.p.nrm, (const float*)gmax, n, bnd);
    const long long waves = (long long)N * P * KR_Q;
    DIC_REQUIRE((waves + 3) / 4 < (1LL << 31), DIC_ERR_UNSUPPORTED, "knn_ranks: N=%lld x m=%d targets: too many for one launch", (long long)N, m);
    hipLaunchKernelGGL(kr_target_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, X, ldx, D, n, targets, m, P, (const float*)bnd, thr);
    for (int p = 0; p < P; ++p) {
        t.thr = thr + (size_t)p * rows * KR_T;
        t.cnt = cnt + (size_t)p * rows * KR_T;
        hipLaunchKernelGGL(kr_count_kernel, tgrid, tblk, PT_LDS, st, t);
    }
    hipLaunchKernelGGL(kr_len_kernel, rgrid, dim3(256), 0, st, (const int32_t*)cnt, n, P, len);
    hipLaunchKernelGGL((cl_scan_kernel<ClArrayLen>), dim3(1), dim3(1024), 0, st, ClArrayLen{len}, n, off, plan);
    KrGatherArgs g{};
    g.p = t.p; g.off = off; g.cursor = cursor; g.list = list; g.entries = (int)o.entries;
    const ClNames nm{"knn_ranks", "a row's bands hold", "pairs", "a row's list was incomplete or held no point"};
    return cl_run_groups(plan, off, bounds, n, 0, o.entries, KR_ENTRY, stats, P, st, nm, [&](int r0, int r1) {
        g.r0 = r0; g.r1 = r1;
        cl_walk_rows(g.p, r0, r1);
        for (int p = 0; p < P; ++p) {
            g.thr = thr + (size_t)p * rows * KR_T;
            g.q0 = p * KR_Q;
            hipLaunchKernelGGL(kr_gather_kernel, dim3(pt_grid(g.p.ntiles)), tblk, PT_LDS, st, g);
        }
        hipLaunchKernelGGL(kr_exact_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, st, X, ldx, D, n, r0, targets, m, (const float*)thr, (const int32_t*)cnt,
                           (const long long*)off, (const int32_t*)cursor, (const KrEntry*)list, o.entries, ranks, plan);
    });
}

}  // extern "C"
