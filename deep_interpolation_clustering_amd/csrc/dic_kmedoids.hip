// k-medoids (PAM: BUILD + steepest-descent SWAP with FastPAM1's shared removal term) on the matrix cores; the definition is stated once, in include/dic_hip.h.
// Classical PAM walks the N x N matrix K times per swap search.  Here one search is an approximate pass on the shared pair-tile loop that only SELECTS
// candidates, and an exact f64 stage that decides among the selected ones -- the idiom of dic_knn.hip and dic_meanshift.hip.
//
// ASSIGN (km_assign_kernel, exact): one wave per query row: d(q, m_k) = sqrt(exact_d2) for the K medoid rows, the nearest slot (ties to the smaller slot), dn
//   and ds (+inf at K = 1).  TD (km_td_kernel): one workgroup of 1024 threads, thread t adds dn[t], dn[t + 1024], .. in ascending order, then the 1024
//   partials are added by a binary tree in LDS (stride 512, 256, .., 1).
//
// DELTA PASS (km_delta_kernel<MODE>): an epilogue of pt_pair_pass.  Row operand = the candidates c, in point order (pa).  Column operand = the points o,
//   GROUPED by n(o): every group starts on a 256-row block and is padded to whole blocks, so a column tile belongs to one slot (km_rank / km_offsets /
//   km_scatter / km_pad rebuild pb from pa -- pb = -2 pa, exact; the rows between the groups zero -- once per pass, with the per-column f32 values dn, ds, ds - dn and the cut-off below).  A lane adds
//   the 64 columns it holds of each of its 2 rows in f32 and stores, for every (row, column half-tile), one partial of the shared term g, of the removal term
//   of the tile's slot, and of the error bound: every partial is stored exactly once, no atomics, nothing to zero.  km_reduce_kernel adds the partials of a
//   candidate in f64, in column order, slot by slot (the blocks of a slot are contiguous: no indexed accumulators).
//   Terms, with d~ = fl32 sqrt of the approximate d^2 (a):   MODE 0 (first BUILD step): d~.   MODE 1 (BUILD): tg = min(d~, dn) - dn.
//   MODE 2 (SWAP): tg, and for the tile's slot  tr = min(d~, ds) - min(d~, dn) - (ds - dn);  r~(c, i) = R_i + sum tr, R_i = sum_{n(o) = i} (ds - dn) in f64
//   (km_rsum_kernel) -- FastPAM1's form, in which a pair with d >= ds adds exactly 0 to both terms (at K = 1, ds = +inf: tr = d~ - min(d~, dn), R_0 = 0).
//   CUT-OFF.  cut = ds (MODE 2), dn (MODE 1), +inf (MODE 0), -inf for padding columns.  A pair is SKIPPED (adds 0, no square root) iff
//   fl(a - b0) > thr, thr = fl32(cut^2 (1 + 2^-20)) (at least FLT_MIN where cut > 0), b0 = fl32(2^-12 (n_c + nmax_J)).  dic_pairtile.h proves
//   |a - d^2| < 0.74 b0-exact, so a skipped pair has d^2 > a - b0 >= thr (1 - 2^-23) > cut^2: its terms ARE 0, no error.  Padding columns always skip.
//
//   ERROR BOUND E(c) >= |D~(c, i) - D(c, i)| for every slot i, D~ = g~ + r~_i (and >= the error of g~ and of every r~_i alone).  Per pair (c, o) the term of
//   D is min(d, dn) - dn (o outside slot i) or min(d, ds) - dn (inside): 1-Lipschitz in d, and 1-Lipschitz in dn and in ds.  So the pair's error is at most
//   |d~ - d| plus the roundings of dn, ds and of the f32 operations.
//   (a) |sqrt(a+) - d|, a+ = max(a, 0): |sqrt x - sqrt y| <= sqrt |x - y| gives <= sqrt(B) (this covers a near 0, where the derivative of the root is
//       unbounded: clipping at 0 moves a towards d^2 >= 0); |sqrt x - sqrt y| = |x - y| / (sqrt x + sqrt y) gives <= B / sqrt(a+).  The kernel takes
//       e = min(fl sqrt(b0), b0 * rsq(a')), a' = max(a, 2^-100) (v_rsq_f32 takes no denormals); b0 >= 1.35 B leaves room for every f32 rounding of e itself,
//       and |sqrt a' - sqrt a+| <= 2^-50 is added per column in the reduction.
//   (b) d~ = a' * rsq(a'): v_rsq_f32 is good to 1 ulp, the product rounds once: |d~ - sqrt a'| < 2^-22 d~.  The subtractions of the terms round to
//       2^-24 of results no larger than d~ + dn + ds.  The kernel adds 2^-20 d~ per unskipped pair.
//   (c) dn, ds, ds - dn enter as f32: 2^-24 relative each, <= 2^-22 (dn + ds) per point and independent of c; with (b)'s dn + ds part:
//       C = 2^-20 sum_o (dn + ds) (finite ds only), in f64 (km_rsum_kernel).
//   (d) summation: a lane's partial is 64 f32 additions and one shuffle addition, off by <= 65 * 2^-24 sum |terms|.  tg <= 0, K = 1's tr >= 0 and MODE 0's
//       d~ >= 0 have ONE sign, so sum |terms| = |partial sum|.  For K > 1, tr <= 0 in exact arithmetic, but ds - dn enters as fl32(ds - dn), rounded
//       independently of fl32(ds) and fl32(dn): a computed tr can be positive by up to 2^-23 (ds + dn), so sum |tr| <= |partial sum| + 2^-22 sum (ds + dn)
//       over the partial's points, and the extra 65 * 2^-24 * 2^-22 sum (ds + dn) lies far inside C's slack (C spends 2^-21 of its 2^-20 on (b) and (c)).
//       Over all partials: <= 2^-17.9 (|g~| + max_i |r~_i - R_i|); the bound's own partials are positive and are scaled by 1 + 2^-16.  The f64 additions of the reduction (at most 2 (N / 256 + K) + 1 per sum) are below 2^-40 of the same magnitudes.
//   E(c) = (1 + 2^-16) sum e  +  (2^-17 + 2^-40) (|g~| + max_i |r~_i - R_i|)  +  C  +  2^-50 (column count).
//   The pass's sums only select candidates: they need this bound, not fixed bits (they happen to be a fixed function of the inputs as well).
//
// SELECT (km_select_*): v(c) = g~(c) + min_i r~(c, i); U = min over non-medoids of v + E; every non-medoid with v - E <= U is listed (the list holds up to N
//   entries: never truncated).  The exact minimum is among them: its v - E <= its D <= D(c*) <= v(c*) + E(c*) = U for the c* that attains U.
//
// EXACT (km_exact_kernel): one workgroup of 16 waves per listed candidate at a time (the workgroups stride over the list; a candidate's sums do not depend
//   on the grid).  Wave w takes the points o = w, w + 16, .. in ascending order, d = sqrt(exact_d2),
//   and adds min(d, dn) - dn to its g and min(d, ds) - min(d, dn) to its r[n(o)] (f64, in LDS: wave-private, sequential).  Then g = the waves' g in wave order,
//   r_i = the waves' r_i in wave order, D(c, i) = g + r_i.  (MODE 0: g = sum d; MODE 1: g alone.)
// PICK (km_pick_kernel): the smallest (D, c, i) in lexicographic order over the listed candidates -- a total order, so the list's order does not matter.
#include <cfloat>
#include <type_traits>
#include "dic_pairtile.h"
#include "dic_exactd2.h"

namespace dic {

constexpr int KM_EXACT_WAVES = 16;

struct KmLayout {
    int64_t s0, rows;                                   // candidate rows (N rounded up to whole blocks), column rows (s0 + 256 K)
    int nrb, ncb;
    PtLayout pt;
    size_t cnrm, cv, rank, blkcnt, blkoff, base, rsum, part, pstride, lo, hi, bmin, total;
};

inline KmLayout km_layout(int64_t N, int K) {
    KmLayout o;
    o.s0 = (N + PT_T - 1) / PT_T * PT_T;
    o.rows = o.s0 + (int64_t)PT_T * K;
    o.nrb = (int)(o.s0 / PT_T);
    o.ncb = (int)(o.rows / PT_T);
    o.pt = pt_layout(o.rows);
    size_t at = o.pt.total;
    auto take = [&](size_t bytes) { const size_t r = at; at += align_up(bytes, 256); return r; };
    o.cnrm = take((size_t)o.rows * 4);
    o.cv = take((size_t)o.rows * 16);
    o.rank = take((size_t)o.s0 * 4);
    o.blkcnt = take((size_t)o.nrb * K * 4);
    o.blkoff = take((size_t)o.nrb * K * 4);
    o.base = take((size_t)(2 * K + 2) * 4);              // K + 1 first rows of the groups, then their K sizes
    o.rsum = take((size_t)(K + 1) * 8);
    o.pstride = (size_t)2 * o.ncb * o.s0;               // floats of one array of partials: g | e | r
    o.part = take(3 * o.pstride * 4);
    o.lo = take((size_t)o.s0 * 8);
    o.hi = take((size_t)o.s0 * 8);
    o.bmin = take((size_t)(o.nrb + 1) * 8);
    o.total = at;
    return o;
}

struct KmTileArgs {
    PtPairArgs p;
    const pf32x4* cv;                                   // per column: {dn, ds, ds - dn, thr}
    float* part;                                        // partials: g | e | r, pstride floats each, [2 column block + half][row]
    long pstride, s0;
};

// ---- exact kernels ------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void km_assign_kernel(const float* Q, long ldq, long long n_rows, int d, const float* X, long ldx, int n, const int32_t* medoids, int K,
                                                        int32_t* nearest, double* dn, double* ds, double* dist) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const ed_f32x4 q = exact_d2_load(Q, ldq, (size_t)row, d);
    double b1 = __builtin_inf(), b2 = __builtin_inf();
    int bi = 0;
    for (int k = 0; k < K; ++k) {
        const double v = sqrt(exact_d2(q, exact_d2_load(X, ldx, (size_t)min(max(medoids[k], 0), n - 1), d)));
        if (dist && lane_id() == 0) dist[(size_t)row * K + k] = v;
        if (v < b1) { b2 = b1; b1 = v; bi = k; }
        else if (v < b2) b2 = v;
    }
    if (lane_id() == 0) {
        if (nearest) nearest[row] = bi;
        if (dn) dn[row] = b1;
        if (ds) ds[row] = b2;
    }
}

__global__ __launch_bounds__(1024) void km_td_kernel(const double* dn, long long n, double* td) {
    __shared__ double part[1024];
    double s = 0.0;
    for (long long o = threadIdx.x; o < n; o += 1024) s += dn[o];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) *td = part[0];
}

// A workgroup takes the candidates blockIdx.x, blockIdx.x + gridDim.x, ..: the grid is sized by the list's CAPACITY (the count stays on the device), so a short
// list costs a short launch.
template <int MODE>
__global__ __launch_bounds__(64 * KM_EXACT_WAVES) void km_exact_kernel(const float* X, long ldx, int n, int d, const int32_t* cand, int m, const int32_t* count,
                                                                      const int32_t* nearest, const double* dn, const double* ds, int K, double* delta) {
    __shared__ double rr[KM_EXACT_WAVES][DIC_MAX_CLUSTERS];
    __shared__ double gg[KM_EXACT_WAVES];
    const int cnt = count ? min(*count, m) : m;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int cols = MODE == 2 ? K : 1;
    for (int j = blockIdx.x; j < cnt; j += gridDim.x) {
        const int c = cand ? cand[j] : j;
        if (c < 0 || c >= n) {                            // (a list entry outside the points: +inf, never picked)
            if ((int)threadIdx.x < cols) delta[(size_t)j * cols + threadIdx.x] = __builtin_inf();
            continue;
        }
        if (MODE == 2 && lane < K) rr[w][lane] = 0.0;
        const ed_f32x4 xc = exact_d2_load(X, ldx, (size_t)c, d);
        double g = 0.0;
        // (four rows in flight per wave; the terms are still added one point at a time, in ascending order)
        for (int o0 = w; o0 < n; o0 += 4 * KM_EXACT_WAVES) {
            ed_f32x4 xr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xr[u] = exact_d2_load(X, ldx, (size_t)min(o0 + u * KM_EXACT_WAVES, n - 1), d);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = o0 + u * KM_EXACT_WAVES;
                if (o >= n) break;
                const double dd = sqrt(exact_d2(xr[u], xc));
                if (MODE == 0) {
                    g += dd;
                } else {
                    const double a = dn[o], m1 = fmin(dd, a);
                    g += m1 - a;
                    if (MODE == 2 && lane == 0) {
                        const int s = min(max(nearest[o], 0), K - 1);
                        rr[w][s] += fmin(dd, ds[o]) - m1;
                    }
                }
            }
        }
        if (lane == 0) gg[w] = g;
        __syncthreads();
        if ((int)threadIdx.x < cols) {
            double gs = gg[0];
            for (int v = 1; v < KM_EXACT_WAVES; ++v) gs += gg[v];
            if (MODE == 2) {
                double rs = rr[0][threadIdx.x];
                for (int v = 1; v < KM_EXACT_WAVES; ++v) rs += rr[v][threadIdx.x];
                gs += rs;
            }
            delta[(size_t)j * cols + threadIdx.x] = gs;
        }
        __syncthreads();                                  // (the sums are read: the next candidate may overwrite them)
    }
}

// The smallest (D, c, i) in lexicographic order: (c, i) packed into one integer key (c < 2^30, i < 64), so an entry is two words.  Thread t takes the
// candidates t, t + 1024, ..; the waves reduce by shuffles, thread 0 the 16 wave results.
__device__ __forceinline__ bool km_before(double da, unsigned long long ka, double db, unsigned long long kb) { return da < db || (da == db && ka < kb); }

__global__ __launch_bounds__(1024) void km_pick_kernel(const int32_t* cand, int m, const int32_t* count, const double* delta, int cols, double* out) {
    __shared__ double sd[16];
    __shared__ unsigned long long sk[16];
    const int cnt = count ? min(*count, m) : m;
    double bd = __builtin_inf();
    unsigned long long bk = ~0ull;                          // (no entry yet)
    for (int j = threadIdx.x; j < cnt; j += 1024) {
        const unsigned long long c = (unsigned long long)(unsigned)(cand ? cand[j] : j);
        for (int i = 0; i < cols; ++i) {
            const double v = delta[(size_t)j * cols + i];
            const unsigned long long key = (c << 6) | (unsigned)i;
            if (v == v && v < __builtin_inf() && km_before(v, key, bd, bk)) { bd = v; bk = key; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const unsigned long long ok = __shfl_xor(bk, o);
        if (km_before(od, ok, bd, bk)) { bd = od; bk = ok; }
    }
    if (lane_id() == 0) { sd[threadIdx.x >> 6] = bd; sk[threadIdx.x >> 6] = bk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (km_before(sd[w], sk[w], bd, bk)) { bd = sd[w]; bk = sk[w]; }
        const bool any = bk != ~0ull;
        out[0] = any ? (double)(bk >> 6) : -1.0;
        out[1] = any ? (double)(bk & 63ull) : 0.0;
        out[2] = any ? bd : 0.0;
        out[3] = (double)cnt;
    }
}

// ---- regrouping the column operand ------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int km_slot(const int32_t* nearest, int o, int K) { return nearest ? min(max(nearest[o], 0), K - 1) : 0; }

// rank of every point among the points of its slot in its 256-row block, and the block's count per slot
__global__ __launch_bounds__(256) void km_rank_kernel(const int32_t* nearest, int n, int K, int32_t* rank, int32_t* blkcnt) {
    __shared__ int lab[256];
    const int t = threadIdx.x, o = blockIdx.x * 256 + t;
    const int mine = o < n ? km_slot(nearest, o, K) : -1;
    lab[t] = mine;
    __syncthreads();
    int rk = 0;
    for (int j = 0; j < t; ++j) rk += lab[j] == mine;
    if (o < n) rank[o] = rk;
    if (t < K) {
        int cn = 0;
        for (int j = 0; j < 256; ++j) cn += lab[j] == t;
        blkcnt[blockIdx.x * K + t] = cn;
    }
}

// per slot: the offset of every block's points inside the group; the groups' first rows, each on a block boundary (base[K] = the end of the last group),
// and behind them the groups' sizes (base[K + 1 + s])
__global__ __launch_bounds__(64) void km_offsets_kernel(const int32_t* __restrict__ blkcnt, int nrb, int K, int32_t* __restrict__ blkoff, int32_t* __restrict__ base) {
    __shared__ int tot[64];
    const int s = threadIdx.x;
    if (s < K) {
        int run = 0;
        for (int b = 0; b < nrb; ++b) {
            blkoff[b * K + s] = run;
            run += blkcnt[b * K + s];
        }
        tot[s] = run;
    }
    __syncthreads();
    if (s == 0) {
        int acc = 0;
        for (int k = 0; k < K; ++k) {
            base[k] = acc;
            base[K + 1 + k] = tot[k];
            acc += (tot[k] + PT_T - 1) / PT_T * PT_T;
        }
        base[K] = acc;
    }
}

// One wave per row of the column operand: a row no point is scattered to -- the padding behind a group, the blocks behind the last group -- becomes a zero
// row of norm 0 whose cut-off is -inf (always skipped).  Rows of points are left to km_scatter_kernel: every row the pass reads is written once per pass.
__global__ __launch_bounds__(256) void km_pad_kernel(__bf16* pb, long plane, int ncols, int K, const int32_t* base, float* cnrm, pf32x4* cv) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= ncols) return;
    bool pad = r >= base[K];
    for (int s = 0; s < K; ++s) pad |= r >= base[s] + base[K + 1 + s] && r < base[s + 1];
    if (!pad) return;
    const __bf16 z = (__bf16)0.f;
    const pbf16x4 zz = {z, z, z, z};
    const size_t at = (size_t)r * PT_LD;
    *reinterpret_cast<pbf16x4*>(pb + at + 4 * lane) = zz;
    *reinterpret_cast<pbf16x4*>(pb + plane + at + 4 * lane) = zz;
    if (lane < 8) {
        *reinterpret_cast<pbf16x4*>(pb + at + PT_D + 4 * lane) = zz;
        *reinterpret_cast<pbf16x4*>(pb + plane + at + PT_D + 4 * lane) = zz;
    }
    if (lane == 0) {
        cnrm[r] = 0.f;
        cv[r] = pf32x4{0.f, 0.f, 0.f, -__builtin_inff()};
    }
}

// One wave per point o: its row of pa becomes row `dest` of the grouped pb (coordinates times -2: exact; the norm columns in pb's arrangement), and the
// column values of the pass.
template <int MODE>
__global__ __launch_bounds__(256) void km_scatter_kernel(const __bf16* pa, __bf16* pb, long plane, const float* nrm, int n, int K, const int32_t* nearest,
                                                         const double* dn, const double* ds, const int32_t* rank, const int32_t* blkoff, const int32_t* base,
                                                         float* cnrm, pf32x4* cv) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n) return;
    const int s = km_slot(nearest, o, K);
    const size_t dest = (size_t)base[s] + blkoff[(o / PT_T) * K + s] + rank[o];
    const size_t src = (size_t)o * PT_LD, dst = dest * PT_LD;
    const pbf16x4 h = *reinterpret_cast<const pbf16x4*>(pa + src + 4 * lane);
    const pbf16x4 l = *reinterpret_cast<const pbf16x4*>(pa + plane + src + 4 * lane);
    pbf16x4 bh, bl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bh[e] = (__bf16)(-2.f * (float)h[e]);
        bl[e] = (__bf16)(-2.f * (float)l[e]);
    }
    *reinterpret_cast<pbf16x4*>(pb + dst + 4 * lane) = bh;
    *reinterpret_cast<pbf16x4*>(pb + plane + dst + 4 * lane) = bl;
    if (lane < 8) {                                     // pa: [n0 n1 n2 1 | 1 1 0 0 | 0 ..]  ->  pb: [1 1 1 n0 | n1 n2 0 0 | 0 ..]
        const pbf16x4 na = *reinterpret_cast<const pbf16x4*>(pa + src + PT_D);
        const __bf16 one = (__bf16)1.f, z = (__bf16)0.f;
        pbf16x4 eb = {z, z, z, z};
        if (lane == 0) eb = pbf16x4{one, one, one, na[0]};
        if (lane == 1) eb = pbf16x4{na[1], na[2], z, z};
        *reinterpret_cast<pbf16x4*>(pb + dst + PT_D + 4 * lane) = eb;
        *reinterpret_cast<pbf16x4*>(pb + plane + dst + PT_D + 4 * lane) = pbf16x4{z, z, z, z};
    }
    if (lane == 0) {
        cnrm[dest] = nrm[o];
        float fdn = 0.f, fds = 0.f, fdd = 0.f, thr = __builtin_inff();
        if (MODE >= 1) {
            const double a = dn[o];
            double cut = a;
            fdn = (float)a;
            if (MODE == 2) {
                const double b = ds[o];
                cut = b;
                fds = (float)b;
                fdd = b < __builtin_inf() ? (float)(b - a) : 0.f;
            }
            thr = fmaxf((float)(cut * cut * (1.0 + 0x1p-20)), cut > 0.0 ? FLT_MIN : 0.f);
        }
        cv[dest] = pf32x4{fdn, fds, fdd, thr};
    }
}

// block i < K: R_i = sum_{n(o) = i} (ds - dn) (finite ds); block K: C = 2^-20 sum (dn + ds) (finite ds).  f64, strided partials and a tree.
template <int MODE>
__global__ __launch_bounds__(256) void km_rsum_kernel(const int32_t* nearest, const double* dn, const double* ds, int n, int K, double* rsum) {
    __shared__ double part[256];
    const int i = blockIdx.x;
    double s = 0.0;
    if (MODE >= 1)
        for (int o = threadIdx.x; o < n; o += 256) {
            const double a = dn[o];
            const double b = MODE == 2 ? ds[o] : 0.0;
            const bool fin = b < __builtin_inf();
            if (i == K) s += a + (fin ? b : 0.0);
            else if (MODE == 2 && fin && km_slot(nearest, o, K) == i) s += b - a;
        }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) rsum[i] = i == K ? part[0] * 0x1p-20 : part[0];
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------------------------------------

template <int MODE>
struct KmDelta {
    const KmTileArgs& a;
    const PtLane ln;

    __device__ __forceinline__ KmDelta(const KmTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        const float bm = a.p.bmax[J0 / PT_T];
        const int cbase = J0 + 128 * ln.wn + 4 * ln.hh;
        const pf32x4* cv = a.cv + cbase;                 // per column: {dn, ds, ds - dn, thr}
        float* out = a.part + (size_t)(2 * (J0 / PT_T) + ln.wn) * a.s0;
        // One row of the lane at a time, and scheduling barriers that keep the loads of later columns from being hoisted: beside the 128 accumulator
        // registers and the next tile's first fragments there is room for about 20 values.
        auto rows = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
            const float b0 = (a.p.nrm[ln.row(I0, mb)] + bm) * 0x1p-12f;
            const float sb = sqrtf(b0);
            float sg = 0.f, sr = 0.f, se = 0.f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                unsigned keep = 0u;                      // bit k: the pair (this row, column k) is not skipped
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float thr = cv[32 * nb + (k & 3) + 8 * (k >> 2)][3];
                    keep |= (acc[nb][mb][k] - b0 > thr) ? 0u : (1u << k);
                    if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
                if (__ballot(keep != 0u) == 0ull) continue;          // (wave-uniform: none of these 32 x 32 pairs can contribute)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    pf32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (MODE >= 1) v = cv[32 * nb + (k & 3) + 8 * (k >> 2)];
                    const bool on = (keep >> k) & 1u;
                    const float ap = fmaxf(acc[nb][mb][k], 0x1p-100f);
                    const float rs = __builtin_amdgcn_rsqf(ap);
                    const float dt = ap * rs;
                    const float ee = fmaf(dt, 0x1p-20f, fminf(sb, b0 * rs));
                    float tg = dt, tr = 0.f;
                    if (MODE >= 1) {
                        const float m1 = fminf(dt, v[0]);
                        tg = m1 - v[0];
                        if (MODE == 2) tr = (fminf(dt, v[1]) - m1) - v[2];
                    }
                    sg += on ? tg : 0.f;
                    if (MODE == 2) sr += on ? tr : 0.f;
                    se += on ? ee : 0.f;
                    if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
            }
            sg += __shfl_xor(sg, 32);
            se += __shfl_xor(se, 32);
            if (MODE == 2) sr += __shfl_xor(sr, 32);
            if (ln.hh == 0) {
                float* at = out + ln.row(I0, mb);
                at[0] = sg;
                at[a.pstride] = se;
                if (MODE == 2) at[2 * a.pstride] = sr;
            }
        };
        rows(std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        rows(std::integral_constant<int, 1>{});
    }
};

template <int MODE>
__global__ __launch_bounds__(512, 1) void km_delta_kernel(KmTileArgs a) {
    KmDelta<MODE> epi(a);
    pt_pair_pass(a.p, epi);
}

// One thread per candidate: the partials in column order, in f64.
template <int MODE>
__global__ __launch_bounds__(256) void km_reduce_kernel(const float* pg, const float* pr, const float* pe, long s0, int n, int K, const int32_t* base,
                                                        const double* rsum, double* g_out, double* r_out, double* e_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int qn = 2 * (base[K] / PT_T);
    double g = 0.0, e = 0.0, rabs = 0.0;
    for (int q = 0; q < qn; ++q) {
        g += (double)pg[(size_t)q * s0 + c];
        e += (double)pe[(size_t)q * s0 + c];
    }
    if (MODE == 2)
        for (int i = 0; i < K; ++i) {
            double r = 0.0;
            for (int q = 2 * (base[i] / PT_T); q < 2 * (base[i + 1] / PT_T); ++q) r += (double)pr[(size_t)q * s0 + c];
            rabs = fmax(rabs, fabs(r));
            r_out[(size_t)c * K + i] = rsum[i] + r;
        }
    g_out[c] = g;
    e_out[c] = (1.0 + 0x1p-16) * e + (0x1p-17 + 0x1p-40) * (fabs(g) + rabs) + rsum[K] + 0x1p-50 * (double)(qn / 2 * PT_T);
}

// ---- selection --------------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void km_select_bounds_kernel(const double* g, const double* r, const double* e, int n, int cols, const int32_t* medoids, int nmed,
                                                               double* lo, double* hi, double* bmin) {
    __shared__ double part[256];
    const int c = blockIdx.x * 256 + threadIdx.x;
    double h = __builtin_inf();
    if (c < n) {
        bool med = false;
        for (int k = 0; k < nmed; ++k) med |= medoids[k] == c;
        double v = g[c], l = __builtin_inf();
        if (cols > 0) {
            double best = __builtin_inf();
            for (int i = 0; i < cols; ++i) best = fmin(best, r[(size_t)c * cols + i]);
            v += best;
        }
        if (!med && v == v) { l = v - e[c]; h = v + e[c]; }
        lo[c] = l;
        hi[c] = h;
    }
    part[threadIdx.x] = h;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = fmin(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) bmin[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void km_select_min_kernel(double* bmin, int nb, int32_t* count) {
    __shared__ double part[256];
    double h = __builtin_inf();
    for (int b = threadIdx.x; b < nb; b += 256) h = fmin(h, bmin[b]);
    part[threadIdx.x] = h;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = fmin(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { bmin[nb] = part[0]; *count = 0; }
}

__global__ __launch_bounds__(256) void km_select_list_kernel(const double* lo, const double* bmin, int nb, int n, int32_t* list, int32_t* count) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    // (integer atomic: the list's order is free, PICK's order is total; lo = +inf: a medoid, never listed)
    if (c < n && lo[c] <= bmin[nb] && lo[c] < __builtin_inf()) list[atomicAdd(count, 1)] = c;
}

static int km_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)km_delta_kernel<0>, (const void*)km_delta_kernel<1>, (const void*)km_delta_kernel<2>}, "kmedoids");
}

static bool km_shape_ok(int64_t N, int K) { return N > 0 && K >= 1 && K <= DIC_MAX_CLUSTERS && N + (int64_t)PT_T * (K + 2) < (1LL << 30); }

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_kmedoids_workspace(int64_t N, int K) {
    if (!km_shape_ok(N, K)) return 0;
    return km_layout(N, K).total;
}

int dic_kmedoids_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, int K, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && K >= 1, DIC_ERR_INVALID_ARG, "kmedoids_prepare: N=%lld D=%d ldx=%ld K=%d", (long long)N, D, ldx, K);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "kmedoids_prepare: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(km_shape_ok(N, K), DIC_ERR_UNSUPPORTED, "kmedoids_prepare: N=%lld K=%d: K <= %d, fewer than 2^30 rows", (long long)N, K, DIC_MAX_CLUSTERS);
    DIC_REQUIRE(X && centre && workspace, DIC_ERR_INVALID_ARG, "kmedoids_prepare: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED,
                "kmedoids_prepare: operands must be 16-B aligned");
    const KmLayout o = km_layout(N, K);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "kmedoids_prepare: workspace %zu < %zu", workspace_bytes, o.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const long plane = (long)((o.rows + PT_T) * PT_LD);
    __bf16* pa = (__bf16*)(ws + o.pt.pa);
    __bf16* pb = (__bf16*)(ws + o.pt.pb);
    float* nrm = (float*)(ws + o.pt.nrm);
    // everything behind the points is zero: the candidate rows of the last block, the rows the column operand may use beyond them
    const size_t tail = (size_t)(o.rows + PT_T - N) * PT_LD * sizeof(__bf16);
    hipError_t e = hipMemsetAsync(pa + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(pa + plane + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(nrm + N, 0, (size_t)(o.rows + PT_T - N) * sizeof(float), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "kmedoids_prepare: memset: %s", hipGetErrorString(e));
    // (pt_prep_kernel also writes the points' rows of pb, in point order: every pass rebuilds pb in grouped order)
    hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, (int)N, D, pa, pb, plane, nrm);
    return check_launch("kmedoids_prepare");
}

int dic_kmedoids_assign(const float* Q, long ldq, int64_t n_rows, int D, const float* X, long ldx, int64_t N, const int32_t* medoids, int K, int32_t* nearest,
                        double* dn, double* ds, double* dist, double* td, dic_stream_t stream) {
    DIC_REQUIRE(n_rows > 0 && N > 0 && D > 0 && ldq >= D && ldx >= D && K >= 1, DIC_ERR_INVALID_ARG, "kmedoids_assign: n_rows=%lld N=%lld D=%d ldq=%ld ldx=%ld K=%d",
                (long long)n_rows, (long long)N, D, ldq, ldx, K);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0 && ldq % 4 == 0, DIC_ERR_UNSUPPORTED, "kmedoids_assign: D=%d (row strides %ld, %ld): at most %d, multiples of 4",
                D, ldq, ldx, PT_D);
    DIC_REQUIRE(K <= DIC_MAX_CLUSTERS && n_rows < (1LL << 40) && N < (1LL << 30), DIC_ERR_UNSUPPORTED, "kmedoids_assign: K=%d n_rows=%lld N=%lld", K,
                (long long)n_rows, (long long)N);
    DIC_REQUIRE(Q && X && medoids && (nearest || dn || ds || dist) && (!td || dn), DIC_ERR_INVALID_ARG, "kmedoids_assign: NULL pointer (td needs dn)");
    DIC_REQUIRE(((uintptr_t)Q & 15) == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)dn & 7) == 0 && ((uintptr_t)ds & 7) == 0 && ((uintptr_t)td & 7) == 0 &&
                    ((uintptr_t)dist & 7) == 0 && ((uintptr_t)nearest & 3) == 0 && ((uintptr_t)medoids & 3) == 0,
                DIC_ERR_UNSUPPORTED, "kmedoids_assign: operands must be aligned to their element size (f32 rows to 16 B)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, Q, ldq, (long long)n_rows, D, X, ldx, (int)N, medoids, K, nearest, dn, ds, dist);
    if (td) hipLaunchKernelGGL(km_td_kernel, dim3(1), dim3(1024), 0, st, (const double*)dn, (long long)n_rows, td);
    return check_launch("kmedoids_assign");
}

int dic_kmedoids_delta_pass(int64_t N, int K_max, int K, int mode, const int32_t* nearest, const double* dn, const double* ds, double* g, double* r, double* E,
                            void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && K_max >= 1 && K >= 1 && K <= K_max && mode >= 0 && mode <= 2, DIC_ERR_INVALID_ARG, "kmedoids_delta_pass: N=%lld K_max=%d K=%d mode=%d",
                (long long)N, K_max, K, mode);
    DIC_REQUIRE(km_shape_ok(N, K_max), DIC_ERR_UNSUPPORTED, "kmedoids_delta_pass: N=%lld K_max=%d: K <= %d, fewer than 2^30 rows", (long long)N, K_max,
                DIC_MAX_CLUSTERS);
    DIC_REQUIRE(g && E && workspace && (mode < 1 || dn) && (mode < 2 || (nearest && ds && r)), DIC_ERR_INVALID_ARG, "kmedoids_delta_pass: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)dn & 7) == 0 && ((uintptr_t)ds & 7) == 0 && ((uintptr_t)g & 7) == 0 && ((uintptr_t)r & 7) == 0 &&
                    ((uintptr_t)E & 7) == 0 && ((uintptr_t)nearest & 3) == 0,
                DIC_ERR_UNSUPPORTED, "kmedoids_delta_pass: operands must be aligned to their element size (the workspace to 16 B)");
    const KmLayout o = km_layout(N, K_max);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "kmedoids_delta_pass: workspace %zu < %zu", workspace_bytes, o.total);
    int rc = km_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const int Kg = mode == 2 ? K : 1;                   // groups of the column operand
    const int32_t* lab = mode == 2 ? nearest : nullptr;
    KmTileArgs t{};
    pt_fill_pair_args(t.p, ws, o.rows);
    const long plane = t.p.plane;
    __bf16* pa = (__bf16*)(ws + o.pt.pa);
    __bf16* pb = (__bf16*)(ws + o.pt.pb);
    float* nrm = (float*)(ws + o.pt.nrm);
    float* cnrm = (float*)(ws + o.cnrm);
    pf32x4* cv = (pf32x4*)(ws + o.cv);
    int32_t *rank = (int32_t*)(ws + o.rank), *blkcnt = (int32_t*)(ws + o.blkcnt), *blkoff = (int32_t*)(ws + o.blkoff), *base = (int32_t*)(ws + o.base);
    double* rsum = (double*)(ws + o.rsum);
    // the column operand: the points scattered into their groups, the rows between and behind the groups zero rows that always skip
    const int ncols = (int)o.s0 + PT_T * Kg;              // the rows the pass reads
    hipLaunchKernelGGL(km_rank_kernel, dim3(o.nrb), dim3(256), 0, st, lab, (int)N, Kg, rank, blkcnt);
    hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)blkcnt, o.nrb, Kg, blkoff, base);
#define KM_MODES(CALL) do { if (mode == 0) { CALL(0); } else if (mode == 1) { CALL(1); } else { CALL(2); } } while (0)
#define KM_SCATTER(M)                                                                                                                                        \
    hipLaunchKernelGGL(km_scatter_kernel<M>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const __bf16*)pa, pb, plane, (const float*)nrm, (int)N, Kg, lab, dn, \
                       ds, (const int32_t*)rank, (const int32_t*)blkoff, (const int32_t*)base, cnrm, cv)
    KM_MODES(KM_SCATTER);
    hipLaunchKernelGGL(km_pad_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, st, pb, plane, ncols, Kg, (const int32_t*)base, cnrm, cv);
#define KM_RSUM(M) hipLaunchKernelGGL(km_rsum_kernel<M>, dim3(Kg + 1), dim3(256), 0, st, lab, dn, ds, (int)N, Kg, rsum)
    KM_MODES(KM_RSUM);
    hipLaunchKernelGGL(pt_block_max_kernel, dim3(ncols / PT_T), dim3(256), 0, st, (const float*)cnrm, ncols, (float*)(ws + o.pt.bmax));
    t.p.n = (int)N;
    t.p.nblk = (int)(o.s0 / PT_T) + Kg;                  // column blocks: the groups end at or before s0 + 256 Kg
    t.p.tile0 = 0;
    t.p.ntiles = (long long)o.nrb * t.p.nblk;
    t.cv = cv;
    t.part = (float*)(ws + o.part);
    t.pstride = (long)o.pstride;
    t.s0 = (long)o.s0;
#define KM_PASS(M) hipLaunchKernelGGL(km_delta_kernel<M>, dim3(pt_grid(t.p.ntiles)), dim3(512), PT_LDS, st, t)
    KM_MODES(KM_PASS);
#define KM_REDUCE(M)                                                                                                                                          \
    hipLaunchKernelGGL(km_reduce_kernel<M>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const float*)t.part, (const float*)(t.part + 2 * t.pstride), (const float*)(t.part + t.pstride), t.s0, \
                       (int)N, Kg, (const int32_t*)base, (const double*)rsum, g, r, E)
    KM_MODES(KM_REDUCE);
#undef KM_SCATTER
#undef KM_RSUM
#undef KM_PASS
#undef KM_REDUCE
    return check_launch("kmedoids_delta_pass");
}

int dic_kmedoids_select(int64_t N, int K_max, int cols, const double* g, const double* r, const double* E, const int32_t* medoids, int n_medoids, int32_t* list,
                        int32_t* count, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && K_max >= 1 && cols >= 0 && cols <= K_max && n_medoids >= 0 && n_medoids <= DIC_MAX_CLUSTERS, DIC_ERR_INVALID_ARG,
                "kmedoids_select: N=%lld K_max=%d cols=%d n_medoids=%d", (long long)N, K_max, cols, n_medoids);
    DIC_REQUIRE(km_shape_ok(N, K_max), DIC_ERR_UNSUPPORTED, "kmedoids_select: N=%lld K_max=%d: K <= %d, fewer than 2^30 rows", (long long)N, K_max, DIC_MAX_CLUSTERS);
    DIC_REQUIRE(g && E && list && count && workspace && (cols == 0 || r) && (n_medoids == 0 || medoids), DIC_ERR_INVALID_ARG, "kmedoids_select: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)g & 7) == 0 && ((uintptr_t)r & 7) == 0 && ((uintptr_t)E & 7) == 0 && ((uintptr_t)list & 3) == 0 &&
                    ((uintptr_t)count & 3) == 0 && ((uintptr_t)medoids & 3) == 0,
                DIC_ERR_UNSUPPORTED, "kmedoids_select: operands must be aligned to their element size (the workspace to 16 B)");
    const KmLayout o = km_layout(N, K_max);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "kmedoids_select: workspace %zu < %zu", workspace_bytes, o.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    double *lo = (double*)(ws + o.lo), *hi = (double*)(ws + o.hi), *bmin = (double*)(ws + o.bmin);
    const int nb = (int)((N + 255) / 256);
    hipLaunchKernelGGL(km_select_bounds_kernel, dim3(nb), dim3(256), 0, st, g, r, E, (int)N, cols, medoids, n_medoids, lo, hi, bmin);
    hipLaunchKernelGGL(km_select_min_kernel, dim3(1), dim3(256), 0, st, bmin, nb, count);
    hipLaunchKernelGGL(km_select_list_kernel, dim3(nb), dim3(256), 0, st, (const double*)lo, (const double*)bmin, nb, (int)N, list, count);
    return check_launch("kmedoids_select");
}

int dic_kmedoids_exact(const float* X, long ldx, int64_t N, int D, const int32_t* cand, int64_t M, const int32_t* count, int mode, const int32_t* nearest,
                       const double* dn, const double* ds, int K, double* delta, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && M > 0 && K >= 1 && mode >= 0 && mode <= 2, DIC_ERR_INVALID_ARG, "kmedoids_exact: N=%lld D=%d ldx=%ld M=%lld K=%d mode=%d",
                (long long)N, D, ldx, (long long)M, K, mode);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "kmedoids_exact: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(K <= DIC_MAX_CLUSTERS && N < (1LL << 30) && M < (1LL << 30), DIC_ERR_UNSUPPORTED, "kmedoids_exact: K=%d N=%lld M=%lld", K, (long long)N, (long long)M);
    DIC_REQUIRE(cand || M <= N, DIC_ERR_INVALID_ARG, "kmedoids_exact: M=%lld > N=%lld without a candidate list", (long long)M, (long long)N);
    DIC_REQUIRE(X && delta && (mode < 1 || dn) && (mode < 2 || (nearest && ds)), DIC_ERR_INVALID_ARG, "kmedoids_exact: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)dn & 7) == 0 && ((uintptr_t)ds & 7) == 0 && ((uintptr_t)delta & 7) == 0 && ((uintptr_t)nearest & 3) == 0 &&
                    ((uintptr_t)cand & 3) == 0 && ((uintptr_t)count & 3) == 0,
                DIC_ERR_UNSUPPORTED, "kmedoids_exact: operands must be aligned to their element size (X to 16 B)");
    hipStream_t st = (hipStream_t)stream;
#define KM_EXACT(MD) \
    hipLaunchKernelGGL(km_exact_kernel<MD>, dim3((unsigned)(M < 4 * kNumCU ? M : 4 * kNumCU)), dim3(64 * KM_EXACT_WAVES), 0, st, X, ldx, (int)N, D, cand, (int)M, \
                       count, nearest, dn, ds, K, delta)
    KM_MODES(KM_EXACT);
#undef KM_EXACT
#undef KM_MODES
    return check_launch("kmedoids_exact");
}

int dic_kmedoids_pick(const int32_t* cand, int64_t M, const int32_t* count, const double* delta, int cols, double* out, dic_stream_t stream) {
    DIC_REQUIRE(M > 0 && cols >= 1 && cols <= DIC_MAX_CLUSTERS, DIC_ERR_INVALID_ARG, "kmedoids_pick: M=%lld cols=%d", (long long)M, cols);
    DIC_REQUIRE(M < (1LL << 30), DIC_ERR_UNSUPPORTED, "kmedoids_pick: M=%lld", (long long)M);
    DIC_REQUIRE(delta && out, DIC_ERR_INVALID_ARG, "kmedoids_pick: NULL pointer");
    DIC_REQUIRE(((uintptr_t)delta & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)cand & 3) == 0 && ((uintptr_t)count & 3) == 0, DIC_ERR_UNSUPPORTED,
                "kmedoids_pick: operands must be aligned to their element size");
    hipLaunchKernelGGL(km_pick_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, cand, (int)M, count, delta, cols, out);
    return check_launch("kmedoids_pick");
}

}  // extern "C"
