// The k-th neighbour distance of every point (p2_clustering_optK.py:110-112: NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0][:, -1]; also OPTICS' core
// distance): kth[i] = the k-th smallest of { |x_i - x_j| : j = 0..N-1 }, the self pair included (k = 1 gives 0), as the f64 square root of the f64
// difference-form squared distance of the f32 coordinates.  Nothing N x N is stored: the pairs are recomputed tile by tile on the matrix cores
// (dic_pairtile.h, the machine dic_dbscan.hip thresholds on), selection instead of thresholding.
//
// THE APPROXIMATE d^2 ONLY NARROWS THE SEARCH.  a_ij is the tile loop's split-bf16 value; it is a fixed function of (i, j) (a tile's accumulation does not
// depend on which workgroup walks it or in which launch), and |a_ij - d^2_ij| < B0 = 2^-12 (n_i + nmax_J) (dic_pairtile.h).  Per row this file uses the wider
//   B_i = 2^-12 (n_i + nmax),   nmax the largest norm of all points,   so |a_ij - d^2_ij| < B_i for every j.
// (1) COUNTING PASSES select on the a values, exactly: every row keeps a bracket (lo_i, hi_i] with  #{j : a_ij <= lo_i} < k <= #{j : a_ij <= hi_i}.  It starts
//     at lo = -2 B_i - tiny (every a_ij > -B_i: count 0) and hi = (sqrt n_i + sqrt nmax)^2 + 2 B_i (every a_ij below it: count N >= k).  A pass counts, for
//     KN_T = 16 thresholds spread evenly inside the bracket, the pairs with a_ij <= t; the bracket becomes the pair of neighbouring thresholds (or ends) whose
//     counts enclose k -- the counts are of the same a values every time, so the invariant holds by construction, whatever the rounding of the thresholds.
//     KN_REFINE = 3 passes shrink the bracket 17^3 = 4913 times, from <= 4 (n_i + nmax) to <= 1.7 B_i; finer than B_i gains nothing.
// (2) WINDOW.  a_(k), the k-th smallest a of the row, lies in (lo, hi].  At least k pairs have d^2 < a_(k) + B, at most k - 1 have d^2 < a_(k) - B, so the exact
//     k-th smallest V = d^2_(k) lies in (lo - B, hi + B).  The candidates of row i are the j with  wlo < a_ij <= whi,  wlo = lo - 2.01 B, whi = hi + 2.01 B
//     (the .01 B covers the f32 rounding of these two sums, < 2^-21 (n_i + nmax)).  Then
//       - every pair with a_ij <= wlo has d^2 < lo - B < V: CERTAINLY BELOW.  c_i = their number.
//       - every pair with a_ij > whi has d^2 > hi + B > V: certainly above.
//       - every pair with d^2 in (lo - B, hi + B) is a candidate.
//     INVARIANTS:  c_i < k <= c_i + |candidates_i|  (c_i <= #{a <= lo} < k <= #{a <= hi} <= c_i + |candidates_i|), and every pair counted into c_i has exact
//     d^2 below every candidate that can hold rank k.  Hence V = the (k - c_i)-th smallest exact d^2 among the candidates.  One more counting pass (the two
//     thresholds wlo, whi) gives c_i and |candidates_i| exactly.
// (3) GATHER + EXACT, over groups of rows sized by the candidate budget: a gather pass walks the tiles of the group's row blocks and appends every candidate
//     j to row i's list (list offsets = the prefix sum of the counts of (2), taken on the device; the slot inside a list comes from an integer atomic
//     cursor -- the order of a list cannot matter, the value at a rank does not depend on it).  The exact kernel computes the f64 difference-form d^2 of every list entry (each term exact,
//     summed in a fixed order) and selects rank k - c_i by a radix select over the bit patterns of the (non-negative) doubles: the value AT the rank, ties or
//     not.  The approximate products never decide the rank and never supply the value.
// No workgroup waits for another inside a kernel; the only atomics are integer adds (counts, list cursors).  Two calls give the same bits.
#include "dic_exactd2.h"
#include "dic_knn_count.h"          // KnTileArgs, KnCount: the counting epilogue, shared with dic_knn_rank.hip
#include "dic_pairtile.h"

namespace dic {

constexpr int KN_T = 16;                               // thresholds per row and refining pass
constexpr int KN_REFINE = 3;                           // refining passes
constexpr int KN_ENTRY = 12;                           // bytes of candidate storage per list entry: int32 index + f64 d^2
constexpr long long KN_DEFAULT_BUDGET = 384LL << 20;   // bytes (list sizes at 75 000 x 256)

struct KnLayout { size_t thr, cnt, lo, hi, bnd, off, cursor, bounds, plan, idx, d2, total; long long entries; };
struct KnPlan { long long total, longest, groups; int flag; };          // device words the host reads back

static long long kn_entries(int64_t N, int64_t budget) {
    if (budget <= 0) budget = KN_DEFAULT_BUDGET;
    const long long all = (long long)N * N;          // every pair a candidate: nothing larger is ever needed
    return max(1LL, min((long long)(budget / KN_ENTRY), all));
}

static KnLayout kn_layout(int64_t N, int64_t budget) {
    KnLayout o;
    const size_t rows = (size_t)(N + PT_T);
    o.entries = kn_entries(N, budget);
    o.thr = align_up(pt_layout(N).total, 256);
    o.cnt = o.thr + align_up(rows * KN_T * sizeof(float), 256);
    o.lo = o.cnt + align_up(rows * KN_T * sizeof(int32_t), 256);
    o.hi = o.lo + align_up(rows * sizeof(float), 256);
    o.bnd = o.hi + align_up(rows * sizeof(float), 256);
    o.off = o.bnd + align_up(rows * sizeof(float), 256);
    o.cursor = o.off + align_up((rows + 1) * sizeof(long long), 256);
    o.bounds = o.cursor + align_up(rows * sizeof(int32_t), 256);
    o.plan = o.bounds + align_up((rows + 1) * sizeof(int32_t), 256);
    o.idx = o.plan + 256;
    o.d2 = o.idx + align_up((size_t)o.entries * sizeof(int32_t), 256);
    o.total = o.d2 + align_up((size_t)o.entries * sizeof(double), 256);
    return o;
}

// nmax = the largest norm (one workgroup over the block maxima)
__global__ __launch_bounds__(256) void kn_gmax_kernel(const float* bmax, int nblk, float* gmax) {
    __shared__ float part[4];
    float v = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) v = fmaxf(v, bmax[i]);
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *gmax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

__device__ __forceinline__ void kn_spread(float lo, float hi, float* thr) {
    const float wdt = hi - lo;
#pragma unroll
    for (int q = 0; q < KN_T; ++q) thr[q] = fminf(lo + wdt * ((float)(q + 1) / (float)(KN_T + 1)), hi);
}

// the first bracket of every row and its thresholds
__global__ __launch_bounds__(256) void kn_init_kernel(const float* nrm, const float* gmax, int n, float* lo, float* hi, float* bnd, float* thr, int32_t* cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float ni = nrm[i], nm = *gmax;
    const float b = (ni + nm) * 0x1p-12f;
    const float s = sqrtf(ni) + sqrtf(nm);
    const float l = -2.f * b - 1e-30f, h = s * s * (1.f + 0x1p-16f) + 2.f * b;
    lo[i] = l; hi[i] = h; bnd[i] = b;
    kn_spread(l, h, thr + (size_t)i * KN_T);
#pragma unroll
    for (int q = 0; q < KN_T; ++q) cnt[(size_t)i * KN_T + q] = 0;
}

// After a refining pass: the new bracket from the counts (zeroed for the next pass), and the next thresholds.
__global__ __launch_bounds__(256) void kn_bracket_kernel(int n, int k, float* lo, float* hi, float* thr, int32_t* cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float l = lo[i], h = hi[i];
    bool open = true;
#pragma unroll
    for (int q = 0; q < KN_T; ++q) {
        const float t = thr[(size_t)i * KN_T + q];
        const int c = cnt[(size_t)i * KN_T + q];
        cnt[(size_t)i * KN_T + q] = 0;
        if (c < k) l = t;
        else if (open) { h = t; open = false; }
    }
    lo[i] = l; hi[i] = h;
    kn_spread(l, h, thr + (size_t)i * KN_T);
}

// the window (wlo, whi) of every row, at stride 2 (a launch of its own: it overwrites the refining thresholds of other rows)
__global__ __launch_bounds__(256) void kn_window_kernel(int n, const float* lo, const float* hi, const float* bnd, float* thr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float m = 2.01f * bnd[i];
    thr[(size_t)i * 2] = lo[i] - m;
    thr[(size_t)i * 2 + 1] = hi[i] + m;
}

// List lengths -> off[0..n] (exclusive prefix sum: row i's list is entries off[i] - off[r0] .. of its group's buffer), their total and the longest.
// One workgroup; thread t owns a contiguous run of rows.
__global__ __launch_bounds__(1024) void kn_scan_kernel(const int32_t* cnt, int n, long long* off, KnPlan* plan) {
    __shared__ long long part[1024], longest[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024, b = min(n, tid * per), e = min(n, b + per);
    long long s = 0, m = 0;
    for (int i = b; i < e; ++i) {
        const long long len = (long long)cnt[(size_t)i * 2 + 1] - cnt[(size_t)i * 2];
        s += len;
        m = max(m, len);
    }
    part[tid] = s; longest[tid] = m;
    __syncthreads();
    if (tid == 0) {
        long long run = 0, mm = 0;
        for (int t = 0; t < 1024; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
            mm = max(mm, longest[t]);
        }
        off[n] = run;
        plan->total = run; plan->longest = mm; plan->groups = 0; plan->flag = 0;
    }
    __syncthreads();
    s = part[tid];
    for (int i = b; i < e; ++i) {
        off[i] = s;
        s += (long long)cnt[(size_t)i * 2 + 1] - cnt[(size_t)i * 2];
    }
}

// The groups: consecutive rows, as many as fit `entries` list entries (no list is longer than that: checked by the host before this runs).
// bounds[g] = first row of group g, bounds[groups] = n.
__global__ void kn_groups_kernel(const long long* off, int n, long long entries, int32_t* bounds, KnPlan* plan) {
    if (threadIdx.x || blockIdx.x) return;
    int g = 0, r = 0;
    while (r < n) {
        bounds[g++] = r;
        const long long lim = off[r] + entries;
        int a = r + 1, b = n;          // the largest e in [r + 1, n] with off[e] <= lim  (off[r + 1] <= lim holds)
        while (a < b) {
            const int mid = (a + b + 1) / 2;
            if (off[mid] <= lim) a = mid;
            else b = mid - 1;
        }
        r = a;
    }
    bounds[g] = n;
    plan->groups = g;
}

// Gather epilogue: rows r0 <= i < r1 append every j with wlo_i < a_ij <= whi_i to their list.
struct KnGather {
    const KnTileArgs& a;
    const PtLane ln;
    __device__ __forceinline__ KnGather(const KnTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(I0, mb);
            const bool iv = gi >= a.r0 && gi < a.r1;
            const float wlo = a.thr[(size_t)gi * 2], whi = a.thr[(size_t)gi * 2 + 1];
            unsigned bits[2] = {0u, 0u};
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float d2 = acc[nb][mb][k];
                    const bool in = iv && d2 > wlo && d2 <= whi;          // (a padding point j is beyond every window: PT_PAD_NORM)
                    bits[nb >> 1] |= in ? (1u << (16 * (nb & 1) + k)) : 0u;
                }
            const int nbits = __builtin_popcount(bits[0]) + __builtin_popcount(bits[1]);
            if (nbits) {
                const int len = a.cnt[(size_t)gi * 2 + 1] - a.cnt[(size_t)gi * 2];          // the list's length: no write beyond it, whatever happens
                const long long o = a.off[gi] - a.off[a.r0];
                int pos = atomicAdd(a.cursor + gi, nbits);
                for (int h = 0; h < 2; ++h) {
                    unsigned b = bits[h];
                    while (b) {
                        const int p = __builtin_ctz(b);
                        b &= b - 1;
                        if (pos < len && o + pos < a.entries) a.idx[o + pos] = ln.col(J0, 2 * h + (p >> 4), p & 15);
                        ++pos;
                    }
                }
            }
        }
    }
};

template <int T>
__global__ __launch_bounds__(512, 1) void kn_count_kernel(KnTileArgs a) {
    KnCount<T> epi(a);
    pt_pair_pass(a.p, epi);
}

__global__ __launch_bounds__(512, 1) void kn_gather_kernel(KnTileArgs a) {
    KnGather epi(a);
    pt_pair_pass(a.p, epi);
}

// One workgroup per row of the group: the exact d^2 of every list entry (one wave per entry: dic_exactd2.h -- lane l holds coordinates 4 l .. 4 l + 3, f64
// difference form, fixed summation order; dic_optics.hip computes its distances with the same function), then the value at rank k - c_i by a radix select over the doubles' bit patterns (non-negative: unsigned order = numeric order),
// eight 8-bit digits from the top.  kth[i] = its square root.  plan->flag is set if a row's rank falls outside its list or a list slot holds no point (the
// invariants say neither can happen).
__global__ __launch_bounds__(256) void kn_exact_kernel(const float* X, long ldx, int d, int n, int r0, int k, const int32_t* cnt, const long long* off,
                                                       const int32_t* idx, double* d2, long long entries, double* kth, KnPlan* plan) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel_prefix;
    __shared__ int sel_rank;
    const int i = r0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = cnt[(size_t)i * 2], len = cnt[(size_t)i * 2 + 1] - c;
    const long long o = off[i] - off[r0];
    int rank = k - c;          // 1-based, within the list
    if (rank < 1 || rank > len || o + len > entries) {
        if (tid == 0) {
            plan->flag = 1;
            kth[i] = __builtin_nan("");
        }
        return;
    }
    const ed_f32x4 xi = exact_d2_load(X, ldx, (size_t)i, d);
    for (int e = w; e < len; e += 4) {
        int j = idx[o + e];
        if ((unsigned)j >= (unsigned)n) {          // a slot the gather pass did not fill (it fills every one): stay inside X and report
            if (lane == 0) plan->flag = 1;
            j = i;
        }
        const double s = exact_d2(xi, exact_d2_load(X, ldx, (size_t)j, d));
        if (lane == 0) d2[o + e] = s;
    }
    __syncthreads();
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int e = tid; e < len; e += 256) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(d2[o + e]);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int r = rank, b = 0;
            for (; b < 255; ++b) {
                const int h = (int)hist[b];
                if (r <= h) break;
                r -= h;
            }
            sel_rank = r;
            sel_prefix = prefix | ((unsigned long long)b << shift);
        }
        __syncthreads();
        rank = sel_rank;
        prefix = sel_prefix;
    }
    if (tid == 0) kth[i] = sqrt(__longlong_as_double((long long)prefix));
}

// ---- neighbour lists (dic_knn_neighbors) ----------------------------------------------------------------------------------------------------------------
// Row q of the result = the k index points j with the smallest keys (d^2(q, j), j), sorted by that key; d^2 the exact distance above.  The same machine on
// the STACKED set: index points in rows [0, N), queries in rows [N, N + M) (the self join: M = 0 and every row is a query).
//   - As operand j a query presents the norm PT_PAD_NORM, exactly as the padding points do: its a_ij = 2^120 lies beyond every threshold, so the counting and
//     gather epilogues above admit the index points only and run unchanged.  As operand i it carries its own norm; nmax is over the stacked set, so B_i holds.
//   - Only the row blocks that hold a query are walked, and of each only the column blocks that hold an index point: the tile loop splits a tile number by
//     PtPairArgs.nblk, so nblk = the column blocks of [0, N) and tile0 = first row block * nblk walk exactly that rectangle.
//   - The counts are over the fixed column set [0, N), N >= k: the bracket argument (1) carries over.  V = d^2_(k) < hi + B, so every pair with d^2 <= V --
//     every tie at V included -- has a_ij < hi + 2 B <= whi: the list { j : a_ij <= whi } (window with wlo = -inf: c_i = 0) holds the whole answer, k entries
//     or more (k plus a few on ordinary data, up to N with duplicates or on a lattice).
//   - Exact stage, one workgroup per row: f64 d^2 of every entry, a radix select of the key of rank k over (bits of d^2, j) -- the select above with the index
//     as four more low-order digits; keys are distinct, so exactly k entries lie at or below it -- those k compacted into LDS (12 KB at k = 1024), a bitonic
//     sort there (keys and indices in arrays of their own: 8-B and 4-B elements at unit stride, so every compare-exchange distance but the last is free of
//     bank conflicts; the last, neighbours 16 B apart, is 2-way), and the row written.  The order the gather filled the list in cannot matter.
constexpr int KN_MAXK = 1024;

// queries (and the padding behind them) as operand j: rows first .. first + count - 1 of pb present the norm pad_norm
__global__ __launch_bounds__(256) void knl_mask_cols_kernel(__bf16* pb, long long first, long long count, float pad_norm) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < count) pb[(size_t)(first + t) * PT_LD + PT_D + 3] = (__bf16)pad_norm;
}

// the list window of every row, at stride 2: everything up to whi
__global__ __launch_bounds__(256) void knl_window_kernel(int n, const float* hi, const float* bnd, float* thr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    thr[(size_t)i * 2] = -__builtin_inff();
    thr[(size_t)i * 2 + 1] = hi[i] + 2.01f * bnd[i];
}

// One workgroup per row r0 + blockIdx.x of the stacked set (row `first` = query 0 = output row 0).  plan->flag is set if a list is shorter than k, a slot
// holds no index point or the select does not leave exactly k entries (the invariants say none can happen); the row is then NaN / -1.
__global__ __launch_bounds__(256) void knl_exact_kernel(const float* X, long ldx, const float* Q, long ldq, int d, int n, int first, int r0, int k,
                                                        const int32_t* cnt, const long long* off, const int32_t* idx, double* d2, long long entries,
                                                        double* dist, int32_t* nbr, KnPlan* plan) {
    __shared__ unsigned long long sk[KN_MAXK];
    __shared__ int sj[KN_MAXK];
    __shared__ unsigned hist[256];
    __shared__ int wtot[4];
    __shared__ int sel_digit, sel_rank, sel_count, filled;
    const int i = r0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int len = cnt[(size_t)i * 2 + 1] - cnt[(size_t)i * 2];
    const long long o = off[i] - off[r0];
    double* drow = dist + (size_t)(i - first) * k;
    int32_t* jrow = nbr + (size_t)(i - first) * k;
    if (k > len || o + len > entries) {
        if (tid == 0) plan->flag = 1;
        for (int r = tid; r < k; r += 256) { drow[r] = __builtin_nan(""); jrow[r] = -1; }
        return;
    }
    const ed_f32x4 xi = Q ? exact_d2_load(Q, ldq, (size_t)(i - first), d) : exact_d2_load(X, ldx, (size_t)i, d);
    for (int e = w; e < len; e += 4) {
        int j = idx[o + e];
        if ((unsigned)j >= (unsigned)n) {          // a slot the gather pass did not fill (it fills every one): stay inside X and report
            if (lane == 0) plan->flag = 1;
            j = 0;
        }
        const double s = exact_d2(xi, exact_d2_load(X, ldx, (size_t)j, d));
        if (lane == 0) d2[o + e] = s;
    }
    if (tid == 0) filled = 0;
    __syncthreads();
    // the key (pd, pj) of rank k: twelve 8-bit digits from the top, eight of the double's bit pattern (non-negative: unsigned order = numeric order), four of j
    unsigned long long pd = ~0ULL;
    unsigned pj = ~0u;
    if (len > k) {
        pd = 0; pj = 0;
        int rank = k;
        for (int p = 0; p < 12; ++p) {
            const int shift = p < 8 ? 56 - 8 * p : 24 - 8 * (p - 8);
            hist[tid] = 0;
            __syncthreads();
            for (int e = tid; e < len; e += 256) {
                const unsigned long long key = (unsigned long long)__double_as_longlong(d2[o + e]);
                const unsigned j = (unsigned)idx[o + e];
                bool in;
                unsigned digit;
                if (p < 8) {
                    in = p == 0 || (key >> (shift + 8)) == (pd >> (shift + 8));
                    digit = (unsigned)(key >> shift) & 255u;
                } else {
                    in = key == pd && (p == 8 || (j >> (shift + 8)) == (pj >> (shift + 8)));
                    digit = (j >> shift) & 255u;
                }
                if (in) atomicAdd(&hist[digit], 1u);
            }
            __syncthreads();
            // inclusive prefix sum of the 256 bins, one per thread; the bin that takes the running count to `rank` holds the digit
            const int h = (int)hist[tid];
            int incl = h;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int up = __shfl_up(incl, s);
                if (lane >= s) incl += up;
            }
            if (lane == 63) wtot[w] = incl;
            __syncthreads();
            for (int q = 0; q < w; ++q) incl += wtot[q];
            if (incl - h < rank && rank <= incl) {          // exactly one bin: 1 <= rank <= the sum of all bins
                sel_digit = tid;
                sel_rank = rank - (incl - h);
                sel_count = h;
            }
            __syncthreads();
            rank = sel_rank;
            if (p < 8) pd |= (unsigned long long)sel_digit << shift;
            else pj |= (unsigned)sel_digit << shift;
            if (p == 7 && sel_count == rank) {          // every entry at d^2 = pd is taken (no tie across the cut: the usual case)
                pj = ~0u;
                break;
            }
        }
    }
    for (int e = tid; e < len; e += 256) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(d2[o + e]);
        const int j = idx[o + e];
        if (key < pd || (key == pd && (unsigned)j <= pj)) {
            const int slot = atomicAdd(&filled, 1);
            if (slot < KN_MAXK) { sk[slot] = key; sj[slot] = j; }
        }
    }
    __syncthreads();
    if (filled != k) {
        if (tid == 0) plan->flag = 1;
        for (int r = tid; r < k; r += 256) { drow[r] = __builtin_nan(""); jrow[r] = -1; }
        return;
    }
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int t = k + tid; t < n2; t += 256) { sk[t] = ~0ULL; sj[t] = 0x7fffffff; }
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < n2 / 2; t += 256) {
                const int a = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), b = a + stride;
                const unsigned long long ka = sk[a], kb = sk[b];
                const int ja = sj[a], jb = sj[b];
                const bool gt = ka > kb || (ka == kb && ja > jb);
                if (gt == ((a & size) == 0)) { sk[a] = kb; sk[b] = ka; sj[a] = jb; sj[b] = ja; }
            }
        }
    __syncthreads();
    for (int r = tid; r < k; r += 256) {
        drow[r] = sqrt(__longlong_as_double((long long)sk[r]));
        jrow[r] = sj[r];
    }
}

// pt_prepare_planes for the stacked set: the index points, the queries behind them (as operand j under the padding points' norm), the padding behind both.
static int knl_prepare_planes(const float* X, long ldx, int64_t N, const float* Q, long ldq, int64_t M, const float* centre, int D, unsigned char* ws,
                              hipStream_t st) {
    const int64_t P = N + M;
    const PtLayout o = pt_layout(P);
    const long plane = (long)((P + PT_T) * PT_LD);
    __bf16* pa = (__bf16*)(ws + o.pa);
    __bf16* pb = (__bf16*)(ws + o.pb);
    float* nrm = (float*)(ws + o.nrm);
    hipError_t e = hipMemsetAsync(pa + (size_t)P * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pa + plane + (size_t)P * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + (size_t)P * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + plane + (size_t)P * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(nrm + P, 0, (size_t)PT_T * sizeof(float), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, (int)N, D, pa, pb, plane, nrm);
    if (M > 0)
        hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, Q, ldq, centre, (int)M, D, pa + (size_t)N * PT_LD, pb + (size_t)N * PT_LD,
                           plane, nrm + N);
    hipLaunchKernelGGL(knl_mask_cols_kernel, dim3((unsigned)((M + PT_T + 255) / 256)), dim3(256), 0, st, pb, (long long)N, (long long)(M + PT_T), PT_PAD_NORM);
    hipLaunchKernelGGL(pt_block_max_kernel, dim3((unsigned)((P + PT_T - 1) / PT_T)), dim3(256), 0, st, (const float*)nrm, (int)P, (float*)(ws + o.bmax));
    return DIC_OK;
}

static int kn_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)kn_count_kernel<KN_T>, (const void*)kn_count_kernel<2>, (const void*)kn_gather_kernel}, "knn");
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_knn_workspace(int64_t N, int D, int64_t candidate_budget) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > PT_D) return 0;
    return kn_layout(N, candidate_budget).total;
}

int dic_knn_kth_distance(const float* X, long ldx, const float* centre, int64_t N, int D, int64_t k, double* kth, int64_t candidate_budget, int64_t* stats,
                         void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && centre && kth && workspace, DIC_ERR_INVALID_ARG, "knn_kth_distance: NULL pointer");
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "knn_kth_distance: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "knn_kth_distance: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx,
                PT_D);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "knn_kth_distance: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(k >= 1 && k <= N, DIC_ERR_UNSUPPORTED, "knn_kth_distance: k=%lld: expected 1 <= k <= N=%lld", (long long)k, (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)kth & 7) == 0,
                DIC_ERR_UNSUPPORTED, "knn_kth_distance: operands must be 16-B aligned");
    const KnLayout o = kn_layout(N, candidate_budget);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "knn_kth_distance: workspace %zu < %zu", workspace_bytes, o.total);
    int rc = kn_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    rc = pt_prepare_planes(X, ldx, centre, N, D, PT_PAD_NORM, ws, st, "knn_kth_distance");
    if (rc) return rc;
    KnTileArgs t{};
    pt_fill_pair_args(t.p, ws, N);
    float* thr = (float*)(ws + o.thr);
    int32_t* cnt = (int32_t*)(ws + o.cnt);
    float* lo = (float*)(ws + o.lo);
    float* hi = (float*)(ws + o.hi);
    float* bnd = (float*)(ws + o.bnd);
    long long* off = (long long*)(ws + o.off);
    int32_t* cursor = (int32_t*)(ws + o.cursor);
    int32_t* bounds = (int32_t*)(ws + o.bounds);
    KnPlan* plan = (KnPlan*)(ws + o.plan);
    float* gmax = (float*)(ws + pt_layout(N).count);
    t.thr = thr; t.cnt = cnt; t.off = off; t.cursor = cursor; t.idx = (int32_t*)(ws + o.idx); t.entries = o.entries;
    const int n = (int)N, kk = (int)k;
    const dim3 rows((unsigned)((N + 255) / 256)), tgrid(pt_grid(t.p.ntiles)), tblk(512);
    // the padding rows' thresholds and window are read (and masked): defined values
    hipError_t e = hipMemsetAsync(thr + (size_t)N * KN_T, 0, (size_t)PT_T * KN_T * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, (size_t)N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_kth_distance: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kn_gmax_kernel, dim3(1), dim3(256), 0, st, t.p.bmax, t.p.nblk, gmax);
    hipLaunchKernelGGL(kn_init_kernel, rows, dim3(256), 0, st, t.p.nrm, (const float*)gmax, n, lo, hi, bnd, thr, cnt);
    for (int p = 0; p < KN_REFINE; ++p) {
        hipLaunchKernelGGL((kn_count_kernel<KN_T>), tgrid, tblk, PT_LDS, st, t);
        hipLaunchKernelGGL(kn_bracket_kernel, rows, dim3(256), 0, st, n, kk, lo, hi, thr, cnt);
    }
    hipLaunchKernelGGL(kn_window_kernel, rows, dim3(256), 0, st, n, (const float*)lo, (const float*)hi, (const float*)bnd, thr);
    hipLaunchKernelGGL((kn_count_kernel<2>), tgrid, tblk, PT_LDS, st, t);
    hipLaunchKernelGGL(kn_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)cnt, n, off, plan);
    rc = check_launch("knn_kth_distance counting");
    if (rc) return rc;
    // the list lengths decide the groups: read their summary back (synchronises the stream)
    KnPlan hp;
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_kth_distance: reading the list lengths: %s", hipGetErrorString(e));
    if (stats) {
        stats[0] = KN_REFINE + 1;
        stats[1] = 0;
        stats[2] = hp.longest;
        stats[3] = hp.total;
        stats[4] = hp.longest * KN_ENTRY;
    }
    DIC_REQUIRE(hp.longest <= o.entries, DIC_ERR_WORKSPACE, "knn_kth_distance: a row has %lld candidates (%lld bytes), candidate_budget holds %lld (%lld "
                "bytes): run again with candidate_budget >= %lld", hp.longest, hp.longest * KN_ENTRY, o.entries, o.entries * KN_ENTRY, hp.longest * KN_ENTRY);
    hipLaunchKernelGGL(kn_groups_kernel, dim3(1), dim3(64), 0, st, (const long long*)off, n, o.entries, bounds, plan);
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_kth_distance: reading the groups: %s", hipGetErrorString(e));
    if (stats) stats[1] = hp.groups;
    constexpr int CHUNK = 1024;          // group bounds come back this many at a time
    int32_t hb[CHUNK + 1];
    for (long long g0 = 0; g0 < hp.groups; g0 += CHUNK) {
        const int ng = (int)min((long long)CHUNK, hp.groups - g0);
        e = hipMemcpyAsync(hb, bounds + g0, (size_t)(ng + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_kth_distance: reading the groups: %s", hipGetErrorString(e));
        for (int g = 0; g < ng; ++g) {
            const int r0 = hb[g], r1 = hb[g + 1];
            DIC_REQUIRE(r0 >= 0 && r0 < r1 && r1 <= n, DIC_ERR_LAUNCH, "knn_kth_distance: group %lld = rows [%d, %d)", g0 + g, r0, r1);
            const int b0 = r0 / PT_T, b1 = (r1 + PT_T - 1) / PT_T;
            t.r0 = r0; t.r1 = r1;
            t.p.tile0 = (long long)b0 * t.p.nblk;
            t.p.ntiles = (long long)(b1 - b0) * t.p.nblk;
            hipLaunchKernelGGL(kn_gather_kernel, dim3(pt_grid(t.p.ntiles)), tblk, PT_LDS, st, t);
            hipLaunchKernelGGL(kn_exact_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, st, X, ldx, D, n, r0, kk, (const int32_t*)cnt, (const long long*)off,
                               (const int32_t*)t.idx, (double*)(ws + o.d2), o.entries, kth, plan);
        }
        rc = check_launch("knn_kth_distance gather");
        if (rc) return rc;
    }
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_kth_distance: %s", hipGetErrorString(e));
    DIC_REQUIRE(hp.flag == 0, DIC_ERR_LAUNCH, "knn_kth_distance: a row's rank fell outside its candidate list or a list was incomplete (non-finite coordinates?)");
    return DIC_OK;
}

size_t dic_knn_neighbors_workspace(int64_t N, int64_t M, int D, int64_t candidate_budget) {
    if (N <= 0 || M < 0 || N + M >= (1LL << 30) || D <= 0 || D > PT_D) return 0;
    return kn_layout(N + M, candidate_budget).total;
}

int dic_knn_neighbors(const float* X, long ldx, int64_t N, const float* Q, long ldq, int64_t M, const float* centre, int D, int k, double* dist, int32_t* idx,
                      int64_t candidate_budget, int64_t* stats, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && centre && dist && idx && workspace, DIC_ERR_INVALID_ARG, "knn_neighbors: NULL pointer");
    if (!Q) { M = 0; ldq = ldx; }
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && (!Q || (M > 0 && ldq >= D)), DIC_ERR_INVALID_ARG, "knn_neighbors: N=%lld M=%lld D=%d ldx=%ld ldq=%ld", (long long)N,
                (long long)M, D, ldx, ldq);
    DIC_REQUIRE(k >= 1 && k <= N, DIC_ERR_INVALID_ARG, "knn_neighbors: k=%d: expected 1 <= k <= N=%lld", k, (long long)N);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0 && ldq % 4 == 0, DIC_ERR_UNSUPPORTED, "knn_neighbors: D=%d (row strides %ld, %ld): at most %d, multiples of 4",
                D, ldx, ldq, PT_D);
    DIC_REQUIRE(k <= KN_MAXK, DIC_ERR_UNSUPPORTED, "knn_neighbors: k=%d: at most %d neighbours", k, KN_MAXK);
    DIC_REQUIRE(N + M < (1LL << 30), DIC_ERR_UNSUPPORTED, "knn_neighbors: N+M=%lld: fewer than 2^30 points", (long long)(N + M));
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                    ((uintptr_t)dist & 7) == 0 && ((uintptr_t)idx & 3) == 0,
                DIC_ERR_UNSUPPORTED, "knn_neighbors: operands must be 16-B aligned");
    const int64_t P = N + M;          // the stacked set
    const KnLayout o = kn_layout(P, candidate_budget);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "knn_neighbors: workspace %zu < %zu", workspace_bytes, o.total);
    int rc = kn_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const PtLayout pl = pt_layout(P);
    KnTileArgs t{};
    pt_fill_pair_args(t.p, ws, P);
    const int nblk = t.p.nblk;                                    // row blocks of the stacked set
    rc = knl_prepare_planes(X, ldx, N, Q, ldq, M, centre, D, ws, st);
    if (rc) return rc;
    const int first = (int)(M > 0 ? N : 0), nq = (int)(P - first);          // the query rows [first, P)
    const int b0 = first / PT_T, rb = b0 * PT_T, nr = (int)(P - rb);      // the rows of the walked blocks [rb, P): all of them get a bracket
    t.p.nblk = (int)((N + PT_T - 1) / PT_T);                             // column blocks holding an index point
    t.p.tile0 = (long long)b0 * t.p.nblk;
    t.p.ntiles = (long long)(nblk - b0) * t.p.nblk;
    float* thr = (float*)(ws + o.thr);
    int32_t* cnt = (int32_t*)(ws + o.cnt);
    float* lo = (float*)(ws + o.lo);
    float* hi = (float*)(ws + o.hi);
    float* bnd = (float*)(ws + o.bnd);
    long long* off = (long long*)(ws + o.off);
    int32_t* cursor = (int32_t*)(ws + o.cursor);
    int32_t* bounds = (int32_t*)(ws + o.bounds);
    KnPlan* plan = (KnPlan*)(ws + o.plan);
    float* gmax = (float*)(ws + pl.count);
    t.thr = thr; t.cnt = cnt; t.off = off; t.cursor = cursor; t.idx = (int32_t*)(ws + o.idx); t.entries = o.entries;
    const dim3 rows((unsigned)((nr + 255) / 256)), tgrid(pt_grid(t.p.ntiles)), tblk(512);
    // the padding rows' thresholds and window are read (and masked): defined values
    hipError_t e = hipMemsetAsync(thr + (size_t)P * KN_T, 0, (size_t)PT_T * KN_T * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, (size_t)P * sizeof(int32_t), st);
    // the refining passes zero the counts of the walked rows at stride KN_T, [KN_T rb, KN_T P); the last pass counts at stride 2, [2 rb, 2 P), which lies
    // below that range when the walk does not start at row 0: zero all of it
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)P * KN_T * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kn_gmax_kernel, dim3(1), dim3(256), 0, st, t.p.bmax, nblk, gmax);
    hipLaunchKernelGGL(kn_init_kernel, rows, dim3(256), 0, st, t.p.nrm + rb, (const float*)gmax, nr, lo + rb, hi + rb, bnd + rb, thr + (size_t)rb * KN_T,
                       cnt + (size_t)rb * KN_T);
    for (int p = 0; p < KN_REFINE; ++p) {
        hipLaunchKernelGGL((kn_count_kernel<KN_T>), tgrid, tblk, PT_LDS, st, t);
        hipLaunchKernelGGL(kn_bracket_kernel, rows, dim3(256), 0, st, nr, k, lo + rb, hi + rb, thr + (size_t)rb * KN_T, cnt + (size_t)rb * KN_T);
    }
    hipLaunchKernelGGL(knl_window_kernel, rows, dim3(256), 0, st, nr, (const float*)(hi + rb), (const float*)(bnd + rb), thr + (size_t)rb * 2);
    hipLaunchKernelGGL((kn_count_kernel<2>), tgrid, tblk, PT_LDS, st, t);
    hipLaunchKernelGGL(kn_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)(cnt + (size_t)first * 2), nq, off + first, plan);
    rc = check_launch("knn_neighbors counting");
    if (rc) return rc;
    // the list lengths decide the groups: read their summary back (synchronises the stream)
    KnPlan hp;
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: reading the list lengths: %s", hipGetErrorString(e));
    if (stats) {
        stats[0] = KN_REFINE + 1;
        stats[1] = 0;
        stats[2] = hp.longest;
        stats[3] = hp.total;
        stats[4] = hp.longest * KN_ENTRY;
    }
    DIC_REQUIRE(hp.longest <= o.entries, DIC_ERR_WORKSPACE, "knn_neighbors: a row's list has %lld entries (%lld bytes), candidate_budget holds %lld (%lld "
                "bytes): run again with candidate_budget >= %lld", hp.longest, hp.longest * KN_ENTRY, o.entries, o.entries * KN_ENTRY, hp.longest * KN_ENTRY);
    hipLaunchKernelGGL(kn_groups_kernel, dim3(1), dim3(64), 0, st, (const long long*)(off + first), nq, o.entries, bounds, plan);
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: reading the groups: %s", hipGetErrorString(e));
    if (stats) stats[1] = hp.groups;
    constexpr int CHUNK = 1024;          // group bounds (relative to the first query row) come back this many at a time
    int32_t hb[CHUNK + 1];
    for (long long g0 = 0; g0 < hp.groups; g0 += CHUNK) {
        const int ng = (int)min((long long)CHUNK, hp.groups - g0);
        e = hipMemcpyAsync(hb, bounds + g0, (size_t)(ng + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: reading the groups: %s", hipGetErrorString(e));
        for (int g = 0; g < ng; ++g) {
            DIC_REQUIRE(hb[g] >= 0 && hb[g] < hb[g + 1] && hb[g + 1] <= nq, DIC_ERR_LAUNCH, "knn_neighbors: group %lld = queries [%d, %d)", g0 + g, hb[g], hb[g + 1]);
            const int r0 = first + hb[g], r1 = first + hb[g + 1];
            const int g0b = r0 / PT_T, g1b = (r1 + PT_T - 1) / PT_T;
            t.r0 = r0; t.r1 = r1;
            t.p.tile0 = (long long)g0b * t.p.nblk;
            t.p.ntiles = (long long)(g1b - g0b) * t.p.nblk;
            hipLaunchKernelGGL(kn_gather_kernel, dim3(pt_grid(t.p.ntiles)), tblk, PT_LDS, st, t);
            hipLaunchKernelGGL(knl_exact_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, st, X, ldx, Q, ldq, D, (int)N, first, r0, k, (const int32_t*)cnt,
                               (const long long*)off, (const int32_t*)t.idx, (double*)(ws + o.d2), o.entries, dist, idx, plan);
        }
        rc = check_launch("knn_neighbors gather");
        if (rc) return rc;
    }
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "knn_neighbors: %s", hipGetErrorString(e));
    DIC_REQUIRE(hp.flag == 0, DIC_ERR_LAUNCH, "knn_neighbors: a row's list was shorter than k or incomplete (non-finite coordinates?)");
    return DIC_OK;
}

}  // extern "C"
