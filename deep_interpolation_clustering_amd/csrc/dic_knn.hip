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
// (3) GATHER + EXACT, over groups of rows sized by the candidate budget (dic_candlist.h has the protocol, what the budget can change and the guards): the
//     list lengths are the counts of (2); the gather pass appends every candidate j to row i's list; the exact kernel computes the f64 difference-form d^2
//     of every list entry (each term exact, summed in a fixed order) and selects rank k - c_i by a radix select over the bit patterns of the (non-negative)
//     doubles: the value AT the rank, ties or not.  The approximate products never decide the rank and never supply the value.
// No workgroup waits for another inside a kernel; the only atomics are integer adds (counts, list cursors).  Two calls give the same bits.
#include "dic_exactd2.h"
#include "dic_candlist.h"          // KnTileArgs, KnCount and the list protocol, shared with dic_knn_rank.hip
#include "dic_pairtile.h"

namespace dic {

constexpr int KN_T = 16;                               // thresholds per row and refining pass
constexpr int KN_REFINE = 3;                           // refining passes
constexpr int KN_ENTRY = 12;                           // bytes of candidate storage per list entry: int32 index + f64 d^2

struct KnLayout { size_t thr, cnt, lo, hi, bnd, off, cursor, bounds, plan, idx, d2, total; long long entries; };

static long long kn_entries(int64_t N, int64_t budget) {
    if (budget <= 0) budget = CL_DEFAULT_BUDGET;
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

// The window (wlo, whi] of every row, at stride 2 (a launch of its own: it overwrites the refining thresholds of other rows).  The k-th distance takes the
// candidates around the bracket, wlo = lo - 2.01 B; a neighbour LIST takes everything up to whi (wlo = -inf: c_i = 0).
template <bool LISTS>
__global__ __launch_bounds__(256) void kn_window_kernel(int n, const float* lo, const float* hi, const float* bnd, float* thr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float m = 2.01f * bnd[i];
    thr[(size_t)i * 2] = LISTS ? -__builtin_inff() : lo[i] - m;
    thr[(size_t)i * 2 + 1] = hi[i] + m;
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

// What both exact kernels open with: d2[o + e] = the exact d^2 of xi and list entry e, e < len (one wave per entry: dic_exactd2.h -- lane l holds coordinates
// 4 l .. 4 l + 3, f64 difference form, fixed summation order; dic_optics.hip computes its distances with the same function).  A slot the gather pass did not
// fill (it fills every one) is reported and read as point `stand_in`, to stay inside X.
__device__ __forceinline__ void kn_list_d2(const float* X, long ldx, int d, int n, const ed_f32x4 xi, int stand_in, const int32_t* idx, double* d2, long long o,
                                           int len, ClPlan* plan) {
    const int lane = threadIdx.x & 63;
    for (int e = threadIdx.x >> 6; e < len; e += 4) {
        int j = idx[o + e];
        if ((unsigned)j >= (unsigned)n) {
            if (lane == 0) plan->flag = 1;
            j = stand_in;
        }
        const double s = exact_d2(xi, exact_d2_load(X, ldx, (size_t)j, d));
        if (lane == 0) d2[o + e] = s;
    }
}

// One workgroup per row of the group: the exact d^2 of every list entry, then the value at rank k - c_i by a radix select over the doubles' bit patterns
// (non-negative: unsigned order = numeric order), eight 8-bit digits from the top.  kth[i] = its square root.  plan->flag is set if a row's rank falls
// outside its list or a list slot holds no point (the invariants say neither can happen).
__global__ __launch_bounds__(256) void kn_exact_kernel(const float* X, long ldx, int d, int n, int r0, int k, const int32_t* cnt, const long long* off,
                                                       const int32_t* idx, double* d2, long long entries, double* kth, ClPlan* plan) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel_prefix;
    __shared__ int sel_rank;
    const int i = r0 + blockIdx.x, tid = threadIdx.x;
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
    kn_list_d2(X, ldx, d, n, exact_d2_load(X, ldx, (size_t)i, d), i, idx, d2, o, len, plan);
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

// One workgroup per row r0 + blockIdx.x of the stacked set (row `first` = query 0 = output row 0).  plan->flag is set if a list is shorter than k, a slot
// holds no index point or the select does not leave exactly k entries (the invariants say none can happen); the row is then NaN / -1.
__global__ __launch_bounds__(256) void knl_exact_kernel(const float* X, long ldx, const float* Q, long ldq, int d, int n, int first, int r0, int k,
                                                        const int32_t* cnt, const long long* off, const int32_t* idx, double* d2, long long entries,
                                                        double* dist, int32_t* nbr, ClPlan* plan) {
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
    kn_list_d2(X, ldx, d, n, Q ? exact_d2_load(Q, ldq, (size_t)(i - first), d) : exact_d2_load(X, ldx, (size_t)i, d), 0, idx, d2, o, len, plan);
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
    hipLaunchKernelGGL(pt_mask_cols_kernel, dim3((unsigned)((M + PT_T + 255) / 256)), dim3(256), 0, st, pb, (long long)N, (long long)(M + PT_T), PT_PAD_NORM);
    hipLaunchKernelGGL(pt_block_max_kernel, dim3((unsigned)((P + PT_T - 1) / PT_T)), dim3(256), 0, st, (const float*)nrm, (int)P, (float*)(ws + o.bmax));
    return DIC_OK;
}

static int kn_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)kn_count_kernel<KN_T>, (const void*)kn_count_kernel<2>, (const void*)kn_gather_kernel}, "knn");
}

// Everything behind the planes, for both entry points, on the P rows of a kn_layout(P) workspace whose planes are filled and whose t.p walks the tiles to
// count: the brackets (1) of the walked rows [rb, P) (whole row blocks), the window (2) of the kind LISTS, and (3) for the listed rows [first, P), rb <=
// first, with the caller's exact kernel enqueued by exact(r0, r1) behind each group's gather pass.  The k-th distance is rb = first = 0.
template <bool LISTS, class Exact>
static int kn_select(KnTileArgs& t, unsigned char* ws, const KnLayout& o, int64_t P, int rb, int first, int k, int64_t* stats, hipStream_t st,
                     const ClNames& nm, Exact&& exact) {
    const int nr = (int)(P - rb), nq = (int)(P - first);
    float* thr = (float*)(ws + o.thr);
    int32_t* cnt = (int32_t*)(ws + o.cnt);
    float* lo = (float*)(ws + o.lo) + rb;
    float* hi = (float*)(ws + o.hi) + rb;
    float* bnd = (float*)(ws + o.bnd) + rb;
    long long* off = (long long*)(ws + o.off);
    int32_t* cursor = (int32_t*)(ws + o.cursor);
    ClPlan* plan = (ClPlan*)(ws + o.plan);
    float* gmax = (float*)(ws + pt_layout(P).count);
    t.thr = thr; t.cnt = cnt; t.off = off; t.cursor = cursor; t.idx = (int32_t*)(ws + o.idx); t.entries = o.entries;
    const dim3 rows((unsigned)((nr + 255) / 256)), tgrid(pt_grid(t.p.ntiles)), tblk(512);
    // the padding rows' thresholds and window are read (and masked): defined values
    hipError_t e = hipMemsetAsync(thr + (size_t)P * KN_T, 0, (size_t)PT_T * KN_T * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, (size_t)P * sizeof(int32_t), st);
    // the refining passes zero the counts of the walked rows at stride KN_T, [KN_T rb, KN_T P); the last pass counts at stride 2, [2 rb, 2 P), which lies
    // below that range when the walk does not start at row 0: zero all of it
    if (e == hipSuccess && rb > 0) e = hipMemsetAsync(cnt, 0, (size_t)P * KN_T * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: memset: %s", nm.who, hipGetErrorString(e));
    hipLaunchKernelGGL(cl_gmax_kernel, dim3(1), dim3(256), 0, st, t.p.bmax, (int)((P + PT_T - 1) / PT_T), gmax);
    hipLaunchKernelGGL(kn_init_kernel, rows, dim3(256), 0, st, t.p.nrm + rb, (const float*)gmax, nr, lo, hi, bnd, thr + (size_t)rb * KN_T, cnt + (size_t)rb * KN_T);
    for (int p = 0; p < KN_REFINE; ++p) {
        hipLaunchKernelGGL((kn_count_kernel<KN_T>), tgrid, tblk, PT_LDS, st, t);
        hipLaunchKernelGGL(kn_bracket_kernel, rows, dim3(256), 0, st, nr, k, lo, hi, thr + (size_t)rb * KN_T, cnt + (size_t)rb * KN_T);
    }
    hipLaunchKernelGGL((kn_window_kernel<LISTS>), rows, dim3(256), 0, st, nr, (const float*)lo, (const float*)hi, (const float*)bnd, thr + (size_t)rb * 2);
    hipLaunchKernelGGL((kn_count_kernel<2>), tgrid, tblk, PT_LDS, st, t);
    hipLaunchKernelGGL((cl_scan_kernel<ClWindowLen>), dim3(1), dim3(1024), 0, st, ClWindowLen{cnt + (size_t)first * 2}, nq, off + first, plan);
    return cl_run_groups(plan, off, (int32_t*)(ws + o.bounds), nq, first, o.entries, KN_ENTRY, stats, KN_REFINE + 1, st, nm, [&](int r0, int r1) {
        t.r0 = r0; t.r1 = r1;
        cl_walk_rows(t.p, r0, r1);
        hipLaunchKernelGGL(kn_gather_kernel, dim3(pt_grid(t.p.ntiles)), tblk, PT_LDS, st, t);
        exact(r0, r1);
    });
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
    const ClNames nm{"knn_kth_distance", "a row has", "candidates", "a row's rank fell outside its candidate list or a list was incomplete"};
    return kn_select<false>(t, ws, o, N, 0, 0, (int)k, stats, st, nm, [&](int r0, int r1) {
        hipLaunchKernelGGL(kn_exact_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, st, X, ldx, D, (int)N, r0, (int)k, (const int32_t*)t.cnt, t.off,
                           (const int32_t*)t.idx, (double*)(ws + o.d2), o.entries, kth, (ClPlan*)(ws + o.plan));
    });
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
    rc = knl_prepare_planes(X, ldx, N, Q, ldq, M, centre, D, ws, st);
    if (rc) return rc;
    KnTileArgs t{};
    pt_fill_pair_args(t.p, ws, P);
    const int first = (int)(M > 0 ? N : 0), rb = first / PT_T * PT_T;          // the query rows [first, P); the rows of their blocks [rb, P) all get a bracket
    t.p.nblk = (int)((N + PT_T - 1) / PT_T);                                  // column blocks holding an index point
    cl_walk_rows(t.p, rb, (int)P);
    const ClNames nm{"knn_neighbors", "a row's list has", "entries", "a row's list was shorter than k or incomplete"};
    return kn_select<true>(t, ws, o, P, rb, first, k, stats, st, nm, [&](int r0, int r1) {
        hipLaunchKernelGGL(knl_exact_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, st, X, ldx, Q, ldq, D, (int)N, first, r0, k, (const int32_t*)t.cnt, t.off,
                           (const int32_t*)t.idx, (double*)(ws + o.d2), o.entries, dist, idx, (ClPlan*)(ws + o.plan));
    });
}

}  // extern "C"

