// Mean shift with the flat kernel (sklearn 1.7.2 cluster/_mean_shift.py) on the matrix cores; the definition is stated once, in include/dic_hip.h.
// sklearn issues one ball-tree radius query per seed per iteration; here ALL seeds advance together, and one iteration is two kernels:
//
// MEMBERS (ms_members_kernel): which points lie within the bandwidth of which seed, m(s) = { j : d2(s, j) <= t }, t = h^2.  One pair pass of dic_pairtile.h
//   over (seed row blocks) x (point column blocks).  The points' planes are prepared once per fit (pt_prep_kernel, centred on the f32 centre); the current
//   seeds are stacked BEHIND them, from row S0 = the point count rounded up to a whole 256-row block, as the row operand only: seeds never act as columns (the
//   column blocks walked are the S0 / 256 blocks of the points, and rows N .. S0 - 1 present PT_PAD_NORM as operand j, like every padding point: neither a
//   member nor a band pair).  Seeds move, so ms_seed_prep_kernel rewrites their rows of pa and their norms before every pass.
//   ERROR BOUND with f64 seeds.  dic_pairtile.h's B0 = 2^-12 (n_i + nmax_J) rests on four items; (2)-(4) speak of the f32 vector v alone and hold for any
//   f32 v.  Item (1) needs every coordinate of v to be ONE rounding away from the exact centred coordinate: |v_k - (s_k - c_k)| <= u |v_k|, u = 2^-24.  A
//   point's v = fl32(x - c) is that by construction.  A seed's is v = (float)(s - (double)c): the f64 subtraction is off by 2^-53 relative, the conversion is
//   the one f32 rounding, together (1 + 2^-29) u -- inside the slack of the bound (0.74 of 2^-12 used).  Forming s - c in f32 from a seed rounded to f32 first
//   would be two roundings, the first relative to |s| and not to |s - c|: that is what the f64 prep avoids.  So every pair has |a - d2| < B0, and a lane decides
//   it in the tile when  y = fl(a + B0) <= tl = t (1 - 2^-20)  (a member) or  z = fl(a - B0) > th = t (1 + 2^-20)  (not one), dic_dbscan.hip's margins in
//   f32 around (float)t; every other pair, a BAND pair, goes to a list (DBSCAN's capacity protocol) and ms_recheck_kernel decides it with the exact d2.
//   Certain members are bits of mask (M, ceil(N / 32)) uint32: a lane holds 16 of the 32 columns of a word, ORs its half with the other half's
//   (__shfl_xor 32) and one lane stores the word -- every word of every seed row is stored exactly once, no atomics in the tile loop; the band pairs then set
//   their bits with integer atomicOr.  The mask is a fixed function of the inputs.
//
// SHIFT (ms_shift_kernel): per seed, count = popcount of its mask row and sum_j mask[s, j] x'_j, x' = (double)x - c: a 0/1 (M x N) by f64 (N x D) product on
//   the f64 matrix cores, v_mfma_f64_16x16x4_f64.  A wave owns 16 seeds and up to 64 coordinates (1 or 4 accumulator tiles of 16 seeds x 16 coordinates);
//   beyond 64 coordinates the four waves of a workgroup share one seed group and take 64 coordinates each.  A k step is 4 points: A = the 4 mask bits of the
//   16 seeds as 0.0 / 1.0 (lane l: seed l & 15, point l >> 4), B = x' of the 4 points (lane l: point l >> 4, coordinate l & 15 of each tile), C/D: lane l
//   holds coordinate l & 15 of seeds (l >> 4) + 4 reg.  Points in ascending order; a 32-point word (or a 4-point step) none of the 16 seeds has a member in
//   is skipped, which adds exact zeros less and changes no bit.  No floating-point atomics: two calls give the same bits.  The epilogue applies the rule of
//   the definition on the device: new seed, moved (the waves' parts of its square added in slice order through LDS), done flag, iteration count.
//
// NEAREST (ms_nearest_kernel): nearest of C f64 centres for f32 or f64 rows by the exact d2, one wave per row: labels_, predict, and one step of the
//   suppression walk (C = 1, rows = the sorted centres).
//
// The exact d2 has dic_exactd2.h's lane order -- lane l holds coordinates 4 l .. 4 l + 3, an fma chain over them, then wave_sum -- with the f64 operand
// (seed or centre) first: t = s_k - (double)x_k.
#include <type_traits>
#include "dic_pairtile.h"
#include "dic_exactd2.h"

namespace dic {

typedef double ms_f64x4 __attribute__((ext_vector_type(4)));

constexpr double MS_MAX_BANDWIDTH = 0x1p50;             // t = h^2 < 2^100 stays below PT_PAD_NORM, as DB_MAX_THRESHOLD
constexpr double MS_STOP = 1e-3;                        // sklearn: stop_thresh = 1e-3 * bandwidth

struct MsTileArgs {
    PtPairArgs p;
    int s0, m, n_words;                                 // first seed row of the stacked set, seeds, mask words per seed
    float tl, th;
    uint32_t* mask; pi32x4* band; long long cap; unsigned long long* band_count;
};

struct MsLayout { int64_t s0, rows; PtLayout pt; };

inline MsLayout ms_layout(int64_t N, int64_t M_max) {
    MsLayout o;
    o.s0 = (N + PT_T - 1) / PT_T * PT_T;
    o.rows = o.s0 + M_max;
    o.pt = pt_layout(o.rows);
    return o;
}

// this lane's four coordinates of an f64 row (zeros beyond d)
__device__ __forceinline__ ms_f64x4 ms_load_f64(const double* R, long ldr, size_t row, int d) {
    const int col = 4 * lane_id();
    ms_f64x4 v = {0.0, 0.0, 0.0, 0.0};
    if (col < d) {
        const double* p = R + row * (size_t)ldr + col;
        v = ms_f64x4{p[0], p[1], p[2], p[3]};
    }
    return v;
}
__device__ __forceinline__ ms_f64x4 ms_load_f32(const float* X, long ldx, size_t row, int d) {
    const ed_f32x4 x = exact_d2_load(X, ldx, row, d);
    return ms_f64x4{(double)x[0], (double)x[1], (double)x[2], (double)x[3]};
}
__device__ __forceinline__ double ms_d2(const ms_f64x4 s, const ms_f64x4 x) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double t = s[q] - x[q];
        acc = fma(t, t, acc);
    }
    return wave_sum(acc);
}

// pt_prep_kernel's row operand for f64 seeds: v = (float)(s - centre), the difference in f64, ONE rounding per coordinate.  One wave per seed.
__global__ __launch_bounds__(256) void ms_seed_prep_kernel(const double* S, long lds, const float* mu, int m, int d, __bf16* pa, long plane, float* nrm_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int col = 4 * lane;
    pf32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col < d) {
        const double* s = S + (size_t)row * lds + col;
        const pf32x4 c = *reinterpret_cast<const pf32x4*>(mu + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)(s[e] - (double)c[e]);
    }
    float nrm = fmaf(v[0], v[0], fmaf(v[1], v[1], fmaf(v[2], v[2], v[3] * v[3])));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) nrm += __shfl_xor(nrm, o);
    pbf16x4 ah, al;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 h = (__bf16)v[e];
        ah[e] = h;
        al[e] = (__bf16)(v[e] - (float)h);
    }
    const size_t at = (size_t)row * PT_LD + col;
    *reinterpret_cast<pbf16x4*>(pa + at) = ah;
    *reinterpret_cast<pbf16x4*>(pa + plane + at) = al;
    if (lane < 8) {                                     // columns 256 + 4 lane ..: [n n n 1 | 1 1 0 0 | 0 ..] (pt_prep_kernel's operand i)
        const __bf16 n0 = (__bf16)nrm;
        const float r1 = nrm - (float)n0;
        const __bf16 n1 = (__bf16)r1;
        const __bf16 n2 = (__bf16)(r1 - (float)n1);
        const __bf16 one = (__bf16)1.f, z = (__bf16)0.f;
        pbf16x4 ea = {z, z, z, z};
        if (lane == 0) ea = pbf16x4{n0, n1, n2, one};
        if (lane == 1) ea = pbf16x4{one, one, z, z};
        const size_t et = (size_t)row * PT_LD + PT_D + 4 * lane;
        *reinterpret_cast<pbf16x4*>(pa + et) = ea;
        *reinterpret_cast<pbf16x4*>(pa + plane + et) = pbf16x4{z, z, z, z};
    }
    if (lane == 0) nrm_out[row] = nrm;
}

// Members epilogue: mask words of the certain members + the band list.
struct MsMembers {
    const MsTileArgs& a;
    const PtLane ln;

    __device__ __forceinline__ MsMembers(const MsTileArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        const float bm = a.p.bmax[J0 / PT_T];
        const int w0 = (J0 + 128 * ln.wn) >> 5;          // mask word of this wave's columns at nb = 0
        auto rows = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
            const int row = ln.row(I0, mb);
            const int gi = row - a.s0;                    // seed (rows past the last seed: stale or zero planes, never stored)
            const bool iv = gi < a.m;
            const float b0 = (a.p.nrm[row] + bm) * 0x1p-12f;
            const float tl = a.tl, th = a.th;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                unsigned word = 0u, bword = 0u;          // bit (k & 3) + 8 (k >> 2) = the column's offset in the lane's half (immediates; the half shifts the word)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float d2 = acc[nb][mb][k];          // (a padding column: PT_PAD_NORM, above tl and th)
                    const bool mem = d2 + b0 <= tl;
                    word |= mem ? (1u << ((k & 3) + 8 * (k >> 2))) : 0u;
                    bword |= (!mem & (d2 - b0 <= th)) ? (1u << ((k & 3) + 8 * (k >> 2))) : 0u;
                }
                word <<= 4 * ln.hh;
                word |= __shfl_xor(word, 32);
                if (ln.hh == 0 && iv && w0 + nb < a.n_words) a.mask[(size_t)gi * a.n_words + w0 + nb] = word;
                if (iv && bword) {                             // band pairs: rare
                    unsigned long long at = atomicAdd(a.band_count, (unsigned long long)__builtin_popcount(bword));
                    while (bword) {
                        const int p = __builtin_ctz(bword);
                        bword &= bword - 1;
                        if (at < (unsigned long long)a.cap) {
                            pi32x4 ent;
                            ent[0] = gi; ent[1] = 32 * (w0 + nb) + 4 * ln.hh + p; ent[2] = 0; ent[3] = 0;
                            a.band[at] = ent;
                        }
                        ++at;
                    }
                }
            }
        };
        rows(std::integral_constant<int, 0>{});
        rows(std::integral_constant<int, 1>{});
    }
};

__global__ __launch_bounds__(512, 1) void ms_members_kernel(MsTileArgs a) {
    MsMembers epi(a);
    pt_pair_pass(a.p, epi);
}

// Band pairs, exactly: one wave per entry (seed, point); a member sets its bit.
__global__ __launch_bounds__(256) void ms_recheck_kernel(const float* X, long ldx, int d, const double* S, long lds, const pi32x4* band, long long nband, double t,
                                                         uint32_t* mask, int n_words) {
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= nband) return;
    const pi32x4 ent = band[idx];
    const double d2 = ms_d2(ms_load_f64(S, lds, (size_t)ent[0], d), ms_load_f32(X, ldx, (size_t)ent[1], d));
    if (lane_id() == 0 && d2 <= t) atomicOr(mask + (size_t)ent[0] * n_words + (ent[1] >> 5), 1u << (ent[1] & 31));
}

// One wave per 16 seeds and NCB accumulator tiles of 16 coordinates; the SLICES waves of a seed group (1 or all 4 of the workgroup) take 16 NCB coordinates
// each (16 NCB SLICES >= d) and add their parts of moved^2 through LDS in slice order.  Narrow accumulators leave room for several waves per SIMD: the loads
// of one wave run under the MFMAs of the others.
template <int NCB, int SLICES>
__global__ __launch_bounds__(256) void ms_shift_kernel(const float* X, long ldx, int n, int d, const double* c, const uint32_t* mask, int n_words, int m, double* S,
                                                       long lds, double stop, int max_iter, int32_t* counts, int32_t* iters, int32_t* done, double* sums) {
    __shared__ double part[SLICES][16];
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s0 = ((blockIdx.x * 4 + wv) / SLICES) * 16;          // (SLICES = 4: the workgroup's one seed group, so its waves leave or stay together)
    const int c0 = (wv % SLICES) * (16 * NCB);
    if (s0 >= m) return;
    const uint32_t* mrow = mask + (size_t)min(s0 + r, m - 1) * n_words;
    double cc[NCB];
    ms_f64x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        cc[cb] = c0 + 16 * cb + r < d ? c[c0 + 16 * cb + r] : 0.0;
        acc[cb] = ms_f64x4{0.0, 0.0, 0.0, 0.0};
    }
    int cnt = 0;
    uint32_t next = mrow[0];
    for (int w = 0; w < n_words; ++w) {
        const uint32_t word = next;
        if (w + 1 < n_words) next = mrow[w + 1];
        cnt += __builtin_popcount(word);
        if (c0 >= d || __ballot(word != 0u) == 0ull) continue;          // (a slice past the last coordinate only counts)
#pragma unroll 2
        for (int ks = 0; ks < 8; ++ks) {
            const uint32_t nib = (word >> (4 * ks)) & 15u;
            if (__ballot(nib != 0u) == 0ull) continue;
            const int j = min(32 * w + 4 * ks + g, n - 1);          // (a bit past the last point is 0: its row only has to be readable)
            const float* xr = X + (size_t)j * ldx + c0 + r;
            const double av = (nib >> g) & 1u ? 1.0 : 0.0;
            float xv[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) xv[cb] = c0 + 16 * cb + r < d ? xr[16 * cb] : 0.f;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, (double)xv[cb] - cc[cb], acc[cb], 0, 0, 0);
        }
    }
    double mv[4];
    int cn[4];
    bool live[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = g + 4 * reg, si = s0 + row;
        cn[reg] = __shfl(cnt, row);                           // (lane `row` has r = row: the count of seed s0 + row)
        live[reg] = si < m && done[min(si, m - 1)] == 0;
        mv[reg] = 0.0;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int col = c0 + 16 * cb + r;
            if (live[reg] && col < d) {
                const double sum = acc[cb][reg];
                if (sums) sums[(size_t)si * d + col] = sum;
                if (cn[reg] > 0) {
                    double* sp = S + (size_t)si * lds + col;
                    const double snew = cc[cb] + sum / (double)cn[reg];
                    const double df = snew - *sp;
                    mv[reg] = fma(df, df, mv[reg]);
                    *sp = snew;
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mv[reg] += __shfl_xor(mv[reg], o);
    }
    if constexpr (SLICES > 1) {                              // moved^2 of the seed group: the slices' parts, added in slice order
        // (the done flags were read above and are written below: the barrier also keeps a slice from reading what slice 0 has written)
        if (r == 0)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) part[wv % SLICES][g + 4 * reg] = mv[reg];
        __syncthreads();
        if (wv % SLICES != 0) return;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            double t = part[0][g + 4 * reg];
#pragma unroll
            for (int sl = 1; sl < SLICES; ++sl) t += part[sl][g + 4 * reg];
            mv[reg] = t;
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int si = s0 + g + 4 * reg;
        if (live[reg] && r == 0) {
            counts[si] = cn[reg];
            if (cn[reg] == 0) {
                done[si] = 1;
            } else {
                const int it = iters[si];
                if (sqrt(mv[reg]) <= stop || it >= max_iter) done[si] = 1;
                else iters[si] = it + 1;
            }
        }
    }
}

// One wave per row: the nearest of C centres by the exact d2, ties to the smaller index.
__global__ __launch_bounds__(256) void ms_nearest_kernel(const float* X, long ldx, const double* R, long ldr, long long n_rows, int d, const double* centres,
                                                         long ldc, int C, int32_t* idx, double* d2_out) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const ms_f64x4 x = X ? ms_load_f32(X, ldx, (size_t)row, d) : ms_load_f64(R, ldr, (size_t)row, d);
    double best = __builtin_inf();
    int bi = -1;
    for (int k = 0; k < C; ++k) {
        const double v = ms_d2(ms_load_f64(centres, ldc, (size_t)k, d), x);
        if (v < best) { best = v; bi = k; }
    }
    if (lane_id() == 0) {
        if (idx) idx[row] = bi;
        if (d2_out) d2_out[row] = best;
    }
}

static int ms_reserve_lds() {
    static bool done = false;
    return pt_reserve_lds(done, {(const void*)ms_members_kernel}, "meanshift");
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_meanshift_workspace(int64_t N, int64_t M_max) {
    if (N <= 0 || M_max <= 0 || N + M_max + PT_T >= (1LL << 30)) return 0;
    return ms_layout(N, M_max).pt.total;
}

int dic_meanshift_prepare(const float* X, long ldx, int64_t N, int D, const float* centre, int64_t M_max, void* workspace, size_t workspace_bytes,
                          dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && M_max > 0, DIC_ERR_INVALID_ARG, "meanshift_prepare: N=%lld D=%d ldx=%ld M_max=%lld", (long long)N, D, ldx,
                (long long)M_max);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "meanshift_prepare: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N + M_max + PT_T < (1LL << 30), DIC_ERR_UNSUPPORTED, "meanshift_prepare: N+M_max=%lld: fewer than 2^30 rows", (long long)(N + M_max));
    DIC_REQUIRE(X && centre && workspace, DIC_ERR_INVALID_ARG, "meanshift_prepare: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED,
                "meanshift_prepare: operands must be 16-B aligned");
    const MsLayout o = ms_layout(N, M_max);
    DIC_REQUIRE(workspace_bytes >= o.pt.total, DIC_ERR_WORKSPACE, "meanshift_prepare: workspace %zu < %zu", workspace_bytes, o.pt.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const long plane = (long)((o.rows + PT_T) * PT_LD);
    __bf16* pa = (__bf16*)(ws + o.pt.pa);
    __bf16* pb = (__bf16*)(ws + o.pt.pb);
    float* nrm = (float*)(ws + o.pt.nrm);
    // everything behind the points is zero: the rows up to S0, the seed rows until a seed is written there, the padding behind them
    const size_t tail = (size_t)(o.rows + PT_T - N) * PT_LD * sizeof(__bf16);
    hipError_t e = hipMemsetAsync(pa + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(pa + plane + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + plane + (size_t)N * PT_LD, 0, tail, st);
    if (e == hipSuccess) e = hipMemsetAsync(nrm + N, 0, (size_t)(o.rows + PT_T - N) * sizeof(float), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "meanshift_prepare: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, (int)N, D, pa, pb, plane, nrm);
    if (o.s0 > N)          // the rows between the last point and the first seed
        hipLaunchKernelGGL(pt_mask_cols_kernel, dim3((unsigned)((o.s0 - N + 255) / 256)), dim3(256), 0, st, pb, (long long)N, (long long)(o.s0 - N), PT_PAD_NORM);
    hipLaunchKernelGGL(pt_block_max_kernel, dim3((unsigned)(o.s0 / PT_T)), dim3(256), 0, st, (const float*)nrm, (int)N, (float*)(ws + o.pt.bmax));
    return check_launch("meanshift_prepare");
}

int dic_meanshift_members(const float* X, long ldx, int64_t N, int D, const float* centre, const double* seeds, int64_t M, int64_t M_max, double bandwidth,
                          uint32_t* mask, int32_t* band, int64_t capacity, int64_t* n_band, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && M > 0 && M <= M_max && capacity >= 0, DIC_ERR_INVALID_ARG,
                "meanshift_members: N=%lld D=%d ldx=%ld M=%lld M_max=%lld capacity=%lld", (long long)N, D, ldx, (long long)M, (long long)M_max, (long long)capacity);
    DIC_REQUIRE(bandwidth > 0.0, DIC_ERR_INVALID_ARG, "meanshift_members: bandwidth=%g: expected > 0", bandwidth);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "meanshift_members: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N + M_max + PT_T < (1LL << 30), DIC_ERR_UNSUPPORTED, "meanshift_members: N+M_max=%lld: fewer than 2^30 rows", (long long)(N + M_max));
    DIC_REQUIRE(bandwidth < MS_MAX_BANDWIDTH, DIC_ERR_UNSUPPORTED, "meanshift_members: bandwidth=%g: below 2^50", bandwidth);
    DIC_REQUIRE(X && centre && seeds && mask && n_band && workspace && (band || capacity == 0), DIC_ERR_INVALID_ARG, "meanshift_members: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0 &&
                    ((uintptr_t)seeds & 7) == 0 && ((uintptr_t)mask & 3) == 0,
                DIC_ERR_UNSUPPORTED, "meanshift_members: operands must be 16-B aligned");
    const MsLayout o = ms_layout(N, M_max);
    DIC_REQUIRE(workspace_bytes >= o.pt.total, DIC_ERR_WORKSPACE, "meanshift_members: workspace %zu < %zu", workspace_bytes, o.pt.total);
    int rc = ms_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    unsigned long long* cnt_dev = (unsigned long long*)(ws + o.pt.count);
    hipError_t e = hipMemsetAsync(cnt_dev, 0, sizeof(unsigned long long), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "meanshift_members: memset: %s", hipGetErrorString(e));
    MsTileArgs t{};
    pt_fill_pair_args(t.p, ws, o.rows);
    const long plane = t.p.plane;
    hipLaunchKernelGGL(ms_seed_prep_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, seeds, (long)D, centre, (int)M, D,
                       (__bf16*)(ws + o.pt.pa) + (size_t)o.s0 * PT_LD, plane, (float*)(ws + o.pt.nrm) + o.s0);
    t.p.n = (int)N;
    t.p.nblk = (int)(o.s0 / PT_T);                              // the column blocks: the points'
    t.p.tile0 = (long long)t.p.nblk * t.p.nblk;                 // from the first seed row block
    t.p.ntiles = (long long)((M + PT_T - 1) / PT_T) * t.p.nblk;
    t.s0 = (int)o.s0;
    t.m = (int)M;
    t.n_words = (int)((N + 31) / 32);
    const double tt = bandwidth * bandwidth;
    const float tf = (float)tt;
    t.tl = tf * (1.f - 0x1p-20f);
    t.th = tf * (1.f + 0x1p-20f);
    t.mask = mask;
    t.band = (pi32x4*)band;
    t.cap = capacity;
    t.band_count = cnt_dev;
    hipLaunchKernelGGL(ms_members_kernel, dim3(pt_grid(t.p.ntiles)), dim3(512), PT_LDS, st, t);
    rc = check_launch("meanshift_members");
    if (rc) return rc;
    unsigned long long nb = 0;
    e = hipMemcpyAsync(&nb, cnt_dev, sizeof(nb), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "meanshift_members: reading the band count: %s", hipGetErrorString(e));
    *n_band = (int64_t)nb;
    DIC_REQUIRE((int64_t)nb <= capacity, DIC_ERR_WORKSPACE, "meanshift_members: %llu band pairs, band list capacity %lld (mask incomplete: run again with "
                "capacity >= n_band)", nb, (long long)capacity);
    if (nb > 0)
        hipLaunchKernelGGL(ms_recheck_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, X, ldx, D, seeds, (long)D, (const pi32x4*)band, (long long)nb, tt,
                           mask, t.n_words);
    return check_launch("meanshift_members recheck");
}

int dic_meanshift_shift(const float* X, long ldx, int64_t N, int D, const double* shift, const uint32_t* mask, int64_t M, double* seeds, double bandwidth,
                        int max_iter, int32_t* counts, int32_t* iters, int32_t* done, double* sums, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && M > 0 && max_iter >= 0, DIC_ERR_INVALID_ARG, "meanshift_shift: N=%lld D=%d ldx=%ld M=%lld max_iter=%d", (long long)N,
                D, ldx, (long long)M, max_iter);
    DIC_REQUIRE(bandwidth > 0.0, DIC_ERR_INVALID_ARG, "meanshift_shift: bandwidth=%g: expected > 0", bandwidth);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "meanshift_shift: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N < (1LL << 30) && M < (1LL << 30), DIC_ERR_UNSUPPORTED, "meanshift_shift: N=%lld M=%lld: fewer than 2^30", (long long)N, (long long)M);
    DIC_REQUIRE(X && shift && mask && seeds && counts && iters && done, DIC_ERR_INVALID_ARG, "meanshift_shift: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)shift & 7) == 0 && ((uintptr_t)seeds & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)mask & 3) == 0,
                DIC_ERR_UNSUPPORTED, "meanshift_shift: operands must be aligned to their element size (X to 16 B)");
    hipStream_t st = (hipStream_t)stream;
    const int nw = (int)((N + 31) / 32);
    const double stop = MS_STOP * bandwidth;
#define MS_SHIFT(NCB, SLICES)                                                                                                                             \
    hipLaunchKernelGGL((ms_shift_kernel<NCB, SLICES>), dim3((unsigned)((M + 64 / SLICES - 1) / (64 / SLICES))), dim3(256), 0, st, X, ldx, (int)N, D, shift, mask, \
                       nw, (int)M, seeds, (long)D, stop, max_iter, counts, iters, done, sums)
    if (D <= 16) MS_SHIFT(1, 1);
    else if (D <= 64) MS_SHIFT(4, 1);
    else MS_SHIFT(4, 4);
#undef MS_SHIFT
    return check_launch("meanshift_shift");
}

int dic_meanshift_nearest(const float* X, long ldx, const double* R, int64_t n_rows, int D, const double* centres, int C, int32_t* idx, double* d2,
                          dic_stream_t stream) {
    DIC_REQUIRE(n_rows > 0 && D > 0 && C > 0, DIC_ERR_INVALID_ARG, "meanshift_nearest: n_rows=%lld D=%d C=%d", (long long)n_rows, D, C);
    DIC_REQUIRE((X != nullptr) != (R != nullptr), DIC_ERR_INVALID_ARG, "meanshift_nearest: exactly one of the f32 rows and the f64 rows");
    DIC_REQUIRE(!X || ldx >= D, DIC_ERR_INVALID_ARG, "meanshift_nearest: ldx=%ld < D=%d", ldx, D);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && (!X || ldx % 4 == 0), DIC_ERR_UNSUPPORTED, "meanshift_nearest: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx,
                PT_D);
    DIC_REQUIRE(n_rows < (1LL << 40), DIC_ERR_UNSUPPORTED, "meanshift_nearest: n_rows=%lld", (long long)n_rows);
    DIC_REQUIRE(centres && (idx || d2), DIC_ERR_INVALID_ARG, "meanshift_nearest: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)R & 7) == 0 && ((uintptr_t)centres & 7) == 0 && ((uintptr_t)d2 & 7) == 0 && ((uintptr_t)idx & 3) == 0,
                DIC_ERR_UNSUPPORTED, "meanshift_nearest: operands must be aligned to their element size (f32 rows to 16 B)");
    hipLaunchKernelGGL(ms_nearest_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, ldx, R, (long)D, (long long)n_rows, D, centres,
                       (long)D, C, idx, d2);
    return check_launch("meanshift_nearest");
}

}  // extern "C"
