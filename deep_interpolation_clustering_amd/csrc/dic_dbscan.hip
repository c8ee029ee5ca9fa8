// DBSCAN on the matrix cores (p2_clustering_optK.py:82-85,90-168, p4_clustering_final.py:181-236): upstream builds pairwise_distances(X) (N x N f32, 22.5 GB
// at 75 000 points) and runs DBSCAN(eps, min_samples, metric='precomputed') on it.  Here every pair pass recomputes the distances tile by tile, nothing N x N is
// ever stored.
//
// NEIGHBOUR RULE (sklearn's, bit for bit): (i, j) are neighbours for eps e iff f32(d^2_ij) <= t_e, where d^2 is the exact squared distance of the f32 points and
// t_e (f32) is the largest float s with np.sqrt(np.float32(s)) <= eps under NumPy's promotion of the caller's eps object (dbscan.py finds it on the host).  The
// self pair counts (d = 0).
//
// PAIR PASSES.  The machine of dic_intra.hip's intra_x3_kernel<ROWS>: one persistent 8-wave workgroup per CU walks a contiguous range of the (I, J) list of
// 256 x 256 point-pair tiles (ALL ordered block pairs, row-major), both operands' 32-column slabs streamed through LDS-DMA rings; d^2 = n_i + n_j - 2 v_i . v_j
// is one inner product of 288-column augmented rows, v = x - mean (f32), every coordinate as bf16 hi + lo with the products hi.hi + lo.hi + hi.lo, the f32 norms
// n = sum v^2 as three exact bf16 pieces.  Lane = point i, registers = points j: a lane's per-i results stay in registers while its workgroup's range stays on
// one row block I and are flushed (integer atomics: exact, order-free) when I changes.
//
// ERROR BOUND of the approximate d^2 (call it a_ij) against the exact d^2_ij of the f32 points, u = 2^-24:
//   (1) v = fl(x - mean): each coordinate of v_i - v_j is off by <= u (|v_ik| + |v_jk|), so |d_v^2 - d^2| <= 2u (|v_i| + |v_j|)^2 (1 + u) <= 4.1u (n_i + n_j).
//   (2) the split: h = bf16(v), |v - h| <= 2^-8 |v|; l = bf16(v - h) (v - h exact in f32), |v - h - l| <= 2^-16 |v|.  The dropped part of a product a.b is
//       l_a l_b + r_a b + (h_a + l_a) r_b, <= 3.1 * 2^-16 |a| |b|; b = -2 v_j splits exactly as -2 (h, l), so -2 v_i . v_j is off by
//       <= 6.2 * 2^-16 sum_k |v_ik| |v_jk| <= 3.1 * 2^-16 (n_i + n_j).
//   (3) f32 accumulation: 288 / 16 * 3 = 54 chained MFMAs of 16 exact products each, at most 54 * 16 = 864 roundings in sequence, each of
//       sum |terms| <= (n_i + n_j) + 2 * (1 + 2^-7) sum |v_ik v_jk| <= 2.02 (n_i + n_j):  <= 864 u * 2.02 (n_i + n_j) <= 2^-13.2 (n_i + n_j).
//   (4) the norms' own f32 rounding (4 fmas + 6 shuffle adds): <= 10u (n_i + n_j).
//   Together |a_ij - d^2_ij| < (0.11 + 0.19 + 0.43 + 0.01) 2^-12 (n_i + n_j) < B0 = 2^-12 (n_i + nmax_J), nmax_J the largest n of j's 256-row block.
// A lane forms y = fl(a + B0) and z = fl(a - B0) and decides the pair itself when
//   y <= tl_e = t_e (1 - 2^-20)   =>  d^2 <= a + B0 <= y (1 + u) < t_e               (a neighbour), or
//   z >  th_e = t_e (1 + 2^-20)   =>  d^2 >= a - B0 >= z (1 - u) > t_e + ulp(t_e)    (not one: its f32 rounding stays above t_e).
// The margin 2^-20 t_e also covers the difference between the exact d^2 and sklearn's f64 norm form (~2^-52 of |x_i|^2 + |x_j|^2), for points with
// |x|^2 < 2^30 t_e.  Every other pair (a BAND pair, in the band of some e) is appended to a device list and rechecked exactly: f64 difference form over the f32
// coordinates (each term exact, 256 of them summed in f64), rounded to f32, compared with every t_e.
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
#include "dic_common.h"

namespace dic {

typedef __bf16 dbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dbf16x4 __attribute__((ext_vector_type(4)));
typedef float df32x16 __attribute__((ext_vector_type(16)));
typedef float df32x4 __attribute__((ext_vector_type(4)));
typedef int di32x4 __attribute__((ext_vector_type(4)));

constexpr int DB_D = 256;                              // coordinates (narrower inputs are zero-padded by the caller to a multiple of 4)
constexpr int DB_LD = 288;                             // columns of an augmented row
constexpr int DB_T = 256;                              // points per tile edge
constexpr int DB_K = 32;                               // columns per slab
constexpr int DB_ROWB = DB_K * 2;                      // 64 B
constexpr int DB_PLANE = DB_T * DB_ROWB;               // 16 KB: one plane of a slab
constexpr int DB_SLOT = 2 * DB_PLANE;                  // 32 KB: hi | lo
constexpr int DB_SLABS = DB_LD / DB_K;                 // 9
constexpr int DB_NI = 3, DB_NJ = 2;                    // ring depths of the two operands
constexpr int DB_LDS = (DB_NI + DB_NJ) * DB_SLOT;      // 163 840 B
constexpr int DB_MAX_EPS = 16;
constexpr int DB_NONE = 0x7fffffff;
static_assert(DB_LDS <= 160 * 1024, "dbscan: LDS budget");

__device__ __forceinline__ void dbdma16(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// Augmented rows relative to one centre, and the f32 norms.  One wave per point: lane l holds coordinates 4 l .. 4 l + 3.
__global__ __launch_bounds__(256) void db_prep_kernel(const float* X, long ldx, const float* mu, int n, int d, __bf16* pa, __bf16* pb, long plane, float* nrm_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int col = 4 * lane;
    df32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col < d) {
        const df32x4 x = *reinterpret_cast<const df32x4*>(X + (size_t)row * ldx + col);
        const df32x4 m = *reinterpret_cast<const df32x4*>(mu + col);
        v = x - m;
    }
    float nrm = fmaf(v[0], v[0], fmaf(v[1], v[1], fmaf(v[2], v[2], v[3] * v[3])));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) nrm += __shfl_xor(nrm, o);
    dbf16x4 ah, al, bh, bl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 h = (__bf16)v[e];
        const __bf16 l = (__bf16)(v[e] - (float)h);
        ah[e] = h; al[e] = l;
        bh[e] = (__bf16)(-2.f * (float)h); bl[e] = (__bf16)(-2.f * (float)l);          // exact
    }
    const size_t at = (size_t)row * DB_LD + col;
    *reinterpret_cast<dbf16x4*>(pa + at) = ah;
    *reinterpret_cast<dbf16x4*>(pa + plane + at) = al;
    *reinterpret_cast<dbf16x4*>(pb + at) = bh;
    *reinterpret_cast<dbf16x4*>(pb + plane + at) = bl;
    if (lane < 8) {                                     // columns 256 + 4 lane ..: [n n n 1 | 1 1 0 0 | 0 ..] and [1 1 1 n | n n 0 0 | 0 ..]
        const __bf16 n0 = (__bf16)nrm;
        const float r1 = nrm - (float)n0;
        const __bf16 n1 = (__bf16)r1;
        const __bf16 n2 = (__bf16)(r1 - (float)n1);
        const __bf16 one = (__bf16)1.f, z = (__bf16)0.f;
        dbf16x4 ea = {z, z, z, z}, eb = {z, z, z, z};
        if (lane == 0) { ea = dbf16x4{n0, n1, n2, one}; eb = dbf16x4{one, one, one, n0}; }
        if (lane == 1) { ea = dbf16x4{one, one, z, z}; eb = dbf16x4{n1, n2, z, z}; }
        const size_t et = (size_t)row * DB_LD + DB_D + 4 * lane;
        const dbf16x4 zz = {z, z, z, z};
        *reinterpret_cast<dbf16x4*>(pa + et) = ea;
        *reinterpret_cast<dbf16x4*>(pa + plane + et) = zz;
        *reinterpret_cast<dbf16x4*>(pb + et) = eb;
        *reinterpret_cast<dbf16x4*>(pb + plane + et) = zz;
    }
    if (lane == 0) nrm_out[row] = nrm;
}

// largest norm of every 256-row block (norms are >= 0; rows past n count 0)
__global__ __launch_bounds__(256) void db_block_max_kernel(const float* nrm, int n, float* bmax) {
    __shared__ float part[4];
    const int i = blockIdx.x * DB_T + threadIdx.x;
    float v = i < n ? nrm[i] : 0.f;
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// ------------------------------------------------------------------------------------------------------------------------------------------
struct DbThresholds { float tl[DB_MAX_EPS], th[DB_MAX_EPS], t[DB_MAX_EPS]; };

struct DbTileArgs {
    const __bf16* pa; const __bf16* pb; long plane;
    const float* nrm; const float* bmax;
    int n, nblk; long long ntiles;
    DbThresholds thr; int n_eps;
    // counts
    int32_t* counts; di32x4* band; long long cap; unsigned long long* band_count;
    // components
    const int32_t* cnt_e; int min_samples; int32_t* L; int32_t* border; int32_t* changed;
};

// MODE 0: counts of every eps (NE thresholds, NE >= n_eps; unused ones never match) + the band list.  MODE 1: one label pass of eps 0 of thr.
template <int MODE, int NE>
__global__ __launch_bounds__(512, 1) void db_tile_kernel(DbTileArgs a) {
    extern __shared__ __align__(16) unsigned char dsm[];
    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l31 = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wm = w & 3, wn = w >> 2;
    const long long nch = gridDim.x;
    const long long per = (a.ntiles + nch - 1) / nch;
    const long long first = (long long)blockIdx.x * per;
    const long long my_tiles = max(0LL, min(per, a.ntiles - first));
    const long long S = my_tiles * DB_SLABS;
    if (S == 0) return;
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char*)dsm);
    const unsigned ldsI = lds0, ldsJ = lds0 + DB_NI * DB_SLOT;
    const unsigned v_dma = (unsigned)(lane >> 2) * (DB_LD * 2) + (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
    // tile t of the range: (first row of I, first row of J), row-major over the block pairs
    auto tile = [&](long long i) {
        const long long t = first + min(i, my_tiles - 1);
        const int bi = (int)(t / a.nblk), bj = (int)(t - (long long)bi * a.nblk);
        di32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane(bi * DB_T);
        r[1] = __builtin_amdgcn_readfirstlane(bj * DB_T);
        r[2] = 0; r[3] = 0;
        return r;
    };
    di32x4 e_cur = tile(0), e_nxt = tile(1), e_prev = e_cur;
    long long cur_tile = 0;
    auto issue = [&](const __bf16* mat, int row0, int ks, unsigned dst) {
        const __bf16* src = mat + (size_t)row0 * DB_LD + ks * DB_K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = w + 8 * j, pl = c >> 4, rg = c & 15;
            const uint64_t p = (uint64_t)(src + (size_t)pl * a.plane + (size_t)(16 * rg) * DB_LD);          // (uniform: keep the base in scalar registers)
            const uint64_t q = ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(p >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)p);
            dbdma16((const void*)q, v_dma, __builtin_amdgcn_readfirstlane(dst + pl * DB_PLANE + rg * 1024));
        }
    };
    auto issue_i = [&](long long s) { issue(a.pa, s / DB_SLABS == cur_tile ? e_cur[0] : e_nxt[0], (int)(s % DB_SLABS), ldsI + (int)(s % DB_NI) * DB_SLOT); };
    auto issue_j = [&](long long s) { issue(a.pb, s / DB_SLABS == cur_tile ? e_cur[1] : e_nxt[1], (int)(s % DB_SLABS), ldsJ + (int)(s % DB_NJ) * DB_SLOT); };
    const int sw = (l31 >> 2) & 3;
    int poff[DB_K / 16];
#pragma unroll
    for (int kk = 0; kk < DB_K / 16; ++kk) poff[kk] = ((2 * kk + hh) ^ sw) * 16;
    const int j_row = (128 * wn + l31) * DB_ROWB;
    const int i_row = (64 * wm + l31) * DB_ROWB;

#pragma unroll
    for (int it = 1 - DB_NI; it < 0; ++it) {
        if (it + DB_NJ - 1 >= 0 && it + DB_NJ - 1 < S) issue_j(it + DB_NJ - 1);
        if (it + DB_NI - 1 < S) issue_i(it + DB_NI - 1);
    }
    df32x16 acc[4][2];
    // per-lane state of the current row block I
    int cur_i = -1;
    float ni[2] = {0.f, 0.f};
    int cnt[2][NE];
    int mn[2] = {DB_NONE, DB_NONE};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int e = 0; e < NE; ++e) cnt[mb][e] = 0;

    auto flush = [&]() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = cur_i + 64 * wm + 32 * mb + l31;
            if constexpr (MODE == 0) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int v = cnt[mb][e] + __shfl_xor(cnt[mb][e], 32);
                    if (hh == 0 && gi < a.n && e < a.n_eps && v) atomicAdd(a.counts + (size_t)e * a.n + gi, v);
                    cnt[mb][e] = 0;
                }
            } else {
                const int m = min(mn[mb], __shfl_xor(mn[mb], 32));
                if (hh == 0 && gi < a.n && m != DB_NONE) {
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
    };
    auto finish = [&](di32x4 e) {
        const int I0 = e[0], J0 = e[1];
        if (I0 != cur_i) {
            flush();
            cur_i = I0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) ni[mb] = a.nrm[I0 + 64 * wm + 32 * mb + l31];          // (padding rows hold 0)
        }
        const float bm = a.bmax[J0 / DB_T];
        const int jw = J0 + 128 * wn;
        if constexpr (MODE == 0) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const int gi = I0 + 64 * wm + 32 * mb + l31;
                const bool iv = gi < a.n;
                const float b0 = (ni[mb] + bm) * 0x1p-12f;
                unsigned bits[2] = {0u, 0u};
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int gj = jw + 32 * nb + 4 * hh + (k & 3) + 8 * (k >> 2);
                        const bool ok = iv && gj < a.n;
                        const float d2 = acc[nb][mb][k];
                        const float y = ok ? d2 + b0 : __builtin_inff();
                        const float z = ok ? d2 - b0 : __builtin_inff();
                        bool inb = false;
#pragma unroll
                        for (int q = 0; q < NE; ++q) inb |= (y > a.thr.tl[q]) & (z <= a.thr.th[q]);
#pragma unroll
                        for (int q = 0; q < NE; ++q) cnt[mb][q] += (int)((y <= a.thr.tl[q]) & !inb);
                        bits[nb >> 1] |= inb ? (1u << (16 * (nb & 1) + k)) : 0u;
                    }
                const int nbits = __builtin_popcount(bits[0]) + __builtin_popcount(bits[1]);
                if (nbits) {
                    unsigned long long base = atomicAdd(a.band_count, (unsigned long long)nbits);
                    for (int h = 0; h < 2; ++h) {
                        unsigned b = bits[h];
                        while (b) {
                            const int p = __builtin_ctz(b);
                            b &= b - 1;
                            const int nb = 2 * h + (p >> 4), k = p & 15;
                            const int gj = jw + 32 * nb + 4 * hh + (k & 3) + 8 * (k >> 2);
                            if (base < (unsigned long long)a.cap) {
                                di32x4 ent;
                                ent[0] = gi; ent[1] = gj; ent[2] = 0; ent[3] = 0;
                                a.band[base] = ent;
                            }
                            ++base;
                        }
                    }
                }
            }
        } else {
            // labels of the 128 points j of this wave's half of the tile (DB_NONE: not a core point, or past the end): lane l holds j = jw + l and jw + 64 + l
            int lc[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = jw + 64 * h + lane;
                lc[h] = (j < a.n && a.cnt_e[j] >= a.min_samples) ? a.L[j] : DB_NONE;
            }
            const float tl = a.thr.tl[0];
            float b0[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) b0[mb] = (ni[mb] + bm) * 0x1p-12f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int jl = 32 * (nb & 1) + 4 * hh + (k & 3) + 8 * (k >> 2);
                    const int v = __shfl(lc[nb >> 1], jl);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        const float y = acc[nb][mb][k] + b0[mb];
                        mn[mb] = min(mn[mb], y <= tl ? v : DB_NONE);
                    }
                }
        }
    };
    for (long long s = 0; s < S; ++s) {
        const int ks = (int)(s % DB_SLABS);
        if (ks == 0 && s > 0) {
            e_prev = e_cur;
            e_cur = e_nxt;
            ++cur_tile;
            e_nxt = tile(cur_tile + 1);
        }
        if (S - 1 - s >= DB_NI - 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const unsigned char* A = dsm + DB_NI * DB_SLOT + (int)(s % DB_NJ) * DB_SLOT + j_row;
        const unsigned char* Bm = dsm + (int)(s % DB_NI) * DB_SLOT + i_row;
        dbf16x8 ah[2][4], bh[2][2], al[4], bl[2];
        auto load_hi = [&](int kk, int set) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bh[set][mb] = *reinterpret_cast<const dbf16x8*>(Bm + mb * 32 * DB_ROWB + poff[kk]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ah[set][nb] = *reinterpret_cast<const dbf16x8*>(A + nb * 32 * DB_ROWB + poff[kk]);
        };
        auto load_lo = [&](int kk) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bl[mb] = *reinterpret_cast<const dbf16x8*>(Bm + DB_PLANE + mb * 32 * DB_ROWB + poff[kk]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) al[nb] = *reinterpret_cast<const dbf16x8*>(A + DB_PLANE + nb * 32 * DB_ROWB + poff[kk]);
        };
        load_hi(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + DB_NJ - 1 < S) issue_j(s + DB_NJ - 1);
        if (s + DB_NI - 1 < S) issue_i(s + DB_NI - 1);
        __builtin_amdgcn_sched_barrier(0);
        if (ks == 0) {
            if (s > 0) finish(e_prev);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) acc[nb][mb][k] = 0.f;
        }
        const bool coords = ks < DB_D / DB_K;
#pragma unroll
        for (int kk = 0; kk < DB_K / 16; ++kk) {
            if (coords) load_lo(kk);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk & 1][nb], bh[kk & 1][mb], acc[nb][mb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (kk + 1 < DB_K / 16) load_hi(kk + 1, (kk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (coords) {
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[nb], bh[kk & 1][mb], acc[nb][mb], 0, 0, 0);
                        acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk & 1][nb], bl[mb], acc[nb][mb], 0, 0, 0);
                    }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    finish(e_cur);
    flush();
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

// ------------------------------------------------------------------------------------------------------------------------------------------
struct DbLayout { size_t pa, pb, nrm, bmax, count, total; };

static DbLayout db_layout(int64_t N) {
    DbLayout o;
    const size_t plane = (size_t)(N + DB_T) * DB_LD * sizeof(__bf16);
    const size_t nblk = (size_t)((N + DB_T - 1) / DB_T);
    o.pa = 0;
    o.pb = o.pa + align_up(2 * plane, 256);
    o.nrm = o.pb + align_up(2 * plane, 256);
    o.bmax = o.nrm + align_up((size_t)(N + DB_T) * sizeof(float), 256);
    o.count = o.bmax + align_up(nblk * sizeof(float), 256);
    o.total = o.count + 256;
    return o;
}

static int db_reserve_lds() {
    static bool attr_set = false;
    if (!attr_set) {
        const void* fns[] = {(const void*)db_tile_kernel<0, 1>, (const void*)db_tile_kernel<0, 4>, (const void*)db_tile_kernel<0, 10>,
                             (const void*)db_tile_kernel<0, 16>, (const void*)db_tile_kernel<1, 1>};
        for (const void* f : fns) {
            hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, DB_LDS);
            DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan: cannot reserve %d B of LDS: %s", DB_LDS, hipGetErrorString(e));
        }
        attr_set = true;
    }
    return DIC_OK;
}

static void db_fill_tile_args(DbTileArgs& t, unsigned char* ws, int64_t N) {
    const DbLayout o = db_layout(N);
    t.pa = (const __bf16*)(ws + o.pa);
    t.pb = (const __bf16*)(ws + o.pb);
    t.plane = (long)((N + DB_T) * DB_LD);
    t.nrm = (const float*)(ws + o.nrm);
    t.bmax = (const float*)(ws + o.bmax);
    t.n = (int)N;
    t.nblk = (int)((N + DB_T - 1) / DB_T);
    t.ntiles = (long long)t.nblk * t.nblk;
}

static unsigned db_grid(long long ntiles) { return (unsigned)max(1LL, min(ntiles, (long long)kNumCU)); }

static void db_margins(float t, float& tl, float& th) {
    tl = t * (1.f - 0x1p-20f);
    th = t * (1.f + 0x1p-20f);
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_dbscan_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > DB_D) return 0;
    return db_layout(N).total;
}

int dic_dbscan_counts(const float* X, long ldx, const float* centre, int64_t N, int D, const float* thresholds, int n_eps, int32_t* counts, int32_t* band,
                      int64_t capacity, int64_t* n_band, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && n_eps > 0 && capacity >= 0, DIC_ERR_INVALID_ARG, "dbscan_counts: N=%lld D=%d ldx=%ld n_eps=%d capacity=%lld",
                (long long)N, D, ldx, n_eps, (long long)capacity);
    DIC_REQUIRE(D <= DB_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "dbscan_counts: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, DB_D);
    DIC_REQUIRE(N < (1LL << 30) && n_eps <= DB_MAX_EPS, DIC_ERR_UNSUPPORTED, "dbscan_counts: N=%lld n_eps=%d (at most %d)", (long long)N, n_eps, DB_MAX_EPS);
    DIC_REQUIRE(X && centre && thresholds && counts && n_band && workspace && (band || capacity == 0), DIC_ERR_INVALID_ARG, "dbscan_counts: NULL pointer");
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0,
                DIC_ERR_UNSUPPORTED, "dbscan_counts: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dbscan_workspace(N, D), DIC_ERR_WORKSPACE, "dbscan_counts: workspace %zu < %zu", workspace_bytes,
                dic_dbscan_workspace(N, D));
    for (int e = 0; e < n_eps; ++e)
        DIC_REQUIRE(thresholds[e] >= 0.f, DIC_ERR_INVALID_ARG, "dbscan_counts: threshold %d = %g", e, (double)thresholds[e]);
    int rc = db_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const DbLayout o = db_layout(N);
    const long plane = (long)((N + DB_T) * DB_LD);
    __bf16* pa = (__bf16*)(ws + o.pa);
    __bf16* pb = (__bf16*)(ws + o.pb);
    float* nrm = (float*)(ws + o.nrm);
    unsigned long long* cnt_dev = (unsigned long long*)(ws + o.count);
    // padding rows behind the last point are read by the last tiles (and masked): zero, and norm 0
    hipError_t e = hipMemsetAsync(pa + (size_t)N * DB_LD, 0, (size_t)DB_T * DB_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pa + plane + (size_t)N * DB_LD, 0, (size_t)DB_T * DB_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + (size_t)N * DB_LD, 0, (size_t)DB_T * DB_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + plane + (size_t)N * DB_LD, 0, (size_t)DB_T * DB_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(nrm + N, 0, (size_t)DB_T * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt_dev, 0, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, (size_t)n_eps * N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan_counts: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(db_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, (int)N, D, pa, pb, plane, nrm);
    const int nblk = (int)((N + DB_T - 1) / DB_T);
    hipLaunchKernelGGL(db_block_max_kernel, dim3(nblk), dim3(256), 0, st, (const float*)nrm, (int)N, (float*)(ws + o.bmax));
    DbTileArgs t{};
    db_fill_tile_args(t, ws, N);
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
    const dim3 grid(db_grid(t.ntiles)), blk(512);
    switch (ne) {
        case 1: hipLaunchKernelGGL((db_tile_kernel<0, 1>), grid, blk, DB_LDS, st, t); break;
        case 4: hipLaunchKernelGGL((db_tile_kernel<0, 4>), grid, blk, DB_LDS, st, t); break;
        case 10: hipLaunchKernelGGL((db_tile_kernel<0, 10>), grid, blk, DB_LDS, st, t); break;
        default: hipLaunchKernelGGL((db_tile_kernel<0, 16>), grid, blk, DB_LDS, st, t); break;
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
    DIC_REQUIRE(D <= DB_D && N < (1LL << 30) && eps_index < DB_MAX_EPS, DIC_ERR_UNSUPPORTED, "dbscan_components_pass: N=%lld D=%d eps_index=%d", (long long)N,
                D, eps_index);
    DIC_REQUIRE(counts_e && labels && border && changed && workspace && (band || n_band == 0), DIC_ERR_INVALID_ARG, "dbscan_components_pass: NULL pointer");
    DIC_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)band & 15) == 0, DIC_ERR_UNSUPPORTED, "dbscan_components_pass: operands must be 16-B aligned");
    DIC_REQUIRE(workspace_bytes >= dic_dbscan_workspace(N, D), DIC_ERR_WORKSPACE, "dbscan_components_pass: workspace %zu < %zu", workspace_bytes,
                dic_dbscan_workspace(N, D));
    DIC_REQUIRE(threshold >= 0.f, DIC_ERR_INVALID_ARG, "dbscan_components_pass: threshold %g", (double)threshold);
    int rc = db_reserve_lds();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(border, 0x7f, (size_t)N * sizeof(int32_t), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "dbscan_components_pass: memset: %s", hipGetErrorString(e));
    DbTileArgs t{};
    db_fill_tile_args(t, (unsigned char*)workspace, N);
    for (int q = 0; q < DB_MAX_EPS; ++q) t.thr.t[q] = t.thr.tl[q] = t.thr.th[q] = -1.f;
    t.thr.t[0] = threshold;
    db_margins(threshold, t.thr.tl[0], t.thr.th[0]);
    t.n_eps = 1;
    t.cnt_e = counts_e;
    t.min_samples = min_samples;
    t.L = labels;
    t.border = border;
    t.changed = changed;
    hipLaunchKernelGGL((db_tile_kernel<1, 1>), dim3(db_grid(t.ntiles)), dim3(512), DB_LDS, st, t);
    if (n_band > 0)
        hipLaunchKernelGGL(db_band_link_kernel, dim3((unsigned)((n_band + 255) / 256)), dim3(256), 0, st, (const di32x4*)band, (long long)n_band, eps_index,
                           counts_e, min_samples, labels, border, changed);
    hipLaunchKernelGGL(db_jump_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, labels, (int)N);
    return check_launch("dbscan_components_pass");
}

}  // extern "C"
