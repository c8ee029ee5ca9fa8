// The pair-tile machine: the split-bf16 planes of the centred points, their layout in a workspace, and the persistent 256 x 256 tile loop, whose result -- the
// approximate d^2 of 2 x 64 (i, j) pairs per lane, in registers -- goes to an epilogue the caller supplies.  Nothing here decides anything.  Built on it: DBSCAN
// (dic_dbscan.hip), the k-th neighbour distances and lists (dic_knn.hip), the neighbour ranks (dic_knn_rank.hip), mean shift (dic_meanshift.hip), k-medoids
// (dic_kmedoids.hip), density peaks (dic_dpeaks.hip), the cluster-distance sums of the K sweep (dic_intra.hip) and the test probe (dic_pairtile_probe.hip).
//
// THE LOOP (pt_pair_pass<Src>).  One persistent 8-wave workgroup per CU walks its share of a list of 256 x 256 point-pair tiles, both operands' 32-column slabs
// (hi | lo: 32 KB) streamed through LDS-DMA rings (3 + 2 slots = all 160 KB), one raw barrier and one counted vmcnt wait per slab; d^2 = n_i + n_j - 2 v_i . v_j
// is one inner product of 288-column augmented rows, v = x - centre (f32), every coordinate as bf16 hi + lo with the products hi.hi + lo.hi + hi.lo, the f32
// norms n = sum v^2 as three exact bf16 pieces.  Lane = point i, registers = points j (the transposed product: a row's sum over j is in-lane): a lane's per-i
// results stay in registers while its workgroup stays on one row block I and are flushed by the epilogue when I changes.
//
// TILE SOURCES say which tiles a workgroup walks, as wave-uniform entries (first row of I, first row of J, e2, e3), and what the epilogue is told of them:
//   PtRowMajorTiles   ALL ordered block pairs (I, J), row-major, tiles tile0 .. tile0 + ntiles - 1 split into contiguous ranges (the default; e2 = e3 = 0 and
//                     the epilogue is given I0, J0 alone);
//   PtListTiles<C>    a host-built list of int4 entries, read through the scalar cache: contiguous ranges (C) or strided over the workgroups (!C); e2 and e3
//                     are the list's own (dic_intra.hip: the end row of a cluster, and a cluster or an output slot).
//
// ERROR BOUND of the approximate d^2 (call it a_ij) against the exact d^2_ij of the f32 points, u = 2^-24:
//   (1) v = fl(x - centre): each coordinate of v_i - v_j is off by <= u (|v_ik| + |v_jk|), so |d_v^2 - d^2| <= 2u (|v_i| + |v_j|)^2 (1 + u) <= 4.1u (n_i + n_j).
//   (2) the split: h = bf16(v), |v - h| <= 2^-8 |v|; l = bf16(v - h) (v - h exact in f32), |v - h - l| <= 2^-16 |v|.  The dropped part of a product a.b is
//       l_a l_b + r_a b + (h_a + l_a) r_b, <= 3.1 * 2^-16 |a| |b|; b = -2 v_j splits exactly as -2 (h, l), so -2 v_i . v_j is off by
//       <= 6.2 * 2^-16 sum_k |v_ik| |v_jk| <= 3.1 * 2^-16 (n_i + n_j).
//   (3) f32 accumulation: 288 / 16 * 3 = 54 chained MFMAs of 16 exact products each, at most 54 * 16 = 864 roundings in sequence, each of
//       sum |terms| <= (n_i + n_j) + 2 * (1 + 2^-7) sum |v_ik v_jk| <= 2.02 (n_i + n_j):  <= 864 u * 2.02 (n_i + n_j) <= 2^-13.2 (n_i + n_j).
//   (4) the norms' own f32 rounding (4 fmas + 6 shuffle adds): <= 10u (n_i + n_j).
//   Together |a_ij - d^2_ij| < (0.11 + 0.19 + 0.43 + 0.01) 2^-12 (n_i + n_j) < B0 = 2^-12 (n_i + nmax_J), nmax_J the largest n of j's 256-row block.
#pragma once
#include <initializer_list>
#include "dic_common.h"

namespace dic {

typedef __bf16 pbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pbf16x4 __attribute__((ext_vector_type(4)));
typedef float pf32x16 __attribute__((ext_vector_type(16)));
typedef float pf32x4 __attribute__((ext_vector_type(4)));
typedef int pi32x4 __attribute__((ext_vector_type(4)));

constexpr int PT_D = 256;                              // coordinates (narrower inputs are zero-padded by the caller to a multiple of 4)
constexpr int PT_LD = 288;                             // columns of an augmented row
constexpr int PT_T = 256;                              // points per tile edge
constexpr int PT_K = 32;                               // columns per slab
constexpr int PT_ROWB = PT_K * 2;                      // 64 B
constexpr int PT_PLANE = PT_T * PT_ROWB;               // 16 KB: one plane of a slab
constexpr int PT_SLOT = 2 * PT_PLANE;                  // 32 KB: hi | lo
constexpr int PT_SLABS = PT_LD / PT_K;                 // 9
constexpr int PT_NI = 3, PT_NJ = 2;                    // ring depths of the two operands
constexpr int PT_LDS = (PT_NI + PT_NJ) * PT_SLOT;      // 163 840 B
static_assert(PT_LDS <= 160 * 1024, "pair tiles: LDS budget");
// The norm the padding points present as j where an epilogue does not mask by index: their a_ij = 2^120 lies above every threshold a caller admits.
constexpr float PT_PAD_NORM = 0x1p120f;

// Workspace of the planes: pa / pb (hi | lo planes of the two operands, N + 256 rows each), the f32 norms (N + 256), the largest norm of every 256-row block,
// and one 256-B scratch word block for the caller.
struct PtLayout { size_t pa, pb, nrm, bmax, count, total; };

inline PtLayout pt_layout(int64_t N) {
    PtLayout o;
    const size_t plane = (size_t)(N + PT_T) * PT_LD * sizeof(__bf16);
    const size_t nblk = (size_t)((N + PT_T - 1) / PT_T);
    o.pa = 0;
    o.pb = o.pa + align_up(2 * plane, 256);
    o.nrm = o.pb + align_up(2 * plane, 256);
    o.bmax = o.nrm + align_up((size_t)(N + PT_T) * sizeof(float), 256);
    o.count = o.bmax + align_up(nblk * sizeof(float), 256);
    o.total = o.count + 256;
    return o;
}

// What the tile loop reads.  The tiles are the ordered block pairs (I, J), row-major; a launch walks tiles tile0 .. tile0 + ntiles - 1 (a run of whole row
// blocks I when tile0 and ntiles are multiples of nblk), split evenly over its workgroups.
struct PtPairArgs {
    const __bf16* pa; const __bf16* pb; long plane;
    const float* nrm; const float* bmax;
    int n, nblk; long long tile0, ntiles;
};

inline void pt_fill_pair_args(PtPairArgs& t, unsigned char* ws, int64_t N) {
    const PtLayout o = pt_layout(N);
    t.pa = (const __bf16*)(ws + o.pa);
    t.pb = (const __bf16*)(ws + o.pb);
    t.plane = (long)((N + PT_T) * PT_LD);
    t.nrm = (const float*)(ws + o.nrm);
    t.bmax = (const float*)(ws + o.bmax);
    t.n = (int)N;
    t.nblk = (int)((N + PT_T - 1) / PT_T);
    t.tile0 = 0;
    t.ntiles = (long long)t.nblk * t.nblk;
}

// What the tile loop reads when the tiles are a host-built list (PtListTiles below): the planes, and ntiles (< 2^31 / 9) int4 entries in device memory, 16-B
// aligned.
struct PtListArgs {
    const __bf16* pa; const __bf16* pb; long plane;
    const int4* tiles; int ntiles;
};

inline PtListArgs pt_list_args(unsigned char* ws, int64_t N, const int32_t* tiles, int ntiles) {
    const PtLayout o = pt_layout(N);
    return PtListArgs{(const __bf16*)(ws + o.pa), (const __bf16*)(ws + o.pb), (long)((N + PT_T) * PT_LD), (const int4*)tiles, ntiles};
}

inline unsigned pt_grid(long long ntiles) { return (unsigned)(ntiles < 1 ? 1 : ntiles < (long long)kNumCU ? ntiles : (long long)kNumCU); }

// The tile kernels `fns` of a file get the loop's dynamic LDS, once per process (`done` is the caller's).
inline int pt_reserve_lds(bool& done, std::initializer_list<const void*> fns, const char* who) {
    if (done) return DIC_OK;
    for (const void* f : fns) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, PT_LDS);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", who, PT_LDS, hipGetErrorString(e));
    }
    done = true;
    return DIC_OK;
}

// The augmented row of one point relative to the centre mu, and its f32 norm.  One wave per point: lane l holds coordinates 4 l .. 4 l + 3.
__device__ __forceinline__ void pt_prep_row(const float* X, long ldx, const float* mu, int row, int lane, int d, __bf16* pa, __bf16* pb, long plane, float* nrm_out) {
    const int col = 4 * lane;
    pf32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col < d) {
        const pf32x4 x = *reinterpret_cast<const pf32x4*>(X + (size_t)row * ldx + col);
        const pf32x4 m = *reinterpret_cast<const pf32x4*>(mu + col);
        v = x - m;
    }
    float nrm = fmaf(v[0], v[0], fmaf(v[1], v[1], fmaf(v[2], v[2], v[3] * v[3])));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) nrm += __shfl_xor(nrm, o);
    pbf16x4 ah, al, bh, bl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 h = (__bf16)v[e];
        const __bf16 l = (__bf16)(v[e] - (float)h);
        ah[e] = h; al[e] = l;
        bh[e] = (__bf16)(-2.f * (float)h); bl[e] = (__bf16)(-2.f * (float)l);          // exact
    }
    const size_t at = (size_t)row * PT_LD + col;
    *reinterpret_cast<pbf16x4*>(pa + at) = ah;
    *reinterpret_cast<pbf16x4*>(pa + plane + at) = al;
    *reinterpret_cast<pbf16x4*>(pb + at) = bh;
    *reinterpret_cast<pbf16x4*>(pb + plane + at) = bl;
    if (lane < 8) {                                     // columns 256 + 4 lane ..: [n n n 1 | 1 1 0 0 | 0 ..] and [1 1 1 n | n n 0 0 | 0 ..]
        const __bf16 n0 = (__bf16)nrm;
        const float r1 = nrm - (float)n0;
        const __bf16 n1 = (__bf16)r1;
        const __bf16 n2 = (__bf16)(r1 - (float)n1);
        const __bf16 one = (__bf16)1.f, z = (__bf16)0.f;
        pbf16x4 ea = {z, z, z, z}, eb = {z, z, z, z};
        if (lane == 0) { ea = pbf16x4{n0, n1, n2, one}; eb = pbf16x4{one, one, one, n0}; }
        if (lane == 1) { ea = pbf16x4{one, one, z, z}; eb = pbf16x4{n1, n2, z, z}; }
        const size_t et = (size_t)row * PT_LD + PT_D + 4 * lane;
        const pbf16x4 zz = {z, z, z, z};
        *reinterpret_cast<pbf16x4*>(pa + et) = ea;
        *reinterpret_cast<pbf16x4*>(pa + plane + et) = zz;
        *reinterpret_cast<pbf16x4*>(pb + et) = eb;
        *reinterpret_cast<pbf16x4*>(pb + plane + et) = zz;
    }
    if (lane == 0) nrm_out[row] = nrm;
}

// Every point relative to one centre (row 0 of mu) ...
static __global__ __launch_bounds__(256) void pt_prep_kernel(const float* X, long ldx, const float* mu, int n, int d, __bf16* pa, __bf16* pb, long plane, float* nrm_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    pt_prep_row(X, ldx, mu, row, lane, d, pa, pb, plane, nrm_out);
}

// ... or relative to the centre of its own segment: row c of mu (K, d), seg[c] <= row < seg[c + 1] (points sorted by cluster, seg the K + 1 boundaries).
// HOW: pt_prepare_planes' (below), which instantiates the kernel only where it centres per segment.
template <int HOW>
static __global__ __launch_bounds__(256) void pt_prep_seg_kernel(const float* X, long ldx, const float* mu, const int32_t* seg, int K, int n, int d, __bf16* pa, __bf16* pb,
                                                                 long plane, float* nrm_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    int lo = 0, hi = K;                                 // seg[lo] <= row < seg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= row) lo = mid; else hi = mid;
    }
    pt_prep_row(X, ldx, mu + (size_t)lo * d, row, lane, d, pa, pb, plane, nrm_out);
}

// largest norm of every 256-row block (norms are >= 0; rows past n count 0)
static __global__ __launch_bounds__(256) void pt_block_max_kernel(const float* nrm, int n, float* bmax) {
    __shared__ float part[4];
    const int i = blockIdx.x * PT_T + threadIdx.x;
    float v = i < n ? nrm[i] : 0.f;
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// The norm columns of the 256 padding points (their rows are zeroed beforehand): pt_prep_kernel's [n n n 1 | 1 1 ..] and [1 1 1 n | n n ..] with the norm 0
// as operand i and `pad_norm` (a power of two: exact in bf16) as operand j.  The ones carry the OTHER point's norm pieces: without them a padding point is no
// zero vector but an absent one -- a_ij = 0 instead of n_j in a padding row, pad_norm alone instead of n_i + pad_norm in a padding column (with
// PT_PAD_NORM the same f32 value; no epilogue flushes a padding row, and those that pass 0 mask the columns by index, so only tests/test_gpu_pairtile.py can
// tell the two apart).
static __global__ __launch_bounds__(256) void pt_pad_rows_kernel(__bf16* pa, __bf16* pb, int n, float pad_norm) {
    const size_t et = (size_t)(n + threadIdx.x) * PT_LD + PT_D;
    const __bf16 one = (__bf16)1.f;
    pa[et + 3] = one; pa[et + 4] = one; pa[et + 5] = one;
    pb[et] = one; pb[et + 1] = one; pb[et + 2] = one;
    pb[et + 3] = (__bf16)pad_norm;
}

// Rows first .. first + count - 1 of pb present the norm pad_norm as operand j: rows behind the points that are no column of anybody's, as the padding
// points are none (the queries dic_knn.hip stacks behind its index points to walk them as operand i; dic_meanshift.hip's rows between the last point and the
// first seed).
static __global__ __launch_bounds__(256) void pt_mask_cols_kernel(__bf16* pb, long long first, long long count, float pad_norm) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < count) pb[(size_t)(first + t) * PT_LD + PT_D + 3] = (__bf16)pad_norm;
}

// Fills the planes, norms and block maxima of a pt_layout(N) workspace from X (N, D) f32 and the centre (1, D).  The 256 padding rows behind the last point,
// which the last tiles read, are zero vectors of norm 0 as operand i (a_ij = n_j); as operand j they present the norm pad_norm, so their approximate d^2 is
// n_i + pad_norm: with 0 an epilogue masks them by index, with a huge value they lie beyond every threshold and need no mask.  (The norm array and the block
// maxima, which feed the error bound, hold 0 for them either way.)  HOW:
constexpr int PT_BY_SEGMENT = 1;          // centre = the centres (K, D) of the K segments seg[c] .. seg[c + 1] - 1 of the rows
constexpr int PT_SUMS_ONLY = 2;           // for epilogues that mask by index and compare a_ij with nothing: padding rows all zero (a_ij = 0 there; pad_norm is
                                          // not used), no block maxima -- two launches fewer
template <int HOW = 0>
static int pt_prepare_planes(const float* X, long ldx, const float* centre, int64_t N, int D, float pad_norm, unsigned char* ws, hipStream_t st, const char* who,
                             const int32_t* seg = nullptr, int K = 1) {
    const PtLayout o = pt_layout(N);
    const long plane = (long)((N + PT_T) * PT_LD);
    __bf16* pa = (__bf16*)(ws + o.pa);
    __bf16* pb = (__bf16*)(ws + o.pb);
    float* nrm = (float*)(ws + o.nrm);
    hipError_t e = hipMemsetAsync(pa + (size_t)N * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pa + plane + (size_t)N * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + (size_t)N * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess) e = hipMemsetAsync(pb + plane + (size_t)N * PT_LD, 0, (size_t)PT_T * PT_LD * sizeof(__bf16), st);
    if (e == hipSuccess && !(HOW & PT_SUMS_ONLY)) e = hipMemsetAsync(nrm + N, 0, (size_t)PT_T * sizeof(float), st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));
    if constexpr (!(HOW & PT_SUMS_ONLY)) hipLaunchKernelGGL(pt_pad_rows_kernel, dim3(1), dim3(256), 0, st, pa, pb, (int)N, pad_norm);
    if constexpr (HOW & PT_BY_SEGMENT)
        hipLaunchKernelGGL(pt_prep_seg_kernel<HOW>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, seg, K, (int)N, D, pa, pb, plane, nrm);
    else
        hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, ldx, centre, (int)N, D, pa, pb, plane, nrm);
    if constexpr (!(HOW & PT_SUMS_ONLY)) {
        const int nblk = (int)((N + PT_T - 1) / PT_T);
        hipLaunchKernelGGL(pt_block_max_kernel, dim3(nblk), dim3(256), 0, st, (const float*)nrm, (int)N, (float*)(ws + o.bmax));
    }
    return DIC_OK;
}

// LDS-DMA as asm (the compiler does not count it in vmcnt): 64 lanes x 16 B -> 1 KiB at lds_dst
__device__ __forceinline__ void ptdma16(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// Where a lane sits in its 8-wave workgroup: wave (wm, wn) owns rows 64 wm .. + 63 and columns 128 wn .. + 127 of the tile; the lane holds rows
// 64 wm + 32 mb + l31 (mb = 0, 1) and, of accumulator acc[nb][mb][k], column 128 wn + 32 nb + 4 hh + (k & 3) + 8 (k >> 2).
struct PtLane {
    int lane, hh, l31, wm, wn;
    __device__ __forceinline__ PtLane() {
        lane = threadIdx.x & 63; hh = lane >> 5; l31 = lane & 31;
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        wm = w & 3; wn = w >> 2;
    }
    __device__ __forceinline__ int row(int I0, int mb) const { return I0 + 64 * wm + 32 * mb + l31; }
    __device__ __forceinline__ int col(int J0, int nb, int k) const { return J0 + 128 * wn + 32 * nb + 4 * hh + (k & 3) + 8 * (k >> 2); }
};

// A tile-list entry through the scalar cache.  (The compiler would use a vector load: counted in vmcnt among DMA instructions it cannot see, it either drains
// the ring or upsets the counted wait.)
__device__ __forceinline__ pi32x4 pt_sload_tile(const int4* p) {
    pi32x4 r;
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory");
    return r;
}

// TILE SOURCES: which tiles a workgroup walks, and what an epilogue is told about them.  A source is built from the kernel's arguments (which also hold the
// planes pa, pb, plane).  count(): the workgroup's number of tiles; at(i), i < count(): the wave-uniform entry (first row of I, first row of J, e2, e3) of its
// i-th tile; finish(epi, e, acc): hands a finished tile to the epilogue; `index`: the width the loop counts tiles and slabs in.

// The row-major block pairs tile0 .. tile0 + ntiles - 1 of PtPairArgs, split evenly into contiguous ranges.  Epilogues get the tile's corner:
// epi.finish(I0, J0, acc).  (Stateless -- count() and at() compute from the arguments and the launch's indices: with the range kept in members the loop's
// scalar code came out differently, for no gain.)
struct PtRowMajorTiles {
    typedef long long index;
    const PtPairArgs& a;
    __device__ __forceinline__ long long per() const {
        const long long nch = gridDim.x;
        return (a.ntiles + nch - 1) / nch;
    }
    __device__ __forceinline__ long long count() const {
        const long long first = (long long)blockIdx.x * per();
        return max(0LL, min(per(), a.ntiles - first));
    }
    __device__ __forceinline__ pi32x4 at(long long i) const {
        const long long first = (long long)blockIdx.x * per();
        const long long t = a.tile0 + first + i;
        const int bi = (int)(t / a.nblk), bj = (int)(t - (long long)bi * a.nblk);
        pi32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane(bi * PT_T);
        r[1] = __builtin_amdgcn_readfirstlane(bj * PT_T);
        r[2] = 0; r[3] = 0;
        return r;
    }
    template <class Epi>
    static __device__ __forceinline__ void finish(Epi& epi, const pi32x4& e, const pf32x16 (&acc)[4][2]) { epi.finish(e[0], e[1], acc); }
};

// The list of PtListArgs, read through the scalar cache.  CONTIGUOUS: workgroup b takes entries b per .. b per + per - 1, per = ceil(ntiles / grid);
// otherwise entries b, b + grid, b + 2 grid, ...  Epilogues get the whole entry: epi.finish(e, acc).  (Counted in int: with 64-bit counters the passes of
// dic_intra.hip were 5 % slower.)
template <bool CONTIGUOUS>
struct PtListTiles {
    typedef int index;
    const int4* tiles;
    int first, step, my_tiles;
    __device__ __forceinline__ PtListTiles(const PtListArgs& a) : tiles(a.tiles) {
        const int nch = gridDim.x, b = blockIdx.x;
        const int per = (a.ntiles + nch - 1) / nch;
        first = CONTIGUOUS ? b * per : b;
        step = CONTIGUOUS ? 1 : nch;
        my_tiles = CONTIGUOUS ? max(0, min(per, a.ntiles - b * per)) : (b < a.ntiles ? (a.ntiles - 1 - b) / nch + 1 : 0);
    }
    __device__ __forceinline__ int count() const { return my_tiles; }
    __device__ __forceinline__ pi32x4 at(int i) const { return pt_sload_tile(tiles + __builtin_amdgcn_readfirstlane(first + i * step)); }
    template <class Epi>
    static __device__ __forceinline__ void finish(Epi& epi, const pi32x4& e, const pf32x16 (&acc)[4][2]) { epi.finish(e, acc); }
};

// The persistent tile loop (launch with 512 threads, PT_LDS bytes of dynamic LDS, __launch_bounds__(512, 1)).  For every tile of the workgroup's share of the
// source Src{a}, in order: the source's finish (above) with acc[nb][mb][k] = the approximate d^2 of (PtLane::row(I0, mb), PtLane::col(J0, nb, k)); after the
// last one epi.flush().  An epilogue keeps its per-row results in registers while I0 stays the same and flushes them itself when it changes.
//
// DMA: a plane of a slab = 16 instructions of 16 rows; wave w issues c = w, w + 8, w + 16, w + 24 of the 32 (plane c >> 4, row group c & 15); lane L -> row
// 16 rg + (L >> 2), physical 16-B piece L & 3 = logical piece (L & 3) ^ ((row >> 2) & 3), and (row >> 2) & 3 = (L >> 4) & 3 for every row group.  Fragment reads:
// row (32 block + l31), logical piece 2 kk + hh -> physical piece ^ ((l31 >> 2) & 3).  The entries of the tile being multiplied and of the next one (whose
// first slabs are requested two iterations ahead, hence the clamp to the last tile) live in scalar registers.
template <class Src = PtRowMajorTiles, class Args, class Epi>
__device__ __forceinline__ void pt_pair_pass(const Args& a, Epi& epi) {
    typedef typename Src::index idx;
    extern __shared__ __align__(16) unsigned char dsm[];
    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l31 = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wm = w & 3, wn = w >> 2;
    const Src src{a};
    const idx my_tiles = src.count();
    const idx S = my_tiles * PT_SLABS;
    if (S == 0) return;
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char*)dsm);
    const unsigned ldsI = lds0, ldsJ = lds0 + PT_NI * PT_SLOT;
    const unsigned v_dma = (unsigned)(lane >> 2) * (PT_LD * 2) + (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
    auto tile = [&](idx i) { return src.at(min(i, my_tiles - 1)); };
    pi32x4 e_cur = tile(0), e_nxt = tile(1), e_prev = e_cur;
    idx cur_tile = 0;
    auto issue = [&](const __bf16* mat, int row0, int ks, unsigned dst) {
        const __bf16* base = mat + (size_t)row0 * PT_LD + ks * PT_K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = w + 8 * j, pl = c >> 4, rg = c & 15;
            const uint64_t p = (uint64_t)(base + (size_t)pl * a.plane + (size_t)(16 * rg) * PT_LD);          // (uniform: keep the base in scalar registers)
            const uint64_t q = ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(p >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)p);
            ptdma16((const void*)q, v_dma, __builtin_amdgcn_readfirstlane(dst + pl * PT_PLANE + rg * 1024));
        }
    };
    auto issue_i = [&](idx s) { issue(a.pa, s / PT_SLABS == cur_tile ? e_cur[0] : e_nxt[0], (int)(s % PT_SLABS), ldsI + (int)(s % PT_NI) * PT_SLOT); };
    auto issue_j = [&](idx s) { issue(a.pb, s / PT_SLABS == cur_tile ? e_cur[1] : e_nxt[1], (int)(s % PT_SLABS), ldsJ + (int)(s % PT_NJ) * PT_SLOT); };
    const int sw = (l31 >> 2) & 3;
    int poff[PT_K / 16];
#pragma unroll
    for (int kk = 0; kk < PT_K / 16; ++kk) poff[kk] = ((2 * kk + hh) ^ sw) * 16;
    const int j_row = (128 * wn + l31) * PT_ROWB;
    const int i_row = (64 * wm + l31) * PT_ROWB;

#pragma unroll
    for (int it = 1 - PT_NI; it < 0; ++it) {
        if (it + PT_NJ - 1 >= 0 && it + PT_NJ - 1 < S) issue_j(it + PT_NJ - 1);
        if (it + PT_NI - 1 < S) issue_i(it + PT_NI - 1);
    }
    pf32x16 acc[4][2];
    for (idx s = 0; s < S; ++s) {
        const int ks = (int)(s % PT_SLABS);
        if (ks == 0 && s > 0) {          // (before this iteration's requests: they may belong to the tile after this one)
            e_prev = e_cur;
            e_cur = e_nxt;
            ++cur_tile;
            e_nxt = tile(cur_tile + 1);
        }
        // counted wait: at the top of iteration s the DMA instructions still allowed in flight are those of I-slab s + 1 (4 per wave), issued last in iteration s - 1
        if (S - 1 - s >= PT_NI - 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // everybody's pieces of slab s are in; everybody is done reading slab s - 1 (its two slots are free)
        const unsigned char* A = dsm + PT_NI * PT_SLOT + (int)(s % PT_NJ) * PT_SLOT + j_row;
        const unsigned char* Bm = dsm + (int)(s % PT_NI) * PT_SLOT + i_row;
        pbf16x8 ah[2][4], bh[2][2], al[4], bl[2];
        auto load_hi = [&](int kk, int set) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bh[set][mb] = *reinterpret_cast<const pbf16x8*>(Bm + mb * 32 * PT_ROWB + poff[kk]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ah[set][nb] = *reinterpret_cast<const pbf16x8*>(A + nb * 32 * PT_ROWB + poff[kk]);
        };
        auto load_lo = [&](int kk) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bl[mb] = *reinterpret_cast<const pbf16x8*>(Bm + PT_PLANE + mb * 32 * PT_ROWB + poff[kk]);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) al[nb] = *reinterpret_cast<const pbf16x8*>(A + PT_PLANE + nb * 32 * PT_ROWB + poff[kk]);
        };
        load_hi(0, 0);
        __builtin_amdgcn_sched_barrier(0);          // (the first fragment reads go out BEFORE the DMA instructions)
        if (s + PT_NJ - 1 < S) issue_j(s + PT_NJ - 1);
        if (s + PT_NI - 1 < S) issue_i(s + PT_NI - 1);
        __builtin_amdgcn_sched_barrier(0);
        if (ks == 0) {
            if (s > 0) Src::finish(epi, e_prev, acc);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int k = 0; k < 16; ++k) acc[nb][mb][k] = 0.f;
        }
        const bool coords = ks < PT_D / PT_K;          // the augmentation slab has empty lo planes
#pragma unroll
        for (int kk = 0; kk < PT_K / 16; ++kk) {
            if (coords) load_lo(kk);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk & 1][nb], bh[kk & 1][mb], acc[nb][mb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (kk + 1 < PT_K / 16) load_hi(kk + 1, (kk + 1) & 1);
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
    Src::finish(epi, e_cur, acc);
    epi.flush();
}

}  // namespace dic
