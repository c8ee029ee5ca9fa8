// Consensus clustering (Monti et al. 2003 / ConsensusClusterPlus) from a label matrix, and the average-linkage agglomeration of its consensus distance:
// the p2 / p4 `--cluster_method consensus` branches (p4_clustering_final.py:241-287 reads labels that were "generated outside"; here they are generated).
// L (N, ldl) uint8 holds, per point and resample h < H, the k-means label 0..K-1 of the point in that resample, or 0xFF where the resample left it out; the
// columns H..ldl-1 hold 0xFF.  For a pair, in integers: both = #{h: L_ih != FF and L_jh != FF}, agree = #{h: L_ih == L_jh != FF}; consensus M = agree / both
// (0 when both == 0), distance d = 1.0 - (double)agree / (double)both (1 when both == 0, 0 on the diagonal), CDF bin t = ceil(100 agree / both) in integers.
//
// THE PAIR PASS (cs_pairs_kernel, cs_rowsum_kernel): 128 x 128 tiles of pairs, a workgroup of 1024 threads, 4 x 4 pairs per thread.  The label bytes of the
// two operands are staged 64 resamples at a time in LDS, transposed (word w of 128 rows side by side, so a thread's four rows are one 16-B read), with "left
// out" recoded to FE on the column operand: FF never equals FE, and no label is either (K <= 254), so agree is the number of zero bytes of a ^ b, four
// resamples per dword: popc(~(x | ((x & 7f7f7f7f) + 7f7f7f7f)) & 80808080), exact per byte (7f + 7f carries nowhere).  both is popc of the ANDed sampled
// masks, one bit per resample, built while staging.  Nothing depends on K.
//   hist, D: the block pairs J >= I only, dealt round-robin to a persistent grid of at most kNumCU workgroups.  hist counts the unordered pairs i < j: each
//       thread keeps its own counts of the bins 0 and 100 (on real inputs nearly every pair) in registers, the other bins go to a per-workgroup LDS histogram by
//       64-bit LDS atomics; one 64-bit global atomic per non-empty bin and workgroup at the end.  Integer sums: the order does not matter.  D is written at
//       (i, j) and mirrored to (j, i) from the same register, hence exactly symmetric.
//   rowsum[i, c] = sum over j != i with y_j = c of M(i, j), in f64: a sum whose bits depend on its order, so it is NOT credited to both rows by atomics.
//       The rows are first sorted by cluster (counting sort on the device, stable, every cluster's segment padded to whole 128-row tiles with never-sampled
//       rows, whose M is +0.0); a workgroup owns a block of 128 rows i and walks every column tile in order: the thread's four columns are added left to right,
//       the 32 threads of a row by one xor tree, and the tile's sum goes to a register that is stored when the tile's cluster changes.  One owner, one order:
//       two calls give the same bits.  This visits all block pairs, not half of them.
//
// THE AGGLOMERATION (lk_step_kernel): scipy.cluster.hierarchy.linkage(., 'average')'s nearest-neighbour chain on the square matrix D, which is destroyed:
//   size[i] = 1, chain empty; N - 1 times: if the chain is empty it becomes [smallest live i]; then repeat: x = chain[-1]; y = the live i != x of smallest
//   (D[x, i], i), except that chain[-2] wins when it ties that minimum; if y == chain[-2] stop, else append y.  Pop both, (x, y) = (min, max), record
//   (x, y, D[x, y], nx + ny), size[x] = 0, size[y] = nx + ny, and D[i, y] = D[y, i] = (nx D[i, x] + ny D[i, y]) / (nx + ny) for every live i != y.
// Each repeat of the inner loop is ONE launch of ONE workgroup: a scan of row x and, when the neighbours are mutual, the update of row and column y.  size,
// chain, its length and the merge count live on the device, every launch reads them where the previous one left them, and no workgroup ever waits for
// another.  A launch pushes or merges, so 3 (N - 1) launches bound the loop; one that finds N - 1 merges done returns at once.  The update is compiled under
// `#pragma clang fp contract(off)` (lk_average): every operation correctly rounded and none contracted to an fma, so every height has the bits scipy computes, and ties fall as scipy's.
// The square layout costs 8 N^2 bytes (45 GB at 75 000 points): the one N x N array of the project.  Average linkage on a ratio-valued similarity has no
// matrix-free form -- the distance between two clusters is a mean over their pairs of quotients that share no structure -- so the matrix is held.
#include "dic_common.h"

namespace dic {

constexpr int CS_T = 128;                       // points per tile edge
constexpr int CS_THREADS = 1024;                // 32 x 32 threads, 4 x 4 pairs each
constexpr int CS_CW = 16;                       // dwords of a row per staged chunk: 64 resamples
constexpr int CS_LDR = CS_T + 4;                // row of the transposed stage: 132 dwords (16-B aligned, and the staging stores hit 64 different banks)
constexpr int CS_BINS = DIC_CONSENSUS_BINS;     // B: the CDF has B + 1 bins
constexpr int CS_MAXK = 254;

typedef unsigned cu32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cu32x2 __attribute__((ext_vector_type(2)));

struct CsStage {
    unsigned a[CS_CW][CS_LDR];                  // row operand, word w of every row
    unsigned b[CS_CW][CS_LDR];                  // column operand (FF -> FE)
    unsigned char ma[CS_T][8];                  // sampled masks: one bit per resample of the chunk
    unsigned char mb[CS_T][8];
};

// 0x80 in every byte of w that is 0xFF
__device__ __forceinline__ unsigned cs_ff_bytes(unsigned w) {
    const unsigned x = ~w;
    return ~(x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
}
__device__ __forceinline__ unsigned cs_equal_bytes(unsigned a, unsigned b) {
    const unsigned x = a ^ b;
    return __builtin_popcount(~(x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u);
}
// bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ unsigned cs_pack4(unsigned z) {
    const unsigned t = z >> 7;
    return (t & 1u) | ((t >> 7) & 2u) | ((t >> 14) & 4u) | ((t >> 21) & 8u);
}

// the 8 bytes thread tid stages of one operand: row tid / 8 of the tile, bytes 8 (tid % 8) .. + 7 of the chunk; FF outside the matrix
__device__ __forceinline__ cu32x2 cs_fetch(const unsigned char* L, long ldl, int nrows, int row0, int chunk) {
    const int r = row0 + (int)(threadIdx.x >> 3);
    const long at = (long)chunk * (CS_CW * 4) + 8 * (threadIdx.x & 7);
    cu32x2 v = {0xffffffffu, 0xffffffffu};
    if (r < nrows && at < ldl) v = *reinterpret_cast<const cu32x2*>(L + (size_t)r * ldl + at);          // (ldl % 16 == 0: the 8 bytes are inside the row)
    return v;
}

__device__ __forceinline__ void cs_put(unsigned (*dst)[CS_LDR], unsigned char (*mask)[8], cu32x2 v, bool column) {
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
    const unsigned z0 = cs_ff_bytes(v[0]), z1 = cs_ff_bytes(v[1]);
    if (column) { v[0] ^= z0 >> 7; v[1] ^= z1 >> 7; }          // FF -> FE
    dst[2 * q][r] = v[0];
    dst[2 * q + 1][r] = v[1];
    mask[r][q] = (unsigned char)(~(cs_pack4(z0) | (cs_pack4(z1) << 4)) & 0xffu);
}

// agree / both of the 4 x 4 pairs (rows 4 ti + r of the row tile, columns 4 tj + c of the column tile) of thread (ti, tj) = (tid / 32, tid % 32).
// Call from all 1024 threads.
__device__ __forceinline__ void cs_tile(CsStage& s, const unsigned char* LA, int nA, int rowA0, const unsigned char* LB, int nB, int rowB0, long ldl,
                                        unsigned (&agree)[4][4], unsigned (&both)[4][4]) {
    const int ti = threadIdx.x >> 5, tj = threadIdx.x & 31;
    const int nchunk = (int)((ldl + CS_CW * 4 - 1) / (CS_CW * 4));
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { agree[r][c] = 0u; both[r][c] = 0u; }
    cu32x2 va = cs_fetch(LA, ldl, nA, rowA0, 0), vb = cs_fetch(LB, ldl, nB, rowB0, 0);
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();          // (the previous chunk, or the previous tile, has been read)
        cs_put(s.a, s.ma, va, false);
        cs_put(s.b, s.mb, vb, true);
        __syncthreads();
        if (ch + 1 < nchunk) {          // in flight under the compares
            va = cs_fetch(LA, ldl, nA, rowA0, ch + 1);
            vb = cs_fetch(LB, ldl, nB, rowB0, ch + 1);
        }
        cu32x2 ma[4], mb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ma[r] = *reinterpret_cast<const cu32x2*>(&s.ma[4 * ti + r][0]);
#pragma unroll
        for (int c = 0; c < 4; ++c) mb[c] = *reinterpret_cast<const cu32x2*>(&s.mb[4 * tj + c][0]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) both[r][c] += __builtin_popcount(ma[r][0] & mb[c][0]) + __builtin_popcount(ma[r][1] & mb[c][1]);
#pragma unroll 4
        for (int w = 0; w < CS_CW; ++w) {
            const cu32x4 a = *reinterpret_cast<const cu32x4*>(&s.a[w][4 * ti]);
            const cu32x4 b = *reinterpret_cast<const cu32x4*>(&s.b[w][4 * tj]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) agree[r][c] += cs_equal_bytes(a[r], b[c]);
        }
    }
}

// block pair t of the upper triangle, row-major: row I holds the nb - I pairs (I, I), (I, I + 1), ..
__device__ __forceinline__ void cs_block_pair(long long t, long long nb, int& I, int& J) {
    const double m = 2.0 * (double)nb + 1.0;
    long long i = (long long)((m - sqrt(m * m - 8.0 * (double)t)) * 0.5);
    i = max(0LL, min(nb - 1, i));
    while (i > 0 && i * nb - i * (i - 1) / 2 > t) --i;
    while ((i + 1) * nb - (i + 1) * i / 2 <= t) ++i;
    I = (int)i;
    J = (int)(i + (t - (i * nb - i * (i - 1) / 2)));
}

__global__ __launch_bounds__(CS_THREADS) void cs_pairs_kernel(const unsigned char* L, long ldl, int n, unsigned long long* hist, double* D) {
    __shared__ __align__(16) CsStage s;
    __shared__ unsigned long long s_hist[CS_BINS + 1];
    const int tid = threadIdx.x, ti = tid >> 5, tj = tid & 31;
    if (tid <= CS_BINS) s_hist[tid] = 0ull;          // (the first tile's barriers order this before the first LDS atomic)
    unsigned long long n0 = 0ull, nfull = 0ull;
    const long long nb = (n + CS_T - 1) / CS_T, total = nb * (nb + 1) / 2;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        int I, J;
        cs_block_pair(t, nb, I, J);
        unsigned agree[4][4], both[4][4];
        cs_tile(s, L, n, I * CS_T, L, n, J * CS_T, ldl, agree, both);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = I * CS_T + 4 * ti + r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = J * CS_T + 4 * tj + c;
                if (i >= n || j >= n) continue;
                const unsigned ag = agree[r][c], bo = both[r][c];
                if (hist && i < j) {
                    const unsigned bin = bo ? (CS_BINS * ag + bo - 1u) / bo : 0u;          // (H <= 65535: 100 agree + both < 2^32)
                    if (bin == 0u) ++n0;
                    else if (bin == CS_BINS) ++nfull;
                    else atomicAdd(&s_hist[bin], 1ull);
                }
                if (D) {
                    const double d = i == j ? 0.0 : (bo ? 1.0 - __ddiv_rn((double)ag, (double)bo) : 1.0);
                    D[(size_t)i * n + j] = d;
                    if (I != J) D[(size_t)j * n + i] = d;          // (a diagonal block computes both of its halves itself)
                }
            }
        }
    }
    if (!hist) return;
    if (n0) atomicAdd(&s_hist[0], n0);
    if (nfull) atomicAdd(&s_hist[CS_BINS], nfull);
    __syncthreads();
    if (tid <= CS_BINS && s_hist[tid]) atomicAdd(&hist[tid], s_hist[tid]);
}

// ---- rows sorted by cluster ----------------------------------------------------------------------------------------------------------------------------------
struct CsSorted { size_t count, start, ntile, tcl, idx, ls, total; };

static CsSorted cs_sorted_layout(int64_t N, long ldl, int K) {
    CsSorted o;
    const size_t rows = (size_t)((N + CS_T - 1) / CS_T + K) * CS_T;          // every cluster pads to whole tiles: fewer than CS_T rows each
    o.count = 0;
    o.start = o.count + align_up((size_t)(CS_MAXK + 2) * sizeof(int), 256);
    o.ntile = o.start + align_up((size_t)(CS_MAXK + 2) * sizeof(int), 256);
    o.tcl = o.ntile + 256;
    o.idx = o.tcl + align_up(rows / CS_T * sizeof(int), 256);
    o.ls = o.idx + align_up(rows * sizeof(int), 256);
    o.total = o.ls + align_up(rows * (size_t)ldl, 256);
    return o;
}

__global__ __launch_bounds__(256) void cs_count_kernel(const int32_t* y, int n, int K, int* count) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int c = y[j];
    if ((unsigned)c < (unsigned)K) atomicAdd(&count[c], 1);
}

// one thread: first sorted row of every cluster, the cluster of every column tile, the number of tiles
__global__ void cs_starts_kernel(const int* count, int K, int* start, int* ntile, int* tcl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int t = 0;
    for (int c = 0; c < K; ++c) {
        start[c] = t * CS_T;
        const int tiles = (count[c] + CS_T - 1) / CS_T;
        for (int k = 0; k < tiles; ++k) tcl[t + k] = c;
        t += tiles;
    }
    *ntile = t;
}

// workgroup c: the members of cluster c in ascending index order (a stable counting sort) -> idx[start[c] + rank]
__global__ __launch_bounds__(256) void cs_rank_kernel(const int32_t* y, int n, const int* start, int32_t* idx) {
    __shared__ int s_w[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = start[c];
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + tid;
        const bool mine = j < n && y[j] == c;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; ++k) before += s_w[k];
        const int all = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (mine) idx[base + before] = j;
        base += all;
        __syncthreads();
    }
}

// sorted copy of the label rows: row p = L[idx[p]], or FF (never sampled) where idx[p] < 0; 16 B per thread
__global__ __launch_bounds__(256) void cs_gather_kernel(const unsigned char* L, long ldl, const int32_t* idx, const int* ntile, unsigned char* Ls) {
    const long per = ldl / 16;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long p = g / per;
    if (p >= (long long)*ntile * CS_T) return;
    const long q = (long)(g - p * per);
    const int src = idx[p];
    cu32x4 v = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (src >= 0) v = *reinterpret_cast<const cu32x4*>(L + (size_t)src * ldl + 16 * q);
    *reinterpret_cast<cu32x4*>(Ls + (size_t)p * ldl + 16 * q) = v;
}

__global__ __launch_bounds__(CS_THREADS) void cs_rowsum_kernel(const unsigned char* L, long ldl, int n, int K, const unsigned char* Ls, const int32_t* idx,
                                                              const int* ntile_p, const int* tcl, double* rowsum) {
    __shared__ __align__(16) CsStage s;
    const int tid = threadIdx.x, ti = tid >> 5, tj = tid & 31;
    const int ntile = *ntile_p, nb = (n + CS_T - 1) / CS_T;
    for (int I = blockIdx.x; I < nb; I += gridDim.x) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int cur = -1;
        auto flush = [&]() {
            if (cur < 0 || tj != 0) return;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = I * CS_T + 4 * ti + r;
                if (i < n) rowsum[(size_t)i * K + cur] = acc[r];
            }
        };
        for (int jt = 0; jt < ntile; ++jt) {
            const int c = tcl[jt];
            if (c != cur) {
                flush();
                cur = c;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = 0.0;
            }
            unsigned agree[4][4], both[4][4];
            cs_tile(s, L, n, I * CS_T, Ls, ntile * CS_T, jt * CS_T, ldl, agree, both);
            int src[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) src[cc] = idx[jt * CS_T + 4 * tj + cc];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = I * CS_T + 4 * ti + r;
                double v = 0.0;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
                    if (src[cc] >= 0 && src[cc] != i && both[r][cc]) v += __ddiv_rn((double)agree[r][cc], (double)both[r][cc]);
#pragma unroll
                for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);          // the 32 threads of the row: lanes that differ in tj only
                acc[r] += v;
            }
        }
        flush();
    }
}

// ---- average linkage -----------------------------------------------------------------------------------------------------------------------------------------
constexpr int LK_THREADS = 1024;
constexpr int LK_WAVES = LK_THREADS / kWave;
constexpr int LK_NONE = 0x7fffffff;

struct LkState { int clen, merges, steps; };          // (steps: the launches that pushed or merged -- read by scripts/consensus_bench.py)
struct LkLayout { size_t size, chain, state, total; };

static LkLayout lk_layout(int64_t N) {
    LkLayout o;
    o.size = 0;
    o.chain = align_up((size_t)N * sizeof(int), 256);
    o.state = o.chain + align_up((size_t)N * sizeof(int), 256);
    o.total = o.state + 256;
    return o;
}

__global__ __launch_bounds__(256) void lk_init_kernel(int n, int* size, LkState* st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) size[i] = 1;
    if (i == 0) { st->clen = 0; st->merges = 0; st->steps = 0; }
}

// (nx a + ny b) / (nx + ny) with every operation rounded on its own: hipcc's default contracts a * b + c into an fma (and the __dmul_rn / __dadd_rn of the
// HIP headers are plain * and +, contracted alike), which changes the last bit of a height and with it the order of the merges
__device__ __forceinline__ double lk_average(double nx, double a, double ny, double b, double ns) {
#pragma clang fp contract(off)
    const double pa = nx * a;
    const double pb = ny * b;
    const double sum = pa + pb;
    return sum / ns;
}

__device__ __forceinline__ bool lk_before(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

// minimum of (v, i), lexicographic, over the workgroup; the result in every thread
__device__ __forceinline__ void lk_block_min(double& v, int& i, double* s_v, int* s_i) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (lk_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();          // (an earlier result has been read)
    if (lane == 0) { s_v[w] = v; s_i[w] = i; }
    __syncthreads();
    v = s_v[0]; i = s_i[0];
#pragma unroll
    for (int k = 1; k < LK_WAVES; ++k)
        if (lk_before(s_v[k], s_i[k], v, i)) { v = s_v[k]; i = s_i[k]; }
}

__global__ __launch_bounds__(LK_THREADS) void lk_step_kernel(double* D, int n, int* size, int* chain, LkState* st, double* rec) {
    __shared__ double s_v[LK_WAVES];
    __shared__ int s_i[LK_WAVES];
    const int tid = threadIdx.x;
    const int merges = st->merges;
    int clen = st->clen;
    if (merges >= n - 1) return;
    // everything a thread reads of the state it reads before the first barrier; thread 0 writes the new state behind the last one
    const bool fresh = clen == 0;
    int x, yprev = -1;
    if (fresh) {
        double v = 0.0;
        int first = LK_NONE;
        for (int i = tid; i < n; i += LK_THREADS)
            if (size[i] > 0) { first = i; break; }
        lk_block_min(v, first, s_v, s_i);
        x = first;
        clen = 1;
    } else {
        x = chain[clen - 1];
        if (clen > 1) yprev = chain[clen - 2];
    }
    const double* row = D + (size_t)x * n;
    double bv = __builtin_inf();
    int bi = LK_NONE;
    for (int i0 = tid; i0 < n; i0 += 4 * LK_THREADS) {
        double v[4];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * LK_THREADS;
            live[u] = i < n && i != x && size[i] > 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = live[u] ? row[i0 + u * LK_THREADS] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (live[u] && v[u] < bv) { bv = v[u]; bi = i0 + u * LK_THREADS; }          // (ascending i: a tie keeps the smaller index)
    }
    lk_block_min(bv, bi, s_v, s_i);
    int y = bi;
    double cur = bv;
    if (yprev >= 0) {
        const double dprev = row[yprev];
        if (!(bv < dprev)) { y = yprev; cur = dprev; }          // the previous chain element wins a tie
    }
    if (y == LK_NONE) return;          // (no live row besides x: not reached while merges < n - 1)
    if (yprev < 0 || y != yprev) {
        if (tid == 0 && clen < n) {          // (chain elements are distinct live clusters: clen < n always; no store past the array whatever D holds)
            if (fresh) chain[0] = x;
            chain[clen] = y;
            st->clen = clen + 1;
            st->steps += 1;
        }
        return;
    }
    const int a = min(x, y), b = max(x, y);
    const int na = size[a], nb = size[b];
    const double fa = (double)na, fb = (double)nb, fs = (double)(na + nb);
    double* ra = D + (size_t)a * n;
    double* rb = D + (size_t)b * n;
    for (int i = tid; i < n; i += LK_THREADS) {
        if (i == a || i == b || size[i] <= 0) continue;
        const double v = lk_average(fa, ra[i], fb, rb[i], fs);
        rb[i] = v;
        D[(size_t)i * n + b] = v;
    }
    __syncthreads();          // (every thread has read size[])
    if (tid == 0) {
        double* r = rec + 4 * (size_t)merges;
        r[0] = (double)a; r[1] = (double)b; r[2] = cur; r[3] = fs;
        size[a] = 0;
        size[b] = na + nb;
        st->clen = clen - 2;
        st->merges = merges + 1;
        st->steps += 1;
    }
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_consensus_pairs_workspace(int64_t N, int H, int K) {
    if (N < 2 || N >= (1LL << 30) || H < 1 || H > 65535 || K < 0 || K > CS_MAXK) return 0;
    if (K == 0) return 256;
    return cs_sorted_layout(N, (long)align_up((size_t)H, 16), K).total;
}

int dic_consensus_pairs(const unsigned char* L, long ldl, int64_t N, int H, const int32_t* y, int K, unsigned long long* hist, double* rowsum, double* D,
                        void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(L, DIC_ERR_INVALID_ARG, "consensus_pairs: NULL label matrix");
    DIC_REQUIRE(hist || rowsum || D, DIC_ERR_INVALID_ARG, "consensus_pairs: NULL pointer for every output");
    DIC_REQUIRE(N >= 2 && H >= 1 && ldl >= H, DIC_ERR_INVALID_ARG, "consensus_pairs: N=%lld H=%d ldl=%ld", (long long)N, H, ldl);
    DIC_REQUIRE(ldl % 16 == 0, DIC_ERR_INVALID_ARG, "consensus_pairs: ldl=%ld: expected a multiple of 16", ldl);
    DIC_REQUIRE(!rowsum || (y && workspace), DIC_ERR_INVALID_ARG, "consensus_pairs: rowsum needs y and a workspace: NULL pointer");
    DIC_REQUIRE(!rowsum || (K >= 1 && K <= CS_MAXK), DIC_ERR_INVALID_ARG, "consensus_pairs: K=%d: expected 1..%d", K, CS_MAXK);
    DIC_REQUIRE(H <= 65535, DIC_ERR_UNSUPPORTED, "consensus_pairs: H=%d: at most 65535 resamples", H);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "consensus_pairs: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(((uintptr_t)L & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && (((uintptr_t)hist | (uintptr_t)rowsum | (uintptr_t)D) & 7) == 0 &&
                    ((uintptr_t)y & 3) == 0,
                DIC_ERR_UNSUPPORTED, "consensus_pairs: L and the workspace must be 16-B aligned, the arrays to their element size");
    DIC_REQUIRE(!rowsum || workspace_bytes >= cs_sorted_layout(N, ldl, K).total, DIC_ERR_WORKSPACE, "consensus_pairs: workspace %zu < %zu", workspace_bytes,
                cs_sorted_layout(N, ldl, K).total);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)N;
    const long long nb = (N + CS_T - 1) / CS_T;
    if (hist || D) {
        if (hist) {
            hipError_t e = hipMemsetAsync(hist, 0, (CS_BINS + 1) * sizeof(unsigned long long), st);
            DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "consensus_pairs: memset: %s", hipGetErrorString(e));
        }
        const long long total = nb * (nb + 1) / 2;
        hipLaunchKernelGGL(cs_pairs_kernel, dim3((unsigned)min(total, (long long)kNumCU)), dim3(CS_THREADS), 0, st, L, ldl, n, hist, D);
    }
    if (rowsum) {
        const CsSorted o = cs_sorted_layout(N, ldl, K);
        unsigned char* ws = (unsigned char*)workspace;
        int* count = (int*)(ws + o.count);
        int* start = (int*)(ws + o.start);
        int* ntile = (int*)(ws + o.ntile);
        int* tcl = (int*)(ws + o.tcl);
        int32_t* idx = (int32_t*)(ws + o.idx);
        unsigned char* Ls = ws + o.ls;
        hipError_t e = hipMemsetAsync(count, 0, o.start - o.count, st);
        if (e == hipSuccess) e = hipMemsetAsync(idx, 0xff, o.ls - o.idx, st);          // -1: a padding row
        if (e == hipSuccess) e = hipMemsetAsync(rowsum, 0, (size_t)N * K * sizeof(double), st);          // (a cluster without members has no tile)
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "consensus_pairs: memset: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(cs_count_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, y, n, K, count);
        hipLaunchKernelGGL(cs_starts_kernel, dim3(1), dim3(64), 0, st, (const int*)count, K, start, ntile, tcl);
        hipLaunchKernelGGL(cs_rank_kernel, dim3((unsigned)K), dim3(256), 0, st, y, n, (const int*)start, idx);
        const long long rows = (nb + K) * CS_T, vecs = rows * (ldl / 16);
        hipLaunchKernelGGL(cs_gather_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, L, ldl, (const int32_t*)idx, (const int*)ntile, Ls);
        hipLaunchKernelGGL(cs_rowsum_kernel, dim3((unsigned)min(nb, (long long)kNumCU)), dim3(CS_THREADS), 0, st, L, ldl, n, K, (const unsigned char*)Ls,
                           (const int32_t*)idx, (const int*)ntile, (const int*)tcl, rowsum);
    }
    return check_launch("consensus_pairs");
}

size_t dic_linkage_average_workspace(int64_t N) {
    if (N < 2 || N >= (1LL << 30)) return 0;
    return lk_layout(N).total;
}

int dic_linkage_average(double* D, int64_t N, double* records, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(D && records && workspace, DIC_ERR_INVALID_ARG, "linkage_average: NULL pointer");
    DIC_REQUIRE(N >= 2, DIC_ERR_INVALID_ARG, "linkage_average: N=%lld: expected at least 2 points", (long long)N);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "linkage_average: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE((((uintptr_t)D | (uintptr_t)records) & 7) == 0 && ((uintptr_t)workspace & 15) == 0, DIC_ERR_UNSUPPORTED,
                "linkage_average: D and the records must be 8-B aligned, the workspace 16-B");
    const LkLayout o = lk_layout(N);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "linkage_average: workspace %zu < %zu", workspace_bytes, o.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    int* size = (int*)(ws + o.size);
    int* chain = (int*)(ws + o.chain);
    LkState* state = (LkState*)(ws + o.state);
    const int n = (int)N;
    hipLaunchKernelGGL(lk_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, size, state);
    const long long steps = 3 * (N - 1);
    for (long long s = 0; s < steps; ++s) {
        hipLaunchKernelGGL(lk_step_kernel, dim3(1), dim3(LK_THREADS), 0, st, D, n, size, chain, state, records);
        if ((s & 4095) == 4095) {          // a stream that refuses launches is not fed the rest of them
            const int rc = check_launch("linkage_average");
            if (rc) return rc;
        }
    }
    return check_launch("linkage_average");
}

}  // extern "C"
