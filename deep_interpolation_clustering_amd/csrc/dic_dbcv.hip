// DBCV's two O(N^2) passes (include/dic_hip.h has the definition; dbcv.py the rest): the all-points core distance of every row inside its cluster, and every
// row's nearest internal row of another cluster in mutual-reachability distance.  Both work on the rows sorted by (cluster, row) with a segment table.
//
// ONE TILE LOOP SERVES BOTH.  A workgroup of 256 threads owns 64 consecutive rows (whatever segments they fall in) and walks 64-column tiles; thread
// (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 pairs of rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 as 16 f64 accumulators.  The coordinates of the
// 64 rows and the 64 columns pass through LDS in chunks of 32, stored coordinate-major ([k][row]) so that a thread reads its four rows and its four columns
// of one coordinate as two 16-B loads (a wave reads 4 + 16 distinct addresses, the rest broadcast); a pair's d^2 is the f64 fma chain over the f64
// differences of its f32 coordinates in coordinate order 0 .. D - 1, the same bits wherever and whenever the pair is computed (zero padding adds exactly).
// Per coordinate a thread issues 8 conversions, 16 subtractions and 16 fmas for 16 pairs: the floor of the pass is the 2 D f64 instructions per pair.
// In the core pass column tiles start at multiples of 64 of the sorted order, so which thread slot a pair falls in depends on the two rows alone.
//
// dbcv_core_kernel walks the column tiles that overlap the segments of its rows TWICE: once for m^2, the smallest nonzero d^2 of each row inside its
// segment, once for S = sum (m / d)^dpow.  A thread adds its columns in ascending order; the 16 slots of a row then meet in LDS and are added in slot order
// 0 .. 15 by one thread: the order of every row's sum is a function of the sorted positions alone, there is no atomic, two calls give the same bits.
// THE TERMS LEFT OUT.  A term is exp(dpow / 2 * log(m^2 / d^2)) <= 1 and the term of the nearest member is exactly 1 (the same bits of d^2 in both
// walks), so S >= 1.  A term with m^2 < exp(-120 / dpow) d^2 is below e^-60 = 8.8e-27; fewer than 2^30 of them are dropped, less than 1e-17 of S in all,
// which moves a = m (S / (n - 1))^(-1 / dpow) by less than 1e-17 / dpow relatively -- five orders below the 1e-12 the tests hold a to.  At dpow = 256 that
// spares the log and the exp of every member beyond 1.26 m; at dpow = 8 of none to speak of.
//
// dbcv_sep_kernel walks once over the FLAGGED rows only, as columns: dbcv_collist_kernel first writes their ascending list (at 256 features the trees are
// hub-like and 6-7 % of the rows are internal nodes), and a column tile is 64 entries of the list, its rows gathered -- the staging reads one 16-B piece
// per row and thread either way.  A pair counts where the column lies in another segment; its value is
// max(a_o, a_p, d(o, p)).  Before the coordinates of a tile are touched every thread asks whether max(a_o, a_p) of any of its pairs is below its running
// minimum of that row -- a pair that is not cannot lower it, whatever d is -- and the tile is skipped when no thread says yes (one workgroup vote).  Strict
// updates in ascending column order keep the smallest column among equal values; the 16 slots of a row meet in LDS under (value, column).
#include "dic_common.h"
#include "dic_hip.h"

namespace dic {

constexpr int DV_TILE = 64;          // rows and columns of a tile
constexpr int DV_KC = 32;            // coordinates per LDS chunk
constexpr int DV_THREADS = 256;
constexpr int DV_SLOTS = 16;         // column slots (tx) of a row

typedef float dv_f32x4 __attribute__((ext_vector_type(4)));

struct alignas(16) DvTile {
    float a[DV_KC][DV_TILE];          // rows, coordinate-major
    float b[DV_KC][DV_TILE];          // columns
};

// rows (row0 ..), columns (col0 .., or the rows cidx[0 .. 63] names where cidx is given: an LDS list, -1 for "none") of coordinates kc .. kc + 31 into LDS;
// rows beyond n - 1 repeat row n - 1 and a column "none" is row 0 (neither is ever used), coordinates beyond d are zero
__device__ __forceinline__ void dv_stage(DvTile& t, const float* X, long ldx, int n, int d, int row0, int col0, const int* cidx, int kc) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int f = threadIdx.x + DV_THREADS * j;          // 512 16-B pieces per side
        const int r = f & (DV_TILE - 1), k = 4 * (f >> 6);
        dv_f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
        if (kc + k < d) {
            va = *reinterpret_cast<const dv_f32x4*>(X + (size_t)min(row0 + r, n - 1) * (size_t)ldx + kc + k);
            const int c = cidx ? min(max(cidx[r], 0), n - 1) : min(col0 + r, n - 1);
            vb = *reinterpret_cast<const dv_f32x4*>(X + (size_t)c * (size_t)ldx + kc + k);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t.a[k + q][r] = va[q];
            t.b[k + q][r] = vb[q];
        }
    }
}

// acc[i][j] = d^2(row0 + 4 ty + i, col0 + 4 tx + j) (or column cidx[4 tx + j]).  Every thread of the workgroup calls it (barriers inside); the caller has a
// barrier between its last read of `t` and this call, and between the writes of cidx and this call.
__device__ __forceinline__ void dv_tile_d2(DvTile& t, const float* X, long ldx, int n, int d, int row0, int col0, const int* cidx, double (&acc)[4][4]) {
    const int tx = threadIdx.x & (DV_SLOTS - 1), ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int kc = 0; kc < d; kc += DV_KC) {
        if (kc) __syncthreads();          // (the previous chunk has been read)
        dv_stage(t, X, ldx, n, d, row0, col0, cidx, kc);
        __syncthreads();
        const int kn = min(DV_KC, d - kc);          // a multiple of 4
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const dv_f32x4 ra = *reinterpret_cast<const dv_f32x4*>(&t.a[k][4 * ty]);
            const dv_f32x4 rb = *reinterpret_cast<const dv_f32x4*>(&t.b[k][4 * tx]);
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = (double)ra[q];
                b[q] = (double)rb[q];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double diff = a[i] - b[j];
                    acc[i][j] = fma(diff, diff, acc[i][j]);
                }
        }
    }
}

// rowseg[i] = the segment of sorted row i: the last s with seg_start[s] <= i (seg_start ascending, seg_start[0] = 0, seg_start[K] = n; whatever the
// contents, the result lies in [0, K - 1])
__global__ __launch_bounds__(256) void dbcv_rowseg_kernel(const int32_t* __restrict__ seg_start, int K, int n, int32_t* __restrict__ rowseg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_start[mid] <= i) lo = mid; else hi = mid - 1;
    }
    rowseg[i] = lo;
}

__global__ __launch_bounds__(DV_THREADS) void dbcv_core_kernel(const float* __restrict__ X, long ldx, int n, int d, const int32_t* __restrict__ seg_start,
                                                                int K, const int32_t* __restrict__ rowseg, double dpow, double keep,
                                                                double* __restrict__ a_out) {
    __shared__ DvTile tile;
    __shared__ double s_red[DV_TILE][DV_SLOTS + 1];
    __shared__ double s_m2[DV_TILE];
    __shared__ int s_cseg[DV_TILE];
    const int tid = threadIdx.x, tx = tid & (DV_SLOTS - 1), ty = tid >> 4;
    const int row0 = blockIdx.x * DV_TILE;
    const int last = min(row0 + DV_TILE, n) - 1;
    // the columns of every segment a row of this tile lies in, from a multiple of 64
    const int sa = rowseg[row0], sb = rowseg[last];
    const int c_lo = max(0, min(seg_start[sa], row0)) & ~(DV_TILE - 1);
    const int c_hi = min(n, max(seg_start[min(sb + 1, K)], last + 1));
    int rs[4];
    double m2[4], sum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + 4 * ty + i;
        rs[i] = r < n ? rowseg[r] : -1;
        m2[i] = __builtin_inf();
        sum[i] = 0.0;
    }
    double acc[4][4];
    for (int pass = 0; pass < 2; ++pass) {
        for (int col0 = c_lo; col0 < c_hi; col0 += DV_TILE) {
            __syncthreads();          // (the previous tile's coordinates and segments have been read)
            if (tid < DV_TILE) s_cseg[tid] = col0 + tid < n ? rowseg[col0 + tid] : -2;
            dv_tile_d2(tile, X, ldx, n, d, row0, col0, nullptr, acc);          // (its barriers publish s_cseg too)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d2 = acc[i][j];
                    if (s_cseg[4 * tx + j] != rs[i] || !(d2 > 0.0)) continue;          // another segment, the row itself or a coincident member
                    if (pass == 0) m2[i] = fmin(m2[i], d2);
                    else if (m2[i] >= keep * d2) sum[i] += exp(0.5 * dpow * log(m2[i] / d2));
                }
        }
        // the 16 slots of a row meet: the minimum after the first walk, the sum after the second
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) s_red[4 * ty + i][tx] = pass == 0 ? m2[i] : sum[i];
        __syncthreads();
        if (pass == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double v = s_red[4 * ty + i][0];
                for (int s = 1; s < DV_SLOTS; ++s) v = fmin(v, s_red[4 * ty + i][s]);
                m2[i] = v;
                if (tx == 0) s_m2[4 * ty + i] = v;
            }
        }
    }
    if (tid < DV_TILE && row0 + tid < n) {
        double S = 0.0;
        for (int s = 0; s < DV_SLOTS; ++s) S += s_red[tid][s];          // slot order
        const int seg = rowseg[row0 + tid];
        const double others = (double)(seg_start[seg + 1] - seg_start[seg] - 1);
        // S >= 1 where a member lies at a nonzero distance (its nearest one contributes exactly 1); otherwise a = 0
        a_out[row0 + tid] = S > 0.0 ? sqrt(s_m2[tid]) * pow(S / others, -1.0 / dpow) : 0.0;
    }
}

// The flagged rows, ascending, and their number: ONE workgroup of 1024 threads, each counting a contiguous run of flags, an inclusive scan of the 1024
// counts in LDS, then each thread writes its run's entries behind those of the runs before it.
constexpr int DV_LIST_THREADS = 1024;
__global__ __launch_bounds__(DV_LIST_THREADS) void dbcv_collist_kernel(const unsigned char* __restrict__ internal, int n, int32_t* __restrict__ list,
                                                                       int32_t* __restrict__ count) {
    __shared__ int s_sum[DV_LIST_THREADS];
    const int tid = threadIdx.x;
    const int per = (n + DV_LIST_THREADS - 1) / DV_LIST_THREADS;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += internal[i] != 0;
    s_sum[tid] = mine;
    __syncthreads();
    for (int off = 1; off < DV_LIST_THREADS; off <<= 1) {
        const int v = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int at = s_sum[tid] - mine;          // (at + mine <= the number of flags <= n: every write lies inside list[0 .. n - 1])
    for (int i = lo; i < hi; ++i)
        if (internal[i] != 0) list[at++] = i;
    if (tid == DV_LIST_THREADS - 1) *count = s_sum[tid];
}

__global__ __launch_bounds__(DV_THREADS) void dbcv_sep_kernel(const float* __restrict__ X, long ldx, int n, int d, const int32_t* __restrict__ rowseg,
                                                               const double* __restrict__ a, const int32_t* __restrict__ list,
                                                               const int32_t* __restrict__ count, double* __restrict__ rowsep,
                                                               int32_t* __restrict__ rowarg) {
    __shared__ DvTile tile;
    __shared__ double s_red[DV_TILE][DV_SLOTS + 1];
    __shared__ int s_arg[DV_TILE][DV_SLOTS + 1];
    __shared__ double s_ca[DV_TILE];
    __shared__ int s_cseg[DV_TILE];
    __shared__ int s_cidx[DV_TILE];
    const int tid = threadIdx.x, tx = tid & (DV_SLOTS - 1), ty = tid >> 4;
    const int row0 = blockIdx.x * DV_TILE;
    const int ncol = min(max(*count, 0), n);          // the flagged rows: list[0 .. ncol - 1], ascending
    int rs[4], arg[4];
    double ra[4], best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + 4 * ty + i;
        rs[i] = r < n ? rowseg[r] : -2;          // (a row beyond the end matches no column: -2 is the mark of a column that does not count)
        ra[i] = r < n ? a[r] : 0.0;
        best[i] = __builtin_inf();
        arg[i] = -1;
    }
    double acc[4][4];
    for (int col0 = 0; col0 < ncol; col0 += DV_TILE) {
        __syncthreads();          // (the previous tile's coordinates, rows, segments and a have been read)
        if (tid < DV_TILE) {
            int c = col0 + tid < ncol ? list[col0 + tid] : -1;
            if ((unsigned)c >= (unsigned)n) c = -1;
            s_cidx[tid] = c;
            s_cseg[tid] = c >= 0 ? rowseg[c] : -2;
            s_ca[tid] = c >= 0 ? a[c] : 0.0;
        }
        __syncthreads();
        bool mine = false;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cs = s_cseg[4 * tx + j];
                mine |= cs != -2 && rs[i] != -2 && cs != rs[i] && fmax(ra[i], s_ca[4 * tx + j]) < best[i];
            }
        if (!__syncthreads_or(mine)) continue;          // no pair of this tile can lower a running minimum
        dv_tile_d2(tile, X, ldx, n, d, row0, col0, s_cidx, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cs = s_cseg[4 * tx + j];
                if (cs == -2 || rs[i] == -2 || cs == rs[i]) continue;
                const double v = fmax(fmax(ra[i], s_ca[4 * tx + j]), sqrt(acc[i][j]));
                if (v < best[i]) {
                    best[i] = v;
                    arg[i] = s_cidx[4 * tx + j];
                }
            }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s_red[4 * ty + i][tx] = best[i];
        s_arg[4 * ty + i][tx] = arg[i];
    }
    __syncthreads();
    if (tid < DV_TILE && row0 + tid < n) {
        double bv = s_red[tid][0];
        int bi = s_arg[tid][0];
        for (int s = 1; s < DV_SLOTS; ++s) {
            const double v = s_red[tid][s];
            const int c = s_arg[tid][s];
            if (c >= 0 && (bi < 0 || v < bv || (v == bv && c < bi))) { bv = v; bi = c; }
        }
        rowsep[row0 + tid] = bi >= 0 ? bv : __builtin_inf();
        rowarg[row0 + tid] = bi;
    }
}

static int dbcv_check(const char* who, const float* X, long ldx, int64_t N, int D, const int32_t* seg_start, int64_t K, void* workspace, size_t workspace_bytes) {
    DIC_REQUIRE(X && seg_start && workspace, DIC_ERR_INVALID_ARG, "%s: NULL pointer", who);
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D && K >= 1 && K <= N, DIC_ERR_INVALID_ARG, "%s: N=%lld D=%d ldx=%ld K=%lld", who, (long long)N, D, ldx, (long long)K);
    DIC_REQUIRE(D <= 4 * kWave && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "%s: D=%d (row stride %ld): at most %d, multiples of 4", who, D, ldx, 4 * kWave);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: N=%lld: fewer than 2^30 rows", who, (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)seg_start & 3) == 0, DIC_ERR_UNSUPPORTED,
                "%s: X and the workspace must be 16-B aligned, the segment table to 4 B", who);
    const size_t need = dic_dbcv_workspace(N, K);
    DIC_REQUIRE(workspace_bytes >= need, DIC_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_dbcv_workspace(int64_t N, int64_t K) {
    if (N <= 0 || N >= (1LL << 30) || K < 1 || K > N) return 0;
    return 2 * align_up((size_t)N * sizeof(int32_t), 256) + 256;          // the rows' segments, the list of flagged rows, its length
}

int dic_dbcv_core(const float* X, long ldx, int64_t N, int D, const int32_t* seg_start, int64_t K, double dpow, double* a, void* workspace,
                  size_t workspace_bytes, dic_stream_t stream) {
    const int rc = dbcv_check("dbcv_core", X, ldx, N, D, seg_start, K, workspace, workspace_bytes);
    if (rc) return rc;
    DIC_REQUIRE(a && ((uintptr_t)a & 7) == 0, DIC_ERR_INVALID_ARG, "dbcv_core: a must be an 8-B aligned pointer");
    DIC_REQUIRE(dpow >= 1.0 && dpow <= 65536.0, DIC_ERR_INVALID_ARG, "dbcv_core: dpow=%g: expected 1 <= dpow <= 65536", dpow);
    int32_t* rowseg = (int32_t*)workspace;
    hipLaunchKernelGGL(dbcv_rowseg_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg_start, (int)K, (int)N, rowseg);
    hipLaunchKernelGGL(dbcv_core_kernel, dim3((unsigned)((N + DV_TILE - 1) / DV_TILE)), dim3(DV_THREADS), 0, (hipStream_t)stream, X, ldx, (int)N, D, seg_start,
                       (int)K, (const int32_t*)rowseg, dpow, exp(-120.0 / dpow), a);
    return check_launch("dbcv_core");
}

int dic_dbcv_separation(const float* X, long ldx, int64_t N, int D, const int32_t* seg_start, int64_t K, const double* a, const unsigned char* internal,
                        double* rowsep, int32_t* rowarg, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    const int rc = dbcv_check("dbcv_separation", X, ldx, N, D, seg_start, K, workspace, workspace_bytes);
    if (rc) return rc;
    DIC_REQUIRE(a && internal && rowsep && rowarg, DIC_ERR_INVALID_ARG, "dbcv_separation: NULL pointer");
    DIC_REQUIRE((((uintptr_t)a | (uintptr_t)rowsep) & 7) == 0 && ((uintptr_t)rowarg & 3) == 0, DIC_ERR_UNSUPPORTED,
                "dbcv_separation: the arrays must be aligned to their element size");
    int32_t* rowseg = (int32_t*)workspace;
    hipLaunchKernelGGL(dbcv_rowseg_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg_start, (int)K, (int)N, rowseg);
    int32_t* list = (int32_t*)((unsigned char*)workspace + align_up((size_t)N * sizeof(int32_t), 256));
    int32_t* count = (int32_t*)((unsigned char*)workspace + 2 * align_up((size_t)N * sizeof(int32_t), 256));
    hipLaunchKernelGGL(dbcv_collist_kernel, dim3(1), dim3(DV_LIST_THREADS), 0, (hipStream_t)stream, internal, (int)N, list, count);
    hipLaunchKernelGGL(dbcv_sep_kernel, dim3((unsigned)((N + DV_TILE - 1) / DV_TILE)), dim3(DV_THREADS), 0, (hipStream_t)stream, X, ldx, (int)N, D,
                       (const int32_t*)rowseg, a, (const int32_t*)list, (const int32_t*)count, rowsep, rowarg);
    return check_launch("dbcv_separation");
}

}  // extern "C"
