// Agreement of two labellings (sklearn.metrics.cluster: contingency table, pair counts, mutual information, entropies and the EXPECTED mutual information of
// the permutation model) for MANY pairs of labellings at once.  The definitions, the grouping of every floating-point expression and the order of every sum
// are stated once, in include/dic_hip.h; this file holds to them.  agreement.py forms every index from what the three stages return.
//
// A pair is a row of the descriptor table `desc` (P, 8) int64 DEVICE: {la, lb, Ka, Kb, table_off, marg_off, part_off, 0} -- the two rows of the code matrix,
// their class counts and where the pair's table (Ka x Kb int32, row-major), its marginals (Ka + Kb int64) and its EMI partials (Ka * ceil(Kb / 64) doubles)
// start in the caller's three buffers.  A pair is the second grid dimension of every kernel: a sweep is one launch per stage (per 65535 pairs).  A descriptor
// that points outside a buffer or names a labelling that is not there is SKIPPED by every kernel (pair_of below): no wild access whatever the table holds.
//
// Integers are added with integer atomics (LDS and global), which commute: the tables and every integer sum are exact and two calls give the same bits.
// Every floating-point sum has a fixed order (agreement_sums_kernel, agreement_emi_kernel) and there is no floating-point atomic.  Contraction into fma is
// switched off for the whole file, so that a * b + c * d rounds as it reads and the numpy restatement of the header (tests/agreement_reference.py) forms the
// same expressions.
#include <algorithm>

#include "dic_common.h"

#pragma clang fp contract(off)

namespace dic {

// LDS budget of the table histogram: 16384 int32 cells = 64 KB of the 160 KB of a gfx950 workgroup processor, so that two workgroups share a CU (a
// histogram's atomics wait on LDS latency, which the second workgroup hides).  Tables of up to 128 x 128 classes fit; agreement.py exposes the figure.
constexpr int AG_LDS_CELLS = 16384;
constexpr int AG_ROWS = 4096;             // rows of the label matrix per workgroup: 16 per thread
constexpr int AG_EMI_COLS = 64;           // columns of the table per EMI work unit (one wave)
constexpr int AG_EMI_SMALL = 32;          // a row with a_i <= this walks its columns lane per column (ranges of n of at most a_i terms), else lane per n
constexpr int AG_DESC = 8;                // int64 words per descriptor
// exp(g) is EXACTLY 0 for g < ln(2^-1075) = -745.13..: below half the smallest subnormal a correctly rounded result is 0, and an exp that is wrong by a few
// ulp cannot cross the 0.87 between that and -746.  A term with g < -746 is therefore a product with an exact 0 and adds +0.0 or -0.0 to a sum that started
// at +0.0: leaving it out changes no bit.
constexpr double AG_EXP_ZERO = -746.0;

struct AgPair {
    int la, lb, Ka, Kb;
    long long toff, moff, poff;
    bool ok;
};

__device__ __forceinline__ AgPair pair_of(const int64_t* __restrict__ desc, long long p, long long L, long long total_cells, long long total_marg) {
    const int64_t* d = desc + p * AG_DESC;
    const long long la = d[0], lb = d[1], Ka = d[2], Kb = d[3];
    AgPair r;
    r.toff = d[4], r.moff = d[5], r.poff = d[6];
    r.ok = la >= 0 && la < L && lb >= 0 && lb < L && Ka >= 1 && Kb >= 1 && Ka < (1LL << 30) && Kb < (1LL << 30) && r.toff >= 0 && r.moff >= 0 && r.poff >= 0 &&
           Ka * Kb <= total_cells - r.toff && Ka + Kb <= total_marg - r.moff;
    r.la = (int)la, r.lb = (int)lb, r.Ka = (int)Ka, r.Kb = (int)Kb;
    return r;
}

// ---- stage 1: contingency tables ----------------------------------------------------------------------------------------------------------------------------
// grid (row chunks, pairs).  A row whose code lies outside [0, K) is skipped (the caller encodes; nothing is read or written outside the table), and so is a
// row whose code equals its labelling's drop code (noise = 'drop').
__global__ __launch_bounds__(256) void agreement_tables_kernel(const int32_t* __restrict__ codes, long long ld, long long L, long long N,
                                                               const int32_t* __restrict__ drop, const int64_t* __restrict__ desc, long long pbase,
                                                               int32_t* __restrict__ tables, long long total_cells) {
    __shared__ int hist[AG_LDS_CELLS];
    const AgPair q = pair_of(desc, pbase + blockIdx.y, L, total_cells, 1LL << 62);
    if (!q.ok) return;
    const long long r0 = (long long)blockIdx.x * AG_ROWS, r1 = min(N, r0 + AG_ROWS);
    const int32_t* __restrict__ ca = codes + q.la * ld;
    const int32_t* __restrict__ cb = codes + q.lb * ld;
    const int da = drop ? drop[q.la] : -1, db = drop ? drop[q.lb] : -1;
    int32_t* __restrict__ T = tables + q.toff;
    const long long cells = (long long)q.Ka * q.Kb;
    if (cells <= AG_LDS_CELLS) {
        for (int c = threadIdx.x; c < (int)cells; c += 256) hist[c] = 0;
        __syncthreads();
        for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
            const int a = ca[r], b = cb[r];
            if ((unsigned)a < (unsigned)q.Ka && (unsigned)b < (unsigned)q.Kb && a != da && b != db) atomicAdd(&hist[a * q.Kb + b], 1);
        }
        __syncthreads();
        for (int c = threadIdx.x; c < (int)cells; c += 256) {
            const int v = hist[c];
            if (v) atomicAdd(&T[c], v);
        }
    } else {
        for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
            const int a = ca[r], b = cb[r];
            if ((unsigned)a < (unsigned)q.Ka && (unsigned)b < (unsigned)q.Kb && a != da && b != db) atomicAdd(&T[(long long)a * q.Kb + b], 1);
        }
    }
}

// ---- stage 2: marginals, integer sums, MI and the entropies -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the 256 per-thread sums added by a binary tree: stride 128, 64, .., 1 (the order the header states); the result in every thread
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// one workgroup per pair
__global__ __launch_bounds__(256) void agreement_sums_kernel(const int32_t* __restrict__ tables, long long total_cells, const int64_t* __restrict__ desc,
                                                             long long L, long long pbase, int64_t* __restrict__ marg, long long total_marg,
                                                             int64_t* __restrict__ isums, double* __restrict__ fsums) {
    __shared__ unsigned long long isum[4];
    __shared__ double red[256];
    const long long p = pbase + blockIdx.x;
    const AgPair q = pair_of(desc, p, L, total_cells, total_marg);
    if (!q.ok) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ T = tables + q.toff;
    int64_t* A = marg + q.moff;
    int64_t* B = A + q.Ka;
    if (tid < 4) isum[tid] = 0;
    __syncthreads();
    // row marginals and sum n^2: a wave per row, lanes along it
    unsigned long long sq = 0;
    for (int i = wave; i < q.Ka; i += 4) {
        const int32_t* row = T + (long long)i * q.Kb;
        int s = 0;
        for (int j = lane; j < q.Kb; j += 64) {
            const int v = row[j];
            s += v;
            sq += (unsigned long long)((long long)v * v);
        }
        s = wave_sum_int(s);
        if (lane == 0) A[i] = s;
    }
    // column marginals: a thread per column, coalesced along the rows of the table
    for (int j = tid; j < q.Kb; j += 256) {
        long long s = 0;
        for (int i = 0; i < q.Ka; ++i) s += T[(long long)i * q.Kb + j];
        B[j] = s;
    }
    __syncthreads();          // (the marginals are read back below by other threads of this workgroup)
    unsigned long long sa = 0, sb = 0, sn = 0;
    for (int i = tid; i < q.Ka; i += 256) {
        const unsigned long long a = (unsigned long long)A[i];
        sa += a * a;
        sn += a;
    }
    for (int j = tid; j < q.Kb; j += 256) {
        const unsigned long long b = (unsigned long long)B[j];
        sb += b * b;
    }
    if (sq) atomicAdd(&isum[0], sq);
    if (sa) atomicAdd(&isum[1], sa);
    if (sb) atomicAdd(&isum[2], sb);
    if (sn) atomicAdd(&isum[3], sn);
    __syncthreads();
    if (tid < 4) isums[p * 4 + tid] = (int64_t)isum[tid];
    const long long Np = (long long)isum[3];
    const double Nd = (double)Np, logN = log(Nd);
    // MI: thread t adds the cells c = t, t + 256, .. of the row-major table in ascending order
    double mi = 0.0;
    const long long cells = (long long)q.Ka * q.Kb;
    for (long long c = tid; c < cells; c += 256) {
        const int v = T[c];
        if (v > 0) {
            const int i = (int)(c / q.Kb), j = (int)(c - (long long)i * q.Kb);
            const double nn = (double)v, cnm = nn / Nd;
            const double log_outer = (-log((double)(A[i] * B[j])) + logN) + logN;
            double t = cnm * (log(nn) - logN) + cnm * log_outer;
            if (fabs(t) < 2.220446049250313e-16) t = 0.0;
            mi += t;
        }
    }
    mi = block_tree_sum(mi, red);
    double ha = 0.0, hb = 0.0;
    for (int i = tid; i < q.Ka; i += 256) {
        const long long a = A[i];
        if (a > 0) ha += ((double)a / Nd) * (log((double)a) - logN);
    }
    ha = block_tree_sum(ha, red);
    for (int j = tid; j < q.Kb; j += 256) {
        const long long b = B[j];
        if (b > 0) hb += ((double)b / Nd) * (log((double)b) - logN);
    }
    hb = block_tree_sum(hb, red);
    if (tid == 0) {
        fsums[p * 3 + 0] = mi;
        fsums[p * 3 + 1] = -ha;
        fsums[p * 3 + 2] = -hb;
    }
}

// ---- stage 3: expected mutual information -------------------------------------------------------------------------------------------------------------------
// One cell's terms n = n0, n0 + step, .. <= hi, added to acc in that order.  c0 = ((lf[a] + lf[b]) + lf[N - a]) + lf[N - b].  Every index into lf lies in
// [0, N]: lo = max(1, a + b - N) <= n <= min(a, b).
__device__ __forceinline__ double emi_cell(double acc, const double* __restrict__ lf, long long a, long long b, long long Np, long long n0, long long hi,
                                           int step, double c0, double lfN, double Nd, double logN, double log_a, double log_b) {
    const long long rest = Np - a - b;
    for (long long n = n0; n <= hi; n += step) {
        const double g = (((c0 - (lf[n] + lfN)) - lf[a - n]) - lf[b - n]) - lf[rest + n];
        if (g >= AG_EXP_ZERO) {
            const double nd = (double)n;
            const double t2 = ((logN + log(nd)) - log_a) - log_b;
            acc += ((nd / Nd) * t2) * exp(g);
        }
    }
    return acc;
}

// grid (ceil(max units / 4), pairs), a wave per unit: unit u = i * nchunk + c is row i of the table and its columns c * 64 .. c * 64 + 63
__global__ __launch_bounds__(256) void agreement_emi_kernel(const int64_t* __restrict__ marg, long long total_marg, const int64_t* __restrict__ desc,
                                                            long long L, long long pbase, const int64_t* __restrict__ isums, const double* __restrict__ lf,
                                                            long long lf_len, double* __restrict__ partials, long long total_units) {
    const long long p = pbase + blockIdx.y;
    const AgPair q = pair_of(desc, p, L, 1LL << 62, total_marg);
    if (!q.ok) return;
    const int lane = threadIdx.x & 63;
    const long long nchunk = (q.Kb + AG_EMI_COLS - 1) / AG_EMI_COLS, units = q.Ka * nchunk;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= units || units > total_units - q.poff) return;
    const int i = (int)(u / nchunk), j0 = (int)(u - i * nchunk) * AG_EMI_COLS, j1 = min(q.Kb, j0 + AG_EMI_COLS);
    const int64_t* __restrict__ A = marg + q.moff;
    const int64_t* __restrict__ B = A + q.Ka;
    const long long Np = isums[p * 4 + 3], a = A[i];
    double acc = 0.0;
    if (Np >= lf_len || a > Np || a < 0) {
        acc = __builtin_nan("");          // (a table of factorials too short for this pair, or marginals that are not this table's)
    } else if (a > 0) {
        const double Nd = (double)Np, logN = log(Nd), log_a = log((double)a), lfN = lf[Np], ga = lf[a], gNa = lf[Np - a];
        if (a <= AG_EMI_SMALL) {
            const int j = j0 + lane;
            const long long b = j < j1 ? B[j] : 0;
            if (b > 0 && b <= Np) {
                const double c0 = ((ga + lf[b]) + gNa) + lf[Np - b];
                acc = emi_cell(acc, lf, a, b, Np, max(1LL, a + b - Np), min(a, b), 1, c0, lfN, Nd, logN, log_a, log((double)b));
            }
        } else {
            for (int j = j0; j < j1; ++j) {
                const long long b = B[j];
                if (b > 0 && b <= Np) {
                    const double c0 = ((ga + lf[b]) + gNa) + lf[Np - b];
                    acc = emi_cell(acc, lf, a, b, Np, max(1LL, a + b - Np) + lane, min(a, b), 64, c0, lfN, Nd, logN, log_a, log((double)b));
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) partials[q.poff + u] = acc;
}

// one workgroup per pair: thread t adds the partials u = t, t + 256, .. in ascending order, then the tree
__global__ __launch_bounds__(256) void agreement_emi_finish_kernel(const int64_t* __restrict__ desc, long long L, long long pbase, long long total_marg,
                                                                   const double* __restrict__ partials, long long total_units, double* __restrict__ emi) {
    __shared__ double red[256];
    const long long p = pbase + blockIdx.x;
    const AgPair q = pair_of(desc, p, L, 1LL << 62, total_marg);
    if (!q.ok) return;
    const long long units = q.Ka * (long long)((q.Kb + AG_EMI_COLS - 1) / AG_EMI_COLS);
    if (units > total_units - q.poff) return;
    double s = 0.0;
    for (long long u = threadIdx.x; u < units; u += 256) s += partials[q.poff + u];
    s = block_tree_sum(s, red);
    if (threadIdx.x == 0) emi[p] = s;
}

constexpr long long AG_MAX_GRID_Y = 65535;

static int agreement_check(const char* what, const void* desc, int64_t L, int64_t P) {
    DIC_REQUIRE(desc, DIC_ERR_INVALID_ARG, "%s: NULL pointer", what);
    DIC_REQUIRE(L >= 1 && P >= 1, DIC_ERR_INVALID_ARG, "%s: L=%lld P=%lld: expected positive sizes", what, (long long)L, (long long)P);
    DIC_REQUIRE(L < (1LL << 24) && P < (1LL << 24), DIC_ERR_UNSUPPORTED, "%s: L=%lld P=%lld: fewer than 2^24 labellings and pairs", what, (long long)L,
                (long long)P);
    DIC_REQUIRE(((uintptr_t)desc & 7) == 0, DIC_ERR_UNSUPPORTED, "%s: operands must be aligned to their element size", what);
    return DIC_OK;
}

}  // namespace dic

using namespace dic;

extern "C" {

int dic_agreement_lds_cells(void) { return AG_LDS_CELLS; }

size_t dic_agreement_workspace(int64_t total_units) { return total_units < 1 || total_units >= (1LL << 40) ? 0 : align_up((size_t)total_units * 8, 16); }

int dic_agreement_tables(const int32_t* codes, int64_t ld, int64_t L, int64_t N, const int32_t* drop, const int64_t* desc, int64_t P, int32_t* tables,
                         int64_t total_cells, dic_stream_t stream) {
    DIC_REQUIRE(codes && tables, DIC_ERR_INVALID_ARG, "agreement_tables: NULL pointer");
    int rc = agreement_check("agreement_tables", desc, L, P);
    if (rc) return rc;
    DIC_REQUIRE(N >= 1 && ld >= N && total_cells >= 1, DIC_ERR_INVALID_ARG, "agreement_tables: N=%lld ld=%lld total_cells=%lld: expected 1 <= N <= ld, cells",
                (long long)N, (long long)ld, (long long)total_cells);
    DIC_REQUIRE(N < (1LL << 31) && total_cells < (1LL << 40), DIC_ERR_UNSUPPORTED, "agreement_tables: N=%lld total_cells=%lld: counts are int32", (long long)N,
                (long long)total_cells);
    DIC_REQUIRE(((uintptr_t)codes & 3) == 0 && ((uintptr_t)tables & 3) == 0 && ((uintptr_t)drop & 3) == 0, DIC_ERR_UNSUPPORTED,
                "agreement_tables: operands must be aligned to their element size");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(tables, 0, (size_t)total_cells * 4, st) != hipSuccess) return check_launch("agreement_tables (memset)");
    const unsigned chunks = (unsigned)((N + AG_ROWS - 1) / AG_ROWS);
    for (long long p0 = 0; p0 < P; p0 += AG_MAX_GRID_Y)
        hipLaunchKernelGGL(agreement_tables_kernel, dim3(chunks, (unsigned)std::min<long long>(AG_MAX_GRID_Y, P - p0)), dim3(256), 0, st, codes, (long long)ld,
                           (long long)L, (long long)N, drop, desc, p0, tables, (long long)total_cells);
    return check_launch("agreement_tables");
}

int dic_agreement_sums(const int32_t* tables, int64_t total_cells, const int64_t* desc, int64_t L, int64_t P, int64_t* marg, int64_t total_marg,
                       int64_t* isums, double* fsums, dic_stream_t stream) {
    DIC_REQUIRE(tables && marg && isums && fsums, DIC_ERR_INVALID_ARG, "agreement_sums: NULL pointer");
    int rc = agreement_check("agreement_sums", desc, L, P);
    if (rc) return rc;
    DIC_REQUIRE(total_cells >= 1 && total_marg >= 2, DIC_ERR_INVALID_ARG, "agreement_sums: total_cells=%lld total_marg=%lld: expected positive sizes",
                (long long)total_cells, (long long)total_marg);
    DIC_REQUIRE(((uintptr_t)tables & 3) == 0 && ((uintptr_t)marg & 7) == 0 && ((uintptr_t)isums & 7) == 0 && ((uintptr_t)fsums & 7) == 0, DIC_ERR_UNSUPPORTED,
                "agreement_sums: operands must be aligned to their element size");
    hipLaunchKernelGGL(agreement_sums_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, tables, (long long)total_cells, desc, (long long)L, 0LL,
                       marg, (long long)total_marg, isums, fsums);
    return check_launch("agreement_sums");
}

int dic_agreement_emi(const int64_t* marg, int64_t total_marg, const int64_t* desc, int64_t L, int64_t P, int64_t max_units, const int64_t* isums,
                      const double* lf, int64_t lf_len, double* emi, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(marg && isums && lf && emi && workspace, DIC_ERR_INVALID_ARG, "agreement_emi: NULL pointer");
    int rc = agreement_check("agreement_emi", desc, L, P);
    if (rc) return rc;
    DIC_REQUIRE(total_marg >= 2 && max_units >= 1 && lf_len >= 2, DIC_ERR_INVALID_ARG, "agreement_emi: total_marg=%lld max_units=%lld lf_len=%lld",
                (long long)total_marg, (long long)max_units, (long long)lf_len);
    DIC_REQUIRE(max_units < (1LL << 26), DIC_ERR_UNSUPPORTED, "agreement_emi: max_units=%lld: fewer than 2^26 units per pair", (long long)max_units);
    DIC_REQUIRE(((uintptr_t)marg & 7) == 0 && ((uintptr_t)isums & 7) == 0 && ((uintptr_t)lf & 7) == 0 && ((uintptr_t)emi & 7) == 0 &&
                    ((uintptr_t)workspace & 15) == 0,
                DIC_ERR_UNSUPPORTED, "agreement_emi: operands must be aligned to their element size, the workspace to 16 bytes");
    DIC_REQUIRE(workspace_bytes >= 8, DIC_ERR_WORKSPACE, "agreement_emi: workspace of %zu bytes", workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long total_units = (long long)(workspace_bytes / 8);
    double* partials = (double*)workspace;
    for (long long p0 = 0; p0 < P; p0 += AG_MAX_GRID_Y)
        hipLaunchKernelGGL(agreement_emi_kernel, dim3((unsigned)((max_units + 3) / 4), (unsigned)std::min<long long>(AG_MAX_GRID_Y, P - p0)), dim3(256), 0, st,
                           marg, (long long)total_marg, desc, (long long)L, p0, isums, lf, (long long)lf_len, partials, total_units);
    hipLaunchKernelGGL(agreement_emi_finish_kernel, dim3((unsigned)P), dim3(256), 0, st, desc, (long long)L, 0LL, (long long)total_marg, partials, total_units,
                       emi);
    return check_launch("agreement_emi");
}

}  // extern "C"
