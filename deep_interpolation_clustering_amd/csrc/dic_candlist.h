// The candidate-list machine of the k-th neighbour distances and neighbour lists (dic_knn.hip) and the neighbour ranks (dic_knn_rank.hip): the pair-tile
// loop's approximate d^2, a_ij (dic_pairtile.h), only decides which pairs an exact f64 stage has to look at.  THE PROTOCOL, the same for every caller:
//   COUNTS    tile passes with the counting epilogue KnCount<T>: cnt[i][q] += #{j : a_ij <= thr[i][q]} for the caller's per-row thresholds.
//   LENGTHS   a row's list length is a difference of such counts (or a sum of differences), so it is known exactly before anything is listed.
//   OFFSETS   cl_scan_kernel: off[0..n] = the exclusive prefix sum of the lengths, their total and the longest (ClPlan), on the device.
//   GROUPS    cl_groups_kernel: consecutive rows, as many as fit the `entries` slots of the candidate buffer.  The host reads the plan and the bounds back.
//   GATHER    per group, the caller's gather epilogue walks the tiles of the group's row blocks again, makes the comparisons the counting pass made on the
//             same a values and appends to row i's list: entries off[i] - off[r0] .. of the buffer, the slot inside a list from an integer atomic cursor.
//   EXACT     per group, the caller's exact kernel, one workgroup per row, judges every list entry by its f64 difference-form d^2 (dic_exactd2.h).
// cl_run_groups is the host half from the scan on.  THE BUDGET (candidate_budget, bytes; entries = budget / entry size, at least 1, at most every pair) sizes
// the groups and nothing else: the lists, their contents and the results are the same for every budget that holds the longest list, and one that does not is
// refused before anything is gathered, stats[4] = budget_needed saying how much would do.  GUARDS that keep a write inside its list, whatever the data
// (non-finite coordinates make the two passes' comparisons meaningless, not unsafe): a gather epilogue writes slot `pos` of a list only while pos is below
// the COUNTED length and the offset below `entries`; the host checks every group's bounds before it launches on them; an exact kernel checks its list's
// offset and length against `entries` and every entry's index against n before it reads through them, and raises plan->flag, which the host reads last.
// The order a list was filled in never matters: every caller's exact stage judges entries by value.  The only atomics are integer adds.
#pragma once
#include <cstdio>
#include "dic_pairtile.h"

namespace dic {

struct KnTileArgs {
    PtPairArgs p;
    const float* thr; int32_t* cnt;                               // counting: (rows, T) thresholds and counts
    const long long* off; int32_t* cursor; int32_t* idx; int r0, r1; long long entries;          // gather
};

// Counting epilogue: cnt[i][q] += #{j : a_ij <= thr[i][q]}.  The product loop leaves few registers free (128 accumulators + 72 operand registers of 256), so
// a row's thresholds are reloaded for every tile (64 B per row, from L2) instead of living through the loop, and the running counts stay in registers as
// 16-bit halves, two thresholds per register: a tile adds at most 64 to a lane's count, so KN_FLUSH_TILES tiles cannot overflow one, and the counts go to
// memory (integer atomics) when the row block changes or after that many tiles.
constexpr int KN_FLUSH_TILES = 1000;
static_assert(KN_FLUSH_TILES * 64 < 65536, "knn: packed counters");

template <int T>
struct KnCount {
    static_assert(T % 2 == 0, "knn: thresholds come in pairs");
    const KnTileArgs& a;
    const PtLane ln;
    int cur_i = -1, tiles = 0;
    unsigned pk[2][T / 2];

    __device__ __forceinline__ KnCount(const KnTileArgs& args) : a(args), ln() {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int q = 0; q < T / 2; ++q) pk[mb][q] = 0u;
    }
    __device__ __forceinline__ void flush() {
        if (cur_i < 0) return;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(cur_i, mb);
#pragma unroll
            for (int q = 0; q < T; ++q) {
                const int own = (int)((pk[mb][q / 2] >> (16 * (q & 1))) & 0xffffu);
                const int v = own + __shfl_xor(own, 32);
                if (ln.hh == 0 && gi < a.p.n && v) atomicAdd(a.cnt + (size_t)gi * T + q, v);
            }
#pragma unroll
            for (int q = 0; q < T / 2; ++q) pk[mb][q] = 0u;
        }
        tiles = 0;
    }
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        if (I0 != cur_i || tiles == KN_FLUSH_TILES) {
            flush();
            cur_i = I0;
        }
        ++tiles;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int gi = ln.row(I0, mb);
            float t[T];
            if constexpr (T % 4 == 0) {
#pragma unroll
                for (int q = 0; q < T; q += 4) {
                    const pf32x4 v = *reinterpret_cast<const pf32x4*>(a.thr + (size_t)gi * T + q);          // (gi < n + 256: inside the array)
                    t[q] = v[0]; t[q + 1] = v[1]; t[q + 2] = v[2]; t[q + 3] = v[3];
                }
            } else {
#pragma unroll
                for (int q = 0; q < T; ++q) t[q] = a.thr[(size_t)gi * T + q];
            }
            int c[T];
#pragma unroll
            for (int q = 0; q < T; ++q) c[q] = 0;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const float d2 = acc[nb][mb][k];          // (a padding point j is beyond every threshold: PT_PAD_NORM; a padding row i is never flushed)
#pragma unroll
                    for (int q = 0; q < T; ++q) c[q] += (int)(d2 <= t[q]);
                }
#pragma unroll
            for (int q = 0; q < T / 2; ++q) pk[mb][q] += (unsigned)c[2 * q] | ((unsigned)c[2 * q + 1] << 16);
        }
    }
};

// (The two gather epilogues, KnGather and KrGather, stay with their callers, each with its own copy of the loop that builds a row half's 64-pair membership
// mask: shared through a function the loop compiles to different code in both tile kernels.)

constexpr long long CL_DEFAULT_BUDGET = 384LL << 20;         // bytes (list sizes at 75 000 x 256)
struct ClPlan { long long total, longest, groups; int flag; };          // device words the host reads back

// nmax = the largest norm (one workgroup over the block maxima)
static __global__ __launch_bounds__(256) void cl_gmax_kernel(const float* bmax, int nblk, float* gmax) {
    __shared__ float part[4];
    float v = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) v = fmaxf(v, bmax[i]);
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *gmax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// where a row's list length comes from: the two counts of its window (stride 2), or an array
struct ClWindowLen {
    const int32_t* cnt;
    __device__ __forceinline__ long long operator()(int i) const { return (long long)cnt[(size_t)i * 2 + 1] - cnt[(size_t)i * 2]; }
};
struct ClArrayLen {
    const long long* len;
    __device__ __forceinline__ long long operator()(int i) const { return len[i]; }
};

// List lengths -> off[0..n] (exclusive prefix sum: row i's list is entries off[i] - off[r0] .. of its group's buffer), their total and the longest.
// One workgroup; thread t owns a contiguous run of rows.
template <class Len>
static __global__ __launch_bounds__(1024) void cl_scan_kernel(Len len, int n, long long* off, ClPlan* plan) {
    __shared__ long long part[1024], longest[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024, b = min(n, tid * per), e = min(n, b + per);
    long long s = 0, m = 0;
    for (int i = b; i < e; ++i) {
        s += len(i);
        m = max(m, len(i));
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
        s += len(i);
    }
}

// The groups: consecutive rows, as many as fit `entries` list entries (no list is longer: checked by the host before this runs).  Rows without entries
// cost nothing, so a group may be long.  bounds[g] = first row of group g, bounds[groups] = n.
static __global__ void cl_groups_kernel(const long long* off, int n, long long entries, int32_t* bounds, ClPlan* plan) {
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

// a gather pass over rows [r0, r1) walks the tiles of their row blocks
inline void cl_walk_rows(PtPairArgs& p, int r0, int r1) {
    const int b0 = r0 / PT_T, b1 = (r1 + PT_T - 1) / PT_T;
    p.tile0 = (long long)b0 * p.nblk;
    p.ntiles = (long long)(b1 - b0) * p.nblk;
}

// what the three callers' messages differ in: "<who>: <row_has> 17 <unit> (.. bytes), candidate_budget holds ..", "<who>: <broken> (non-finite coordinates?)"
struct ClNames { const char* who; const char* row_has; const char* unit; const char* broken; };

// The host half of the protocol, from "the scan has been launched" to "the flag is read and checked".  The listed rows are first .. first + n - 1 of `off`
// (the scan wrote off[first .. first + n]; bounds come back relative to `first`); `entries` slots of `entry_bytes` each; stats as include/dic_hip.h has them,
// stats[0] = passes.  launch(r0, r1) enqueues the caller's gather and exact kernels for the rows [r0, r1) of one group.
template <class Launch>
static int cl_run_groups(ClPlan* plan, const long long* off, int32_t* bounds, int n, int first, long long entries, int entry_bytes, int64_t* stats, int passes,
                         hipStream_t st, const ClNames& nm, Launch&& launch) {
    char what[64];
    snprintf(what, sizeof(what), "%s counting", nm.who);
    int rc = check_launch(what);
    if (rc) return rc;
    // the list lengths decide the groups: read their summary back (synchronises the stream)
    ClPlan hp;
    hipError_t e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: reading the list lengths: %s", nm.who, hipGetErrorString(e));
    if (stats) {
        stats[0] = passes;
        stats[1] = 0;
        stats[2] = hp.longest;
        stats[3] = hp.total;
        stats[4] = hp.longest * entry_bytes;
    }
    DIC_REQUIRE(hp.longest <= entries, DIC_ERR_WORKSPACE, "%s: %s %lld %s (%lld bytes), candidate_budget holds %lld (%lld bytes): run again with "
                "candidate_budget >= %lld", nm.who, nm.row_has, hp.longest, nm.unit, hp.longest * entry_bytes, entries, entries * entry_bytes,
                hp.longest * entry_bytes);
    // (the gather epilogues hold a list's length in an int; only the ranks' lists, sums of bands, can be that long)
    DIC_REQUIRE(hp.longest < (1LL << 31), DIC_ERR_UNSUPPORTED, "%s: %s %lld %s: fewer than 2^31", nm.who, nm.row_has, hp.longest, nm.unit);
    hipLaunchKernelGGL(cl_groups_kernel, dim3(1), dim3(64), 0, st, off + first, n, entries, bounds, plan);
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: reading the groups: %s", nm.who, hipGetErrorString(e));
    if (stats) stats[1] = hp.groups;
    constexpr int CHUNK = 1024;          // group bounds come back this many at a time
    int32_t hb[CHUNK + 1];
    snprintf(what, sizeof(what), "%s gather", nm.who);
    for (long long g0 = 0; g0 < hp.groups; g0 += CHUNK) {
        const int ng = (int)min((long long)CHUNK, hp.groups - g0);
        e = hipMemcpyAsync(hb, bounds + g0, (size_t)(ng + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: reading the groups: %s", nm.who, hipGetErrorString(e));
        for (int g = 0; g < ng; ++g) {
            DIC_REQUIRE(hb[g] >= 0 && hb[g] < hb[g + 1] && hb[g + 1] <= n, DIC_ERR_LAUNCH, "%s: group %lld = rows [%d, %d) of %d", nm.who, g0 + g, hb[g],
                        hb[g + 1], n);
            launch(first + hb[g], first + hb[g + 1]);
        }
        rc = check_launch(what);
        if (rc) return rc;
    }
    e = hipMemcpyAsync(&hp, plan, sizeof(hp), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: %s", nm.who, hipGetErrorString(e));
    DIC_REQUIRE(hp.flag == 0, DIC_ERR_LAUNCH, "%s: %s (non-finite coordinates?)", nm.who, nm.broken);
    return DIC_OK;
}

}  // namespace dic
