// HDBSCAN's expensive part (sklearn.cluster.HDBSCAN, _linkage.pyx: mst_from_mutual_reachability) without the distance matrix: Prim's minimum spanning tree of
// the mutual-reachability graph mr(p, q) = max(core[p], core[q], d(p, q)), in the self-consistent form sklearn has with metric='precomputed' on the f64
// difference-form matrix:
//   reach = inf, pred = -1, point 0 is first; N - 1 times: the current point p is in the tree; every q outside the tree with mr(p, q) < reach[q] (strictly)
//   gets reach[q] = mr(p, q) and pred[q] = p; the next point is the one outside the tree of smallest reach (ties: the smallest index).
// The loop is dic_optics.hip's with one more max: sequential in p, each step O(N D) and ONE launch, a row pass over the points.  d(p, q) is dic_exactd2.h's
// distance, the same bits dic_knn.hip took core[] from: every edge into a sparse point weighs exactly that point's core distance, such edges tie, and the
// index breaks the tie -- the bits decide the walk.  Nothing is rounded (HDBSCAN has no around15), there is no max_eps and no point that does not expand;
// zero weights occur (duplicated points with min_samples <= their multiplicity) and order like any other value.
//
// A STEP (hd_step_kernel, at most 256 workgroups of 16 waves, and never two of them on one CU: each reserves 96 KiB of the CU's 160 KiB of LDS, HD_LDS_HOLD,
// which it does not touch): every wave reads the current point p from the slot the previous step left it in and holds p's row in registers; it then takes
// rows q = wave, wave + #waves, .., four at a time: rows in the tree cost one flag byte and no row load, the others one coalesced 16-B-per-lane load, their
// reach and core (8 B each), the f64 distance, the update of reach / pred by lane 0, and enter the wave's running minimum of (reach, index) -- lexicographic.
// Wave minima meet in LDS, the workgroup's minimum goes to its 16-B slot of `part`.
// THE GRID'S MINIMUM is taken by the workgroup that arrives last, in the same launch, exactly as in dic_optics.hip: one lane stores the partial with two 8-B
// write-through (sc1) stores, waits for them (vmcnt(0)) and adds 1 to the ticket, an agent-scope atomic; the workgroup whose add returns gridDim.x - 1 knows
// every partial is in memory, reads them with sc1 loads (past its L1, which other CUs' stores never refresh) behind a workgroup barrier its adding wave
// joined, reduces them, and leaves for the next launch: the next point in the slot and in `ordering`, its in-tree flag, the ticket at 0.  No workgroup waits
// for another: every launch ends on its own.  Nothing the last workgroup writes is read in its own launch (every other workgroup has left its row loop
// before it took its ticket), and everything a launch reads besides `part` was written by an earlier launch.
// The host enqueues init + N - 1 steps and returns; it never learns an intermediate point.  Two calls give the same bits.
#include "dic_exactd2.h"

namespace dic {

constexpr int HD_WAVES = 16;                    // waves per workgroup
constexpr int HD_THREADS = HD_WAVES * kWave;
constexpr int HD_MAX_BLOCKS = kNumCU;           // one workgroup per CU at most: the hand-off of the partials is the one-per-CU form
constexpr int HD_LDS_HOLD = 96 * 1024;          // dynamic LDS a step asks for and never touches: more than half a CU's 160 KiB, so that no second workgroup of
                                                // a step can be placed on the same CU
constexpr int HD_UNROLL = 4;                    // rows in flight per wave
constexpr int HD_NONE = 0x7fffffff;             // the index of "no row outside the tree"

struct HdLayout { size_t done, part, slot, total; };
struct HdSlot { int32_t cur; unsigned ticket; };

static HdLayout hd_layout(int64_t N) {
    HdLayout o;
    o.done = 0;
    o.part = align_up((size_t)N, 256);
    o.slot = o.part + align_up((size_t)HD_MAX_BLOCKS * 2 * sizeof(unsigned long long), 256);
    o.total = o.slot + 256;
    return o;
}

static int hd_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)HD_MAX_BLOCKS, (N + HD_WAVES - 1) / HD_WAVES)); }

struct HdArgs {
    const float* X; long ldx; int n, d;
    const double* core;
    int32_t* ordering; double* reach; int32_t* pred;
    unsigned char* done; unsigned long long* part; HdSlot* slot;
    int step;
};

__device__ __forceinline__ bool hd_before(double ra, int ia, double rb, int ib) { return ra < rb || (ra == rb && ia < ib); }

__global__ __launch_bounds__(256) void hd_init_kernel(int n, int32_t* ordering, double* reach, int32_t* pred, unsigned char* done, HdSlot* slot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    reach[i] = __builtin_inf();
    pred[i] = -1;
    done[i] = i == 0;          // Prim starts from point 0
    if (i == 0) {
        ordering[0] = 0;
        slot->cur = 0;
        slot->ticket = 0u;
    }
}

// The last workgroup of a step: every partial is in memory.  nblk <= HD_MAX_BLOCKS = 256 partials, one per thread of the first four waves, read past L1.
__device__ __forceinline__ void hd_pick(const HdArgs& a, int nblk, double* s_r, int* s_i) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = a.n;
    double br = __builtin_inf();
    int bi = HD_NONE;
    if (tid < nblk) {
        br = __longlong_as_double((long long)__hip_atomic_load(a.part + 2 * (size_t)tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        bi = (int)(unsigned)__hip_atomic_load(a.part + 2 * (size_t)tid + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (w < HD_MAX_BLOCKS / kWave) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double orr = __shfl_xor(br, m);
            const int oi = __shfl_xor(bi, m);
            if (hd_before(orr, oi, br, bi)) { br = orr; bi = oi; }
        }
    }
    __syncthreads();          // (s_r / s_i of the first reduction have been read)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < HD_MAX_BLOCKS / kWave; ++k)
            if (hd_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
        const bool any = (unsigned)bi < (unsigned)n;
        a.slot->cur = any ? bi : -1;
        a.slot->ticket = 0u;
        if (any) {
            a.ordering[a.step + 1] = bi;          // (step + 1 < n: a row outside the tree exists)
            a.done[bi] = 1;
        }
    }
}

__global__ __launch_bounds__(HD_THREADS) void hd_step_kernel(HdArgs a) {
    __shared__ double s_r[HD_WAVES];
    __shared__ int s_i[HD_WAVES];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = a.n;
    const int p = a.slot->cur;
    if ((unsigned)p >= (unsigned)n) return;          // (no row outside the tree was left: the host launches no such step)
    const double cp = a.core[p];
    const ed_f32x4 xp = exact_d2_load(a.X, a.ldx, (size_t)p, a.d);
    double br = __builtin_inf();
    int bi = HD_NONE;
    const int stride = gridDim.x * HD_WAVES;
    for (int q0 = blockIdx.x * HD_WAVES + w; q0 < n; q0 += HD_UNROLL * stride) {
        bool live[HD_UNROLL];
        double rq[HD_UNROLL], cq[HD_UNROLL];
        ed_f32x4 xq[HD_UNROLL];
#pragma unroll
        for (int u = 0; u < HD_UNROLL; ++u) {
            const int q = q0 + u * stride;
            live[u] = q < n && a.done[q] == 0;
        }
#pragma unroll
        for (int u = 0; u < HD_UNROLL; ++u) {
            const int q = q0 + u * stride;
            rq[u] = 0.0;
            cq[u] = 0.0;
            xq[u] = xp;
            if (live[u]) {
                rq[u] = a.reach[q];
                cq[u] = a.core[q];
                xq[u] = exact_d2_load(a.X, a.ldx, (size_t)q, a.d);
            }
        }
#pragma unroll
        for (int u = 0; u < HD_UNROLL; ++u) {
            const int q = q0 + u * stride;
            if (!live[u]) continue;
            double r = rq[u];
            const double dist = sqrt(exact_d2(xp, xq[u]));
            const double mr = fmax(fmax(dist, cp), cq[u]);
            if (mr < r) {
                r = mr;
                if (lane == 0) {
                    a.reach[q] = mr;
                    a.pred[q] = p;
                }
            }
            if (hd_before(r, q, br, bi)) { br = r; bi = q; }
        }
    }
    // wave -> workgroup (br, bi are the same in every lane of a wave)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < HD_WAVES; ++k)
            if (hd_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
        // workgroup -> grid: write-through stores, drained, then the ticket
        unsigned long long* mine = a.part + 2 * (size_t)blockIdx.x;
        __hip_atomic_store(mine, (unsigned long long)__double_as_longlong(br), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 1, (unsigned long long)(unsigned)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(&a.slot->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    hd_pick(a, (int)gridDim.x, s_r, s_i);
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_hdbscan_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave) return 0;
    return hd_layout(N).total;
}

int dic_hdbscan_mst(const float* X, long ldx, int64_t N, int D, const double* core, int32_t* ordering, double* reachability, int32_t* predecessor,
                    void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && core && ordering && reachability && predecessor && workspace, DIC_ERR_INVALID_ARG, "hdbscan_mst: NULL pointer");
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "hdbscan_mst: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(D <= 4 * kWave && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "hdbscan_mst: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx,
                4 * kWave);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "hdbscan_mst: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && (((uintptr_t)core | (uintptr_t)reachability) & 7) == 0 &&
                    (((uintptr_t)ordering | (uintptr_t)predecessor) & 3) == 0,
                DIC_ERR_UNSUPPORTED, "hdbscan_mst: X and the workspace must be 16-B aligned, the arrays to their element size");
    const HdLayout o = hd_layout(N);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "hdbscan_mst: workspace %zu < %zu", workspace_bytes, o.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    HdArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D;
    a.core = core;
    a.ordering = ordering; a.reach = reachability; a.pred = predecessor;
    a.done = ws + o.done; a.part = (unsigned long long*)(ws + o.part); a.slot = (HdSlot*)(ws + o.slot);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)hd_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HD_LDS_HOLD);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "hdbscan_mst: cannot reserve %d B of LDS: %s", HD_LDS_HOLD, hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(hd_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a.n, ordering, reachability, predecessor, a.done, a.slot);
    const dim3 grid((unsigned)hd_blocks(N));
    for (int s = 0; s + 1 < a.n; ++s) {          // (N = 1: no step)
        a.step = s;
        hipLaunchKernelGGL(hd_step_kernel, grid, dim3(HD_THREADS), HD_LDS_HOLD, st, a);
        if ((s & 4095) == 4095) {          // a stream that refuses launches is not fed the rest of them
            const int rc = check_launch("hdbscan_mst");
            if (rc) return rc;
        }
    }
    return check_launch("hdbscan_mst");
}

}  // extern "C"
