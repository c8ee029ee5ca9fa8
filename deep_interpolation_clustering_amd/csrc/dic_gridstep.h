// One launch per step of a sequential walk: the device pattern dic_optics.hip, dic_hdbscan.hip and dic_ward.hip share.  A step is a row pass over N rows by
// the whole chip that ends in ONE decision (the next point, a push, a merge) taken in the same launch; the host enqueues all steps back to back and never
// learns an intermediate result.  Two layers: THE HAND-OFF (all three files) and THE WALK (OPTICS and Prim, which differ in a rule of a few lines).
//
// THE HAND-OFF.  A step kernel runs at most GS_MAX_BLOCKS = 256 workgroups of GS_WAVES = 16 waves, and never two of them on one CU: each launch reserves
// GS_LDS_HOLD = 96 KiB of the CU's 160 KiB of LDS as dynamic LDS, which it does not touch.  Every wave reads the walk's state where the previous launch left
// it, takes rows q = wave, wave + #waves, .., GS_UNROLL = 4 at a time, and keeps a running minimum of (value, index), lexicographic (gs_before), so that inf
// and ties go to the smallest index.  Wave minima meet in LDS, and the workgroup's partial -- a few 8-B words -- goes to the workgroup's slot of `part`.
// The grid's minimum is taken by the workgroup that arrives last, in the same launch (gs_post):
//   1. thread 0 stores the partial with 8-B write-through (sc1) stores, waits for them (vmcnt(0)) and adds 1 to the ticket, an agent-scope atomic;
//   2. the workgroup whose add returns gridDim.x - 1 knows every partial is in memory: each add was issued after its workgroup's stores had drained;
//   3. it reads the partials with sc1 loads (gs_load_f64 / gs_load_int: past its L1, which other CUs' stores never refresh) behind the workgroup barrier
//      thread 0 joined after its add (the one that tells the other threads the add's result), reduces them, writes the state of the next launch and sets the ticket to 0.
// WHY THIS IS SOUND.  No workgroup waits for another: every launch ends on its own, whatever the others do -- no cooperative launch, no persistent kernel,
// no spin.  Nothing the last workgroup writes is read in its own launch: every other workgroup has read the state and left its row loop before it took
// its ticket, and the last workgroup is past its own row loop too; what it reads itself of the state it overwrites, it reads first (dic_ward.hip's tail says
// which).  Everything a launch reads besides `part` was written by an earlier launch, and launches on one stream are ordered.  The ticket is reset by the last
// workgroup, after every add of the launch (it saw the last one), so the next launch counts from 0; the init kernel sets it to 0 for the first.
// The alternative, a second one-workgroup kernel per step that reduces plainly stored partials, was measured against this on one MI355X with OPTICS
// (DESIGN.md section 5): 20.8 against 20.3 us per step at 75 000 x 256, 10.1 against 10.8 at 20 000 x 256, identical results; the in-launch form is kept
// for the cohort size.  A change of form is made here, once.
//
// THE WALK (walk_step<Rule>).  reach = inf, pred = -1, point 0 is first; N - 1 times: every wave reads the current point p from the slot and holds p's row in
// registers; a row q already taken costs one flag byte and no row load, the others one coalesced 16-B-per-lane load, their reach (and core, if the rule asks),
// dic_exactd2.h's f64 distance, the rule's weight w, the strict update reach[q] = w, pred[q] = p by lane 0 if w < reach[q], and enter the minimum of
// (reach, index).  walk_pick leaves for the next launch: the next point in the slot and in `ordering`, its flag, the ticket at 0.  A rule has
//   kCoreQ                whether core[q] is loaded (cq; 0 otherwise),
//   expands(cp)           whether p updates anything at all (if not, no row is loaded),
//   applies(dist, a)      whether the edge p - q exists,
//   weight(dist, cp, cq)  its weight.
// The host enqueues init + N - 1 steps (the last point needs no pass; N = 1: no step) and returns.  Two calls give the same bits.
#pragma once
#include "dic_exactd2.h"

namespace dic {

// ---- the hand-off ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int GS_WAVES = 16;                    // waves per workgroup
constexpr int GS_THREADS = GS_WAVES * kWave;
constexpr int GS_MAX_BLOCKS = kNumCU;           // one workgroup per CU at most: the hand-off of the partials is the one-per-CU form
constexpr int GS_LDS_HOLD = 96 * 1024;          // dynamic LDS a step asks for and never touches: more than half a CU's 160 KiB, so that no second workgroup of
                                                // a step can be placed on the same CU, whatever the dispatcher would otherwise do (16 waves, 64 VGPRs: two would fit)
constexpr int GS_UNROLL = 4;                    // rows in flight per wave
constexpr int GS_NONE = 0x7fffffff;             // the index of "no row"

static int gs_blocks(int64_t N) { return (int)max((int64_t)1, min((int64_t)GS_MAX_BLOCKS, (N + GS_WAVES - 1) / GS_WAVES)); }

__device__ __forceinline__ bool gs_before(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

// the 8-B words of a partial
__device__ __forceinline__ unsigned long long gs_word(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned long long gs_word(int i) { return (unsigned long long)(unsigned)i; }
__device__ __forceinline__ double gs_load_f64(const unsigned long long* p) {
    return __longlong_as_double((long long)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int gs_load_int(const unsigned long long* p) {
    return (int)(unsigned)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Steps 1 and 2 above, by the ONE thread that holds the workgroup's partial `w`: it posts the words to `mine`, this workgroup's slot of `part`, and returns
// whether its workgroup arrived last.  The caller hands that to the other threads through LDS and a workgroup barrier -- step 3's barrier.
template <int W>
__device__ __forceinline__ bool gs_post(unsigned long long* mine, unsigned* ticket, const unsigned long long (&w)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) __hip_atomic_store(mine + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
}

// host: `count` launches of step kernel K over N rows, after K's LDS reservation (once per kernel); `step` (or NULL) is the field of `a` that takes the
// launch's number
template <auto K, typename Args>
static int gs_enqueue(const char* who, Args& a, int* step, int64_t N, long long count, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, GS_LDS_HOLD);
        DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", who, GS_LDS_HOLD, hipGetErrorString(e));
        attr_set = true;
    }
    const dim3 grid((unsigned)gs_blocks(N));
    for (long long s = 0; s < count; ++s) {
        if (step) *step = (int)s;
        hipLaunchKernelGGL(K, grid, dim3(GS_THREADS), GS_LDS_HOLD, st, a);
        if ((s & 4095) == 4095) {          // a stream that refuses launches is not fed the rest of them
            const int rc = check_launch(who);
            if (rc) return rc;
        }
    }
    return check_launch(who);
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------------------------
struct WalkLayout { size_t done, part, slot, total; };
struct WalkSlot { int32_t cur; unsigned ticket; };

static WalkLayout walk_layout(int64_t N) {
    WalkLayout o;
    o.done = 0;
    o.part = align_up((size_t)N, 256);
    o.slot = o.part + align_up((size_t)GS_MAX_BLOCKS * 2 * sizeof(unsigned long long), 256);
    o.total = o.slot + 256;
    return o;
}

struct WalkArgs {
    const float* X; long ldx; int n, d;
    const double* core; double max_eps;          // (max_eps: OPTICS' rule alone)
    int32_t* ordering; double* reach; int32_t* pred;
    unsigned char* done; unsigned long long* part; WalkSlot* slot;
    int step;
};

// the body of a 256-thread init kernel over ceil(n / 256) workgroups
__device__ __forceinline__ void walk_init(const WalkArgs& a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    a.reach[i] = __builtin_inf();
    a.pred[i] = -1;
    a.done[i] = i == 0;          // all reach equal: the first point is index 0
    if (i == 0) {
        a.ordering[0] = 0;
        a.slot->cur = 0;
        a.slot->ticket = 0u;
    }
}

// The last workgroup of a step: every partial is in memory.  nblk <= GS_MAX_BLOCKS = 256 partials, one per thread of the first four waves, read past L1.
__device__ __forceinline__ void walk_pick(const WalkArgs& a, int nblk, double* s_r, int* s_i) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = a.n;
    double br = __builtin_inf();
    int bi = GS_NONE;
    if (tid < nblk) {
        br = gs_load_f64(a.part + 2 * (size_t)tid);
        bi = gs_load_int(a.part + 2 * (size_t)tid + 1);
    }
    if (w < GS_MAX_BLOCKS / kWave) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double orr = __shfl_xor(br, m);
            const int oi = __shfl_xor(bi, m);
            if (gs_before(orr, oi, br, bi)) { br = orr; bi = oi; }
        }
    }
    __syncthreads();          // (s_r / s_i of the first reduction have been read)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < GS_MAX_BLOCKS / kWave; ++k)
            if (gs_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
        const bool any = (unsigned)bi < (unsigned)n;
        a.slot->cur = any ? bi : -1;
        a.slot->ticket = 0u;
        if (any) {
            a.ordering[a.step + 1] = bi;          // (step + 1 < n: a row not yet taken exists)
            a.done[bi] = 1;
        }
    }
}

// the body of a step kernel of GS_THREADS threads
template <typename Rule>
__device__ __forceinline__ void walk_step(const WalkArgs& a) {
    __shared__ double s_r[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = a.n;
    const int p = a.slot->cur;
    if ((unsigned)p >= (unsigned)n) return;          // (no row was left: the host launches no such step)
    const double cp = a.core[p];
    const bool expand = Rule::expands(cp);
    ed_f32x4 xp = {0.f, 0.f, 0.f, 0.f};
    if (expand) xp = exact_d2_load(a.X, a.ldx, (size_t)p, a.d);
    double br = __builtin_inf();
    int bi = GS_NONE;
    const int stride = gridDim.x * GS_WAVES;
    for (int q0 = blockIdx.x * GS_WAVES + w; q0 < n; q0 += GS_UNROLL * stride) {
        bool live[GS_UNROLL];
        double rq[GS_UNROLL], cq[GS_UNROLL];
        ed_f32x4 xq[GS_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            live[u] = q < n && a.done[q] == 0;
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            rq[u] = 0.0;
            cq[u] = 0.0;
            xq[u] = xp;
            if (live[u]) {
                rq[u] = a.reach[q];
                if (Rule::kCoreQ) cq[u] = a.core[q];
                if (expand) xq[u] = exact_d2_load(a.X, a.ldx, (size_t)q, a.d);
            }
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            if (!live[u]) continue;
            double r = rq[u];
            if (expand) {
                const double dist = sqrt(exact_d2(xp, xq[u]));
                if (Rule::applies(dist, a)) {
                    const double cand = Rule::weight(dist, cp, cq[u]);
                    if (cand < r) {
                        r = cand;
                        if (lane == 0) {
                            a.reach[q] = cand;
                            a.pred[q] = p;
                        }
                    }
                }
            }
            if (gs_before(r, q, br, bi)) { br = r; bi = q; }
        }
    }
    // wave -> workgroup (br, bi are the same in every lane of a wave)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < GS_WAVES; ++k)
            if (gs_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
        // workgroup -> grid
        const unsigned long long partial[2] = {gs_word(br), gs_word(bi)};
        s_last = gs_post(a.part + 2 * (size_t)blockIdx.x, &a.slot->ticket, partial);
    }
    __syncthreads();
    if (!s_last) return;
    walk_pick(a, (int)gridDim.x, s_r, s_i);
}

// host: init + N - 1 steps.  Init and Step are the __global__ wrappers of walk_init and walk_step<Rule>; the caller has checked the arguments.
template <auto Init, auto Step>
static int walk_run(const char* who, const float* X, long ldx, int64_t N, int D, const double* core, double max_eps, int32_t* ordering, double* reach,
                    int32_t* pred, void* workspace, hipStream_t st) {
    const WalkLayout o = walk_layout(N);
    unsigned char* ws = (unsigned char*)workspace;
    WalkArgs a{};
    a.X = X; a.ldx = ldx; a.n = (int)N; a.d = D;
    a.core = core; a.max_eps = max_eps;
    a.ordering = ordering; a.reach = reach; a.pred = pred;
    a.done = ws + o.done; a.part = (unsigned long long*)(ws + o.part); a.slot = (WalkSlot*)(ws + o.slot);
    hipLaunchKernelGGL(Init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a);
    return gs_enqueue<Step>(who, a, &a.step, N, N - 1, st);
}

}  // namespace dic
