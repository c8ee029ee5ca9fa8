// OPTICS' main loop (p2_clustering_optK.py:86-88,171-223: sklearn.cluster.OPTICS) without the distance matrix: the ordering, reachability and predecessor of
// N points from their core distances, in the self-consistent form sklearn has with metric='precomputed' on the f64 difference-form matrix:
//   reach = inf, pred = -1, nothing processed; N times: p = the unprocessed point of smallest reach (ties, all-inf included: the smallest index); append p,
//   mark it; if core[p] is finite, every unprocessed q with d(p, q) <= max_eps gets r = around15(max(d(p, q), core[p])) if r < reach[q] (strictly), and
//   pred[q] = p.  around15(v) = rint(v * 1e15) / 1e15 is numpy's np.around(v, 15); core arrives rounded that way, and inf where it exceeds max_eps.
// The loop is sequential in p and each step is O(N D): a step is ONE launch, a row pass over the points.  d(p, q) is dic_exactd2.h's distance, the same
// bits dic_knn.hip took core[p] from -- every q inside p's core radius ties at core[p] and the index breaks the tie, so the bits decide the ordering.
//
// The step, the hand-off of the grid's minimum and the host loop are dic_gridstep.h's walk with OpRule: a p with infinite core distance updates nothing and
// loads no row; an edge applies within max_eps and weighs around15(max(d(p, q), core[p])); core[q] is not read.
#include "dic_gridstep.h"

namespace dic {

struct OpRule {
    static constexpr bool kCoreQ = false;
    static __device__ __forceinline__ double around15(double v) { return rint(v * 1e15) / 1e15; }
    static __device__ __forceinline__ bool expands(double cp) { return cp < __builtin_inf(); }
    static __device__ __forceinline__ bool applies(double dist, const WalkArgs& a) { return dist <= a.max_eps; }
    static __device__ __forceinline__ double weight(double dist, double cp, double) { return around15(fmax(dist, cp)); }
};

__global__ __launch_bounds__(256) void op_init_kernel(WalkArgs a) { walk_init(a); }
__global__ __launch_bounds__(GS_THREADS) void op_step_kernel(WalkArgs a) { walk_step<OpRule>(a); }

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_optics_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave) return 0;
    return walk_layout(N).total;
}

int dic_optics_order(const float* X, long ldx, int64_t N, int D, const double* core, double max_eps, int32_t* ordering, double* reachability,
                     int32_t* predecessor, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && core && ordering && reachability && predecessor && workspace, DIC_ERR_INVALID_ARG, "optics_order: NULL pointer");
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "optics_order: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(max_eps >= 0.0, DIC_ERR_INVALID_ARG, "optics_order: max_eps=%g: expected >= 0", max_eps);
    DIC_REQUIRE(D <= 4 * kWave && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "optics_order: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx,
                4 * kWave);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "optics_order: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && (((uintptr_t)core | (uintptr_t)reachability) & 7) == 0 &&
                    (((uintptr_t)ordering | (uintptr_t)predecessor) & 3) == 0,
                DIC_ERR_UNSUPPORTED, "optics_order: X and the workspace must be 16-B aligned, the arrays to their element size");
    const size_t need = walk_layout(N).total;
    DIC_REQUIRE(workspace_bytes >= need, DIC_ERR_WORKSPACE, "optics_order: workspace %zu < %zu", workspace_bytes, need);
    return walk_run<op_init_kernel, op_step_kernel>("optics_order", X, ldx, N, D, core, max_eps, ordering, reachability, predecessor, workspace,
                                                     (hipStream_t)stream);
}

}  // extern "C"
