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
// The step, the hand-off of the grid's minimum and the host loop are dic_gridstep.h's walk with PrimRule: every p expands, core[q] is one more 8-B load per
// row outside the tree, and every edge applies and weighs max(d(p, q), core[p], core[q]).
#include "dic_gridstep.h"

namespace dic {

struct PrimRule {
    static constexpr bool kCoreQ = true;
    static __device__ __forceinline__ bool expands(double) { return true; }
    static __device__ __forceinline__ bool applies(double, const WalkArgs&) { return true; }
    static __device__ __forceinline__ double weight(double dist, double cp, double cq) { return fmax(fmax(dist, cp), cq); }
};

__global__ __launch_bounds__(256) void hd_init_kernel(WalkArgs a) { walk_init(a); }
__global__ __launch_bounds__(GS_THREADS) void hd_step_kernel(WalkArgs a) { walk_step<PrimRule>(a); }

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_hdbscan_workspace(int64_t N, int D) {
    if (N <= 0 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave) return 0;
    return walk_layout(N).total;
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
    const size_t need = walk_layout(N).total;
    DIC_REQUIRE(workspace_bytes >= need, DIC_ERR_WORKSPACE, "hdbscan_mst: workspace %zu < %zu", workspace_bytes, need);
    return walk_run<hd_init_kernel, hd_step_kernel>("hdbscan_mst", X, ldx, N, D, core, 0.0, ordering, reachability, predecessor, workspace,
                                                     (hipStream_t)stream);
}

}  // extern "C"
