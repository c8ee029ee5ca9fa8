// What the two Gaussian mixture files share (dic_gmm.hip: diagonal and spherical covariances; dic_gmm_full.hip: full and tied ones): the constants of the
// definition in include/dic_hip.h, the block-order sum both reductions are made of, the end of an EM iteration -- the lower bound's bookkeeping and THE STOPPING
// RULE, which defines converged_ and n_iter_ of both estimators -- and the checks of the points every entry point starts with.  The passes, the M-steps and
// the factor stay in their files: the two families share no arithmetic beyond these.  dic_bgmm.hip (the variational Bayesian mixture) takes the block-order
// sum, the bookkeeping of an iteration's end -- with its own lower bound, a sum -- and the checks of the points from here.  dic_fcm.hip (fuzzy c-means, no
// mixture, but the same pass / block-order reduction / status block) takes the block-order sum and the checks, and has its own end of an iteration below.
#pragma once
#include "dic_common.h"

namespace dic {

constexpr double GMM_LOG_2PI = 1.8378770664093453;
constexpr double GMM_NK_EPS = 10.0 * 2.220446049250313e-16;

// sum_b p[b * stride] in block order: BATCH loads in flight (a plain loop waits for one trip to memory per block, 256 in a row), the additions strictly
// sequential -- the bits of the plain loop
template <int BATCH>
__device__ __forceinline__ double gmm_sum_blocks(const double* p, size_t stride, int nblk) {
#pragma clang fp contract(off)
    double s = 0.0;
    int b = 0;
    for (; b + BATCH <= nblk; b += BATCH) {
        double v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) v[u] = p[(size_t)(b + u) * stride];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) s += v[u];
    }
    for (; b < nblk; ++b) s += p[(size_t)b * stride];
    return s;
}

// The end of an EM iteration of restart `run`, by the one thread that owns it.  st: the restart's DIC_GMM_STATUS_WORDS block (0 done, 1 iterations, 2 stopped
// by tol, 3 last lower bound, 4 tol, 5 max_iter); sum_lse = sum_i lse_i; fn = N.  Appends the lower bound, counts the iteration and decides whether the restart
// is done: |lb_t - lb_(t-1)| < tol (lb_0 = -inf), or max_iter reached.
__device__ __forceinline__ void gmm_end_iteration(double* st, double sum_lse, double fn, double* lower_bounds, int lb_stride, int run) {
#pragma clang fp contract(off)
    const double lb = sum_lse / fn;
    const double prev = st[3];
    const int it = (int)st[1];
    if (it < lb_stride) lower_bounds[(size_t)run * lb_stride + it] = lb;
    st[1] = (double)(it + 1);
    st[3] = lb;
    if (fabs(lb - prev) < st[4]) { st[0] = 1.0; st[2] = 1.0; }
    else if ((double)(it + 1) >= st[5]) st[0] = 1.0;
}

// The end of a fuzzy c-means iteration of restart `run` (dic_fcm.hip), by the one thread that owns it: the same status block, word 3 the last objective J.
// Appends J, counts the iteration and decides whether the restart is done: after iteration t >= 2 if |J_(t-1) - J_t| <= tol J_(t-1) -- a RELATIVE decrease,
// where the mixtures compare an absolute one, and never after the first iteration, whose J belongs to the initial centres -- or when t reaches max_iter.
__device__ __forceinline__ void fcm_end_iteration(double* st, double J, double* objectives, int obj_stride, int run) {
#pragma clang fp contract(off)
    const double prev = st[3];
    const int it = (int)st[1];
    if (it < obj_stride) objectives[(size_t)run * obj_stride + it] = J;
    st[1] = (double)(it + 1);
    st[3] = J;
    if (it >= 1 && fabs(prev - J) <= st[4] * prev) { st[0] = 1.0; st[2] = 1.0; }
    else if ((double)(it + 1) >= st[5]) st[0] = 1.0;
}

// The checks of the points, in the order the host tests assert: the invalid arguments, then the unsupported shapes (4 * kWave = 256 columns: both families').
static int gmm_check_points(const char* what, const float* X, long ldx, int64_t N, int D, int D0, int K) {
    DIC_REQUIRE(X, DIC_ERR_INVALID_ARG, "%s: NULL pointer", what);
    DIC_REQUIRE(N >= 2, DIC_ERR_INVALID_ARG, "%s: N=%lld: expected at least 2 points", what, (long long)N);
    DIC_REQUIRE(D > 0 && ldx >= D && D0 >= 1 && D0 <= D && K >= 1, DIC_ERR_INVALID_ARG, "%s: N=%lld D=%d D0=%d ldx=%ld K=%d", what, (long long)N, D, D0, ldx, K);
    DIC_REQUIRE(D <= 4 * kWave && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "%s: D=%d (row stride %ld): at most %d, multiples of 4", what, D, ldx,
                4 * kWave);
    DIC_REQUIRE(K <= DIC_MAX_CLUSTERS, DIC_ERR_UNSUPPORTED, "%s: K=%d: at most %d components", what, K, DIC_MAX_CLUSTERS);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "%s: N=%lld: fewer than 2^30 points", what, (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0, DIC_ERR_UNSUPPORTED, "%s: X must be 16-B aligned", what);
    return DIC_OK;
}

}  // namespace dic
