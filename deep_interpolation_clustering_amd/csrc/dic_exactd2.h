// The exact squared distance of two f32 points, one wave per pair: the quantity dic_knn.hip ranks and dic_optics.hip walks.  Both files take it from here,
// so the distance of a pair has the same bits wherever it is computed -- OPTICS breaks its ties on that (a point's min_samples-th neighbour lies AT its
// core distance, and d(p, q) = d(q, p): (a - b)^2 = (b - a)^2 exactly, term by term).
// Lane l holds coordinates 4 l .. 4 l + 3 (D <= 256 = 64 lanes x 4; lanes beyond D hold zeros, which add exactly): an f64 fma chain over the lane's four
// differences in coordinate order (every difference of two f32 is exact in f64), then wave_sum's xor tree.  The result is in every lane.
#pragma once
#include "dic_common.h"

namespace dic {

typedef float ed_f32x4 __attribute__((ext_vector_type(4)));

// this lane's four coordinates of row `row` (zeros beyond d); d % 4 == 0, rows 16-B aligned
__device__ __forceinline__ ed_f32x4 exact_d2_load(const float* X, long ldx, size_t row, int d) {
    const int col = 4 * lane_id();
    ed_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col < d) v = *reinterpret_cast<const ed_f32x4*>(X + row * (size_t)ldx + col);
    return v;
}

__device__ __forceinline__ double exact_d2(const ed_f32x4 xi, const ed_f32x4 xj) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double t = (double)xi[q] - (double)xj[q];
        s = fma(t, t, s);
    }
    return wave_sum(s);
}

}  // namespace dic
