// The counting epilogue of the pair-tile loop with per-row thresholds, shared by the k-th neighbour distances / neighbour lists (dic_knn.hip) and the neighbour
// ranks (dic_knn_rank.hip): cnt[i][q] += #{j : a_ij <= thr[i][q]} over the walked tiles, a_ij the loop's approximate d^2 (dic_pairtile.h).
#pragma once
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

}  // namespace dic
