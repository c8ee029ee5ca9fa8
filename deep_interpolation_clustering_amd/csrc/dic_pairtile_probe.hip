// A TEST INSTRUMENT, not a clustering back end: the approximate d^2 of dic_pairtile.h's tile loop, written out.  DBSCAN, the k-th neighbour distances, the
// neighbour lists, mean shift and k-medoids decide on a_ij in registers and never store it; tests/test_gpu_pairtile.py holds it to the header's bound
// |a_ij - d^2_ij| < 2^-12 (n_i + nmax_J) against f64 through this file.  It runs pt_prepare_planes and pt_pair_pass unchanged -- the same planes, the same
// loop, the same launch shape as the consumers -- with an epilogue that stores every accumulator where PtLane says it belongs:
//   out[PtLane::row(I0, mb)][PtLane::col(J0, nb, k)] = acc[nb][mb][k],   out an (nblk 256) x (nblk 256) f32 matrix, padding rows and columns included,
// and counts the visits of every tile (one lane per workgroup and finish()).  The caller fills out with NaN and visits with 0 beforehand, so what a launch
// did not touch stays visible.  tile0 / ntiles / grid are the caller's: any range of the row-major tile list, over any number of workgroups.
#include "dic_pairtile.h"

namespace dic {

struct PpArgs {
    PtPairArgs p;
    float* out; long ld;          // ld = nblk * 256 columns
    int32_t* visits;              // (nblk, nblk)
};

struct PpStore {
    const PpArgs& a;
    const PtLane ln;
    __device__ __forceinline__ PpStore(const PpArgs& args) : a(args), ln() {}
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish(int I0, int J0, const pf32x16 (&acc)[4][2]) {
        // (I0, J0 < nblk * 256 by the host's check of the tile range: every row and column below lies inside out)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            float* orow = a.out + (size_t)ln.row(I0, mb) * a.ld;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {          // registers 4 q .. 4 q + 3 are four neighbouring columns
                    const pf32x4 v = {acc[nb][mb][4 * q], acc[nb][mb][4 * q + 1], acc[nb][mb][4 * q + 2], acc[nb][mb][4 * q + 3]};
                    *reinterpret_cast<pf32x4*>(orow + ln.col(J0, nb, 4 * q)) = v;
                }
        }
        if (threadIdx.x == 0) atomicAdd(a.visits + (size_t)(I0 / PT_T) * a.p.nblk + J0 / PT_T, 1);
    }
};

__global__ __launch_bounds__(512, 1) void pp_store_kernel(PpArgs a) {
    PpStore epi(a);
    pt_pair_pass(a.p, epi);
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_pairtile_probe_workspace(int64_t N, int D) {
    if (N <= 0 || N > 65536 || D <= 0 || D > PT_D) return 0;
    return pt_layout(N).total;
}

int dic_pairtile_probe(const float* X, long ldx, const float* centre, int64_t N, int D, float pad_norm, int64_t tile0, int64_t ntiles, int grid, float* out,
                       int32_t* visits, float* nrm, float* bmax, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && centre && out && visits && nrm && bmax && workspace, DIC_ERR_INVALID_ARG, "pairtile_probe: NULL pointer");
    DIC_REQUIRE(N > 0 && D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "pairtile_probe: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(D <= PT_D && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "pairtile_probe: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx, PT_D);
    DIC_REQUIRE(N <= 65536, DIC_ERR_UNSUPPORTED, "pairtile_probe: N=%lld: at most 65536 points (the matrix is written out)", (long long)N);
    DIC_REQUIRE(pad_norm >= 0.f && pad_norm <= 0x1p127f, DIC_ERR_INVALID_ARG, "pairtile_probe: pad_norm=%g", (double)pad_norm);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)centre & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                    ((uintptr_t)visits & 3) == 0 && ((uintptr_t)nrm & 3) == 0 && ((uintptr_t)bmax & 3) == 0,
                DIC_ERR_UNSUPPORTED, "pairtile_probe: operands must be 16-B aligned");
    const PtLayout o = pt_layout(N);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "pairtile_probe: workspace %zu < %zu", workspace_bytes, o.total);
    PpArgs t{};
    unsigned char* ws = (unsigned char*)workspace;
    pt_fill_pair_args(t.p, ws, N);
    const long long all = t.p.ntiles;
    DIC_REQUIRE(tile0 >= 0 && tile0 < all && ntiles >= 0 && ntiles <= all - tile0, DIC_ERR_INVALID_ARG, "pairtile_probe: tiles [%lld, +%lld) of %lld",
                (long long)tile0, (long long)ntiles, all);
    DIC_REQUIRE(grid >= 0 && grid <= 65535, DIC_ERR_INVALID_ARG, "pairtile_probe: grid=%d", grid);
    t.p.tile0 = tile0;
    t.p.ntiles = ntiles ? ntiles : all - tile0;
    t.out = out; t.ld = (long)t.p.nblk * PT_T; t.visits = visits;
    static bool reserved = false;
    int rc = pt_reserve_lds(reserved, {(const void*)pp_store_kernel}, "pairtile_probe");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = pt_prepare_planes(X, ldx, centre, N, D, pad_norm, ws, st, "pairtile_probe");
    if (rc) return rc;
    hipLaunchKernelGGL(pp_store_kernel, dim3(grid ? (unsigned)grid : pt_grid(t.p.ntiles)), dim3(512), PT_LDS, st, t);
    rc = check_launch("pairtile_probe");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(nrm, ws + o.nrm, (size_t)(N + PT_T) * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(bmax, ws + o.bmax, (size_t)t.p.nblk * sizeof(float), hipMemcpyDeviceToDevice, st);
    DIC_REQUIRE(e == hipSuccess, DIC_ERR_LAUNCH, "pairtile_probe: copying the norms: %s", hipGetErrorString(e));
    return DIC_OK;
}

}  // extern "C"
