// Ward's agglomerative clustering of N f32 points without the distance matrix: scipy.cluster.hierarchy.linkage(X, 'ward')'s dendrogram from the sizes and
// centroids of the live clusters alone (the p2 / p4 `--cluster_method ward` branches).  Ward's distance of two clusters depends on nothing else, so a step
// of scipy's nearest-neighbour chain is one row pass over the live centroids.
// THE DEFINITION.  A live cluster i has a size n_i (int32; 0: merged away), the f64 coordinate sums S_i and the centroid C_i; at the start n_i = 1 and
// S_i = C_i = (double)x_i.  C_i = S_i / n_i, one rounded division per coordinate, is computed when the cluster is made and never again.
//   d2(i, j) = (2 n_i n_j / (n_i + n_j)) * sum_k (C_i[k] - C_j[k])^2
// with the sum taken as dic_exactd2.h takes its own -- lane l holds the coordinates 4 l .. 4 l + 3, one rounded f64 difference each, an fma chain over the
// four in coordinate order, then wave_sum's xor tree -- and the factor in f64 as (2.0 * ((double)n_i * (double)n_j)) / ((double)n_i + (double)n_j): every
// operation is symmetric in i and j, so d2(i, j) and d2(j, i) have the same bits.  The height of a merge is sqrt(d2).
// A merge of a < b writes the result into b: S_b = S_a + S_b, n_b = n_a + n_b, C_b = S_b / n_b, n_a = 0.
// The chain is scipy's nn_chain as dic_consensus.hip's lk_step_kernel states it: an empty chain becomes [the smallest live index]; repeat x = chain[-1],
// y = the live i != x of smallest (d2(x, i), i), lexicographic, except that chain[-2] wins when it ties that minimum (`!(best < d_prev)`), until
// y == chain[-2], else append y; a reciprocal pair is popped (two elements), merged and recorded as (a, b, height, n_a + n_b).
// Every expression whose rounding must not depend on contraction (the factor, the product with the sum, the differences, the sums S and the division) is
// under `#pragma clang fp contract(off)`; the fma chain is written as fma.  DESIGN.md's consensus section has the reason.
//
// A STEP (wd_step_kernel) IS ONE LAUNCH in dic_gridstep.h's hand-off form (its constants, gs_before, gs_post, the past-L1 loads, the host loop; the proof
// is there).  Every wave reads the chain's state where the previous launch left it and holds C_x in registers (32 B per lane: two 16-B loads); it then
// takes rows q = wave, wave + #waves, .., four at a time: a dead row (and x itself) costs one size load and no row load, a live one its 32 B per lane, the
// distance, and enters the wave's running minimum of (d2, index).  The wave that meets chain[-2] keeps its distance, d_prev.  Wave minima and d_prev meet in
// LDS, and the workgroup's partial (d2, index, d_prev; -1 = not met) goes to its 32-B slot of `part`.
// The workgroup that arrives last reduces the partials and does what lk_step_kernel's tail does: it compares with d_prev and either pushes y or merges --
// S_b, C_b, the sizes, the record, the chain length, the merge and step counts -- and sets the ticket to 0.  What the hand-off asks of it: of the state it
// overwrites it reads S_a, S_b (each coordinate by the thread that writes it), the sizes and the cursor first, behind a barrier where another thread writes
// them.
// THE SMALLEST LIVE INDEX only grows (a merge kills the smaller name), so a cursor serves the fresh chain: when a merge kills the cursor's cluster a, the
// last workgroup moves it to the first live index above a -- b at the latest; the sizes it scans, those strictly between a and b, nobody writes in this
// launch.  The scans of all merges together pass over every index once.
// The host enqueues one init kernel and 3 (N - 1) steps -- a launch pushes or merges, and a fresh chain pushes two -- and returns; a step that finds
// N - 1 merges done returns at once.  The host never reads an intermediate result.  Two calls give the same bits.
#include "dic_gridstep.h"

namespace dic {

constexpr int WD_PART = 4;                      // 8-B words of a workgroup's partial: d2, index, d_prev, (unused)

typedef double wd_f64x2 __attribute__((ext_vector_type(2)));
struct WdRow { wd_f64x2 lo, hi; };              // a lane's four coordinates

// (steps: the launches that pushed or merged -- read by scripts/ward_bench.py and the tests; first: the smallest live index)
struct WdState { int clen, merges, steps, first; unsigned ticket; };
struct WdLayout { size_t S, C, size, chain, part, state, total; };

static WdLayout wd_layout(int64_t N, int D) {
    WdLayout o;
    const size_t row = (size_t)((D + 3) / 4 * 4) * sizeof(double);          // D': the width padded to a lane's four coordinates
    o.S = 0;
    o.C = o.S + align_up((size_t)N * row, 256);
    o.size = o.C + align_up((size_t)N * row, 256);
    o.chain = o.size + align_up((size_t)N * sizeof(int), 256);
    o.part = o.chain + align_up((size_t)N * sizeof(int), 256);
    o.state = o.part + align_up((size_t)GS_MAX_BLOCKS * WD_PART * sizeof(unsigned long long), 256);
    o.total = o.state + 256;
    return o;
}

struct WdArgs {
    int n, d;
    double* S; double* C; int* size; int* chain;
    unsigned long long* part; WdState* st; double* rec;
};

// this lane's four coordinates of row `row` of an (n, d) f64 matrix (zeros beyond d); d % 4 == 0, rows 32-B aligned
__device__ __forceinline__ WdRow wd_load(const double* M, int d, size_t row) {
    const int col = 4 * lane_id();
    WdRow r;
    r.lo = wd_f64x2{0.0, 0.0};
    r.hi = wd_f64x2{0.0, 0.0};
    if (col < d) {
        const double* p = M + row * (size_t)d + col;
        r.lo = *reinterpret_cast<const wd_f64x2*>(p);
        r.hi = *reinterpret_cast<const wd_f64x2*>(p + 2);
    }
    return r;
}

// sum_k (a[k] - b[k])^2: the result in every lane, the same bits for (a, b) and (b, a)
__device__ __forceinline__ double wd_sqdiff(const WdRow& a, const WdRow& b) {
#pragma clang fp contract(off)
    const double t0 = a.lo[0] - b.lo[0];
    const double t1 = a.lo[1] - b.lo[1];
    const double t2 = a.hi[0] - b.hi[0];
    const double t3 = a.hi[1] - b.hi[1];
    double s = 0.0;
    s = fma(t0, t0, s);
    s = fma(t1, t1, s);
    s = fma(t2, t2, s);
    s = fma(t3, t3, s);
    return wave_sum(s);
}

__device__ __forceinline__ double wd_d2(int ni, int nj, double sum) {
#pragma clang fp contract(off)
    const double fi = (double)ni, fj = (double)nj;
    const double prod = fi * fj;
    const double num = 2.0 * prod;
    const double den = fi + fj;
    const double f = num / den;
    return f * sum;
}

__device__ __forceinline__ double wd_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double wd_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// one wave per row, four rows per workgroup, grid-stride
__global__ __launch_bounds__(256) void wd_init_kernel(const float* X, long ldx, WdArgs a) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int col = 4 * lane;
    for (long long i = (long long)blockIdx.x * 4 + w; i < a.n; i += (long long)gridDim.x * 4) {
        if (col < a.d) {
            const float* x = X + (size_t)i * ldx + col;
            const float4 v = *reinterpret_cast<const float4*>(x);
            const wd_f64x2 lo = {(double)v.x, (double)v.y}, hi = {(double)v.z, (double)v.w};
            double* s = a.S + (size_t)i * a.d + col;
            double* c = a.C + (size_t)i * a.d + col;
            *reinterpret_cast<wd_f64x2*>(s) = lo;
            *reinterpret_cast<wd_f64x2*>(s + 2) = hi;
            *reinterpret_cast<wd_f64x2*>(c) = lo;
            *reinterpret_cast<wd_f64x2*>(c + 2) = hi;
        }
        if (lane == 0) a.size[i] = 1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.st->clen = 0; a.st->merges = 0; a.st->steps = 0; a.st->first = 0; a.st->ticket = 0u;
    }
}

// The last workgroup of a step: every partial is in memory.  The grid's (d2, index) and d_prev, in every thread.  nblk <= GS_MAX_BLOCKS = 256 partials, one
// per thread of the first four waves, read past L1.
__device__ __forceinline__ void wd_pick(const WdArgs& a, int nblk, double& br, int& bi, double& dp, double* s_r, int* s_i, double* s_d) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    br = __builtin_inf();
    bi = GS_NONE;
    dp = -1.0;
    if (tid < nblk) {
        const unsigned long long* p = a.part + (size_t)WD_PART * tid;
        br = gs_load_f64(p);
        bi = gs_load_int(p + 1);
        dp = gs_load_f64(p + 2);
    }
    if (w < GS_MAX_BLOCKS / kWave) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double orr = __shfl_xor(br, m);
            const int oi = __shfl_xor(bi, m);
            const double od = __shfl_xor(dp, m);
            if (gs_before(orr, oi, br, bi)) { br = orr; bi = oi; }
            dp = fmax(dp, od);          // (one workgroup met chain[-2]; the others hold -1)
        }
    }
    __syncthreads();          // (s_r / s_i / s_d of the first reduction have been read)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; s_d[w] = dp; }
    __syncthreads();
    br = s_r[0]; bi = s_i[0]; dp = s_d[0];
#pragma unroll
    for (int k = 1; k < GS_MAX_BLOCKS / kWave; ++k) {
        if (gs_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
        dp = fmax(dp, s_d[k]);
    }
}

// The first live index strictly between a and b, or b: by the whole workgroup, the result in every thread.  Nobody writes these sizes in this launch.
__device__ __forceinline__ int wd_next_live(const int* size, int a, int b, int* s_i) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    for (int base = a + 1; base < b; base += GS_THREADS) {
        const int i = base + tid;
        const bool live = i < b && size[i] > 0;
        const unsigned long long m = __ballot(live);
        __syncthreads();          // (an earlier round, or wd_pick, has been read)
        if (lane == 0) s_i[w] = m ? base + w * kWave + (int)__builtin_ctzll(m) : GS_NONE;
        __syncthreads();
        int found = GS_NONE;
#pragma unroll
        for (int k = 0; k < GS_WAVES; ++k) found = min(found, s_i[k]);
        if (found != GS_NONE) return found;
    }
    return b;
}

__global__ __launch_bounds__(GS_THREADS) void wd_step_kernel(WdArgs a) {
    __shared__ double s_r[GS_WAVES];
    __shared__ double s_d[GS_WAVES];
    __shared__ int s_i[GS_WAVES];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int n = a.n, d = a.d;
    // the state, as the previous launch left it: the last workgroup rewrites it only after every workgroup has taken its ticket
    const int merges = a.st->merges;
    int clen = a.st->clen;
    if (merges >= n - 1) return;          // (a step after the last merge)
    const bool fresh = clen <= 0;
    int x, yprev = -1;
    if (fresh) {
        x = a.st->first;
        clen = 1;
    } else {
        x = a.chain[clen - 1];
        if (clen > 1) yprev = a.chain[clen - 2];
    }
    if ((unsigned)x >= (unsigned)n) return;          // (not reached: the chain holds live indices; no load outside the arrays whatever the state holds)
    const int nx = a.size[x];
    const WdRow cx = wd_load(a.C, d, (size_t)x);
    double br = __builtin_inf(), dp = -1.0;
    int bi = GS_NONE;
    const int stride = gridDim.x * GS_WAVES;
    for (int q0 = blockIdx.x * GS_WAVES + w; q0 < n; q0 += GS_UNROLL * stride) {
        int nq[GS_UNROLL];
        WdRow cq[GS_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            nq[u] = (q < n && q != x) ? a.size[q] : 0;
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            cq[u] = cx;
            if (nq[u] > 0) cq[u] = wd_load(a.C, d, (size_t)q);
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
            const int q = q0 + u * stride;
            if (nq[u] <= 0) continue;
            const double v = wd_d2(nx, nq[u], wd_sqdiff(cx, cq[u]));
            if (q == yprev) dp = v;
            if (gs_before(v, q, br, bi)) { br = v; bi = q; }
        }
    }
    // wave -> workgroup (br, bi, dp are the same in every lane of a wave)
    if (lane == 0) { s_r[w] = br; s_i[w] = bi; s_d[w] = dp; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < GS_WAVES; ++k) {
            if (gs_before(s_r[k], s_i[k], br, bi)) { br = s_r[k]; bi = s_i[k]; }
            dp = fmax(dp, s_d[k]);
        }
        // workgroup -> grid
        const unsigned long long partial[3] = {gs_word(br), gs_word(bi), gs_word(dp)};
        s_last = gs_post(a.part + (size_t)WD_PART * blockIdx.x, &a.st->ticket, partial);
    }
    __syncthreads();
    if (!s_last) return;

    // ---- the last workgroup: lk_step_kernel's tail; every thread holds the same values
    wd_pick(a, (int)gridDim.x, br, bi, dp, s_r, s_i, s_d);
    int y = bi;
    double cur = br;
    if (yprev >= 0 && !(br < dp)) { y = yprev; cur = dp; }          // the previous chain element wins a tie
    if ((unsigned)y >= (unsigned)n) {          // (no live row besides x: not reached while merges < n - 1)
        if (tid == 0) a.st->ticket = 0u;
        return;
    }
    if (yprev < 0 || y != yprev) {
        if (tid == 0) {
            if (clen < n) {          // (chain elements are distinct live clusters: clen < n always; no store past the array whatever the rows hold)
                if (fresh) a.chain[0] = x;
                a.chain[clen] = y;
                a.st->clen = clen + 1;
                a.st->steps += 1;
            }
            a.st->ticket = 0u;
        }
        return;
    }
    const int ia = min(x, y), ib = max(x, y);
    const int na = a.size[ia], nb = a.size[ib];
    const int first = a.st->first;
    const double fs = (double)(na + nb);
    if (tid < d) {          // (d <= 256 < GS_THREADS: a coordinate per thread, read and written by that thread alone)
        double* sa = a.S + (size_t)ia * d + tid;
        double* sb = a.S + (size_t)ib * d + tid;
        const double s = wd_add(*sa, *sb);
        *sb = s;
        a.C[(size_t)ib * d + tid] = wd_div(s, fs);
    }
    int nfirst = first;
    if (first == ia) nfirst = wd_next_live(a.size, ia, ib, s_i);
    __syncthreads();          // (every thread has read the sizes and the state)
    if (tid == 0) {
        double* r = a.rec + 4 * (size_t)merges;
        r[0] = (double)ia; r[1] = (double)ib; r[2] = sqrt(cur); r[3] = fs;
        a.size[ia] = 0;
        a.size[ib] = na + nb;
        a.st->clen = clen - 2;
        a.st->merges = merges + 1;
        a.st->steps += 1;
        a.st->first = nfirst;
        a.st->ticket = 0u;
    }
}

}  // namespace dic

using namespace dic;

extern "C" {

size_t dic_ward_workspace(int64_t N, int D) {
    if (N < 2 || N >= (1LL << 30) || D <= 0 || D > 4 * kWave) return 0;
    return wd_layout(N, D).total;
}

int dic_ward_linkage(const float* X, long ldx, int64_t N, int D, double* records, void* workspace, size_t workspace_bytes, dic_stream_t stream) {
    DIC_REQUIRE(X && records && workspace, DIC_ERR_INVALID_ARG, "ward_linkage: NULL pointer");
    DIC_REQUIRE(N >= 2, DIC_ERR_INVALID_ARG, "ward_linkage: N=%lld: expected at least 2 points", (long long)N);
    DIC_REQUIRE(D > 0 && ldx >= D, DIC_ERR_INVALID_ARG, "ward_linkage: N=%lld D=%d ldx=%ld", (long long)N, D, ldx);
    DIC_REQUIRE(D <= 4 * kWave && D % 4 == 0 && ldx % 4 == 0, DIC_ERR_UNSUPPORTED, "ward_linkage: D=%d (row stride %ld): at most %d, multiples of 4", D, ldx,
                4 * kWave);
    DIC_REQUIRE(N < (1LL << 30), DIC_ERR_UNSUPPORTED, "ward_linkage: N=%lld: fewer than 2^30 points", (long long)N);
    DIC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)records & 7) == 0, DIC_ERR_UNSUPPORTED,
                "ward_linkage: X and the workspace must be 16-B aligned, the records 8-B");
    const WdLayout o = wd_layout(N, D);
    DIC_REQUIRE(workspace_bytes >= o.total, DIC_ERR_WORKSPACE, "ward_linkage: workspace %zu < %zu", workspace_bytes, o.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    WdArgs a{};
    a.n = (int)N; a.d = D;
    a.S = (double*)(ws + o.S); a.C = (double*)(ws + o.C); a.size = (int*)(ws + o.size); a.chain = (int*)(ws + o.chain);
    a.part = (unsigned long long*)(ws + o.part); a.st = (WdState*)(ws + o.state); a.rec = records;
    hipLaunchKernelGGL(wd_init_kernel, dim3((unsigned)min((N + 3) / 4, (int64_t)(8 * kNumCU))), dim3(256), 0, st, X, ldx, a);
    return gs_enqueue<wd_step_kernel>("ward_linkage", a, (int*)nullptr, N, 3 * (N - 1), st);
}

}  // extern "C"
