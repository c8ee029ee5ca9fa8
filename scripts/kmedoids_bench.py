"""k-medoids of p2 / p4 (--cluster_method kmedoids) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/ward_bench.py's recipe), K = 4 and K = 10 from BUILD.  Per K: the milliseconds of one delta pass (regrouping the column operand, the tile pass, the
reduction) and of one exact stage (selection, the exact kernel over the listed candidates, the pick) in the state BUILD leaves, and of the whole fit (planes,
BUILD, SWAP); every figure is the best of 3 windows after a warm-up, a window being ``--reps`` repetitions inside one host clock that ends in a device
synchronise.  The candidates sent to the exact stage are printed per BUILD step and per SWAP iteration.  For comparison: one ``dic_dbscan_counts`` pass over
the same points -- the same tile loop with a lighter epilogue.  That call includes its plane preparation and the host read of its band count; the delta
pass figure includes the regrouping and the reduction but not the one-off preparation, which is timed on its own, so that the ratio can be read either
way.  As a CPU figure, the numpy yardstick of tests/test_kmedoids_host.py on ``--cpu_n`` of the points.  One JSON line at the end.

    python scripts/kmedoids_bench.py [--n 75000] [--ks 4 10] [--reps 5] [--cpu_n 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import kmedoids as KM  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _Counts, sq_threshold  # noqa: E402


def latents(n, seed=0):
    rng = np.random.default_rng(seed)
    k = 12
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(int(n * 0.92), np.full(k, 1 / k))
    widths = rng.uniform(0.04, 0.12, k)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)]
                       + [rng.normal(0, 0.45, (n - int(sizes.sum()), 256))])
    return rng.permutation(X).astype(np.float32)


def best_of_windows(fn, reps, windows=3):
    """Seconds per repetition: the best of ``windows`` windows of ``reps`` repetitions, after one warm-up repetition."""
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(windows):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) / reps)
    return best


def exact_stage(pts, m, k):
    """``_Points.search`` behind the pass, without the host read."""
    L, st = N.lib(), N.stream_of(pts.x)
    N.check(L.dic_kmedoids_select(pts.n, pts.k_max, k, N.ptr(pts.g), N.ptr(pts.r), N.ptr(pts.e), N.ptr(m), k, N.ptr(pts.list), N.ptr(pts.count), N.ptr(pts.ws),
                                  pts.ws.numel(), st), 'dic_kmedoids_select')
    N.check(L.dic_kmedoids_exact(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, N.ptr(pts.list), pts.n, N.ptr(pts.count), 2, N.ptr(pts.nearest), N.ptr(pts.dn),
                                 N.ptr(pts.ds), k, N.ptr(pts.delta), st), 'dic_kmedoids_exact')
    N.check(L.dic_kmedoids_pick(N.ptr(pts.list), pts.n, N.ptr(pts.count), N.ptr(pts.delta), k, N.ptr(pts.out), st), 'dic_kmedoids_pick')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--ks', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eps', type=float, default=0.5, help='eps of the DBSCAN counting pass of the comparison')
    ap.add_argument('--cpu_n', type=int, default=4000, help='points of the numpy yardstick on the CPU (0: skip)')
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    KM.KMedoids(4).fit(x[:2048])                          # warm-up: code objects, the LDS attribute, the allocator
    out = {'metric': 'kmedoids', 'n': a.n, 'd': x.shape[1], 'reps': a.reps, 'ks': {}}
    for k in a.ks:
        pts = KM._Points(x, k)
        torch.cuda.synchronize()
        t = time.perf_counter()
        med, build_counts = pts.build(k)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t
        m = torch.as_tensor(med, dtype=torch.int32, device=x.device)
        centre = x.double().mean(dim=0).float().contiguous()
        prepare_s = best_of_windows(lambda: N.check(N.lib().dic_kmedoids_prepare(N.ptr(x), x.stride(0), pts.n, pts.d, N.ptr(centre), k, N.ptr(pts.ws),
                                                                                 pts.ws.numel(), N.stream_of(x)), 'dic_kmedoids_prepare'), a.reps)
        assign_s = best_of_windows(lambda: pts.assign(m), a.reps)
        first_s = best_of_windows(lambda: pts.delta_pass(0, 0), a.reps)
        build_pass_s = best_of_windows(lambda: pts.delta_pass(k, 1), a.reps)
        pass_s = best_of_windows(lambda: pts.delta_pass(k, 2), a.reps)
        exact_s = best_of_windows(lambda: exact_stage(pts, m, k), a.reps)
        listed = int(pts.count.item())
        td = float(pts.td.item())
        e_over_td = float(pts.e.max().item()) / td
        del pts
        fits = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fit = KM.KMedoids(k).fit(x)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t)
        row = {'build_s': build_s, 'prepare_ms': 1e3 * prepare_s, 'assign_ms': 1e3 * assign_s, 'first_build_pass_ms': 1e3 * first_s, 'build_pass_ms': 1e3 * build_pass_s,
               'delta_pass_ms': 1e3 * pass_s, 'exact_stage_ms': 1e3 * exact_s, 'exact_stage_candidates': listed, 'max_E_over_TD': e_over_td,
               'fit_s': min(fits), 'fit_s_all': fits, 'n_iter': fit.n_iter_, 'converged': fit.converged_, 'inertia': fit.inertia_,
               'build_n_exact': list(fit.build_n_exact_), 'n_exact': list(fit.n_exact_), 'inertia_after_build': td}
        out['ks'][k] = row
        print('K = %d: prepare %.2f ms, assign %.2f ms, delta pass %.2f ms (BUILD step %.2f ms, first BUILD step %.2f ms), exact stage %.2f ms for %d candidate(s), '
              'max E / TD %.3g; BUILD %.3f s; whole fit %.3f s (%d swaps, converged %s, TD %.6g after BUILD, %.6g at the end)'
              % (k, row['prepare_ms'], row['assign_ms'], row['delta_pass_ms'], row['build_pass_ms'], row['first_build_pass_ms'], row['exact_stage_ms'], listed, e_over_td, build_s,
                 row['fit_s'], fit.n_iter_, fit.converged_, td, fit.inertia_), flush=True)
        print('K = %d: candidates sent to the exact stage: BUILD steps %s, SWAP iterations %s' % (k, row['build_n_exact'], row['n_exact']), flush=True)
    thr = sq_threshold(a.eps)
    counts_s = best_of_windows(lambda: _Counts(x, [thr]), a.reps)
    out['dbscan_counts_ms'] = 1e3 * counts_s
    for k in a.ks:
        out['ks'][k]['pass_over_dbscan_counts'] = out['ks'][k]['delta_pass_ms'] / out['dbscan_counts_ms']
    print('dic_dbscan_counts over the same points (eps %.3g, one threshold): %.2f ms; delta pass / counting pass = %s'
          % (a.eps, out['dbscan_counts_ms'], {k: round(out['ks'][k]['pass_over_dbscan_counts'], 3) for k in a.ks}), flush=True)
    if a.cpu_n:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_kmedoids_host import dist_matrix, y_build, y_pam
        sub = X[:a.cpu_n]
        t = time.perf_counter()
        Dm = dist_matrix(sub)
        t_matrix = time.perf_counter() - t
        t = time.perf_counter()
        med = y_build(Dm, a.ks[0])[0]
        t_build = time.perf_counter() - t
        t = time.perf_counter()
        ref = y_pam(Dm, med)
        t_swap = time.perf_counter() - t
        out['cpu'] = {'n': a.cpu_n, 'k': a.ks[0], 'matrix_s': t_matrix, 'build_s': t_build, 'swap_s': t_swap, 'searches': ref.n_iter + 1,
                      'cpus': len(os.sched_getaffinity(0))}
        print('numpy yardstick on %d points, K = %d, on the CPU (%d threads allowed): matrix %.2f s, BUILD %.2f s, SWAP %.2f s (%d searches)'
              % (a.cpu_n, a.ks[0], out['cpu']['cpus'], t_matrix, t_build, t_swap, ref.n_iter + 1), flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
