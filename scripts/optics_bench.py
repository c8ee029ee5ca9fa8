"""OPTICS of p2 (--cluster_method optics) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/dbscan_bench.py's
recipe), min_samples = 257, max_eps = inf.  Prints the wall time of ``optics_graph`` and of its two phases (the core distances, the N - 1 steps of the main
loop), steps per second, microseconds per step and the effective bytes per second of the row pass counted as N * D * 4 bytes per step (the pass skips the
rows of processed points, half of them on average, so the bytes actually moved are about half of that); then the host-side xi extraction, and sklearn's
``OPTICS(metric='precomputed')`` on the f64 distance matrix of --sk_n of the points for comparison.  sklearn's loop is O(N^2) with N sequential steps: its
time at 75 000 points is given as the N^2 extrapolation of the measured one, not as a measurement.  One JSON line at the end.

    python scripts/optics_bench.py [--n 75000] [--sk_n 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd import knn  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _device_points  # noqa: E402
from deep_interpolation_clustering_amd.optics import around15, cluster_optics_xi, device_walk, optics_graph  # noqa: E402


def latents(n, seed=0):
    rng = np.random.default_rng(seed)
    k = 12
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(int(n * 0.92), np.full(k, 1 / k))
    widths = rng.uniform(0.04, 0.12, k)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)]
                       + [rng.normal(0, 0.45, (n - int(sizes.sum()), 256))])
    return rng.permutation(X).astype(np.float32)


def sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def main_loop(x, core):
    """The N - 1 steps alone (the C entry point, as optics_graph calls it)."""
    return device_walk(x, core, 'dic_optics_workspace', 'dic_optics_order', float('inf'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--min_samples', type=int, default=257)
    ap.add_argument('--sk_n', type=int, default=4000, help='points of the sklearn comparison (0: none)')
    a = ap.parse_args()
    X = latents(a.n)
    x = _device_points(torch.as_tensor(X, device='cuda'))
    n, d = x.shape
    optics_graph(x[:4096], a.min_samples)             # warm-up: module load, LDS attribute, allocator
    core, t_core = sync_time(lambda: around15(knn.kth_neighbor_distance(x, a.min_samples)))
    _, t_loop = sync_time(lambda: main_loop(x, core))
    (ordering, core2, reach, pred), t_all = sync_time(lambda: optics_graph(x, a.min_samples))
    assert np.array_equal(core, core2)
    steps = n - 1
    rec = {'wall_s': t_all, 'core_s': t_core, 'loop_s': t_loop, 'steps': steps, 'steps_per_s': steps / t_loop, 'us_per_step': 1e6 * t_loop / steps,
           'row_pass_GBps': steps * n * d * 4 / t_loop / 1e9}
    print('optics_graph %d x %d, min_samples %d: %.2f s (core distances %.3f s, main loop %.2f s)' % (n, d, a.min_samples, t_all, t_core, t_loop))
    print('main loop: %d steps, %.0f steps/s, %.2f us per step, %.0f GB/s at N*D*4 = %.1f MB per step'
          % (steps, rec['steps_per_s'], rec['us_per_step'], rec['row_pass_GBps'], n * d * 4 / 1e6), flush=True)
    t = time.perf_counter()
    labels, hier = cluster_optics_xi(reachability=reach, predecessor=pred, ordering=ordering, min_samples=a.min_samples, min_cluster_size=a.min_samples, xi=.05)
    rec['xi_s'] = time.perf_counter() - t
    rec['n_clusters'] = int(labels.max() + 1)
    rec['n_noise'] = int((labels == -1).sum())
    print('xi extraction on the host: %.2f s, %d clusters, %d noise, %d nested clusters in the hierarchy' % (rec['xi_s'], rec['n_clusters'], rec['n_noise'], len(hier)))
    sk = None
    if a.sk_n:
        try:
            from sklearn.cluster import OPTICS as SkOPTICS
            Xs = X[:a.sk_n].astype(np.float64)
            t = time.perf_counter()
            D = np.empty((a.sk_n, a.sk_n))
            for s in range(0, a.sk_n, 64):
                diff = Xs[s:s + 64, None, :] - Xs[None, :, :]
                D[s:s + 64] = np.sqrt(np.einsum('ijk,ijk->ij', diff, diff))
            t_d = time.perf_counter() - t
            t = time.perf_counter()
            ref = SkOPTICS(min_samples=a.min_samples, metric='precomputed').fit(D)
            t_fit = time.perf_counter() - t
            (o_small, _, _, _), t_small = sync_time(lambda: optics_graph(x[:a.sk_n], a.min_samples))
            sk = {'n': a.sk_n, 'matrix_s': t_d, 'fit_s': t_fit, 'gpu_s': t_small, 'same_ordering': bool(np.array_equal(ref.ordering_, o_small)),
                  'fit_s_extrapolated_to_n': t_fit * (n / a.sk_n) ** 2, 'matrix_bytes_at_n': 8 * n * n}
            print('sklearn OPTICS(metric=precomputed) on %d points: matrix %.1f s, fit %.1f s (GPU: %.3f s, same ordering: %s); N^2 extrapolation to %d points: '
                  '%.0f s and a %.0f GB matrix' % (a.sk_n, t_d, t_fit, t_small, sk['same_ordering'], n, sk['fit_s_extrapolated_to_n'], 8 * n * n / 1e9))
        except ImportError:
            pass
    print(json.dumps({'metric': 'optics_graph', 'n': n, 'd': d, 'min_samples': a.min_samples, 'gpu': rec, 'sklearn': sk}))


if __name__ == '__main__':
    main()
