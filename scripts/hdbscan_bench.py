"""HDBSCAN of p2 (--cluster_method hdbscan) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/optics_bench.py's
recipe), min_samples = 257.  Prints the wall time of ``hdbscan_mst`` and of its two phases (the core distances, the N - 1 steps of Prim's walk), steps per
second, microseconds per step and the effective bytes per second of the row pass counted as N * D * 4 bytes per step (the pass skips the rows of points in
the tree, half of them on average, so the bytes actually moved are about half of that); then the host-side extraction (single-linkage tree, condensed tree
and labels for min_cluster_size = min_samples), and sklearn's ``HDBSCAN(metric='precomputed', algorithm='brute')`` on the f64 distance matrix of --sk_n of
the points for comparison.  sklearn's Prim is O(N^2) with N sequential steps: its time at 75 000 points is given as the N^2 extrapolation of the measured
one, not as a measurement.  One JSON line at the end.

    python scripts/hdbscan_bench.py [--n 75000] [--sk_n 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd import knn  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _device_points  # noqa: E402
from deep_interpolation_clustering_amd.hdbscan import condense_tree, hdbscan_mst, single_linkage_tree, tree_to_labels  # noqa: E402
from deep_interpolation_clustering_amd.optics import device_walk  # noqa: E402
from optics_bench import latents, sync_time  # noqa: E402


def walk(x, core):
    """The N - 1 steps alone (the C entry point, as hdbscan_mst calls it)."""
    return device_walk(x, core, 'dic_hdbscan_workspace', 'dic_hdbscan_mst')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--min_samples', type=int, default=257)
    ap.add_argument('--sk_n', type=int, default=4000, help='points of the sklearn comparison (0: none)')
    a = ap.parse_args()
    X = latents(a.n)
    x = _device_points(torch.as_tensor(X, device='cuda'))
    n, d = x.shape
    hdbscan_mst(x[:4096], min(a.min_samples, 4096))             # warm-up: module load, LDS attribute, allocator
    core, t_core = sync_time(lambda: knn.kth_neighbor_distance(x, a.min_samples))
    _, t_walk = sync_time(lambda: walk(x, core))
    (ordering, core2, reach, pred), t_all = sync_time(lambda: hdbscan_mst(x, a.min_samples))
    assert np.array_equal(core, core2)
    steps = n - 1
    rec = {'wall_s': t_all, 'core_s': t_core, 'walk_s': t_walk, 'steps': steps, 'steps_per_s': steps / t_walk, 'us_per_step': 1e6 * t_walk / steps,
           'row_pass_GBps': steps * n * d * 4 / t_walk / 1e9}
    print('hdbscan_mst %d x %d, min_samples %d: %.2f s (core distances %.3f s, walk %.2f s)' % (n, d, a.min_samples, t_all, t_core, t_walk))
    print('walk: %d steps, %.0f steps/s, %.2f us per step, %.0f GB/s at N*D*4 = %.1f MB per step'
          % (steps, rec['steps_per_s'], rec['us_per_step'], rec['row_pass_GBps'], n * d * 4 / 1e6), flush=True)
    t = time.perf_counter()
    slt = single_linkage_tree(ordering, reach)
    rec['single_linkage_s'] = time.perf_counter() - t
    t = time.perf_counter()
    condensed = condense_tree(slt, a.min_samples)
    labels, _ = tree_to_labels(slt, a.min_samples, condensed=condensed)
    rec['extract_s'] = time.perf_counter() - t
    rec['n_clusters'] = int(labels.max() + 1)
    rec['n_noise'] = int((labels == -1).sum())
    print('extraction on the host: single-linkage tree %.2f s, condensed tree and labels %.2f s, %d clusters, %d noise'
          % (rec['single_linkage_s'], rec['extract_s'], rec['n_clusters'], rec['n_noise']))
    sk = None
    if a.sk_n:
        try:
            from sklearn.cluster import HDBSCAN as SkHDBSCAN
            Xs = X[:a.sk_n].astype(np.float64)
            k = min(a.min_samples, a.sk_n)
            t = time.perf_counter()
            D = np.empty((a.sk_n, a.sk_n))
            for s in range(0, a.sk_n, 64):
                diff = Xs[s:s + 64, None, :] - Xs[None, :, :]
                D[s:s + 64] = np.sqrt(np.einsum('ijk,ijk->ij', diff, diff))
            t_d = time.perf_counter() - t
            t = time.perf_counter()
            ref = SkHDBSCAN(min_cluster_size=k, min_samples=k, metric='precomputed', algorithm='brute').fit(D)
            t_fit = time.perf_counter() - t
            (o_small, _, r_small, _), t_small = sync_time(lambda: hdbscan_mst(x[:a.sk_n], k))
            ours = tree_to_labels(single_linkage_tree(o_small, r_small), k)[0]
            sk = {'n': a.sk_n, 'matrix_s': t_d, 'fit_s': t_fit, 'gpu_s': t_small, 'same_labels': bool(np.array_equal(ref.labels_, ours)),
                  'fit_s_extrapolated_to_n': t_fit * (n / a.sk_n) ** 2, 'matrix_bytes_at_n': 8 * n * n}
            print('sklearn HDBSCAN(metric=precomputed) on %d points: matrix %.1f s, fit %.1f s (GPU: %.3f s, same labels: %s -- sklearn sorts equal weights '
                  'unstably); N^2 extrapolation to %d points: %.0f s and a %.0f GB matrix'
                  % (a.sk_n, t_d, t_fit, t_small, sk['same_labels'], n, sk['fit_s_extrapolated_to_n'], 8 * n * n / 1e9))
        except ImportError:
            pass
    print(json.dumps({'metric': 'hdbscan_mst', 'n': n, 'd': d, 'min_samples': a.min_samples, 'gpu': rec, 'sklearn': sk}))


if __name__ == '__main__':
    main()
