"""Ward linkage of p2 / p4 (--cluster_method ward) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/optics_bench.py's recipe).  Prints the wall time of ``ward_linkage`` and of its parts: the device part (one init kernel and 3 (N - 1) enqueued
launches, of which ``steps`` pushed or merged and the rest returned at once), microseconds per enqueued launch and per launch that did work, and the host
finish (the stable sort of the heights and scipy's relabelling, a Python loop over the N - 1 merges); then ``cut_many`` for K = 2..10, and scipy's
``linkage(., 'ward')`` on --sp_n of the points for scale.  scipy needs the condensed matrix (8 N (N - 1) / 2 bytes) and O(N^2) time: its time at the full
size is given as the N^2 extrapolation of the measured one, not as a measurement.  One JSON line at the end.

    python scripts/ward_bench.py [--n 75000] [--sp_n 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd.consensus import _relabel  # noqa: E402
from deep_interpolation_clustering_amd.ward import _device_points, cut_many, ward_linkage, ward_records  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--sp_n', type=int, default=4000, help='points of the scipy comparison (0: none)')
    a = ap.parse_args()
    X = latents(a.n)
    x = _device_points(torch.as_tensor(X, device='cuda'))
    n, d = x.shape
    ward_linkage(x[:4096])             # warm-up: module load, LDS attribute, allocator
    stats = {}
    rec, t_dev = sync_time(lambda: ward_records(x, stats))
    t = time.perf_counter()
    Z = _relabel(rec, n)
    t_host = time.perf_counter() - t
    Z2, t_all = sync_time(lambda: ward_linkage(x))
    assert np.array_equal(Z, Z2)
    t = time.perf_counter()
    cuts = cut_many(Z, range(2, 11))
    t_cut = time.perf_counter() - t
    launches, steps = stats['launches'], stats['steps']
    gpu = {'wall_s': t_all, 'device_s': t_dev, 'host_finish_s': t_host, 'cut_2_to_10_s': t_cut, 'launches': launches, 'steps': steps,
           'steps_per_merge': steps / (n - 1), 'us_per_launch': 1e6 * t_dev / launches, 'us_per_step': 1e6 * t_dev / steps,
           'workspace_bytes': 2 * 8 * n * d + 8 * n}
    print('ward_linkage %d x %d: %.2f s (device %.2f s, host finish %.2f s); cut_many K = 2..10: %.2f s' % (n, d, t_all, t_dev, t_host, t_cut))
    print('device: %d launches enqueued, %d pushed or merged (%.2f per merge): %.2f us per enqueued launch, %.2f us per launch that did work'
          % (launches, steps, gpu['steps_per_merge'], gpu['us_per_launch'], gpu['us_per_step']), flush=True)
    print('sizes at K = 10: %s' % np.bincount(cuts[10]).tolist())
    sp = None
    if a.sp_n:
        try:
            from scipy.cluster.hierarchy import linkage
            Xs = X[:a.sp_n].astype(np.float64)
            t = time.perf_counter()
            ref = linkage(Xs, 'ward')
            t_fit = time.perf_counter() - t
            Zs, t_small = sync_time(lambda: ward_linkage(x[:a.sp_n]))
            sp = {'n': a.sp_n, 'fit_s': t_fit, 'gpu_s': t_small, 'same_merges': bool(np.array_equal(ref[:, [0, 1, 3]], Zs[:, [0, 1, 3]])),
                  'max_rel_height_diff': float(np.max(np.abs(ref[:, 2] - Zs[:, 2]) / ref[:, 2])),
                  'fit_s_extrapolated_to_n': t_fit * (n / a.sp_n) ** 2, 'condensed_bytes_at_n': 4 * n * (n - 1)}
            print('scipy linkage(ward) on %d points: %.2f s (GPU: %.3f s, same merges: %s, heights within %.1e); N^2 extrapolation to %d points: %.0f s and a '
                  '%.1f GB condensed matrix' % (a.sp_n, t_fit, t_small, sp['same_merges'], sp['max_rel_height_diff'], n, sp['fit_s_extrapolated_to_n'],
                                                4 * n * (n - 1) / 1e9))
        except ImportError:
            pass
    print(json.dumps({'metric': 'ward_linkage', 'n': n, 'd': d, 'gpu': gpu, 'scipy': sp}))


if __name__ == '__main__':
    main()
