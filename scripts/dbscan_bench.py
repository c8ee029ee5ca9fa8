"""DBSCAN sweep of p2 (--cluster_method dbscan) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (clusters of
several widths + a diffuse background), eps = 0.5 .. 5.0 (np.arange(.5, 5.1, .5)), min_samples = 257.  Prints per-phase GPU times (the counting
pass, every components pass, the silhouettes), the components passes and band pairs per eps, the whole sweep, and sklearn's precomputed path
(pairwise_distances + DBSCAN(metric='precomputed')) on 20 000 of the points on 16 threads for comparison.  One JSON line at the end.

    python scripts/dbscan_bench.py [--n 75000] [--sk_n 20000] [--sk_budget 120]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd import cluster_stats  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _Counts, _device_points, sq_threshold  # noqa: E402


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


def gpu_sweep(X, eps_range, min_samples, verbose=True):
    x = _device_points(torch.as_tensor(X, device='cuda'))
    rec = {'eps': [float(e) for e in eps_range], 'passes': [], 'pass_ms': [], 'silhouette_ms': [], 'n_clusters': []}
    t0 = time.perf_counter()
    cp, rec['counts_ms'] = sync_time(lambda: _Counts(x, [sq_threshold(e) for e in eps_range]))
    rec['counts_ms'] *= 1e3
    rec['band_pairs'] = cp.n_band
    for e in range(len(eps_range)):
        (lab, core, passes), t = sync_time(lambda: cp.components(e, min_samples))
        rec['passes'].append(passes)
        rec['pass_ms'].append(1e3 * t / max(passes, 1))
        ncl = len(set(lab.tolist())) - (1 if (lab == -1).any() else 0)
        rec['n_clusters'].append(ncl)
        ts = 0.0
        if ncl > 1:
            keep = lab != -1
            _, t1 = sync_time(lambda: cluster_stats.silhouette_score(x, lab))
            _, t2 = sync_time(lambda: cluster_stats.silhouette_score(x[torch.as_tensor(keep, device='cuda')], lab[keep]))
            ts = t1 + t2
        rec['silhouette_ms'].append(1e3 * ts)
        if verbose:
            print('eps %.1f: core %d clusters %d noise %d | %d components passes, %.1f ms each | silhouettes %.1f ms'
                  % (eps_range[e], len(np.flatnonzero(core)), ncl, int((lab == -1).sum()), passes, rec['pass_ms'][-1], 1e3 * ts), flush=True)
    torch.cuda.synchronize()
    rec['sweep_s'] = time.perf_counter() - t0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--sk_n', type=int, default=20000)
    ap.add_argument('--sk_budget', type=float, default=120.0, help='seconds of sklearn fits at most (eps are taken in order)')
    a = ap.parse_args()
    eps_range = np.arange(.5, 5.1, .5)
    X = latents(a.n)
    gpu_sweep(X[:4096], eps_range[:2], 257, verbose=False)             # warm-up: module load, LDS attribute, allocator
    rec = gpu_sweep(X, eps_range, 257)
    print('counting pass (10 eps): %.1f ms, band pairs %d' % (rec['counts_ms'], rec['band_pairs']))
    print('whole sweep (counts + components + 2 silhouettes per eps): %.2f s' % rec['sweep_s'])
    small = gpu_sweep(X[:a.sk_n], eps_range, 257, verbose=False)
    print('GPU sweep on %d points: %.2f s' % (a.sk_n, small['sweep_s']))
    sk = {'n': a.sk_n, 'threads': 16, 'fits': []}
    try:
        from sklearn.cluster import DBSCAN
        from sklearn.metrics import pairwise_distances
        Xs = X[:a.sk_n]
        t = time.perf_counter()
        D = pairwise_distances(Xs, n_jobs=16)
        sk['pairwise_s'] = time.perf_counter() - t
        spent = sk['pairwise_s']
        for e in eps_range:
            if spent > a.sk_budget:
                break
            t = time.perf_counter()
            DBSCAN(e, min_samples=257, metric='precomputed', n_jobs=16).fit(D)
            dt = time.perf_counter() - t
            spent += dt
            sk['fits'].append([float(e), dt])
            print('sklearn eps %.1f on %d points: %.2f s' % (e, a.sk_n, dt), flush=True)
        del D
    except ImportError:
        sk = None
    print(json.dumps({'metric': 'dbscan_p2_sweep', 'n': a.n, 'd': 256, 'gpu': rec, 'gpu_small': {'n': a.sk_n, 'sweep_s': small['sweep_s']},
                      'sklearn': sk}))


if __name__ == '__main__':
    main()
