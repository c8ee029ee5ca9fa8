"""The k-distance graph of p2 (--cluster_method dbscan --select_eps k_distance_graph) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like
p1's output (scripts/dbscan_bench.py's), k = 256.  Prints the seconds of knn.kth_neighbor_distance, its counting passes, row groups and candidate totals, the
time of dbscan_sweep's counting pass (10 eps) on the same data -- the yardstick for "one pair pass" -- and, where sklearn imports, the time of
NearestNeighbors(n_neighbors=256, n_jobs=5).fit(X).kneighbors(X) with its deviation from the GPU result.  One JSON line at the end.

    python scripts/knn_bench.py [--n 75000] [--k 256] [--budget_mb 384] [--sk_n 75000]
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
from dbscan_bench import latents, sync_time  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _Counts, _device_points, sq_threshold  # noqa: E402
from deep_interpolation_clustering_amd.knn import kneedle_elbow, kth_neighbor_distance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--budget_mb', type=int, default=0, help='candidate budget in MiB (0: the default)')
    ap.add_argument('--sk_n', type=int, default=75000, help='points of the sklearn comparison (0: skip it)')
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    X = latents(a.n)
    x = _device_points(torch.as_tensor(X, device='cuda'))
    budget = (a.budget_mb << 20) or None
    kth_neighbor_distance(x[:4096], min(a.k, 4096))          # warm-up: module load, LDS attribute, allocator
    _Counts(x[:4096], [sq_threshold(1.0)])
    kneedle_elbow(np.arange(8.0) ** 2)          # (imports scipy.signal)
    rec = {'metric': 'knn_k_distance', 'n': a.n, 'd': 256, 'k': a.k, 'seconds': [], 'counts_ms': []}
    stats = {}
    for _ in range(a.repeats):
        stats = {}
        kth, t = sync_time(lambda: kth_neighbor_distance(x, a.k, candidate_budget=budget, stats=stats))
        rec['seconds'].append(t)
    rec.update(stats)
    eps_range = np.arange(.5, 5.1, .5)
    for _ in range(a.repeats):
        _, t = sync_time(lambda: _Counts(x, [sq_threshold(e) for e in eps_range]))
        rec['counts_ms'].append(1e3 * t)
    t0 = time.perf_counter()
    ex, ey = kneedle_elbow(np.sort(kth))
    rec['elbow_s'] = time.perf_counter() - t0
    rec['elbow'] = [ex, ey]
    best, one = min(rec['seconds']), min(rec['counts_ms']) / 1e3
    print('kth_neighbor_distance %d x 256, k = %d: %.3f s (best of %d: %s)' % (a.n, a.k, best, a.repeats, ' '.join('%.3f' % s for s in rec['seconds'])))
    print('  counting passes %d, groups %d, longest list %d, candidates %d (%.0f per row, %.0f MB of list storage), the longest list alone needs %.1f KB'
          % (stats['passes'], stats['groups'], stats['max_list'], stats['candidates'], stats['candidates'] / a.n, 12 * stats['candidates'] / 2 ** 20, stats['budget_needed'] / 2 ** 10))
    print('dbscan counting pass (10 eps) on the same points: %.1f ms; expectation (passes + 1) x that = %.3f s, measured / expectation = %.2f'
          % (1e3 * one, (stats['passes'] + 1) * one, best / ((stats['passes'] + 1) * one)))
    print('elbow of the sorted curve: x %s y %s (%.3f s on the host)' % (ex, ey, rec['elbow_s']))
    if a.sk_n:
        try:
            from sklearn.neighbors import NearestNeighbors
            Xs = X[:a.sk_n]
            t0 = time.perf_counter()
            dist = NearestNeighbors(n_neighbors=a.k, n_jobs=5).fit(Xs).kneighbors(Xs)[0][:, -1]
            rec['sklearn'] = {'n': a.sk_n, 'n_jobs': 5, 'seconds': time.perf_counter() - t0}
            ours = kth if a.sk_n == a.n else kth_neighbor_distance(x[:a.sk_n], a.k)
            rec['sklearn']['max_rel_dev'] = float(np.max(np.abs(dist - ours) / ours))
            print('sklearn NearestNeighbors(n_jobs=5).kneighbors on %d points: %.2f s; max relative deviation from the GPU result %.3g'
                  % (a.sk_n, rec['sklearn']['seconds'], rec['sklearn']['max_rel_dev']), flush=True)
        except ImportError:
            rec['sklearn'] = None
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
