"""Exact neighbour lists at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/dbscan_bench.py's), k = 257 (p4's
--transfer_k default, feat_dim + 1).  Prints the seconds of knn.kneighbors for the self join and for a 20 000-row query set against the 75 000 points, with
their list sizes and row groups; beside them, in the same process, knn.kth_neighbor_distance on the same points -- the six pair passes the lists cannot do
without -- and the ratio; and, where sklearn imports, NearestNeighbors(n_neighbors=k, algorithm='brute').kneighbors on the same sets, with its deviation from
the GPU result.  One JSON line at the end.

    python scripts/knn_lists_bench.py [--n 75000] [--m 20000] [--k 257] [--budget_mb 0] [--sk 1] [--out FILE]
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
from deep_interpolation_clustering_amd.dbscan import _device_points  # noqa: E402
from deep_interpolation_clustering_amd.knn import kneighbors, kth_neighbor_distance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--m', type=int, default=20000)
    ap.add_argument('--k', type=int, default=257)
    ap.add_argument('--budget_mb', type=int, default=0, help='candidate budget in MiB (0: the default)')
    ap.add_argument('--sk', type=int, default=1, help='0: skip the sklearn comparison')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON record to this file')
    a = ap.parse_args()
    P = latents(a.n + a.m)
    X, Q = P[:a.n], P[a.n:]
    x = _device_points(torch.as_tensor(X, device='cuda'))
    q = _device_points(torch.as_tensor(Q, device='cuda'))
    budget = (a.budget_mb << 20) or None
    kth_neighbor_distance(x[:4096], min(a.k, 4096))          # warm-up: module load, LDS attribute, allocator
    kneighbors(x[:4096], min(a.k, 1024), Q=q[:512])
    rec = {'metric': 'knn_lists', 'n': a.n, 'm': a.m, 'd': 256, 'k': a.k, 'kth_s': [], 'self_s': [], 'cross_s': []}
    for _ in range(a.repeats):
        kth, t = sync_time(lambda: kth_neighbor_distance(x, a.k, candidate_budget=budget))
        rec['kth_s'].append(t)
    st_self, st_cross = {}, {}
    for _ in range(a.repeats):
        own, t = sync_time(lambda: kneighbors(x, a.k, candidate_budget=budget, stats=st_self, return_device=True))
        rec['self_s'].append(t)
    for _ in range(a.repeats):
        cross, t = sync_time(lambda: kneighbors(x, a.k, Q=q, candidate_budget=budget, stats=st_cross, return_device=True))
        rec['cross_s'].append(t)
    rec['self_stats'], rec['cross_stats'] = st_self, st_cross
    rec['last_column_is_kth'] = bool(np.array_equal(own[0][:, -1].cpu().numpy(), kth))
    b_kth, b_self, b_cross = min(rec['kth_s']), min(rec['self_s']), min(rec['cross_s'])
    rec['self_over_kth'] = b_self / b_kth
    print('kth_neighbor_distance %d x 256, k = %d: %.3f s (%s)' % (a.n, a.k, b_kth, ' '.join('%.3f' % s for s in rec['kth_s'])))
    for name, best, runs, st, rows in (('self join', b_self, rec['self_s'], st_self, a.n), ('%d queries' % a.m, b_cross, rec['cross_s'], st_cross, a.m)):
        print('kneighbors, %s: %.3f s (%s); groups %d, longest list %d, %.0f entries per row (%.0f MB of list storage), %.1f MB written'
              % (name, best, ' '.join('%.3f' % s for s in runs), st['groups'], st['max_list'], st['candidates'] / rows, 12 * st['candidates'] / 2 ** 20,
                 12 * a.k * rows / 2 ** 20))
    print('self join / kth_neighbor_distance = %.2f; last column == kth_neighbor_distance bit for bit: %s' % (rec['self_over_kth'], rec['last_column_is_kth']),
          flush=True)
    if a.sk:
        try:
            from sklearn.neighbors import NearestNeighbors
            X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
            nn = NearestNeighbors(n_neighbors=a.k, algorithm='brute').fit(X64)
            rec['sklearn'] = {}
            for name, pts, ours in (('self', X64, own), ('cross', Q64, cross)):
                t0 = time.perf_counter()
                d, i = nn.kneighbors(pts)
                t = time.perf_counter() - t0
                od, oi = ours[0].cpu().numpy(), ours[1].cpu().numpy()
                far = od > 0
                rec['sklearn'][name] = {'seconds': t, 'max_rel_dev': float(np.max(np.abs(d[far] - od[far]) / od[far])), 'index_agreement': float((i == oi).mean())}
                print('sklearn brute kneighbors, %s: %.2f s (%.0f x); max relative deviation %.3g, %.4f %% of the indices equal'
                      % (name, t, t / (b_self if name == 'self' else b_cross), rec['sklearn'][name]['max_rel_dev'], 100 * rec['sklearn'][name]['index_agreement']),
                      flush=True)
        except ImportError:
            rec['sklearn'] = None
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
