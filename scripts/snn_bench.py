"""Shared-nearest-neighbour clustering at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/dbscan_bench.py's), k = 257
(p2's --snn_k default, feat_dim + 1).  Times the three stages of snn.snn_sweep apart -- the neighbour lists (knn.kneighbors), the similarity pass
(dic_snn_similarity) and one labelling per eps (density + label passes + numbering) -- each as the median of --repeats repeats taken in alternation (lists,
similarity, every eps, and round again), so that a drift of the shared host lands on all of them alike.  Beside them the arithmetic of the similarity pass
(N k^2 list entries read, 4 bytes each, log2(next power of two >= k) + 1 LDS reads each) as rates, and the CPU baseline: M M^T with scipy.sparse on the same
lists (M the N x N membership matrix), on --cpu_rows rows of M against all of M^T and scaled by N / cpu_rows, because the full product does not fit (it fills
in within every cluster); the same rows check the GPU similarities at this size.  One JSON line at the end.

    python scripts/snn_bench.py [--n 75000] [--k 257] [--eps 51 77 103 128 154 180 206] [--min_samples 64] [--repeats 5] [--cpu_rows 2000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbscan_bench import latents, sync_time  # noqa: E402
from deep_interpolation_clustering_amd import snn  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _device_points  # noqa: E402
from deep_interpolation_clustering_amd.knn import kneighbors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--k', type=int, default=257)
    ap.add_argument('--eps', type=int, nargs='+', default=None, help='default round(k t / 10), t = 2..8')
    ap.add_argument('--min_samples', type=int, default=None, help='default k // 4')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cpu_rows', type=int, default=2000, help='rows of the scipy.sparse baseline (0: skip it)')
    ap.add_argument('--out', default=None, help='also write the JSON record to this file')
    a = ap.parse_args()
    k = a.k
    eps_values = a.eps or sorted({int(round(k * t / 10.0)) for t in range(2, 9)})
    ms = a.min_samples if a.min_samples is not None else k // 4
    x = _device_points(torch.as_tensor(latents(a.n), device='cuda'))
    snn.snn_sweep(x[:4096], min(k, 1024), [max(1, min(k, 1024) // 2)], ms)          # warm-up: module load, LDS attribute, allocator
    rec = {'metric': 'snn', 'n': a.n, 'd': 256, 'k': k, 'eps': eps_values, 'min_samples': ms, 'lists_s': [], 'similarity_s': [],
           'label_s': {e: [] for e in eps_values}}
    for _ in range(a.repeats):          # in alternation
        (_, idx), t = sync_time(lambda: kneighbors(x, k, return_device=True))
        rec['lists_s'].append(t)
        sim, t = sync_time(lambda: snn.snn_similarity(idx))
        rec['similarity_s'].append(t)
        fits = {}
        for e in eps_values:
            fits[e], t = sync_time(lambda: snn._label(idx, sim, e, ms))
            rec['label_s'][e].append(t)
    med = statistics.median
    t_sim = med(rec['similarity_s'])
    entries = a.n * k * k
    reads = (k - 1).bit_length() + 1          # log2 of the padded length, and the final compare
    rec.update(lists_median_s=med(rec['lists_s']), similarity_median_s=t_sim, label_median_s={e: med(v) for e, v in rec['label_s'].items()},
               list_entries=entries, gathered_gb_per_s=4e-9 * entries / t_sim, lds_probes_per_s=entries * reads / t_sim,
               label_passes={e: fits[e][3] for e in eps_values},
               n_clusters={e: int(fits[e][0].max() + 1) for e in eps_values}, n_noise={e: int((fits[e][0] < 0).sum()) for e in eps_values},
               n_core={e: len(fits[e][1]) for e in eps_values})
    print('lists %d x 256, k = %d: median %.4f s (%s)' % (a.n, k, rec['lists_median_s'], ' '.join('%.4f' % s for s in rec['lists_s'])))
    print('similarity pass: median %.4f s (%s); %.3g list entries, %.0f GB/s of gathered rows, %.3g LDS probes/s'
          % (t_sim, ' '.join('%.4f' % s for s in rec['similarity_s']), entries, rec['gathered_gb_per_s'], rec['lds_probes_per_s']))
    for e in eps_values:
        print('eps %d, min_samples %d: labelling median %.4f s (%s), %d label passes; %d clusters, %d core, %d noise'
              % (e, ms, rec['label_median_s'][e], ' '.join('%.4f' % s for s in rec['label_s'][e]), rec['label_passes'][e], rec['n_clusters'][e],
                 rec['n_core'][e], rec['n_noise'][e]), flush=True)
    if a.cpu_rows:
        try:
            from scipy import sparse
            h_idx, h_sim = idx.cpu().numpy(), sim.cpu().numpy()
            n = a.n
            M = sparse.csr_matrix((np.ones(n * k, np.float32), h_idx.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
            rows = np.sort(np.random.default_rng(0).choice(n, min(a.cpu_rows, n), replace=False))
            t0 = time.perf_counter()
            Mt = M.T.tocsr()
            t_tr = time.perf_counter() - t0
            t0 = time.perf_counter()
            G = (M[rows] @ Mt).tocsr()
            t_prod = time.perf_counter() - t0
            shared = np.asarray(G[np.arange(len(rows))[:, None], h_idx[rows]].todense()).astype(np.int32)
            back = np.asarray(M[h_idx[rows].ravel(), np.repeat(rows, k)]).reshape(len(rows), k) > 0          # i in L(j)
            ref = np.where(back & (h_idx[rows] != rows[:, None]), shared, 0)
            rec['cpu'] = {'rows': len(rows), 'transpose_s': t_tr, 'product_s': t_prod, 'scaled_full_s': t_tr + t_prod * n / len(rows),
                          'product_nnz_per_row': G.nnz / len(rows), 'equal_on_rows': bool(np.array_equal(ref, h_sim[rows]))}
            print('scipy.sparse M M^T on %d of %d rows: %.2f s (+ %.2f s for M^T), %.0f nonzeros per row; SCALED to all rows: %.0f s (%.0f x the similarity '
                  'pass); GPU similarities equal on these rows: %s' % (len(rows), n, t_prod, t_tr, rec['cpu']['product_nnz_per_row'],
                                                                      rec['cpu']['scaled_full_s'], rec['cpu']['scaled_full_s'] / t_sim, rec['cpu']['equal_on_rows']), flush=True)
        except ImportError:
            rec['cpu'] = None
            print('scipy is not installed: no CPU baseline')
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
