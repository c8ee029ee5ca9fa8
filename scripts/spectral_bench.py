"""Spectral clustering at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/dbscan_bench.py's), k = 10 (sklearn's and
p2's default) and k = 257 (feat_dim + 1), m = 10 eigenpairs.  Times the four stages of spectral.SpectralClustering apart -- the neighbour lists
(knn.kneighbors), the graph build (spectral.symmetrise_lists), the decomposition (spectral.eigsh_largest) and the assignment (the ten k-means fits of
KMeans(10, n_init=10) on the embedding) -- each as the median of --repeats repeats taken in alternation (every stage of every k, and round again), so that a
drift of the shared host lands on all of them alike.  For the decomposition: the outer iterations, the SpMMs, and the fused SpMM kernel timed alone on a block of
the solver's width (--spmm_calls calls between two synchronisations), as ms per call and as GB/s of the bytes it must move -- 5 bytes per CSR entry, the dd
vector, X read and Y written once -- against the HBM roof (8 TB/s peak, about 6.3 TB/s achievable), and of the bytes it gathers (8 b per entry, served by the
caches: the block is 8 N b bytes).  --sklearn K .. also times sklearn's SpectralClustering(affinity='nearest_neighbors', eigen_solver='arpack') on the same
points on the host, once per K, AFTER the record of the GPU stages is written, and says whether its partition equals the GPU fit's up to renumbering.  One JSON line at the end.

    python scripts/spectral_bench.py [--n 75000] [--k 10 257] [--m 10] [--repeats 3] [--spmm_calls 20] [--max_iter 200] [--sklearn 10] [--gpu 1] [--out FILE]

--gpu 0 skips the device stages and runs the sklearn baseline alone (it needs no device).
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbscan_bench import latents, sync_time  # noqa: E402
from deep_interpolation_clustering_amd import spectral as S  # noqa: E402

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0
JOBS = min(16, int(os.environ.get('OMP_NUM_THREADS') or os.cpu_count() or 1))          # the host baseline's workers: a preset thread count, 16 at the most


def write(rec, out):
    line = json.dumps(rec)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')
    return line


def sklearn_once(X, k, m):
    from sklearn.cluster import SpectralClustering
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fit = SpectralClustering(n_clusters=m, affinity='nearest_neighbors', n_neighbors=k, eigen_solver='arpack', random_state=0, n_jobs=JOBS).fit(
            X.astype(np.float64))
    return time.perf_counter() - t0, fit.labels_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--k', type=int, nargs='+', default=[10, 257])
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--spmm_calls', type=int, default=20)
    ap.add_argument('--max_iter', type=int, default=200)
    ap.add_argument('--sklearn', type=int, nargs='*', default=[], help='neighbour counts to time sklearn at, on the host (none: skip it)')
    ap.add_argument('--gpu', type=int, default=1, help='0: only the sklearn baseline (no device needed)')
    ap.add_argument('--out', default=None, help='also write the JSON record to this file')
    a = ap.parse_args()
    X = latents(a.n)
    m = a.m
    rec = {'metric': 'spectral', 'n': a.n, 'd': 256, 'm': m, 'k': a.k, 'stages': {}}
    gpu_labels = {}
    if a.gpu:
        from deep_interpolation_clustering_amd.dbscan import _device_points
        from deep_interpolation_clustering_amd.kmeans import KMeans
        from deep_interpolation_clustering_amd.knn import kneighbors
        x = _device_points(torch.as_tensor(X, device='cuda'))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            S.SpectralClustering(m, n_neighbors=10, random_state=0, max_iter=3).fit(x[:4096])          # warm-up: module load, allocator
        st = {k: {'lists_s': [], 'graph_s': [], 'decomposition_s': [], 'assignment_s': [], 'spmm_ms': []} for k in a.k}
        last = {}
        for _ in range(a.repeats):          # in alternation
            for k in a.k:
                (_, idx), t = sync_time(lambda: kneighbors(x, k, return_device=True))
                st[k]['lists_s'].append(t)
                graph, t = sync_time(lambda: S.symmetrise_lists(idx))
                st[k]['graph_s'].append(t)
                del idx
                stats = {}
                (theta, V, res, n_iter, converged), t = sync_time(lambda: S.eigsh_largest(graph, m, 1e-10, a.max_iter, 0, stats))
                st[k]['decomposition_s'].append(t)
                emb = S.sign_flip(V / graph[3][:, None])
                km, t = sync_time(lambda: KMeans(m, n_init=10, random_state=0).fit(emb))
                st[k]['assignment_s'].append(t)
                B = torch.randn((a.n, stats['b']), dtype=torch.float64, device='cuda')
                Y = torch.empty_like(B)
                S.spmm(graph, B, out=Y)
                _, t = sync_time(lambda: [S.spmm(graph, B, 0.7, -0.2, out=Y) for _ in range(a.spmm_calls)])
                st[k]['spmm_ms'].append(1e3 * t / a.spmm_calls)
                last[k] = dict(n_iter=n_iter, converged=bool(converged), spmm=stats['spmm'], b=stats['b'], orth_passes=stats.get('orth_passes', 0),
                               orth_shifted=stats.get('orth_shifted', 0), nnz=int(graph[1].numel()), longest_row=int(torch.diff(graph[0]).max()),
                               largest_residual=float(res.max()), eigenvalues=[float(v) for v in theta],
                               components=int((theta >= 1 - 1e-9).sum()), cluster_sizes=np.bincount(km.labels_, minlength=m).tolist())
                gpu_labels[k] = km.labels_
                del graph, V, emb, B, Y
        med = statistics.median
        for k in a.k:
            s, info = st[k], last[k]
            ms = med(s['spmm_ms'])
            must = 5.0 * info['nnz'] + 8.0 * a.n + 8.0 * (a.n + 1) + 2 * 8.0 * a.n * info['b']
            gathered = 8.0 * info['b'] * info['nnz']
            info.update({key[:-2] + '_median_s': med(v) for key, v in s.items() if key.endswith('_s')})
            info.update(spmm_median_ms=ms, spmm_must_move_gb_per_s=must / ms * 1e-6, spmm_gathered_gb_per_s=gathered / ms * 1e-6,
                        spmm_share_of_hbm_peak=must / ms * 1e-6 / HBM_PEAK_GBS, spmm_share_of_decomposition=info['spmm'] * ms * 1e-3 / med(s['decomposition_s']),
                        raw=s)
            rec['stages'][k] = info
            print('k = %d: lists %.4f s, graph build %.4f s (%d entries, longest row %d), decomposition %.4f s (%d outer iterations, %d SpMMs, b = %d, '
                  'converged %s, largest residual %.3g, %d components), assignment (ten k-means fits) %.4f s'
                  % (k, info['lists_median_s'], info['graph_median_s'], info['nnz'], info['longest_row'], info['decomposition_median_s'], info['n_iter'],
                     info['spmm'], info['b'], info['converged'], info['largest_residual'], info['components'], info['assignment_median_s']))
            print('        SpMM alone: %.4f ms per call; %.0f GB/s of the bytes it must move (%.1f %% of the 8 TB/s HBM peak, %.1f %% of the 6.3 TB/s achievable), '
                  '%.0f GB/s gathered from the caches; the SpMMs are %.0f %% of the decomposition'
                  % (ms, info['spmm_must_move_gb_per_s'], 100 * info['spmm_share_of_hbm_peak'], 100 * info['spmm_must_move_gb_per_s'] / HBM_ACHIEVABLE_GBS,
                     info['spmm_gathered_gb_per_s'], 100 * info['spmm_share_of_decomposition']))
            print('        eigenvalues %s; cluster sizes %s' % (' '.join('%.6f' % v for v in info['eigenvalues']), info['cluster_sizes']), flush=True)
        write(rec, a.out)
    rec['sklearn'] = {}
    for k in a.sklearn:
        try:
            t, labels = sklearn_once(X, k, m)
        except ImportError:
            print('sklearn is not installed: no CPU baseline')
            break
        rec['sklearn'][k] = {'fit_s': t, 'jobs': JOBS, 'cluster_sizes': np.bincount(labels, minlength=m).tolist()}
        if k in gpu_labels:          # the same partition up to renumbering: as many distinct label pairs as labels on either side
            pairs = len(set(zip(labels.tolist(), gpu_labels[k].tolist())))
            rec['sklearn'][k]['same_partition'] = bool(pairs == len(set(labels.tolist())) == len(set(gpu_labels[k].tolist())))
        print('sklearn SpectralClustering(nearest_neighbors, arpack), k = %d, on the host (%d workers), once: %.1f s%s'
              % (k, JOBS, t, '; same partition as the GPU fit: %s' % rec['sklearn'][k]['same_partition'] if k in gpu_labels else ''), flush=True)
        write(rec, a.out)
    print(write(rec, a.out))


if __name__ == '__main__':
    main()
