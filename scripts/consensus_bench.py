"""Consensus clustering of p2 / p4 (--cluster_method consensus) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/optics_bench.py's recipe), H = 100 resamples of 80 % of the points, one K.  Prints the wall time of the H k-means fits that fill the label matrix,
of one pair pass for every combination of its outputs (histogram, distance matrix, row sums), and of the average-linkage agglomeration: its 3 (N - 1)
launches, how many of them did work (pushed or merged; the rest find the dendrogram finished and return), microseconds per launch and per working launch;
then the host finish (stable sort, relabelling, cut) and the peak device memory.  One JSON line at the end.

    python scripts/consensus_bench.py [--n 75000] [--reps 100] [--k 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import consensus  # noqa: E402
from optics_bench import latents, sync_time  # noqa: E402


def linkage_on_device(D):
    """The C entry point as consensus.average_linkage calls it: (records on the device, (chain length, merges, working launches))."""
    L = N.lib()
    n = D.shape[0]
    ws = torch.empty(L.dic_linkage_average_workspace(n), dtype=torch.uint8, device=D.device)
    rec = torch.empty((n - 1, 4), dtype=torch.float64, device=D.device)
    N.check(L.dic_linkage_average(N.ptr(D), n, N.ptr(rec), N.ptr(ws), ws.numel(), N.stream_of(D)), 'dic_linkage_average')
    return rec, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--k', type=int, default=4)
    a = ap.parse_args()
    x = torch.as_tensor(latents(a.n), device='cuda')
    n, d = x.shape
    consensus.ConsensusKMeans([a.k], reps=4).fit(x[:2048])             # warm-up: module load, allocator
    torch.cuda.reset_peak_memory_stats()
    resamples = consensus.draw_resamples(n, a.reps, 0.8, 0)
    L, t_fit = sync_time(lambda: consensus.label_matrix(x, a.k, resamples))
    print('label matrix %d x %d, K = %d: %d k-means fits of %d points in %.2f s (%.1f ms per fit)'
          % (n, a.reps, a.k, a.reps, len(resamples[0]), t_fit, 1e3 * t_fit / a.reps), flush=True)
    rec = {'fits_s': t_fit, 'ms_per_fit': 1e3 * t_fit / a.reps}
    (hist, _, _), rec['pairs_hist_s'] = sync_time(lambda: consensus.consensus_pairs(L))
    cdf, area = consensus.cdf_area(hist)
    (_, _, D), rec['pairs_distance_s'] = sync_time(lambda: consensus.consensus_pairs(L, want_distance=True, want_hist=False))
    del D
    (_, _, D), rec['pairs_hist_distance_s'] = sync_time(lambda: consensus.consensus_pairs(L, want_distance=True))
    pairs = n * (n - 1) // 2
    print('pair pass (%.2e pairs x %d resamples): histogram %.1f ms, distance matrix (%.1f GB) %.1f ms, both %.1f ms; area under the CDF %.4f'
          % (pairs, a.reps, 1e3 * rec['pairs_hist_s'], 8 * n * n / 1e9, 1e3 * rec['pairs_distance_s'], 1e3 * rec['pairs_hist_distance_s'], area), flush=True)
    (records, ws), t_link = sync_time(lambda: linkage_on_device(D))
    state = ws[-256:-244].view(torch.int32).cpu().numpy()
    launches, working = 3 * (n - 1), int(state[2])
    assert int(state[1]) == n - 1
    rec.update(linkage_s=t_link, launches=launches, working_launches=working, us_per_launch=1e6 * t_link / launches)
    print('average linkage: %d launches in %.2f s (%.2f us per launch), %d of them pushed or merged (%d merges)'
          % (launches, t_link, rec['us_per_launch'], working, n - 1), flush=True)
    del D
    t = time.perf_counter()
    Z = consensus._relabel(records.cpu().numpy(), n)
    labels = consensus.cut_linkage(Z, a.k)
    rec['host_finish_s'] = time.perf_counter() - t
    (_, rowsum, _), rec['pairs_rowsum_s'] = sync_time(lambda: consensus.consensus_pairs(L, y=labels - 1, want_hist=False, n_clusters=a.k))
    (_, _, _), rec['pairs_hist_rowsum_s'] = sync_time(lambda: consensus.consensus_pairs(L, y=labels - 1, n_clusters=a.k))
    cluster, _ = consensus.consensus_summaries(rowsum, labels - 1)
    rec['peak_bytes'] = int(torch.cuda.max_memory_allocated())
    rec['cluster_sizes'] = np.bincount(labels)[1:].tolist()
    print('host finish (sort, relabel, cut): %.2f s; row sums %.1f ms, with the histogram %.1f ms; cluster sizes %s, cluster consensus %s'
          % (rec['host_finish_s'], 1e3 * rec['pairs_rowsum_s'], 1e3 * rec['pairs_hist_rowsum_s'], rec['cluster_sizes'], np.round(cluster, 4).tolist()))
    print('peak device memory %.2f GB (the distance matrix is %.2f GB)' % (rec['peak_bytes'] / 1e9, 8 * n * n / 1e9))
    print(json.dumps({'metric': 'consensus', 'n': n, 'd': d, 'reps': a.reps, 'k': a.k, 'area': area, 'gpu': rec}))


if __name__ == '__main__':
    main()
