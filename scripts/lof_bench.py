"""The local outlier factor (lof.py) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/kmedoids_bench.py's recipe),
at k = 20 alone and for the sweep k = 10, 15, .., 50 from one join.  Writes profiles/lof_bench.json and prints it as one JSON line.

Per configuration, host-clock figures (the best of 3 windows of ``--reps`` repetitions after a warm-up, a window ending in a device synchronise): the
``kneighbors`` self join at max(ks) + 1; ``drop_self`` (the self column dropped with torch on the device); ``lof_from_lists`` (the index check, the k-distance
columns and the two kernels); and the whole ``lof_sweep``.  Device times of the two kernels (``lof_lrd_kernel``, ``lof_scores_kernel``) come from one
profiled call (torch.profiler's kernel records), with the bytes each gathers from its table (N sum(ks) 8) over that time.

Outside baseline: ``sklearn.neighbors.LocalOutlierFactor(n_neighbors=20, algorithm='brute')`` on the first ``--sklearn_n`` points fed as f64 on this host's
CPUs (0: skip; skipped when sklearn is not installed) beside this package on the same points, and the largest difference of the two over the largest value.

    python scripts/lof_bench.py [--n 75000] [--reps 3] [--sklearn_n 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.autograd import DeviceType
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from deep_interpolation_clustering_amd import knn  # noqa: E402
from deep_interpolation_clustering_amd import lof as LOF  # noqa: E402
from kmedoids_bench import best_of_windows, latents  # noqa: E402

KERNELS = ('lof_lrd_kernel', 'lof_scores_kernel')


def kernel_ms(fn):
    """{kernel: device ms, summed over its launches} of one call of ``fn``."""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        for k in KERNELS:
            if k in e.name:
                out[k] = out.get(k, 0.0) + float(getattr(e, 'device_time_total', 0.0) or 0.0) / 1e3
    return out


def configuration(x, ks, reps):
    n = x.shape[0]
    kmax = ks[-1]
    rec = {'ks': ks}
    rec['join_ms'] = 1e3 * best_of_windows(lambda: knn.kneighbors(x, kmax + 1, return_device=True), reps)
    raw = knn.kneighbors(x, kmax + 1, return_device=True)
    rec['drop_self_ms'] = 1e3 * best_of_windows(lambda: LOF.drop_self(*raw), reps)
    dist, idx = LOF.drop_self(*raw)
    rec['from_lists_ms'] = 1e3 * best_of_windows(lambda: LOF.lof_from_lists(dist, idx, ks), reps)
    km = kernel_ms(lambda: LOF.lof_from_lists(dist, idx, ks))
    rec['lrd_kernel_ms'], rec['scores_kernel_ms'] = km.get('lof_lrd_kernel'), km.get('lof_scores_kernel')
    rec['gathered_table_bytes'] = n * sum(ks) * 8
    for name in ('lrd', 'scores'):
        ms = rec[name + '_kernel_ms']
        rec[name + '_gather_gb_per_s'] = rec['gathered_table_bytes'] / (ms * 1e-3) / 1e9 if ms else None
    rec['lof_sweep_ms'] = 1e3 * best_of_windows(lambda: LOF.lof_sweep(x, ks, return_device=True), reps)
    rec['after_join_ms'] = rec['drop_self_ms'] + rec['from_lists_ms']
    rec['after_join_over_join'] = rec['after_join_ms'] / rec['join_ms']
    nof = LOF.lof_sweep(x, ks)
    rec['n_outliers_auto'] = [int((row < -1.5).sum()) for row in nof]
    rec['max_lof'] = [float((-row).max()) for row in nof]
    print('ks=%s: join %.2f ms; drop_self %.2f ms; lof_from_lists %.2f ms (lrd kernel %s ms, scores kernel %s ms); lof_sweep %.2f ms; after the join / join = '
          '%.3f' % (ks, rec['join_ms'], rec['drop_self_ms'], rec['from_lists_ms'], rec['lrd_kernel_ms'], rec['scores_kernel_ms'], rec['lof_sweep_ms'],
                    rec['after_join_over_join']), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sklearn_n', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lof_bench.json'))
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    LOF.lof_sweep(x[:2048], [5, 20])          # warm-up: code objects, the allocator
    out = {'metric': 'lof', 'n': n, 'd': d, 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    out['k20'] = configuration(x, [20], a.reps)
    out['sweep'] = configuration(x, list(range(10, 51, 5)), a.reps)
    sweep, alone = LOF.lof_sweep(x, list(range(10, 51, 5))), LOF.lof_sweep(x, [20])
    out['sweep_column_bit_equal_to_k20'] = bool(np.array_equal(sweep[2], alone[0]))

    def save():
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    save()          # (the CPU baseline below takes a while: the device figures are on disk before it starts)

    if a.sklearn_n:
        try:
            from sklearn.neighbors import LocalOutlierFactor
            m = min(a.sklearn_n, n)
            t = time.perf_counter()
            ref = LocalOutlierFactor(n_neighbors=20, algorithm='brute').fit(X[:m].astype(np.float64)).negative_outlier_factor_
            sk_s = time.perf_counter() - t
            LOF.lof_sweep(x[:m], [20])
            torch.cuda.synchronize()
            t = time.perf_counter()
            ours = LOF.lof_sweep(x[:m], [20])[0]
            torch.cuda.synchronize()
            ours_s = time.perf_counter() - t
            diff = float(np.abs(ours - ref).max() / np.abs(ref).max())
            out['sklearn'] = {'n': m, 'k': 20, 'seconds': sk_s, 'cpus': len(os.sched_getaffinity(0))}
            out['same_subset'] = {'n': m, 'k': 20, 'seconds': ours_s, 'largest_difference_over_largest_value': diff}
            print('sklearn LocalOutlierFactor(brute, f64) on %d points, k = 20 (%d threads allowed): %.2f s; this package on the same points: %.4f s; largest '
                  'difference %.3e of the largest value' % (m, out['sklearn']['cpus'], sk_s, ours_s, diff), flush=True)
        except ImportError:
            out['sklearn'] = None
    save()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
