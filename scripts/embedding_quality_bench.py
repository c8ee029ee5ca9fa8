"""Trustworthiness, continuity and neighbours kept (embedding_quality.py) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/kmedoids_bench.py's recipe) and their exact t-SNE map at perplexity 30 (``--iters`` iterations).  Writes profiles/embedding_quality_bench.json and
prints it as one JSON line.

Host-clock figures (the best of 3 windows of ``--reps`` repetitions after a warm-up, a window ending in a device synchronise): per space (``x``: the latents,
``y``: the map rounded to f32) the ``kneighbors`` self join at max(ks) + 1 and the ``neighbor_ranks`` call on the targets the quality computation ranks (the
entries of the other space's lists that this space's lists lack, moved to the front of their rows); and the whole ``embedding_quality(ks)``.
Device times PER KERNEL come from one profiled call (torch.profiler's kernel records): every counting pass (``kr_count_kernel``, one launch per 8 targets),
the gather passes, the exact stage and the target kernel.  The yardstick of a counting pass is ``db_count_kernel`` of a DBSCAN counting call in the same run
at ``--eps`` (next to no band pairs), as scripts/dpeaks_bench.py has it: the ratio is reported.  Band pairs: per ranked target (mean) and the longest row's;
targets per row: mean and largest.

Outside baseline: ``sklearn.manifold.trustworthiness`` on the first ``--sklearn_n`` points on this host's CPUs (0: skip; skipped when sklearn is not
installed) beside this package on the same points and the same map rows.

    python scripts/embedding_quality_bench.py [--n 75000] [--ks 5 10 30] [--iters 1000] [--reps 3] [--eps 0.5] [--sklearn_n 20000]
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
from deep_interpolation_clustering_amd import embedding_quality as EQ  # noqa: E402
from deep_interpolation_clustering_amd import knn  # noqa: E402
from deep_interpolation_clustering_amd import tsne as T  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _Counts, sq_threshold  # noqa: E402
from kmedoids_bench import best_of_windows, latents  # noqa: E402

KERNELS = ('db_count_kernel', 'kr_target_kernel', 'kr_count_kernel', 'kr_gather_kernel', 'kr_exact_kernel', 'kn_count_kernel', 'kn_gather_kernel',
           'knl_exact_kernel')


def kernel_launches(fn):
    """{kernel: [device ms of every launch]} of one call of ``fn``."""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        for k in KERNELS:
            if k in e.name:
                out.setdefault(k, []).append(float(getattr(e, 'device_time_total', 0.0) or 0.0) / 1e3)
    return out


def front_targets(own, other):
    """The targets embedding_quality ranks in the space of ``own``: the entries of ``other`` it lacks, at the front of their rows, -1 behind them."""
    missing = ~(other[:, :, None] == own[:, None, :]).any(dim=2)
    m = max(1, int(missing.sum(dim=1).max()))
    order = torch.sort((~missing).to(torch.int8), dim=1, stable=True).indices[:, :m]
    front = torch.gather(missing, 1, order)
    return torch.where(front, torch.gather(other, 1, order), torch.full_like(order, -1, dtype=other.dtype)).to(torch.int32).contiguous(), missing


def space(name, z, own, other, reps, kmax, base_ms):
    rec = {}
    rec['join_ms'] = 1e3 * best_of_windows(lambda: knn.kneighbors(z, kmax + 1, return_device=True), reps)
    targets, missing = front_targets(own, other)
    per_row = missing.sum(dim=1)
    rec['targets'], rec['targets_per_row_mean'], rec['targets_per_row_max'] = int(per_row.sum()), float(per_row.float().mean()), int(per_row.max())
    st = {}
    knn.neighbor_ranks(z, targets, stats=st, return_device=True)
    rec['stats'] = st
    rec['band_pairs_per_target_mean'] = st['candidates'] / max(1, rec['targets'])
    rec['band_pairs_longest_row'] = st['max_list']
    rec['ranks_ms'] = 1e3 * best_of_windows(lambda: knn.neighbor_ranks(z, targets, return_device=True), reps)
    km = kernel_launches(lambda: knn.neighbor_ranks(z, targets, return_device=True))
    rec['count_pass_ms'] = km.get('kr_count_kernel', [])
    rec['gather_pass_ms'] = km.get('kr_gather_kernel', [])
    rec['exact_ms'] = sum(km.get('kr_exact_kernel', []))
    rec['target_kernel_ms'] = sum(km.get('kr_target_kernel', []))
    if base_ms and rec['count_pass_ms']:
        rec['count_pass_over_db_count_kernel'] = float(np.mean(rec['count_pass_ms'])) / base_ms
        rec['gather_pass_over_db_count_kernel'] = float(np.mean(rec['gather_pass_ms'])) / base_ms if rec['gather_pass_ms'] else None
    print('%s: join %.2f ms; %d targets (%.2f per row, at most %d) in %d passes; neighbor_ranks %.2f ms: counting passes %s ms, gather passes %s ms, exact '
          'stage %.3f ms; band pairs %.2f per target, longest row %d; counting pass / db_count_kernel = %s'
          % (name, rec['join_ms'], rec['targets'], rec['targets_per_row_mean'], rec['targets_per_row_max'], st['passes'], rec['ranks_ms'],
             [round(v, 3) for v in rec['count_pass_ms']], [round(v, 3) for v in rec['gather_pass_ms']], rec['exact_ms'], rec['band_pairs_per_target_mean'],
             rec['band_pairs_longest_row'], rec.get('count_pass_over_db_count_kernel')), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--ks', type=int, nargs='+', default=[5, 10, 30])
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--eps', type=float, default=0.5, help='eps of the DBSCAN counting pass that is the yardstick (next to no band pairs)')
    ap.add_argument('--sklearn_n', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'embedding_quality_bench.json'))
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    kmax = max(a.ks)
    warm = T.TSNE(perplexity=10.0, max_iter=250).fit(x[:2048])          # warm-up: code objects, the LDS attribute, the allocator
    warm.quality((5,))
    out = {'metric': 'embedding_quality', 'n': n, 'd': d, 'ks': sorted(a.ks), 'perplexity': a.perplexity, 'iters': a.iters, 'reps': a.reps,
           'device': torch.cuda.get_device_name(0)}

    torch.cuda.synchronize()
    t = time.perf_counter()
    fit = T.TSNE(perplexity=a.perplexity, max_iter=a.iters).fit(x)
    torch.cuda.synchronize()
    out['fit_s'], out['kl'] = time.perf_counter() - t, fit.kl_divergence_
    y = EQ._on_device(fit.embedding_)
    out['map_abs_max'] = float(np.abs(fit.embedding_).max())

    light = sq_threshold(a.eps)
    _Counts(x, [light])
    base = kernel_launches(lambda: _Counts(x, [light])).get('db_count_kernel')
    out['db_count_kernel_ms'] = float(np.mean(base)) if base else None
    out['db_count_band_pairs'] = _Counts(x, [light]).n_band

    lx, ly = EQ._own_lists(x, kmax), EQ._own_lists(y, kmax)
    out['x'] = space('x (75 000 x 256 latents)' if n == 75000 else 'x', x, lx, ly, a.reps, kmax, out['db_count_kernel_ms'])
    out['y'] = space('y (the map, f32)', y, ly, lx, a.reps, kmax, out['db_count_kernel_ms'])
    out['embedding_quality_ms'] = 1e3 * best_of_windows(lambda: EQ.embedding_quality(x, y, a.ks), a.reps)
    quality = EQ.embedding_quality(x, y, a.ks)
    out['quality'] = {str(k): list(v) for k, v in quality.items()}
    out['quality_from_fit'] = fit.quality(a.ks) == quality
    print('embedding_quality(ks=%s): %.2f ms; db_count_kernel %.3f ms; %s' % (sorted(a.ks), out['embedding_quality_ms'], out['db_count_kernel_ms'] or float('nan'),
                                                                             {k: tuple(round(v, 6) for v in q) for k, q in quality.items()}), flush=True)

    def save():
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    save()          # (the CPU baseline below takes minutes: the device figures are on disk before it starts)

    if a.sklearn_n:
        try:
            from sklearn.manifold import trustworthiness
            m = min(a.sklearn_n, n)
            sub, ysub = X[:m], fit.embedding_[:m]
            k = sorted(a.ks)[0]
            t = time.perf_counter()
            ref = float(trustworthiness(sub, ysub.astype(np.float32), n_neighbors=k))
            sk_s = time.perf_counter() - t
            EQ.trustworthiness(x[:m], ysub, k)
            torch.cuda.synchronize()
            t = time.perf_counter()
            ours = EQ.trustworthiness(x[:m], ysub, k)
            torch.cuda.synchronize()
            ours_s = time.perf_counter() - t
            out['sklearn_trustworthiness'] = {'n': m, 'k': k, 'seconds': sk_s, 'value': ref, 'cpus': len(os.sched_getaffinity(0))}
            out['same_subset'] = {'n': m, 'k': k, 'seconds': ours_s, 'value': ours}
            print('sklearn.manifold.trustworthiness on %d points, k = %d (%d threads allowed): %.2f s, %.12f; this package on the same points: %.4f s, %.12f'
                  % (m, k, out['sklearn_trustworthiness']['cpus'], sk_s, ref, ours_s, ours), flush=True)
        except ImportError:
            out['sklearn_trustworthiness'] = None
    save()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
