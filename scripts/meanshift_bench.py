"""Mean shift of p2 / p4 (--cluster_method meanshift) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/ward_bench.py's recipe), the bandwidth ``estimate_bandwidth(X, 0.3)``, every point a seed.  The estimator's own loop is walked by hand so that the
two kernels of an iteration can be timed apart: per iteration the active seeds, the members pass (seed planes, tile pass, band recheck; it ends with the host
read of the band count, so its time is a host clock around the call) and the shift kernel (a host clock around a device synchronise), summed over the seed
groups the mask budget makes.  The members pass is set against one counting pass of ``kth_neighbor_distance`` over the same rectangle (a quarter of its
63 ms at 75 000 seeds), the shift kernel against the f64 matrix-core time of the 0/1 product (2 M N D flops at 78.6 TFLOP/s) -- which the kernel undercuts
where whole 4-point steps have no member.  Then the whole ``MeanShift(bandwidth).fit``, and sklearn's fit of a ``--sk_n`` subsample on the CPU where sklearn
is importable, for scale.  One JSON line at the end.

    python scripts/meanshift_bench.py [--n 75000] [--quantile 0.3] [--shifts 0] [--sk_n 4000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_interpolation_clustering_amd import meanshift as M  # noqa: E402

F64_MFMA_FLOPS = 78.6e12


def latents(n, seed=0):
    rng = np.random.default_rng(seed)
    k = 12
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(int(n * 0.92), np.full(k, 1 / k))
    widths = rng.uniform(0.04, 0.12, k)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)]
                       + [rng.normal(0, 0.45, (n - int(sizes.sum()), 256))])
    return rng.permutation(X).astype(np.float32)


def walk(pts, h, max_iter, mask_budget, max_shifts):
    """``MeanShift._run_seeds`` with a clock around either kernel: a list of {active, groups, members_s, shift_s, band_pairs} per iteration."""
    dev = pts.x.device
    s = pts.x.double().contiguous()
    m_all = s.shape[0]
    group = max(256, mask_budget // (4 * pts.words) // 256 * 256)
    m_max = min(m_all, group)
    ws = pts.workspace(m_max, 4 * m_max * pts.words + 3 * 8 * m_all * pts.d)
    mask = torch.empty((m_max, pts.words), dtype=torch.int32, device=dev)
    cnt, it, dn = (torch.zeros(m_all, dtype=torch.int32, device=dev) for _ in range(3))
    band = None
    rows = []
    while s.shape[0] and (not max_shifts or len(rows) < max_shifts):
        m = s.shape[0]
        row = {'active': m, 'groups': -(-m // m_max), 'members_s': 0.0, 'shift_s': 0.0, 'band_pairs': 0}
        for g0 in range(0, m, m_max):
            g1 = min(m, g0 + m_max)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            band = M.members(pts, s[g0:g1], h, mask, m_max, ws, band, row)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            M.shift(pts, mask, s[g0:g1], h, max_iter, cnt[g0:g1], it[g0:g1], dn[g0:g1])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            row['members_s'] += t1 - t0
            row['shift_s'] += t2 - t1
        row['mean_members'] = float(cnt.double().mean())
        rows.append(row)
        keep = dn == 0
        s, cnt, it, dn = s[keep].contiguous(), cnt[keep].contiguous(), it[keep].contiguous(), dn[keep].contiguous()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--quantile', type=float, default=0.3)
    ap.add_argument('--shifts', type=int, default=0, help='iterations of the timed walk (0: until every seed is done)')
    ap.add_argument('--mask_budget', type=int, default=M.DEFAULT_MASK_BUDGET)
    ap.add_argument('--sk_n', type=int, default=4000, help='points of the sklearn comparison on the CPU (0: skip)')
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    torch.cuda.synchronize()
    t = time.perf_counter()
    h = M.estimate_bandwidth(x, a.quantile)
    bw_s = time.perf_counter() - t
    print('estimate_bandwidth(X, %.2f) = %.6g: %.3f s' % (a.quantile, h, bw_s), flush=True)
    M.MeanShift(bandwidth=h).fit(x[:2048])          # warm-up: code objects, the LDS attribute, the allocator
    pts = M._Points(x)
    n, d = pts.n, pts.d
    rows = walk(pts, h, 300, a.mask_budget, a.shifts)
    for i, r in enumerate(rows):
        floor = 2.0 * r['active'] * n * d / F64_MFMA_FLOPS
        print('iteration %3d: %6d active seeds in %d group(s), %8.1f members per seed; members pass %8.2f ms (%d band pairs), shift %8.2f ms (dense f64 '
              'matrix-core time %7.2f ms)' % (i, r['active'], r['groups'], r['mean_members'], 1e3 * r['members_s'], r['band_pairs'], 1e3 * r['shift_s'],
                                              1e3 * floor), flush=True)
    print('walk: %d iterations, members %.3f s, shift %.3f s' % (len(rows), sum(r['members_s'] for r in rows), sum(r['shift_s'] for r in rows)), flush=True)
    fit = None
    if not a.shifts:
        torch.cuda.synchronize()
        t = time.perf_counter()
        ms = M.MeanShift(bandwidth=h, mask_budget=a.mask_budget)._fit_points(M._Points(x))
        torch.cuda.synchronize()
        fit = {'fit_s': time.perf_counter() - t, 'n_clusters': len(ms.cluster_centers_), 'n_iter': ms.n_iter_, 'shifts': ms.stats_['shifts']}
        print('MeanShift(bandwidth=%.6g).fit: %.3f s (%d centres, n_iter %d, %d shifts enqueued)' % (h, fit['fit_s'], fit['n_clusters'], fit['n_iter'],
                                                                                                   fit['shifts']), flush=True)
    sk = None
    if a.sk_n:
        try:
            from sklearn.cluster import MeanShift as SkMeanShift
            sub = X[:a.sk_n].astype(np.float64)
            t = time.perf_counter()
            ref = SkMeanShift(bandwidth=h).fit(sub)
            sk = {'n': len(sub), 'fit_s': time.perf_counter() - t, 'n_clusters': len(ref.cluster_centers_), 'n_iter': int(ref.n_iter_),
                  'cpus': len(os.sched_getaffinity(0))}
            print('sklearn MeanShift(bandwidth=%.6g).fit of %d points on the CPU (%d threads allowed, n_jobs=None): %.2f s (%d centres, n_iter %d)'
                  % (h, sk['n'], sk['cpus'], sk['fit_s'], sk['n_clusters'], sk['n_iter']), flush=True)
        except ImportError:
            print('sklearn is not importable: no CPU comparison')
    print(json.dumps({'metric': 'meanshift', 'n': n, 'd': d, 'quantile': a.quantile, 'bandwidth': h, 'estimate_bandwidth_s': bw_s, 'walk': rows, 'fit': fit,
                      'sklearn': sk}))


if __name__ == '__main__':
    main()
