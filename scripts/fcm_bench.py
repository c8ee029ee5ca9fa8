"""Fuzzy c-means of p2 / p4 (--cluster_method fcm) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/gmm_bench.py's
recipe), K = 2..10, one and ten restarts, at m = 2 (the short cut: no exp / log) and m = 1.2.  Per (m, K, restarts): the initial centres are fixed random rows
(no seeding time in the figure), then ``--iters`` iterations are enqueued back to back with a tolerance of 0 and a max_iter beyond them (nothing stops early)
and timed by a host clock around a device synchronise, after a warm-up of the same shape; the best of ``--repeats`` windows and their spread are kept.
IN THE SAME RUN, on the same points, the diagonal Gaussian mixture's EM iteration (``dic_gmm_em_iter``, gmm_bench's window) is timed for every (K, restarts),
and the ratio fcm / gmm is printed: the first phase has the same arithmetic (K D differences and products per row), the accumulation phase half of it (no
second moment).  Then whole ``FuzzyCMeans(K).fit`` calls with k-means++ initialisation.  One JSON line at the end.

    python scripts/fcm_bench.py [--n 75000] [--iters 50] [--repeats 3] [--fit_ks 4 10]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import fcm as F  # noqa: E402
from deep_interpolation_clustering_amd import gmm as G  # noqa: E402
from gmm_bench import em_window, latents  # noqa: E402


def fcm_window(pts, K, runs, m, iters, ws, rows):
    """Seconds of ``iters`` iterations of ``runs`` restarts, enqueued back to back (tol = 0: none stops early), from the centres ``rows`` (runs, K) index."""
    L = N.lib()
    centers = F.shifted_centers(pts, pts.x[rows][:, :, :pts.d0])
    status = torch.zeros((runs, 8), dtype=torch.float64, device=pts.x.device)
    status[:, 3] = -float('inf')
    status[:, 4] = -1.0          # (|dJ| <= tol J is never true)
    status[:, 5] = float(iters + 1)
    objs = torch.empty((runs, iters + 1), dtype=torch.float64, device=pts.x.device)
    st = N.stream_of(pts.x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        N.check(L.dic_fcm_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, K, runs, float(m), N.ptr(pts.shift), N.ptr(centers), N.ptr(status), N.ptr(objs),
                               iters + 1, N.ptr(ws), ws.numel(), st), 'dic_fcm_iter')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert int(status[0, 1]) == iters and bool(torch.isfinite(objs[:, :iters]).all())
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ks', type=int, nargs='+', default=list(range(2, 11)))
    ap.add_argument('--ms', type=float, nargs='+', default=[2.0, 1.2])
    ap.add_argument('--fit_ks', type=int, nargs='*', default=[4, 10], help='Ks of the whole fits')
    a = ap.parse_args()
    X = latents(a.n)
    pts = G._Points(torch.as_tensor(X, device='cuda'))
    n, d = pts.n, pts.d
    rng = np.random.default_rng(1)
    rows = []
    for runs in (1, 10):
        for K in a.ks:
            gws = G._workspace(pts, K, runs)
            labels = torch.as_tensor(rng.integers(0, K, (runs, n)).astype(np.int32), device='cuda')
            em_window(pts, K, runs, 5, gws, labels)          # warm-up of this shape
            gmm = min(em_window(pts, K, runs, a.iters, gws, labels) for _ in range(a.repeats)) / a.iters
            ws = F._workspace(pts, K, runs)
            start = torch.as_tensor(np.stack([rng.choice(n, K, replace=False) for _ in range(runs)]), device='cuda')
            for m in a.ms:
                fcm_window(pts, K, runs, m, 5, ws, start)
                times = [fcm_window(pts, K, runs, m, a.iters, ws, start) for _ in range(a.repeats)]
                per_iter = min(times) / a.iters
                rows.append({'m': m, 'K': K, 'restarts': runs, 'us_per_iter': 1e6 * per_iter, 'us_per_iter_per_restart': 1e6 * per_iter / runs,
                             'spread': (max(times) - min(times)) / min(times), 'gmm_us_per_iter': 1e6 * gmm, 'ratio_to_gmm': per_iter / gmm})
                print('m = %-4g K = %2d, %2d restart(s): %8.1f us per iteration (%7.1f per restart; spread of %d windows %.1f %%); gmm_em_iter %8.1f us: x %.2f'
                      % (m, K, runs, 1e6 * per_iter, 1e6 * per_iter / runs, a.repeats, 100 * rows[-1]['spread'], 1e6 * gmm, per_iter / gmm), flush=True)
    fits = []
    for m in a.ms:
        for K in a.fit_ks:
            for runs in (1, 10):
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')          # (a collapsed fit is a figure of the table here)
                    F.FuzzyCMeans(K, m=m, n_init=runs, random_state=0).fit(pts.x[:4096])          # warm-up
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fit = F.FuzzyCMeans(K, m=m, n_init=runs, random_state=0)._fit_points(pts)
                    torch.cuda.synchronize()
                fits.append({'m': m, 'K': K, 'restarts': runs, 'fit_s': time.perf_counter() - t, 'n_iter': fit.n_iter_, 'converged': fit.converged_,
                             'objective': fit.objective_, 'partition_coefficient': fit.partition_coefficient_, 'n_coincident': len(fit.coincident_centers_)})
                print('FuzzyCMeans(%d, m=%g, n_init=%d).fit with k-means++ initialisation: %.3f s (%d iterations of the winner, PC %.4f, %d coincident pairs)'
                      % (K, m, runs, fits[-1]['fit_s'], fit.n_iter_, fit.partition_coefficient_, len(fit.coincident_centers_)), flush=True)
    print(json.dumps({'metric': 'fcm_iter', 'n': n, 'd': d, 'iters': a.iters, 'iter': rows, 'fit': fits}))


if __name__ == '__main__':
    main()
