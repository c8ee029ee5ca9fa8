"""Gaussian mixtures of p2 / p4 (--cluster_method gmm) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/ward_bench.py's recipe), diagonal covariances, K = 2..10, one and ten restarts.  Per (K, restarts): the initialisation is an M-step from fixed random
hard labels (so that no k-means time is in the figure), then ``--iters`` EM iterations are enqueued back to back with a tolerance of 0 (nothing stops early)
and timed by a host clock around a device synchronise, after a warm-up of the same shape; the best of ``--repeats`` windows and their spread are kept.  The
per-iteration time is set against the floor of one read of X (N D 4 bytes) from HBM (8 TB/s) -- X, 77 MB, fits the 256 MB Infinity Cache, so the later
iterations of a fit can be served from there -- and against the f64 work the definition needs (7 N K D flops: 3 per coordinate and component in the E-step, 4
in the M-step) at the vector f64 peak of 78.6 TFLOP/s; the larger of the two floors is named.  Then a whole ``GaussianMixture(K).fit`` with k-means
initialisation, and sklearn's fit of the same K on the CPU where sklearn is importable (``--sk_ks``).  One JSON line at the end.

    python scripts/gmm_bench.py [--n 75000] [--iters 50] [--repeats 3] [--sk_ks 4 10]
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
from deep_interpolation_clustering_amd import gmm as G  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
F64_FLOPS = 78.6e12


def latents(n, seed=0):
    rng = np.random.default_rng(seed)
    k = 12
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(int(n * 0.92), np.full(k, 1 / k))
    widths = rng.uniform(0.04, 0.12, k)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)]
                       + [rng.normal(0, 0.45, (n - int(sizes.sum()), 256))])
    return rng.permutation(X).astype(np.float32)


def em_window(pts, K, runs, iters, ws, labels):
    """Seconds of ``iters`` EM iterations of ``runs`` restarts, enqueued back to back (tol = 0: none stops early), from the M-step of ``labels``."""
    L = N.lib()
    w, mu, var = G.mstep(pts, K, 0, 1e-6, labels=labels, ws=ws)
    status = torch.zeros((runs, 8), dtype=torch.float64, device=pts.x.device)
    status[:, 3] = -float('inf')
    status[:, 5] = float(iters + 1)
    lbs = torch.empty((runs, iters + 1), dtype=torch.float64, device=pts.x.device)
    st = N.stream_of(pts.x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        N.check(L.dic_gmm_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, runs, 0, 1e-6, N.ptr(pts.shift), N.ptr(w), N.ptr(mu), N.ptr(var),
                                  N.ptr(status), N.ptr(lbs), iters + 1, N.ptr(ws), ws.numel(), st), 'dic_gmm_em_iter')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert int(status[0, 1]) == iters and bool(torch.isfinite(lbs[:, :iters]).all())
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ks', type=int, nargs='+', default=list(range(2, 11)))
    ap.add_argument('--sk_ks', type=int, nargs='*', default=[4, 10], help='Ks of the sklearn comparison on the CPU (none: skip)')
    a = ap.parse_args()
    X = latents(a.n)
    pts = G._Points(torch.as_tensor(X, device='cuda'))
    n, d = pts.n, pts.d
    floor_bytes = n * d * 4 / HBM_BYTES_PER_S
    rng = np.random.default_rng(1)
    rows = []
    for runs in (1, 10):
        for K in a.ks:
            ws = G._workspace(pts, K, runs)
            labels = torch.as_tensor(rng.integers(0, K, (runs, n)).astype(np.int32), device='cuda')
            em_window(pts, K, runs, 5, ws, labels)          # warm-up of this shape: code objects, the LDS attribute, the allocator
            times = [em_window(pts, K, runs, a.iters, ws, labels) for _ in range(a.repeats)]
            per_iter = min(times) / a.iters
            floor_flops = 7.0 * n * K * d * runs / F64_FLOPS
            floor = max(floor_bytes * runs, floor_flops)
            rows.append({'K': K, 'restarts': runs, 'us_per_iter': 1e6 * per_iter, 'us_per_iter_per_restart': 1e6 * per_iter / runs,
                         'spread': (max(times) - min(times)) / min(times), 'floor_us': 1e6 * floor, 'floor': 'flops' if floor_flops > floor_bytes * runs else 'bytes',
                         'times_floor': per_iter / floor})
            print('K = %2d, %2d restart(s): %8.1f us per EM iteration (%7.1f per restart; spread of %d windows %.1f %%); floor %6.1f us (%s): x %.1f'
                  % (K, runs, 1e6 * per_iter, 1e6 * per_iter / runs, a.repeats, 100 * rows[-1]['spread'], 1e6 * floor, rows[-1]['floor'], per_iter / floor),
                  flush=True)
    fits = []
    for K in a.sk_ks or [4]:
        for runs in (1, 10):
            G.GaussianMixture(K, n_init=runs, random_state=0).fit(pts.x[:4096])          # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = G.GaussianMixture(K, n_init=runs, random_state=0)._fit_points(pts)
            torch.cuda.synchronize()
            fits.append({'K': K, 'restarts': runs, 'fit_s': time.perf_counter() - t, 'n_iter': m.n_iter_, 'lower_bound': m.lower_bound_})
            print('GaussianMixture(%d, n_init=%d).fit with k-means initialisation: %.3f s (%d iterations of the winner, lower bound %.4f)'
                  % (K, runs, fits[-1]['fit_s'], m.n_iter_, m.lower_bound_), flush=True)
    sk = []
    if a.sk_ks:
        try:
            from sklearn.mixture import GaussianMixture as SkGaussianMixture
            X64 = X.astype(np.float64)
            for K in a.sk_ks:
                t = time.perf_counter()
                ref = SkGaussianMixture(K, covariance_type='diag', n_init=1, random_state=0).fit(X64)
                sk.append({'K': K, 'restarts': 1, 'fit_s': time.perf_counter() - t, 'n_iter': int(ref.n_iter_), 'lower_bound': float(ref.lower_bound_),
                           'cpus': len(os.sched_getaffinity(0))})
                print('sklearn GaussianMixture(%d, diag, n_init=1).fit on the CPU (%d threads allowed): %.2f s (%d iterations, lower bound %.4f)'
                      % (K, sk[-1]['cpus'], sk[-1]['fit_s'], ref.n_iter_, ref.lower_bound_), flush=True)
        except ImportError:
            print('sklearn is not importable: no CPU comparison')
    print(json.dumps({'metric': 'gmm_em', 'n': n, 'd': d, 'iters': a.iters, 'em': rows, 'fit': fits, 'sklearn': sk}))


if __name__ == '__main__':
    main()
