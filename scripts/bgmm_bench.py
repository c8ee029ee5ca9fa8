"""Bayesian Gaussian mixtures of p2 / p4 (--cluster_method bgmm) at full size on one MI355X, beside the plain mixture's EM on the same points in the same
run: 75 000 x 256 synthetic latents shaped like p1's output (scripts/gmm_bench.py's recipe), diagonal covariances, K = 10 and 20, one and ten restarts.  Per
(K, restarts) both mixtures start from the M-step of the same fixed random hard labels (no k-means time in the figure); ``--iters`` iterations are enqueued
back to back with a tolerance of 0 (nothing stops early) and timed by a host clock around a device synchronise, after a warm-up of the same shape; the best
of ``--repeats`` windows and their spread are kept.  Then a whole ``BayesianGaussianMixture(K).fit`` against sklearn's on the CPU FROM THE SAME INITIAL
LABELS (``--sk_ks``; one-hot responsibilities through sklearn's ``_initialize``), where sklearn is importable.  One JSON line at the end.

    python scripts/bgmm_bench.py [--n 75000] [--iters 50] [--repeats 3] [--ks 10 20] [--sk_ks 10]
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
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import bgmm as B  # noqa: E402
from deep_interpolation_clustering_amd import gmm as G  # noqa: E402
from gmm_bench import em_window as gmm_window, latents  # noqa: E402


def bgmm_window(pts, K, runs, iters, ws, labels, pri):
    """Seconds of ``iters`` iterations of ``runs`` restarts of the Bayesian mixture, enqueued back to back, from the M-step of ``labels``."""
    L = N.lib()
    mu, var, comp = B.init(pts, K, pri, 1e-6, labels=labels, ws=ws)
    status = torch.zeros((runs, 8), dtype=torch.float64, device=pts.x.device)
    status[:, 3] = -float('inf')
    status[:, 5] = float(iters + 1)
    lbs = torch.empty((runs, iters + 1), dtype=torch.float64, device=pts.x.device)
    st = N.stream_of(pts.x)
    scalars = pri.scalars(1e-6)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        N.check(L.dic_bgmm_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, runs, *scalars, N.ptr(pts.shift), N.ptr(pri.m0), N.ptr(pri.s0),
                                   N.ptr(mu), N.ptr(var), N.ptr(comp), N.ptr(status), N.ptr(lbs), iters + 1, N.ptr(ws), ws.numel(), st), 'dic_bgmm_em_iter')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert int(status[0, 1]) == iters and bool(torch.isfinite(lbs[:, :iters]).all())
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ks', type=int, nargs='+', default=[10, 20])
    ap.add_argument('--sk_ks', type=int, nargs='*', default=[10], help='Ks of the whole-fit comparison with sklearn on the CPU (none: skip)')
    a = ap.parse_args()
    X = latents(a.n)
    pts = G._Points(torch.as_tensor(X, device='cuda'))
    n, d = pts.n, pts.d
    rng = np.random.default_rng(1)
    rows = []
    for runs in (1, 10):
        for K in a.ks:
            pri = B.BayesianGaussianMixture(K)._priors(pts)
            ws_b, ws_g = B._workspace(pts, K, runs), G._workspace(pts, K, runs)
            labels = torch.as_tensor(rng.integers(0, K, (runs, n)).astype(np.int32), device='cuda')
            bgmm_window(pts, K, runs, 5, ws_b, labels, pri)          # warm-ups of this shape: code objects, the LDS attribute, the allocator
            gmm_window(pts, K, runs, 5, ws_g, labels)
            tb = [bgmm_window(pts, K, runs, a.iters, ws_b, labels, pri) for _ in range(a.repeats)]
            tg = [gmm_window(pts, K, runs, a.iters, ws_g, labels) for _ in range(a.repeats)]
            rows.append({'K': K, 'restarts': runs, 'bgmm_ms_per_iter': 1e3 * min(tb) / a.iters, 'gmm_ms_per_iter': 1e3 * min(tg) / a.iters,
                         'bgmm_spread': (max(tb) - min(tb)) / min(tb), 'gmm_spread': (max(tg) - min(tg)) / min(tg), 'ratio': min(tb) / min(tg)})
            print('K = %2d, %2d restart(s): bgmm %7.3f ms per iteration (spread of %d windows %.1f %%), gmm %7.3f ms (%.1f %%): x %.3f'
                  % (K, runs, rows[-1]['bgmm_ms_per_iter'], a.repeats, 100 * rows[-1]['bgmm_spread'], rows[-1]['gmm_ms_per_iter'], 100 * rows[-1]['gmm_spread'],
                     rows[-1]['ratio']), flush=True)
    fits, sk = [], []
    for K in a.sk_ks:
        labels0 = rng.integers(0, K, n)
        model = B.BayesianGaussianMixture(K)
        model._fit_points(G._Points(pts.x[:4096]), init_labels=labels0[None, :4096])          # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = B.BayesianGaussianMixture(K)._fit_points(pts, init_labels=labels0[None])
        torch.cuda.synchronize()
        fits.append({'K': K, 'fit_s': time.perf_counter() - t, 'n_iter': m.n_iter_, 'lower_bound': m.lower_bound_, 'n_active': len(m.active_components_)})
        print('BayesianGaussianMixture(%d).fit from given labels: %.3f s (%d iterations, lower bound %.4f, %d active components)'
              % (K, fits[-1]['fit_s'], m.n_iter_, m.lower_bound_, fits[-1]['n_active']), flush=True)
        try:
            from sklearn.mixture import BayesianGaussianMixture as SkBayesianGaussianMixture
        except ImportError:
            print('sklearn is not importable: no CPU comparison')
            continue
        resp = np.zeros((n, K))
        resp[np.arange(n), labels0] = 1.0

        class FromLabels(SkBayesianGaussianMixture):
            def _initialize_parameters(self, X, random_state):
                self._initialize(X, resp)

        X64 = X.astype(np.float64)
        t = time.perf_counter()
        ref = FromLabels(n_components=K, covariance_type='diag').fit(X64)
        sk.append({'K': K, 'fit_s': time.perf_counter() - t, 'n_iter': int(ref.n_iter_), 'lower_bound': float(ref.lower_bound_),
                   'cpus': len(os.sched_getaffinity(0))})
        print('sklearn BayesianGaussianMixture(%d, diag).fit from the same labels on the CPU (%d threads allowed): %.2f s (%d iterations, lower bound %.4f)'
              % (K, sk[-1]['cpus'], sk[-1]['fit_s'], ref.n_iter_, ref.lower_bound_), flush=True)
    print(json.dumps({'metric': 'bgmm_em', 'n': n, 'd': d, 'iters': a.iters, 'em': rows, 'fit': fits, 'sklearn': sk}))


if __name__ == '__main__':
    main()
