"""Full- and tied-covariance Gaussian mixtures (gmm_full.py) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/gmm_bench.py's recipe), K = 2..10, one and ten restarts.  Per (K, restarts), from an M-step of fixed random hard labels: ``--iters`` whole EM
iterations enqueued back to back with a tolerance of 0, and separately the calls that isolate a kernel family -- the E-step of one restart
(dic_gmm_full_estep: gf_pass_kernel alone), the factor of restarts x K matrices (dic_gmm_full_factor: gf_factor_kernel alone), and the M-step from given
responsibilities (dic_gmm_full_mstep: the scatter, reduce and factor kernels; minus the factor's time it is the scatter SIDE: gf_scatter_kernel with
gf_resp_kernel, gf_params_kernel and gf_cov_kernel; the scatter kernel alone is timed by the kernel trace below) -- each timed by a host clock
around a device synchronise after a warm-up, best of ``--repeats`` windows.  Next to each time stands the dense matrix-core time of its flops at the f64 MFMA
peak DESIGN.md uses (78.6 TFLOP/s): the E-step and the scatter are each N K D^2 flops per restart after the triangular / symmetric halving (2 N K D^2 / 2),
the factor about (2/3) D^3 per matrix (Cholesky D^3 / 3, inverse D^3 / 3).  (The tied E-step is set against N D^2, the flops of x' P once; the kernel
forms (x' - mu'_k) P per component as the definition says, N K D^2.)  Per-kernel times inside an EM iteration come from running this script under
``rocprofv3 --kernel-trace --stats``.  Then a whole ``FullGaussianMixture(4).fit`` of both types, and once sklearn's 'full' fit on the CPU from the same
initial parameters (``--sklearn``).  One JSON line at the end.

    python scripts/gmm_full_bench.py [--n 75000] [--iters 10] [--repeats 3] [--ks 2 .. 10] [--sklearn]
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
from deep_interpolation_clustering_amd import gmm_full as GF  # noqa: E402
from deep_interpolation_clustering_amd.gmm import _Points  # noqa: E402
from gmm_bench import latents  # noqa: E402

F64_FLOPS = 78.6e12


def timed(fn, repeats):
    fn()          # warm-up of this shape: code objects, the LDS attribute, the allocator
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return min(out), (max(out) - min(out)) / min(out)


def em_window(pts, cov, par0, runs, iters, ws):
    """``iters`` EM iterations of every restart, enqueued back to back (tol = 0: none stops early)."""
    par = {k: (v.clone() if k != 'total' else v) for k, v in par0.items()}
    status = GF.new_status(runs, 0.0, 10 ** 9, pts.x.device)          # (the windows of one shape share it: none may reach max_iter)
    lbs = torch.empty((runs, iters + 1), dtype=torch.float64, device=pts.x.device)
    K, st, L = par['w'].shape[1], N.stream_of(pts.x), N.lib()

    def run():
        for _ in range(iters):
            N.check(L.dic_gmm_full_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, runs, cov, 1e-6, N.ptr(pts.shift), N.ptr(par['w']),
                                           N.ptr(par['mu']), N.ptr(par['cov']), N.ptr(par['P']), N.ptr(par['log_det']), N.ptr(par.get('total')), N.ptr(status),
                                           N.ptr(lbs), iters + 1, N.ptr(ws), ws.numel(), st), 'dic_gmm_full_em_iter')
    return run, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ks', type=int, nargs='+', default=list(range(2, 11)))
    ap.add_argument('--restarts', type=int, nargs='+', default=[1, 10])
    ap.add_argument('--types', nargs='+', default=['full', 'tied'])
    ap.add_argument('--fit_k', type=int, default=4, help='K of the whole fits (0: none)')
    ap.add_argument('--sklearn', action='store_true', help="sklearn's 'full' fit of --fit_k on the CPU from the same initial parameters, once")
    a = ap.parse_args()
    X = latents(a.n)
    pts = _Points(torch.as_tensor(X, device='cuda'))
    n, d = pts.n, pts.d
    rng = np.random.default_rng(1)
    rows = []
    for name in a.types:
        cov = GF.COV_TYPES[name]
        for runs in a.restarts:
            for K in a.ks:
                Kc = K if cov == 2 else 1
                ws = GF._workspace(pts, K, runs, cov)
                labels = torch.as_tensor(rng.integers(0, K, (runs, n)).astype(np.int32), device='cuda')
                par = GF.mstep(pts, K, cov, 1e-6, labels=labels, ws=ws)
                run, status = em_window(pts, cov, par, runs, a.iters, ws)
                t_em, spread = timed(run, a.repeats)
                assert bool((status[:, 7] == 0).all())
                t_em /= a.iters
                t_e, _ = timed(lambda: GF.estep(pts, cov, par['w'][0], par['mu'][0], par['P'][0], par['log_det'][0], total=True, ws=ws), a.repeats)
                t_f, _ = timed(lambda: GF.factor(par['cov'], pts.d0), a.repeats)
                resp = torch.rand((runs, n, K), dtype=torch.float64, device='cuda')
                resp /= resp.sum(dim=2, keepdim=True)
                t_m, _ = timed(lambda: GF.mstep(pts, K, cov, 1e-6, resp=resp, total=par.get('total'), compute_total=False, ws=ws), a.repeats)
                dense_e = n * Kc * d * d / F64_FLOPS          # one restart
                dense_s = n * K * d * d * runs / F64_FLOPS if cov == 2 else 0.0
                dense_f = 2.0 / 3.0 * d ** 3 * runs * Kc / F64_FLOPS
                row = {'type': name, 'K': K, 'restarts': runs, 'em_iter_ms': 1e3 * t_em, 'em_spread': spread, 'em_dense_ms': 1e3 * (dense_e * runs + dense_s + dense_f),
                       'estep_one_restart_ms': 1e3 * t_e, 'estep_dense_ms': 1e3 * dense_e, 'factor_ms': 1e3 * t_f, 'factor_dense_ms': 1e3 * dense_f,
                       'mstep_from_resp_ms': 1e3 * t_m, 'scatter_side_ms': 1e3 * (t_m - t_f), 'scatter_dense_ms': 1e3 * dense_s}
                rows.append(row)
                print('%s K = %2d, %2d restart(s): EM iteration %8.2f ms (dense %6.2f: x %5.1f; spread %.1f %%) | E-step of one restart %7.2f ms (dense %5.2f: x %5.1f) | '
                      'factor of %3d matrices %6.2f ms (dense %.3f) | M-step from responsibilities %7.2f ms, without the factor %7.2f (scatter dense %5.2f%s)'
                      % (name, K, runs, row['em_iter_ms'], row['em_dense_ms'], row['em_iter_ms'] / row['em_dense_ms'], 100 * spread, row['estep_one_restart_ms'],
                         row['estep_dense_ms'], t_e / dense_e, runs * Kc, row['factor_ms'], row['factor_dense_ms'], row['mstep_from_resp_ms'], row['scatter_side_ms'],
                         row['scatter_dense_ms'], ': x %.1f' % ((t_m - t_f) / dense_s) if dense_s else ''), flush=True)
                del ws, par, resp
    fits, sk = [], []
    for name in a.types if a.fit_k else []:
        for runs in a.restarts:
            GF.FullGaussianMixture(a.fit_k, covariance_type=name, n_init=runs, random_state=0).fit(pts.x[:4096])          # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = GF.FullGaussianMixture(a.fit_k, covariance_type=name, n_init=runs, random_state=0)._fit_points(pts)
            torch.cuda.synchronize()
            fits.append({'type': name, 'K': a.fit_k, 'restarts': runs, 'fit_s': time.perf_counter() - t, 'n_iter': m.n_iter_, 'lower_bound': m.lower_bound_})
            print('FullGaussianMixture(%d, %s, n_init=%d).fit with k-means initialisation: %.3f s (%d iterations of the winner, lower bound %.4f)'
                  % (a.fit_k, name, runs, fits[-1]['fit_s'], m.n_iter_, m.lower_bound_), flush=True)
    if a.sklearn and a.fit_k:
        from sklearn.mixture import GaussianMixture as SkGaussianMixture
        K = a.fit_k
        labels = rng.integers(0, K, (1, n)).astype(np.int32)
        ours = GF.FullGaussianMixture(K, covariance_type='full')
        torch.cuda.synchronize()
        t = time.perf_counter()
        ours._fit_points(pts, init_labels=labels)
        torch.cuda.synchronize()
        t_ours = time.perf_counter() - t
        X64 = X.astype(np.float64)
        r = np.zeros((n, K))
        r[np.arange(n), labels[0]] = 1.0
        nk = r.sum(axis=0)
        mu = r.T @ X64 / nk[:, None]
        C = np.stack([((X64 - mu[k]) * r[:, k:k + 1]).T @ (X64 - mu[k]) / nk[k] + 1e-6 * np.eye(d) for k in range(K)])
        t = time.perf_counter()
        ref = SkGaussianMixture(K, covariance_type='full', weights_init=nk / n, means_init=mu, precisions_init=np.linalg.inv(C)).fit(X64)
        t_sk = time.perf_counter() - t
        sk.append({'K': K, 'ours_s': t_ours, 'ours_n_iter': ours.n_iter_, 'sklearn_s': t_sk, 'sklearn_n_iter': int(ref.n_iter_), 'ours_lower_bound': ours.lower_bound_,
                   'sklearn_lower_bound': float(ref.lower_bound_), 'cpus': len(os.sched_getaffinity(0))})
        print("from the same initial parameters, K = %d, 'full': this fit %.3f s (%d iterations, lower bound %.6f); sklearn on the CPU (%d threads allowed) %.2f s "
              '(%d iterations, lower bound %.6f)' % (K, t_ours, ours.n_iter_, ours.lower_bound_, sk[-1]['cpus'], t_sk, ref.n_iter_, ref.lower_bound_), flush=True)
    print(json.dumps({'metric': 'gmm_full_em', 'n': n, 'd': d, 'iters': a.iters, 'f64_matrix_flops': F64_FLOPS, 'em': rows, 'fit': fits, 'sklearn': sk}))


if __name__ == '__main__':
    main()
