"""``FullGaussianMixture``: Gaussian mixtures with full (scikit-learn's default) or tied covariances on the MI355X (csrc/dic_gmm_full.hip), beside ``gmm.py``'s
diagonal and spherical ones: the p2 / p4 ``--cluster_method gmm --gmm_covariance_type full | tied`` branches.

The latents are 256 strongly correlated outputs of an auto-encoder; a diagonal mixture spends components on describing correlation, a full one does not.  The
model, the estimator surface, the control flow and the shifted points are ``_gmm_base.py``'s, shared with ``gmm.py``; this file adds the native calls, the
Cholesky factors of its covariances and the total scatter matrix of the tied type.  The arithmetic is the f64 definition in include/dic_hip.h: the E-step
(x - mu_k) P_k and the weighted scatter matrices run on the f64 matrix cores, the Cholesky factors P_k = L_k^-T are computed on the device, and every sum has
a fixed order, so two fits give the same bits.

Outputs are NumPy f64, like sklearn's.  The module imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from ._gmm_base import _dev64, _MixtureBase, _Points, estep_outputs, new_status, run_em, workspace

COV_TYPES = {'full': 2, 'tied': 3}
_ILL_DEFINED = ('Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by singleton or collapsed '
                'samples). Try to decrease the number of components, increase reg_covar, or scale the input data.')
_NEEDS = ('-covariance Gaussian mixture of {n} points needs {nbytes} bytes on the device, {free} are free: log r (8 N K), the partial sums and the '
          'slab matrices of the scatter kernel (8 K D^2 each for full covariances; K = {k}, D = {d}), per restart ({runs})')


def _workspace(pts, K, n_runs, cov_type):
    return workspace(pts, K, n_runs, lambda *shape: N.lib().dic_gmm_full_workspace(*shape, cov_type), 'gmm_full',
                     'the ' + ('full' if cov_type == 2 else 'tied') + _NEEDS)


def factor(cov, d0):
    """covariances (n_runs, n_mats, D, D) f64 on the device -> (prec_chol (same shape, upper triangular), log_det (n_runs, n_mats), status (n_runs, 8): [7] is 1
    where a pivot was not a finite positive number)."""
    n_runs, n_mats, D, _ = cov.shape
    cov = cov.contiguous()
    P = torch.empty_like(cov)
    ld = torch.empty((n_runs, n_mats), dtype=torch.float64, device=cov.device)
    status = torch.zeros((n_runs, 8), dtype=torch.float64, device=cov.device)
    ws = torch.empty(max(16, cov.numel() * 8), dtype=torch.uint8, device=cov.device)
    N.check(N.lib().dic_gmm_full_factor(N.ptr(cov), n_runs, n_mats, D, d0, N.ptr(P), N.ptr(ld), N.ptr(status), N.ptr(ws), ws.numel(), N.stream_of(cov)),
            'dic_gmm_full_factor')
    return P, ld, status


def mstep(pts, K, cov_type, reg_covar, labels=None, resp=None, total=None, compute_total=True, status=None, ws=None):
    """The M-step of every restart, factor included, from hard labels ((n_runs, N) int32 on the device) or responsibilities ((n_runs, N, K) f64).  Returns a
    dict: w (n_runs, K), mu (n_runs, K, D), cov and P (n_runs, Kc, D, D), log_det (n_runs, Kc), total ((D, D): T, tied only), status."""
    src = labels if labels is not None else resp
    n_runs, dev, D = src.shape[0], pts.x.device, pts.d
    Kc = K if cov_type == 2 else 1
    out = {'w': torch.empty((n_runs, K), dtype=torch.float64, device=dev), 'mu': torch.empty((n_runs, K, D), dtype=torch.float64, device=dev),
           'cov': torch.empty((n_runs, Kc, D, D), dtype=torch.float64, device=dev), 'P': torch.empty((n_runs, Kc, D, D), dtype=torch.float64, device=dev),
           'log_det': torch.empty((n_runs, Kc), dtype=torch.float64, device=dev),
           'status': torch.zeros((n_runs, 8), dtype=torch.float64, device=dev) if status is None else status}
    if cov_type == 3:
        out['total'] = torch.empty((D, D), dtype=torch.float64, device=dev) if total is None else total
        compute_total = bool(compute_total) or total is None
    ws = _workspace(pts, K, n_runs, cov_type) if ws is None else ws
    N.check(N.lib().dic_gmm_full_mstep(N.ptr(pts.x), pts.x.stride(0), pts.n, D, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift), N.ptr(labels),
                                       N.ptr(resp), N.ptr(out.get('total')), int(bool(compute_total)), N.ptr(out['w']), N.ptr(out['mu']), N.ptr(out['cov']),
                                       N.ptr(out['P']), N.ptr(out['log_det']), N.ptr(out['status']), N.ptr(ws), ws.numel(), N.stream_of(pts.x)),
            'dic_gmm_full_mstep')
    return out


def em(pts, cov_type, reg_covar, par, status, max_iter, ws=None):
    """EM on every restart of ``par`` (the dict of ``mstep``, updated in place) until each is done.  Returns (status (n_runs, 8) numpy, lower bounds
    (n_runs, max_iter) numpy, NaN beyond a restart's iterations)."""
    L = N.lib()
    n_runs, K = par['w'].shape
    ws = _workspace(pts, K, n_runs, cov_type) if ws is None else ws
    st = N.stream_of(pts.x)

    def iterate(lbs):
        N.check(L.dic_gmm_full_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift),
                                       N.ptr(par['w']), N.ptr(par['mu']), N.ptr(par['cov']), N.ptr(par['P']), N.ptr(par['log_det']), N.ptr(par.get('total')),
                                       N.ptr(status), N.ptr(lbs), max_iter, N.ptr(ws), ws.numel(), st), 'dic_gmm_full_em_iter')
    return run_em(iterate, status, max_iter)


def estep(pts, cov_type, w, mu, P, log_det, lse=False, log_resp=False, labels=False, total=False, ws=None):
    """The E-step of one parameter set ((K), (K, D), (Kc, D, D), (Kc) f64 on the device): a dict of the requested outputs, as ``gmm.estep``."""
    K = w.shape[-1]
    out = estep_outputs(pts, K, lse, log_resp, labels, total)
    ws = _workspace(pts, K, 1, cov_type) if ws is None else ws
    N.check(N.lib().dic_gmm_full_estep(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, cov_type, N.ptr(pts.shift), N.ptr(w.contiguous()),
                                       N.ptr(mu.contiguous()), N.ptr(P.contiguous()), N.ptr(log_det.contiguous()), N.ptr(out.get('lse')),
                                       N.ptr(out.get('log_resp')), N.ptr(out.get('labels')), N.ptr(out.get('total')), N.ptr(ws), ws.numel(),
                                       N.stream_of(pts.x)), 'dic_gmm_full_estep')
    return out


def n_parameters(n_components, n_features, covariance_type):
    """Free parameters of the model (``_gaussian_mixture.py:881-893``), with the true feature count."""
    cov = n_features * (n_features + 1) // 2 * (n_components if covariance_type == 'full' else 1)
    return int(cov + n_features * n_components + n_components - 1)


def _host_factor(prec):
    """(P upper triangular with P P^T = prec, log det P) of one given precision matrix, on the host: the Cholesky factor of the precision with rows and
    columns reversed, reversed back -- the P = L^-T of the covariance without inverting anything."""
    P = np.linalg.cholesky(prec[::-1, ::-1])[::-1, ::-1]
    return np.triu(P), float(np.log(np.diag(P)).sum())


def _pad_square(a, D, device):
    """(.., D0, D0) numpy -> (.., D, D) on the device, the identity in the padding."""
    a = np.asarray(a, dtype=np.float64)
    d0 = a.shape[-1]
    out = np.zeros(a.shape[:-2] + (D, D))
    out[...] = np.eye(D)
    out[..., :d0, :d0] = a
    return torch.as_tensor(out, device=device)


class FullGaussianMixture(_MixtureBase):
    _NAME = 'gmm_full'
    _count_parameters = staticmethod(n_parameters)

    def __init__(self, n_components=1, *, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans', weights_init=None,
                 means_init=None, precisions_init=None, random_state=None):
        if covariance_type not in COV_TYPES:
            raise ValueError("covariance_type must be 'full' or 'tied' (gmm.GaussianMixture has 'diag' and 'spherical'), got %r" % (covariance_type,))
        super().__init__(n_components, covariance_type, tol, reg_covar, max_iter, n_init, init_params, weights_init, means_init, precisions_init, random_state)

    @property
    def _per_component(self):          # (tied covariances are shared and stay)
        return ('covariances_', 'precisions_', 'precisions_cholesky_', '_log_det') if self.covariance_type == 'full' else ()

    def _check_precisions(self, p, d0):
        """The given precisions as (P, log_det) per matrix, factorised once on the host."""
        want = (self.n_components, d0, d0) if self.covariance_type == 'full' else (d0, d0)
        if p.shape != want:
            raise ValueError("The parameter '%s precision' should have the shape of %s, but got %s" % (self.covariance_type, want, p.shape))
        facs = []
        for m in p.reshape(-1, d0, d0):
            if not (np.allclose(m, m.T) and np.all(np.linalg.eigvalsh(m) > 0.0)):
                raise ValueError("'%s precision' should be symmetric, positive-definite" % self.covariance_type)
            facs.append(_host_factor(m))
        return np.stack([f[0] for f in facs]), np.array([f[1] for f in facs])

    def _initial_parameters(self, pts, ws, status, init_labels=None, total=None):
        K, n_runs, dev, D = self.n_components, self.n_init, pts.x.device, pts.d
        cov = COV_TYPES[self.covariance_type]
        inits = self._check_inits(pts.d0)
        if len(inits) < 3:
            labels, resp = self._draw(pts, init_labels)
            par = mstep(pts, K, cov, self.reg_covar, labels=labels, resp=resp, total=total, compute_total=total is None, status=status, ws=ws)
        else:          # everything is given: nothing is drawn.  Tied covariances still need T, which the M-step of any labels forms
            Kc = K if cov == 2 else 1
            if cov == 3 and total is None:
                total = mstep(pts, K, cov, self.reg_covar, labels=torch.zeros((1, pts.n), dtype=torch.int32, device=dev), ws=ws)['total']
            par = {'w': torch.empty((n_runs, K), dtype=torch.float64, device=dev), 'mu': torch.empty((n_runs, K, D), dtype=torch.float64, device=dev),
                   'cov': torch.eye(D, dtype=torch.float64, device=dev).repeat(n_runs, Kc, 1, 1), 'P': torch.empty((n_runs, Kc, D, D), dtype=torch.float64, device=dev),
                   'log_det': torch.empty((n_runs, Kc), dtype=torch.float64, device=dev)}
            if cov == 3:
                par['total'] = total
        par['status'] = status
        if 'w' in inits:
            par['w'][:] = _dev64(inits['w'], (1, K), dev)
        if 'mu' in inits:
            m = torch.zeros((K, D), dtype=torch.float64, device=dev)
            m[:, :pts.d0] = _dev64(inits['mu'] - pts.shift_host[None, :], (K, pts.d0), dev)
            par['mu'][:] = m[None]
        if 'prec' in inits:
            par['P'][:] = _pad_square(inits['prec'][0], D, dev)[None]
            par['log_det'][:] = _dev64(inits['prec'][1], (1, -1), dev)
            status[:, 0] = 0.0          # (the factors are the given ones: whatever the covariances of the drawn responsibilities were)
            status[:, 7] = 0.0
        return par

    def _device_parameters(self, pts):
        """The fitted parameters against the training shift, padded; the factor of the kept covariances is the kept one (``precisions_cholesky_``)."""
        K, dev, d0 = self.n_components, pts.x.device, self.n_features_in_
        mu = torch.zeros((K, pts.d), dtype=torch.float64, device=dev)
        mu[:, :d0] = _dev64(self._means_shifted, (K, d0), dev)
        P = _pad_square(self.precisions_cholesky_.reshape(-1, d0, d0), pts.d, dev)
        ld = _dev64(self._log_det, (-1,), dev)
        return _dev64(self.weights_, (K,), dev), mu, P, ld

    def _estep_points(self, pts, **want):
        return estep(pts, COV_TYPES[self.covariance_type], *self._device_parameters(pts), **want)

    def _fit_points(self, pts, init_labels=None, total=None):
        K, d0 = self.n_components, pts.d0
        if pts.n < K:
            raise ValueError('Expected n_samples >= n_components but got n_components = %d, n_samples = %d' % (K, pts.n))
        cov = COV_TYPES[self.covariance_type]
        ws = _workspace(pts, K, self.n_init, cov)
        status = new_status(self.n_init, self.tol, self.max_iter, pts.x.device)
        par = self._initial_parameters(pts, ws, status, init_labels, total)
        status, lbs = em(pts, cov, self.reg_covar, par, status, self.max_iter, ws=ws)
        self._status, self._all_lower_bounds = status, lbs
        self._scatter_total = par.get('total')
        if (status[:, 7] != 0).any():
            raise ValueError(_ILL_DEFINED)
        best = self._publish(pts, status, lbs, par['w'], par['mu'])
        C = par['cov'][best, :, :d0, :d0].cpu().numpy()
        P = par['P'][best, :, :d0, :d0].cpu().numpy()
        self._log_det = par['log_det'][best].cpu().numpy()
        if self.covariance_type == 'tied':
            C, P = C[0], P[0]
        self.covariances_ = np.ascontiguousarray(C)
        self.precisions_cholesky_ = np.ascontiguousarray(P)
        self.precisions_ = P @ np.swapaxes(P, -1, -2)
        self._all_parameters = {k: par[k].cpu().numpy() for k in ('w', 'mu', 'cov', 'P', 'log_det')}
        # the final E-step (_base.py:321-325): labels consistent with the kept parameters
        self.labels_ = estep(pts, cov, par['w'][best], par['mu'][best], par['P'][best], par['log_det'][best], labels=True, ws=ws)['labels'].cpu().numpy()
        return self


def gmm_full_sweep(X, ks, **kw):
    """{K: fitted ``FullGaussianMixture(n_components=K, **kw)``} for every K of ``ks``: X is uploaded, padded and shifted once, and for tied covariances the
    total scatter matrix T is formed once, by the first fit."""
    pts = _Points(X)
    fits, total = {}, None
    for k in ks:
        fits[int(k)] = FullGaussianMixture(n_components=int(k), **kw)._fit_points(pts, total=total)
        total = fits[int(k)]._scatter_total
    return fits
