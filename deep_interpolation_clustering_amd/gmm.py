"""``GaussianMixture`` with scikit-learn's estimator surface on the MI355X, for diagonal and spherical covariances (csrc/dic_gmm.hip): the p2 / p4
``--cluster_method gmm`` branches.

Every other clustering family of the post-hoc side returns a hard partition; the mixture gives responsibilities per encounter (comparable with DEC's ``q``),
BIC and AIC per K from the fits themselves, and a model p4 applies unchanged to the validation and test cohorts.  The estimator surface, the draws of the
initialisations and the control flow of a fit are ``_gmm_base.py``'s, shared with ``gmm_full.py``; this file adds the native calls and the covariance
parameters of its two types.  The arithmetic is the f64 definition in include/dic_hip.h: one EM iteration is one pass over the f32 points and a fixed-order
reduction, so two fits give the same bits.

Outputs are NumPy f64, like sklearn's.  The package imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from ._gmm_base import _dev64, _MixtureBase, _Points, estep_outputs, new_status, run_em, workspace

COV_TYPES = {'diag': 0, 'spherical': 1}
_NEEDS = ('the Gaussian mixture of {n} points needs {nbytes} bytes on the device, {free} are free: the f64 partial sums of at most 256 workgroups, '
          '8 (2 K D + K + 1) bytes each (K = {k}, D = {d}), per restart ({runs})')


def _workspace(pts, K, n_runs):
    return workspace(pts, K, n_runs, N.lib().dic_gmm_workspace, 'gmm', _NEEDS)


def mstep(pts, K, cov_type, reg_covar, labels=None, resp=None, ws=None):
    """The M-step of every restart from hard labels ((n_runs, N) int32 on the device, -1: no component) or from responsibilities ((n_runs, N, K) f64):
    (weights (n_runs, K), shifted means (n_runs, K, D), variances (n_runs, K, D)), f64 on the device."""
    src = labels if labels is not None else resp
    n_runs, dev = src.shape[0], pts.x.device
    w = torch.empty((n_runs, K), dtype=torch.float64, device=dev)
    mu = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
    var = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    N.check(N.lib().dic_gmm_mstep_labels(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift),
                                         N.ptr(labels), N.ptr(resp), N.ptr(w), N.ptr(mu), N.ptr(var), N.ptr(ws), ws.numel(), N.stream_of(pts.x)),
            'dic_gmm_mstep_labels')
    return w, mu, var


def em(pts, cov_type, reg_covar, w, mu, var, tol, max_iter, ws=None):
    """EM on every restart of (w, mu, var) -- updated in place -- until each is done.  Returns (status (n_runs, 8) f64 numpy: done, iterations, stopped by tol,
    last lower bound, ..; lower_bounds (n_runs, max_iter) f64 numpy, NaN beyond a restart's iterations)."""
    L = N.lib()
    n_runs, K = w.shape
    status = new_status(n_runs, tol, max_iter, pts.x.device)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    st = N.stream_of(pts.x)

    def iterate(lbs):
        N.check(L.dic_gmm_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift), N.ptr(w),
                                  N.ptr(mu), N.ptr(var), N.ptr(status), N.ptr(lbs), max_iter, N.ptr(ws), ws.numel(), st), 'dic_gmm_em_iter')
    return run_em(iterate, status, max_iter)


def estep(pts, w, mu, var, lse=False, log_resp=False, labels=False, total=False, ws=None):
    """The E-step of one parameter set ((K), (K, D), (K, D) f64 on the device).  Returns a dict of the requested outputs, on the device: ``lse`` (N) f64,
    ``log_resp`` (N, K) f64, ``labels`` (N) int32, ``total`` (1) f64 = sum_i lse_i."""
    K = w.shape[-1]
    out = estep_outputs(pts, K, lse, log_resp, labels, total)
    ws = _workspace(pts, K, 1) if ws is None else ws
    N.check(N.lib().dic_gmm_estep(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, N.ptr(pts.shift), N.ptr(w), N.ptr(mu), N.ptr(var),
                                  N.ptr(out.get('lse')), N.ptr(out.get('log_resp')), N.ptr(out.get('labels')), N.ptr(out.get('total')), N.ptr(ws), ws.numel(),
                                  N.stream_of(pts.x)), 'dic_gmm_estep')
    return out


def n_parameters(n_components, n_features, covariance_type):
    """Free parameters of the model (``_gaussian_mixture.py:881-893``), with the true feature count."""
    cov = n_components * n_features if covariance_type == 'diag' else n_components
    return int(cov + n_features * n_components + n_components - 1)


class GaussianMixture(_MixtureBase):
    _NAME = 'gmm'
    _per_component = ('covariances_', 'precisions_', 'precisions_cholesky_')
    _count_parameters = staticmethod(n_parameters)

    def __init__(self, n_components=1, *, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans',
                 weights_init=None, means_init=None, precisions_init=None, random_state=None, warm_start=False, verbose=0, verbose_interval=10):
        if covariance_type in ('full', 'tied'):
            raise NotImplementedError("covariance_type=%r is not on the accelerated path: K x 256 x 256 Cholesky factors are a different kernel; "
                                      "use 'diag' or 'spherical'" % (covariance_type,))
        if covariance_type not in COV_TYPES:
            raise ValueError("covariance_type must be 'diag' or 'spherical' ('full' and 'tied' are not implemented), got %r" % (covariance_type,))
        if warm_start:
            raise NotImplementedError('warm_start is not implemented: every fit draws its initialisations and runs its restarts together')
        super().__init__(n_components, covariance_type, tol, reg_covar, max_iter, n_init, init_params, weights_init, means_init, precisions_init, random_state)
        self.warm_start = False
        self.verbose = verbose
        self.verbose_interval = verbose_interval

    def _check_precisions(self, p, d0):
        want = (self.n_components, d0) if self.covariance_type == 'diag' else (self.n_components,)
        if p.shape != want:
            raise ValueError("The parameter '%s precision' should have the shape of %s, but got %s" % (self.covariance_type, want, p.shape))
        if (p <= 0).any():
            raise ValueError("'%s precision' should be positive" % self.covariance_type)
        return p

    def _initial_parameters(self, pts, ws, init_labels=None):
        """(w, mu', var) of the n_init restarts on the device: the M-step of the draws, then the given initial parameters in their place."""
        K, n_runs, dev = self.n_components, self.n_init, pts.x.device
        inits = self._check_inits(pts.d0)
        if len(inits) < 3:
            labels, resp = self._draw(pts, init_labels)
            w, mu, var = mstep(pts, K, COV_TYPES[self.covariance_type], self.reg_covar, labels=labels, resp=resp, ws=ws)
        else:
            w = torch.empty((n_runs, K), dtype=torch.float64, device=dev)
            mu = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
            var = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
        if 'w' in inits:
            w[:] = _dev64(inits['w'], (1, K), dev)
        if 'mu' in inits:
            m = torch.zeros((K, pts.d), dtype=torch.float64, device=dev)
            m[:, :pts.d0] = _dev64(inits['mu'] - pts.shift_host[None, :], (K, pts.d0), dev)
            mu[:] = m[None]
        if 'prec' in inits:
            v = torch.full((K, pts.d), 1.0, dtype=torch.float64, device=dev)
            p = inits['prec'] if self.covariance_type == 'diag' else np.repeat(inits['prec'][:, None], pts.d0, axis=1)
            v[:, :pts.d0] = _dev64(1.0 / p, (K, pts.d0), dev)
            if self.covariance_type == 'spherical':
                v[:, pts.d0:] = v[:, :1]
            var[:] = v[None]
        return w.contiguous(), mu.contiguous(), var.contiguous()

    def _device_parameters(self, pts):
        """The fitted parameters against the shift of ``pts`` (the training shift: ``predict`` on another cohort keeps the model, not the cohort's means)."""
        K, dev = self.n_components, pts.x.device
        if pts.d0 != self.n_features_in_:
            raise ValueError('X has %d features, but GaussianMixture is expecting %d features as input.' % (pts.d0, self.n_features_in_))
        mu = torch.zeros((K, pts.d), dtype=torch.float64, device=dev)
        mu[:, :pts.d0] = _dev64(self._means_shifted, (K, pts.d0), dev)
        var = torch.ones((K, pts.d), dtype=torch.float64, device=dev)
        cov = self.covariances_ if self.covariance_type == 'diag' else np.repeat(self.covariances_[:, None], pts.d0, axis=1)
        var[:, :pts.d0] = _dev64(cov, (K, pts.d0), dev)
        return _dev64(self.weights_, (K,), dev), mu, var

    def _estep_points(self, pts, **want):
        return estep(pts, *self._device_parameters(pts), **want)

    def _fit_points(self, pts, init_labels=None):
        K = self.n_components
        if pts.n < K:
            raise ValueError('Expected n_samples >= n_components but got n_components = %d, n_samples = %d' % (K, pts.n))
        ws = _workspace(pts, K, self.n_init)
        w, mu, var = self._initial_parameters(pts, ws, init_labels)
        status, lbs = em(pts, COV_TYPES[self.covariance_type], self.reg_covar, w, mu, var, self.tol, self.max_iter, ws=ws)
        self._status, self._all_lower_bounds = status, lbs
        best = self._publish(pts, status, lbs, w, mu)
        v = var[best, :, :pts.d0].cpu().numpy()
        self.covariances_ = v if self.covariance_type == 'diag' else v[:, 0].copy()
        self.precisions_cholesky_ = 1.0 / np.sqrt(self.covariances_)
        self.precisions_ = self.precisions_cholesky_ ** 2
        self._all_parameters = (w.cpu().numpy(), mu[:, :, :pts.d0].cpu().numpy(), var[:, :, :pts.d0].cpu().numpy())
        # the final E-step (_base.py:321-325): labels consistent with the kept parameters
        self.labels_ = estep(pts, w[best].contiguous(), mu[best].contiguous(), var[best].contiguous(), labels=True, ws=ws)['labels'].cpu().numpy()
        return self


def gmm_sweep(X, ks, **kw):
    """{K: fitted ``GaussianMixture(n_components=K, **kw)``} for every K of ``ks``: X is uploaded, padded and shifted once."""
    pts = _Points(X)
    return {int(k): GaussianMixture(n_components=int(k), **kw)._fit_points(pts) for k in ks}
