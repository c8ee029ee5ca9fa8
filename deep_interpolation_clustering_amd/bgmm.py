"""``BayesianGaussianMixture`` with scikit-learn's estimator surface on the MI355X, for diagonal and spherical covariances (csrc/dic_bgmm.hip): the p2 / p4
``--cluster_method bgmm`` branches.

Every other method of the post-hoc side answers "how many phenotypes" with a sweep over K and an index per K, or with a density threshold.  The variational
mixture is given an upper bound on the number of components; its Dirichlet-process prior empties the components the data do not support, so ONE fit returns
the effective number of components (``active_components_``), responsibilities per encounter (comparable with DEC's ``q``) and a model p4 applies unchanged
to the other cohorts.  The estimator surface, the draws of the initialisations, the restarts-together loop and the winner choice are ``_gmm_base.py``'s,
shared with ``gmm.py`` and ``gmm_full.py``; this file adds the priors, the native calls and the parameters of the variational posterior.  The arithmetic is
the f64 definition at the head of csrc/dic_bgmm.hip (sklearn 1.7.2's ``_bayesian_mixture.py``): one iteration is one pass over the f32 points, a fixed-order
reduction and a finish step, so two fits give the same bits.

Outputs are NumPy f64, like sklearn's.  The module imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from ._gmm_base import _dev64, _MixtureBase, _Points, estep_outputs, new_status, run_em, workspace

COV_TYPES = {'diag': 0, 'spherical': 1}
PRIOR_TYPES = {'dirichlet_process': 0, 'dirichlet_distribution': 1}
# rows of the per-component block `comp` (n_runs, COMP_WORDS, K): include/dic_hip.h
COMP_WORDS = 10
C_NK, C_KAPPA, C_NU, C_L, C_LOGLAMBDA, C_LGAMMA, C_A, C_B, C_ELOGPI, C_LC = range(COMP_WORDS)
_NEEDS = ('the Bayesian Gaussian mixture of {n} points needs {nbytes} bytes on the device, {free} are free: the f64 partial sums of at most 256 workgroups, '
          '8 (2 K D + K + 2) bytes each (K = {k}, D = {d}), per restart ({runs})')


def _workspace(pts, K, n_runs):
    return workspace(pts, K, n_runs, N.lib().dic_bgmm_workspace, 'bgmm', _NEEDS)


def prior_moments(pts):
    """The per-column ``var(ddof=1)`` of the points, (D) f64 on the device (0 in the padding), formed once per point set and kept on it."""
    if getattr(pts, '_column_var', None) is None:
        xs = pts.x.double() - pts.shift[None, :]
        v = (xs * xs).sum(dim=0) / float(pts.n - 1)          # (the shift is the column mean: the second moment about it)
        v[pts.d0:] = 0.0
        pts._column_var = v.contiguous()
    return pts._column_var


class _Priors:
    """The priors of one fit as the kernels take them: the scalars, and ``m0`` (shifted) and ``s0`` as (D) f64 device arrays."""

    def __init__(self, cov_type, prior_type, gamma0, kappa0, nu0, m0, s0):
        self.cov_type, self.prior_type, self.gamma0, self.kappa0, self.nu0, self.m0, self.s0 = cov_type, prior_type, gamma0, kappa0, nu0, m0, s0

    def scalars(self, reg_covar):
        return (self.cov_type, self.prior_type, float(reg_covar), float(self.gamma0), float(self.kappa0), float(self.nu0))


def init(pts, K, pri, reg_covar, labels=None, resp=None, ws=None):
    """The M-step of every restart from hard labels ((n_runs, N) int32 on the device, -1: no component) or from responsibilities ((n_runs, N, K) f64), and
    the constants of the first pass: (shifted means (n_runs, K, D), variances (n_runs, K, D), comp (n_runs, COMP_WORDS, K)), f64 on the device."""
    src = labels if labels is not None else resp
    n_runs, dev = src.shape[0], pts.x.device
    mu = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
    var = torch.empty((n_runs, K, pts.d), dtype=torch.float64, device=dev)
    comp = torch.zeros((n_runs, COMP_WORDS, K), dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    N.check(N.lib().dic_bgmm_init(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, *pri.scalars(reg_covar), N.ptr(pts.shift), N.ptr(pri.m0),
                                  N.ptr(pri.s0), N.ptr(labels), N.ptr(resp), N.ptr(mu), N.ptr(var), N.ptr(comp), N.ptr(ws), ws.numel(), N.stream_of(pts.x)),
            'dic_bgmm_init')
    return mu, var, comp


def em(pts, pri, reg_covar, mu, var, comp, tol, max_iter, ws=None):
    """Variational EM on every restart of (mu, var, comp) -- updated in place -- until each is done.  Returns what ``_gmm_base.run_em`` returns."""
    L = N.lib()
    n_runs, K = comp.shape[0], comp.shape[2]
    status = new_status(n_runs, tol, max_iter, pts.x.device)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    st = N.stream_of(pts.x)
    scalars = pri.scalars(reg_covar)

    def iterate(lbs):
        N.check(L.dic_bgmm_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, *scalars, N.ptr(pts.shift), N.ptr(pri.m0), N.ptr(pri.s0),
                                   N.ptr(mu), N.ptr(var), N.ptr(comp), N.ptr(status), N.ptr(lbs), max_iter, N.ptr(ws), ws.numel(), st), 'dic_bgmm_em_iter')
    return run_em(iterate, status, max_iter)


def estep(pts, lc, mu, var, lse=False, log_resp=False, labels=False, total=False, ws=None):
    """The E-step of one parameter set (lc (K), mu (K, D), var (K, D) f64 on the device).  Returns a dict of the requested outputs, on the device."""
    K = lc.shape[-1]
    out = estep_outputs(pts, K, lse, log_resp, labels, total)
    ws = _workspace(pts, K, 1) if ws is None else ws
    N.check(N.lib().dic_bgmm_estep(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, N.ptr(pts.shift), N.ptr(lc), N.ptr(mu), N.ptr(var),
                                   N.ptr(out.get('lse')), N.ptr(out.get('log_resp')), N.ptr(out.get('labels')), N.ptr(out.get('total')), N.ptr(ws), ws.numel(),
                                   N.stream_of(pts.x)), 'dic_bgmm_estep')
    return out


def special_probe(x):
    """(psi(x), lgamma(x)) as the kernels evaluate them, for a 1-D array of positive f64: the tests' view of the device functions."""
    from .kmeans import _device
    xd = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=_device()).reshape(-1).contiguous()
    psi, lg = torch.empty_like(xd), torch.empty_like(xd)
    torch.cuda.current_stream(xd.device).synchronize()          # (the probe runs on the null stream)
    N.check(N.lib().dic_bgmm_special_probe(N.ptr(xd), xd.numel(), N.ptr(psi), N.ptr(lg)), 'dic_bgmm_special_probe')
    torch.cuda.synchronize(xd.device)
    return psi.cpu().numpy(), lg.cpu().numpy()


def _weights(prior_type, conc):
    """sklearn's ``_set_parameters`` weights on the host: stick breaking for the process."""
    if prior_type == 'dirichlet_process':
        total = conc[0] + conc[1]
        tmp = conc[1] / total
        w = conc[0] / total * np.hstack((1, np.cumprod(tmp[:-1])))
        return w / np.sum(w)
    return conc / np.sum(conc)


def _interval_error(name, value, array_like=False):
    return ValueError("The '%s' parameter of BayesianGaussianMixture must be None%s or a float in the range (0.0, inf). Got %r instead."
                      % (name, ', an array-like' if array_like else '', value))


def _positive_or_none(name, value):
    if value is None:
        return
    if isinstance(value, bool) or not isinstance(value, (numbers.Real, np.floating, np.integer)) or not value > 0:
        raise _interval_error(name, value)


class BayesianGaussianMixture(_MixtureBase):
    """sklearn.mixture.BayesianGaussianMixture for ``covariance_type='diag' | 'spherical'``.  The default covariance type is ``'diag'`` HERE and ``'full'``
    in sklearn: ``full`` and ``tied`` need the Wishart forms on the matrix-core kernels of dic_gmm_full.hip and raise ``NotImplementedError``.
    Beyond sklearn's attributes a fit has ``labels_``, ``lower_bounds_`` and ``active_components_``: the components that are the label of at least one
    training row, ascending."""
    _NAME = 'bgmm'
    _per_component = ('covariances_', 'precisions_', 'precisions_cholesky_', 'mean_precision_', 'degrees_of_freedom_', '_log_const')

    def __init__(self, n_components=1, *, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans',
                 weight_concentration_prior_type='dirichlet_process', weight_concentration_prior=None, mean_precision_prior=None, mean_prior=None,
                 degrees_of_freedom_prior=None, covariance_prior=None, random_state=None, warm_start=False, verbose=0, verbose_interval=10):
        if covariance_type in ('full', 'tied'):
            raise NotImplementedError("covariance_type=%r is not on the accelerated path: the Wishart forms of full and tied covariances need the matrix-core "
                                      "kernels of the full-covariance mixtures; use 'diag' or 'spherical'" % (covariance_type,))
        if covariance_type not in COV_TYPES:
            raise ValueError("covariance_type must be 'diag' or 'spherical' ('full' and 'tied' are not implemented), got %r" % (covariance_type,))
        if warm_start:
            raise NotImplementedError('warm_start is not implemented: every fit draws its initialisations and runs its restarts together')
        if weight_concentration_prior_type not in PRIOR_TYPES:
            raise ValueError("The 'weight_concentration_prior_type' parameter of BayesianGaussianMixture must be a str among {'dirichlet_distribution', "
                             "'dirichlet_process'}. Got %r instead." % (weight_concentration_prior_type,))
        _positive_or_none('weight_concentration_prior', weight_concentration_prior)
        _positive_or_none('mean_precision_prior', mean_precision_prior)
        _positive_or_none('degrees_of_freedom_prior', degrees_of_freedom_prior)
        if covariance_prior is not None and np.ndim(covariance_prior) == 0 and not (isinstance(covariance_prior, (numbers.Real, np.floating, np.integer))
                                                                                     and not isinstance(covariance_prior, bool) and covariance_prior > 0):
            raise _interval_error('covariance_prior', covariance_prior, array_like=True)
        super().__init__(n_components, covariance_type, tol, reg_covar, max_iter, n_init, init_params, None, None, None, random_state)
        self.weight_concentration_prior_type = weight_concentration_prior_type
        self.weight_concentration_prior = weight_concentration_prior
        self.mean_precision_prior = mean_precision_prior
        self.mean_prior = mean_prior
        self.degrees_of_freedom_prior = degrees_of_freedom_prior
        self.covariance_prior = covariance_prior
        self.warm_start = False
        self.verbose = verbose
        self.verbose_interval = verbose_interval

    @property
    def bic(self):          # (sklearn's estimator has neither bic nor aic: the variational bound is no likelihood to penalise)
        raise AttributeError("'BayesianGaussianMixture' object has no attribute 'bic'")

    @property
    def aic(self):
        raise AttributeError("'BayesianGaussianMixture' object has no attribute 'aic'")

    # -- the priors -----------------------------------------------------------------------------
    def _check_priors(self, d0):
        """sklearn's ``_check_parameters`` for ``d0`` features, on the host: sets the ``*_prior_`` attributes that do not depend on the points (the defaults
        of ``mean_prior_`` and ``covariance_prior_`` do: ``_priors`` sets them) and raises sklearn's errors."""
        self.weight_concentration_prior_ = 1.0 / self.n_components if self.weight_concentration_prior is None else self.weight_concentration_prior
        self.mean_precision_prior_ = 1.0 if self.mean_precision_prior is None else self.mean_precision_prior
        if self.mean_prior is not None:
            self.mean_prior_ = np.asarray(self.mean_prior, dtype=np.float64)
            if self.mean_prior_.shape != (d0,):
                raise ValueError("The parameter 'means' should have the shape of (%d,), but got %s" % (d0, self.mean_prior_.shape))
        if self.degrees_of_freedom_prior is None:
            self.degrees_of_freedom_prior_ = d0
        elif self.degrees_of_freedom_prior > d0 - 1.0:
            self.degrees_of_freedom_prior_ = self.degrees_of_freedom_prior
        else:
            raise ValueError("The parameter 'degrees_of_freedom_prior' should be greater than %d, but got %.3f." % (d0 - 1, self.degrees_of_freedom_prior))
        if self.covariance_prior is None:
            return
        if self.covariance_type == 'diag':
            self.covariance_prior_ = np.asarray(self.covariance_prior, dtype=np.float64)
            if self.covariance_prior_.shape != (d0,):
                raise ValueError("The parameter 'diag covariance_prior' should have the shape of (%d,), but got %s" % (d0, self.covariance_prior_.shape))
            if (self.covariance_prior_ <= 0).any():
                raise ValueError("'diag precision' should be positive")
        else:
            if np.ndim(self.covariance_prior) != 0:
                raise ValueError("The parameter 'spherical covariance_prior' should be a positive float, but got an array of shape %s"
                                 % (np.shape(self.covariance_prior),))
            self.covariance_prior_ = self.covariance_prior

    def _priors(self, pts):
        """The priors against the points, in the device form: the defaults of the mean and covariance priors are the points' column moments."""
        d0, dev = pts.d0, pts.x.device
        self._check_priors(d0)
        m0 = torch.zeros(pts.d, dtype=torch.float64, device=dev)
        if self.mean_prior is None:
            self.mean_prior_ = pts.shift_host.copy()
        else:
            m0[:d0] = _dev64(self.mean_prior_ - pts.shift_host, (d0,), dev)
        s0 = torch.zeros(pts.d, dtype=torch.float64, device=dev)
        if self.covariance_prior is None:
            col = prior_moments(pts)
            if self.covariance_type == 'diag':
                s0 = col
                self.covariance_prior_ = col[:d0].cpu().numpy()
            else:
                mean = col[:d0].sum() / float(d0)
                s0[:d0] = mean
                self.covariance_prior_ = float(mean.cpu())
        elif self.covariance_type == 'diag':
            s0[:d0] = _dev64(self.covariance_prior_, (d0,), dev)
        else:
            s0[:d0] = float(self.covariance_prior)
        return _Priors(COV_TYPES[self.covariance_type], PRIOR_TYPES[self.weight_concentration_prior_type], self.weight_concentration_prior_,
                       self.mean_precision_prior_, self.degrees_of_freedom_prior_, m0.contiguous(), s0.contiguous())

    # -- fitting ----------------------------------------------------------------------------------
    def _device_parameters(self, pts):
        """The fitted parameters against the shift of ``pts`` (the training shift): (lc (K), m (K, D), v (K, D)) on the device."""
        K, dev = self.n_components, pts.x.device
        if pts.d0 != self.n_features_in_:
            raise ValueError('X has %d features, but BayesianGaussianMixture is expecting %d features as input.' % (pts.d0, self.n_features_in_))
        mu = torch.zeros((K, pts.d), dtype=torch.float64, device=dev)
        mu[:, :pts.d0] = _dev64(self._means_shifted, (K, pts.d0), dev)
        var = torch.ones((K, pts.d), dtype=torch.float64, device=dev)
        cov = self.covariances_ if self.covariance_type == 'diag' else np.repeat(self.covariances_[:, None], pts.d0, axis=1)
        var[:, :pts.d0] = _dev64(cov, (K, pts.d0), dev)
        return _dev64(self._log_const, (K,), dev), mu, var

    def _estep_points(self, pts, **want):
        return estep(pts, *self._device_parameters(pts), **want)

    def _fit_points(self, pts, init_labels=None):
        K = self.n_components
        if pts.n < K:
            raise ValueError('Expected n_samples >= n_components but got n_components = %d, n_samples = %d' % (K, pts.n))
        pri = self._priors(pts)
        ws = _workspace(pts, K, self.n_init)
        labels, resp = self._draw(pts, init_labels)
        mu, var, comp = init(pts, K, pri, self.reg_covar, labels=labels, resp=resp, ws=ws)
        self._initial_parameters_ = (mu[:, :, :pts.d0].cpu().numpy(), var[:, :, :pts.d0].cpu().numpy(), comp.cpu().numpy())
        status, lbs = em(pts, pri, self.reg_covar, mu, var, comp, self.tol, self.max_iter, ws=ws)
        self._status, self._all_lower_bounds = status, lbs
        best = self._publish(pts, status, lbs, None, mu)
        c = comp.cpu().numpy()
        self._all_parameters = (mu[:, :, :pts.d0].cpu().numpy(), var[:, :, :pts.d0].cpu().numpy(), c)
        cb = c[best]
        if self.weight_concentration_prior_type == 'dirichlet_process':
            self.weight_concentration_ = (cb[C_A].copy(), cb[C_B].copy())
        else:
            self.weight_concentration_ = cb[C_A].copy()
        self.weights_ = _weights(self.weight_concentration_prior_type, self.weight_concentration_)
        self.mean_precision_ = cb[C_KAPPA].copy()
        self.degrees_of_freedom_ = cb[C_NU].copy()
        self._log_const = cb[C_LC].copy()
        v = var[best, :, :pts.d0].cpu().numpy()
        self.covariances_ = v if self.covariance_type == 'diag' else v[:, 0].copy()
        self.precisions_cholesky_ = 1.0 / np.sqrt(self.covariances_)
        self.precisions_ = self.precisions_cholesky_ ** 2
        # the final E-step (_base.py:321-325): labels consistent with the kept parameters
        self.labels_ = estep(pts, comp[best, C_LC].contiguous(), mu[best].contiguous(), var[best].contiguous(), labels=True, ws=ws)['labels'].cpu().numpy()
        self.active_components_ = np.unique(self.labels_).astype(np.int64)
        return self

    def reorder(self, order):
        """Renumber the components: new component j is old component ``order[j]``.  The Dirichlet parameters are permuted with the rest (the stick-breaking
        weights were formed from them in the fitted order and are permuted, not formed again)."""
        order = np.asarray(order, dtype=np.int64)
        old_active = self.active_components_
        super().reorder(order)
        if isinstance(self.weight_concentration_, tuple):
            self.weight_concentration_ = tuple(a[order].copy() for a in self.weight_concentration_)
        else:
            self.weight_concentration_ = self.weight_concentration_[order].copy()
        inverse = np.empty_like(order)
        inverse[order] = np.arange(len(order))
        self.active_components_ = np.sort(inverse[old_active])
        return self

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, covariance_type=self.covariance_type, tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter,
                    n_init=self.n_init, init_params=self.init_params, weight_concentration_prior_type=self.weight_concentration_prior_type,
                    weight_concentration_prior=self.weight_concentration_prior, mean_precision_prior=self.mean_precision_prior, mean_prior=self.mean_prior,
                    degrees_of_freedom_prior=self.degrees_of_freedom_prior, covariance_prior=self.covariance_prior, random_state=self.random_state,
                    warm_start=self.warm_start, verbose=self.verbose, verbose_interval=self.verbose_interval)


def bgmm_sweep(X, concentrations, **kw):
    """{gamma0: fitted ``BayesianGaussianMixture(weight_concentration_prior=gamma0, **kw)``} for every value of ``concentrations``: X is uploaded, padded
    and shifted once, and its prior moments are formed once."""
    pts = _Points(X)
    prior_moments(pts)
    return {float(g): BayesianGaussianMixture(weight_concentration_prior=float(g), **kw)._fit_points(pts) for g in concentrations}
