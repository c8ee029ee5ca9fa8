"""``GaussianMixture`` with scikit-learn's estimator surface on the MI355X, for diagonal and spherical covariances (csrc/dic_gmm.hip): the p2 / p4
``--cluster_method gmm`` branches.

Every other clustering family of the post-hoc side returns a hard partition; the mixture gives responsibilities per encounter (comparable with DEC's ``q``),
BIC and AIC per K from the fits themselves, and a model p4 applies unchanged to the validation and test cohorts.  Control flow follows scikit-learn 1.7.2
(``mixture/_base.py`` fit_predict :223-330, ``_initialize_parameters`` :98-141; ``_gaussian_mixture.py`` ``_initialize`` :788-817, bic / aic :881-933).  The
arithmetic is the f64 definition in include/dic_hip.h: one EM iteration is one pass over the f32 points and a fixed-order reduction, so two fits give the same
bits.  The points enter shifted by their column means ``c`` (x' = (double)x - c, the means are kept as mu - c on the device): algebraically the same model,
without the E[x^2] - mu^2 cancellation for latents far from the origin.  EM consumes no randomness, so the ``n_init`` initialisations are drawn first, in
order, from one stream, and the restarts then advance TOGETHER (grid.y = restart), as ``kmeans.lloyd`` runs them; the host reads the done flags every
``_POLL_EVERY`` iterations.

Outputs are NumPy f64, like sklearn's.  The package imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .kmeans import KMeans, _as_device_matrix, _device, _pad_features, _pp_init
from .ward import _usable_view

_POLL_EVERY = 4      # EM iterations enqueued between two host reads of the done flags
COV_TYPES = {'diag': 0, 'spherical': 1}
_NOT_CONVERGED = ('Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check for degenerate data.')


class _Points:
    """The points as the kernels take them: ``x`` (N, D) f32 on the device (a qualifying strided view in place, else a zero-padded copy), the true feature
    count ``d0``, and the shift ``c`` (D) f64 on the device (zeros in the padding)."""

    def __init__(self, X, shift=None):
        shape = tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape
        if len(shape) != 2:
            raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (shape,))
        n, width = shape
        if width > MAX_DIM:
            raise NotImplementedError('gmm: at most %d features (got %d)' % (MAX_DIM, width))
        if n < 2 or width < 1:
            raise ValueError('gmm needs at least 2 points of at least 1 feature, got shape %s' % (shape,))
        self.x = X.detach() if _usable_view(X) else _pad_features(_as_device_matrix(X, _device())).contiguous()
        self.n, self.d0, self.d = n, width, self.x.shape[1]
        dev = self.x.device
        if shift is None:
            c = self.x.double().mean(dim=0)          # (a contiguous f64 copy whatever the strides: the same bits for a view and for its copy)
        else:
            c = torch.zeros(self.d, dtype=torch.float64, device=dev)
            c[:width] = torch.as_tensor(np.asarray(shift, dtype=np.float64).reshape(width), device=dev)
        self.shift = c.contiguous()
        self.shift_host = self.shift[:width].cpu().numpy()


def _require_bytes(nbytes, device, n, d, k, runs):
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > free:
        raise MemoryError('the Gaussian mixture of %d points needs %d bytes on the device, %d are free: the f64 partial sums of at most 256 workgroups, '
                          '8 (2 K D + K + 1) bytes each (K = %d, D = %d), per restart (%d)' % (n, nbytes, free, k, d, runs))


def _workspace(pts, K, n_runs):
    nbytes = int(N.lib().dic_gmm_workspace(pts.n, pts.d, K, n_runs))
    if nbytes == 0:
        raise ValueError('gmm: N=%d D=%d K=%d n_init=%d is outside the kernel\'s limits (2 <= N < 2^30, K <= %d)' % (pts.n, pts.d, K, n_runs, N.MAX_CLUSTERS))
    _require_bytes(nbytes, pts.x.device, pts.n, pts.d, K, n_runs)
    return torch.empty(max(16, nbytes), dtype=torch.uint8, device=pts.x.device)


def _dev64(a, shape, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=device).reshape(shape).contiguous()


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
    dev = pts.x.device
    status = torch.zeros((n_runs, 8), dtype=torch.float64, device=dev)
    status[:, 3] = -float('inf')
    status[:, 4] = float(tol)
    status[:, 5] = float(max_iter)
    lbs = torch.full((n_runs, max_iter), float('nan'), dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    st = N.stream_of(pts.x)
    it = 0
    while it < max_iter:
        for _ in range(min(_POLL_EVERY, max_iter - it)):
            N.check(L.dic_gmm_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift), N.ptr(w),
                                      N.ptr(mu), N.ptr(var), N.ptr(status), N.ptr(lbs), max_iter, N.ptr(ws), ws.numel(), st), 'dic_gmm_em_iter')
            it += 1
        if bool((status[:, 0] != 0).all()):          # the only host sync of the loop
            break
    return status.cpu().numpy(), lbs.cpu().numpy()


def estep(pts, w, mu, var, lse=False, log_resp=False, labels=False, total=False, ws=None):
    """The E-step of one parameter set ((K), (K, D), (K, D) f64 on the device).  Returns a dict of the requested outputs, on the device: ``lse`` (N) f64,
    ``log_resp`` (N, K) f64, ``labels`` (N) int32, ``total`` (1) f64 = sum_i lse_i."""
    K, dev = w.shape[-1], pts.x.device
    out = {}
    if lse:
        out['lse'] = torch.empty(pts.n, dtype=torch.float64, device=dev)
    if log_resp:
        out['log_resp'] = torch.empty((pts.n, K), dtype=torch.float64, device=dev)
    if labels:
        out['labels'] = torch.empty(pts.n, dtype=torch.int32, device=dev)
    if total:
        out['total'] = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, 1) if ws is None else ws
    N.check(N.lib().dic_gmm_estep(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, N.ptr(pts.shift), N.ptr(w), N.ptr(mu), N.ptr(var),
                                  N.ptr(out.get('lse')), N.ptr(out.get('log_resp')), N.ptr(out.get('labels')), N.ptr(out.get('total')), N.ptr(ws), ws.numel(),
                                  N.stream_of(pts.x)), 'dic_gmm_estep')
    return out


def n_parameters(n_components, n_features, covariance_type):
    """Free parameters of the model (``_gaussian_mixture.py:881-893``), with the true feature count."""
    cov = n_components * n_features if covariance_type == 'diag' else n_components
    return int(cov + n_features * n_components + n_components - 1)


class GaussianMixture:
    def __init__(self, n_components=1, *, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans',
                 weights_init=None, means_init=None, precisions_init=None, random_state=None, warm_start=False, verbose=0, verbose_interval=10):
        if covariance_type in ('full', 'tied'):
            raise NotImplementedError("covariance_type=%r is not on the accelerated path: K x 256 x 256 Cholesky factors are a different kernel; "
                                      "use 'diag' or 'spherical'" % (covariance_type,))
        if covariance_type not in COV_TYPES:
            raise ValueError("covariance_type must be 'diag' or 'spherical' ('full' and 'tied' are not implemented), got %r" % (covariance_type,))
        if warm_start:
            raise NotImplementedError('warm_start is not implemented: every fit draws its initialisations and runs its restarts together')
        if isinstance(n_components, bool) or not isinstance(n_components, (numbers.Integral, np.integer)) or n_components < 1:
            raise ValueError('n_components must be an int >= 1, got %r' % (n_components,))
        if n_components > N.MAX_CLUSTERS:
            raise ValueError('n_components=%d > %d: outside the compiled limit' % (n_components, N.MAX_CLUSTERS))
        if isinstance(n_init, bool) or not isinstance(n_init, (numbers.Integral, np.integer)) or n_init < 1:
            raise ValueError('n_init must be an int >= 1, got %r' % (n_init,))
        if isinstance(max_iter, bool) or not isinstance(max_iter, (numbers.Integral, np.integer)) or max_iter < 1:
            raise ValueError('max_iter must be an int >= 1, got %r' % (max_iter,))
        if not tol >= 0 or not reg_covar >= 0:
            raise ValueError('tol and reg_covar must be >= 0, got %r and %r' % (tol, reg_covar))
        if init_params not in ('kmeans', 'k-means++', 'random', 'random_from_data'):
            raise ValueError("init_params must be 'kmeans', 'k-means++', 'random' or 'random_from_data', got %r" % (init_params,))
        self.n_components = int(n_components)
        self.covariance_type = covariance_type
        self.tol = float(tol)
        self.reg_covar = float(reg_covar)
        self.max_iter = int(max_iter)
        self.n_init = int(n_init)
        self.init_params = init_params
        self.weights_init = weights_init
        self.means_init = means_init
        self.precisions_init = precisions_init
        self.random_state = random_state
        self.warm_start = False
        self.verbose = verbose
        self.verbose_interval = verbose_interval

    # -- helpers ------------------------------------------------------------------------------
    _random_state = KMeans._random_state

    def _check_inits(self, d0):
        K = self.n_components
        out = {}
        if self.weights_init is not None:
            w = np.asarray(self.weights_init, dtype=np.float64)
            if w.shape != (K,):
                raise ValueError("The parameter 'weights' should have the shape of (%d,), but got %s" % (K, w.shape))
            if (w < 0).any() or (w > 1).any() or not np.allclose(np.abs(1.0 - w.sum()), 0.0):
                raise ValueError("The parameter 'weights' should be in the range [0, 1] and normalized")
            out['w'] = w
        if self.means_init is not None:
            m = np.asarray(self.means_init, dtype=np.float64)
            if m.shape != (K, d0):
                raise ValueError("The parameter 'means' should have the shape of (%d, %d), but got %s" % (K, d0, m.shape))
            out['mu'] = m
        if self.precisions_init is not None:
            p = np.asarray(self.precisions_init, dtype=np.float64)
            want = (K, d0) if self.covariance_type == 'diag' else (K,)
            if p.shape != want:
                raise ValueError("The parameter '%s precision' should have the shape of %s, but got %s" % (self.covariance_type, want, p.shape))
            if (p <= 0).any():
                raise ValueError("'%s precision' should be positive" % self.covariance_type)
            out['prec'] = p
        return out

    def _initial_parameters(self, pts, ws, init_labels=None):
        """(w, mu', var) of the n_init restarts on the device.  Every random number is drawn here, restart by restart, in sklearn's order.  ``init_labels``
        ((n_init, N) ints; the tests' seam) replaces the draws by given hard labels."""
        K, n_runs, dev = self.n_components, self.n_init, pts.x.device
        cov = COV_TYPES[self.covariance_type]
        inits = self._check_inits(pts.d0)
        w = mu = var = None
        if len(inits) < 3:
            rs = self._random_state()
            labels = resp = None
            if init_labels is not None:
                labels = torch.as_tensor(np.ascontiguousarray(init_labels, dtype=np.int32).reshape(n_runs, pts.n), device=dev)
            elif self.init_params == 'random':
                resp = np.empty((n_runs, pts.n, K), dtype=np.float64)
                for r in range(n_runs):
                    u = rs.uniform(size=(pts.n, K))
                    resp[r] = u / u.sum(axis=1)[:, np.newaxis]
                resp = torch.as_tensor(resp, device=dev)
            else:
                labels = torch.full((n_runs, pts.n), -1, dtype=torch.int32, device=dev)
                comps = torch.arange(K, dtype=torch.int32, device=dev)
                for r in range(n_runs):
                    if self.init_params == 'kmeans':
                        km = KMeans(n_clusters=K, n_init=1, random_state=rs).fit(pts.x[:, :pts.d0])
                        labels[r] = torch.as_tensor(km.labels_.astype(np.int32), device=dev)
                    elif self.init_params == 'random_from_data':
                        idx = rs.choice(pts.n, size=K, replace=False)
                        labels[r, torch.as_tensor(idx, device=dev)] = comps
                    else:          # 'k-means++': the rows kmeans._pp_init chooses; a chosen row is found again by its values (equal rows give equal parameters)
                        rows = _pp_init(pts.x.contiguous(), K, 1, rs)[0]          # (the k-means kernels take packed rows)
                        for k in range(K):
                            hit = (pts.x == rows[k]).all(dim=1) if not torch.isnan(rows[k]).any() else None
                            if hit is None:
                                raise ValueError('gmm: the points contain NaN')
                            labels[r, int(torch.nonzero(hit)[0])] = k
            w, mu, var = mstep(pts, K, cov, self.reg_covar, labels=labels, resp=resp, ws=ws)
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

    def _points(self, X):
        if not hasattr(self, 'weights_'):
            raise RuntimeError('This GaussianMixture instance is not fitted yet.')
        if hasattr(X, 'shape') and len(X.shape) == 2 and X.shape[1] != self.n_features_in_:
            raise ValueError('X has %d features, but GaussianMixture is expecting %d features as input.' % (X.shape[1], self.n_features_in_))
        return _Points(X, shift=self._shift)

    # -- estimator API ------------------------------------------------------------------------
    def _fit_points(self, pts, init_labels=None):
        K = self.n_components
        if pts.n < K:
            raise ValueError('Expected n_samples >= n_components but got n_components = %d, n_samples = %d' % (K, pts.n))
        cov = COV_TYPES[self.covariance_type]
        ws = _workspace(pts, K, self.n_init)
        w, mu, var = self._initial_parameters(pts, ws, init_labels)
        status, lbs = em(pts, cov, self.reg_covar, w, mu, var, self.tol, self.max_iter, ws=ws)
        best, max_lb = 0, -np.inf
        for r in range(self.n_init):          # _base.py:283-290: the first of equal bounds wins
            if status[r, 3] > max_lb or max_lb == -np.inf:
                best, max_lb = r, status[r, 3]
        self.converged_ = bool(status[best, 2] != 0)
        if not self.converged_:
            warnings.warn(_NOT_CONVERGED, UserWarning)
        self.n_iter_ = int(status[best, 1])
        self.lower_bound_ = float(status[best, 3])
        self.lower_bounds_ = lbs[best, :self.n_iter_].copy()
        self.n_features_in_ = pts.d0
        self._shift = pts.shift_host.copy()
        self._means_shifted = mu[best, :, :pts.d0].cpu().numpy()
        self.weights_ = w[best].cpu().numpy()
        self.means_ = self._means_shifted + self._shift[None, :]
        v = var[best, :, :pts.d0].cpu().numpy()
        self.covariances_ = v if self.covariance_type == 'diag' else v[:, 0].copy()
        self.precisions_cholesky_ = 1.0 / np.sqrt(self.covariances_)
        self.precisions_ = self.precisions_cholesky_ ** 2
        self._status, self._all_lower_bounds = status, lbs
        self._all_parameters = (w.cpu().numpy(), mu[:, :, :pts.d0].cpu().numpy(), var[:, :, :pts.d0].cpu().numpy())
        # the final E-step (_base.py:321-325): labels consistent with the kept parameters
        self.labels_ = estep(pts, w[best].contiguous(), mu[best].contiguous(), var[best].contiguous(), labels=True, ws=ws)['labels'].cpu().numpy()
        return self

    def fit(self, X, y=None):
        return self._fit_points(_Points(X))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def _estep(self, X, **want):
        pts = self._points(X)
        return pts, estep(pts, *self._device_parameters(pts), **want)

    def predict(self, X):
        """(N,) int32 numpy: the component of largest weighted log-probability (the first of equal ones)."""
        return self._estep(X, labels=True)[1]['labels'].cpu().numpy()

    def predict_proba(self, X):
        """(N, K) f64 numpy: the responsibilities, exp(log r)."""
        return torch.exp(self._estep(X, log_resp=True)[1]['log_resp']).cpu().numpy()

    def score_samples(self, X):
        """(N,) f64 numpy: the log-likelihood of every row."""
        return self._estep(X, lse=True)[1]['lse'].cpu().numpy()

    def score(self, X, y=None):
        """The mean log-likelihood per row, summed in fixed order on the device."""
        pts, out = self._estep(X, total=True)
        return float(out['total'].cpu().numpy()[0]) / pts.n

    def reorder(self, order):
        """Renumber the components: new component j is old component ``order[j]`` (p4 orders them by systolic pressure)."""
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(self.n_components)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (self.n_components - 1, order.tolist()))
        for name in ('weights_', 'means_', '_means_shifted', 'covariances_', 'precisions_', 'precisions_cholesky_'):
            setattr(self, name, getattr(self, name)[order].copy())
        if hasattr(self, 'labels_'):
            inverse = np.empty_like(order)
            inverse[order] = np.arange(len(order))
            self.labels_ = inverse[self.labels_].astype(self.labels_.dtype)
        return self

    def _n_parameters(self):
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    def bic(self, X):
        n = X.shape[0]
        return -2 * self.score(X) * n + self._n_parameters() * np.log(n)

    def aic(self, X):
        return -2 * self.score(X) * X.shape[0] + 2 * self._n_parameters()

    def sample(self, n_samples=1):
        raise NotImplementedError('sample is not implemented: the accelerated path fits and scores; draw from means_ / covariances_ with NumPy')

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, covariance_type=self.covariance_type, tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter,
                    n_init=self.n_init, init_params=self.init_params, weights_init=self.weights_init, means_init=self.means_init,
                    precisions_init=self.precisions_init, random_state=self.random_state)


def gmm_sweep(X, ks, **kw):
    """{K: fitted ``GaussianMixture(n_components=K, **kw)``} for every K of ``ks``: X is uploaded, padded and shifted once."""
    pts = _Points(X)
    return {int(k): GaussianMixture(n_components=int(k), **kw)._fit_points(pts) for k in ks}
