"""What the Gaussian mixture front ends share: ``gmm.py`` (diagonal and spherical covariances), ``gmm_full.py`` (full and tied ones) and ``bgmm.py`` (the
variational Bayesian mixture) add their native calls, their parameters and their errors to the estimator below.

Control flow follows scikit-learn 1.7.2 (``mixture/_base.py`` fit_predict :223-330, ``_initialize_parameters`` :98-141; ``_gaussian_mixture.py``
``_initialize`` :788-817, bic / aic :881-933).  The points enter shifted by their column means ``c`` (x' = (double)x - c, the means are kept as mu - c on the
device): algebraically the same model, without the E[x^2] - mu^2 cancellation for latents far from the origin.  EM consumes no randomness, so the ``n_init``
initialisations are drawn first, in order, from one stream (``_draw``), and the restarts then advance TOGETHER (grid.y = restart), as ``kmeans.lloyd`` runs
them; the host reads the done flags every ``_POLL_EVERY`` iterations (``run_em``).  The first of equal lower bounds wins (``_publish``).

Outputs are NumPy f64, like sklearn's.  The module imports neither sklearn nor scipy; there is no CPU fallback.
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


def _dev64(a, shape, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=device).reshape(shape).contiguous()


def workspace(pts, K, n_runs, size, name, needs):
    """The workspace of ``n_runs`` restarts: ``size(N, D, K, n_runs)`` is the native size function, ``name`` the module in the error of a shape it refuses,
    ``needs`` the ``MemoryError`` text (fields n, nbytes, free, k, d, runs)."""
    nbytes = int(size(pts.n, pts.d, K, n_runs))
    if nbytes == 0:
        raise ValueError('%s: N=%d D=%d K=%d n_init=%d is outside the kernel\'s limits (2 <= N < 2^30, K <= %d)' % (name, pts.n, pts.d, K, n_runs, N.MAX_CLUSTERS))
    free = torch.cuda.mem_get_info(pts.x.device)[0]
    if nbytes > free:
        raise MemoryError(needs.format(n=pts.n, nbytes=nbytes, free=free, k=K, d=pts.d, runs=n_runs))
    return torch.empty(max(16, nbytes), dtype=torch.uint8, device=pts.x.device)


def new_status(n_runs, tol, max_iter, device):
    """The status block of ``n_runs`` restarts, (n_runs, 8) f64 on the device: done, iterations, stopped by tol, last lower bound, tol, max_iter, .."""
    status = torch.zeros((n_runs, 8), dtype=torch.float64, device=device)
    status[:, 3] = -float('inf')
    status[:, 4] = float(tol)
    status[:, 5] = float(max_iter)
    return status


def run_em(iterate, status, max_iter):
    """EM until every restart of ``status`` is done: ``iterate(lower_bounds)`` enqueues one iteration of all of them.  Returns (status (n_runs, 8) f64 numpy,
    lower_bounds (n_runs, max_iter) f64 numpy, NaN beyond a restart's iterations)."""
    lbs = torch.full((status.shape[0], max_iter), float('nan'), dtype=torch.float64, device=status.device)
    it = 0
    while it < max_iter:
        for _ in range(min(_POLL_EVERY, max_iter - it)):
            iterate(lbs)
            it += 1
        if bool((status[:, 0] != 0).all()):          # the only host sync of the loop
            break
    return status.cpu().numpy(), lbs.cpu().numpy()


def estep_outputs(pts, K, lse=False, log_resp=False, labels=False, total=False):
    """The requested outputs of an E-step, on the device: ``lse`` (N) f64, ``log_resp`` (N, K) f64, ``labels`` (N) int32, ``total`` (1) f64 = sum_i lse_i."""
    dev = pts.x.device
    out = {}
    if lse:
        out['lse'] = torch.empty(pts.n, dtype=torch.float64, device=dev)
    if log_resp:
        out['log_resp'] = torch.empty((pts.n, K), dtype=torch.float64, device=dev)
    if labels:
        out['labels'] = torch.empty(pts.n, dtype=torch.int32, device=dev)
    if total:
        out['total'] = torch.empty(1, dtype=torch.float64, device=dev)
    return out


class _MixtureBase:
    """The estimator surface of both families.  A subclass gives ``_NAME`` (the module in its messages), ``_per_component`` (the covariance attributes
    ``reorder`` permutes), ``_count_parameters``, ``_check_precisions``, ``_fit_points``, ``_device_parameters`` and ``_estep_points``."""

    def __init__(self, n_components, covariance_type, tol, reg_covar, max_iter, n_init, init_params, weights_init, means_init, precisions_init, random_state):
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

    # -- helpers ------------------------------------------------------------------------------
    _random_state = KMeans._random_state

    def _check_inits(self, d0):
        """The given initial parameters, checked: 'w', 'mu', and 'prec' as the subclass's ``_check_precisions`` returns them."""
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
            out['prec'] = self._check_precisions(np.asarray(self.precisions_init, dtype=np.float64), d0)
        return out

    def _draw(self, pts, init_labels):
        """(labels (n_init, N) int32, -1: no component; resp (n_init, N, K) f64) of the restarts, one of them None, on the device.  Every random number is
        drawn here, restart by restart, in sklearn's order.  ``init_labels`` ((n_init, N) ints; the tests' seam) replaces the draws by given hard labels."""
        K, n_runs, dev = self.n_components, self.n_init, pts.x.device
        rs = self._random_state()
        if init_labels is not None:
            return torch.as_tensor(np.ascontiguousarray(init_labels, dtype=np.int32).reshape(n_runs, pts.n), device=dev), None
        if self.init_params == 'random':
            resp = np.empty((n_runs, pts.n, K), dtype=np.float64)
            for r in range(n_runs):
                u = rs.uniform(size=(pts.n, K))
                resp[r] = u / u.sum(axis=1)[:, np.newaxis]
            return None, torch.as_tensor(resp, device=dev)
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
                    if torch.isnan(rows[k]).any():
                        raise ValueError('%s: the points contain NaN' % self._NAME)
                    labels[r, int(torch.nonzero((pts.x == rows[k]).all(dim=1))[0])] = k
        return labels, None

    def _publish(self, pts, status, lbs, w, mu):
        """Picks the winner among the restarts (``status``, ``lbs``: what ``run_em`` returned; w (n_init, K), mu (n_init, K, D) on the device) and sets the
        fitted attributes both families have.  Returns the winner's index."""
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
        if w is not None:          # (the Bayesian mixture forms its weights from the Dirichlet parameters)
            self.weights_ = w[best].cpu().numpy()
        self.means_ = self._means_shifted + self._shift[None, :]
        return best

    def _points(self, X):
        if not hasattr(self, 'weights_'):
            raise RuntimeError('This %s instance is not fitted yet.' % type(self).__name__)
        if hasattr(X, 'shape') and len(X.shape) == 2 and X.shape[1] != self.n_features_in_:
            raise ValueError('X has %d features, but %s is expecting %d features as input.' % (X.shape[1], type(self).__name__, self.n_features_in_))
        return _Points(X, shift=self._shift)

    # -- estimator API ------------------------------------------------------------------------
    def fit(self, X, y=None):
        return self._fit_points(_Points(X))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def _estep(self, X, **want):
        pts = self._points(X)
        return pts, self._estep_points(pts, **want)

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
        """Renumber the components: new component j is old component ``order[j]`` (p4 orders them by systolic pressure).  What the components share (tied
        covariances) stays."""
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(self.n_components)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (self.n_components - 1, order.tolist()))
        for name in ('weights_', 'means_', '_means_shifted') + tuple(self._per_component):
            setattr(self, name, getattr(self, name)[order].copy())
        if hasattr(self, 'labels_'):
            inverse = np.empty_like(order)
            inverse[order] = np.arange(len(order))
            self.labels_ = inverse[self.labels_].astype(self.labels_.dtype)
        return self

    def _n_parameters(self):
        return self._count_parameters(self.n_components, self.n_features_in_, self.covariance_type)

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
