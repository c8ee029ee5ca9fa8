"""``FullGaussianMixture``: Gaussian mixtures with full (scikit-learn's default) or tied covariances on the MI355X (csrc/dic_gmm_full.hip), beside ``gmm.py``'s
diagonal and spherical ones: the p2 / p4 ``--cluster_method gmm --gmm_covariance_type full | tied`` branches.

The latents are 256 strongly correlated outputs of an auto-encoder; a diagonal mixture spends components on describing correlation, a full one does not.  The
model, the control flow (scikit-learn 1.7.2's, the restarts advancing together, one host read of the done flags every ``_POLL_EVERY`` iterations) and the
shifted points are ``gmm.py``'s; the arithmetic is the f64 definition in include/dic_hip.h: the E-step (x - mu_k) P_k and the weighted scatter matrices run on
the f64 matrix cores, the Cholesky factors P_k = L_k^-T are computed on the device, and every sum has a fixed order, so two fits give the same bits.

Outputs are NumPy f64, like sklearn's.  The module imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from .gmm import _NOT_CONVERGED, _POLL_EVERY, GaussianMixture, _dev64, _Points
from .kmeans import KMeans, _pp_init

COV_TYPES = {'full': 2, 'tied': 3}
_ILL_DEFINED = ('Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by singleton or collapsed '
                'samples). Try to decrease the number of components, increase reg_covar, or scale the input data.')


def _require_bytes(nbytes, device, n, d, k, runs, cov_type):
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > free:
        raise MemoryError('the %s-covariance Gaussian mixture of %d points needs %d bytes on the device, %d are free: log r (8 N K), the partial sums and the '
                          'slab matrices of the scatter kernel (8 K D^2 each for full covariances; K = %d, D = %d), per restart (%d)'
                          % ('full' if cov_type == 2 else 'tied', n, nbytes, free, k, d, runs))


def _workspace(pts, K, n_runs, cov_type):
    nbytes = int(N.lib().dic_gmm_full_workspace(pts.n, pts.d, K, n_runs, cov_type))
    if nbytes == 0:
        raise ValueError('gmm_full: N=%d D=%d K=%d n_init=%d is outside the kernel\'s limits (2 <= N < 2^30, K <= %d)' % (pts.n, pts.d, K, n_runs, N.MAX_CLUSTERS))
    _require_bytes(nbytes, pts.x.device, pts.n, pts.d, K, n_runs, cov_type)
    return torch.empty(max(16, nbytes), dtype=torch.uint8, device=pts.x.device)


def new_status(n_runs, tol, max_iter, device):
    status = torch.zeros((n_runs, 8), dtype=torch.float64, device=device)
    status[:, 3] = -float('inf')
    status[:, 4] = float(tol)
    status[:, 5] = float(max_iter)
    return status


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
    dev = pts.x.device
    lbs = torch.full((n_runs, max_iter), float('nan'), dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, n_runs, cov_type) if ws is None else ws
    st = N.stream_of(pts.x)
    it = 0
    while it < max_iter:
        for _ in range(min(_POLL_EVERY, max_iter - it)):
            N.check(L.dic_gmm_full_em_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, pts.d0, K, n_runs, cov_type, float(reg_covar), N.ptr(pts.shift),
                                           N.ptr(par['w']), N.ptr(par['mu']), N.ptr(par['cov']), N.ptr(par['P']), N.ptr(par['log_det']), N.ptr(par.get('total')),
                                           N.ptr(status), N.ptr(lbs), max_iter, N.ptr(ws), ws.numel(), st), 'dic_gmm_full_em_iter')
            it += 1
        if bool((status[:, 0] != 0).all()):          # the only host sync of the loop
            break
    return status.cpu().numpy(), lbs.cpu().numpy()


def estep(pts, cov_type, w, mu, P, log_det, lse=False, log_resp=False, labels=False, total=False, ws=None):
    """The E-step of one parameter set ((K), (K, D), (Kc, D, D), (Kc) f64 on the device): a dict of the requested outputs, as ``gmm.estep``."""
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


class FullGaussianMixture:
    def __init__(self, n_components=1, *, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans', weights_init=None,
                 means_init=None, precisions_init=None, random_state=None):
        if covariance_type not in COV_TYPES:
            raise ValueError("covariance_type must be 'full' or 'tied' (gmm.GaussianMixture has 'diag' and 'spherical'), got %r" % (covariance_type,))
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

    _random_state = KMeans._random_state

    def _check_inits(self, d0):
        """The given initial parameters, checked: w, mu, and the precisions as (P, log_det) per matrix, factorised once on the host."""
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
            want = (K, d0, d0) if self.covariance_type == 'full' else (d0, d0)
            if p.shape != want:
                raise ValueError("The parameter '%s precision' should have the shape of %s, but got %s" % (self.covariance_type, want, p.shape))
            mats = p.reshape(-1, d0, d0)
            facs = []
            for m in mats:
                if not (np.allclose(m, m.T) and np.all(np.linalg.eigvalsh(m) > 0.0)):
                    raise ValueError("'%s precision' should be symmetric, positive-definite" % self.covariance_type)
                facs.append(_host_factor(m))
            out['prec'] = (np.stack([f[0] for f in facs]), np.array([f[1] for f in facs]))
        return out

    def _draw(self, pts, init_labels):
        """(labels, resp) of the n_init restarts: every random number is drawn here, restart by restart, in sklearn's order (``gmm.py``'s draws)."""
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
            else:          # 'k-means++'
                rows = _pp_init(pts.x.contiguous(), K, 1, rs)[0]
                for k in range(K):
                    if torch.isnan(rows[k]).any():
                        raise ValueError('gmm_full: the points contain NaN')
                    labels[r, int(torch.nonzero((pts.x == rows[k]).all(dim=1))[0])] = k
        return labels, None

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

    def _points(self, X):
        if not hasattr(self, 'weights_'):
            raise RuntimeError('This FullGaussianMixture instance is not fitted yet.')
        if hasattr(X, 'shape') and len(X.shape) == 2 and X.shape[1] != self.n_features_in_:
            raise ValueError('X has %d features, but FullGaussianMixture is expecting %d features as input.' % (X.shape[1], self.n_features_in_))
        return _Points(X, shift=self._shift)

    def _device_parameters(self, pts):
        """The fitted parameters against the training shift, padded; the factor of the kept covariances is the kept one (``precisions_cholesky_``)."""
        K, dev, d0 = self.n_components, pts.x.device, self.n_features_in_
        mu = torch.zeros((K, pts.d), dtype=torch.float64, device=dev)
        mu[:, :d0] = _dev64(self._means_shifted, (K, d0), dev)
        P = _pad_square(self.precisions_cholesky_.reshape(-1, d0, d0), pts.d, dev)
        ld = _dev64(self._log_det, (-1,), dev)
        return _dev64(self.weights_, (K,), dev), mu, P, ld

    # -- estimator API ------------------------------------------------------------------------
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
        self.n_features_in_ = d0
        self._shift = pts.shift_host.copy()
        self._means_shifted = par['mu'][best, :, :d0].cpu().numpy()
        self.weights_ = par['w'][best].cpu().numpy()
        self.means_ = self._means_shifted + self._shift[None, :]
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

    def fit(self, X, y=None):
        return self._fit_points(_Points(X))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def _estep(self, X, **want):
        pts = self._points(X)
        return pts, estep(pts, COV_TYPES[self.covariance_type], *self._device_parameters(pts), **want)

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
        """Renumber the components: new component j is old component ``order[j]``.  Tied covariances are shared and stay."""
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(self.n_components)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (self.n_components - 1, order.tolist()))
        names = ['weights_', 'means_', '_means_shifted']
        if self.covariance_type == 'full':
            names += ['covariances_', 'precisions_', 'precisions_cholesky_', '_log_det']
        for name in names:
            setattr(self, name, getattr(self, name)[order].copy())
        if hasattr(self, 'labels_'):
            inverse = np.empty_like(order)
            inverse[order] = np.arange(len(order))
            self.labels_ = inverse[self.labels_].astype(self.labels_.dtype)
        return self

    def _n_parameters(self):
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    bic = GaussianMixture.bic
    aic = GaussianMixture.aic

    def sample(self, n_samples=1):
        raise NotImplementedError('sample is not implemented: the accelerated path fits and scores; draw from means_ / covariances_ with NumPy')

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, covariance_type=self.covariance_type, tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter,
                    n_init=self.n_init, init_params=self.init_params, weights_init=self.weights_init, means_init=self.means_init,
                    precisions_init=self.precisions_init, random_state=self.random_state)


def gmm_full_sweep(X, ks, **kw):
    """{K: fitted ``FullGaussianMixture(n_components=K, **kw)``} for every K of ``ks``: X is uploaded, padded and shifted once, and for tied covariances the
    total scatter matrix T is formed once, by the first fit."""
    pts = _Points(X)
    fits, total = {}, None
    for k in ks:
        fits[int(k)] = FullGaussianMixture(n_components=int(k), **kw)._fit_points(pts, total=total)
        total = fits[int(k)]._scatter_total
    return fits
