"""``FuzzyCMeans`` (Bezdek's fuzzy c-means) on the MI355X (csrc/dic_fcm.hip): the p2 / p4 ``--cluster_method fcm`` branches.

The Gaussian mixtures are the other soft assignments of the post-hoc side, and in 256 dimensions their posteriors saturate to 0 / 1.  The memberships here
are a function of distance RATIOS only -- u_ik = 1 / sum_j (d_ik / d_jk)^(2 / (m - 1)), the counterpart of DEC's ``q`` -- with one knob for their softness, the
fuzzifier ``m`` > 1 (m -> 1: k-means; m = 2: the textbook default).  There are centres, so p4 applies the training fit to the other cohorts unchanged, and
the fuzzy validity indices (partition coefficient, partition entropy, Xie-Beni) give a criterion for K that needs no likelihood.

The arithmetic is the f64 definition at the head of csrc/dic_fcm.hip: one iteration is one pass over the f32 points and a fixed-order reduction, so two
fits give the same bits.  The points, the restarts-together loop, the status block and the workspace are ``_gmm_base.py``'s (``_Points``, ``run_em``,
``new_status``, ``workspace``).  The iterations consume no randomness, so the ``n_init`` initialisations are drawn first, restart by restart, from one
stream; the smallest final J wins, the first of equal ones.

IN HIGH DIMENSIONS FCM COLLAPSES: all centres run to the centre of gravity and every membership becomes 1 / K (at m = 2 on 256-dimensional blobs within five
iterations).  A fit says so: ``coincident_centers_`` lists the pairs of centres closer than 0.01 x the RMS distance of the points from their mean -- a fixed
rule -- and a non-empty list raises a ``UserWarning`` that advises a smaller ``m``.

Outputs are NumPy f64.  The module imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import math
import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from . import cluster_stats
from ._gmm_base import _dev64, _Points, new_status, run_em, workspace
from .kmeans import KMeans, _pp_init

COINCIDENT_FRACTION = 0.01      # of the RMS distance of the points from their mean: centres closer than that are one centre
INITS = ('k-means++', 'kmeans', 'random')
_NEEDS = ('fuzzy c-means of {n} points needs {nbytes} bytes on the device, {free} are free: the f64 partial sums of at most 256 workgroups, '
          '8 (K D + K + 3) bytes each (K = {k}, D = {d}), per restart ({runs})')


def _workspace(pts, K, n_runs):
    return workspace(pts, K, n_runs, N.lib().dic_fcm_workspace, 'fcm', _NEEDS)


def rms_radius(pts):
    """sqrt(mean_i |x_i - c|^2), c the column means: the scale ``coincident_centers_`` is judged against.  Formed once per point set and kept on it."""
    if getattr(pts, '_rms_radius', None) is None:
        xs = pts.x.double() - pts.shift[None, :]
        pts._rms_radius = math.sqrt(float((xs * xs).sum()) / pts.n)
    return pts._rms_radius


def shifted_centers(pts, centers):
    """Centres ((.., K, D0), a NumPy array or a device tensor, any float type) as the kernels take them: f64 on the device, minus the shift -- the same
    rounded subtraction a point goes through, so a centre that IS a point has distance 0 to it -- and zero in the padding."""
    dev = pts.x.device
    c = centers.detach().to(device=dev, dtype=torch.float64) if torch.is_tensor(centers) else torch.as_tensor(np.asarray(centers, dtype=np.float64), device=dev)
    out = torch.zeros(tuple(c.shape[:-1]) + (pts.d,), dtype=torch.float64, device=dev)
    out[..., :pts.d0] = c[..., :pts.d0] - pts.shift[:pts.d0]
    return out.contiguous()


def iterate(pts, m, centers, tol, max_iter, ws=None):
    """Fuzzy c-means on every restart of ``centers`` ((n_runs, K, D) f64 on the device, shifted; updated in place) until each is done.  Returns what
    ``_gmm_base.run_em`` returns: (status (n_runs, 8), the J history (n_runs, max_iter), NaN beyond a restart's iterations)."""
    L = N.lib()
    n_runs, K = centers.shape[0], centers.shape[1]
    status = new_status(n_runs, tol, max_iter, pts.x.device)
    ws = _workspace(pts, K, n_runs) if ws is None else ws
    st = N.stream_of(pts.x)

    def step(objs):
        N.check(L.dic_fcm_iter(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, K, n_runs, float(m), N.ptr(pts.shift), N.ptr(centers), N.ptr(status), N.ptr(objs),
                               max_iter, N.ptr(ws), ws.numel(), st), 'dic_fcm_iter')
    return run_em(step, status, max_iter)


def memberships(pts, m, centers, u=False, labels=False, d2=False, sums=False, ws=None):
    """One centre set ((K, D) f64 on the device, shifted) against the points.  Returns a dict of the requested outputs, on the device: ``u`` (N, K) f64,
    ``labels`` (N) int32 (the first maximum), ``d2`` (N, K) f64, ``sums`` (3) f64 = J, S2, SE."""
    K, dev = centers.shape[0], pts.x.device
    out = {}
    if u:
        out['u'] = torch.empty((pts.n, K), dtype=torch.float64, device=dev)
    if labels:
        out['labels'] = torch.empty(pts.n, dtype=torch.int32, device=dev)
    if d2:
        out['d2'] = torch.empty((pts.n, K), dtype=torch.float64, device=dev)
    if sums:
        out['sums'] = torch.empty(3, dtype=torch.float64, device=dev)
    ws = _workspace(pts, K, 1) if ws is None else ws
    N.check(N.lib().dic_fcm_memberships(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, K, float(m), N.ptr(pts.shift), N.ptr(centers), N.ptr(out.get('u')),
                                        N.ptr(out.get('labels')), N.ptr(out.get('d2')), N.ptr(out.get('sums')), N.ptr(ws), ws.numel(), N.stream_of(pts.x)),
            'dic_fcm_memberships')
    return out


def _positive_int(name, value):
    if isinstance(value, bool) or not isinstance(value, (numbers.Integral, np.integer)) or value < 1:
        raise ValueError('%s must be an int >= 1, got %r' % (name, value))
    return int(value)


class FuzzyCMeans:
    """Fuzzy c-means of ``n_clusters`` (2 .. 32) centres with the fuzzifier ``m`` > 1.  ``X``: a NumPy array or a device tensor, (N, D), D <= 256.  A restart
    stops after iteration t >= 2 when |J_(t-1) - J_t| <= tol J_(t-1) (``converged_``) or at ``max_iter``.  ``init``: 'k-means++' (the rows
    ``kmeans._pp_init`` chooses), 'kmeans' (the centres of one ``KMeans(n_init=1)`` fit per restart), 'random' (K distinct rows) or a (K, D) array (one
    restart).  ``centers_init`` (n_init, K, D) replaces the draws by given centres.

    After ``fit``: ``cluster_centers_`` (K, D), ``labels_`` (N) int32, the first largest membership, ``objectives_`` (J of every iteration, each from the
    centres that entered it), ``objective_`` (its last entry), ``n_iter_``, ``converged_``; and from one more pass with the KEPT centres
    ``partition_coefficient_`` = sum u^2 / N, ``partition_entropy_`` = -sum u log u / N, ``modified_partition_coefficient_`` = (K PC - 1) / (K - 1) and
    ``xie_beni_`` = J / (N min_{j != k} |v_j - v_k|^2), inf when two centres are equal; ``center_separation_`` (K, K), the distances between the centres,
    and ``coincident_centers_``, the pairs (j, k), j < k, closer than 0.01 x the RMS distance of the points from their mean -- a collapsed fit."""

    def __init__(self, n_clusters, m=2.0, tol=1e-6, max_iter=300, n_init=1, init='k-means++', random_state=None, *, centers_init=None):
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, (numbers.Integral, np.integer)) or n_clusters < 2:
            raise ValueError('n_clusters must be an int >= 2, got %r' % (n_clusters,))
        if n_clusters > N.MAX_CLUSTERS:
            raise ValueError('n_clusters=%d > %d: outside the compiled limit' % (n_clusters, N.MAX_CLUSTERS))
        if isinstance(m, bool) or not isinstance(m, (numbers.Real, np.floating, np.integer)) or not (m > 1 and math.isfinite(m)):
            raise ValueError('m (the fuzzifier) must be a finite number > 1, got %r' % (m,))
        if not tol >= 0:
            raise ValueError('tol must be >= 0, got %r' % (tol,))
        if isinstance(init, str) and init not in INITS:
            raise ValueError("init must be 'k-means++', 'kmeans', 'random' or a (n_clusters, n_features) array, got %r" % (init,))
        self.n_clusters = int(n_clusters)
        self.m = float(m)
        self.tol = float(tol)
        self.max_iter = _positive_int('max_iter', max_iter)
        self.n_init = _positive_int('n_init', n_init)
        self.init = init
        self.random_state = random_state
        self.centers_init = centers_init

    _random_state = KMeans._random_state

    # -- fitting ----------------------------------------------------------------------------------
    def _draw(self, pts):
        """The initial centres of the restarts, (n_runs, K, D) f64 on the device, shifted.  Every random number is drawn here, restart by restart."""
        K, d0 = self.n_clusters, pts.d0
        if self.centers_init is not None:
            c = self.centers_init if torch.is_tensor(self.centers_init) else np.asarray(self.centers_init, dtype=np.float64)
            if tuple(c.shape) != (self.n_init, K, d0):
                raise ValueError('centers_init should have the shape (%d, %d, %d), but got %s' % (self.n_init, K, d0, tuple(c.shape)))
            return shifted_centers(pts, c)
        if not isinstance(self.init, str):
            c = self.init if torch.is_tensor(self.init) else np.asarray(self.init, dtype=np.float64)
            if tuple(c.shape) != (K, d0):
                raise ValueError('init should have the shape (%d, %d), but got %s' % (K, d0, tuple(c.shape)))
            return shifted_centers(pts, c[None])          # (given centres: one restart, as KMeans)
        rs = self._random_state()
        if self.init == 'k-means++':
            return shifted_centers(pts, _pp_init(pts.x.contiguous(), K, self.n_init, rs))          # (the k-means kernels take packed rows)
        if self.init == 'kmeans':
            return shifted_centers(pts, np.stack([np.asarray(KMeans(n_clusters=K, n_init=1, random_state=rs).fit(pts.x[:, :d0]).cluster_centers_,
                                                             dtype=np.float64) for _ in range(self.n_init)]))
        idx = np.stack([rs.choice(pts.n, size=K, replace=False) for _ in range(self.n_init)])
        return shifted_centers(pts, pts.x[torch.as_tensor(idx, device=pts.x.device)])

    def _fit_points(self, pts):
        K = self.n_clusters
        if pts.n < K:
            raise ValueError('Expected n_samples >= n_clusters but got n_clusters = %d, n_samples = %d' % (K, pts.n))
        centers = self._draw(pts)
        n_runs = centers.shape[0]
        ws = _workspace(pts, K, n_runs)
        self._initial_centers = centers[:, :, :pts.d0].cpu().numpy()
        status, objs = iterate(pts, self.m, centers, self.tol, self.max_iter, ws=ws)
        self._status, self._all_objectives = status, objs
        self._all_centers = centers[:, :, :pts.d0].cpu().numpy()
        best, least = 0, np.inf
        for r in range(n_runs):          # the first of equal objectives wins
            if status[r, 3] < least:
                best, least = r, status[r, 3]
        self.converged_ = bool(status[best, 2] != 0)
        self.n_iter_ = int(status[best, 1])
        self.objectives_ = objs[best, :self.n_iter_].copy()
        self.objective_ = float(status[best, 3])
        self.n_features_in_ = pts.d0
        self._shift = pts.shift_host.copy()
        self._centers_shifted = self._all_centers[best].copy()
        self.cluster_centers_ = self._centers_shifted + self._shift[None, :]
        # one more pass: the labels and the indices of the kept centres
        out = memberships(pts, self.m, centers[best].contiguous(), labels=True, sums=True, ws=ws)
        self.labels_ = out['labels'].cpu().numpy()
        J, S2, SE = (float(v) for v in out['sums'].cpu().numpy())
        self._final_sums = (J, S2, SE)
        self.partition_coefficient_ = S2 / pts.n
        self.partition_entropy_ = -SE / pts.n
        self.modified_partition_coefficient_ = (K * self.partition_coefficient_ - 1.0) / (K - 1.0)
        diff = self._centers_shifted[:, None, :] - self._centers_shifted[None, :, :]
        self.center_separation_ = np.sqrt((diff * diff).sum(axis=2))
        off = self.center_separation_[~np.eye(K, dtype=bool)]
        closest = float(off.min())
        self.xie_beni_ = J / (pts.n * closest * closest) if closest > 0 else float('inf')
        limit = COINCIDENT_FRACTION * rms_radius(pts)
        self.coincident_centers_ = [(j, k) for j in range(K) for k in range(j + 1, K) if self.center_separation_[j, k] < limit]
        if self.coincident_centers_:
            warnings.warn('fuzzy c-means with m = %g collapsed: the centres of the pairs %s are closer than %g x the RMS distance of the points from their mean '
                          '(%g), so these clusters are one and their memberships equal.  In high dimensions the distance ratios approach 1: choose a '
                          'smaller m (closer to 1).' % (self.m, self.coincident_centers_, COINCIDENT_FRACTION, limit / COINCIDENT_FRACTION), UserWarning)
        return self

    def fit(self, X, y=None):
        return self._fit_points(_Points(X))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    # -- the fitted model against other points ------------------------------------------------------
    def _points(self, X):
        if not hasattr(self, 'cluster_centers_'):
            raise RuntimeError('This %s instance is not fitted yet.' % type(self).__name__)
        if hasattr(X, 'shape') and len(X.shape) == 2 and X.shape[1] != self.n_features_in_:
            raise ValueError('X has %d features, but %s is expecting %d features as input.' % (X.shape[1], type(self).__name__, self.n_features_in_))
        return _Points(X, shift=self._shift)

    def _memberships(self, X, **want):
        pts = self._points(X)
        centers = torch.zeros((self.n_clusters, pts.d), dtype=torch.float64, device=pts.x.device)
        centers[:, :pts.d0] = _dev64(self._centers_shifted, (self.n_clusters, pts.d0), pts.x.device)
        return pts, memberships(pts, self.m, centers.contiguous(), **want)

    def predict(self, X):
        """(N,) int32 numpy: the centre of largest membership (the first of equal ones)."""
        return self._memberships(X, labels=True)[1]['labels'].cpu().numpy()

    def predict_proba(self, X):
        """(N, K) f64 numpy: the memberships; every row sums to 1."""
        return self._memberships(X, u=True)[1]['u'].cpu().numpy()

    memberships = predict_proba

    def transform(self, X):
        """(N, K) f64 numpy: the distances to the centres."""
        return torch.sqrt(self._memberships(X, d2=True)[1]['d2']).cpu().numpy()

    def fuzzy_silhouette(self, X, alpha=1.0):
        """Campello and Hruschka's fuzzy silhouette: the mean of ``cluster_stats.silhouette_samples`` of the hard labels, every point weighted by
        (its largest membership - its second largest)^alpha.  NaN where the hard labels have fewer than two clusters or every weight is 0."""
        pts, out = self._memberships(X, u=True, labels=True)
        labels = np.unique(out['labels'].cpu().numpy(), return_inverse=True)[1].astype(np.int64)          # (a centre without a point is skipped)
        if labels.max() < 1:
            return float('nan')
        top = torch.topk(out['u'], 2, dim=1).values
        weight = (top[:, 0] - top[:, 1]) ** float(alpha)
        s = cluster_stats.silhouette_samples(pts.x[:, :pts.d0], labels).double()
        total = float(weight.sum())
        return float((weight * s).sum()) / total if total > 0 else float('nan')

    def reorder(self, order):
        """Renumber the clusters: new cluster j is old cluster ``order[j]`` (p4 orders them by systolic pressure)."""
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(self.n_clusters)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (self.n_clusters - 1, order.tolist()))
        inverse = np.empty_like(order)
        inverse[order] = np.arange(len(order))
        for name in ('cluster_centers_', '_centers_shifted'):
            setattr(self, name, getattr(self, name)[order].copy())
        self.center_separation_ = self.center_separation_[np.ix_(order, order)].copy()
        self.coincident_centers_ = sorted(tuple(sorted((int(inverse[j]), int(inverse[k])))) for j, k in self.coincident_centers_)
        self.labels_ = inverse[self.labels_].astype(self.labels_.dtype)
        return self

    def get_params(self, deep=True):
        return dict(n_clusters=self.n_clusters, m=self.m, tol=self.tol, max_iter=self.max_iter, n_init=self.n_init, init=self.init,
                    random_state=self.random_state)


def fcm_sweep(X, ks, m=2.0, **kw):
    """{K: fitted ``FuzzyCMeans(K, m=m, **kw)``} for every K of ``ks``: X is uploaded, padded and shifted once, and its RMS radius is formed once."""
    pts = _Points(X)
    return {int(k): FuzzyCMeans(int(k), m=m, **kw)._fit_points(pts) for k in ks}
