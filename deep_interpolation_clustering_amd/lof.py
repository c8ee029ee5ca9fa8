"""Which encounters belong to no neighbourhood?  The local outlier factor (Breunig, Kriegel, Ng & Sander 2000) of the latents on the MI355X:
``sklearn.neighbors.LocalOutlierFactor`` for the euclidean metric, exact for the f32 coordinates, and for a range of k from ONE neighbour join.

The definition (include/dic_hip.h states it for every layer).  A fit on X (N rows) with ``n_neighbors`` uses k = max(1, min(n_neighbors, N - 1)).
``(dist, idx)``: the k nearest rows of every row sorted by (distance, index), its own index left out by the rule of ``knn.NearestNeighbors.kneighbors(X=None)``
(take k + 1, drop the entry whose index is the row's own, the first column where it is not among them).

    kdist[j] = dist[j, k - 1];   reach(i, s) = max(kdist[idx[i, s]], dist[i, s]);   lrd[i] = 1 / (mean_s reach(i, s) + 1e-10)
    negative_outlier_factor_[i] = -mean_s (lrd[idx[i, s]] / lrd[i])

New rows Q (novelty): ``(dist, idx)`` are their k nearest rows of X, nothing left out; kdist and the neighbours' lrd are the fit's, lrd_q is formed as above,
``score_samples = -mean_s (lrd[idx[q, s]] / lrd_q[q])``.  The first k columns of a (distance, index)-ordered list are the list at k, so several k come from
one join at max(ks): ``lof_sweep``.

The join is ``knn.kneighbors`` (csrc/dic_knn.hip); everything after it stays on the device: the self column is dropped (``tsne.drop_self``) and the
k-distance columns are taken with torch, and csrc/dic_lof.hip (``dic_lof_lrd``, ``dic_lof_scores``) does the two gathers-and-sums, every sum in a fixed order -- two calls give the same
bits and a k of a sweep has the bits of its own call.  Only the (N, nk) results reach the host.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .knn import MAX_NEIGHBORS, _check_k, _shape_of, kneighbors
from .tsne import drop_self

MAX_KS = 64          # csrc/dic_lof.hip: LOF_MAXK, the values of k one call takes


def check_ks(ks):
    """``ks`` (an int or a sequence of ints >= 1) as a list of ints, in the caller's order."""
    if isinstance(ks, (numbers.Integral, np.integer)) and not isinstance(ks, bool):
        ks = (ks,)
    out = []
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
            raise ValueError('n_neighbors must be an integer, got %r' % (k,))
        if k < 1:
            raise ValueError('Expected n_neighbors > 0. Got %d' % k)
        out.append(int(k))
    if not out:
        raise ValueError('ks must name at least one n_neighbors')
    return out


def _ks_array(ks):
    ks = check_ks(ks)
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError('ks must be strictly ascending, got %r' % (ks,))
    if len(ks) > MAX_KS:
        raise NotImplementedError('lof_from_lists: at most %d values of k per call (got %d)' % (MAX_KS, len(ks)))
    return ks, (N.C.c_int * len(ks))(*ks)


def _table(t, what, rows, nk, device):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != (rows, nk):
        raise ValueError('%s must be a float64 tensor of shape (%d, %d), got %s' % (
            what, rows, nk, '%s %s' % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    if t.device != device:
        raise ValueError('%s is on %s, the lists are on %s' % (what, t.device, device))
    return t.contiguous()


def lof_from_lists(dist, idx, ks, n_fit=None, fit=None, out=None):
    """``(nof, lrd, kdist)``, each an (M, nk) float64 device tensor whose column t belongs to ``ks[t]``: the device-level combination of the definition
    (module docstring) on lists that are already on the device.

    ``dist`` (M, W) float64 and ``idx`` (M, W) integer tensors on the GPU: per row the W nearest rows of the fitted set sorted by (distance, index);
    ``ks``: strictly ascending, at most 64 values, max(ks) <= W (wider lists are read up to each k only).  Without ``fit`` the lists are the self-excluded
    ones of the fitted set itself (M = ``n_fit``, which may be left out) and the result is the fit: ``nof`` is ``negative_outlier_factor_``.  With
    ``fit=(lrd_fit, kdist_fit)``, the (n, nk) tables of a fit at the same ``ks``, the rows are new points and ``nof`` is ``score_samples``; ``lrd`` and
    ``kdist`` are then the new rows' own.  ``out``: an (M, nk) float64 tensor to receive ``nof``.  Every bad input -- indices that are no integers or lie
    outside [0, n), shapes that disagree, a k beyond the lists -- raises ValueError before anything is launched or written."""
    if not (torch.is_tensor(dist) and torch.is_tensor(idx)):
        raise ValueError('dist and idx must be torch tensors on the GPU, got %s and %s' % (type(dist).__name__, type(idx).__name__))
    if idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
        raise ValueError('idx must be integers, got %s' % (idx.dtype,))
    if dist.dim() != 2 or tuple(dist.shape) != tuple(idx.shape):
        raise ValueError('dist and idx must be (n_rows, width) both, got %s and %s' % (tuple(dist.shape), tuple(idx.shape)))
    if dist.dtype != torch.float64:
        raise ValueError('dist must be float64, got %s' % (dist.dtype,))
    ks, ks_c = _ks_array(ks)
    m, width = dist.shape
    nk = len(ks)
    if m < 1 or width < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (m, width))
    if ks[-1] > width:
        raise ValueError('the lists hold %d neighbours, n_neighbors = %d needs as many' % (width, ks[-1]))
    N.require_gpu(dist, idx)
    if idx.device != dist.device:
        raise ValueError('idx is on %s, dist is on %s' % (idx.device, dist.device))
    if fit is None:
        n = m if n_fit is None else int(n_fit)
        if n != m:
            raise ValueError('Found input variables with inconsistent numbers of samples: [%d, %d]' % (n, m))
    else:
        lrd_fit, kdist_fit = fit
        if not torch.is_tensor(lrd_fit) or lrd_fit.dim() != 2:
            raise ValueError('fit must be (lrd_fit, kdist_fit), two (n_fit, nk) float64 tensors')
        n = int(lrd_fit.shape[0])
        if n_fit is not None and int(n_fit) != n:
            raise ValueError('Found input variables with inconsistent numbers of samples: [%d, %d]' % (int(n_fit), n))
        lrd_fit = _table(lrd_fit, 'lrd_fit', n, nk, dist.device)
        kdist_fit = _table(kdist_fit, 'kdist_fit', n, nk, dist.device)
    if out is not None:
        if not (torch.is_tensor(out) and out.is_contiguous()):
            raise ValueError('out must be a contiguous tensor')
        out = _table(out, 'out', m, nk, dist.device)
    lo, hi = int(idx.min()), int(idx.max())          # on the device: an index outside the fitted set would be a wild read
    if lo < 0 or hi >= n:
        raise ValueError('idx must lie in [0, n_samples_fit = %d), got %d' % (n, lo if lo < 0 else hi))
    dist, idx = dist.contiguous(), idx.to(torch.int32).contiguous()
    cols = torch.as_tensor([k - 1 for k in ks], dtype=torch.int64, device=dist.device)
    kdist = dist.index_select(1, cols).contiguous()
    lrd = torch.empty((m, nk), dtype=torch.float64, device=dist.device)
    nof = torch.empty((m, nk), dtype=torch.float64, device=dist.device) if out is None else out
    L = N.lib()
    st = N.stream_of(dist)
    N.check(L.dic_lof_lrd(N.ptr(dist), N.ptr(idx), m, width, N.ptr(kdist if fit is None else kdist_fit), n, ks_c, nk, N.ptr(lrd), st), 'dic_lof_lrd')
    N.check(L.dic_lof_scores(N.ptr(idx), m, width, N.ptr(lrd if fit is None else lrd_fit), n, N.ptr(lrd), ks_c, nk, N.ptr(nof), st), 'dic_lof_scores')
    return nof, lrd, kdist


def _check_points(X, what):
    n, d = _shape_of(X)
    if n < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (n, d))
    if d > MAX_DIM:
        raise NotImplementedError('%s: at most %d features (got %d)' % (what, MAX_DIM, d))
    return n, d


def _fit_lists(X, ks, candidate_budget=None):
    """The fit at the ascending distinct ``ks``: one self join at max(ks) + 1, the self column dropped on the device, then the two kernels."""
    dist, idx = kneighbors(X, ks[-1] + 1, candidate_budget=candidate_budget, return_device=True)
    dist, idx = drop_self(dist, idx)
    return lof_from_lists(dist, idx, ks)


def lof_sweep(X, ks, candidate_budget=None, return_device=False):
    """``nof (nk, N)`` float64: row t is ``LocalOutlierFactor(n_neighbors=ks[t]).fit(X).negative_outlier_factor_`` (module docstring), for all of ``ks``
    from ONE self join at max(ks) + 1 -- every row has the bits of its own call.  ``X`` (N, D): a numpy array or tensor, D <= 256; every k of ``ks`` (any
    order, at most 64 distinct values) below N and <= 1023, for the join takes k + 1 <= 1024.  No clamping here: a k >= N is refused as sklearn's
    ``kneighbors`` refuses it.  A numpy array, or a device tensor with ``return_device=True``."""
    n, d = _check_points(X, 'lof_sweep')
    ks = check_ks(ks)
    order = sorted(set(ks))
    if order[-1] + 1 > MAX_NEIGHBORS:
        raise NotImplementedError('lof_sweep: at most %d neighbours (got %d)' % (MAX_NEIGHBORS - 1, order[-1]))
    if len(order) > MAX_KS:
        raise NotImplementedError('lof_sweep: at most %d values of k per call (got %d)' % (MAX_KS, len(order)))
    _check_k(order[-1] + 1, n, n, query_is_train=True)
    nof = _fit_lists(X, order, candidate_budget)[0]
    nof = nof[:, [order.index(k) for k in ks]].t().contiguous()
    return nof if return_device else nof.cpu().numpy()


def check_contamination(contamination):
    """sklearn's refusal (utils/_param_validation.py) of a contamination that is neither 'auto' nor a float in (0, 0.5]."""
    if isinstance(contamination, str) and contamination == 'auto':
        return contamination
    if isinstance(contamination, float) and 0.0 < contamination <= 0.5:
        return contamination
    raise ValueError("The 'contamination' parameter of LocalOutlierFactor must be a str among {'auto'} or a float in the range (0.0, 0.5]. "
                     "Got %r instead." % (contamination,))


def offset_of(nof, contamination):
    """``offset_``: -1.5 for 'auto', else the 100 contamination-th percentile of ``nof`` (numpy's default, linear interpolation)."""
    return -1.5 if contamination == 'auto' else float(np.percentile(nof, 100.0 * contamination))


class LocalOutlierFactor:
    """``sklearn.neighbors.LocalOutlierFactor(n_neighbors, contamination=, novelty=)`` for the euclidean metric (module docstring): ``fit``, ``fit_predict``
    (``novelty=False``), ``score_samples`` / ``decision_function`` / ``predict`` (``novelty=True``), ``negative_outlier_factor_``, ``n_neighbors_``,
    ``offset_``; labels are +1 (inlier) and -1 (outlier)."""

    def __init__(self, n_neighbors=20, contamination='auto', novelty=False):
        self.n_neighbors = n_neighbors
        self.contamination = contamination
        self.novelty = novelty

    def fit(self, X, y=None):
        check_contamination(self.contamination)
        if isinstance(self.n_neighbors, bool) or not isinstance(self.n_neighbors, (numbers.Integral, np.integer)) or self.n_neighbors < 1:
            raise ValueError("The 'n_neighbors' parameter of LocalOutlierFactor must be an int in the range [1, inf) or None. Got %r instead." % (
                self.n_neighbors,))
        n, d = _check_points(X, 'LocalOutlierFactor')
        if n < 2:
            raise ValueError('Expected n_neighbors < n_samples_fit, but n_neighbors = 1, n_samples_fit = %d, n_samples = %d' % (n, n))
        if self.n_neighbors >= n:          # (sklearn is silent at n_neighbors == n_samples, where it clamps too; here every clamp warns)
            warnings.warn('n_neighbors (%s) is %s the total number of samples (%s). n_neighbors will be set to (n_samples - 1) for estimation.'
                          % (self.n_neighbors, 'greater than' if self.n_neighbors > n else 'equal to', n))
        k = max(1, min(int(self.n_neighbors), n - 1))
        if k + 1 > MAX_NEIGHBORS:
            raise NotImplementedError('LocalOutlierFactor: at most %d neighbours (got %d)' % (MAX_NEIGHBORS - 1, k))
        self._fit_X = X
        self.n_samples_fit_, self.n_features_in_, self.n_neighbors_ = n, d, k
        nof, self._lrd, self._kdist = _fit_lists(X, [k])
        self.negative_outlier_factor_ = nof[:, 0].cpu().numpy()
        self.offset_ = offset_of(self.negative_outlier_factor_, self.contamination)
        if np.min(self.negative_outlier_factor_) < -1e7 and not self.novelty:
            warnings.warn('Duplicate values are leading to incorrect results. Increase the number of neighbors for more accurate results.')
        return self

    def _fitted(self):
        if not hasattr(self, 'negative_outlier_factor_'):
            raise RuntimeError("This LocalOutlierFactor instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")

    def fit_predict(self, X, y=None):
        if self.novelty:
            raise AttributeError('fit_predict is not available when novelty=True. Use novelty=False if you want to predict on the training set.')
        self.fit(X)
        labels = np.ones(self.n_samples_fit_, dtype=int)
        labels[self.negative_outlier_factor_ < self.offset_] = -1
        return labels

    def score_samples(self, X):
        if not self.novelty:
            raise AttributeError('score_samples is not available when novelty=False. The scores of the training samples are always available through the '
                                 'negative_outlier_factor_ attribute. Use novelty=True if you want to use LOF for novelty detection and compute '
                                 'score_samples for new unseen data.')
        self._fitted()
        m, d = _shape_of(X)
        if d != self.n_features_in_:
            raise ValueError('X has %d features, but LocalOutlierFactor is expecting %d features as input.' % (d, self.n_features_in_))
        if m < 1:
            raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (m, d))
        dist, idx = kneighbors(self._fit_X, self.n_neighbors_, Q=X, return_device=True)
        return lof_from_lists(dist, idx, [self.n_neighbors_], fit=(self._lrd, self._kdist))[0][:, 0].cpu().numpy()

    def decision_function(self, X):
        if not self.novelty:
            raise AttributeError('decision_function is not available when novelty=False. Use novelty=True if you want to use LOF for novelty detection and '
                                 'compute decision_function for new unseen data. Note that the opposite LOF of the training samples is always available by '
                                 'considering the negative_outlier_factor_ attribute.')
        return self.score_samples(X) - self.offset_

    def predict(self, X=None):
        if not self.novelty:
            raise AttributeError('predict is not available when novelty=False, use fit_predict if you want to predict on training data. Use novelty=True if '
                                 'you want to use LOF for novelty detection and predict on new unseen data.')
        self._fitted()
        if X is None:
            below = self.negative_outlier_factor_ < self.offset_
        else:
            below = self.decision_function(X) < 0
        labels = np.ones(below.shape[0], dtype=int)
        labels[below] = -1
        return labels


class LofSweep:
    """A fit of one cohort at several k (one self join) that scores other cohorts as new points (one query join each): what p4 --outlier lof runs.
    ``ks`` in any order; the columns of every result follow it.  ``nof`` (N, nk) is the fit's ``negative_outlier_factor_`` per k, ``offsets`` (nk) its
    ``offset_`` per k at ``contamination``."""

    def __init__(self, X, ks, contamination='auto', candidate_budget=None):
        check_contamination(contamination)
        n, self._d = _check_points(X, 'LofSweep')
        self.ks = check_ks(ks)
        self._order = sorted(set(self.ks))
        self._cols = [self._order.index(k) for k in self.ks]
        if self._order[-1] + 1 > MAX_NEIGHBORS:
            raise NotImplementedError('LofSweep: at most %d neighbours (got %d)' % (MAX_NEIGHBORS - 1, self._order[-1]))
        if len(self._order) > MAX_KS:
            raise NotImplementedError('LofSweep: at most %d values of k per call (got %d)' % (MAX_KS, len(self._order)))
        _check_k(self._order[-1] + 1, n, n, query_is_train=True)
        self._X, self._budget = X, candidate_budget
        nof, self._lrd, self._kdist = _fit_lists(X, self._order, candidate_budget)
        self.nof = nof[:, self._cols].cpu().numpy()
        self.offsets = np.array([offset_of(self.nof[:, t], contamination) for t in range(len(self.ks))], dtype=np.float64)

    def score_samples(self, Q):
        """``score_samples`` (M, nk) of the new rows ``Q`` against the fitted cohort, per k."""
        m, d = _shape_of(Q)
        if d != self._d:
            raise ValueError('X has %d features, but LocalOutlierFactor is expecting %d features as input.' % (d, self._d))
        dist, idx = kneighbors(self._X, self._order[-1], Q=Q, candidate_budget=self._budget, return_device=True)
        return lof_from_lists(dist, idx, self._order, fit=(self._lrd, self._kdist))[0][:, self._cols].cpu().numpy()
