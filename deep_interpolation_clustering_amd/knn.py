"""k-th neighbour distances on the MI355X without the distance matrix, and the k-distance elbow p2 chooses DBSCAN's eps with (p2_clustering_optK.py:102-120).

Upstream: ``NearestNeighbors(n_neighbors=k, n_jobs=5).fit(X).kneighbors(X)[0][:, -1]`` -- a brute-force all-pairs pass on the CPU -- sorted, and the knee of
that curve from ``kneed.KneeLocator(point_num, sorted_dist, S=1.0, curve='convex', direction='increasing')``.  Here the distances come from
csrc/dic_knn.hip: counting passes of the DBSCAN tile machine with per-row thresholds narrow every row's k-th distance to a short candidate list, and the
value at the exact rank is taken from f64 difference-form distances of the candidates.  The convention is upstream's: the point itself is its own first
neighbour (k = 1 gives 0, duplicates give zeros).  The same quantity is OPTICS' core distance (``core_distances``): optics.py builds on it.

Neighbour LISTS come from the same file (``dic_knn_neighbors``): ``kneighbors`` gives, for every query, its k nearest index points sorted by (distance, index),
of a set against itself or of a query set against an index set; ``NearestNeighbors`` wraps it in sklearn's interface (``kneighbors``, ``kneighbors_graph`` as
CSR triples), and ``knn_transfer_labels`` is the uniform vote of ``KNeighborsClassifier`` -- the out-of-sample labels p4 gives DBSCAN and HDBSCAN with
``--transfer knn``.

Neighbour RANKS come from csrc/dic_knn_rank.hip (``dic_knn_ranks``): ``neighbor_ranks`` says where given points stand among a row's neighbours, the quantity
trustworthiness and continuity (embedding_quality.py) are sums of.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM, _device_points

STAT_NAMES = ('passes', 'groups', 'max_list', 'candidates', 'budget_needed')


class CandidateBudgetError(RuntimeError):
    """One row's candidate list alone exceeds ``candidate_budget``; ``needed`` is the budget (bytes) that holds it."""

    def __init__(self, message, needed):
        super().__init__(message)
        self.needed = int(needed)


def _shape_of(X):
    shape = tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (shape,))
    return shape


def _candidate_call(front, entry, candidate_budget, stats, run):
    """What the three front ends of the candidate-list entry points end with: ``candidate_budget`` parsed (None: the library's default), ``run(budget, st)``
    -- the caller's remaining checks, its allocations and its call of ``entry`` with the stats words ``st`` -- giving ``(rc, result)``; then ``stats``
    filled, a list longer than the budget raised as ``CandidateBudgetError`` and any other failure through ``N.check``."""
    budget = 0 if candidate_budget is None else int(candidate_budget)
    if candidate_budget is not None and budget < 1:
        raise ValueError('candidate_budget must be positive, got %r' % (candidate_budget,))
    st = (N.C.c_int64 * len(STAT_NAMES))()
    rc, result = run(budget, st)
    if stats is not None:
        stats.update(zip(STAT_NAMES, (int(v) for v in st)))
    if rc == -3 and st[4] > 0:          # DIC_ERR_WORKSPACE: one list alone is longer than the budget
        raise CandidateBudgetError('%s: %s' % (front, N.lib().dic_last_error_string().decode()), st[4])
    N.check(rc, entry)
    return result


def kth_neighbor_distance(X, k, candidate_budget=None, stats=None):
    """(N,) float64 numpy: for every row of ``X`` (numpy array or tensor, (N, D), D <= 256) the k-th smallest euclidean distance to the rows of ``X``, itself
    included -- ``NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0][:, -1]``, but exact for the f32 coordinates (f64 difference form).
    ``candidate_budget``: bytes of candidate-list storage (default 384 MiB); it sizes the row groups of the last phase, never the result.  ``stats`` (a dict,
    optional) receives ``passes``, ``groups``, ``max_list``, ``candidates`` and ``budget_needed``."""
    n, _ = _shape_of(X)
    k = int(k)
    if k < 1:
        raise ValueError('Expected n_neighbors > 0. Got %d' % k)
    if k > n:
        raise ValueError('Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d' % (k, n))

    def run(budget, st):
        x = _device_points(X)
        d = x.shape[1]
        if d > MAX_DIM:
            raise NotImplementedError('kth_neighbor_distance: at most %d features (got %d)' % (MAX_DIM, d))
        L = N.lib()
        ws = torch.empty(max(16, L.dic_knn_workspace(n, d, budget)), dtype=torch.uint8, device=x.device)
        out = torch.empty(n, dtype=torch.float64, device=x.device)
        centre = x.mean(0, keepdim=True, dtype=torch.float64).float().contiguous()
        return L.dic_knn_kth_distance(N.ptr(x), x.stride(0), N.ptr(centre), n, d, k, N.ptr(out), budget, st, N.ptr(ws), ws.numel(), N.stream_of(x)), out

    return _candidate_call('kth_neighbor_distance', 'dic_knn_kth_distance', candidate_budget, stats, run).cpu().numpy()


MAX_NEIGHBORS = 1024          # csrc/dic_knn.hip: KN_MAXK, the rows the exact stage sorts in LDS


def _check_k(k, n_fit, n_queries, query_is_train=False):
    """sklearn's wording (neighbors/_base.py, KNeighborsMixin.kneighbors); ``k`` already counts the extra neighbour of ``query_is_train``."""
    if k - int(query_is_train) <= 0:
        raise ValueError('Expected n_neighbors > 0. Got %d' % (k - int(query_is_train)))
    if k > n_fit:
        raise ValueError('Expected %s, but n_neighbors = %d, n_samples_fit = %d, n_samples = %d' % (
            'n_neighbors < n_samples_fit' if query_is_train else 'n_neighbors <= n_samples_fit', k - int(query_is_train), n_fit, n_queries))
    if k > MAX_NEIGHBORS:
        raise NotImplementedError('kneighbors: at most %d neighbours (got %d)' % (MAX_NEIGHBORS, k))


def kneighbors(X, k, Q=None, candidate_budget=None, stats=None, return_device=False):
    """``(dist (M, k) float64, idx (M, k) int32)``: for every row of ``Q`` (every row of ``X`` when ``Q`` is None: the self join, the row itself included
    as an ordinary neighbour at distance 0) the k rows of ``X`` with the smallest (distance, index), in that order --
    ``NearestNeighbors(n_neighbors=k, algorithm='brute').fit(X).kneighbors(Q)``, but exact for the f32 coordinates (f64 difference form) and with ties in
    distance settled by the smaller index.  ``X`` (N, D) and ``Q`` (M, D): numpy arrays or tensors, D <= 256, k <= min(N, 1024).  numpy results, or device
    tensors with ``return_device=True``.  ``candidate_budget`` and ``stats`` as for ``kth_neighbor_distance``: the budget never changes the result.  The
    approximate products that narrow the search are centred on the mean of ``X``: queries far from the index points get longer candidate lists -- the same
    result, but a distant query cohort may need a larger ``candidate_budget`` (``CandidateBudgetError.needed`` says how large)."""
    n, dx = _shape_of(X)
    m = n
    if Q is not None:
        m, dq = _shape_of(Q)
        if dq != dx:
            raise ValueError('X has %d features, but NearestNeighbors is expecting %d features as input.' % (dq, dx))
    if n < 1 or m < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (min(n, m), dx))
    k = int(k)
    _check_k(k, n, m)

    def run(budget, st):
        if dx > MAX_DIM:
            raise NotImplementedError('kneighbors: at most %d features (got %d)' % (MAX_DIM, dx))
        x = _device_points(X)
        q = None
        if Q is not None:
            q = _device_points(Q).to(x.device)
        d = x.shape[1]
        L = N.lib()
        ws = torch.empty(max(16, L.dic_knn_neighbors_workspace(n, 0 if q is None else m, d, budget)), dtype=torch.uint8, device=x.device)
        dist = torch.empty((m, k), dtype=torch.float64, device=x.device)
        idx = torch.empty((m, k), dtype=torch.int32, device=x.device)
        centre = x.mean(0, keepdim=True, dtype=torch.float64).float().contiguous()
        return L.dic_knn_neighbors(N.ptr(x), x.stride(0), n, None if q is None else N.ptr(q), 0 if q is None else q.stride(0), 0 if q is None else m,
                                   N.ptr(centre), d, k, N.ptr(dist), N.ptr(idx), budget, st, N.ptr(ws), ws.numel(), N.stream_of(x)), (dist, idx)

    dist, idx = _candidate_call('kneighbors', 'dic_knn_neighbors', candidate_budget, stats, run)
    if return_device:
        return dist, idx
    return dist.cpu().numpy(), idx.cpu().numpy()


MAX_TARGETS = 1023          # csrc/dic_knn_rank.hip: KR_MAXM, the targets of a row the exact stage tallies in LDS


def neighbor_ranks(X, targets, candidate_budget=None, stats=None, return_device=False):
    """``ranks (N, m) int32``: where ``targets[i, q]`` stands among the neighbours of row i of ``X`` -- the counterpart of ``kneighbors``, which gives the
    neighbour at a rank.  ``rank = 1 + #{l != i : (d2(i, l), l) < (d2(i, j), j)}`` (include/dic_hip.h, dic_knn_ranks): the 1-based position of j in row i of
    ``kneighbors(X, N)[1]`` after the row's own index is dropped, d2 the f64 difference-form squared distance of the f32 coordinates, ties in distance
    settled by the smaller index.  A target equal to its row's index or negative (absent) has rank 0.  ``X`` (N, D): a numpy array or tensor, D <= 256;
    ``targets`` (N, m): integers below N, m <= 1023.  Nothing N x N is stored (csrc/dic_knn_rank.hip).  numpy result, or a device tensor with
    ``return_device=True``.  ``candidate_budget`` and ``stats`` as for ``kneighbors`` (8 bytes per pair the approximate pass cannot place; ``passes`` counts
    the counting passes, one per 8 targets): the budget never changes the result."""
    n, dx = _shape_of(X)
    tshape = tuple(targets.shape) if hasattr(targets, 'shape') else np.asarray(targets).shape
    if len(tshape) != 2:
        raise ValueError('targets must be 2-D (n_samples, n_targets), got shape %s' % (tshape,))
    if n < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (n, dx))
    if tshape[0] != n:
        raise ValueError('Found input variables with inconsistent numbers of samples: [%d, %d]' % (n, tshape[0]))
    m = int(tshape[1])
    if m < 1:
        raise ValueError('Expected n_targets > 0. Got %d' % m)
    if m > MAX_TARGETS:
        raise NotImplementedError('neighbor_ranks: at most %d targets per row (got %d)' % (MAX_TARGETS, m))

    def run(budget, st):
        if dx > MAX_DIM:
            raise NotImplementedError('neighbor_ranks: at most %d features (got %d)' % (MAX_DIM, dx))
        tt = torch.as_tensor(targets)
        if tt.dtype.is_floating_point or tt.dtype == torch.bool or tt.dtype.is_complex:
            raise ValueError('targets must be integers, got %s' % (tt.dtype,))
        x = _device_points(X)
        tt = tt.to(x.device)
        if int(tt.max()) >= n:
            raise ValueError('targets must be below n_samples = %d (negative: absent), got %d' % (n, int(tt.max())))
        tt = tt.clamp(min=-1).to(torch.int32).contiguous()
        d = x.shape[1]
        L = N.lib()
        ws = torch.empty(max(16, L.dic_knn_ranks_workspace(n, d, m, budget)), dtype=torch.uint8, device=x.device)
        ranks = torch.empty((n, m), dtype=torch.int32, device=x.device)
        centre = x.mean(0, keepdim=True, dtype=torch.float64).float().contiguous()
        return L.dic_knn_ranks(N.ptr(x), x.stride(0), N.ptr(centre), n, d, N.ptr(tt), m, N.ptr(ranks), budget, st, N.ptr(ws), ws.numel(), N.stream_of(x)), ranks

    ranks = _candidate_call('neighbor_ranks', 'dic_knn_ranks', candidate_budget, stats, run)
    return ranks if return_device else ranks.cpu().numpy()


class NearestNeighbors:
    """``sklearn.neighbors.NearestNeighbors(n_neighbors, algorithm='brute')`` for the euclidean metric, on ``kneighbors`` above."""

    def __init__(self, n_neighbors=5):
        self.n_neighbors = n_neighbors

    def fit(self, X, y=None):
        n, d = _shape_of(X)
        if n < 1:
            raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (n, d))
        if d > MAX_DIM:
            raise NotImplementedError('NearestNeighbors: at most %d features (got %d)' % (MAX_DIM, d))
        if int(self.n_neighbors) <= 0:
            raise ValueError('Expected n_neighbors > 0. Got %d' % int(self.n_neighbors))
        self._fit_X = X
        self.n_samples_fit_, self.n_features_in_ = n, d
        return self

    def _fitted(self):
        if not hasattr(self, '_fit_X'):
            raise RuntimeError("This NearestNeighbors instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        """``(dist, idx)`` (``idx`` alone with ``return_distance=False``).  ``X=None`` queries the fitted points and leaves each point out of its own list, as
        sklearn 1.7.2 does it: k + 1 neighbours are taken and the entry whose index is the row's own is dropped; where the row's own index is not among
        them (k + 1 or more duplicates of the point sort before it) the first column is dropped."""
        self._fitted()
        k = int(self.n_neighbors if n_neighbors is None else n_neighbors)
        query_is_train = X is None
        n = self.n_samples_fit_
        if query_is_train:
            _check_k(k + 1, n, n, query_is_train=True)
            dist, idx = kneighbors(self._fit_X, k + 1)
            keep = idx != np.arange(n, dtype=idx.dtype)[:, None]
            keep[np.all(keep, axis=1), 0] = False
            dist, idx = dist[keep].reshape(n, k), idx[keep].reshape(n, k)
        else:
            m, d = _shape_of(X)
            if d != self.n_features_in_:
                raise ValueError('X has %d features, but NearestNeighbors is expecting %d features as input.' % (d, self.n_features_in_))
            _check_k(k, n, m)
            dist, idx = kneighbors(self._fit_X, k, Q=X)
        return (dist, idx) if return_distance else idx

    def kneighbors_graph(self, X=None, n_neighbors=None, mode='connectivity'):
        """The k-neighbour graph as the CSR triple ``(data (M k,) float64, indices (M k,) int32, indptr (M + 1,) int64)`` of an (M, n_samples_fit) matrix
        -- ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(M, n_samples_fit))`` is sklearn's ``kneighbors_graph``.  ``mode='connectivity'``: ones;
        ``'distance'``: the distances."""
        if mode not in ('connectivity', 'distance'):
            raise ValueError('Unsupported mode, must be one of "connectivity", or "distance" but got "%s" instead' % (mode,))
        dist, idx = self.kneighbors(X, n_neighbors)
        m, k = idx.shape
        data = np.ones(m * k, dtype=np.float64) if mode == 'connectivity' else np.ascontiguousarray(dist).ravel()
        return data, np.ascontiguousarray(idx).ravel(), np.arange(0, m * k + 1, k, dtype=np.int64)


def knn_transfer_labels(X_train, labels_train, Q, k, candidate_budget=None):
    """``(labels (M,) int32, share (M,) float32)``: every row of ``Q`` takes the label most frequent among its k nearest rows of ``X_train`` --
    ``KNeighborsClassifier(n_neighbors=k, algorithm='brute').fit(X_train, labels_train).predict(Q)``, uniform weights.  Every distinct label is a class,
    -1 (noise) included; on equal votes the smallest label wins.  ``share`` is the winner's fraction of the k votes.  The vote runs on the device."""
    n, _ = _shape_of(X_train)
    y = np.asarray(labels_train)
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError('Found input variables with inconsistent numbers of samples: [%d, %d]' % (n, y.shape[0] if y.ndim else 0))
    if not np.issubdtype(y.dtype, np.integer):
        raise ValueError('labels_train must be integers, got %s' % y.dtype)
    _, idx = kneighbors(X_train, k, Q=Q, candidate_budget=candidate_budget, return_device=True)
    classes, codes = np.unique(y, return_inverse=True)          # ascending: the first maximum below is the smallest label
    votes = torch.as_tensor(codes.astype(np.int64), device=idx.device)[idx.long()]          # (M, k) class codes
    tally = torch.zeros((idx.shape[0], len(classes)), dtype=torch.int64, device=idx.device)
    tally.scatter_add_(1, votes, torch.ones_like(votes))
    best = tally.max(dim=1).values
    win = (tally == best[:, None]).int().argmax(dim=1)          # argmax returns the FIRST maximal index (documented by torch): of the classes at the maximum, the smallest label
    labels = classes[win.cpu().numpy()].astype(np.int32)
    share = (best.float() / float(idx.shape[1])).cpu().numpy().astype(np.float32)
    return labels, share


def core_distances(X, min_samples, candidate_budget=None, stats=None):
    """``sklearn.cluster.OPTICS(min_samples=min_samples, max_eps=inf).fit(X).core_distances_``: the distance to the min_samples-th neighbour, the point itself
    counted -- ``kth_neighbor_distance(X, min_samples)``.  optics.py rounds it to 15 decimals, as sklearn does, and walks the ordering from it."""
    return kth_neighbor_distance(X, min_samples, candidate_budget, stats)


def kneedle_elbow(y_sorted, S=1.0):
    """The knee of the increasing convex curve (x, y), x = 1..N: ``(elbow_x, elbow_y)``, or ``(None, None)`` when there is none.  It restates what upstream
    asks of the ``kneed`` package -- ``KneeLocator(x, y, S=S, curve='convex', direction='increasing')`` with its defaults ``interp_method='interp1d'``,
    ``online=False`` (Satopaa et al., "Finding a 'Kneedle' in a Haystack", 2011):

        xn = (x - x_0) / (x_N - x_0);  yn = (y - min) / (max - min);  yt = flip(max(yn) - yn);  D = yt - xn
        maxima / minima of D: scipy.signal.argrelextrema with np.greater_equal / np.less_equal;  Tmx = D[maxima] - S * mean(|diff(xn)|)
        walk i upwards from the first maximum: at a maximum set the threshold (its Tmx) and the candidate (i); at a minimum reset the threshold to 0; the
        first i with D[i + 1] < threshold ends the walk: the knee is x[N - 1 - candidate] (the flip turns the index round).
    """
    from scipy.signal import argrelextrema
    y = np.asarray(y_sorted, dtype=np.float64).ravel()
    n = y.size
    if n < 2:
        return None, None
    span = y.max() - y.min()
    if not span > 0:
        return None, None
    x = np.arange(1, n + 1, dtype=np.float64)
    xn = (x - x[0]) / (x[-1] - x[0])
    yn = (y - y.min()) / span
    yt = np.flip(yn.max() - yn)
    D = yt - xn
    maxima = argrelextrema(D, np.greater_equal)[0]
    minima = argrelextrema(D, np.less_equal)[0]
    if not maxima.size:
        return None, None
    Tmx = D[maxima] - S * np.abs(np.diff(xn).mean())
    # the walk, all samples at once: the threshold in force at i comes from the last maximum or minimum at or before i (a minimum, which resets it to 0,
    # wins where a sample is both), the candidate is the last maximum at or before i
    idx = np.arange(n)
    is_max = np.zeros(n, dtype=bool)
    is_max[maxima] = True
    is_min = np.zeros(n, dtype=bool)
    is_min[minima] = True
    tmx_at = np.zeros(n)
    tmx_at[maxima] = Tmx
    last_event = np.maximum.accumulate(np.where(is_max | is_min, idx, -1))
    candidate = np.maximum.accumulate(np.where(is_max, idx, -1))
    first = int(maxima[0])
    ev = last_event[first:n - 1]          # (the last sample, xn = 1, ends the walk; from the first maximum on every sample has an event behind it)
    threshold = np.where(is_min[ev], 0.0, tmx_at[ev])
    hits = np.flatnonzero(D[first + 1:] < threshold)
    if not hits.size:
        return None, None
    at = n - 1 - int(candidate[first + hits[0]])
    return int(x[at]), float(y[at])


def k_distance_graph(X, k, candidate_budget=None, stats=None):
    """p2's k-distance graph (p2_clustering_optK.py:110-119): ``dict(k, sorted_dist (N,) float64 ascending, elbow_x, elbow_y)``."""
    dist = np.sort(kth_neighbor_distance(X, k, candidate_budget, stats))
    ex, ey = kneedle_elbow(dist, S=1.0)
    return {'k': int(k), 'sorted_dist': dist, 'elbow_x': ex, 'elbow_y': ey}
