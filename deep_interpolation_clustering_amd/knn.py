"""k-th neighbour distances on the MI355X without the distance matrix, and the k-distance elbow p2 chooses DBSCAN's eps with (p2_clustering_optK.py:102-120).

Upstream: ``NearestNeighbors(n_neighbors=k, n_jobs=5).fit(X).kneighbors(X)[0][:, -1]`` -- a brute-force all-pairs pass on the CPU -- sorted, and the knee of
that curve from ``kneed.KneeLocator(point_num, sorted_dist, S=1.0, curve='convex', direction='increasing')``.  Here the distances come from
csrc/dic_knn.hip: counting passes of the DBSCAN tile machine with per-row thresholds narrow every row's k-th distance to a short candidate list, and the
value at the exact rank is taken from f64 difference-form distances of the candidates.  The convention is upstream's: the point itself is its own first
neighbour (k = 1 gives 0, duplicates give zeros).  The same quantity is OPTICS' core distance (``core_distances``): optics.py builds on it.
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
    budget = 0 if candidate_budget is None else int(candidate_budget)
    if candidate_budget is not None and budget < 1:
        raise ValueError('candidate_budget must be positive, got %r' % (candidate_budget,))
    x = _device_points(X)
    d = x.shape[1]
    if d > MAX_DIM:
        raise NotImplementedError('kth_neighbor_distance: at most %d features (got %d)' % (MAX_DIM, d))
    L = N.lib()
    ws = torch.empty(max(16, L.dic_knn_workspace(n, d, budget)), dtype=torch.uint8, device=x.device)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    centre = x.mean(0, keepdim=True, dtype=torch.float64).float().contiguous()
    st = (N.C.c_int64 * len(STAT_NAMES))()
    rc = L.dic_knn_kth_distance(N.ptr(x), x.stride(0), N.ptr(centre), n, d, k, N.ptr(out), budget, st, N.ptr(ws), ws.numel(), N.stream_of(x))
    if stats is not None:
        stats.update(zip(STAT_NAMES, (int(v) for v in st)))
    if rc == -3 and st[4] > 0:          # DIC_ERR_WORKSPACE: one list alone is longer than the budget
        raise CandidateBudgetError('kth_neighbor_distance: %s' % L.dic_last_error_string().decode(), st[4])
    N.check(rc, 'dic_knn_kth_distance')
    return out.cpu().numpy()


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
