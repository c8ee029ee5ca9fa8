"""DBCV, Density-Based Clustering Validation (Moulavi, Jaskowiak, Campello, Zimek and Sander, SDM 2014), on the MI355X without the distance matrix: one
number in [-1, 1] for a labelling with clusters of arbitrary shape and a noise label -- what ``hdbscan.validity.validity_index`` computes on the CPU.

include/dic_hip.h states the definition once.  Each cluster is weighed by its share of ALL rows, noise included, and judged by its loosest internal connection
(density sparseness: the largest internal edge of its mutual-reachability spanning tree) against its tightest connection to any other cluster (density
separation), both with the all-points core distance ``a`` in place of HDBSCAN's k-th neighbour distance.

ONE DEVIATION FROM THE CPU PACKAGE, on purpose: the package raises ``1 / d(o, p)`` to the power of the number of features, which leaves f64's range for
almost every pair at 256 features; here ``a`` is formed in log space with the largest term factored out (every term in (0, 1]), so it exists at any dimension.

The two O(N^2) passes are csrc/dic_dbcv.hip (``dic_dbcv_core``, ``dic_dbcv_separation``); the spanning trees are one ``dic_hdbscan_mst`` walk per cluster
on the slice of the sorted rows, results kept on the device until all walks are enqueued; the segment minima are torch's.  What remains is O(N) host work
on the walks' arrays, in the plain numpy functions below, which need no GPU: ``tree_degrees``, ``internal_nodes``, ``internal_edges``, ``sparseness``,
``cluster_validity``, ``weighted_score`` and ``partition``.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from . import knn
from .dbscan import MAX_DIM, _device_points

NOISE = -1


# ---- host: plain numpy on the walks' arrays ------------------------------------------------------------------------------------------------------------
def tree_degrees(pred):
    """Degrees of the tree whose edges are ``(q, pred[q])`` for every q with ``pred[q] >= 0`` (a walk's predecessor array: -1 for its first point)."""
    pred = np.asarray(pred, dtype=np.int64)
    deg = np.zeros(len(pred), dtype=np.int64)
    child = np.flatnonzero(pred >= 0)
    np.add.at(deg, child, 1)
    np.add.at(deg, pred[child], 1)
    return deg


def internal_nodes(pred):
    """(n,) bool: the members of tree degree >= 2; where there are none (a pair), the cluster's first member."""
    internal = tree_degrees(pred) >= 2
    if not internal.any():
        internal[0] = True
    return internal


def internal_edges(pred, internal):
    """(n,) bool over the edges ``(q, pred[q])``, indexed by q: both ends internal; where there is none (a pair, a path of three, a star), every edge."""
    pred = np.asarray(pred, dtype=np.int64)
    edge = pred >= 0
    both = edge & internal & internal[np.where(edge, pred, 0)]
    return both if both.any() else edge


def sparseness(pred, reach):
    """``(DSC, internal)`` of one cluster's walk: the largest internal edge weight (``reach[q]`` weighs the edge ``(q, pred[q])``) and the internal-node mask."""
    internal = internal_nodes(pred)
    return float(np.asarray(reach, dtype=np.float64)[internal_edges(pred, internal)].max()), internal


def cluster_validity(dsc, sep):
    """V = (sep - DSC) / max(sep, DSC), elementwise; 0 where both are 0."""
    dsc, sep = np.asarray(dsc, dtype=np.float64), np.asarray(sep, dtype=np.float64)
    top = np.maximum(sep, dsc)
    return np.where(top > 0, (sep - dsc) / np.where(top > 0, top, 1.0), 0.0)


def weighted_score(sizes, validity, n_total):
    """DBCV = sum_C |C| / N V(C), N counting every row."""
    return float(np.sum(np.asarray(sizes, dtype=np.float64) / float(n_total) * np.asarray(validity, dtype=np.float64)))


def partition(labels):
    """What the definition keeps of a labelling: ``(cluster_ids, sizes, order, seg_start, n_noise, n_singletons)`` -- the ids of the clusters with at least
    two members, ascending, their sizes, the kept rows sorted by (cluster, row), the K + 1 segment offsets into that order, the rows labelled -1 and the
    number of one-member clusters (treated as noise).  Fewer than two kept clusters: ValueError."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError('labels must be a 1-D integer array, got %s %s' % (labels.dtype, labels.shape))
    labels = labels.astype(np.int64)
    ids, inverse, counts = np.unique(labels, return_inverse=True, return_counts=True)
    kept_id = (ids != NOISE) & (counts >= 2)
    n_singletons = int(((ids != NOISE) & (counts == 1)).sum())
    n_noise = int((labels == NOISE).sum())
    if kept_id.sum() < 2:
        raise ValueError('DBCV needs at least 2 clusters of at least 2 members, got %d' % int(kept_id.sum()))
    rows = np.flatnonzero(kept_id[inverse])
    order = rows[np.argsort(labels[rows], kind='stable')]
    sizes = counts[kept_id].astype(np.int64)
    seg_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return ids[kept_id], sizes, order, seg_start, n_noise, n_singletons


def _exponent(d, width):
    if d is None:
        return int(width)
    if isinstance(d, bool) or not isinstance(d, numbers.Real) or not 1 <= d <= 65536:
        raise ValueError('d must be a number in [1, 65536], got %r' % (d,))
    return d


class DBCV:
    """The result for one labelling.  ``score``; per kept cluster, in ascending id order: ``cluster_ids``, ``sizes``, ``sparseness``, ``separation``,
    ``validity``, ``nearest_cluster`` (the id of the cluster that sets the separation); ``n_noise``, ``n_singletons``; per row, in the caller's order:
    ``core_distances_`` (NaN for noise and singletons) and ``internal_`` (bool)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'DBCV(score=%.6f, clusters=%d, n_noise=%d, n_singletons=%d)' % (self.score, len(self.cluster_ids), self.n_noise, self.n_singletons)


# ---- device ---------------------------------------------------------------------------------------------------------------------------------------------
def device_core_distances(xs, seg_d, dpow):
    """``dic_dbcv_core`` on sorted device rows: (n,) f64 device tensor."""
    L = N.lib()
    n, D = xs.shape
    K = seg_d.numel() - 1
    ws = torch.empty(max(16, L.dic_dbcv_workspace(n, K)), dtype=torch.uint8, device=xs.device)
    a = torch.empty(n, dtype=torch.float64, device=xs.device)
    N.check(L.dic_dbcv_core(N.ptr(xs), xs.stride(0), n, D, N.ptr(seg_d), K, float(dpow), N.ptr(a), N.ptr(ws), ws.numel(), N.stream_of(xs)), 'dic_dbcv_core')
    return a


def device_walks(xs, seg_start, a):
    """One ``dic_hdbscan_mst`` walk per segment on the slice pointers, ``core = a``; the walks share one workspace (a stream runs them in order) and their
    results stay on the device: ``(reach f64, pred int32)`` (n,) device tensors, ``pred`` local to its segment (-1 for the segment's first row)."""
    L = N.lib()
    n, D = xs.shape
    ldx = xs.stride(0)
    dev = xs.device
    ordering = torch.empty(n, dtype=torch.int32, device=dev)
    reach = torch.empty(n, dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    biggest = int(np.max(np.diff(seg_start)))
    ws = torch.empty(max(16, L.dic_hdbscan_workspace(biggest, D)), dtype=torch.uint8, device=dev)
    stream = N.stream_of(xs)
    for s0, s1 in zip(seg_start[:-1].tolist(), seg_start[1:].tolist()):
        N.check(L.dic_hdbscan_mst(xs.data_ptr() + 4 * s0 * ldx, ldx, s1 - s0, D, a.data_ptr() + 8 * s0, ordering.data_ptr() + 4 * s0,
                                  reach.data_ptr() + 8 * s0, pred.data_ptr() + 4 * s0, N.ptr(ws), ws.numel(), stream), 'dic_hdbscan_mst')
    return reach, pred


def device_separation(xs, seg_d, a, internal_d):
    """``dic_dbcv_separation``: ``(rowsep f64, rowarg int32)`` (n,) device tensors."""
    L = N.lib()
    n, D = xs.shape
    K = seg_d.numel() - 1
    ws = torch.empty(max(16, L.dic_dbcv_workspace(n, K)), dtype=torch.uint8, device=xs.device)
    rowsep = torch.empty(n, dtype=torch.float64, device=xs.device)
    rowarg = torch.empty(n, dtype=torch.int32, device=xs.device)
    N.check(L.dic_dbcv_separation(N.ptr(xs), xs.stride(0), n, D, N.ptr(seg_d), K, N.ptr(a), N.ptr(internal_d), N.ptr(rowsep), N.ptr(rowarg), N.ptr(ws),
                                  ws.numel(), N.stream_of(xs)), 'dic_dbcv_separation')
    return rowsep, rowarg


def _segment_minima(rowsep, rowarg, internal_d, sizes):
    """Per segment: the smallest ``rowsep`` over its internal rows and the segment of the row that attains it (the first such row, its ``rowarg``)."""
    dev = rowsep.device
    n, K = rowsep.numel(), len(sizes)
    segid = torch.repeat_interleave(torch.arange(K, device=dev), torch.as_tensor(sizes, device=dev))
    vals = torch.where(internal_d.bool(), rowsep, torch.full_like(rowsep, float('inf')))
    segmin = torch.full((K,), float('inf'), dtype=torch.float64, device=dev).scatter_reduce_(0, segid, vals, 'amin')
    at = torch.where(vals == segmin[segid], torch.arange(n, device=dev), torch.full((n,), n, device=dev))
    first = torch.full((K,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, segid, at, 'amin')
    partner = rowarg.long()[first.clamp(max=n - 1)]
    nearest = torch.where(partner >= 0, segid[partner.clamp(min=0)], torch.full_like(partner, -1))
    return segmin.cpu().numpy(), nearest.cpu().numpy()


def _score(x, width, labels, d):
    n_rows = x.shape[0]
    labels = np.asarray(labels)
    if labels.shape != (n_rows,):
        raise ValueError('labels must have one entry per row of X: %s against %d rows' % (labels.shape, n_rows))
    ids, sizes, order, seg_start, n_noise, n_singletons = partition(labels)
    dpow = _exponent(d, width)
    dev = x.device
    xs = x.index_select(0, torch.as_tensor(order, device=dev)).contiguous()
    seg_d = torch.as_tensor(seg_start, dtype=torch.int32, device=dev)
    a = device_core_distances(xs, seg_d, dpow)
    reach_d, pred_d = device_walks(xs, seg_start, a)
    reach, pred = reach_d.cpu().numpy(), pred_d.cpu().numpy().astype(np.int64)
    K = len(sizes)
    dsc = np.empty(K)
    internal = np.zeros(len(order), dtype=bool)
    for s in range(K):
        s0, s1 = seg_start[s], seg_start[s + 1]
        dsc[s], internal[s0:s1] = sparseness(pred[s0:s1], reach[s0:s1])
    internal_d = torch.as_tensor(internal.astype(np.uint8), device=dev)
    rowsep, rowarg = device_separation(xs, seg_d, a, internal_d)
    sep, nearest = _segment_minima(rowsep, rowarg, internal_d, sizes)
    validity = cluster_validity(dsc, sep)
    core = np.full(n_rows, np.nan)
    core[order] = a.cpu().numpy()
    internal_rows = np.zeros(n_rows, dtype=bool)
    internal_rows[order] = internal
    return DBCV(score=weighted_score(sizes, validity, n_rows), cluster_ids=ids, sizes=sizes, sparseness=dsc, separation=sep, validity=validity,
                nearest_cluster=np.where(nearest >= 0, ids[np.maximum(nearest, 0)], NOISE), n_noise=n_noise, n_singletons=n_singletons,
                core_distances_=core, internal_=internal_rows)


def _points(X):
    n, width = knn._shape_of(X)
    if width > MAX_DIM:
        raise NotImplementedError('dbcv: at most %d features (got %d)' % (MAX_DIM, width))
    return _device_points(X), width


def dbcv(X, labels, d=None):
    """The ``DBCV`` result of one labelling of ``X`` (numpy array or tensor, (N, D), D <= 256; a tensor on the device gives the same bits as the numpy
    array).  ``labels`` (N,) int, -1 for noise; ``d`` the exponent, default the column count of ``X``.  Fewer than two clusters of at least two
    members: ValueError."""
    x, width = _points(X)
    return _score(x, width, labels, d)


def validity_index(X, labels, d=None, per_cluster=False):
    """``hdbscan.validity.validity_index`` for the euclidean metric: the DBCV score, and with ``per_cluster`` also the (K,) validities of the kept
    clusters in ascending id order."""
    res = dbcv(X, labels, d)
    return (res.score, res.validity) if per_cluster else res.score


def dbcv_sweep(X, labellings, d=None):
    """``{name: DBCV}`` for every entry of ``labellings`` (``{name: labels}``): the points are uploaded once; each entry has the bits of its own call."""
    x, width = _points(X)
    return {name: _score(x, width, labels, d) for name, labels in labellings.items()}
