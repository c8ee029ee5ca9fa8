"""Ward's agglomerative clustering on the MI355X without the distance matrix (``scipy.cluster.hierarchy.linkage(X, 'ward')``,
``sklearn.cluster.AgglomerativeClustering(linkage='ward')``): the p2 / p4 ``--cluster_method ward`` branches.

Ward's criterion optimises the within-cluster variance k-means optimises, but builds ONE tree that serves every K: p2's K sweep cuts it at K = 2..k_max instead
of fitting per K, and because Ward clusters have centroids p4 labels the validation and test cohorts by the nearest training centre, as its k-means branch
does.  scipy and sklearn agglomerate on top of the condensed distance matrix (22 GB at 75 000 points) or a connectivity heap.  Ward's distance of two clusters
depends only on their sizes and centroids, ``d2(i, j) = (2 n_i n_j / (n_i + n_j)) |C_i - C_j|^2``, so every step of scipy's nearest-neighbour chain is one row
pass over the centroids of the live clusters on the device (csrc/dic_ward.hip): the launches -- at most 3 (N - 1) -- are enqueued back to back, all state stays
on the device, and the host reads the N - 1 merges once.

The host finish is consensus.py's: the stable sort of the merges by height and scipy's relabelling (``consensus._relabel``), then the cuts.  The package does
not import scipy or sklearn.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from . import cluster_stats
from .consensus import _relabel
from .dbscan import MAX_DIM
from .kmeans import KMeans, _as_device_matrix, _device, _pad_features


def _shape_of(X):
    shape = tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (shape,))
    n, width = shape
    if width > MAX_DIM:
        raise NotImplementedError('ward: at most %d features (got %d)' % (MAX_DIM, width))
    if n < 2 or width < 1:
        raise ValueError('ward needs at least 2 points of at least 1 feature, got shape %s' % (shape,))
    return n, width


def _usable_view(X):
    """A device tensor the kernel can read where it lies: f32 rows of a multiple of 4 features, 16-B aligned, unit column stride."""
    return (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] % 4 == 0 and X.stride(1) == 1
            and X.stride(0) >= X.shape[1] and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0)


def _device_points(X):
    """The points as the kernel takes them: (N, D') f32 on the device, the features zero-padded to a multiple of 4 as ``kmeans._pad_features`` pads them (zero
    columns change no centroid distance).  A strided view that already qualifies is used in place."""
    if _usable_view(X):
        return X.detach()
    return _pad_features(_as_device_matrix(X, _device())).contiguous()


def _require_bytes(nbytes, device, n, d):
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > free:
        raise MemoryError('the Ward linkage of %d points needs %d bytes on the device, %d are free: the f64 sums and centroids of the clusters, 2 x 8 N D bytes '
                          '(D = %d)' % (n, nbytes, free, d))


def ward_records(X, stats=None):
    """The raw merges of the nearest-neighbour chain, in the order they happen: (N - 1, 4) f64 numpy, rows (a, b, height, size) with a < b the names of the two
    clusters (the merged cluster keeps the name b).  ``stats`` (a dict, optional) receives ``steps``, the launches that pushed or merged (<= 3 (N - 1)), and
    ``launches``, the launches enqueued."""
    n, _ = _shape_of(X)
    x = _device_points(X)
    d = x.shape[1]
    L = N.lib()
    dev = x.device
    nbytes = int(L.dic_ward_workspace(n, d))
    if nbytes == 0:
        raise ValueError('ward: N=%d D=%d is outside the kernel\'s limits (2 <= N < 2^30)' % (n, d))
    _require_bytes(nbytes + 32 * (n - 1), dev, n, d)
    ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=dev)
    rec = torch.empty((n - 1, 4), dtype=torch.float64, device=dev)
    N.check(L.dic_ward_linkage(N.ptr(x), x.stride(0), n, d, N.ptr(rec), N.ptr(ws), ws.numel(), N.stream_of(x)), 'dic_ward_linkage')
    out = rec.cpu().numpy()
    if stats is not None:
        state = ws[nbytes - 256:nbytes - 240].cpu().numpy().view(np.int32)          # chain length, merges done, launches that pushed or merged, cursor
        stats['steps'], stats['merges'], stats['launches'] = int(state[2]), int(state[1]), 3 * (n - 1)
    return out


def ward_linkage(X, stats=None):
    """``scipy.cluster.hierarchy.linkage(X.astype(np.float64), 'ward')`` for the f32 points ``X`` (numpy array or tensor, (N, D), N >= 2, D <= 256): Z
    (N - 1, 4) f64, numpy, in scipy's format -- the merges in stable order of their heights, every merged cluster named N, N + 1, .. as it is made, the smaller
    name first.  A tensor on the device gives the same bits as the numpy array of the same points.  MemoryError (naming the bytes) when the workspace, linear
    in N, does not fit."""
    rec = ward_records(X, stats)
    return _relabel(rec, len(rec) + 1)


def _check_ks(ks, n):
    out = []
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
            raise ValueError('the numbers of clusters must be ints, got %r' % (k,))
        if not 1 <= int(k) <= n:
            raise ValueError('K must be in 1..%d, got %d' % (n, int(k)))
        out.append(int(k))
    return out


def cut_many(Z, ks):
    """The partitions of the dendrogram ``Z`` after N - K merges for every K of ``ks``, in one top-down walk of Z: {K: (N,) int64}, 0-based, the clusters
    numbered in order of first appearance by point index -- for one K, ``consensus.cut_linkage(Z, K) - 1``."""
    Z = np.asarray(Z)
    n = len(Z) + 1
    ks = _check_ks(ks, n)
    if not ks:
        return {}
    parent = np.full(2 * n - 1, 2 * n - 1, dtype=np.int64)          # (the root's parent: a name above every threshold)
    made = n + np.arange(n - 1)
    parent[Z[:, 0].astype(np.int64)] = made
    parent[Z[:, 1].astype(np.int64)] = made
    first_absent = np.array([2 * n - k for k in ks], dtype=np.int64)          # at the cut of K the clusters n .. 2 n - K - 1 have been made
    top = np.empty((2 * n - 1, len(ks)), dtype=np.int64)          # the cluster a node belongs to at every cut (a node not made yet: unused)
    par = parent.tolist()
    for node in range(2 * n - 2, -1, -1):          # a merged cluster has a larger name than its parts: top down
        p = par[node]
        if p >= 2 * n - 1:
            top[node] = node
        else:
            top[node] = np.where(p >= first_absent, node, top[p])
    out = {}
    for j, k in enumerate(ks):
        uniq, first, inv = np.unique(top[:n, j], return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), dtype=np.int64)
        rank[np.argsort(first, kind='stable')] = np.arange(len(uniq))
        out[k] = rank[inv.reshape(-1)]
    return out


def member_means(X, labels, K):
    """(K, D) f32 numpy: the means of the rows of ``X`` per 0-based label, summed in f64 on the device (``dic_segment_sum_f64``)."""
    x = _as_device_matrix(X, _device())
    lab = torch.as_tensor(np.asarray(labels, dtype=np.int64), device=x.device)
    cnt = torch.bincount(lab, minlength=K).double()
    return (cluster_stats._segment_sum(x, lab, K) / cnt[:, None]).float().cpu().numpy()


class Ward:
    """Ward linkage of the points and its cuts.  ``n_clusters``: the K of ``labels_`` / ``cluster_centers_`` (default: the largest of ``ks``, or 2);
    ``ks``: every K to cut at (``n_clusters`` is added).  After ``fit``: ``linkage_`` (Z, scipy's format), ``labels_by_k_`` {K: (N,) int64, 0-based, numbered
    by first appearance}, ``labels_``, ``cluster_centers_by_k_`` {K: (K, D) f32, the means of the members, computed on the device}, ``cluster_centers_``,
    ``heights_by_k_`` {K: the height of the merge that takes K clusters to K - 1} and ``n_steps_``, the launches that pushed or merged.
    ``predict`` labels points by the nearest centre of ``cluster_centers_`` through the k-means assignment kernel.  A training point's tree label need not be
    its nearest centre: Ward merges greedily and never reassigns."""

    def __init__(self, n_clusters=None, ks=None, metric='euclidean', linkage='ward'):
        if metric == 'precomputed':
            raise NotImplementedError("metric='precomputed' is not supported: pass the points themselves -- the distances are recomputed on the GPU, "
                                      'which is what spares the N x N matrix')
        if metric not in ('euclidean', 'l2'):
            raise NotImplementedError('only the euclidean metric is on the accelerated path')
        if linkage != 'ward':
            raise NotImplementedError("only linkage='ward' is on the accelerated path (average linkage of a matrix: consensus.average_linkage)")
        ks = [] if ks is None else list(ks)
        for k in ks + ([] if n_clusters is None else [n_clusters]):
            if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)) or k < 1:
                raise ValueError('the numbers of clusters must be ints >= 1, got %r' % (k,))
        if n_clusters is None:
            n_clusters = max(ks) if ks else 2
        self.n_clusters = int(n_clusters)
        self.ks = sorted(set(int(k) for k in ks) | {self.n_clusters})

    def fit(self, X, y=None):
        n, width = _shape_of(X)
        _check_ks(self.ks, n)
        stats = {}
        self.linkage_ = ward_linkage(X, stats)
        self.n_steps_ = stats['steps']
        self.labels_by_k_ = cut_many(self.linkage_, self.ks)
        self.heights_by_k_ = {k: float(self.linkage_[n - k, 2]) for k in self.ks if k >= 2}
        self.cluster_centers_by_k_ = {k: member_means(X, self.labels_by_k_[k], k) for k in self.ks}
        self.labels_ = self.labels_by_k_[self.n_clusters]
        self.cluster_centers_ = self.cluster_centers_by_k_[self.n_clusters]
        self.n_features_in_ = width
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def _assigner(self, centers=None):
        km = KMeans(n_clusters=self.n_clusters)
        km.cluster_centers_ = self.cluster_centers_ if centers is None else centers
        return km

    def predict(self, X, centers=None):
        """(N,) int32 numpy: the index of the nearest row of ``cluster_centers_`` (or of ``centers``), by the k-means E-step kernel."""
        return self._assigner(centers).predict(X)

    def nearest_distance(self, X, centers=None):
        """(N,) f32 on the device: the distance of every row of ``X`` to its nearest centre (``KMeans.nearest_distance``)."""
        return self._assigner(centers).nearest_distance(X)
