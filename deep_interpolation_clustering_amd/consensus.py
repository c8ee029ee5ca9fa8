"""Consensus clustering on the MI355X (Monti et al. 2003 / ConsensusClusterPlus, k-means base clusterer): the p2 / p4 ``--cluster_method consensus`` branches.

Upstream's p4 only reads ``raw_consensus_result/<cohort>_consensus.csv`` (p4_clustering_final.py:241-287), labels that were "generated outside"; this module
generates them.  H times a fraction ``p_item`` of the points is drawn without replacement and clustered by ``kmeans.KMeans`` for every K; the labels go to a
label matrix (N, H) uint8, 0xFF = "not in this resample".  csrc/dic_consensus.hip then makes, from the label matrix alone and in integers, the consensus
``M(i, j) = agree / both`` of every pair: its histogram (the CDF, its area A(K) and the relative change of the area, the curves K is chosen from), the
distance ``1 - M`` as a square f64 matrix, and the per-cluster row sums that cluster and item consensus are made of.  The final labels cut the average-linkage
dendrogram of that distance at K clusters; the agglomeration runs on the device, one launch per step of scipy's nearest-neighbour chain, bit for bit scipy's
``linkage(squareform(D), 'average')``, ties included -- on real inputs most merge heights are exactly 0 or exactly 1, so the ties decide the partition.

THE ONE N x N ARRAY OF THE PACKAGE is that distance matrix: 8 N^2 bytes, 45 GB at 75 000 points.  Average linkage on a ratio-valued similarity has no
matrix-free form (the distance of two clusters is a mean of quotients over their pairs), so the matrix is held, after checking that it fits.

The package does not import scipy or sklearn; the stable sort of the merges by height, scipy's relabelling and the cut run on the host in numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .kmeans import KMeans, _as_device_matrix, _device

BINS = 100            # B: the CDF is evaluated at b / B, b = 0..B (DIC_CONSENSUS_BINS)
UNSAMPLED = 0xFF
MAX_K, MAX_H = 254, 65535


def draw_resamples(n, reps, p_item, seed):
    """``reps`` index sets of ``floor(p_item * n)`` points each, without replacement, from one ``np.random.RandomState(seed)``; the same sets serve every K."""
    m = int(np.floor(p_item * n))
    if not 1 <= m <= n:
        raise ValueError('p_item=%r leaves %d of %d points in a resample' % (p_item, m, n))
    if not 1 <= reps <= MAX_H:
        raise ValueError('reps must be in 1..%d, got %r' % (MAX_H, reps))
    rs = np.random.RandomState(seed)
    return [rs.choice(n, m, replace=False) for _ in range(reps)]


def label_matrix(X, K, resamples, n_init=1, seed=0):
    """The label matrix of ``K``: (N, ldl) uint8 on the device, ldl = the number of resamples rounded up to a multiple of 16; column h holds the labels 0..K-1 of
    ``KMeans(K, n_init=n_init)`` fitted on ``X[resamples[h]]`` (seeded from ``(seed, h, K)``) and 0xFF for the points resample h left out, as do the padding
    columns."""
    K = int(K)
    if not 2 <= K <= min(MAX_K, N.MAX_CLUSTERS):
        raise ValueError('K must be in 2..%d, got %d' % (min(MAX_K, N.MAX_CLUSTERS), K))
    if not 1 <= len(resamples) <= MAX_H:
        raise ValueError('1..%d resamples, got %d' % (MAX_H, len(resamples)))
    Xd = _as_device_matrix(X, _device())
    n = Xd.shape[0]
    L = torch.full((n, -(-len(resamples) // 16) * 16), UNSAMPLED, dtype=torch.uint8, device=Xd.device)
    for h, idx in enumerate(resamples):
        idx_d = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=Xd.device)
        km = KMeans(n_clusters=K, n_init=n_init, random_state=np.random.RandomState([int(seed), h, K])).fit(Xd[idx_d])
        L[idx_d, h] = torch.as_tensor(km.labels_.astype(np.uint8), device=Xd.device)
    return L


def _device_labels(L):
    """(label matrix (N, ldl) uint8 on the device with ldl % 16 == 0 and 0xFF padding, H).  A padding column is a resample nobody was in."""
    if isinstance(L, torch.Tensor):
        t = L
    else:
        t = torch.from_numpy(np.array(L, order='C'))          # (a copy: the caller's array may be read-only)
    if t.dim() != 2 or t.dtype != torch.uint8:
        raise ValueError('the label matrix is a 2-D uint8 array, got %s %s' % (tuple(t.shape), t.dtype))
    n, h = t.shape
    if n < 2 or not 1 <= h <= MAX_H:
        raise ValueError('the label matrix needs N >= 2 rows and 1..%d columns, got %s' % (MAX_H, (n, h)))
    t = t.to(_device())
    if h % 16 or not t.is_contiguous():
        p = torch.full((n, -(-h // 16) * 16), UNSAMPLED, dtype=torch.uint8, device=t.device)
        p[:, :h] = t
        t = p
    return t, h


def _require_bytes(nbytes, device, what):
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > free:
        raise MemoryError('%s needs %d bytes on the device, %d are free: the consensus distance is held as a square f64 matrix, 8 N^2 bytes'
                          % (what, nbytes, free))


def consensus_pairs(L, y=None, want_distance=False, want_hist=True, n_clusters=None):
    """One pair pass over the label matrix ``L`` ((N, H) uint8, numpy or tensor; 0xFF = not sampled): ``(hist, rowsum, D)``.
    ``hist`` (BINS + 1,) uint64, numpy: the exact count, over the pairs i < j, of ``ceil(BINS * agree / both)`` (0 when both == 0); None unless ``want_hist``.
    ``rowsum`` (N, K) f64, numpy: ``sum_{j != i, y_j == c} agree / both`` for ``y`` (N,) the 0-based labels and K = ``n_clusters`` (default max(y) + 1);
    None without ``y``.  ``D`` (N, N) f64 ON THE DEVICE: ``1.0 - agree / both`` (1 when both == 0, 0 on the diagonal), exactly symmetric; None unless
    ``want_distance``; MemoryError when its 8 N^2 bytes do not fit.  Each output has the same bits whichever others are asked for."""
    Ld, H = _device_labels(L)
    n, ldl = Ld.shape
    dev = Ld.device
    if not (want_hist or want_distance or y is not None):
        raise ValueError('consensus_pairs: nothing asked for')
    lib = N.lib()
    hist = torch.empty(BINS + 1, dtype=torch.int64, device=dev) if want_hist else None
    K, yd, rowsum, ws = 0, None, None, None
    if y is not None:
        yh = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int32)
        if yh.shape != (n,):
            raise ValueError('y has shape %s, expected (%d,)' % (yh.shape, n))
        K = int(yh.max()) + 1 if n_clusters is None else int(n_clusters)
        if not 1 <= K <= MAX_K:
            raise ValueError('n_clusters must be in 1..%d, got %d' % (MAX_K, K))
        yd = torch.as_tensor(yh, device=dev)
        rowsum = torch.empty((n, K), dtype=torch.float64, device=dev)
        ws = torch.empty(max(16, lib.dic_consensus_pairs_workspace(n, H, K)), dtype=torch.uint8, device=dev)
    D = None
    if want_distance:
        _require_bytes(8 * n * n, dev, 'the consensus distance of %d points' % n)
        D = torch.empty((n, n), dtype=torch.float64, device=dev)
    N.check(lib.dic_consensus_pairs(N.ptr(Ld), ldl, n, H, N.ptr(yd), K, N.ptr(hist), N.ptr(rowsum), N.ptr(D), N.ptr(ws), 0 if ws is None else ws.numel(),
                                    N.stream_of(Ld)), 'dic_consensus_pairs')
    return (None if hist is None else hist.cpu().numpy().view(np.uint64), None if rowsum is None else rowsum.cpu().numpy(), D)


def _relabel(records, n):
    """scipy's finish of a nearest-neighbour-chain linkage: the merges in stable order of their heights, every merged cluster renamed n, n + 1, .. as it is
    made, the smaller name first."""
    rec = records[np.argsort(records[:, 2], kind='stable')]
    parent = np.arange(2 * n - 1)
    size = np.ones(2 * n - 1, dtype=np.int64)
    Z = np.empty((n - 1, 4), dtype=np.float64)
    left, right = rec[:, 0].astype(np.int64).tolist(), rec[:, 1].astype(np.int64).tolist()
    parent_l = parent.tolist()
    for i in range(n - 1):
        roots = []
        for x in (left[i], right[i]):
            r = x
            while parent_l[r] != r:
                r = parent_l[r]
            while parent_l[x] != r:          # path compression
                parent_l[x], x = r, parent_l[x]
            roots.append(r)
        a, b = min(roots), max(roots)
        parent_l[a] = parent_l[b] = n + i
        size[n + i] = size[a] + size[b]
        Z[i, 0], Z[i, 1], Z[i, 3] = a, b, size[n + i]
    Z[:, 2] = rec[:, 2]
    return Z


def average_linkage(D, overwrite=False):
    """``scipy.cluster.hierarchy.linkage(squareform(D), 'average')`` for the square symmetric f64 matrix ``D`` (numpy or tensor, zero diagonal): Z (N - 1, 4)
    f64, numpy, bit for bit scipy's, ties included.  The agglomeration destroys its matrix: a device tensor is copied first unless ``overwrite``.  8 N^2
    bytes must be free on the device (MemoryError names them) unless the tensor is already there and may be overwritten."""
    dev = _device()
    shape = tuple(D.shape)
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] < 2:
        raise ValueError('expected a square matrix of at least 2 points, got shape %s' % (shape,))
    n = shape[0]
    in_place = isinstance(D, torch.Tensor) and D.is_cuda and D.dtype == torch.float64 and D.is_contiguous() and overwrite
    if in_place:
        Dd = D
    else:
        _require_bytes(8 * n * n, dev, 'the average linkage of %d points' % n)
        if isinstance(D, torch.Tensor):
            Dd = D.to(device=dev, dtype=torch.float64).contiguous().clone()
        else:
            Dd = torch.as_tensor(np.ascontiguousarray(D, dtype=np.float64), device=dev)
    lib = N.lib()
    ws = torch.empty(max(16, lib.dic_linkage_average_workspace(n)), dtype=torch.uint8, device=Dd.device)
    rec = torch.empty((n - 1, 4), dtype=torch.float64, device=Dd.device)
    N.check(lib.dic_linkage_average(N.ptr(Dd), n, N.ptr(rec), N.ptr(ws), ws.numel(), N.stream_of(Dd)), 'dic_linkage_average')
    return _relabel(rec.cpu().numpy(), n)


def cut_linkage(Z, K):
    """R's ``cutree(., k=K)`` of the dendrogram ``Z``: the partition after N - K merges, (N,) int64, the clusters numbered 1..K in order of first appearance
    by point index -- the 1-based form p4 reads."""
    Z = np.asarray(Z)
    n = len(Z) + 1
    K = int(K)
    if not 1 <= K <= n:
        raise ValueError('K must be in 1..%d, got %d' % (n, K))
    root = list(range(2 * n - 1))
    for i in range(n - K):
        root[int(Z[i, 0])] = root[int(Z[i, 1])] = n + i
    for node in range(2 * n - 2, -1, -1):          # a merged cluster has a larger name than its parts: top down
        if root[node] != node:
            root[node] = root[root[node]]
    leaf = np.asarray(root[:n])
    uniq, first, inv = np.unique(leaf, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(1, len(uniq) + 1)
    return rank[inv.reshape(-1)]


def cdf_area(hist):
    """``(cdf (BINS + 1,) f64, area)``: ``cdf[b] = sum_{t <= b} hist[t] / sum(hist)`` (sum(hist) = N (N - 1) / 2) and ``area = (1 / BINS) sum_{b = 1..BINS}
    cdf[b]``, the area under the CDF of the consensus values."""
    h = np.asarray(hist).astype(np.uint64)
    total = int(h.sum())
    if total <= 0:
        raise ValueError('empty histogram')
    cdf = np.cumsum(h).astype(np.float64) / float(total)
    return cdf, float(cdf[1:].sum() / (len(h) - 1))


def delta_area(areas):
    """Monti's relative change of the area under the CDF, for ``areas`` = {K: A(K)}: the first K keeps its area, then ``(A(K) - A(K')) / A(K')`` with K' the
    K before it.  Returns {K: delta}."""
    out, prev = {}, None
    for k in sorted(areas):
        out[k] = float(areas[k]) if prev is None else float((areas[k] - areas[prev]) / areas[prev])
        prev = k
    return out


def consensus_summaries(rowsum, labels):
    """``(cluster_consensus (K,), item_consensus (N, K))`` from ``rowsum`` (N, K) and the 0-based ``labels``: the mean consensus of the pairs inside cluster c,
    and the mean consensus of point i with the members of cluster c other than itself (NaN where there is no such pair)."""
    n, K = rowsum.shape
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    inside = np.zeros(K)
    np.add.at(inside, labels, rowsum[np.arange(n), labels])
    with np.errstate(invalid='ignore', divide='ignore'):
        cluster = inside / (counts * (counts - 1))
        item = rowsum / (counts[None, :] - (labels[:, None] == np.arange(K)[None, :]))
    return cluster, item


class ConsensusKMeans:
    """Consensus clustering with a k-means base clusterer for every K of ``ks``.  After ``fit``: ``labels_`` {K: (N,) int64, 1-based}, ``cdf_`` {K: (BINS + 1,)},
    ``area_`` and ``delta_area_`` {K: float}, ``cluster_consensus_`` {K: (K,)}, ``item_consensus_`` {K: (N, K)}, ``linkage_`` {K: Z}, ``hist_`` {K: (BINS + 1,)
    uint64} and ``resamples_``.  Two fits with the same seed give the same bits; a device tensor and the numpy array of the same points too."""

    def __init__(self, ks, reps=100, p_item=0.8, n_init=1, seed=0):
        self.ks = sorted(int(k) for k in ks)
        if not self.ks or self.ks[0] < 2 or self.ks[-1] > min(MAX_K, N.MAX_CLUSTERS) or len(set(self.ks)) != len(self.ks):
            raise ValueError('ks must be distinct integers in 2..%d, got %r' % (min(MAX_K, N.MAX_CLUSTERS), ks))
        self.reps, self.p_item, self.n_init, self.seed = int(reps), float(p_item), int(n_init), int(seed)

    def fit(self, X, y=None):
        shape = tuple(X.shape)
        if len(shape) != 2:
            raise ValueError('expected a 2-D array, got shape %s' % (shape,))
        n, width = shape
        if width > MAX_DIM:
            raise NotImplementedError('consensus: at most %d features (got %d)' % (MAX_DIM, width))
        resamples = draw_resamples(n, self.reps, self.p_item, self.seed)
        if len(resamples[0]) < self.ks[-1] or n < 2:
            raise ValueError('a resample of %d points cannot be split into %d clusters' % (len(resamples[0]), self.ks[-1]))
        Xd = _as_device_matrix(X, _device())
        _require_bytes(8 * n * n, Xd.device, 'the consensus distance of %d points' % n)
        self.resamples_ = resamples
        self.labels_, self.cdf_, self.area_, self.hist_, self.linkage_, self.cluster_consensus_, self.item_consensus_ = {}, {}, {}, {}, {}, {}, {}
        for K in self.ks:
            L = label_matrix(Xd, K, resamples, self.n_init, self.seed)
            hist, _, D = consensus_pairs(L, want_distance=True)
            Z = average_linkage(D, overwrite=True)
            del D
            labels = cut_linkage(Z, K)
            _, rowsum, _ = consensus_pairs(L, y=labels - 1, want_hist=False, n_clusters=K)
            self.hist_[K], self.linkage_[K], self.labels_[K] = hist, Z, labels
            self.cdf_[K], self.area_[K] = cdf_area(hist)
            self.cluster_consensus_[K], self.item_consensus_[K] = consensus_summaries(rowsum, labels - 1)
        self.delta_area_ = delta_area(self.area_)
        return self
