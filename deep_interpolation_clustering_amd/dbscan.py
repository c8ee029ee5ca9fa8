"""DBSCAN on the MI355X without the distance matrix (p2_clustering_optK.py:82-85,90-168, p4_clustering_final.py:181-236).

Upstream fits ``sklearn.cluster.DBSCAN(eps, min_samples, metric='precomputed')`` on ``pairwise_distances(X)`` -- an N x N f32 matrix (22.5 GB at
75 000 points).  Here the pairs are recomputed tile by tile on the matrix cores (csrc/dic_dbscan.hip): one counting pass for every eps of a sweep, then per
eps a few label passes over the core graph, whose last one also yields the border points.  The neighbour rule is sklearn's, bit for bit: ``dist <= eps``
with ``dist`` the f32 ``np.sqrt`` of the f32-rounded squared distance, and eps compared under NumPy's promotion of the caller's eps object (a Python
``float`` compares in f32, a NumPy ``float64`` in f64) -- each eps becomes one f32 threshold on the squared distance (``sq_threshold``).  Pairs the split-bf16
products cannot decide are rechecked exactly in f64 on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

MAX_EPS_PER_PASS = 16           # dic_dbscan_counts: thresholds per counting pass
MAX_DIM = 256
MAX_SQ_THRESHOLD = 2.0 ** 100   # dic_dbscan_counts: squared-distance thresholds stay below it (the padding points sit at 2^120), i.e. eps < 2^50


def sq_threshold(eps):
    """The largest f32 ``s`` with ``np.sqrt(np.float32(s)) <= eps`` (``eps`` as the caller passed it: its NumPy promotion decides the comparison)."""
    if not eps > 0:
        raise ValueError('eps must be > 0, got %r' % (eps,))
    s = np.float32(float(eps) * float(eps))
    inf = np.float32(np.inf)
    while not np.sqrt(s) <= eps:
        s = np.nextafter(s, np.float32(0))
    while True:
        nxt = np.nextafter(s, inf)
        if not np.sqrt(nxt) <= eps:
            return float(s)
        s = nxt


def _device_points(X):
    x = torch.as_tensor(X)
    if x.dim() != 2:
        raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (tuple(x.shape),))
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('deep_interpolation_clustering_amd.dbscan runs only on an MI355X; there is no CPU path by design')
        x = x.to('cuda')
    x = x.to(torch.float32)
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))          # zero columns change no distance
    return x.contiguous()


class _Counts:
    """One counting pass: the device points, workspace, counts (n_eps, N) int32 and the band list, kept for the label passes."""

    def __init__(self, x, thresholds, band_capacity=None):
        L = N.lib()
        n, d = x.shape
        self.x, self.n, self.d, self.thresholds = x, n, d, [float(t) for t in thresholds]
        ne = len(self.thresholds)
        self.ws = torch.empty(max(16, L.dic_dbscan_workspace(n, d)), dtype=torch.uint8, device=x.device)
        self.counts = torch.empty((ne, n), dtype=torch.int32, device=x.device)
        centre = x.mean(0, keepdim=True, dtype=torch.float64).float().contiguous()
        cap = int(band_capacity) if band_capacity is not None else max(1 << 16, 16 * n)
        thr = (N.C.c_float * ne)(*self.thresholds)
        self.reruns = 0
        while True:
            band = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=x.device)
            nb = N.C.c_int64(0)
            rc = L.dic_dbscan_counts(N.ptr(x), x.stride(0), N.ptr(centre), n, d, thr, ne, N.ptr(self.counts), N.ptr(band), cap, N.C.byref(nb),
                                     N.ptr(self.ws), self.ws.numel(), N.stream_of(x))
            if rc == -3 and nb.value > cap:          # DIC_ERR_WORKSPACE: the band list overflowed -- the whole pass again, with room for every band pair
                cap = nb.value
                self.reruns += 1
                continue
            N.check(rc, 'dic_dbscan_counts')
            break
        self.band, self.n_band = band, int(nb.value)

    def components(self, e, min_samples):
        """(labels (N) int64 numpy in sklearn's numbering, core mask (N) bool numpy, label passes) of eps ``e``."""
        L = N.lib()
        cnt = self.counts[e].contiguous()
        core = cnt >= min_samples
        n = self.n
        passes = 0
        dev = self.x.device
        lab = torch.arange(n, dtype=torch.int32, device=dev)
        border = torch.empty(n, dtype=torch.int32, device=dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        if bool(core.any()):
            while True:
                changed.zero_()
                N.check(L.dic_dbscan_components_pass(n, self.d, self.thresholds[e], e, N.ptr(cnt), int(min_samples), N.ptr(self.band), self.n_band,
                                                     N.ptr(lab), N.ptr(border), N.ptr(changed), N.ptr(self.ws), self.ws.numel(), N.stream_of(cnt)),
                        'dic_dbscan_components_pass')
                passes += 1
                if int(changed.item()) == 0:
                    break
        out = torch.full((n,), -1, dtype=torch.int64, device=dev)
        if passes:
            roots = torch.unique(lab[core].to(torch.int64), sorted=True)             # cluster id = rank of the smallest core index of the component
            out[core] = torch.searchsorted(roots, lab[core].to(torch.int64))
            bmask = (~core) & (border < n)
            out[bmask] = torch.searchsorted(roots, border[bmask].to(torch.int64))
        return out.cpu().numpy(), core.cpu().numpy(), passes


def dbscan_sweep(X, eps_values, min_samples, band_capacity=None, stats=None):
    """DBSCAN of ``X`` for every eps of ``eps_values`` with one counting pass (up to 16 eps per pass): a list of ``(labels, core_sample_indices)`` numpy
    int64 pairs, each identical to ``sklearn.cluster.DBSCAN(eps, min_samples=min_samples, metric='precomputed').fit(pairwise_distances(X))``.  ``stats``
    (a dict, optional) receives ``band_pairs``, ``components_passes`` (per eps) and ``counts_reruns``."""
    min_samples = int(min_samples)
    if min_samples < 1:
        raise ValueError('min_samples must be >= 1, got %d' % min_samples)
    eps_values = list(eps_values)
    thresholds = [sq_threshold(e) for e in eps_values]
    for e, t in zip(eps_values, thresholds):
        if not t < MAX_SQ_THRESHOLD:
            raise ValueError('dbscan: eps must be below 2^50 (about 1.1e15), got %r' % (e,))
    x = _device_points(X)
    if x.shape[1] > MAX_DIM:
        raise NotImplementedError('dbscan: at most %d features (got %d)' % (MAX_DIM, x.shape[1]))
    out = []
    if stats is not None:
        stats.setdefault('band_pairs', [])
        stats.setdefault('components_passes', [])
        stats.setdefault('counts_reruns', 0)
    for g in range(0, len(eps_values), MAX_EPS_PER_PASS):
        group = thresholds[g:g + MAX_EPS_PER_PASS]
        cp = _Counts(x, group, band_capacity)
        for e in range(len(group)):
            labels, core, passes = cp.components(e, min_samples)
            out.append((labels, np.flatnonzero(core).astype(np.int64)))
            if stats is not None:
                stats['components_passes'].append(passes)
        if stats is not None:
            stats['band_pairs'].append(cp.n_band)
            stats['counts_reruns'] += cp.reruns
        del cp
    return out


class DBSCAN:
    """``sklearn.cluster.DBSCAN`` (euclidean) on the MI355X: ``fit`` sets ``labels_`` (N) int64, ``core_sample_indices_`` (sorted int64) and
    ``components_`` (= X[core]), identical to sklearn's fit on ``pairwise_distances(X)`` with ``metric='precomputed'``."""

    def __init__(self, eps=0.5, min_samples=5, metric='euclidean', *, metric_params=None, algorithm='auto', leaf_size=30, p=None, n_jobs=None,
                 band_capacity=None):
        if metric == 'precomputed':
            raise NotImplementedError("metric='precomputed' is not supported: pass the points themselves -- the distances are recomputed on the GPU, "
                                      'which is what spares the N x N matrix')
        if metric != 'euclidean' or metric_params is not None or p not in (None, 2):
            raise NotImplementedError('only the euclidean metric is on the accelerated path')
        self.eps, self.min_samples, self.metric = eps, min_samples, metric
        self.metric_params, self.algorithm, self.leaf_size, self.p, self.n_jobs = metric_params, algorithm, leaf_size, p, n_jobs
        self.band_capacity = band_capacity
        self.stats_ = None

    def fit(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError('sample_weight is not supported on the accelerated path')
        self.stats_ = {}
        (labels, core), = dbscan_sweep(X, [self.eps], self.min_samples, self.band_capacity, self.stats_)
        self.labels_ = labels
        self.core_sample_indices_ = core
        Xn = X.detach().cpu().numpy() if torch.is_tensor(X) else np.asarray(X)
        self.components_ = Xn[core].copy()
        return self

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_
