"""``DensityPeaks`` (Rodriguez and Laio, "Clustering by fast search and find of density peaks", Science 2014) on the MI355X (csrc/dic_dpeaks.hip): the p2 / p4
``--cluster_method densitypeaks`` branches.

Every point gets a density ``rho`` and the distance ``delta`` to its nearest DENSER point; centres are the few points where both are large, and the
``(rho, delta)`` decision graph is the picture from which the number of clusters is read.  Every other point follows its nearest denser neighbour, and a halo
marks the points between clusters.  Like k-medoids, the centres are rows of X -- encounters that can be shown.  The definition is stated once in
include/dic_hip.h; sklearn has no counterpart.  The classical implementation needs the N x N distance matrix; here the densities come from the DBSCAN counting
pass (``density='cutoff'``) or the k-th neighbour distances (``'knn'``), and delta / parent from a masked nearest-neighbour join on the matrix cores: the points
are gathered into density order, so "denser" is ``column < row``; a bound pass and a candidate pass narrow every row to a short list that provably holds its
minimiser, and an exact f64 stage supplies every value and decides every tie.  Centre selection, label propagation (pointer doubling) and the halo rule run on
the host; the halo's border densities are one more pair pass on the workspace the counting pass left.

Outputs are NumPy.  The package imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM, MAX_SQ_THRESHOLD, _Counts, sq_threshold
from .kmedoids import _device_rows, _has_nan, _shape_of

_DENSITIES = ('cutoff', 'knn')


# -- the host side of the definition (no GPU) ------------------------------------------------------------------------------------------
def density_order(rho):
    """(order, rank): ``order[r]`` = the point of rank r, rank 0 the densest; i is denser than j iff rho_i > rho_j, or rho_i == rho_j and i < j."""
    rho = np.asarray(rho)
    order = np.argsort(-rho.astype(np.float64) if rho.dtype.kind == 'f' else -rho.astype(np.int64), kind='stable').astype(np.int64)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size, dtype=np.int64)
    return order, rank


def select_centres(rho, delta, rank, n_clusters=None, rho_min=None, delta_min=None):
    """The centres (original indices, int64) in the order of their ranks.  ``n_clusters=K``: the K largest gamma = rho delta, ties to the smaller rank; else
    every point with rho > rho_min and delta > delta_min (a bound left None does not constrain), and the densest point always."""
    rho, delta, rank = np.asarray(rho), np.asarray(delta, dtype=np.float64), np.asarray(rank)
    n = rank.size
    if n_clusters is not None:
        if rho_min is not None or delta_min is not None:
            raise ValueError('give either n_clusters or rho_min / delta_min, not both')
        k = _check_k(n_clusters, n)
        gamma = rho.astype(np.float64) * delta
        chosen = np.lexsort((rank, -gamma))[:k]
    else:
        if rho_min is None and delta_min is None:
            raise ValueError('give n_clusters, or rho_min and / or delta_min')
        keep = np.ones(n, dtype=bool)
        if rho_min is not None:
            keep &= rho > rho_min
        if delta_min is not None:
            keep &= delta > delta_min
        keep[rank == 0] = True
        chosen = np.flatnonzero(keep)
    return chosen[np.argsort(rank[chosen], kind='stable')].astype(np.int64)


def propagate_labels(parent, centres):
    """(N,) int64: a centre's root is itself, every other point takes its parent's root; the label is the root's position in ``centres``.  Pointer doubling:
    parents have smaller rank, so at most ceil(log2 N) + 1 rounds."""
    parent = np.asarray(parent, dtype=np.int64)
    centres = np.asarray(centres, dtype=np.int64)
    n = parent.size
    root = parent.copy()
    root[centres] = centres
    if (root < 0).any():
        raise ValueError('the densest point (parent -1) must be a centre')
    for _ in range(max(1, int(n).bit_length()) + 1):
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    slot = np.full(n, -1, dtype=np.int64)
    slot[centres] = np.arange(centres.size, dtype=np.int64)
    labels = slot[root]
    if (labels < 0).any():
        raise ValueError('parent holds a cycle: parents must have smaller rank')
    return labels


def halo_rule(rho, labels, border2):
    """(N,) bool: i is halo iff 2 rho_i < border2[label_i] (strict)."""
    return 2 * np.asarray(rho, dtype=np.int64) < np.asarray(border2, dtype=np.int64)[np.asarray(labels, dtype=np.int64)]


def gamma_gap(gamma, k):
    """gamma_(K) / gamma_(K+1) of the descending gammas: the gap that suggests K (inf where there is no K+1-th or it is 0)."""
    g = np.sort(np.asarray(gamma, dtype=np.float64))[::-1]
    if k < 1 or k > g.size:
        raise ValueError('k=%d outside 1..%d' % (k, g.size))
    if k == g.size or g[k] == 0:
        return float('inf')
    return float(g[k - 1] / g[k])


def _check_k(k, n):
    if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
        raise ValueError('n_clusters must be an int, got %r' % (k,))
    if k < 1:
        raise ValueError('n_clusters must be >= 1, got %d' % k)
    if n is not None and k > n:
        raise ValueError('n_clusters=%d must be <= n_samples=%d' % (k, n))
    return int(k)


def _check_input(X):
    """Shape, width and NaN checks that need no GPU."""
    n, width = _shape_of(X)
    if width > MAX_DIM:
        raise NotImplementedError('density peaks: at most %d features (got %d)' % (MAX_DIM, width))
    if n < 1 or width < 1:
        raise ValueError('density peaks needs at least 1 point of at least 1 feature, got shape %s' % ((n, width),))
    if _has_nan(X):
        raise ValueError('density peaks: X contains NaN')
    return n, width


# -- the device computation ------------------------------------------------------------------------------------------------------------
def delta_parent(xs, capacity=None):
    """dic_dpeaks_prepare + dic_dpeaks_delta on ``xs`` (N, D) f32 device rows in DENSITY ORDER: (delta (N) f64, parent (N) int32, cand (n_cand, 4) int32,
    stats), device tensors in rank space.  The candidate list grows when it overflows (the call is then run again)."""
    L = N.lib()
    n, d = xs.shape
    nbytes = int(L.dic_dpeaks_workspace(n, d))
    if nbytes == 0:
        raise ValueError('density peaks: N=%d, D=%d is outside the kernel\'s limits' % (n, d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xs.device)
    centre = xs.double().mean(dim=0).float().contiguous()
    st = N.stream_of(xs)
    N.check(L.dic_dpeaks_prepare(N.ptr(xs), xs.stride(0), n, d, N.ptr(centre), N.ptr(ws), ws.numel(), st), 'dic_dpeaks_prepare')
    delta = torch.empty(n, dtype=torch.float64, device=xs.device)
    parent = torch.empty(n, dtype=torch.int32, device=xs.device)
    cap = int(capacity) if capacity is not None else max(1 << 16, 16 * n)
    reruns = 0
    while True:
        cand = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=xs.device)
        nc = N.C.c_int64(0)
        stats = (N.C.c_int64 * 2)()
        rc = L.dic_dpeaks_delta(N.ptr(xs), xs.stride(0), n, d, N.ptr(cand), cap, N.ptr(delta), N.ptr(parent), N.C.byref(nc), stats, N.ptr(ws), ws.numel(), st)
        if rc == -3 and nc.value > cap:          # DIC_ERR_WORKSPACE: the list overflowed -- the passes again, with room for every candidate
            cap = int(nc.value)
            reruns += 1
            continue
        N.check(rc, 'dic_dpeaks_delta')
        break
    return delta, parent, cand[:int(nc.value)], {'candidates': int(stats[0]), 'longest_row': int(stats[1]), 'reruns': reruns}


class _Computation:
    """rho, delta and parent of one point set -- the ONE device computation every cut shares -- and what the halo pass needs (the counting pass's workspace
    and band list)."""

    def __init__(self, X, density, dc, percent, n_neighbors, shape=None):
        n, width = shape if shape is not None else _check_input(X)
        self.x = _device_rows(X)
        self.n, self.d0, self.d = n, width, self.x.shape[1]
        self.density, self.dc, self.counts = density, None, None
        if density == 'cutoff':
            if isinstance(dc, str):
                from .meanshift import estimate_bandwidth
                dc = estimate_bandwidth(self.x, quantile=percent / 100.0)          # (zero-padded columns change no distance)
            if not dc > 0:
                raise ValueError('density peaks: d_c = %r; pass dc > 0 (duplicated points make the k-th neighbour distance 0)' % (dc,))
            self.dc = float(dc)
            self.threshold = sq_threshold(self.dc)
            if not self.threshold < MAX_SQ_THRESHOLD:
                raise ValueError('density peaks: dc must be below 2^50, got %r' % (dc,))
            self.counts = _Counts(self.x, [self.threshold])
            self.rho = self.counts.counts[0].cpu().numpy().astype(np.int64) - 1
        else:
            from .knn import kth_neighbor_distance
            k = max(1, int(n * percent / 100.0)) if n_neighbors is None else n_neighbors
            if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)) or k < 1 or k > n:
                raise ValueError('n_neighbors must be an int in 1..n_samples=%d, got %r' % (n, k))
            self.kth = kth_neighbor_distance(self.x, int(k))
            mean = float(np.mean(self.kth, dtype=np.float64))
            self.rho = 1.0 / (1.0 + self.kth / mean) if mean > 0 else np.ones(n, dtype=np.float64)
        self.order, self.rank = density_order(self.rho)
        xs = self.x[torch.as_tensor(self.order, device=self.x.device)].contiguous()
        ds, ps, cand, self.stats = delta_parent(xs)
        self.candidates = cand
        ds, ps = ds.cpu().numpy(), ps.cpu().numpy().astype(np.int64)
        self.delta = np.empty(n, dtype=np.float64)
        self.delta[self.order] = ds
        self.parent = np.empty(n, dtype=np.int64)
        self.parent[self.order] = np.where(ps >= 0, self.order[np.maximum(ps, 0)], -1)
        self.gamma = self.rho.astype(np.float64) * self.delta

    def border2(self, labels, k):
        """border2 (k) int64 of the labels (dic_dpeaks_border, on the counting pass's workspace)."""
        cp, dev = self.counts, self.x.device
        lab = torch.as_tensor(labels.astype(np.int32), device=dev)
        rho = torch.as_tensor(self.rho.astype(np.int32), device=dev)
        out = torch.empty(k, dtype=torch.int32, device=dev)
        N.check(N.lib().dic_dpeaks_border(self.n, self.d, self.threshold, N.ptr(lab), N.ptr(rho), k, N.ptr(cp.band), cp.n_band, N.ptr(out), N.ptr(cp.ws),
                                          cp.ws.numel(), N.stream_of(lab)), 'dic_dpeaks_border')
        return out.cpu().numpy().astype(np.int64)


class DensityPeaks:
    def __init__(self, n_clusters=None, *, density='cutoff', dc='auto', percent=2.0, n_neighbors=None, rho_min=None, delta_min=None, halo=False):
        if n_clusters is not None:
            _check_k(n_clusters, None)
            if rho_min is not None or delta_min is not None:
                raise ValueError('give either n_clusters or rho_min / delta_min, not both')
        elif rho_min is None and delta_min is None:
            raise ValueError('give n_clusters, or rho_min and / or delta_min')
        if density not in _DENSITIES:
            raise ValueError('density must be one of %r, got %r' % (_DENSITIES, density))
        if isinstance(dc, str):
            if dc != 'auto':
                raise ValueError("dc must be 'auto' or a positive number, got %r" % (dc,))
        elif not dc > 0:
            raise ValueError("dc must be 'auto' or a positive number, got %r" % (dc,))
        if not 0 < percent <= 100:
            raise ValueError('percent must be in (0, 100], got %r' % (percent,))
        if halo and density != 'cutoff':
            raise ValueError("halo=True needs density='cutoff': the paper defines the border through d_c")
        self.n_clusters = None if n_clusters is None else int(n_clusters)
        self.density, self.dc, self.percent, self.n_neighbors = density, dc, float(percent), n_neighbors
        self.rho_min, self.delta_min, self.halo = rho_min, delta_min, bool(halo)

    def _cut(self, comp):
        if self.n_clusters is not None:
            _check_k(self.n_clusters, comp.n)
        self.rho_, self.delta_, self.parent_, self.gamma_, self.order_ = comp.rho, comp.delta, comp.parent, comp.gamma, comp.order
        self.dc_, self.n_candidates_, self.stats_ = comp.dc, comp.stats['candidates'], dict(comp.stats)
        self.n_features_in_ = comp.d0
        centres = select_centres(comp.rho, comp.delta, comp.rank, self.n_clusters, self.rho_min, self.delta_min)
        k = centres.size
        self.center_indices_ = centres
        self.cluster_centers_ = comp.x[torch.as_tensor(centres, device=comp.x.device), :comp.d0].cpu().numpy()
        self.core_labels_ = propagate_labels(comp.parent, centres)
        self.gamma_gap_ = gamma_gap(comp.gamma, k)
        if self.halo:
            b2 = comp.border2(self.core_labels_, k)
            self.border_density_ = b2.astype(np.float64) / 2.0
            self.halo_ = halo_rule(comp.rho, self.core_labels_, b2)
        else:
            self.border_density_ = None
            self.halo_ = np.zeros(comp.n, dtype=bool)
        self.labels_ = np.where(self.halo_, -1, self.core_labels_)
        return self

    def fit(self, X, y=None):
        shape = _check_input(X)
        if self.n_clusters is not None:
            _check_k(self.n_clusters, shape[0])
        return self._cut(_Computation(X, self.density, self.dc, self.percent, self.n_neighbors, shape))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        """(N,) int64 numpy: the slot of the nearest centre of every row, ties to the smaller slot (``knn.kneighbors``: exact)."""
        if not hasattr(self, 'cluster_centers_'):
            raise RuntimeError('This DensityPeaks instance is not fitted yet.')
        n, width = _check_input(X)
        if width != self.n_features_in_:
            raise ValueError('X has %d features, but DensityPeaks is expecting %d features as input.' % (width, self.n_features_in_))
        from .knn import kneighbors
        _, idx = kneighbors(self.cluster_centers_, 1, Q=X)
        return idx[:, 0].astype(np.int64)

    def decision_graph(self):
        """(rho, delta, gamma): the decision graph, one entry per point."""
        if not hasattr(self, 'rho_'):
            raise RuntimeError('This DensityPeaks instance is not fitted yet.')
        return self.rho_, self.delta_, self.gamma_

    def reorder(self, order):
        """Renumber the clusters: new cluster j is old cluster ``order[j]`` (p4 orders them by systolic pressure)."""
        order = np.asarray(order, dtype=np.int64)
        k = self.center_indices_.size
        if sorted(order.tolist()) != list(range(k)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (k - 1, order.tolist()))
        self.cluster_centers_ = self.cluster_centers_[order].copy()
        self.center_indices_ = self.center_indices_[order].copy()
        if self.border_density_ is not None:
            self.border_density_ = self.border_density_[order].copy()
        inverse = np.empty_like(order)
        inverse[order] = np.arange(k)
        self.core_labels_ = inverse[self.core_labels_]
        self.labels_ = np.where(self.labels_ >= 0, inverse[np.maximum(self.labels_, 0)], -1)
        return self

    def get_params(self, deep=True):
        return dict(n_clusters=self.n_clusters, density=self.density, dc=self.dc, percent=self.percent, n_neighbors=self.n_neighbors, rho_min=self.rho_min,
                    delta_min=self.delta_min, halo=self.halo)


def density_peaks_sweep(X, ks, **kw):
    """{K: fitted ``DensityPeaks(K, **kw)``}: ONE device computation of rho, delta and parent, one cut per K on the host (with ``halo=True`` one border pass
    per K on top).  ``gamma_gap_`` of every model is gamma_(K) / gamma_(K+1), the gap that suggests K."""
    ks = [int(k) for k in ks]
    if not ks:
        return {}
    shape = _check_input(X)
    models = {k: DensityPeaks(k, **kw) for k in ks}
    for k in ks:
        _check_k(k, shape[0])
    first = models[ks[0]]
    comp = _Computation(X, first.density, first.dc, first.percent, first.n_neighbors, shape)
    return {k: models[k]._cut(comp) for k in ks}
