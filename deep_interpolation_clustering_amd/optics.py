"""OPTICS on the MI355X without the distance matrix (p2_clustering_optK.py:86-88,171-223).

Upstream fits ``sklearn.cluster.OPTICS`` on the CPU: N strictly sequential steps of O(N) each, on top of an N x N ``pairwise_distances`` matrix (45 GB in
f64 at 75 000 points).  Here the core distances come from ``knn.kth_neighbor_distance`` and every step of the main loop is one row pass over the points on
the device (csrc/dic_optics.hip): the distances of the current point are recomputed, reachability and predecessor updated, and the next point found, in one
launch; the N launches are enqueued back to back and the host reads the result once.

The definition is sklearn's in its self-consistent form -- ``OPTICS(metric='precomputed').fit(D)`` with ``D`` the f64 difference-form distances of the f32
points: one distance function serves the core distances and the steps (bit for bit, and symmetric), so the many ties the algorithm produces (every
neighbour inside a point's core radius is reached at exactly its core distance) are broken by index, as sklearn's ``argmin`` breaks them.  ``fit(X)`` of
sklearn mixes two distance routines (a GEMM-form k-NN query and ``cdist``) and is not self-consistent in that sense; its labels agree, its ordering need not.

The label extraction (``cluster_optics_dbscan``, ``cluster_optics_xi``) runs on the host in numpy: it is O(N) with short scalar loops (0.5 s at 75 000
points in sklearn) and restates sklearn's; the package does not import sklearn.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from . import knn
from .dbscan import MAX_DIM, _device_points


def around15(v):
    """``np.around(v, 15)`` -- sklearn rounds core and reachability distances to f64's 15 decimal digits: multiply by 1e15, rint, divide by 1e15."""
    return np.around(np.asarray(v, dtype=np.float64), 15)


def _resolve_size(size, n, name):
    """sklearn's rule for ``min_samples`` / ``min_cluster_size``: an integer >= 2 as it stands, a float in [0, 1] as the fraction ``max(2, int(f * n))``;
    more than ``n`` is an error."""
    if isinstance(size, bool) or not isinstance(size, numbers.Real):
        raise ValueError('%s must be an int >= 2 or a float in [0, 1], got %r' % (name, size))
    if isinstance(size, numbers.Integral):
        if size < 2:
            raise ValueError('%s must be an int >= 2 or a float in [0, 1], got %r' % (name, size))
    elif not 0 <= size <= 1:
        raise ValueError('%s must be an int >= 2 or a float in [0, 1], got %r' % (name, size))
    if size > n:
        raise ValueError('%s must be no greater than the number of samples (%d). Got %d' % (name, n, size))
    if size <= 1:
        size = max(2, int(size * n))
    return int(size)


def device_walk(x, core, workspace, entry, *params, stats=None):
    """The walk OPTICS and HDBSCAN share (csrc/dic_gridstep.h), enqueued by the C entry point ``entry`` on a workspace sized by the C function
    ``workspace``: ``x`` the device points (``_device_points``), ``core`` (N,) f64 numpy, ``params`` what ``entry`` takes between ``core`` and
    ``ordering``.  Returns ``(ordering int64, reach f64, pred int64)``, numpy; ``stats['steps']`` receives the launches of the walk."""
    L = N.lib()
    n, d = x.shape
    dev = x.device
    core_d = torch.as_tensor(core, device=dev)
    ws = torch.empty(max(16, getattr(L, workspace)(n, d)), dtype=torch.uint8, device=dev)
    ordering = torch.empty(n, dtype=torch.int32, device=dev)
    reach = torch.empty(n, dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    N.check(getattr(L, entry)(N.ptr(x), x.stride(0), n, d, N.ptr(core_d), *params, N.ptr(ordering), N.ptr(reach), N.ptr(pred), N.ptr(ws), ws.numel(),
                              N.stream_of(x)), entry)
    if stats is not None:
        stats['steps'] = n - 1
    return ordering.cpu().numpy().astype(np.int64), reach.cpu().numpy(), pred.cpu().numpy().astype(np.int64)


def optics_graph(X, min_samples, max_eps=np.inf, stats=None):
    """``sklearn.cluster.compute_optics_graph`` (euclidean): ``(ordering int64, core_distances f64, reachability f64, predecessor int64)``, numpy, each (N,).
    ``X`` (numpy array or tensor, (N, D), D <= 256); a tensor on the device gives the same bits as the numpy array.  ``stats`` (a dict, optional) receives the
    k-NN phase's counters and ``steps``, the launches of the main loop."""
    n, width = knn._shape_of(X)
    if width > MAX_DIM:
        raise NotImplementedError('optics: at most %d features (got %d)' % (MAX_DIM, width))
    k = _resolve_size(min_samples, n, 'min_samples')
    max_eps = float(max_eps)
    if not max_eps >= 0:
        raise ValueError('max_eps must be >= 0, got %r' % (max_eps,))
    if k > n:          # (a fraction of a tiny set: max(2, .) exceeds it -- sklearn fails in its neighbour query with this message)
        raise ValueError('Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d' % (k, n))
    x = _device_points(X)
    core = knn.kth_neighbor_distance(x, k, stats=stats)
    core[core > max_eps] = np.inf
    core = around15(core)
    ordering, reach, pred = device_walk(x, core, 'dic_optics_workspace', 'dic_optics_order', max_eps, stats=stats)
    return ordering, core, reach, pred


def cluster_optics_dbscan(*, reachability, core_distances, ordering, eps):
    """``sklearn.cluster.cluster_optics_dbscan``: the DBSCAN labels at ``eps`` read off the OPTICS graph.  Walking the ordering, a point that cannot be
    reached within eps but is itself a core point at eps opens the next cluster; everything up to the next such point belongs to it, except the points that
    are neither reachable nor core at eps -- noise."""
    reachability, core_distances, ordering = np.asarray(reachability), np.asarray(core_distances), np.asarray(ordering)
    unreachable = reachability > eps
    core = core_distances <= eps
    labels = np.zeros(len(core_distances), dtype=int)
    labels[ordering] = np.cumsum((unreachable & core)[ordering]) - 1
    labels[unreachable & ~core] = -1
    return labels


def _steep_area_end(steep, opposite, start, patience):
    """The last steep point of the maximal steep area that begins at ``start`` (Ankerst et al. 1999, definition 10): the area runs on over steep points and over
    non-steep ones that do not turn the other way, at most ``patience`` of the latter in a row; a point going the ``opposite`` way ends it at once."""
    last, idle = start, 0
    for i in range(start, len(steep)):
        if steep[i]:
            last, idle = i, 0
        elif opposite[i]:
            break
        else:
            idle += 1
            if idle > patience:
                break
    return last


def _xi_clusters(plot, pred_plot, ordering, xi, min_samples, min_cluster_size, predecessor_correction):
    """The xi-steep clusters of a reachability plot (figure 19 of the OPTICS paper with sklearn's corrections): ``(n, 2)`` inclusive [start, end] positions
    in the ordering, nested clusters before the ones that hold them."""
    n = len(plot)
    plot = np.append(plot, np.inf)          # a closing upward step, so that a cluster at the very end is seen
    keep = 1 - xi
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = plot[:-1] / plot[1:]
    steep_up, steep_down = ratio <= keep, ratio >= 1 / keep
    up, down = ratio < 1, ratio > 1
    position = np.full(n + 1, -1, dtype=np.int64)          # position[point] in the ordering; slot n takes the predecessor -1
    position[ordering] = np.arange(n)
    down_areas = []          # [start, end, maximum in between since the area ended]
    clusters = []
    index, mib = 0, 0.0
    for at in np.flatnonzero(steep_up | steep_down):
        at = int(at)
        if at < index:          # inside an area already walked
            continue
        mib = max(mib, float(plot[index:at + 1].max()))
        # a down area survives only while nothing in between rose above its start by the factor 1 - xi
        if np.isinf(mib):
            down_areas = []
        else:
            down_areas = [a for a in down_areas if mib <= plot[a[0]] * keep]
            for a in down_areas:
                a[2] = max(a[2], mib)
        if steep_down[at]:
            end = _steep_area_end(steep_down, up, at, min_samples)
            down_areas.append([at, end, 0.0])
            index = end + 1
            mib = float(plot[index])
            continue
        u_start, u_end = at, _steep_area_end(steep_up, down, at, min_samples)
        index = u_end + 1
        mib = float(plot[index])
        found = []
        for d_start, d_end, d_mib in down_areas:
            s, e = d_start, u_end
            after = plot[e + 1]
            if after * keep < d_mib:          # something between the two areas is too high for this pair
                continue
            top = plot[d_start]
            if top * keep >= after:          # the down area starts much higher than the cluster ends: move the start down to that level
                while plot[s + 1] > after and s < d_end:
                    s += 1
            elif after * keep >= top:          # the up area ends much higher than the cluster starts: move the end down to that level
                while plot[e - 1] > top and e > u_start:
                    e -= 1
            if predecessor_correction:          # Schubert & Gertz 2018, algorithm 2: drop trailing points whose predecessor lies outside the cluster
                while s < e and not plot[s] > plot[e] and not s <= position[pred_plot[e]] < e:
                    e -= 1
                if not s < e:
                    continue
            if e - s + 1 < min_cluster_size or s > d_end or e < u_start:
                continue
            found.append((s, e))
        clusters.extend(reversed(found))          # the areas are listed outermost first: the smaller clusters go first
    return np.array(clusters, dtype=np.int64).reshape(-1, 2)


def cluster_optics_xi(*, reachability, predecessor, ordering, min_samples, min_cluster_size=None, xi=0.05, predecessor_correction=True):
    """``sklearn.cluster.cluster_optics_xi``: ``(labels (N,) int, cluster_hierarchy (n_clusters, 2) int)``.  The hierarchy lists every xi-steep cluster as
    inclusive [start, end] positions in the ordering, inner clusters first; the labels number, in that order, the clusters that overlap no cluster
    numbered before them -- the leaves -- and leave every other point at -1."""
    reachability, predecessor, ordering = np.asarray(reachability), np.asarray(predecessor), np.asarray(ordering)
    n = len(reachability)
    min_samples = _resolve_size(min_samples, n, 'min_samples')
    min_cluster_size = min_samples if min_cluster_size is None else _resolve_size(min_cluster_size, n, 'min_cluster_size')
    if not 0 <= xi <= 1:
        raise ValueError('xi must be in [0, 1], got %r' % (xi,))
    clusters = _xi_clusters(reachability[ordering], predecessor[ordering], ordering, xi, min_samples, min_cluster_size, predecessor_correction)
    along = np.full(n, -1, dtype=int)
    label = 0
    for s, e in clusters:
        if (along[s:e + 1] == -1).all():
            along[s:e + 1] = label
            label += 1
    labels = np.empty(n, dtype=int)
    labels[ordering] = along
    return labels, clusters


class OPTICS:
    """``sklearn.cluster.OPTICS`` (euclidean) on the MI355X: ``fit`` sets ``ordering_``, ``core_distances_``, ``reachability_``, ``predecessor_``, ``labels_``
    and, for ``cluster_method='xi'``, ``cluster_hierarchy_`` -- what sklearn's fit on the f64 distance matrix with ``metric='precomputed'`` gives."""

    def __init__(self, *, min_samples=5, max_eps=np.inf, metric='euclidean', p=2, metric_params=None, cluster_method='xi', eps=None, xi=0.05,
                 predecessor_correction=True, min_cluster_size=None, algorithm='auto', leaf_size=30, memory=None, n_jobs=None):
        if metric == 'precomputed':
            raise NotImplementedError("metric='precomputed' is not supported: pass the points themselves -- the distances are recomputed on the GPU, "
                                      'which is what spares the N x N matrix')
        if metric not in ('euclidean', 'minkowski') or metric_params is not None or p not in (None, 2):
            raise NotImplementedError('only the euclidean metric is on the accelerated path')
        if cluster_method not in ('xi', 'dbscan'):
            raise ValueError("cluster_method must be 'xi' or 'dbscan', got %r" % (cluster_method,))
        self.min_samples, self.max_eps, self.metric, self.p, self.metric_params = min_samples, max_eps, metric, p, metric_params
        self.cluster_method, self.eps, self.xi, self.predecessor_correction = cluster_method, eps, xi, predecessor_correction
        self.min_cluster_size, self.algorithm, self.leaf_size, self.memory, self.n_jobs = min_cluster_size, algorithm, leaf_size, memory, n_jobs
        self.stats_ = None

    def fit(self, X, y=None):
        eps = self.max_eps if self.eps is None else self.eps
        if self.cluster_method == 'dbscan' and eps > self.max_eps:
            raise ValueError('Specify an epsilon smaller than %s. Got %s.' % (self.max_eps, eps))
        self.stats_ = {}
        self.ordering_, self.core_distances_, self.reachability_, self.predecessor_ = optics_graph(X, self.min_samples, self.max_eps, self.stats_)
        if self.cluster_method == 'xi':
            self.labels_, self.cluster_hierarchy_ = cluster_optics_xi(
                reachability=self.reachability_, predecessor=self.predecessor_, ordering=self.ordering_, min_samples=self.min_samples,
                min_cluster_size=self.min_cluster_size, xi=self.xi, predecessor_correction=self.predecessor_correction)
        else:
            self.labels_ = cluster_optics_dbscan(reachability=self.reachability_, core_distances=self.core_distances_, ordering=self.ordering_, eps=eps)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
