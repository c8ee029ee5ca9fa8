"""Shared-nearest-neighbour (SNN) clustering on the MI355X (no upstream counterpart): density clustering in which two points are as close as the number of
their k nearest neighbours they share -- an integer rank statistic without a scale, the standard remedy where euclidean distances concentrate (D = 256) and
DBSCAN's eps flips from "everything is noise" to "one cluster" within a narrow band.  Jarvis & Patrick, "Clustering using a similarity measure based on
shared near neighbors", 1973; Ertoz, Steinbach & Kumar, "Finding clusters of different sizes, shapes, and densities in noisy, high dimensional data", 2003.

The definition is stated once, in include/dic_hip.h (dic_snn_similarity); in short, with L(i) the k-neighbour list of i from ``knn.kneighbors`` (the point
itself an ordinary neighbour):  sim(i, j) = |L(i) n L(j)| where each is in the other's list, else 0;  density(i) = the number of j with sim(i, j) >= eps;
core: density >= min_samples;  clusters: components of the cores under sim >= eps, numbered by their smallest core index;  a non-core point with such an
edge to a core joins the core of largest sim (the smaller index on equal sim);  the rest is noise, -1.  ``min_samples=0`` makes every point core: that IS
Jarvis-Patrick clustering -- the components of the mutual k-neighbour graph thresholded at eps, isolated points as singleton clusters.

Nothing N x N exists: one pass over the lists gives the (N, k) similarities (csrc/dic_snn.hip), a few label passes per eps the components.  Every result is
an integer and does not depend on the run.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .knn import _check_k, _shape_of, kneighbors


def _check_params(k, eps_values, min_samples):
    """``(eps list, min_samples)`` as ints; k is the list length."""
    out = []
    for eps in eps_values:
        if int(eps) != eps:
            raise ValueError('eps must be an integer (a count of shared neighbours), got %r' % (eps,))
        if not 1 <= int(eps) <= k:
            raise ValueError('eps must lie in [1, n_neighbors = %d], got %r' % (k, eps))
        out.append(int(eps))
    if int(min_samples) != min_samples or int(min_samples) < 0:
        raise ValueError('min_samples must be an integer >= 0, got %r' % (min_samples,))
    return out, int(min_samples)


def _check_x(X, n_neighbors, candidate_budget=None):
    n, d = _shape_of(X)
    if n < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (n, d))
    if int(n_neighbors) != n_neighbors:
        raise ValueError('n_neighbors must be an integer, got %r' % (n_neighbors,))
    k = int(n_neighbors)
    if k < 2:
        raise ValueError('snn: n_neighbors must be >= 2 (the point itself is the first neighbour), got %d' % k)
    _check_k(k, n, n)
    if candidate_budget is not None and int(candidate_budget) < 1:
        raise ValueError('candidate_budget must be positive, got %r' % (candidate_budget,))
    if d > MAX_DIM:
        raise NotImplementedError('snn: at most %d features (got %d)' % (MAX_DIM, d))
    return k


def _device_lists(idx, sim=None):
    """(N, k) int32 contiguous device tensors of neighbour lists (and similarities) given as numpy arrays or tensors."""
    out = []
    for name, a in (('idx', idx), ('sim', sim)):
        if a is None:
            continue
        t = torch.as_tensor(a.copy() if isinstance(a, np.ndarray) and not a.flags.writeable else a)          # (torch warns about read-only arrays)
        if t.dim() != 2:
            raise ValueError('%s must be 2-D (n_samples, n_neighbors), got shape %s' % (name, tuple(t.shape)))
        if t.dtype.is_floating_point or t.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError('%s must be integers, got %s' % (name, t.dtype))
        out.append(t)
    n, k = out[0].shape
    if len(out) == 2 and out[1].shape != out[0].shape:
        raise ValueError('idx and sim must have one shape, got %s and %s' % (tuple(out[0].shape), tuple(out[1].shape)))
    if n < 1 or k < 2 or k > n:
        raise ValueError('snn: lists of shape (%d, %d): expected 2 <= n_neighbors <= n_samples' % (n, k))
    _check_k(k, n, n)
    return out


def _to_device(tensors):
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('deep_interpolation_clustering_amd.snn runs only on an MI355X; there is no CPU path by design')
        dev = torch.device('cuda', torch.cuda.current_device())
    return [t.to(device=dev, dtype=torch.int32).contiguous() for t in tensors]


def snn_similarity(idx):
    """``sim`` (N, k) int32 on the device for neighbour lists ``idx`` (N, k) (numpy array or tensor; ``knn.kneighbors(X, k)[1]`` of the self join): the
    kernel alone.  Entries outside [0, N) count as absent."""
    idx, = _to_device(_device_lists(idx))
    n, k = idx.shape
    sim = torch.empty_like(idx)
    N.check(N.lib().dic_snn_similarity(N.ptr(idx), n, k, N.ptr(sim), N.stream_of(idx)), 'dic_snn_similarity')
    return sim


def snn_graph(X, n_neighbors, candidate_budget=None, return_device=False):
    """``(idx (N, k) int32, sim (N, k) int32)``: the k-neighbour lists of ``X`` (numpy array or tensor, (N, D), D <= 256; 2 <= k <= min(N, 1024)) and the
    shared-neighbour similarity of every list entry (0 for the point itself and for a pair that is not mutual).  numpy, or device tensors with
    ``return_device=True``.  ``candidate_budget`` as for ``knn.kneighbors``: it never changes the result."""
    k = _check_x(X, n_neighbors, candidate_budget)
    dist, idx = kneighbors(X, k, candidate_budget=candidate_budget, return_device=True)
    del dist          # (N, k) f64, twice the lists: gone before sim is allocated (154 MB against 77 + 77 at 75 000 x 257)
    sim = snn_similarity(idx)
    if return_device:
        return idx, sim
    return idx.cpu().numpy(), sim.cpu().numpy()


def _label(idx, sim, eps, min_samples):
    """``(labels int64, core_sample_indices int64, density int32, label passes)`` of one eps on device lists."""
    L = N.lib()
    n, k = idx.shape
    dev = idx.device
    density = (sim >= eps).sum(1, dtype=torch.int32)
    core = density >= min_samples
    lab = torch.arange(n, dtype=torch.int32, device=dev)
    border = torch.empty(n, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    passes = 0
    out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if bool(core.any()):
        while True:
            changed.zero_()
            N.check(L.dic_snn_components_pass(N.ptr(idx), N.ptr(sim), n, k, eps, N.ptr(density), min_samples, N.ptr(lab), N.ptr(border), N.ptr(changed),
                                              N.stream_of(idx)), 'dic_snn_components_pass')
            passes += 1
            if int(changed.item()) == 0:
                break
        lab64 = lab.to(torch.int64)
        roots = torch.unique(lab64[core], sorted=True)             # cluster id = rank of the smallest core index of the component
        out[core] = torch.searchsorted(roots, lab64[core])
        bmask = (~core) & (border >= 0)
        out[bmask] = torch.searchsorted(roots, lab64[border[bmask].to(torch.int64)])
    return out.cpu().numpy(), torch.nonzero(core).flatten().cpu().numpy().astype(np.int64), density.cpu().numpy(), passes


def snn_labels(idx, sim, eps, min_samples):
    """``(labels (N) int64, core_sample_indices int64, density (N) int32)``, numpy, of the graph ``(idx, sim)`` -- device tensors from ``snn_graph``, or numpy
    arrays -- at the integer threshold ``eps`` (1 <= eps <= k) and ``min_samples`` >= 0 (0: Jarvis-Patrick, every point core)."""
    lists = _device_lists(idx, sim)
    (eps,), min_samples = _check_params(lists[0].shape[1], [eps], min_samples)
    idx, sim = _to_device(lists)
    return _label(idx, sim, eps, min_samples)[:3]


def snn_sweep(X, n_neighbors, eps_values, min_samples, stats=None, candidate_budget=None):
    """SNN clustering of ``X`` for every eps of ``eps_values`` on ONE graph: a list of ``(labels, core_sample_indices, density)`` numpy triples, each what
    ``SNN(n_neighbors, eps, min_samples).fit(X)`` sets.  ``stats`` (a dict, optional) receives ``label_passes`` (per eps) and ``similarity_hist`` ((k + 1)
    int64: the list entries per similarity 0..k, the self entries and the pairs that are not mutual at 0 -- the curve eps is read from)."""
    k = _check_x(X, n_neighbors, candidate_budget)
    eps_values, min_samples = _check_params(k, list(eps_values), min_samples)
    idx, sim = snn_graph(X, k, candidate_budget, return_device=True)
    if stats is not None:
        stats.setdefault('label_passes', [])
        stats['similarity_hist'] = torch.bincount(sim.flatten().long(), minlength=k + 1).cpu().numpy()
    out = []
    for eps in eps_values:
        labels, core, density, passes = _label(idx, sim, eps, min_samples)
        out.append((labels, core, density))
        if stats is not None:
            stats['label_passes'].append(passes)
    return out


class SNN:
    """Shared-nearest-neighbour clustering (module docstring).  ``fit`` sets ``labels_`` (N) int64 (-1: noise), ``core_sample_indices_`` (sorted int64),
    ``density_`` (N) int32, ``neighbors_`` (N, k) int32 (the lists) and ``stats_``; ``similarity_`` (N, k) int32 stays on the device until it is asked
    for.  ``min_samples=0`` is Jarvis-Patrick clustering."""

    def __init__(self, n_neighbors=20, eps=10, min_samples=5, candidate_budget=None):
        self.n_neighbors, self.eps, self.min_samples, self.candidate_budget = n_neighbors, eps, min_samples, candidate_budget
        self.stats_ = None
        self._sim = self._sim_host = None

    def fit(self, X, y=None):
        k = _check_x(X, self.n_neighbors, self.candidate_budget)
        (eps,), min_samples = _check_params(k, [self.eps], self.min_samples)
        idx, sim = snn_graph(X, k, self.candidate_budget, return_device=True)
        self.labels_, self.core_sample_indices_, self.density_, passes = _label(idx, sim, eps, min_samples)
        self.neighbors_ = idx.cpu().numpy()
        self._sim, self._sim_host = sim, None
        self.stats_ = {'label_passes': [passes]}
        return self

    @property
    def similarity_(self):
        if self._sim is None:
            raise AttributeError("This SNN instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")
        if self._sim_host is None:
            self._sim_host = self._sim.cpu().numpy()
        return self._sim_host

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
