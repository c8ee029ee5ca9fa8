"""``MeanShift`` with scikit-learn's estimator surface on the MI355X (csrc/dic_meanshift.hip): the p2 / p4 ``--cluster_method meanshift`` branches.

Mean shift finds the modes of the latent density: it picks the number of clusters itself, like the density methods, and every cluster has a centre, so
``predict`` is "nearest centre" and p4 carries the model to the validation and test cohorts as it does for k-means, Ward and the mixtures.  The definition
is sklearn 1.7.2's ``cluster/_mean_shift.py`` (flat kernel) written as f64 arithmetic, stated once in include/dic_hip.h.  sklearn issues one ball-tree radius
query per seed per iteration; here ALL seeds advance together: one iteration is a members pass on the matrix cores (which points lie within the bandwidth of
which seed: a bit mask, decided exactly) and a shift kernel on the f64 matrix cores (member counts and sums, the new seeds, the stopping rule).  The host
reads the done flags every ``_POLL_EVERY`` iterations and compacts the active seeds, so the passes shrink as seeds converge.  The mask is held for a group of
seeds at a time under ``mask_budget`` bytes; no result depends on it.  The suppression walk over the sorted centres runs on the host, one ``nearest`` launch
per surviving centre.

Outputs are NumPy, like sklearn's.  The package imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .kmeans import _as_device_matrix, _device, _pad_features
from .ward import _usable_view

_POLL_EVERY = 4                     # shifts enqueued between two host reads of the done flags
DEFAULT_MASK_BUDGET = 256 << 20     # bytes of member mask held at a time (75 000 points: 9.4 KB per seed, 27 000 seeds per group)
MAX_BANDWIDTH = 2.0 ** 50           # csrc/dic_meanshift.hip: MS_MAX_BANDWIDTH


def _shape_of(X):
    shape = tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (shape,))
    return shape


class _Points:
    """The points as the kernels take them: ``x`` (N, D) f32 on the device (a qualifying strided view in place, else a zero-padded copy), the true feature
    count ``d0``, the shift ``c`` (D) f64 = the column means, the planes' centre (float)c, and the prepared workspace of the members pass."""

    def __init__(self, X):
        n, width = _shape_of(X)
        if width > MAX_DIM:
            raise NotImplementedError('meanshift: at most %d features (got %d)' % (MAX_DIM, width))
        if n < 1 or width < 1:
            raise ValueError('meanshift needs at least 1 point of at least 1 feature, got shape %s' % ((n, width),))
        self.x = X.detach() if _usable_view(X) else _pad_features(_as_device_matrix(X, _device())).contiguous()
        self.n, self.d0, self.d = n, width, self.x.shape[1]
        self.shift = self.x.double().mean(dim=0).contiguous()          # (a contiguous f64 copy whatever the strides: the same bits for a view and its copy)
        self.centre = self.shift.float().contiguous()
        self.words = (n + 31) // 32
        self._ws, self._ws_seeds = None, 0

    def workspace(self, m_max, extra_bytes):
        """The prepared planes with room for ``m_max`` seeds behind the points (kept: the bandwidths of a sweep share them)."""
        if self._ws is not None and self._ws_seeds == m_max:
            return self._ws
        L = N.lib()
        nbytes = int(L.dic_meanshift_workspace(self.n, m_max))
        if nbytes == 0:
            raise ValueError('meanshift: N=%d with %d seeds per pass is outside the kernel\'s limits (N + seeds + 256 < 2^30)' % (self.n, m_max))
        self._ws = None
        free = torch.cuda.mem_get_info(self.x.device)[0]
        if nbytes + extra_bytes > free:
            raise MemoryError('mean shift of %d points with %d seeds per pass needs %d bytes on the device, %d are free: the bf16 planes of the points and '
                              'seeds (2304 bytes per row), the member mask (N / 8 bytes per seed) and the f64 seeds' % (self.n, m_max, nbytes + extra_bytes, free))
        ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=self.x.device)
        N.check(L.dic_meanshift_prepare(N.ptr(self.x), self.x.stride(0), self.n, self.d, N.ptr(self.centre), m_max, N.ptr(ws), ws.numel(),
                                        N.stream_of(self.x)), 'dic_meanshift_prepare')
        self._ws, self._ws_seeds = ws, m_max
        return ws

    def rows64(self, A, what):
        """(M, D) f64 on the device, zero-padded, from an (M, d0) array or tensor."""
        a = A.detach().to(device=self.x.device, dtype=torch.float64) if isinstance(A, torch.Tensor) else \
            torch.as_tensor(np.ascontiguousarray(A, dtype=np.float64), device=self.x.device)
        if a.dim() != 2 or a.shape[1] != self.d0:
            raise ValueError('%s must be of shape (n, %d), got %s' % (what, self.d0, tuple(a.shape)))
        if a.shape[1] != self.d:
            a = torch.nn.functional.pad(a, (0, self.d - a.shape[1]))
        return a.contiguous()


def members(pts, seeds, bandwidth, mask, m_max, ws, band=None, stats=None):
    """The member mask of ``seeds`` ((M, D) f64 device, M <= m_max) into ``mask`` ((>= M, words) int32 device) (dic_meanshift_members).  Returns the band list
    buffer (grown when it overflowed: the pass is then run again)."""
    L = N.lib()
    m = seeds.shape[0]
    if band is None:
        band = torch.empty((max(1 << 16, 4 * m), 4), dtype=torch.int32, device=seeds.device)
    while True:
        nb = N.C.c_int64(0)
        rc = L.dic_meanshift_members(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, N.ptr(pts.centre), N.ptr(seeds), m, m_max, float(bandwidth), N.ptr(mask),
                                     N.ptr(band), band.shape[0], N.C.byref(nb), N.ptr(ws), ws.numel(), N.stream_of(seeds))
        if stats is not None:
            stats['band_pairs'] = stats.get('band_pairs', 0) + int(nb.value)
        if rc == -3 and nb.value > band.shape[0]:          # DIC_ERR_WORKSPACE: the band list overflowed -- the pass again, with room for every band pair
            band = torch.empty((int(nb.value), 4), dtype=torch.int32, device=seeds.device)
            if stats is not None:
                stats['band_reruns'] = stats.get('band_reruns', 0) + 1
            continue
        N.check(rc, 'dic_meanshift_members')
        return band


def shift(pts, mask, seeds, bandwidth, max_iter, counts, iters, done, sums=None):
    """One shift of the seeds whose done flag is clear, from their mask rows, in place (dic_meanshift_shift)."""
    N.check(N.lib().dic_meanshift_shift(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, N.ptr(pts.shift), N.ptr(mask), seeds.shape[0], N.ptr(seeds),
                                        float(bandwidth), int(max_iter), N.ptr(counts), N.ptr(iters), N.ptr(done), N.ptr(sums), N.stream_of(seeds)),
            'dic_meanshift_shift')


def nearest(centres, x=None, rows=None, want_d2=True):
    """(idx (n) int32, d2 (n) f64), device: the nearest of ``centres`` ((C, D) f64 device) for the f32 device points ``x`` or the f64 device ``rows``."""
    src = x if x is not None else rows
    n, d = src.shape
    idx = torch.empty(n, dtype=torch.int32, device=src.device)
    d2 = torch.empty(n, dtype=torch.float64, device=src.device) if want_d2 else None
    N.check(N.lib().dic_meanshift_nearest(N.ptr(x), 0 if x is None else x.stride(0), N.ptr(rows), n, d, N.ptr(centres), centres.shape[0], N.ptr(idx),
                                          N.ptr(d2), N.stream_of(src)), 'dic_meanshift_nearest')
    return idx, d2


def estimate_bandwidth(X, quantile=0.3, candidate_budget=None):
    """sklearn's ``estimate_bandwidth(X, quantile)`` with ``n_samples=None``: the f64 mean over the points of the distance to their k-th neighbour, the point
    itself included, k = max(1, int(N * quantile)) (``knn.kth_neighbor_distance``: exact for the f32 coordinates)."""
    from .knn import kth_neighbor_distance
    if not 0 <= quantile <= 1:
        raise ValueError('quantile must be in [0, 1], got %r' % (quantile,))
    n, _ = _shape_of(X)
    k = max(1, int(n * quantile))
    return float(np.mean(kth_neighbor_distance(X, k, candidate_budget=candidate_budget), dtype=np.float64))


def get_bin_seeds(X, bin_size, min_bin_freq=1):
    """sklearn's ``get_bin_seeds``: the points binned to a grid of ``bin_size``, the bins of at least ``min_bin_freq`` points (in the order their first point
    appears) as f32 grid coordinates times ``bin_size``; ``X`` itself, with sklearn's warning, when every point has a bin of its own."""
    X = np.asarray(X)
    if bin_size == 0:
        return X
    binned = np.round(X / bin_size)
    uniq, first, freq = np.unique(binned, axis=0, return_index=True, return_counts=True)
    keep = freq >= min_bin_freq
    order = np.argsort(first[keep], kind='stable')
    bin_seeds = np.array(uniq[keep][order], dtype=np.float32).reshape(-1, X.shape[1])
    if len(bin_seeds) == len(X):
        warnings.warn('Binning data failed with provided bin_size=%f, using data points as seeds.' % bin_size)
        return X
    return bin_seeds * np.float32(bin_size)


def _check_int(name, v, low):
    if isinstance(v, bool) or not isinstance(v, (numbers.Integral, np.integer)) or v < low:
        raise ValueError('%s must be an int >= %d, got %r' % (name, low, v))
    return int(v)


class MeanShift:
    def __init__(self, *, bandwidth=None, seeds=None, bin_seeding=False, min_bin_freq=1, cluster_all=True, n_jobs=None, max_iter=300,
                 mask_budget=DEFAULT_MASK_BUDGET):
        if bandwidth is not None and not bandwidth > 0:
            raise ValueError('bandwidth must be > 0 or None, got %r' % (bandwidth,))
        if bandwidth is not None and not bandwidth < MAX_BANDWIDTH:
            raise ValueError('bandwidth must be below 2^50, got %r' % (bandwidth,))
        self.bandwidth = None if bandwidth is None else float(bandwidth)
        self.seeds = seeds
        self.bin_seeding = bool(bin_seeding)
        self.min_bin_freq = _check_int('min_bin_freq', min_bin_freq, 1)
        self.cluster_all = bool(cluster_all)
        self.n_jobs = n_jobs
        self.max_iter = _check_int('max_iter', max_iter, 0)
        self.mask_budget = _check_int('mask_budget', mask_budget, 1)

    # -- the iteration ------------------------------------------------------------------------
    def _run_seeds(self, pts, seeds, h):
        """All seeds to their modes: (final seeds (M, D) f64 device, counts (M), iterations (M) int32 device)."""
        dev = pts.x.device
        m_all = seeds.shape[0]
        group = max(256, self.mask_budget // (4 * pts.words) // 256 * 256)          # seeds whose mask rows fit the budget, whole row blocks
        m_max = min(m_all, group)
        ws = pts.workspace(m_max, 4 * m_max * pts.words + 3 * 8 * m_all * pts.d)
        mask = torch.empty((m_max, pts.words), dtype=torch.int32, device=dev)
        fin_s = seeds.clone()
        fin_c = torch.zeros(m_all, dtype=torch.int32, device=dev)
        fin_i = torch.zeros(m_all, dtype=torch.int32, device=dev)
        orig = torch.arange(m_all, device=dev)
        s = seeds.clone()
        cnt, it, dn = (torch.zeros(m_all, dtype=torch.int32, device=dev) for _ in range(3))
        band = None
        self.stats_ = stats = {'shifts': 0, 'groups': -(-m_all // m_max), 'active': [], 'band_pairs': 0}
        while s.shape[0]:
            m = s.shape[0]
            for _ in range(_POLL_EVERY):
                stats['active'].append(m)
                for g0 in range(0, m, m_max):
                    g1 = min(m, g0 + m_max)
                    band = members(pts, s[g0:g1], h, mask, m_max, ws, band, stats)
                    shift(pts, mask, s[g0:g1], h, self.max_iter, cnt[g0:g1], it[g0:g1], dn[g0:g1])
                stats['shifts'] += 1
                if stats['shifts'] > self.max_iter:          # (every seed is done after max_iter + 1 shifts)
                    break
            finished = dn != 0                               # the host read of the loop
            if bool(finished.any()):
                at = orig[finished]
                fin_s[at], fin_c[at], fin_i[at] = s[finished], cnt[finished], it[finished]
                keep = ~finished
                orig, s, cnt, it, dn = orig[keep], s[keep].contiguous(), cnt[keep].contiguous(), it[keep].contiguous(), dn[keep].contiguous()
        return fin_s, fin_c, fin_i

    def _centres(self, pts, fin_s, counts, h):
        """The suppression walk: the surviving centres (K, D) f64 device, in walk order."""
        live = np.flatnonzero(counts > 0)
        if live.size == 0:
            raise ValueError('No point was within bandwidth=%f of any seed. Try a different seeding strategy or increase the bandwidth.' % h)
        cand = fin_s[torch.as_tensor(live, device=fin_s.device)].contiguous()
        host = cand[:, :pts.d0].cpu().numpy()
        # descending by (count, tuple(coordinates)): ascending lexicographic order, reversed (equal keys are equal rows: their order cannot matter)
        keys = [host[:, c] for c in range(pts.d0 - 1, -1, -1)] + [counts[live]]
        order = np.lexsort(keys)[::-1].copy()
        srt = cand[torch.as_tensor(order, device=cand.device)].contiguous()
        n_c = srt.shape[0]
        t = h * h
        alive = np.ones(n_c, dtype=bool)
        keep = []
        i = 0
        while i < n_c:
            keep.append(i)
            _, d2 = nearest(srt[i:i + 1], rows=srt)
            alive &= ~(d2 <= t).cpu().numpy()               # (itself among them: d2 = 0)
            nxt = np.flatnonzero(alive[i + 1:])
            i = i + 1 + int(nxt[0]) if nxt.size else n_c
        return srt[torch.as_tensor(np.asarray(keep), device=srt.device)].contiguous()

    # -- estimator API ------------------------------------------------------------------------
    def _fit_points(self, pts, X=None):
        h = self.bandwidth
        if h is None:
            h = estimate_bandwidth(pts.x[:, :pts.d0])
            if not h > 0:
                raise ValueError('the estimated bandwidth is %r: pass bandwidth > 0 (duplicated points make the k-th neighbour distance 0)' % (h,))
        if self.seeds is not None:
            seeds = pts.rows64(self.seeds, 'seeds')
        elif self.bin_seeding:
            host = pts.x[:, :pts.d0].cpu().numpy().astype(np.float64)
            b = get_bin_seeds(host, h, self.min_bin_freq)
            seeds = pts.x.double().contiguous() if b is host else pts.rows64(b, 'seeds')
        else:
            seeds = pts.x.double().contiguous()
        if seeds.shape[0] < 1:
            raise ValueError('meanshift: no seeds (min_bin_freq=%d leaves no bin)' % self.min_bin_freq)
        fin_s, fin_c, fin_i = self._run_seeds(pts, seeds, h)
        self.seed_counts_ = fin_c.cpu().numpy()
        self.seed_iterations_ = fin_i.cpu().numpy()
        self.seed_positions_ = fin_s[:, :pts.d0].cpu().numpy()
        self.n_iter_ = int(self.seed_iterations_.max())
        self.bandwidth_ = float(h)
        self.n_features_in_ = pts.d0
        centres = self._centres(pts, fin_s, self.seed_counts_, h)
        self.cluster_centers_ = centres[:, :pts.d0].cpu().numpy()
        idx, d2 = nearest(centres, x=pts.x)
        labels = idx.cpu().numpy().astype(np.int64)
        if not self.cluster_all:
            labels[d2.cpu().numpy() > h * h] = -1
        self.labels_ = labels
        return self

    def fit(self, X, y=None):
        return self._fit_points(_Points(X))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X, orphans=False):
        """(N,) int64 numpy: the nearest centre of every row (no orphans, as sklearn; ``orphans=True``: -1 where it lies farther than the bandwidth, the rule
        ``cluster_all=False`` applies to ``labels_``)."""
        if not hasattr(self, 'cluster_centers_'):
            raise RuntimeError('This MeanShift instance is not fitted yet.')
        n, width = _shape_of(X)
        if width != self.n_features_in_:
            raise ValueError('X has %d features, but MeanShift is expecting %d features as input.' % (width, self.n_features_in_))
        x = X.detach() if _usable_view(X) else _pad_features(_as_device_matrix(X, _device())).contiguous()
        c = torch.zeros((self.cluster_centers_.shape[0], x.shape[1]), dtype=torch.float64, device=x.device)
        c[:, :width] = torch.as_tensor(self.cluster_centers_, device=x.device)
        idx, d2 = nearest(c, x=x, want_d2=orphans)
        labels = idx.cpu().numpy().astype(np.int64)
        if orphans:
            labels[d2.cpu().numpy() > self.bandwidth_ * self.bandwidth_] = -1
        return labels

    def reorder(self, order):
        """Renumber the clusters: new cluster j is old cluster ``order[j]`` (p4 orders them by systolic pressure)."""
        order = np.asarray(order, dtype=np.int64)
        k = self.cluster_centers_.shape[0]
        if sorted(order.tolist()) != list(range(k)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (k - 1, order.tolist()))
        self.cluster_centers_ = self.cluster_centers_[order].copy()
        inverse = np.empty_like(order)
        inverse[order] = np.arange(k)
        self.labels_ = np.where(self.labels_ >= 0, inverse[np.maximum(self.labels_, 0)], -1).astype(self.labels_.dtype)
        return self

    def get_params(self, deep=True):
        return dict(bandwidth=self.bandwidth, seeds=self.seeds, bin_seeding=self.bin_seeding, min_bin_freq=self.min_bin_freq, cluster_all=self.cluster_all,
                    n_jobs=self.n_jobs, max_iter=self.max_iter)


def mean_shift_sweep(X, bandwidths, **kw):
    """{bandwidth: fitted ``MeanShift(bandwidth=bandwidth, **kw)``} for every bandwidth: X is uploaded once and its planes are prepared once."""
    pts = _Points(X)
    return {float(b): MeanShift(bandwidth=float(b), **kw)._fit_points(pts) for b in bandwidths}
