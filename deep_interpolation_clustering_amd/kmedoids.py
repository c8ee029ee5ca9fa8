"""``KMedoids`` (PAM) on the MI355X (csrc/dic_kmedoids.hip): the p2 / p4 ``--cluster_method kmedoids`` branches.

k-medoids is the package's exemplar-based method: every centre is an actual row of X -- an encounter that can be shown -- and the objective is the sum of
unsquared Euclidean distances, the quantity the silhouette and Dunn indices are built on.  The definition (BUILD, then steepest-descent SWAP with FastPAM1's
shared removal term, all in f64) is stated once in include/dic_hip.h.  Classical PAM needs the N x N matrix; here one swap search is an approximate pass on
the matrix cores that comes with a rigorous error bound per candidate and only SELECTS candidates, and an exact f64 stage that decides among them, so the
result is the definition's.  The host reads one small record per iteration (the winner, its Delta, the candidate count).

Outputs are NumPy.  The package imports neither sklearn nor scipy; there is no CPU fallback.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .kmeans import _as_device_matrix, _device, _pad_features, _pp_init
from .ward import _usable_view

MAX_CLUSTERS = N.MAX_CLUSTERS
_INITS = ('build', 'random', 'k-medoids++')


def _shape_of(X):
    shape = tuple(X.shape) if hasattr(X, 'shape') else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError('X must be 2-D (n_samples, n_features), got shape %s' % (shape,))
    return shape


def _has_nan(X):
    if isinstance(X, torch.Tensor):
        return bool(torch.isnan(X).any())
    return bool(np.isnan(np.asarray(X, dtype=np.float64)).any())


def _check_k(k, n):
    if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
        raise ValueError('n_clusters must be an int, got %r' % (k,))
    if k < 1:
        raise ValueError('n_clusters must be >= 1, got %d' % k)
    if k > MAX_CLUSTERS:
        raise ValueError('n_clusters must be <= %d, got %d' % (MAX_CLUSTERS, k))
    if n is not None and k > n:
        raise ValueError('n_clusters=%d must be <= n_samples=%d' % (k, n))
    return int(k)


def _check_input(X):
    """Shape, width and NaN checks that need no GPU."""
    n, width = _shape_of(X)
    if width > MAX_DIM:
        raise NotImplementedError('kmedoids: at most %d features (got %d)' % (MAX_DIM, width))
    if n < 1 or width < 1:
        raise ValueError('kmedoids needs at least 1 point of at least 1 feature, got shape %s' % ((n, width),))
    if _has_nan(X):
        raise ValueError('kmedoids: X contains NaN')
    return n, width


def _device_rows(X):
    return X.detach() if _usable_view(X) else _pad_features(_as_device_matrix(X, _device())).contiguous()


class _Points:
    """The points as the kernels take them (``x`` (N, D) f32 on the device: a qualifying strided view in place, else a zero-padded copy), the prepared planes
    for up to ``k_max`` slots, and the buffers of a search."""

    def __init__(self, X, k_max, shape=None):
        n, width = shape if shape is not None else _check_input(X)          # (``shape``: the caller has run the checks)
        self.x = _device_rows(X)
        self.n, self.d0, self.d, self.k_max = n, width, self.x.shape[1], int(k_max)
        dev = self.x.device
        L = N.lib()
        nbytes = int(L.dic_kmedoids_workspace(n, self.k_max))
        if nbytes == 0:
            raise ValueError('kmedoids: N=%d with K=%d is outside the kernel\'s limits' % (n, self.k_max))
        centre = self.x.double().mean(dim=0).float().contiguous()
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        N.check(L.dic_kmedoids_prepare(N.ptr(self.x), self.x.stride(0), n, self.d, N.ptr(centre), self.k_max, N.ptr(self.ws), self.ws.numel(),
                                       N.stream_of(self.x)), 'dic_kmedoids_prepare')
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.nearest = torch.empty(n, **i32)
        self.dn, self.ds, self.td = torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(1, **f64)
        self.g, self.r, self.e = torch.empty(n, **f64), torch.empty((n, self.k_max), **f64), torch.empty(n, **f64)
        self.list, self.count = torch.empty(n, **i32), torch.zeros(1, **i32)
        self.delta = torch.empty((n, self.k_max), **f64)
        self.out = torch.empty(4, **f64)

    # -- the ABI, one call each ----------------------------------------------------------------------------------------------------
    def assign(self, medoids, q=None):
        """nearest, dn, ds, td of ``q`` (default: the points themselves, into the buffers of the search) against the medoid rows."""
        x = self.x
        if q is None:
            q, nearest, dn, ds, td = x, self.nearest, self.dn, self.ds, self.td
        else:
            nearest = torch.empty(q.shape[0], dtype=torch.int32, device=x.device)
            dn, ds = (torch.empty(q.shape[0], dtype=torch.float64, device=x.device) for _ in range(2))
            td = torch.empty(1, dtype=torch.float64, device=x.device)
        N.check(N.lib().dic_kmedoids_assign(N.ptr(q), q.stride(0), q.shape[0], self.d, N.ptr(x), x.stride(0), self.n, N.ptr(medoids), medoids.numel(),
                                            N.ptr(nearest), N.ptr(dn), N.ptr(ds), None, N.ptr(td), N.stream_of(x)), 'dic_kmedoids_assign')
        return nearest, dn, ds, td

    def delta_pass(self, k, mode):
        """g~, r~ and the bound E of every candidate (into the buffers)."""
        N.check(N.lib().dic_kmedoids_delta_pass(self.n, self.k_max, max(k, 1), mode, N.ptr(self.nearest), N.ptr(self.dn), N.ptr(self.ds), N.ptr(self.g),
                                                N.ptr(self.r), N.ptr(self.e), N.ptr(self.ws), self.ws.numel(), N.stream_of(self.x)), 'dic_kmedoids_delta_pass')

    def search(self, medoids, mode):
        """One search from the assignment in the buffers: (c, i, Delta, candidates sent to the exact stage); c = -1 when no candidate is left."""
        L, st = N.lib(), N.stream_of(self.x)
        k = medoids.numel() if medoids is not None else 0
        cols = k if mode == 2 else 0
        self.delta_pass(k, mode)
        r = self.r if self.k_max == max(k, 1) or mode != 2 else self.r.view(-1)[:self.n * k].view(self.n, k)
        N.check(L.dic_kmedoids_select(self.n, self.k_max, cols, N.ptr(self.g), N.ptr(r), N.ptr(self.e), N.ptr(medoids), k, N.ptr(self.list), N.ptr(self.count),
                                      N.ptr(self.ws), self.ws.numel(), st), 'dic_kmedoids_select')
        # (every workgroup past the candidate count, which stays on the device, leaves at once)
        N.check(L.dic_kmedoids_exact(N.ptr(self.x), self.x.stride(0), self.n, self.d, N.ptr(self.list), self.n, N.ptr(self.count), mode, N.ptr(self.nearest),
                                     N.ptr(self.dn), N.ptr(self.ds), max(k, 1), N.ptr(self.delta), st), 'dic_kmedoids_exact')
        N.check(L.dic_kmedoids_pick(N.ptr(self.list), self.n, N.ptr(self.count), N.ptr(self.delta), max(cols, 1), N.ptr(self.out), st), 'dic_kmedoids_pick')
        c, i, dl, cnt = self.out.cpu().tolist()          # the host read of the iteration
        return int(c), int(i), float(dl), int(cnt)

    def build(self, k):
        """The BUILD medoids of ``k`` (host list) and the candidates sent to the exact stage per step."""
        dev = self.x.device
        med, counts = [], []
        for step in range(k):
            m = torch.as_tensor(med, dtype=torch.int32, device=dev) if med else None
            if m is not None:
                self.assign(m)
            c, _, _, cnt = self.search(m, 1 if step else 0)
            if c < 0:
                raise RuntimeError('kmedoids BUILD: no candidate at step %d' % step)
            med.append(c)
            counts.append(cnt)
        return med, counts


def _find_rows(pts, rows):
    """The index of every row of ``rows`` in the points, by value (the first match; equal rows are interchangeable as medoids up to their index)."""
    out = []
    for k in range(rows.shape[0]):
        hit = (pts.x[:, :rows.shape[1]] == rows[k]).all(dim=1)
        at = torch.nonzero(hit)
        if at.numel() == 0:
            raise RuntimeError('kmedoids: an initial row was not found among the points')
        for cand in at.flatten().tolist():          # k-means++ may choose equal rows: take distinct indices where there are any
            if cand not in out:
                out.append(cand)
                break
        else:
            raise ValueError('kmedoids: k-medoids++ chose more equal rows than X holds; use init=\'build\'')
    return out


class KMedoids:
    def __init__(self, n_clusters=8, *, init='build', max_iter=300, random_state=None):
        self.n_clusters = _check_k(n_clusters, None)
        if isinstance(init, str):
            if init not in _INITS:
                raise ValueError('init must be one of %r or an array of row indices, got %r' % (_INITS, init))
        else:
            init = np.asarray(init)
            if init.ndim != 1 or init.dtype.kind not in 'iu' or init.size != self.n_clusters:
                raise ValueError('init as an array must hold n_clusters=%d row indices, got %r' % (self.n_clusters, init))
            if np.unique(init).size != init.size:
                raise ValueError('init holds duplicate row indices: %r' % (init.tolist(),))
            if init.min() < 0:
                raise ValueError('init holds a row index out of range: %r' % (init.tolist(),))
        self.init = init
        if isinstance(max_iter, bool) or not isinstance(max_iter, (numbers.Integral, np.integer)) or max_iter < 0:
            raise ValueError('max_iter must be an int >= 0, got %r' % (max_iter,))
        self.max_iter = int(max_iter)
        self.random_state = random_state

    def _check_against(self, n):
        _check_k(self.n_clusters, n)
        if not isinstance(self.init, str) and self.init.max() >= n:
            raise ValueError('init holds a row index out of range (n_samples=%d): %r' % (n, self.init.tolist()))

    def _initial(self, pts, build_prefix):
        K = self.n_clusters
        self.build_n_exact_ = []
        if not isinstance(self.init, str):
            return [int(v) for v in self.init]
        if self.init == 'build':
            if build_prefix is not None:
                med, self.build_n_exact_ = build_prefix[0][:K], build_prefix[1][:K]
            else:
                med, self.build_n_exact_ = pts.build(K)
            return list(med)
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
        if self.init == 'random':
            return [int(v) for v in rs.choice(pts.n, K, replace=False)]
        rows = _pp_init(pts.x.contiguous(), K, 1, rs)[0]          # 'k-medoids++': the rows kmeans._pp_init chooses, found again by value
        return _find_rows(pts, rows)

    def _fit_points(self, pts, build_prefix=None):
        self._check_against(pts.n)
        K, dev = self.n_clusters, pts.x.device
        med = self._initial(pts, build_prefix)
        self.initial_medoid_indices_ = np.asarray(med, dtype=np.int64)
        self.swaps_, self.n_exact_ = [], []
        self.converged_, self.n_iter_ = False, 0
        m = torch.as_tensor(med, dtype=torch.int32, device=dev)
        pts.assign(m)
        for it in range(self.max_iter):
            c, i, dl, cnt = pts.search(m, 2)
            self.n_exact_.append(cnt)
            if c < 0 or not dl < 0:
                self.converged_ = True
                break
            self.swaps_.append((it, i, med[i], c, dl))
            med[i] = c
            self.n_iter_ = it + 1          # iterations that swapped: the search that stops is not counted
            m = torch.as_tensor(med, dtype=torch.int32, device=dev)
            pts.assign(m)
        self.medoid_indices_ = np.asarray(med, dtype=np.int64)
        self.cluster_centers_ = pts.x[m.long(), :pts.d0].cpu().numpy()
        self.labels_ = pts.nearest.cpu().numpy().astype(np.int64)
        self.inertia_ = float(pts.td.item())
        self.n_features_in_ = pts.d0
        return self

    def fit(self, X, y=None):
        shape = _check_input(X)
        self._check_against(shape[0])
        return self._fit_points(_Points(X, self.n_clusters, shape))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def _against_medoids(self, X):
        if not hasattr(self, 'cluster_centers_'):
            raise RuntimeError('This KMedoids instance is not fitted yet.')
        n, width = _check_input(X)
        if width != self.n_features_in_:
            raise ValueError('X has %d features, but KMedoids is expecting %d features as input.' % (width, self.n_features_in_))
        q = _device_rows(X)
        c = _pad_features(torch.as_tensor(self.cluster_centers_, device=q.device)).contiguous()
        return q, c

    def predict(self, X):
        """(N,) int64 numpy: the slot of the nearest medoid of every row, ties to the smaller slot."""
        q, c = self._against_medoids(X)
        K = c.shape[0]
        m = torch.arange(K, dtype=torch.int32, device=q.device)
        nearest = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        N.check(N.lib().dic_kmedoids_assign(N.ptr(q), q.stride(0), q.shape[0], q.shape[1], N.ptr(c), c.stride(0), K, N.ptr(m), K, N.ptr(nearest), None, None,
                                            None, None, N.stream_of(q)), 'dic_kmedoids_assign')
        return nearest.cpu().numpy().astype(np.int64)

    def transform(self, X):
        """(N, K) f64 numpy: the distance of every row to every medoid."""
        q, c = self._against_medoids(X)
        K = c.shape[0]
        m = torch.arange(K, dtype=torch.int32, device=q.device)
        out = torch.empty((q.shape[0], K), dtype=torch.float64, device=q.device)
        N.check(N.lib().dic_kmedoids_assign(N.ptr(q), q.stride(0), q.shape[0], q.shape[1], N.ptr(c), c.stride(0), K, N.ptr(m), K, None, None, None,
                                            N.ptr(out), None, N.stream_of(q)), 'dic_kmedoids_assign')
        return out.cpu().numpy()

    def reorder(self, order):
        """Renumber the clusters: new cluster j is old cluster ``order[j]`` (p4 orders them by systolic pressure)."""
        order = np.asarray(order, dtype=np.int64)
        k = self.n_clusters
        if sorted(order.tolist()) != list(range(k)):
            raise ValueError('order must be a permutation of 0..%d, got %r' % (k - 1, order.tolist()))
        self.cluster_centers_ = self.cluster_centers_[order].copy()
        self.medoid_indices_ = self.medoid_indices_[order].copy()
        inverse = np.empty_like(order)
        inverse[order] = np.arange(k)
        self.labels_ = inverse[self.labels_]
        return self

    def get_params(self, deep=True):
        return dict(n_clusters=self.n_clusters, init=self.init, max_iter=self.max_iter, random_state=self.random_state)


def kmedoids_sweep(X, ks, **kw):
    """{K: fitted ``KMedoids(K, **kw)``}: the planes are prepared once, and with ``init='build'`` one BUILD of max(ks) serves every K (the BUILD medoids of K
    are a prefix of those of any larger K); SWAP then runs per K."""
    ks = [int(k) for k in ks]
    if not ks:
        return {}
    shape = _check_input(X)
    models = {k: KMedoids(k, **kw) for k in ks}
    for mdl in models.values():
        mdl._check_against(shape[0])
    pts = _Points(X, max(ks), shape)
    prefix = pts.build(max(ks)) if kw.get('init', 'build') == 'build' else None
    return {k: models[k]._fit_points(pts, prefix) for k in ks}
