"""Spectral clustering on the MI355X (``sklearn.cluster.SpectralClustering(affinity='nearest_neighbors')``): a partition into exactly K groups that need not
be convex, and the eigengap as a criterion for K.  The p2 / p4 ``--cluster_method spectral`` branches.

The definition is stated once, in include/dic_hip.h (dic_spectral_spmm); in short, with L(i) the k-neighbour list of i from ``knn.kneighbors`` (the point
itself its first entry):  W = 0.5 (A + A^T) of the 0/1 matrix A of the lists, without its diagonal;  dd = sqrt(row sums);  M = D^-1/2 W D^-1/2;  the m largest
eigenpairs (theta, V) of M (sklearn's Laplacian is I - M);  embedding = V / dd, every column's entry of largest magnitude made positive;  labels from the
first K columns by k-means (``KMeans(K, n_init=10)``) or by sklearn's ``cluster_qr``, restated here in numpy.  ``n_components`` only sizes the decomposition:
the labels of K clusters always come from the first K columns (in sklearn k-means takes all ``n_components`` columns).

sklearn runs ARPACK on a sparse matrix on the CPU.  Here the graph is a CSR with one weight byte per entry (M itself is never stored) and the eigenpairs come
from Chebyshev-filtered subspace iteration on a block of b = m + guard <= 64 vectors: Rayleigh-Ritz, then a degree-12 Chebyshev polynomial that damps
[-1, theta_b], each of its steps one fused kernel (csrc/dic_spectral.hip).  The block is orthonormalised by CholeskyQR on the gram kernel, repeated until
||X^T X - I||_max <= 2e-13 is MEASURED, with a shifted Cholesky factor where the plain one fails (Fukaya et al., "Shifted Cholesky QR for computing the QR
factorization of ill-conditioned matrices", 2020): it stays on this package's deterministic kernels, where a library QR of a 75 000 x 15 block would not.
Every result has the same bits from call to call.  The package imports neither sklearn nor scipy.
"""
from __future__ import annotations

import numbers
import warnings

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .kmeans import KMeans
from .knn import _check_k, _shape_of, kneighbors

FILTER_DEGREE = 12          # SpMMs per outer iteration
ORTH_TOL = 2e-13            # ||X^T X - I||_max a block is held to (measured by the gram kernel after the last pass)
NOT_CONNECTED = 'Graph is not fully connected, spectral embedding may not work as expected.'


# ------------------------------------------------------------------------------------------------------------------------------------------ checks
def _check_x(X, n_neighbors):
    n, d = _shape_of(X)
    if n < 1:
        raise ValueError('Found array with 0 sample(s) (shape=(%d, %d)) while a minimum of 1 is required.' % (n, d))
    if int(n_neighbors) != n_neighbors:
        raise ValueError('n_neighbors must be an integer, got %r' % (n_neighbors,))
    k = int(n_neighbors)
    if k < 2:
        raise ValueError('spectral: n_neighbors must be >= 2 (the point itself is the first neighbour), got %d' % k)
    _check_k(k, n, n)
    if d > MAX_DIM:
        raise NotImplementedError('spectral: at most %d features (got %d)' % (MAX_DIM, d))
    return n, k


def _check_components(m, n, what='n_components'):
    if isinstance(m, bool) or not isinstance(m, (numbers.Integral, np.integer)) or m < 1:
        raise ValueError('%s must be an int >= 1, got %r' % (what, m))
    if m > N.MAX_CLUSTERS:
        raise ValueError('%s=%d > %d: outside the compiled limit' % (what, m, N.MAX_CLUSTERS))
    if n is not None and m > n:
        raise ValueError('%s=%d should be <= n_samples=%d.' % (what, m, n))
    return int(m)


def _random_state(rs):
    if rs is None or rs is np.random:
        return np.random.mtrand._rand          # sklearn's check_random_state(None): numpy's global state
    if isinstance(rs, (numbers.Integral, np.integer)):
        return np.random.RandomState(rs)
    return rs


def _block_width(m, n):
    """b = m + guard: max(4, m // 2) extra vectors, capped so that b <= min(64, N)."""
    return min(m + max(4, m // 2), 64, n)


def _require_bytes(n, k, b, device):
    """The graph build sorts 2 N k int64 keys (the keys, the sorted copy, the sort's scratch and the counts: 5 x 8 bytes each) and the solver holds at most
    eight (N, b) f64 blocks beside the CSR (13 bytes an entry)."""
    need = 2 * n * k * (5 * 8 + 13) + 8 * 8 * n * b
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise MemoryError('spectral clustering of %d points with %d neighbours needs %d bytes on the device, %d are free: the sort of the 2 N k graph keys '
                          'and eight (N, %d) f64 blocks' % (n, k, need, free, b))


# ------------------------------------------------------------------------------------------------------------------------------------------- graph
def symmetrise_lists(idx):
    """``(indptr (N + 1) int64, indices int32, weight uint8, dd (N) f64)`` on the device of the lists ``idx`` (N, k) (a device tensor of distinct entries per
    row, as ``knn.kneighbors`` gives them): the CSR of W = 0.5 (A + A^T) without its diagonal, ascending within a row, weight 1 = 0.5 and 2 = 1.0, and
    dd = sqrt(row sums).  One sort of the 2 N k keys i N + j gives rows, order and weights in one go."""
    n, k = idx.shape
    dev = idx.device
    rows = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    keys, counts = torch.unique(torch.cat([rows * n + cols, cols * n + rows]), sorted=True, return_counts=True)
    del rows, cols, keep
    ri = torch.div(keys, n, rounding_mode='floor')
    indices = (keys - ri * n).to(torch.int32)
    per_row = torch.bincount(ri, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(per_row, 0)
    # sums of halves below 2^53: exact in any order
    deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, ri, counts.to(torch.float64)) * 0.5
    return indptr, indices, counts.to(torch.uint8), torch.sqrt(deg)


def spectral_graph(X, n_neighbors, return_device=False):
    """``(indptr, indices, weight, dd)`` of the symmetrised ``n_neighbors``-neighbour graph of ``X`` (numpy array or tensor, (N, D), D <= 256;
    2 <= n_neighbors <= min(N, 1024)) -- ``symmetrise_lists`` of ``knn.kneighbors(X, n_neighbors)``.  numpy, or device tensors with ``return_device=True``."""
    n, k = _check_x(X, n_neighbors)
    dist, idx = kneighbors(X, k, return_device=True)
    del dist
    graph = symmetrise_lists(idx)
    return graph if return_device else tuple(t.cpu().numpy() for t in graph)


# ----------------------------------------------------------------------------------------------------------------------------------------- kernels
def spmm(graph, X, alpha=1.0, beta=0.0, gamma=0.0, Z=None, out=None):
    """``alpha (M X) + beta X + gamma Z`` for a device graph and (N, b) f64 device blocks (dic_spectral_spmm).  ``out`` may be ``Z``, never ``X``."""
    indptr, indices, weight, dd = graph
    n, b = X.shape
    Y = torch.empty_like(X) if out is None else out
    N.check(N.lib().dic_spectral_spmm(N.ptr(indptr), N.ptr(indices), N.ptr(weight), N.ptr(dd), n, indices.numel(), b, N.ptr(X), N.ptr(Z), float(alpha),
                                      float(beta), float(gamma), N.ptr(Y), N.stream_of(X)), 'dic_spectral_spmm')
    return Y


def gram(A, B):
    """``A^T B`` (b, b) f64 on the device for two (N, b) f64 device blocks (dic_spectral_gram)."""
    n, b = A.shape
    L = N.lib()
    ws = torch.empty(max(16, L.dic_spectral_gram_workspace(n, b)), dtype=torch.uint8, device=A.device)
    G = torch.empty((b, b), dtype=torch.float64, device=A.device)
    N.check(L.dic_spectral_gram(N.ptr(A), N.ptr(B), n, b, N.ptr(G), N.ptr(ws), ws.numel(), N.stream_of(A)), 'dic_spectral_gram')
    return G


def rotate(X, C):
    """``X C`` for an (N, b) f64 device block and a (b, b) matrix (numpy or tensor) (dic_spectral_rotate)."""
    n, b = X.shape
    Cd = torch.as_tensor(np.ascontiguousarray(C) if isinstance(C, np.ndarray) else C, dtype=torch.float64, device=X.device).contiguous()
    Y = torch.empty_like(X)
    N.check(N.lib().dic_spectral_rotate(N.ptr(X), N.ptr(Cd), n, b, N.ptr(Y), N.stream_of(X)), 'dic_spectral_rotate')
    return Y


def orthonormalise(X, stats=None):
    """The (N, b) f64 device block with the same span and ||X^T X - I||_max <= ORTH_TOL, measured: CholeskyQR passes X <- X R^-1 with R^T R = X^T X from the
    gram kernel, repeated until the gram of the result passes; where X^T X is not positive definite in f64 the factor of X^T X + s I is taken
    (s = 11 (N b + b (b + 1)) 2^-53 ||X^T X||_2)."""
    n, b = X.shape
    eye = np.eye(b)
    for passes in range(8):
        G = gram(X, X).cpu().numpy()
        G = 0.5 * (G + G.T)
        if not np.isfinite(G).all():
            raise FloatingPointError('spectral: the block has non-finite entries')
        if passes and np.abs(G - eye).max() <= ORTH_TOL:
            if stats is not None:
                stats['orth_passes'] = stats.get('orth_passes', 0) + passes
            return X
        try:
            Lc = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            shift = 11.0 * (n * b + b * (b + 1)) * 2.0 ** -53 * np.linalg.norm(G, 2)
            Lc = np.linalg.cholesky(G + shift * eye)
            if stats is not None:
                stats['orth_shifted'] = stats.get('orth_shifted', 0) + 1
        X = rotate(X, np.linalg.inv(Lc).T)
    raise RuntimeError('spectral: the block could not be orthonormalised to %g in 8 CholeskyQR passes' % ORTH_TOL)


# ------------------------------------------------------------------------------------------------------------------------------------------ solver
def eigsh_largest(graph, m, tol=1e-10, max_iter=200, random_state=None, stats=None):
    """The m largest eigenpairs of M by Chebyshev-filtered subspace iteration: ``(theta (m,) f64 numpy descending, V (N, m) f64 device, orthonormal columns,
    residuals (m,) f64 numpy ||M v - theta v||_2, n_iter, converged)``.  ``stats`` (a dict, optional) receives ``spmm`` (the SpMMs run), ``b``,
    ``orth_passes`` and ``orth_shifted``."""
    dd = graph[3]
    n = dd.shape[0]
    b = _block_width(m, n)
    if int(max_iter) < 1:
        raise ValueError('max_iter must be >= 1, got %r' % (max_iter,))
    rs = _random_state(random_state)
    X = orthonormalise(torch.as_tensor(rs.standard_normal((n, b)), device=dd.device), stats)
    n_spmm = 0
    converged = False
    for n_iter in range(1, int(max_iter) + 1):
        MX = spmm(graph, X)
        n_spmm += 1
        H = gram(X, MX).cpu().numpy()
        theta, Q = np.linalg.eigh(0.5 * (H + H.T))
        theta, Q = theta[::-1].copy(), Q[:, ::-1].copy()
        V, MV = rotate(X, Q), rotate(MX, Q)
        R = MV - V * torch.as_tensor(theta, device=V.device)
        res = np.sqrt(np.diag(gram(R, R).cpu().numpy()))
        del MX, MV, R
        if (res[:m] <= tol).all():
            converged = True
            break
        if n_iter == max_iter or b == n:          # (b == N: the Rayleigh-Ritz step is exact already)
            break
        # damp [-1, cut]: the scaled three-term recurrence of Zhou & Saad, "A Chebyshev-Davidson algorithm for large symmetric eigenproblems", 2007, the
        # scale fixed by the known top of the spectrum, 1, which the filter maps to 1
        cut = max(float(theta[-1]), -0.9)
        e, c = 0.5 * (cut + 1.0), 0.5 * (cut - 1.0)
        sigma = e / (1.0 - c)
        tau = 2.0 / sigma
        prev, cur = V, spmm(graph, V, sigma / e, -c * sigma / e)
        for _ in range(2, FILTER_DEGREE + 1):
            sn = 1.0 / (tau - sigma)
            nxt = spmm(graph, cur, 2.0 * sn / e, -2.0 * c * sn / e, -sigma * sn, Z=prev, out=prev)
            prev, cur, sigma = cur, nxt, sn
        n_spmm += FILTER_DEGREE
        del prev, V
        X = orthonormalise(cur, stats)
    if stats is not None:
        stats['spmm'], stats['b'] = n_spmm, b
    return theta[:m].copy(), V[:, :m], res[:m].copy(), n_iter, converged


def sign_flip(E):
    """sklearn's ``_deterministic_vector_sign_flip`` for the COLUMNS of the device matrix ``E``: the entry of largest magnitude of every column is made
    positive, the first one on equal magnitude (torch.argmax returns the first maximal index)."""
    at = torch.argmax(E.abs(), dim=0)
    sign = torch.sign(E[at, torch.arange(E.shape[1], device=E.device)])
    return E * torch.where(sign == 0, torch.ones_like(sign), sign)


def sign_flip_numpy(E):
    """``sign_flip`` for a numpy matrix (columns)."""
    at = np.argmax(np.abs(E), axis=0)
    sign = np.sign(E[at, np.arange(E.shape[1])])
    return E * np.where(sign == 0, 1.0, sign)


def _embed(X, m, n_neighbors, tol, max_iter, random_state, stats=None):
    """graph, eigenvalues (numpy), embedding (device), residuals, n_iter, converged, components -- and the two warnings."""
    n, k = _check_x(X, n_neighbors)
    m = _check_components(m, n)
    if not torch.cuda.is_available():
        raise RuntimeError('deep_interpolation_clustering_amd.spectral runs only on an MI355X; there is no CPU path by design')
    dev = X.device if isinstance(X, torch.Tensor) and X.is_cuda else torch.device('cuda', torch.cuda.current_device())
    _require_bytes(n, k, _block_width(m, n), dev)
    graph = spectral_graph(X, k, return_device=True)
    theta, V, res, n_iter, converged = eigsh_largest(graph, m, tol, max_iter, random_state, stats)
    emb = sign_flip(V / graph[3][:, None])
    components = int((theta >= 1.0 - 10.0 * tol).sum())
    if not converged:
        warnings.warn('spectral: the eigen-solver did not reach tol=%g in max_iter=%d iterations (largest residual %.3g); try a larger max_iter'
                      % (tol, max_iter, res.max()), UserWarning)
    if components > 1:
        warnings.warn(NOT_CONNECTED, UserWarning)
    return graph, theta, emb, res, n_iter, converged, components


def spectral_embedding(X, n_components, n_neighbors=10, tol=1e-10, max_iter=200, random_state=None, return_device=False):
    """``(eigenvalues (m,) f64 descending, embedding (N, m) f64)`` of the ``n_neighbors``-neighbour graph of ``X``: the m = ``n_components`` largest
    eigenvalues of M and V / dd, sign-flipped -- sklearn's ``spectral_embedding(norm_laplacian=True, drop_first=False)``, whose eigenvalues are
    1 - these.  The eigenvalues are numpy; the embedding is numpy, or a device tensor with ``return_device=True``.  UserWarning when ``max_iter`` is
    exhausted before every residual is <= ``tol``, and when the graph is not connected."""
    _, theta, emb, _, _, _, _ = _embed(X, n_components, n_neighbors, tol, max_iter, _random_state(random_state))
    return theta, (emb if return_device else emb.cpu().numpy())


# --------------------------------------------------------------------------------------------------------------------------------------- labelling
def cluster_qr(vectors):
    """sklearn's ``cluster_qr(vectors)`` ((N, K) numpy -> (N,) int64), restated without scipy: the first K pivots of the column-pivoted QR of vectors^T
    (greedy: the column of largest remaining norm, the first one on equal norms, as LAPACK's geqp3 chooses), the SVD U S V' of those K rows transposed, and
    the argmax over the columns of |vectors U V'| (Damle, Minden & Ying, "Simple, direct and efficient multi-way spectral clustering", 2019)."""
    vectors = np.asarray(vectors, dtype=np.float64)
    k = vectors.shape[1]
    A = vectors.T.copy()
    piv = []
    for _ in range(k):
        norms = np.einsum('ij,ij->j', A, A)
        norms[piv] = -1.0
        p = int(np.argmax(norms))
        piv.append(p)
        q = A[:, p] / np.sqrt(norms[p]) if norms[p] > 0 else np.zeros(k)
        A -= np.outer(q, q @ A)
    ut, _, v = np.linalg.svd(vectors[piv, :].T)
    return np.abs(vectors @ (ut @ v.conj())).argmax(axis=1).astype(np.int64)


class SpectralClustering:
    """``sklearn.cluster.SpectralClustering(n_clusters, affinity='nearest_neighbors', n_neighbors, assign_labels, n_init, eigen_tol, random_state)`` (module
    docstring).  ``n_components`` (default: the largest K asked for) sizes the decomposition; ``ks`` asks for a labelling per K from ONE decomposition, as
    ``Ward(ks=...)`` does (``n_clusters`` is added).  After ``fit``: ``labels_`` (N,) int64, ``labels_by_k_`` {K: labels from the first K columns},
    ``eigenvalues_`` (m,) f64 descending (of M: sklearn's are 1 - these), ``embedding_`` (N, m) f64, ``residuals_`` (m,), ``n_iter_``, ``converged_``,
    ``n_connected_components_`` (the eigenvalues >= 1 - 10 eigen_tol among the m computed), ``affinity_matrix_`` (the CSR triple indptr, indices, data
    with data 0.5 or 1.0, without the diagonal) and ``stats_``.  There is no ``predict``: the method has none."""

    def __init__(self, n_clusters=8, n_neighbors=10, n_components=None, assign_labels='kmeans', n_init=10, eigen_tol=1e-10, random_state=None, ks=None,
                 max_iter=200):
        if assign_labels not in ('kmeans', 'cluster_qr'):
            raise ValueError("assign_labels must be 'kmeans' or 'cluster_qr' ('discretize' is not provided), got %r" % (assign_labels,))
        ks = [] if ks is None else list(ks)
        for K in ks + [n_clusters]:
            _check_components(K, None, 'n_clusters')
        if n_components is not None:
            _check_components(n_components, None)
        self.n_clusters, self.n_neighbors, self.n_components, self.assign_labels = int(n_clusters), n_neighbors, n_components, assign_labels
        self.n_init, self.eigen_tol, self.random_state, self.max_iter = n_init, eigen_tol, random_state, max_iter
        self.ks = sorted(set(int(K) for K in ks) | {self.n_clusters})

    def fit(self, X, y=None):
        n, _ = _check_x(X, self.n_neighbors)
        m = max(self.ks) if self.n_components is None else int(self.n_components)
        if m < max(self.ks):
            raise ValueError('n_components=%d is smaller than the largest number of clusters, %d' % (m, max(self.ks)))
        for K in self.ks:
            _check_components(K, n, 'n_clusters')
        rs = _random_state(self.random_state)
        stats = {}
        graph, theta, emb, res, n_iter, converged, components = _embed(X, m, self.n_neighbors, self.eigen_tol, self.max_iter, rs, stats)
        self.eigenvalues_, self.residuals_, self.n_iter_, self.converged_, self.n_connected_components_ = theta, res, n_iter, converged, components
        self.embedding_ = emb.cpu().numpy()
        self.labels_by_k_ = {}
        for K in self.ks:
            if self.assign_labels == 'cluster_qr':
                self.labels_by_k_[K] = cluster_qr(self.embedding_[:, :K])
            else:
                self.labels_by_k_[K] = KMeans(K, n_init=self.n_init, random_state=rs).fit(emb[:, :K]).labels_.astype(np.int64)
        self.labels_ = self.labels_by_k_[self.n_clusters]
        indptr, indices, weight, _ = graph
        self.affinity_matrix_ = (indptr.cpu().numpy(), indices.cpu().numpy(), weight.cpu().numpy().astype(np.float64) * 0.5)
        self.stats_ = stats
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def spectral_sweep(X, ks, n_neighbors=10, assign_labels='kmeans', n_init=10, eigen_tol=1e-10, random_state=None, max_iter=200, n_components=None, return_fit=False):
    """A labelling of ``X`` per K of ``ks`` from ONE graph and ONE decomposition with m = max(ks): {K: (N,) int64}, each from the first K columns of the
    embedding -- ``SpectralClustering(n_clusters=max(ks), ks=ks, ...).fit(X).labels_by_k_``.  ``n_components`` > max(ks) computes more eigenpairs than the
    labellings use (p2 takes one more, for the gap after its last K).  ``return_fit``: the fitted estimator instead."""
    ks = list(ks)
    if not ks:
        raise ValueError('ks must name at least one number of clusters')
    fit = SpectralClustering(n_clusters=max(ks), n_neighbors=n_neighbors, assign_labels=assign_labels, n_init=n_init, eigen_tol=eigen_tol,
                             random_state=random_state, ks=ks, max_iter=max_iter, n_components=n_components).fit(X)
    return fit if return_fit else fit.labels_by_k_
