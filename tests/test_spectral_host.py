"""Spectral clustering without a GPU: the numpy yardstick, the cases, and the host pieces of spectral.py against sklearn's and scipy's compiled ones.

The yardstick is dense: A from sklearn's ``kneighbors_graph(include_self=True)`` on the f64 copy of the points (``sklearn_W``: and where distances tie), W = 0.5 (A + A^T) without its diagonal,
M = D^-1/2 W D^-1/2 and ``numpy.linalg.eigh``.  Every case is asserted CLEAR here -- a gap after K, the number of components, sklearn's labels (both
``assign_labels``) and k-means on the yardstick's embedding equal up to renumbering -- so that tests/test_gpu_spectral.py can demand equality.

CASES: name -> (N, D, k, K, m, connected components).  The smallest shapes at which the kernels can go wrong:
  n17_k3        17 x 2: five workgroups of the row kernels (4 rows each, the last one row), one of the gram kernel, a block narrower than the guard wants (b = 6 of 17)
  rings600      two noisy concentric rings: non-convex, and a gap of 1e-3 after K = 2, so the filter has to work
  blobs1030_k4  four components: the eigenvalue 1 is four-fold
  overlap1030   connected, distinct leading eigenvalues: single eigenvectors are comparable
  d13           500 x 13 (zero-padded features), a centre point per group whose row of the symmetric graph is longer than a wave (> 64 entries)
  dups255       twenty identical rows: index ties in the lists and the long rows around them
  d256_k7       4100 x 256, k = 17, seven components, m = 10: full-width rows, many workgroups, b = 15
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import spectral as S
from test_knn_lists_host import kneighbors_exact

CASES = {
    'n17_k3': (17, 2, 3, 2, 2, 2),
    'rings600': (600, 2, 10, 2, 2, 2),
    'blobs1030_k4': (1030, 8, 10, 4, 4, 4),
    'overlap1030': (1030, 8, 15, 3, 3, 1),
    'd13': (500, 13, 10, 3, 3, 3),
    'dups255': (255, 4, 24, 3, 3, 3),
    'd256_k7': (4100, 256, 17, 7, 10, 7),
}
TOL = 1e-10
TIED = ('dups255',)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def _blobs(rng, sizes, d, spread, sigma):
    centres = rng.normal(0, spread, (len(sizes), d))
    return np.concatenate([c + rng.normal(0, sigma, (s, d)) for c, s in zip(centres, sizes)])


@functools.lru_cache(maxsize=None)
def points(name):
    n, d, k, K, m, comps = CASES[name]
    rng = np.random.default_rng(2 if name == 'n17_k3' else 7)          # (seeds chosen so that test_conditions_of_the_cases holds)
    if name == 'n17_k3':
        X = np.concatenate([rng.normal(0, 0.3, (9, 2)), rng.normal(0, 0.3, (8, 2)) + [6.0, 0.0]])
    elif name == 'rings600':
        t = rng.uniform(0, 2 * np.pi, 600)
        r = np.where(np.arange(600) < 300, 1.0, 2.0) + rng.normal(0, 0.03, 600)
        X = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    elif name == 'blobs1030_k4':
        X = _blobs(rng, (300, 250, 280, 200), 8, 10.0, 0.5)
    elif name == 'overlap1030':
        X = _blobs(rng, (400, 330, 300), 8, 1.6, 1.0)
    elif name == 'd13':          # per group a centre and a shell around it: the shell points are farther from each other than from the centre
        parts = []
        for g, s in enumerate((170, 165, 165)):
            shell = rng.normal(0, 1, (s - 1, 13))
            shell *= (1.0 + rng.normal(0, 0.02, (s - 1, 1))) / np.linalg.norm(shell, axis=1, keepdims=True)
            centre = np.zeros((1, 13))
            parts.append(np.concatenate([centre, shell]) + 20.0 * g)
        X = np.concatenate(parts)
    elif name == 'dups255':
        X = _blobs(rng, (100, 80, 75), 4, 12.0, 0.6)
        X[40:60] = X[40]          # twenty identical rows inside the first group
    elif name == 'd256_k7':
        X = _blobs(rng, (700, 650, 600, 600, 550, 500, 500), 256, 3.0, 0.5)
    X = X.astype(np.float32)
    assert X.shape == (n, d)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def lists(name):
    """(N, k) int32: the exact lists, sorted by (distance, index) -- what ``knn.kneighbors`` gives."""
    n, k = CASES[name][0], CASES[name][2]
    idx = kneighbors_exact(points(name), None, k)[1] if n <= 1100 else exact_lists(points(name), k)
    idx.setflags(write=False)
    return idx


def exact_lists(X, k, extra=16):
    """``test_knn_lists_host.kneighbors_exact(X, None, k)[1]`` without its N^2 D differences (21 s at 4100 x 256): the k + ``extra`` candidates of every row by
    the f64 expansion |x|^2 + |y|^2 - 2 x.y (a BLAS product), then the exact difference-form d^2 of the candidates alone, sorted by (d^2, index).  Asserted
    safe: every row's k-th exact d^2 lies below its last candidate's expanded d^2 by more than the expansion can err (1e-10 of the largest 4 |x|^2; its own
    rounding is about D 2^-52 of that), so no point outside the candidates can belong to the list.  (Exact ties at the k-th place fail the assertion: such cases
    take kneighbors_exact.)  test_conditions_of_the_cases holds it to kneighbors_exact on overlap1030."""
    X64 = np.asarray(X, dtype=np.float64)
    n = len(X64)
    sq = np.einsum('ij,ij->i', X64, X64)
    approx = sq[:, None] + sq[None, :] - 2.0 * (X64 @ X64.T)
    c = min(n, k + extra)
    cand = np.sort(np.argpartition(approx, c - 1, axis=1)[:, :c], axis=1)
    last = np.take_along_axis(approx, cand, 1).max(1)
    idx = np.empty((n, k), np.int32)
    step = max(1, (1 << 24) // (c * X64.shape[1]))
    for s0 in range(0, n, step):
        rows = slice(s0, s0 + step)
        diff = X64[rows, None, :] - X64[cand[rows]]
        d2 = np.einsum('ijk,ijk->ij', diff, diff)
        order = np.lexsort((cand[rows], d2), axis=1)[:, :k]
        idx[rows] = np.take_along_axis(cand[rows], order, 1)
        if c < n:
            assert (np.take_along_axis(d2, order[:, -1:], 1)[:, 0] < last[rows] - 1e-10 * 4.0 * sq.max()).all()
    return idx


def symmetrise_numpy(idx):
    """``(indptr int64, indices int32, weight uint8, dd f64)``: the CSR of W = 0.5 (A + A^T) without its diagonal for the lists ``idx``, weight 1 = 0.5 and
    2 = 1.0, rows ascending -- spectral.symmetrise_lists in numpy."""
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1).astype(np.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    keys, counts = np.unique(np.concatenate([rows * n + cols, cols * n + rows]), return_counts=True)
    ri = keys // n
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(ri, minlength=n))
    deg = np.bincount(ri, weights=counts.astype(np.float64), minlength=n) * 0.5
    return indptr, (keys - ri * n).astype(np.int32), counts.astype(np.uint8), np.sqrt(deg)


@functools.lru_cache(maxsize=None)
def graph(name):
    g = symmetrise_numpy(lists(name))
    for a in g:
        a.setflags(write=False)
    return g


def dense_of(g):
    """The dense M of a CSR graph, each entry (0.5 weight) / (dd_i dd_j) as the kernel forms it."""
    indptr, indices, weight, dd = g
    n = len(dd)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    M = np.zeros((n, n))
    M[rows, indices] = (0.5 * weight) / (dd[rows] * dd[indices])
    return M


@functools.lru_cache(maxsize=None)
def sklearn_W(name):
    """W = 0.5 (A + A^T) as sklearn's SpectralClustering builds it (scipy CSR, the diagonal still in).  TIED: where distances tie exactly (the identical
    rows, and every point that is equally far from all of them) sklearn's brute-force order among equals is unspecified while the definition's is by index, so
    A comes from the exact lists there and sklearn is given the matrix (affinity='precomputed': the same code from there on)."""
    from scipy.sparse import csr_matrix
    from sklearn.neighbors import kneighbors_graph
    n, k = CASES[name][0], CASES[name][2]
    if name in TIED:
        A = csr_matrix((np.ones(n * k), lists(name).ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    else:
        A = kneighbors_graph(points(name).astype(np.float64), n_neighbors=k, include_self=True)
    return 0.5 * (A + A.T)


@functools.lru_cache(maxsize=None)
def yard(name):
    """``(lam (N,) descending, U (N, N) the eigenvectors in that order, dd)`` of the dense M from sklearn's graph."""
    W = np.asarray(sklearn_W(name).todense())
    np.fill_diagonal(W, 0.0)
    dd = np.sqrt(W.sum(1))
    M = W / np.outer(dd, dd)
    lam, U = np.linalg.eigh(0.5 * (M + M.T))
    lam, U = lam[::-1].copy(), U[:, ::-1].copy()
    for a in (lam, U, dd):
        a.setflags(write=False)
    return lam, U, dd


def yard_embedding(name, m):
    lam, U, dd = yard(name)
    return S.sign_flip_numpy(U[:, :m] / dd[:, None])


def same_partition(a, b):
    """Equal up to renumbering (ARI == 1)."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def max_row(name):
    return int(np.diff(graph(name)[0]).max())


def rounding(name):
    """(longest row + 16) 2^-52: the rounding term of the bounds."""
    return (max_row(name) + 16) * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def sklearn_labels(name, assign):
    from sklearn.cluster import SpectralClustering
    n, d, k, K, m, comps = CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name in TIED:
            return SpectralClustering(n_clusters=K, affinity='precomputed', assign_labels=assign, eigen_solver='arpack', random_state=0).fit(
                sklearn_W(name)).labels_
        return SpectralClustering(n_clusters=K, affinity='nearest_neighbors', n_neighbors=k, assign_labels=assign, eigen_solver='arpack',
                                  random_state=0).fit(points(name).astype(np.float64)).labels_


# ------------------------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize('name', list(CASES))
def test_conditions_of_the_cases(name):
    pytest.importorskip('sklearn')
    from scipy.sparse.csgraph import connected_components
    from sklearn.cluster import KMeans
    n, d, k, K, m, comps = CASES[name]
    lam, U, dd = yard(name)
    # the exact lists give sklearn's graph: the GPU graph can be compared with the numpy symmetrisation of the lists
    W = sklearn_W(name).copy()
    W.setdiag(0.0)
    W.eliminate_zeros()
    W.sort_indices()
    indptr, indices, weight, gdd = graph(name)
    assert np.array_equal(W.indptr, indptr) and np.array_equal(W.indices, indices) and np.array_equal(W.data, 0.5 * weight)
    assert np.array_equal(gdd, dd)
    assert np.abs(dense_of(graph(name)) - dense_of(graph(name)).T).max() == 0          # M_ij is formed symmetrically, bit for bit
    # clear: components, the gap after K and after m
    assert connected_components(W, directed=False)[0] == comps
    assert int((lam >= 1 - 10 * TOL).sum()) == comps and lam[0] <= 1 + 1e-12 and lam[-1] >= -1 - 1e-12
    gap = lam[K - 1] - lam[K]
    print('%s: gap after K = %d: %.3g; longest row %d; lam[:m + 1] = %s' % (name, K, gap, max_row(name), lam[:m + 1]))
    assert gap >= 1e-3
    # sklearn's labels, both ways, and k-means on the yardstick's embedding: one partition
    emb = yard_embedding(name, K)
    km = KMeans(K, n_init=10, random_state=0).fit(emb).labels_
    assert same_partition(sklearn_labels(name, 'kmeans'), km)
    assert same_partition(sklearn_labels(name, 'cluster_qr'), km)
    assert same_partition(S.cluster_qr(emb), km)
    assert len(set(km.tolist())) == K
    if name == 'overlap1030':          # the candidate shortcut the large case takes gives the lists of the yardstick the kNN tests use
        assert np.array_equal(lists(name), exact_lists(points(name), k))
    if name == 'd13':
        assert max_row(name) > 64
    if name == 'dups255':
        assert (points(name)[40:60] == points(name)[40]).all() and (lists(name)[40:60, :20] == np.arange(40, 60)).all()
    if name == 'overlap1030':          # single eigenvectors are comparable: the leading eigenvalues are distinct
        assert np.diff(lam[:K + 1]).max() <= -1e-3


def test_cluster_qr_equals_sklearns():
    pytest.importorskip('sklearn')
    from sklearn.cluster._spectral import cluster_qr
    for name in CASES:
        K = CASES[name][3]
        emb = yard_embedding(name, K)
        np.testing.assert_array_equal(S.cluster_qr(emb), cluster_qr(emb))
    rng = np.random.default_rng(0)
    for n, k in ((40, 1), (200, 5), (300, 12)):
        V = np.linalg.qr(rng.normal(size=(n, k)))[0]
        np.testing.assert_array_equal(S.cluster_qr(V), cluster_qr(V))


def test_sign_flip_equals_sklearns():
    pytest.importorskip('sklearn')
    from sklearn.utils.extmath import _deterministic_vector_sign_flip
    rng = np.random.default_rng(1)
    E = rng.normal(size=(50, 6))
    E[7, 2], E[31, 2] = 9.0, -9.0          # equal magnitude: the first one wins
    E[3, 4], E[12, 4] = -9.0, 9.0
    ref = _deterministic_vector_sign_flip(E.T.copy()).T
    np.testing.assert_array_equal(S.sign_flip_numpy(E), ref)
    np.testing.assert_array_equal(S.sign_flip(torch.as_tensor(E)).numpy(), ref)
    assert ref[7, 2] > 0 and ref[3, 4] > 0


def test_symmetrisation_equals_scipys():
    from scipy.sparse import csr_matrix
    rng = np.random.default_rng(2)
    n, k = 60, 7
    idx = np.stack([np.concatenate([[i], rng.choice(np.delete(np.arange(n), i), k - 1, replace=False)]) for i in range(n)]).astype(np.int32)
    A = csr_matrix((np.ones(n * k), idx.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    W = 0.5 * (A + A.T)
    W.setdiag(0.0)
    W.eliminate_zeros()
    W.sort_indices()
    indptr, indices, weight, dd = symmetrise_numpy(idx)
    assert np.array_equal(W.indptr, indptr) and np.array_equal(W.indices, indices) and np.array_equal(W.data, 0.5 * weight)
    assert np.array_equal(dd, np.sqrt(np.asarray(W.sum(1)).ravel()))
    got = S.symmetrise_lists(torch.as_tensor(idx))          # the torch build runs on any device
    for a, b in zip(got[:3], (indptr, indices, weight)):
        assert a.numpy().dtype == b.dtype and np.array_equal(a.numpy(), b)
    assert got[3].dtype == torch.float64 and (np.abs(got[3].numpy() - dd) <= np.spacing(dd)).all()          # (torch's vectorised sqrt: to 1 ulp)


def test_block_width():
    assert S._block_width(2, 17) == 6 and S._block_width(10, 4100) == 15 and S._block_width(32, 10 ** 5) == 48 and S._block_width(4, 5) == 5


# ------------------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    X = np.zeros((5, 4), np.float32)
    for call in (lambda **kw: S.spectral_graph(X, **kw), lambda **kw: S.spectral_embedding(X, 2, **kw),
                 lambda **kw: S.SpectralClustering(2, **kw).fit(X), lambda **kw: S.spectral_sweep(X, [2], **kw)):
        with pytest.raises(ValueError, match='n_neighbors must be >= 2'):
            call(n_neighbors=1)
        with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit, but n_neighbors = 6, n_samples_fit = 5, n_samples = 5'):
            call(n_neighbors=6)
        with pytest.raises(ValueError, match='integer'):
            call(n_neighbors=2.5)
    with pytest.raises(NotImplementedError, match='at most 1024 neighbours'):
        S.spectral_graph(np.zeros((1100, 4), np.float32), 1025)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        S.spectral_graph(np.zeros((5, 260), np.float32), 2)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        S.SpectralClustering(2, 2).fit(torch.zeros(5, 260))
    with pytest.raises(ValueError, match='2-D'):
        S.spectral_graph(np.zeros(5, np.float32), 2)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        S.spectral_embedding(np.zeros((50, 4), np.float32), N.MAX_CLUSTERS + 1, 3)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        S.SpectralClustering(N.MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        S.SpectralClustering(2, n_components=N.MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match='should be <= n_samples'):
        S.SpectralClustering(6, 3).fit(X)
    with pytest.raises(ValueError, match='smaller than the largest number of clusters'):
        S.SpectralClustering(4, 3, n_components=3).fit(X)
    with pytest.raises(ValueError, match='assign_labels'):
        S.SpectralClustering(2, assign_labels='discretize')
    with pytest.raises(ValueError, match='must be an int >= 1'):
        S.SpectralClustering(0)
    with pytest.raises(ValueError, match='at least one'):
        S.spectral_sweep(X, [])
    assert not hasattr(S.SpectralClustering, 'predict')
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU path'):
            S.spectral_embedding(X, 2, 3)
        with pytest.raises(RuntimeError, match='no CPU path'):
            S.SpectralClustering(2, 3).fit(X)


def test_module_does_not_import_scipy_or_sklearn():
    with open(S.__file__) as f:
        text = f.read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', text, flags=re.M)


def test_header_and_signatures_agree():
    names = {'dic_spectral_spmm', 'dic_spectral_gram_workspace', 'dic_spectral_gram', 'dic_spectral_rotate'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    assert len(N.SIGNATURES['dic_spectral_spmm'][1]) == 14 and len(N.SIGNATURES['dic_spectral_gram'][1]) == 8
    assert set(N.header_symbols()) == set(N.SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    odd = ctypes.c_void_p((1 << 20) + 4)

    def spmm(indptr=fake, indices=fake, weight=fake, dd=fake, n=1000, nnz=5000, b=6, X=fake, Z=None, Y=ctypes.c_void_p(1 << 21)):
        return lib.dic_spectral_spmm(indptr, indices, weight, dd, n, nnz, b, X, Z, 1.0, 0.0, 0.0, Y, None)

    def gram(A=fake, B=fake, n=1000, b=6, G=fake, ws=fake, nbytes=1 << 20):
        return lib.dic_spectral_gram(A, B, n, b, G, ws, nbytes, None)

    def rotate(X=fake, C=fake, n=1000, b=6, Y=ctypes.c_void_p(1 << 21)):
        return lib.dic_spectral_rotate(X, C, n, b, Y, None)

    for call, pointers in ((spmm, ('indptr', 'indices', 'weight', 'dd', 'X', 'Y')), (gram, ('A', 'B', 'G', 'ws')), (rotate, ('X', 'C', 'Y'))):
        for name in pointers:
            assert call(**{name: None}) == -1 and b'NULL' in lib.dic_last_error_string(), name
        for kw in ({'n': 0}, {'n': -3}, {'b': 0}):
            assert call(**kw) == -1 and b'expected N >= 1, b >= 1' in lib.dic_last_error_string(), kw
        assert call(b=65) == -2 and b'at most 64 columns' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
    assert spmm(nnz=-1) == -1 and b'nnz' in lib.dic_last_error_string()
    assert spmm(Y=fake) == -1 and b'Y must not be X' in lib.dic_last_error_string()
    assert rotate(Y=fake) == -1 and b'Y must not be X' in lib.dic_last_error_string()
    for kw in ({'indptr': odd}, {'dd': odd}, {'X': odd}, {'Z': odd}, {'Y': odd}, {'indices': ctypes.c_void_p((1 << 20) + 2)}):
        assert spmm(**kw) == -2 and b'aligned' in lib.dic_last_error_string(), kw
    for kw in ({'A': odd}, {'B': odd}, {'G': odd}, {'ws': odd}):
        assert gram(**kw) == -2 and b'aligned' in lib.dic_last_error_string()
    assert gram(nbytes=64) == -3 and b'needed' in lib.dic_last_error_string()
    assert lib.dic_spectral_gram_workspace(1000, 6) == 2304 and lib.dic_spectral_gram_workspace(1000, 65) == 0          # 8 workgroups x 36 sums x 8 bytes


# ------------------------------------------------------------------------------------------------------------------------------------------ parsers
def test_p2_parser_accepts_the_spectral_flags():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    a = p2.get_arguments([])
    assert (a.cluster_method, a.spectral_k, a.spectral_assign) == ('kmeans', 10, 'kmeans')
    a = p2.get_arguments(['--cluster_method', 'spectral', '--spectral_k', '25', '--spectral_assign', 'cluster_qr', '--k_max', '6'])
    assert (a.cluster_method, a.spectral_k, a.spectral_assign, a.k_max) == ('spectral', 25, 'cluster_qr', 6)
    with pytest.raises(SystemExit):
        p2.get_arguments(['--spectral_assign', 'discretize'])
    for k_max in (1, 0, N.MAX_CLUSTERS, 100):          # k_max + 1 eigenpairs must fit the compiled limit: refused in the driver's own words, before any file
        with pytest.raises(ValueError, match='--k_max must lie in .2, %d.' % (N.MAX_CLUSTERS - 1)):
            p2.Spectral(k_max, '/nonexistent/never/made', [])
    assert not os.path.exists('/nonexistent')


def test_p4_parser_accepts_the_spectral_flags_and_admits_knn_transfer(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p4.get_arguments([])
    assert (a.cluster_method, a.spectral_k, a.spectral_assign) == ('kmeans', 10, 'kmeans')
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'spectral', '--transfer', 'knn', '--num_clusters', '3'])
    args.restore_metric = ['ae_mse']
    with pytest.raises(FileNotFoundError):          # past the refusal: it goes on to read the latents, which are not there
        p4.main(args)


# --------------------------------------------------------------------------------------------------------------------------------------- registers
def test_spectral_kernels_do_not_spill_to_scratch():
    """The SpMM runs hundreds of times per fit: require ScratchSize == 0 and no vector-register spills for every kernel of dic_spectral.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_spectral.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'warning' not in res.stderr
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('spectral_spmm_kernel', 'spectral_gram_kernel', 'spectral_gram_sum_kernel', 'spectral_rotate_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills) == 11          # six widths of the SpMM, three of the gram kernel, the sum and the rotation
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
