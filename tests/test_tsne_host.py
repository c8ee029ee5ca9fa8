"""t-SNE (tsne.py, csrc/dic_tsne.hip): the definition in numpy f64, held against sklearn where sklearn is installed, and what needs no GPU.

The functions below ARE the definition the GPU tests (test_gpu_tsne.py) and scripts/tsne_probe.py compare against: the conditional p by sklearn's
bracket-and-bisect search, the dense gradient / KL / Z, the update rule of sklearn's ``_gradient_descent`` and the placement ``transform`` makes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import tsne as T

ENTROPY_TOL, MAX_STEPS = 1e-10, 200


# ------------------------------------------------------------------------------------------------------------------------------------ definition
def blobs(n=600, d=16, seed=0):
    """Three well-separated gaussian blobs (centres 4 N(0, 1) per coordinate, unit noise): ``(X (n, d) f32, blob label (n,))``."""
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(3, d)) * 4
    lab = rng.integers(0, 3, n)
    return (cent[lab] + rng.normal(size=(n, d))).astype(np.float32), lab


def neighbour_lists(X, k):
    """``(dist (n, k) f64, idx (n, k))``: the k nearest other points of every point, sorted by (distance, index); f64 difference form of the coordinates."""
    x = np.asarray(X, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def cond_p(d2, perplexity):
    """``(p (m, k), beta (m,), capped (m,) bool)`` from squared distances (m, k): include/dic_hip.h, dic_tsne_perplexity.  p and beta are those of the last
    evaluation; ``capped`` marks the rows that ended at the 200th evaluation and not by the entropy tolerance."""
    d2 = np.asarray(d2, dtype=np.float64)
    logu = np.log(perplexity)
    p, beta, capped = np.empty_like(d2), np.empty(len(d2)), np.zeros(len(d2), dtype=bool)
    for i, row in enumerate(d2):
        r = row - row.min()
        b, lo, hi = 1.0, -np.inf, np.inf
        for step in range(MAX_STEPS):
            e = np.exp(-b * r)
            s = e.sum()
            diff = np.log(s) + b * (r * e).sum() / s - logu
            if abs(diff) <= ENTROPY_TOL:
                break
            if step == MAX_STEPS - 1:
                capped[i] = True
                break
            if diff > 0:
                lo = b
                b = b * 2.0 if hi == np.inf else 0.5 * (b + hi)
            else:
                hi = b
                b = b * 0.5 if lo == -np.inf else 0.5 * (b + lo)
        p[i], beta[i] = e / s, b
    return p, beta, capped


def joint_dense(idx, p):
    """The dense symmetric P (n, n) of the lists ``idx`` (n, k) and their conditional ``p``: (p_j|i + p_i|j) / total."""
    n = len(idx)
    C = np.zeros((n, n))
    C[np.repeat(np.arange(n), idx.shape[1]), idx.ravel()] = p.ravel()
    S = C + C.T
    return S / S.sum()


def csr_dense(graph):
    indptr, indices, data = (np.asarray(a) for a in graph)
    n = len(indptr) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    return A


def dense_objective(Y, Pd, exaggeration=1.0):
    """``(kl, grad (n, 2), Z, bound (n, 2))`` of the map Y under e Pd: q = 1 / (1 + d^2) off the diagonal, Z = sum q, w = (e P - q / Z) q,
    grad_i = 4 sum_j w_ij (y_i - y_j), KL = sum e P log(e P / (q / Z)) over P > 0; ``bound`` = 4 sum_j |w_ij| |y_i - y_j|, the terms a summation error
    is measured in."""
    Y = np.asarray(Y, dtype=np.float64)
    d = Y[:, None, :] - Y[None, :, :]
    d2 = (d ** 2).sum(-1)
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    Pe = exaggeration * Pd
    W = (Pe - q / Z) * q
    grad = 4.0 * (W[:, :, None] * d).sum(1)
    bound = 4.0 * (np.abs(W)[:, :, None] * np.abs(d)).sum(1)
    m = Pd > 0
    kl = float(np.sum(Pe[m] * (np.log(Pe[m]) + np.log1p(d2[m]) + np.log(Z))))
    return kl, grad, float(Z), bound


def descend(Y0, Pd, iters, lr, early_exaggeration=12.0, pert=0.0, seed=1):
    """``iters`` iterations of sklearn's ``_gradient_descent`` from Y0 on ``dense_objective``: 250 at the exaggeration and momentum 0.5, then 1 and 0.8.
    ``pert``: every gradient is multiplied by 1 + pert N(0, 1) per entry -- a stand-in for a kernel with that relative error.  Returns (Y, the last KL)."""
    rng = np.random.default_rng(seed)
    Y = np.array(Y0, dtype=np.float64)
    U, G = np.zeros_like(Y), np.ones_like(Y)
    kl = np.nan
    for it in range(iters):
        e, mom = (early_exaggeration, 0.5) if it < T.EXPLORATION_ITER else (1.0, 0.8)
        kl, g, _, _ = dense_objective(Y, Pd, e)
        if pert:
            g = g * (1.0 + pert * rng.standard_normal(g.shape))
        G = np.maximum(np.where(U * g < 0.0, G + 0.2, G * 0.8), 0.01)
        U = mom * U - lr * (g * G)
        Y = Y + U
    return Y, kl


def transform_ref(Y_train, dist, idx, perplexity):
    """The placement of queries with neighbour lists (dist, idx) into the training map: the p-weighted mean of the neighbours' positions."""
    p, _, _ = cond_p(np.asarray(dist, dtype=np.float64) ** 2, perplexity)
    return (p[:, :, None] * np.asarray(Y_train)[np.asarray(idx)]).sum(1)


def same_blob_share(Y, lab, k=5):
    """The share of points whose k nearest map neighbours all carry the point's blob label."""
    _, idx = neighbour_lists(Y, k)
    return float(np.mean((lab[idx] == lab[:, None]).all(1)))


def trustworthiness(X, Y, k=5):
    """``sklearn.manifold.trustworthiness(X, Y, n_neighbors=k)`` (Venna and Kaski 2001): 1 - 2 / (n k (2 n - 3 k - 1)) sum_i sum_{j in U_i} (r(i, j) - k)
    with U_i the k nearest map neighbours of i and r(i, j) the rank of j among the input-space neighbours of i (1 = the nearest)."""
    x = np.asarray(X, dtype=np.float64)
    n = len(x)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind='stable')
    rank = np.empty((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order] = np.arange(1, n + 1)[None, :]
    _, idx = neighbour_lists(Y, k)
    excess = np.take_along_axis(rank, idx, axis=1) - k
    return 1.0 - 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)) * float(excess[excess > 0].sum())


# ------------------------------------------------------------------------------------------------------------------------------- against sklearn
@pytest.fixture(scope='module')
def blob_p():
    X, lab = blobs()
    dist, idx = neighbour_lists(X, T.n_neighbors_of(30.0, len(X)))
    p, beta, capped = cond_p(dist ** 2, 30.0)
    return X, dist, idx, p, joint_dense(idx, p)


def test_joint_p_against_sklearn(blob_p):
    """sklearn searches in f32 with an entropy tolerance of 1e-5: observed 5.2e-6 of the largest entry, allowed 1e-4 of it."""
    pytest.importorskip('scipy')
    tsne_mod = pytest.importorskip('sklearn.manifold._t_sne')
    if not hasattr(tsne_mod, '_joint_probabilities_nn'):
        pytest.skip('this sklearn has no _joint_probabilities_nn')
    from sklearn.neighbors import NearestNeighbors
    X, dist, idx, p, Pd = blob_p
    G = NearestNeighbors(n_neighbors=idx.shape[1]).fit(X).kneighbors_graph(mode='distance')
    G.data **= 2
    ref = tsne_mod._joint_probabilities_nn(G, 30.0, 0).toarray()
    err = np.abs(ref - Pd).max() / ref.max()
    print('joint P: max abs difference / largest entry = %.3g' % err)
    assert (np.abs(p.sum(1) - 1) <= 1e-14).all() and abs(Pd.sum() - 1) <= 1e-12 and np.array_equal(Pd, Pd.T)
    assert err <= 1e-4


@pytest.mark.parametrize('exaggeration', [1.0, 12.0])
@pytest.mark.parametrize('scale', [1e-4, 10.0])
def test_kl_and_gradient_against_sklearn(blob_p, scale, exaggeration):
    """``_kl_divergence`` on the densified P: observed 1.6e-15 relative, allowed 1e-12."""
    squareform = pytest.importorskip('scipy.spatial.distance').squareform
    tsne_mod = pytest.importorskip('sklearn.manifold._t_sne')
    if not hasattr(tsne_mod, '_kl_divergence'):
        pytest.skip('this sklearn has no _kl_divergence')
    Pd = blob_p[4]
    n = len(Pd)
    Y = np.random.default_rng(5).normal(size=(n, 2)) * scale
    kl, grad, _, _ = dense_objective(Y, Pd, exaggeration)
    kl_ref, grad_ref = tsne_mod._kl_divergence(Y.ravel(), squareform(exaggeration * Pd, checks=False), 1.0, n, 2)
    print('kl %.17g sklearn %.17g; gradient: max abs difference / max abs = %.3g' % (kl, kl_ref, np.abs(grad.ravel() - grad_ref).max() / np.abs(grad_ref).max()))
    assert abs(kl - kl_ref) <= 1e-12 * abs(kl_ref)
    assert np.abs(grad.ravel() - grad_ref).max() <= 1e-12 * np.abs(grad_ref).max()


def test_trustworthiness_against_sklearn():
    manifold = pytest.importorskip('sklearn.manifold')
    X, _ = blobs(300, 8, seed=3)
    rng = np.random.default_rng(4)
    for Y in (X[:, :2].astype(np.float64), rng.normal(size=(300, 2))):
        assert abs(trustworthiness(X, Y, 5) - manifold.trustworthiness(X, Y, n_neighbors=5)) <= 1e-12


def test_definition_handles_duplicates_and_the_step_cap():
    """A row whose nearest entries are all at distance 0, more of them than the perplexity: the entropy never comes down to log(perplexity), beta doubles
    to the cap and p is uniform over the zeros."""
    d2 = np.concatenate([np.zeros(8), np.linspace(1.0, 2.0, 8)])[None, :]
    p, beta, capped = cond_p(d2, 5.0)
    assert capped[0] and beta[0] == 2.0 ** (MAX_STEPS - 1) and np.array_equal(p[0], np.r_[np.full(8, 0.125), np.zeros(8)])
    p, beta, capped = cond_p(d2, 12.0)          # reachable: 8 zeros < 12
    assert not capped[0] and abs(-(p[p > 0] * np.log(p[p > 0])).sum() - np.log(12.0)) <= 2e-10


# ---------------------------------------------------------------------------------------------------------------------------------- without a GPU
def test_value_errors_before_any_gpu_work():
    X = np.zeros((100, 8), np.float32)
    with pytest.raises(ValueError, match='n_components'):
        T.TSNE(n_components=3)
    with pytest.raises(ValueError, match='perplexity must be less than'):
        T.TSNE(perplexity=99.0).fit(X)
    with pytest.raises(ValueError, match='perplexity must be less than'):
        T.joint_probabilities(X, 99.0)
    T._check(100, 8, 98.9)          # (N - 1 itself is the first value refused)
    big = np.zeros((2000, 8), np.float32)
    with pytest.raises(ValueError, match='at most 1024'):
        T.TSNE(perplexity=341.0).fit(big)          # int(3 * 341 + 1) + 1 = 1025
    with pytest.raises(ValueError, match='at most 1024'):
        T.tsne_sweep(big, [30.0, 341.0])
    T._check(2000, 8, 340.9)          # 1023 + 1 = 1024: the widest list
    with pytest.raises(ValueError, match='n_components'):
        T.tsne_sweep(X, [5.0], n_components=3)
    with pytest.raises(ValueError, match='features'):
        T.TSNE(perplexity=5.0).fit(np.zeros((100, 260), np.float32))
    with pytest.raises(ValueError, match='2-D'):
        T.TSNE(perplexity=5.0).fit(np.zeros(100, np.float32))
    with pytest.raises(ValueError, match='init'):
        T.TSNE(perplexity=5.0, init='spectral')
    with pytest.raises(ValueError, match='init'):
        T.TSNE(perplexity=5.0, init=np.zeros((99, 2))).fit(X)
    with pytest.raises(ValueError, match='max_iter'):
        T.TSNE(max_iter=100)
    with pytest.raises(ValueError, match='perplexity'):
        T.TSNE(perplexity=0.0).fit(X)
    with pytest.raises(RuntimeError, match='not fitted'):
        T.TSNE().transform(X)
    assert T.n_neighbors_of(30.0, 75000) == 91 and T.n_neighbors_of(30.0, 50) == 49


def test_cli_options():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    for mod in (p2, p4):
        a = mod.get_arguments([])
        assert a.embed is None and a.tsne_perplexity == 30.0 and a.tsne_max_iter == 1000
        a = mod.get_arguments(['--cluster_method', 'ward', '--embed', 'tsne', '--tsne_perplexity', '12.5', '--tsne_max_iter', '300'])
        assert a.embed == 'tsne' and a.tsne_perplexity == 12.5 and a.tsne_max_iter == 300 and a.cluster_method == 'ward'
        with pytest.raises(SystemExit):
            mod.get_arguments(['--embed', 'umap'])


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    err = lib.dic_last_error_string

    def perp(d2=fake, m=10, k=91, u=30.0, beta=fake, p=fake):
        return lib.dic_tsne_perplexity(d2, m, k, u, beta, p, None)
    for kw in ({'d2': None}, {'beta': None}, {'p': None}):
        assert perp(**kw) == -1 and b'NULL' in err()
    assert perp(k=0) == -1 and perp(m=0) == -1 and perp(u=0.0) == -1 and perp(u=float('nan')) == -1 and perp(u=float('inf')) == -1
    assert perp(k=1025) == -2 and b'at most 1024' in err()
    assert perp(d2=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in err()

    ws = lib.dic_tsne_repulsion_workspace(1000)
    assert ws > 0 and lib.dic_tsne_repulsion_workspace(1) == 0 and lib.dic_tsne_repulsion_workspace(1 << 30) == 0
    assert lib.dic_tsne_repulsion(None, 1000, fake, ws, None) == -1 and lib.dic_tsne_repulsion(fake, 1000, None, ws, None) == -1
    assert lib.dic_tsne_repulsion(fake, 1, fake, ws, None) == -1 and lib.dic_tsne_repulsion(fake, 1 << 30, fake, 1 << 40, None) == -2
    assert lib.dic_tsne_repulsion(fake, 1000, fake, ws - 1, None) == -3 and b'workspace' in err()
    assert lib.dic_tsne_repulsion(ctypes.c_void_p((1 << 20) + 8), 1000, fake, ws, None) == -2 and b'16-B' in err()

    def step(indptr=fake, indices=fake, pval=fake, n=1000, nnz=5000, Y=fake, work=fake, nbytes=ws, e=1.0, update=fake, gains=fake, Ynew=ctypes.c_void_p(1 << 21),
             grad=None, partials=fake):
        return lib.dic_tsne_step(indptr, indices, pval, n, nnz, Y, work, nbytes, e, 0.5, 200.0, update, gains, Ynew, grad, partials, None)
    for kw in ({'indptr': None}, {'indices': None}, {'pval': None}, {'Y': None}, {'work': None}, {'partials': None}):
        assert step(**kw) == -1 and b'NULL' in err()
    assert step(update=None) == -1 and b'go together' in err()
    assert step(update=None, gains=None, Ynew=None) == -1 and b'nothing to do' in err()
    assert step(Ynew=fake) == -1 and b'must not be Y' in err()
    assert step(nnz=-1) == -1 and step(e=0.0) == -1 and step(n=1) == -1
    assert step(nbytes=ws - 1) == -3 and b'workspace' in err()


def test_splits_and_workspace_are_functions_of_n(lib):
    """The column splits fix the order of the repulsion's sums: a function of N alone, at least 512 columns each, enough workgroups at the workload's N."""
    assert lib.dic_tsne_splits(257) == 1 and lib.dic_tsne_splits(600) == 2 and lib.dic_tsne_splits(1000) == 2
    s = lib.dic_tsne_splits(75000)
    assert s * ((75000 + 255) // 256) >= 2048 and s <= 64
    sizes = [lib.dic_tsne_repulsion_workspace(n) for n in (2, 255, 256, 257, 600, 1000, 5000, 75000, 300000)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.dic_tsne_repulsion_workspace(75000) < 64 * 3 * 8 * 75000 + (1 << 20)          # O(S N), nothing N x N
    assert lib.dic_tsne_step_partials(75000) == 18750 and lib.dic_tsne_step_partials(257) == 65 and lib.dic_tsne_step_partials(1) == 0


def test_tsne_kernels_do_not_spill_to_scratch():
    """The repulsion kernel keeps four rows' coordinates and twelve f64 sums per lane, the perplexity kernel up to 16 distances and 16 weights: require
    ScratchSize == 0 and no spills for every kernel of dic_tsne.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_tsne.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    assert sum('tsne_perplexity_kernel' in n for n in names) == 5
    for kernel in ('tsne_repulsion_kernel', 'tsne_zrows_kernel', 'tsne_zsum_kernel', 'tsne_step_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
