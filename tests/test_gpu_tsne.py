"""Exact t-SNE on the MI355X (tsne.py, csrc/dic_tsne.hip) against the numpy definition of test_tsne_host.py.

Every bound below is about the kernels' arithmetic, not about what they were seen to give: the unit roundoff of f64 (u = 2^-53), the number of terms of a
sum, the entropy tolerance of the perplexity search, and the spread of the numpy definition itself under rounding-sized noise (scripts/tsne_probe.py,
tests/golden/tsne_spread.json)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import knn as K
from deep_interpolation_clustering_amd import tsne as T
from deep_interpolation_clustering_amd.info import COHORTS
from test_gpu_optics import _write_latents
from test_tsne_host import (blobs, cond_p, csr_dense, dense_objective, descend, same_blob_share, transform_ref, trustworthiness)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tsne_spread.json')


@functools.lru_cache(maxsize=None)
def points(name):
    """'n257', 'n600', 'n1000': three blobs in 16 dimensions (no size a multiple of 256); 'dup': 300 such points, 40 of them copies of one point -- more
    copies than either perplexity, so those rows never reach the entropy and end at the step cap with beta = 2^199."""
    if name == 'dup':
        X, lab = blobs(300, 16, seed=2)
        X[260:300] = X[0]
        lab[260:300] = lab[0]
        return X, lab
    return blobs({'n257': 257, 'n600': 600, 'n1000': 1000}[name], 16, seed={'n257': 1, 'n600': 0, 'n1000': 3}[name])


@functools.lru_cache(maxsize=None)
def conditional(name, perplexity):
    """The lists without the point itself and the kernel's (beta, p), all numpy."""
    X, _ = points(name)
    k = T.n_neighbors_of(perplexity, len(X))
    dist, idx = T.drop_self(*K.kneighbors(X, k + 1, return_device=True))
    beta, p = T.conditional_probabilities(dist * dist, perplexity)
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64), beta.cpu().numpy(), p.cpu().numpy()


@functools.lru_cache(maxsize=None)
def affinities(name, perplexity=30.0):
    """``joint_probabilities`` as numpy and its dense form."""
    graph = T.joint_probabilities(points(name)[0], perplexity)
    return graph, csr_dense(graph)


def random_init(n, seed=0):
    return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------------------- perplexity kernel
@pytest.mark.parametrize('perplexity', [5.0, 30.0])
@pytest.mark.parametrize('name', ['n257', 'n600', 'dup'])
def test_perplexity_kernel(name, perplexity):
    dist, idx, beta, p = conditional(name, perplexity)
    n, k = p.shape
    assert k == int(3 * perplexity + 1) and np.isfinite(p).all() and np.isfinite(beta).all() and (p >= 0).all()
    d2 = dist ** 2
    r = d2 - d2.min(1, keepdims=True)
    row_err = np.abs(p.sum(1) - 1).max()
    # where the step cap did not bind the entropy is within the search's tolerance (1e-10) of log(perplexity); 2e-10 leaves the rounding of this recomputation
    _, _, capped = cond_p(d2, perplexity)
    logp = np.log(np.where(p > 0, p, 1.0))
    H = -(p * logp).sum(1)
    h_err = np.abs(H - np.log(perplexity))[~capped].max()
    print('%s perplexity %g: rows %d, capped %d, max |row sum - 1| %.3g, max |H - log u| %.3g' % (name, perplexity, n, capped.sum(), row_err, h_err))
    assert row_err <= k * 2.0 ** -52
    assert h_err <= 2e-10
    if name == 'dup':          # the 40 copies and the point they copy: 40 zeros in a row of which perplexity < 40 can never be reached
        zero_rows = (d2[:, :39] == 0).all(1)
        assert zero_rows.sum() == 41 and capped[zero_rows].all() and (beta[zero_rows] == 2.0 ** 199).all()
    else:
        assert not capped.any()
    # p is exp(-beta r) / sum of the RETURNED beta
    e = np.exp(-beta[:, None] * r)
    np.testing.assert_allclose(p, e / e.sum(1, keepdims=True), rtol=1e-12, atol=0)


@pytest.mark.parametrize('perplexity', [5.0, 30.0])
@pytest.mark.parametrize('name', ['n257', 'n600', 'dup'])
def test_joint_p(name, perplexity):
    _, idx, _, _ = conditional(name, perplexity)
    n, k = idx.shape
    indptr, indices, data = T.joint_probabilities(points(name)[0], perplexity)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64 and indptr[0] == 0 and indptr[-1] == len(indices) == len(data)
    stored = np.zeros((n, n), dtype=bool)
    stored[np.repeat(np.arange(n), np.diff(indptr)), indices] = True
    assert stored.sum() == len(indices)          # no entry twice
    wanted = np.zeros((n, n), dtype=bool)          # the definition's pattern: j in L(i) or i in L(j)
    wanted[np.repeat(np.arange(n), k), idx.ravel()] = True
    wanted |= wanted.T
    assert np.array_equal(stored, wanted) and not stored.diagonal().any()
    for i in range(n):
        assert (np.diff(indices[indptr[i]:indptr[i + 1]]) > 0).all()
    P = csr_dense((indptr, indices, data))
    assert same_bytes(P, P.T.copy())
    assert abs(data.sum() - 1) <= 1e-12 and (data >= 0).all()


# ------------------------------------------------------------------------------------------------------------------------- gradient, Z and KL
@pytest.mark.parametrize('exaggeration', [1.0, 12.0])
@pytest.mark.parametrize('scale', [1e-4, 10.0])
@pytest.mark.parametrize('name', ['n257', 'n600', 'n1000'])
def test_gradient_z_and_kl(name, scale, exaggeration):
    """Every sum of the kernels has at most N terms, each formed with a handful of roundings: |error| <= 8 N u times the sum of the terms' magnitudes."""
    graph, Pd = affinities(name)
    n = len(Pd)
    Y = np.random.default_rng(n).normal(size=(n, 2)) * scale
    Y[7] = Y[3]          # two coincident map points: q = 1 between them, no force
    Y[n - 1] = Y[n - 2]          # and two in the padded last block
    kl_ref, grad_ref, z_ref, bound = dense_objective(Y, Pd, exaggeration)
    kl, grad, z = T.tsne_gradient(Y, graph, exaggeration)
    tol = 8 * n * U
    worst = np.max(np.abs(grad - grad_ref) / bound)
    print('%s scale %g e %g: max |grad - ref| / bound term %.3g (allowed %.3g); Z rel %.3g; KL rel %.3g'
          % (name, scale, exaggeration, worst, tol, abs(z - z_ref) / z_ref, abs(kl - kl_ref) / abs(kl_ref)))
    assert (bound > 0).all() and np.isfinite(grad).all()
    assert (np.abs(grad - grad_ref) <= tol * bound).all()
    assert abs(z - z_ref) <= tol * z_ref
    assert abs(kl - kl_ref) <= tol * abs(kl_ref)


def test_gradient_takes_device_tensors_and_repeats():
    graph, _ = affinities('n600')
    Y = random_init(600, 3) * 1e4
    a = T.tsne_gradient(Y, graph, 12.0)
    dev = torch.device('cuda', torch.cuda.current_device())
    b = T.tsne_gradient(torch.as_tensor(Y, device=dev), tuple(torch.as_tensor(g, device=dev) for g in graph), 12.0)
    assert a[0] == b[0] and a[2] == b[2] and same_bytes(a[1], b[1])
    with pytest.raises(ValueError, match='rows'):
        T.tsne_gradient(Y[:-1], graph)


# ---------------------------------------------------------------------------------------------------------------------------------- trajectory
def test_trajectory_against_the_definition():
    """20 exaggerated iterations (e = 12, momentum 0.5, learning rate 50) from the random init of the full-fit test, on the device's own P, against the numpy
    definition: max|Y - Y_ref| <= 1e-10 max|Y_ref|.  scripts/tsne_probe.py on this data: the definition run beside itself deviates by 2.1e-14 max|Y| at
    iteration 20 when its gradients carry 1e-15 relative noise (rounding order), and by 2.2e-6 when they carry 1e-7 (f32 pair terms).  1e-10 is more than
    100x from either, so the issue's bound stands: it passes any f64 summation order and fails any f32-sized error."""
    graph, Pd = affinities('n600')
    Y0 = random_init(600)
    ref, _ = descend(Y0, Pd, 20, 50.0, 12.0)
    Y = T.tsne_descend(Y0, graph, 20, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    dev = np.abs(Y - ref).max() / np.abs(ref).max()
    print('trajectory: max|Y - Y_ref| / max|Y_ref| after 20 iterations = %.3g' % dev)
    assert dev <= 1e-10


# -------------------------------------------------------------------------------------------------------------------------------- repeatability
def test_two_fits_give_identical_bits():
    X, _ = points('n600')
    kw = dict(perplexity=30.0, max_iter=300, init='random', random_state=0)
    a, b = T.TSNE(**kw).fit(X), T.TSNE(**kw).fit(torch.as_tensor(X, device='cuda'))
    assert same_bytes(a.embedding_, b.embedding_) and a.kl_history_ == b.kl_history_ and a.kl_divergence_ == b.kl_divergence_
    assert same_bytes(a.betas_, b.betas_) and all(same_bytes(u, v) for u, v in zip(a.affinities_, b.affinities_))
    assert [it for it, _ in a.kl_history_] == [50, 100, 150, 200, 250, 300] and a.n_iter_ == 300 and a.learning_rate_ == 50.0
    assert same_bytes(T.TSNE(**kw).fit_transform(X), a.embedding_)


def test_sweep_is_one_join_and_equals_the_stand_alone_fits(monkeypatch):
    X, _ = points('dup')          # (duplicates: where the point itself is not among its own first neighbours the prefix rule matters)
    kw = dict(max_iter=250, init='random', random_state=0)
    calls = []
    real = T.kneighbors
    monkeypatch.setattr(T, 'kneighbors', lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    fits = T.tsne_sweep(X, [5.0, 30.0], **kw)
    assert calls == [92] and sorted(fits) == [5.0, 30.0]
    for u in (5.0, 30.0):
        alone = T.TSNE(perplexity=u, **kw).fit(X)
        assert same_bytes(fits[u].embedding_, alone.embedding_) and same_bytes(fits[u].betas_, alone.betas_)
        assert all(same_bytes(a, b) for a, b in zip(fits[u].affinities_, alone.affinities_))


# ------------------------------------------------------------------------------------------------------------------------------------- full fit
@functools.lru_cache(maxsize=None)
def full_fit():
    return T.TSNE(perplexity=30.0, max_iter=500, init='random', random_state=0).fit(points('n600')[0])


def test_full_fit_quality():
    """Positions are chaotic past iteration 50, so the fit is held to the QUALITY of the numpy definition run from the same init five times with 1e-15
    gradient noise (tests/golden/tsne_spread.json): KL no larger than the largest + 3 x their spread, trustworthiness no smaller than the smallest - 3 x
    theirs, and every point's five nearest map neighbours in its own blob for 99 % of the points (the definition's runs meet that: recorded there)."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold['n'] == 600 and gold['iters'] == 500 and min(gold['same_blob_share']) >= 0.99
    X, lab = points('n600')
    fit = full_fit()
    trust = trustworthiness(X, fit.embedding_, 5)
    share = same_blob_share(fit.embedding_, lab, 5)
    kl_max = max(gold['kl']) + 3 * (max(gold['kl']) - min(gold['kl']))
    trust_min = min(gold['trustworthiness']) - 3 * (max(gold['trustworthiness']) - min(gold['trustworthiness']))
    print('full fit: kl %.6f (allowed %.6f), trustworthiness %.6f (at least %.6f), same-blob share %.4f' % (fit.kl_divergence_, kl_max, trust, trust_min, share))
    assert fit.n_iter_ == 500 and np.isfinite(fit.embedding_).all()
    assert fit.kl_divergence_ <= kl_max
    assert trust >= trust_min
    assert share >= 0.99
    # the error of the last iteration is that of the definition at the map before the last update: recompute it at the final map for the order of magnitude
    assert abs(dense_objective(fit.embedding_, csr_dense(fit.affinities_))[0] - fit.kl_divergence_) <= 1e-2 * fit.kl_divergence_


def test_pca_init_is_sklearns():
    X, _ = points('n257')
    dev = torch.device('cuda', torch.cuda.current_device())
    Y = T.pca_init(X, dev).cpu().numpy()
    xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    _, _, vt = np.linalg.svd(xc, full_matrices=False)
    comp = vt[:2] * np.sign(vt[:2][np.arange(2), np.argmax(np.abs(vt[:2]), axis=1)])[:, None]          # svd_flip(u_based_decision=False)
    ref = xc @ comp.T
    ref = ref / ref[:, 0].std() * 1e-4
    np.testing.assert_allclose(Y, ref, rtol=1e-9, atol=1e-15)
    assert abs(Y[:, 0].std() - 1e-4) <= 1e-16
    fit = T.TSNE(perplexity=10.0, max_iter=250).fit(X)          # the default init runs
    assert fit.n_iter_ == 250 and np.isfinite(fit.embedding_).all()


# ------------------------------------------------------------------------------------------------------------------------------------ transform
def test_transform_places_held_out_points():
    X, lab = points('n600')
    Xt, Xq, lt, lq = X[:500], X[500:], lab[:500], lab[500:]
    fit = T.TSNE(perplexity=30.0, max_iter=500, init='random', random_state=0).fit(Xt)
    before = fit.embedding_.copy()
    Yq = fit.transform(Xq)
    assert Yq.shape == (100, 2) and Yq.dtype == np.float64 and same_bytes(fit.embedding_, before)
    dist, idx = K.kneighbors(Xt, T.n_neighbors_of(30.0, 500), Q=Xq)
    np.testing.assert_allclose(Yq, transform_ref(fit.embedding_, dist, idx, 30.0), rtol=1e-12, atol=0)
    for c in range(3):
        lo, hi = fit.embedding_[lt == c].min(0), fit.embedding_[lt == c].max(0)
        assert ((Yq[lq == c] >= lo) & (Yq[lq == c] <= hi)).all()
    assert same_bytes(fit.transform(torch.as_tensor(Xq, device='cuda')), Yq)
    with pytest.raises(ValueError, match='features'):
        fit.transform(Xq[:, :8])


# ------------------------------------------------------------------------------------------------------------------------------------- stopping
def test_stopping_rules():
    X, _ = points('n257')
    fit = T.TSNE(perplexity=10.0, max_iter=250, init='random', random_state=0).fit(X)
    assert fit.n_iter_ == 250 and [it for it, _ in fit.kl_history_] == [50, 100, 150, 200, 250]
    early = T.TSNE(perplexity=10.0, max_iter=1000, init='random', random_state=0, min_grad_norm=1e10).fit(X)
    assert early.n_iter_ == 50 and [it for it, _ in early.kl_history_] == [50] and early.kl_divergence_ == fit.kl_history_[0][1]


# -------------------------------------------------------------------------------------------------------------------------------- p2 and p4
def test_p2_embed_tsne(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'ward', '--k_max', '3', '--embed', 'tsne', '--tsne_perplexity', '20', '--tsne_max_iter', '300'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_ward_aligned' / 'plot'
    xy, kl = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Tsne.FILES)
    assert list(xy.columns) == ['x', 'y'] and len(xy) == len(data['training']['hidden']) and np.isfinite(xy.to_numpy()).all()
    assert list(kl.columns) == ['iteration', 'kl'] and kl.iteration.tolist() == [50, 100, 150, 200, 250, 300] and np.isfinite(kl.kl).all()
    assert len(pd.read_csv(plot / 'ward_labels.csv')) == len(xy)          # the labels the map is there to draw, row for row
    direct = T.TSNE(perplexity=20.0, max_iter=300).fit(data['training']['hidden'])
    assert same_bytes(xy.to_numpy(), direct.embedding_) and kl.kl.tolist() == [v for _, v in direct.kl_history_]
    # a second run finds the files and does not recompute; overwrite=True does
    ts = p2.Tsne(str(plot.parent), 20.0, 300)
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Tsne.FILES]
    again = ts.train(data['training'], data['validation'])
    assert ts.fit_ is None and [(plot / name).stat().st_mtime_ns for name in p2.Tsne.FILES] == stamps and again.kl.tolist() == kl.kl.tolist()
    redo = ts.train(data['training'], data['validation'], overwrite=True)
    assert ts.fit_ is not None and redo.kl.tolist() == kl.kl.tolist()


def test_p4_embed_tsne(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'ward', '--num_clusters', '3', '--embed', 'tsne', '--tsne_perplexity', '20', '--tsne_max_iter', '300'])
    args.restore_metric = ['ae_mse']
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_ward_aligned'
    out.mkdir(parents=True)
    np.save(out / ('%s_tsne.npy' % COHORTS[2]), {'kept': True})          # an existing file is left alone
    p4.main(args)
    assert sorted(p.name for p in out.iterdir()) == sorted(['%s_tsne.npy' % c for c in COHORTS] + ['%s_3.npy' % c for c in COHORTS])
    assert np.load(out / ('%s_tsne.npy' % COHORTS[2]), allow_pickle=True).item() == {'kept': True}
    direct = T.TSNE(perplexity=20.0, max_iter=300).fit(data['training']['hidden'])
    for cohort in COHORTS[:2]:
        s = np.load(out / ('%s_tsne.npy' % cohort), allow_pickle=True).item()
        assert sorted(s) == ['encounter_id', 'hidden', 'tsne'] and s['tsne'].shape == (len(data[cohort]['hidden']), 2) and np.isfinite(s['tsne']).all()
        assert same_bytes(s['hidden'], data[cohort]['hidden']) and same_bytes(s['encounter_id'], data[cohort]['encounter_id'])
        want = direct.embedding_ if cohort == 'training' else direct.transform(data[cohort]['hidden'])
        assert same_bytes(s['tsne'], want)
    assert 'cluster_id' in np.load(out / ('%s_3.npy' % COHORTS[0]), allow_pickle=True).item()
