"""Neighbour ranks (knn.neighbor_ranks, csrc/dic_knn_rank.hip) and trustworthiness / continuity / neighbours kept (embedding_quality.py) on the GPU.

Ranks are held to the definition as INTEGERS: rank(i, j) = 1 + #{l != i : (d2(i, l), l) < (d2(i, j), j)}, d2 the f64 difference-form squared distance of
the f32 points.  The rank test data lie on a 2^-8 grid inside a small box, so every difference, square and sum of the reference is exact in f64 in any
summation order: the reference is the definition itself, not an approximation of it, and ties are real ties that only the index rule settles."""
import functools
import os
import os.path as osp

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import embedding_quality as EQ
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.tsne import TSNE, tsne_sweep
from test_gpu_optics import _write_latents
from test_tsne_host import blobs, neighbour_lists
from test_tsne_host import trustworthiness as host_trustworthiness

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------------- reference
def rank_matrix(X):
    """(N, N) int32: R[i, j] = rank(i, j) of the definition, R[i, i] = 0.  lexsort by (d2, index), the row's own index dropped."""
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    n = len(x)
    R = np.zeros((n, n), dtype=np.int32)
    ids = np.arange(n)
    for r0 in range(0, n, 128):
        rows = ids[r0:r0 + 128]
        d2 = ((x[rows, None, :] - x[None, :, :]) ** 2).sum(-1)
        order = np.lexsort((np.broadcast_to(ids, d2.shape), d2), axis=1)
        others = order[order != rows[:, None]].reshape(len(rows), n - 1)
        R[rows[:, None], others] = np.arange(1, n, dtype=np.int32)[None, :]
    return R


def grid_points(n, d, seed, shift=0.0):
    """Gaussian points rounded to the 2^-8 grid (module docstring), optionally shifted."""
    rng = np.random.default_rng(seed)
    return (np.clip(np.round(rng.normal(size=(n, d)) * 256.0) / 256.0, -8.0, 8.0) + shift).astype(np.float32)


@functools.lru_cache(maxsize=None)
def dataset(kind, n, d):
    if kind == 'random':
        X = grid_points(n, d, 100 + n + d)
    elif kind == 'lattice':          # integer coordinates in a small box: most distances tie
        X = np.random.default_rng(7).integers(0, 4, size=(n, d)).astype(np.float32)
    elif kind == 'duplicates':          # every third row is a copy of another row, with a smaller or a larger index than its twin
        X = grid_points(n, d, 11)
        rng = np.random.default_rng(12)
        dst = np.arange(0, n, 3)
        X[dst] = X[rng.integers(0, n, size=len(dst))]
        X[n - 1] = X[0]
        X[1] = X[n - 2]
    elif kind == 'shifted':          # +1000 in every coordinate: the coordinates carry 10 bits less below the point, the centre has to take the shift out
        X = grid_points(n, d, 13, shift=1000.0)
    elif kind == 'split':          # two groups 2000 apart in every coordinate: the centre lies between them, the norms (1e6 d) dwarf the distances
        X = grid_points(n, d, 14)          # inside a group, the bands (2^-12 of the norms) hold every pair of a group: nearly everything goes to the exact stage
        X[::2] += 1000.0
        X[1::2] -= 1000.0
    else:
        raise AssertionError(kind)
    R = rank_matrix(X)
    R.setflags(write=False)
    return X, R


def make_targets(R, m, seed):
    """(N, m) targets by kind, (i + q) % 5: the nearest, the farthest, a random point, absent (-1), the row itself."""
    n = len(R)
    rng = np.random.default_rng(seed)
    order = np.argsort(R, axis=1, kind='stable')          # column 0 = the row itself (rank 0), then ranks 1 .. n - 1
    i, q = np.meshgrid(np.arange(n), np.arange(m), indexing='ij')
    kind = (i + q) % 5
    t = rng.integers(0, n, size=(n, m))
    t = np.where(kind == 0, order[:, 1][:, None], t)
    t = np.where(kind == 1, order[:, n - 1][:, None], t)
    t = np.where(kind == 3, -1, t)
    t = np.where(kind == 4, i, t)
    return t.astype(np.int32)


def expected(R, targets):
    n = len(R)
    rows = np.arange(n)[:, None]
    return np.where((targets >= 0) & (targets != rows), R[rows, np.maximum(targets, 0)], 0).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize('m', [1, 8, 9, 40])
@pytest.mark.parametrize('d', [2, 3, 16, 256])
@pytest.mark.parametrize('n', [257, 600, 1000])
def test_ranks_equal_the_definition(n, d, m):
    X, R = dataset('random', n, d)
    targets = make_targets(R, m, n + d + m)
    st = {}
    got = knn.neighbor_ranks(X, targets, stats=st)
    assert got.dtype == np.int32 and got.shape == targets.shape
    assert st['passes'] == (m + 7) // 8
    assert np.array_equal(got, expected(R, targets))


@pytest.mark.parametrize('kind,n,d,m', [('lattice', 600, 3, 9), ('lattice', 1000, 2, 40), ('duplicates', 600, 16, 9), ('duplicates', 257, 3, 8),
                                        ('shifted', 600, 16, 9), ('shifted', 1000, 256, 8), ('split', 600, 16, 9), ('split', 1000, 3, 40)])
def test_ranks_on_ties_duplicates_and_wide_bands(kind, n, d, m):
    X, R = dataset(kind, n, d)
    targets = make_targets(R, m, 5)
    if kind == 'duplicates':          # the twin of a duplicated row as a target, from either side
        targets[n - 1, 0], targets[0, 0], targets[1, 0], targets[n - 2, 0] = 0, n - 1, n - 2, 1
    st = {}
    got = knn.neighbor_ranks(X, targets, stats=st)
    assert np.array_equal(got, expected(R, targets))
    if kind == 'split':          # the bands are wide: a target's band holds its whole group
        assert st['max_list'] > n


def test_all_points_equal():
    """Every distance 0, every norm 0 after centring: the index rule alone ranks, rank(i, j) = j + 1 - [j > i]."""
    n = 300
    X = np.full((n, 4), 3.0, dtype=np.float32)
    targets = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 150) % n], axis=1).astype(np.int32)
    want = targets + 1 - (targets > np.arange(n)[:, None])
    assert np.array_equal(knn.neighbor_ranks(X, targets), want)


def test_budget_changes_grouping_not_result():
    X, R = dataset('split', 600, 16)
    targets = make_targets(R, 9, 5)
    st = {}
    want = knn.neighbor_ranks(X, targets, stats=st)
    assert st['groups'] == 1
    small = {}
    got = knn.neighbor_ranks(X, targets, candidate_budget=st['budget_needed'] * 4, stats=small)
    assert small['groups'] > 10 and small['candidates'] == st['candidates']
    assert np.array_equal(got, want) and np.array_equal(got, expected(R, targets))
    with pytest.raises(knn.CandidateBudgetError) as err:
        knn.neighbor_ranks(X, targets, candidate_budget=st['budget_needed'] // 2)
    assert err.value.needed == st['budget_needed']
    assert np.array_equal(knn.neighbor_ranks(X, targets, candidate_budget=err.value.needed), want)


def test_ranks_of_the_packages_own_lists_and_determinism():
    X, _ = dataset('duplicates', 600, 16)
    k = 12
    idx = knn.kneighbors(X, k + 1)[1]
    lists = EQ.drop_own(torch.as_tensor(idx)).numpy()
    a = knn.neighbor_ranks(X, lists)
    b = knn.neighbor_ranks(torch.as_tensor(X).cuda(), torch.as_tensor(lists).cuda(), return_device=True)
    assert np.array_equal(a, np.broadcast_to(np.arange(1, k + 1, dtype=np.int32), a.shape))
    assert b.is_cuda and np.array_equal(a, b.cpu().numpy())


def test_argument_errors():
    X = np.zeros((10, 4), dtype=np.float32)
    with pytest.raises(ValueError, match='targets must be 2-D'):
        knn.neighbor_ranks(X, np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError, match='inconsistent numbers of samples'):
        knn.neighbor_ranks(X, np.zeros((9, 2), dtype=np.int32))
    with pytest.raises(ValueError, match='must be below n_samples'):
        knn.neighbor_ranks(X, np.full((10, 2), 10, dtype=np.int32))
    with pytest.raises(ValueError, match='must be integers'):
        knn.neighbor_ranks(X, np.zeros((10, 2)))
    with pytest.raises(NotImplementedError, match='at most 1023 targets'):
        knn.neighbor_ranks(X, np.zeros((10, 1024), dtype=np.int32))
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        knn.neighbor_ranks(np.zeros((10, 260), dtype=np.float32), np.zeros((10, 2), dtype=np.int32))
    with pytest.raises(ValueError, match='candidate_budget must be positive'):
        knn.neighbor_ranks(X, np.zeros((10, 2), dtype=np.int32), candidate_budget=0)


# ------------------------------------------------------------------------------------------------------------ trustworthiness, continuity, kept
KS = (5, 10, 30)


@functools.lru_cache(maxsize=None)
def blob_points():
    return blobs()[0]


@functools.lru_cache(maxsize=None)
def short_fit():
    return TSNE(perplexity=30.0, max_iter=250, init='random', random_state=0).fit(blob_points())


def a_map(name):
    X = blob_points()
    if name == 'slice':
        return X[:, :2].astype(np.float64)
    if name == 'random':
        return np.random.default_rng(4).normal(size=(len(X), 2)) * 50.0
    return short_fit().embedding_


def host_quality(X, Y, k):
    """(T, C, kept) of the definition, dense numpy, on the map rounded to f32."""
    y32 = np.asarray(Y).astype(np.float32)
    ix, iy = neighbour_lists(X, k)[1], neighbour_lists(y32, k)[1]
    kept = np.mean([len(set(a) & set(b)) for a, b in zip(ix, iy)]) / k
    return host_trustworthiness(X, y32, k), host_trustworthiness(y32, X, k), kept


@pytest.mark.parametrize('name', ['slice', 'random', 'tsne'])
def test_quality_against_the_host_definition(name):
    X, Y = blob_points(), a_map(name)
    got = EQ.embedding_quality(X, Y, KS)
    assert sorted(got) == list(KS)
    for k in KS:
        want = host_quality(X, Y, k)
        print('%s k=%d: T %.17g C %.17g kept %.17g (host %.17g %.17g %.17g)' % ((name, k) + got[k] + want))
        assert all(abs(g - w) <= 1e-12 for g, w in zip(got[k], want))
        # every k of the sweep has the bits of its stand-alone call
        assert got[k] == (EQ.trustworthiness(X, Y, k), EQ.continuity(X, Y, k), EQ.neighbors_kept(X, Y, k))
    assert EQ.embedding_quality(torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda(), KS) == got          # two calls, and device tensors: identical bits
    if name == 'slice':
        assert got[5][0] > got[5][2] and got[5][0] > EQ.trustworthiness(X, a_map('random'), 5)          # (a projection beats noise)


def test_tsne_quality_is_embedding_quality():
    X, fit = blob_points(), short_fit()
    want = EQ.embedding_quality(X, fit.embedding_, KS)
    assert fit.quality(KS) == want
    assert fit.quality() == {5: want[5]} and fit.quality((95, 5))[5] == want[5]          # (95 + 1 is wider than the fit's own lists: a join of its own)
    with pytest.raises(ValueError, match=r'n_neighbors \(300\) should be less than n_samples / 2 \(300.0\)'):
        fit.quality((300,))
    with pytest.raises(RuntimeError, match='not fitted'):
        TSNE().quality()


def test_sweep_fits_answer_quality_from_the_shared_join(monkeypatch):
    X = blob_points()
    fits = tsne_sweep(X, [10.0, 30.0], max_iter=250, init='random', random_state=0)
    calls = []
    real = EQ.kneighbors
    monkeypatch.setattr(EQ, 'kneighbors', lambda Z, k, **kw: calls.append(tuple(Z.shape)) or real(Z, k, **kw))
    got = {u: fits[u].quality(KS) for u in fits}
    assert calls == [(600, 2), (600, 2)]          # the map's join only: the input-space side comes from the sweep's one join, for either perplexity
    monkeypatch.undo()
    for u in fits:
        assert got[u] == EQ.embedding_quality(X, fits[u].embedding_, KS)


# -------------------------------------------------------------------------------------------------------------------------------- p2 and p4
def read_quality(path):
    import pandas as pd
    df = pd.read_csv(path, float_precision='round_trip')
    assert list(df.columns) == ['k', 'trustworthiness', 'continuity', 'neighbors_kept']
    return {int(r.k): (float(r.trustworthiness), float(r.continuity), float(r.neighbors_kept)) for r in df.itertuples()}


def test_p2_embed_quality(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    base = ['--cluster_method', 'ward', '--k_max', '3', '--embed', 'tsne', '--tsne_perplexity', '20', '--tsne_max_iter', '250']
    assert p2.get_arguments(base).embed_quality_k is None
    args = p2.get_arguments(base + ['--embed_quality_k', '5', '10', '30'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_ward_aligned' / 'plot'
    xy = pd.read_csv(plot / 'tsne.csv', float_precision='round_trip').to_numpy()
    got = read_quality(plot / p2.Tsne.QUALITY_FILE)
    assert got == EQ.embedding_quality(data['training']['hidden'], xy, KS)
    # without the flag the table is neither written nor looked for
    other = tmp_path / 'other'
    p2.Tsne(str(other), 20.0, 250).train(data['training'], data['validation'])
    assert sorted(p.name for p in (other / 'plot').iterdir()) == sorted(p2.Tsne.FILES)


def test_p4_embed_quality(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    base = ['--cluster_method', 'ward', '--num_clusters', '3', '--embed', 'tsne', '--tsne_perplexity', '20', '--tsne_max_iter', '250']
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_ward_aligned'
    args = p4.get_arguments(base)
    assert args.embed_quality_k is None
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert not any('quality' in p.name for p in out.iterdir())          # without the flag: no table
    args = p4.get_arguments(base + ['--embed_quality_k', '5', '10', '30'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert sorted(p.name for p in out.iterdir() if 'quality' in p.name) == ['training_tsne_quality.csv']          # the training cohort only
    tsne = np.load(out / 'training_tsne.npy', allow_pickle=True).item()['tsne']
    assert read_quality(out / 'training_tsne_quality.csv') == EQ.embedding_quality(data['training']['hidden'], tsne, KS)
