"""The local outlier factor on the GPU (csrc/dic_lof.hip, lof.py) against the numpy definition of test_lof_host.py.

Two bars.  ``lof_from_lists`` on the GPU's own lists: a relative 8 (k + 2) 2^-53 per value -- every sum is over positive terms, so any order is within
(k - 1) 2^-53 of exact, lrd enters twice, and 8 (k + 2) covers both sides' orders with a factor of two to spare.  End to end (the join included) against
numpy's own lists: 1e-12 relative; the derived bound (3 k + D + 10) 2^-53 is below 6e-14 for k <= 64 and D <= 256."""
import functools

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd import lof as LOF
from test_gpu_optics import _write_latents
from test_lof_host import N_PLANTED, SHAPES, cluster_sets, duplicates_set, lists, lof_fit, lof_score

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
END_TO_END = 1e-12


def points(n, d, seed):
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(3, d))[rng.integers(0, 3, n)] * 4 + rng.normal(size=(n, d))).astype(np.float32)
    X[:min(3, n // 8)] += 15
    return X


def close(got, ref, bar, what):
    got, ref = np.asarray(got), np.asarray(ref)
    err = float((np.abs(got - ref) / np.abs(ref)).max())
    print('%s: largest relative difference %.3e, bar %.3e' % (what, err, bar))
    assert got.shape == ref.shape and np.isfinite(got).all() and err <= bar, what


def gpu_lists(X, k, Q=None):
    """The package's own lists on the device: the self join at k + 1 without the self column, or the query join at k."""
    if Q is None:
        return LOF.drop_self(*knn.kneighbors(X, k + 1, return_device=True))
    return knn.kneighbors(X, k, Q=Q, return_device=True)


def check_from_lists(X, ks, width=None):
    """lof_from_lists on the device's lists of ``X`` (``width`` columns, default max(ks)) against the numpy definition on the same lists."""
    dist, idx = gpu_lists(X, max(ks) if width is None else width)
    nof, lrd, kdist = LOF.lof_from_lists(dist, idx, ks)
    assert nof.shape == lrd.shape == kdist.shape == (len(X), len(ks)) and nof.dtype == torch.float64
    ref = lof_fit(dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64), ks)
    for t, k in enumerate(ks):
        what = 'N=%d D=%d k=%d of %s' % (X.shape[0], X.shape[1], k, list(ks))
        assert np.array_equal(kdist[:, t].cpu().numpy(), ref[k][2])
        close(lrd[:, t].cpu().numpy(), ref[k][1], 8 * (k + 2) * EPS, 'lrd ' + what)
        close(nof[:, t].cpu().numpy(), ref[k][0], 8 * (k + 2) * EPS, 'nof ' + what)
    return nof, lrd, kdist


@pytest.mark.parametrize('n,d,ks', [(2, 4, [1]), (65, 8, [1]), (65, 8, [7]), (65, 8, [64]), (300, 8, [1, 5, 20, 35]), (130, 12, list(range(1, 65)))],
                         ids=['N2-k1', 'N65-k1', 'N65-k7', 'N65-k64', 'N300-sweep', 'N130-nk64'])
def test_from_lists_against_the_definition(n, d, ks):
    check_from_lists(cluster_sets()[(300, 8)][0] if (n, d) == (300, 8) else points(n, d, 100 + n), ks)


def test_from_lists_wider_than_the_largest_k():
    X = points(130, 12, 7)
    wide = check_from_lists(X, [5, 20], width=40)          # the row stride (40) is not the width read (20)
    narrow = check_from_lists(X, [5, 20])
    assert all(torch.equal(a, b) for a, b in zip(wide, narrow))


@pytest.mark.parametrize('m', [1, 67])
def test_from_lists_novelty_against_the_definition(m):
    X, ks = points(130, 12, 7), [1, 5, 20, 35]
    Q = (X[:m] + np.random.default_rng(m).normal(size=(m, 12)) * 1.5).astype(np.float32)
    _, lrd, kdist = LOF.lof_from_lists(*gpu_lists(X, max(ks)), ks)
    dist_q, idx_q = gpu_lists(X, max(ks), Q)
    nof_q, lrd_q, kdist_q = LOF.lof_from_lists(dist_q, idx_q, ks, fit=(lrd, kdist))
    assert nof_q.shape == lrd_q.shape == kdist_q.shape == (m, len(ks))
    for t, k in enumerate(ks):
        ref = lof_score(dist_q.cpu().numpy(), idx_q.cpu().numpy().astype(np.int64), lrd[:, t].cpu().numpy(), kdist[:, t].cpu().numpy(), k)
        close(nof_q[:, t].cpu().numpy(), ref, 8 * (k + 2) * EPS, 'novelty M=%d k=%d' % (m, k))
        assert np.array_equal(kdist_q[:, t].cpu().numpy(), dist_q[:, k - 1].cpu().numpy())


def test_bit_equality():
    X = cluster_sets()[(300, 8)][0]
    sweep = LOF.lof_sweep(X, [5, 20, 35])
    assert sweep.shape == (3, 300) and sweep.dtype == np.float64
    assert np.array_equal(sweep, LOF.lof_sweep(X, [5, 20, 35]))          # two calls: the same bits
    assert np.array_equal(sweep[1], LOF.lof_sweep(X, [20])[0])          # a column of a sweep: the bits of its own call
    assert np.array_equal(sweep[::-1], LOF.lof_sweep(X, [35, 20, 5]))          # the rows follow the caller's order
    dev = LOF.lof_sweep(X, [20], return_device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy()[0], sweep[1])
    assert np.array_equal(LOF.LocalOutlierFactor(n_neighbors=20).fit(X).negative_outlier_factor_, sweep[1])


@functools.lru_cache(maxsize=None)
def end_to_end_sets():
    shifted = (cluster_sets()[(300, 8)][0] + np.float32(1000.0)).astype(np.float32)
    return {'500x256': (cluster_sets()[(500, 256)][0], 20), 'shifted': (shifted, 20), 'duplicates': (duplicates_set(), 5)}


@pytest.mark.parametrize('name', ['500x256', 'shifted', 'duplicates'])
def test_end_to_end_against_the_definition(name, recwarn):
    X, k = end_to_end_sets()[name]
    ref = lof_fit(*lists(X, k=k), [k])[k][0]
    if name == 'duplicates':
        assert ref.min() < -1e9          # the 1e-10 guard's scale, held to the same relative bar
    fit = LOF.LocalOutlierFactor(n_neighbors=k).fit(X)
    close(fit.negative_outlier_factor_, ref, END_TO_END, 'LocalOutlierFactor ' + name)
    close(LOF.lof_sweep(torch.as_tensor(X), [k])[0], ref, END_TO_END, 'lof_sweep ' + name)
    assert any('Duplicate values are leading to incorrect results' in str(w.message) for w in recwarn) == (name == 'duplicates')


def test_end_to_end_novelty_against_the_definition():
    X, Q = cluster_sets()[(500, 256)]
    k = 20
    _, lrd, kd = lof_fit(*lists(X, k=k), [k])[k]
    est = LOF.LocalOutlierFactor(n_neighbors=k, novelty=True).fit(X)
    scores = est.score_samples(Q)
    close(scores, lof_score(*lists(X, Q, k=k), lrd, kd, k), END_TO_END, 'score_samples 500x256')
    assert np.array_equal(est.decision_function(Q), scores - est.offset_) and est.offset_ == -1.5
    assert np.array_equal(est.predict(Q), np.where(scores - est.offset_ < 0, -1, 1))
    with pytest.raises(ValueError, match='X has 8 features, but LocalOutlierFactor is expecting 256 features as input'):
        est.score_samples(np.zeros((3, 8), np.float32))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_labels_and_offset_equal_sklearns(shape):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = cluster_sets()[shape][0]
    sk = neighbors.LocalOutlierFactor(n_neighbors=20, algorithm='brute', contamination=0.05)
    theirs = sk.fit_predict(X.astype(np.float64))
    assert np.abs(sk.negative_outlier_factor_ - sk.offset_).min() > 1e-9          # the condition of the reference: no label hangs on the last bits
    est = LOF.LocalOutlierFactor(n_neighbors=20, contamination=0.05)
    ours = est.fit_predict(X)
    assert np.array_equal(ours, theirs) and (ours[:N_PLANTED] == -1).all()
    assert abs(est.offset_ - sk.offset_) <= END_TO_END * abs(sk.offset_)


def test_the_limit():
    X = points(1100, 4, 3)
    ref = lof_fit(*lists(X, k=1023), [1023])[1023][0]
    close(LOF.lof_sweep(X, [1023])[0], ref, END_TO_END, 'N=1100 k=1023')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='at most 1023 neighbours'):
        LOF.lof_sweep(X, [1024])
    assert torch.cuda.memory_allocated() == before          # refused before any GPU work


@pytest.mark.parametrize('bad', ['n', 'negative', 'float'])
def test_refusal_before_launch(bad):
    X = points(130, 12, 7)
    dist, idx = gpu_lists(X, 10)
    out = torch.full((130, 2), 7.25, dtype=torch.float64, device=dist.device)
    if bad == 'float':
        idx = idx.double()
    else:
        idx = idx.clone()
        idx[77, 3] = 130 if bad == 'n' else -1
    with pytest.raises(ValueError, match='idx must be integers' if bad == 'float' else r'idx must lie in \[0, n_samples_fit = 130\)'):
        LOF.lof_from_lists(dist, idx, [5, 10], out=out)
    assert bool((out == 7.25).all())
    if bad == 'n':          # the same index is fine against a larger fitted set: the bound is the fit's, not the rows'
        lrd = torch.ones((131, 2), dtype=torch.float64, device=dist.device)
        nof = LOF.lof_from_lists(dist, idx, [5, 10], fit=(lrd, lrd.clone()), out=out)[0]
        assert nof.data_ptr() == out.data_ptr() and bool((out != 7.25).all())
        with pytest.raises(ValueError, match='inconsistent numbers of samples'):
            LOF.lof_from_lists(dist, idx, [5, 10], n_fit=131)


def test_p2_outlier_lof(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    X = data['training']['hidden']
    monkeypatch.chdir(tmp_path)
    base = ['--cluster_method', 'kmeans', '--k_max', '4', '--n_init', '2', '--gap_b', '2']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_kmeans_aligned' / 'plot'
    args = p2.get_arguments(base)
    args.restore_metric = ['ae_mse']
    p2.main(args)
    assert not any('lof' in p.name for p in plot.parent.rglob('*'))          # without the flag: neither file
    args = p2.get_arguments(base + ['--outlier', 'lof', '--outlier_k', '5', '20'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    assert sorted(p.name for p in plot.iterdir() if 'lof' in p.name) == sorted(p2.Lof.FILES)
    df = pd.read_csv(plot / 'lof.csv', float_precision='round_trip')
    assert list(df.columns) == ['lof_k5', 'outlier_k5', 'lof_k20', 'outlier_k20', 'lof_max'] and len(df) == len(X)
    nof = LOF.lof_sweep(X, [5, 20])
    for t, k in enumerate((5, 20)):
        assert np.array_equal(df['lof_k%d' % k].to_numpy(), -nof[t])
        assert np.array_equal(df['outlier_k%d' % k].to_numpy(), (nof[t] < -1.5).astype(np.int64))
    assert np.array_equal(df['lof_max'].to_numpy(), (-nof).max(axis=0))
    summary = pd.read_csv(plot / 'lof_summary.csv', float_precision='round_trip')
    assert list(summary.columns) == ['k', 'offset', 'n_outliers', 'max_lof'] and summary['k'].tolist() == [5, 20]
    assert summary['offset'].tolist() == [-1.5, -1.5] and summary['n_outliers'].tolist() == [int((nof[t] < -1.5).sum()) for t in range(2)]
    assert summary['max_lof'].tolist() == [float((-nof[t]).max()) for t in range(2)] and min(summary['n_outliers']) > 0


def test_p4_outlier_lof(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    base = ['--cluster_method', 'ward', '--num_clusters', '3']
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_ward_aligned'
    args = p4.get_arguments(base)
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert not any('lof' in p.name for p in out.iterdir())          # without the flag: no file
    args = p4.get_arguments(base + ['--outlier', 'lof', '--outlier_k', '20', '5', '--outlier_contamination', '0.1'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert sorted(p.name for p in out.iterdir() if 'lof' in p.name) == ['testing_lof.npy', 'training_lof.npy', 'validation_lof.npy']
    X = data['training']['hidden']
    fits = {k: LOF.LocalOutlierFactor(n_neighbors=k, contamination=0.1, novelty=True).fit(X) for k in (5, 20)}
    for cohort in ('training', 'validation', 'testing'):
        got = np.load(out / ('%s_lof.npy' % cohort), allow_pickle=True).item()
        assert sorted(got) == ['encounter_id', 'ks', 'lof', 'outlier'] and got['ks'].tolist() == [5, 20]
        assert np.array_equal(got['encounter_id'], data[cohort]['encounter_id'])
        assert got['lof'].dtype == np.float64 and got['outlier'].dtype == np.bool_ and got['lof'].shape == got['outlier'].shape == (len(got['encounter_id']), 2)
        for t, k in enumerate((5, 20)):
            nof = fits[k].negative_outlier_factor_ if cohort == 'training' else fits[k].score_samples(data[cohort]['hidden'])
            assert np.array_equal(got['lof'][:, t], -nof)
            assert np.array_equal(got['outlier'][:, t], nof < fits[k].offset_)          # the TRAINING fit's offset, for every cohort
    train = np.load(out / 'training_lof.npy', allow_pickle=True).item()
    assert abs(train['outlier'].mean(axis=0) - 0.1).max() <= 1.0 / 400
