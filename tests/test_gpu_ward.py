"""Ward linkage on the GPU (csrc/dic_ward.hip, ward.py, the p2 / p4 ward branches) against the numpy yardstick of tests/test_ward_host.py and scipy.

The cases are the smallest shapes at which the step kernel can still go wrong (tests/test_ward_host.py: CASES): one and two merges, two workgroups and the
ticket (17 rows), full-width rows (64 and 256 features), several trips of the unrolled row loop with a ragged tail (1030), the full grid of 256 workgroups
(4100), exact zero heights (dup, same) and a strided input.  test_ward_host.py shows on the CPU that every decision of every case is an exact tie at 0 or
separated by more than 1e-10 relative, so the merges must be EQUAL to the yardstick's, in the same order."""
import functools

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import cluster_stats
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.ward import Ward, ward_linkage, ward_records
from test_gpu_optics import _write_latents
from test_ward_host import BLOB_CASES, CASES, points, same_partition, scipy_linkage, yardstick

pytestmark = pytest.mark.gpu

KS = range(2, 8)


def device_points(case):
    """The case's points on the device; 'strided' as a view with a row stride of 16 floats into a buffer whose other columns hold NaN."""
    X = torch.as_tensor(np.array(points(case)), device='cuda')
    if case != 'strided':
        return X
    buf = torch.full((X.shape[0], 16), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, :8] = X
    view = buf[:, :8]
    assert view.stride(0) == 16 and not view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def device_run(case):
    """(records, stats, Z) of one run on the device tensor, shared by the tests of a case."""
    stats = {}
    x = device_points(case)
    keep = x.clone()
    rec = ward_records(x, stats)
    assert torch.equal(x, keep)          # the input is only read
    return rec, stats, ward_linkage(x)


def partition_after(Z, k):
    n = len(Z) + 1
    members = {i: [i] for i in range(n)}
    for i in range(n - k):
        members[n + i] = members.pop(int(Z[i, 0])) + members.pop(int(Z[i, 1]))
    lab = np.empty(n, dtype=np.int64)
    for c, m in enumerate(members.values()):
        lab[m] = c
    return lab


@pytest.mark.parametrize('case', list(CASES))
def test_records_equal_the_yardstick(case):
    ref, _, gaps = yardstick(case)
    rec, stats, _ = device_run(case)
    n = len(ref) + 1
    assert rec.shape == (n - 1, 4) and rec.dtype == np.float64
    np.testing.assert_array_equal(rec[:, [0, 1, 3]], ref[:, [0, 1, 3]])          # the same merges, in the same order
    zero = ref[:, 2] == 0
    assert np.all(rec[zero, 2] == 0)
    rel = np.abs(rec[~zero, 2] - ref[~zero, 2]) / ref[~zero, 2]
    print(case, 'heights: largest relative deviation', rel.max() if rel.size else 0.0, 'steps', stats['steps'], 'of', 3 * (n - 1))
    assert np.all(rel <= 1e-13)
    assert stats['merges'] == n - 1 and stats['steps'] <= 3 * (n - 1)
    assert stats['steps'] == len(gaps)          # a launch is one repeat of the chain's inner loop
    if case == 'dup':
        assert zero.sum() == 40
    if case == 'same':
        assert zero.all()


@pytest.mark.parametrize('case', list(CASES))
def test_linkage_equals_the_yardstick_and_scipy(case):
    _, Zy, _ = yardstick(case)
    _, _, Z = device_run(case)
    assert np.array_equal(Z[:, [0, 1, 3]], Zy[:, [0, 1, 3]])
    ref = scipy_linkage(case)
    assert np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]])
    zero = ref[:, 2] == 0
    assert np.all(Z[zero, 2] == 0)
    np.testing.assert_allclose(Z[~zero, 2], ref[~zero, 2], rtol=1e-12, atol=0)
    assert np.all(np.diff(Z[:, 2]) >= 0)


@pytest.mark.parametrize('case', list(CASES))
def test_two_calls_and_a_host_array_give_identical_bits(case):
    rec, _, _ = device_run(case)
    again = ward_records(device_points(case))
    assert rec.tobytes() == again.tobytes()
    if case in ('n17', 'n255', 'strided'):          # the numpy array of the same points: the contiguous, padded copy
        assert rec.tobytes() == ward_records(np.array(points(case))).tobytes()


def test_features_are_padded_to_a_multiple_of_four():
    X = np.array(points('n255'))[:, :13]          # 13 features: three zero columns are added
    Z = ward_linkage(X)
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    ref = hier.linkage(X.astype(np.float64), 'ward')
    assert np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]])
    np.testing.assert_allclose(Z[:, 2], ref[:, 2], rtol=1e-12, atol=0)


@pytest.mark.parametrize('case', list(CASES))
def test_fit_cuts_centres_and_predict(case):
    """``same`` has no fcluster counterpart (with every height 0, fcluster's 'maxclust' threshold gives one cluster for every K): its labels are held to the
    partition after N - K merges of the yardstick's Z instead, as are those of every other case besides fcluster."""
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    X = np.array(points(case))
    n = len(X)
    ks = [k for k in KS if k <= n]
    fit = Ward(ks=ks).fit(device_points(case))
    _, Zy, _ = yardstick(case)
    assert fit.n_clusters == ks[-1] and sorted(fit.labels_by_k_) == ks
    assert np.array_equal(fit.linkage_[:, [0, 1, 3]], Zy[:, [0, 1, 3]])
    for k in ks:
        lab = fit.labels_by_k_[k]
        assert lab.shape == (n,) and sorted(set(lab.tolist())) == list(range(k))
        assert same_partition(lab, partition_after(Zy, k))
        if case != 'same':
            assert same_partition(lab, hier.fcluster(scipy_linkage(case), k, 'maxclust'))
        assert fit.heights_by_k_[k] == fit.linkage_[n - k, 2]
        means = np.stack([X[lab == c].astype(np.float64).mean(0) for c in range(k)])
        got = fit.cluster_centers_by_k_[k]
        assert got.dtype == np.float32 and got.shape == means.shape
        np.testing.assert_allclose(got, means, rtol=1e-6, atol=1e-6)
    assert np.array_equal(fit.labels_, fit.labels_by_k_[ks[-1]]) and np.array_equal(fit.cluster_centers_, fit.cluster_centers_by_k_[ks[-1]])
    if len(ks) < 2:
        return
    # predict: the nearest centre, wherever the f64 argmin is decided by more than 1e-5 relative
    pred = fit.predict(X)
    centres = fit.cluster_centers_.astype(np.float64)
    d = np.sqrt(((X.astype(np.float64)[:, None, :] - centres[None, :, :]) ** 2).sum(-1))
    order = np.sort(d, axis=1)
    decided = (order[:, 1] - order[:, 0]) > 1e-5 * order[:, 1]
    print(case, 'predict: decided', decided.mean())
    assert np.array_equal(pred[decided], np.argmin(d, axis=1)[decided])
    if case in BLOB_CASES and n >= 17:
        assert decided.mean() >= 0.99


def test_a_workspace_that_does_not_fit_raises_memory_error(monkeypatch):
    X = np.array(points('n255'))
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (100000, 1 << 30))
    need = 2 * 8 * 255 * 64          # S and C alone
    with pytest.raises(MemoryError, match=r'255 points needs (\d+) bytes on the device, 100000 are free') as err:
        ward_linkage(X)
    assert int(str(err.value).split('needs ')[1].split(' bytes')[0]) >= need


def _run_p2(tmp_path, monkeypatch, p2):
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'ward', '--k_max', '5'])
    args.restore_metric = ['ae_mse']
    return data, p2.main(args)


def test_p2_ward_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data, res = _run_p2(tmp_path, monkeypatch, p2)
    X, V = data['training']['hidden'], data['validation']['hidden']
    n = len(X)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_ward_aligned' / 'plot'
    link, table, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Ward.FILES)          # (%.17g: exact)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(link.columns) == ['left', 'right', 'height', 'size'] and len(link) == n - 1
    assert list(table.columns) == ['k', 'height', 'train_distortion', 'valid_distortion'] + metrics and table.k.tolist() == [2, 3, 4, 5]
    assert list(labels.columns) == ['k2', 'k3', 'k4', 'k5'] and len(labels) == n
    fit = Ward(ks=range(2, 6)).fit(X)
    assert np.array_equal(link.to_numpy(), fit.linkage_)
    for row, k in enumerate(range(2, 6)):
        lab = labels['k%d' % k].to_numpy()
        np.testing.assert_array_equal(lab, fit.labels_by_k_[k])
        assert table.height[row] == fit.linkage_[n - k, 2]
        direct = [cluster_stats.silhouette_score(X, lab), cluster_stats.davies_bouldin_score(X, lab), cluster_stats.calinski_harabasz_score(X, lab)]
        np.testing.assert_allclose(table[metrics].to_numpy()[row], direct, rtol=1e-12, atol=0)
        centres = np.stack([X[lab == c].astype(np.float64).mean(0) for c in range(k)])
        for col, Y in (('train_distortion', X), ('valid_distortion', V)):
            dist = np.sqrt(((Y.astype(np.float64)[:, None, :] - centres[None]) ** 2).sum(-1)).min(1).mean()
            np.testing.assert_allclose(table[col][row], dist, rtol=1e-5)
    assert np.all(np.diff(table.height.to_numpy()) <= 0)          # Ward's heights are monotone
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy())
    # a second run finds the files and does not recompute; overwrite=True does
    wd = p2.Ward(5, str(plot.parent), metrics)
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Ward.FILES]
    calls = []
    real = p2.WardLinkage
    monkeypatch.setattr(p2, 'WardLinkage', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = wd.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Ward.FILES] == stamps
    assert np.array_equal(again.to_numpy(), table.to_numpy()) and wd.fit_ is None
    redo = wd.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and np.array_equal(redo.to_numpy(), table.to_numpy())
    assert np.array_equal(wd.fit_.linkage_, fit.linkage_)
    # --metric_sample: the indices on a subsample, the rest unchanged
    sub = p2.Ward(5, str(plot.parent), metrics, metric_sample=100).train(data['training'], data['validation'], overwrite=True)
    pick = np.random.RandomState(0).choice(n, 100, replace=False)
    lab3 = fit.labels_by_k_[3]
    np.testing.assert_allclose(sub['Sihouette'][1], cluster_stats.silhouette_score(X[pick], lab3[pick]), rtol=1e-12, atol=0)
    assert np.array_equal(sub[['k', 'height', 'train_distortion', 'valid_distortion']].to_numpy(),
                          table[['k', 'height', 'train_distortion', 'valid_distortion']].to_numpy())


def test_p4_ward_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'ward', '--num_clusters', '3'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_ward_aligned'
    saved = {cohort: np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    for cohort in COHORTS:
        assert sorted(saved[cohort]) == ['cluster_id', 'encounter_id', 'hidden'] and len(saved[cohort]['cluster_id']) == len(data[cohort]['hidden'])
        assert sorted(set(np.asarray(saved[cohort]['cluster_id']).tolist())) == [0, 1, 2]
    # training: a renaming of the tree's cut, in the order of descending systolic pressure
    X = data['training']['hidden']
    ids = np.asarray(saved['training']['cluster_id'])
    raw = Ward(n_clusters=3).fit(X).labels_
    assert same_partition(ids, raw)
    sbp = data['training']['ob'][:, 0, :].mean(1)
    means = [sbp[ids == i].mean() for i in range(3)]
    assert means[0] > means[1] > means[2]
    # validation and test: the nearest aligned training centre
    centres = np.stack([X[ids == i].astype(np.float64).mean(0) for i in range(3)])
    for cohort in COHORTS[1:]:
        h = data[cohort]['hidden'].astype(np.float64)
        d = np.sqrt(((h[:, None, :] - centres[None]) ** 2).sum(-1))
        order = np.sort(d, axis=1)
        decided = (order[:, 1] - order[:, 0]) > 1e-5 * order[:, 1]
        got = np.asarray(saved[cohort]['cluster_id'])
        assert decided.mean() >= 0.99 and np.array_equal(got[decided], np.argmin(d, axis=1)[decided])
    # an existing result is left alone
    stamps = [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
