"""Shared-nearest-neighbour clustering on the GPU (csrc/dic_snn.hip, snn.py, the p2 / p4 snn branches) against the numpy yardstick of tests/test_snn_host.py.

The cases are the smallest shapes at which the kernels can still go wrong (tests/test_snn_host.py: CASES, and the conditions it holds them to): one row pair,
k = N, less than a wave and more than one workgroup, full-width rows, k exactly one wave, the workload's k = 257 (four waves and one lane, a padded sort), the
largest k (the full LDS sort), and components 200 hops long.  Every result is an integer: all comparisons are for equality."""
import ctypes

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn as K
from deep_interpolation_clustering_amd import snn as S
from deep_interpolation_clustering_amd.info import COHORTS
from test_gpu_optics import _write_latents
from test_snn_host import CASES, points, snn_labels_exact, yard

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def assert_fit(got, name, eps=None, min_samples=None):
    labels, core, density = got
    _, _, y_labels, y_core, y_density, _ = yard(name, eps, min_samples)
    assert labels.dtype == np.int64 and core.dtype == np.int64 and density.dtype == np.int32
    np.testing.assert_array_equal(density, y_density)
    np.testing.assert_array_equal(core, y_core)
    np.testing.assert_array_equal(labels, y_labels)


@pytest.mark.parametrize('name', list(CASES))
def test_kernels_alone_on_the_yardstick_lists(name):
    eps, ms = CASES[name][3:5]
    idx, sim = yard(name)[:2]
    got = S.snn_similarity(idx)
    assert got.is_cuda and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), sim)
    assert_fit(S.snn_labels(idx, sim, eps, ms), name)                                   # numpy (idx, sim)
    assert_fit(S.snn_labels(torch.as_tensor(idx.copy(), device=DEV), got, eps, ms), name)      # device tensors


@pytest.mark.parametrize('name', list(CASES))
def test_end_to_end_equals_the_yardstick(name):
    k, eps, ms = CASES[name][2:5]
    X = points(name)
    y_idx, y_sim = yard(name)[:2]
    idx, sim = S.snn_graph(X, k)
    assert idx.dtype == sim.dtype == np.int32
    np.testing.assert_array_equal(idx, y_idx)
    np.testing.assert_array_equal(sim, y_sim)
    fit = S.SNN(k, eps, ms).fit(X)
    assert_fit((fit.labels_, fit.core_sample_indices_, fit.density_), name)
    np.testing.assert_array_equal(fit.neighbors_, y_idx)
    assert fit._sim.is_cuda and fit._sim_host is None          # the similarities stay on the device until asked for
    np.testing.assert_array_equal(fit.similarity_, y_sim)
    np.testing.assert_array_equal(S.SNN(k, eps, ms).fit_predict(X), fit.labels_)
    print('%s: label passes %s' % (name, fit.stats_['label_passes']))


@pytest.mark.parametrize('name,eps_values', [('chain400_k6', (2, 3, 4)), ('n130_d256_k16', (5, 7, 9))])
def test_sweep_equals_single_fits(name, eps_values):
    k, ms = CASES[name][2], CASES[name][4]
    X = points(name)
    stats = {}
    sweep = S.snn_sweep(X, k, eps_values, ms, stats=stats)
    print('%s: label passes per eps %s' % (name, stats['label_passes']))
    assert len(sweep) == len(stats['label_passes']) == 3
    for eps, got in zip(eps_values, sweep):
        assert_fit(got, name, eps, ms)
        fit = S.SNN(k, eps, ms).fit(X)
        for a, b in zip(got, (fit.labels_, fit.core_sample_indices_, fit.density_)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(stats['similarity_hist'], np.bincount(yard(name)[1].ravel(), minlength=k + 1))
    if name == 'chain400_k6':          # a component of two or more points moves a label in the first pass, and only a pass that moves none is the last
        assert stats['label_passes'][1] > 1


def test_min_samples_zero_is_jarvis_patrick():
    name = 'n65_d8_k8'
    k, eps = CASES[name][2:4]
    fit = S.SNN(k, eps, 0).fit(points(name))
    assert_fit((fit.labels_, fit.core_sample_indices_, fit.density_), name, eps, 0)
    assert len(fit.core_sample_indices_) == 65 and (fit.labels_ >= 0).all()


def test_input_forms_and_two_calls_give_identical_results():
    name = 'n1030_d12_k64'
    k, eps, ms = CASES[name][2:5]
    X = points(name)
    wide = torch.zeros((2 * len(X), 20), device=DEV)
    wide[::2, 3:15] = torch.as_tensor(X, device=DEV)
    forms = [X, torch.as_tensor(X, device=DEV), wide[::2, 3:15], X]
    assert not forms[2].is_contiguous()
    fits = [S.SNN(k, eps, ms).fit(f) for f in forms]
    for fit in fits:
        assert_fit((fit.labels_, fit.core_sample_indices_, fit.density_), name)
        np.testing.assert_array_equal(fit.neighbors_, fits[0].neighbors_)
        np.testing.assert_array_equal(fit.similarity_, fits[0].similarity_)
    idx, sim = S.snn_graph(forms[2], k, return_device=True)
    assert idx.is_cuda and sim.is_cuda
    np.testing.assert_array_equal(sim.cpu().numpy(), yard(name)[1])


@pytest.mark.parametrize('name', ['n65_d8_k8', 'n1600_d8_k257'])
def test_similarity_overwrites_every_entry_and_nothing_else(name):
    idx, sim = yard(name)[:2]
    n, k = idx.shape
    guard, sentinel = 256, 0x5a5a5a5a
    buf = torch.full((guard + n * k + guard,), sentinel, dtype=torch.int32, device=DEV)
    d_idx = torch.as_tensor(idx.copy(), device=DEV)
    out = ctypes.c_void_p(buf.data_ptr() + 4 * guard)
    N.check(N.lib().dic_snn_similarity(N.ptr(d_idx), n, k, out, N.stream_of(buf)), 'dic_snn_similarity')
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[guard:guard + n * k].reshape(n, k), sim)          # (no yardstick value is the sentinel: sim <= 1024)
    assert (got[:guard] == sentinel).all() and (got[-guard:] == sentinel).all()


def test_entries_outside_the_range_count_as_absent():
    """idx is a public input: an entry outside [0, N) is absent from its list and is never a row index."""
    name = 'n65_d8_k8'
    idx = yard(name)[0].copy()
    n, k = idx.shape
    rng = np.random.default_rng(0)
    for bad in (-1, n, n + 7, -2 ** 31, 2 ** 31 - 1):
        idx[rng.integers(0, n, 6), rng.integers(0, k, 6)] = bad
    sets = [set(int(v) for v in r if 0 <= v < n) for r in idx]
    ref = np.zeros((n, k), np.int32)
    for i in range(n):
        for c in range(k):
            j = int(idx[i, c])
            if 0 <= j < n and j != i and i in sets[j]:
                ref[i, c] = len(sets[i] & sets[j])
    sim = S.snn_similarity(idx)
    np.testing.assert_array_equal(sim.cpu().numpy(), ref)
    labels, core, density = S.snn_labels(idx, sim, 4, 4)
    y_labels, y_core, y_density, _ = snn_labels_exact(np.where((idx >= 0) & (idx < n), idx, np.arange(n)[:, None]), ref, 4, 4)
    np.testing.assert_array_equal(density, y_density)
    np.testing.assert_array_equal(core, y_core)
    np.testing.assert_array_equal(labels, y_labels)


# ------------------------------------------------------------------------------------------------------------------------------------- p2 and p4
SNN_FLAGS = ['--snn_eps', '5']          # k = feat_dim + 1 = 17 and min_samples = k // 4 = 4 by default


def test_p2_snn_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import cluster_stats
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'snn', '--snn_k', '12', '--snn_eps', '4', '6', '8', '--snn_min_samples', '4'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X = data['training']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_snn_aligned' / 'plot'
    table, hist, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Snn.FILES)
    assert list(table.columns) == ['eps', 'n_core', 'n_clusters', 'n_noise', 'silhouette', 'denoise_silhouette', 'k', 'min_samples']
    assert table.eps.tolist() == [4, 6, 8] and table.k.tolist() == [12] * 3 and table.min_samples.tolist() == [4] * 3
    assert list(hist.columns) == ['similarity', 'pairs'] and hist.similarity.tolist() == list(range(13)) and hist.pairs.sum() == 400 * 12
    assert list(labels.columns) == ['eps4', 'eps6', 'eps8'] and len(labels) == len(X)
    stats = {}
    sweep = S.snn_sweep(X, 12, [4, 6, 8], 4, stats=stats)
    np.testing.assert_array_equal(hist.pairs.to_numpy(), stats['similarity_hist'])
    for row, (eps, (lab, core, _)) in enumerate(zip((4, 6, 8), sweep)):
        np.testing.assert_array_equal(labels['eps%d' % eps].to_numpy(), lab)
        assert table.n_core[row] == len(core) and table.n_noise[row] == (lab == -1).sum() and table.n_clusters[row] == lab.max() + 1
        if lab.max() > 0:          # the silhouettes: exactly as the dbscan branch computes them
            keep = lab != -1
            assert table.silhouette[row] == cluster_stats.silhouette_score(torch.as_tensor(X, device=DEV), lab)
            assert table.denoise_silhouette[row] == cluster_stats.silhouette_score(torch.as_tensor(X[keep], device=DEV), lab[keep])
    assert (table.n_clusters >= 2).any()
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(dtype=float), table.to_numpy(dtype=float), equal_nan=True)
    # a second run finds the files and does not recompute; overwrite=True does
    sn = p2.Snn(12, [4, 6, 8], 4, str(plot.parent))
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Snn.FILES]
    calls = []
    real = p2.snn_sweep
    monkeypatch.setattr(p2, 'snn_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = sn.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Snn.FILES] == stamps and sn.labels_ is None
    assert np.array_equal(again.to_numpy(dtype=float), table.to_numpy(dtype=float), equal_nan=True)
    sn.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and sorted(sn.labels_) == [4, 6, 8]
    # the defaults: k = feat_dim + 1, eps = round(k t / 10), min_samples = k // 4
    args = p2.get_arguments(['--cluster_method', 'snn'])
    args.restore_metric = ['ae_mse']
    for name in p2.Snn.FILES:
        (plot / name).unlink()
    df = p2.main(args)['ae_mse']
    assert df.eps.tolist() == p2.snn_default_eps(17) and df.k.tolist() == [17] * 7 and df.min_samples.tolist() == [4] * 7


@pytest.mark.parametrize('transfer', ['centre', 'knn'])
def test_p4_snn_branch(transfer, tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'snn', '--transfer', transfer] + SNN_FLAGS)
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_snn_aligned'
    stem = '%s_snn-k17-eps5-ms4' + ('_knn' if transfer == 'knn' else '') + '.npy'
    assert sorted(p.name for p in out.iterdir()) == sorted(stem % c for c in COHORTS)
    saved = {c: np.load(out / (stem % c), allow_pickle=True).item() for c in COHORTS}
    keys = ['cluster_id', 'encounter_id', 'hidden'] + (['cluster_vote'] if transfer == 'knn' else [])
    for cohort in COHORTS:
        s = saved[cohort]
        assert sorted(s) == sorted(keys) and len(s['cluster_id']) == len(data[cohort]['hidden'])
        assert sorted(set(s['cluster_id'].tolist()) - {-1}) == [0, 1, 2]
        if transfer == 'centre':          # every cohort is fitted on its own: the same partition as a direct fit, re-numbered
            raw = S.SNN(17, 5, 4).fit(data[cohort]['hidden']).labels_
            assert ((raw == -1) == (s['cluster_id'] == -1)).all()
            pairs = set(zip(raw.tolist(), s['cluster_id'].tolist()))
            assert len(pairs) == len(set(raw.tolist())) == len(set(s['cluster_id'].tolist()))
    train = saved['training']
    # generate_align_map: ids by descending mean of channel 0
    ob = data['training']['ob'][:, 0, :].mean(1)
    means = [ob[train['cluster_id'] == c].mean() for c in range(3)]
    assert means[0] > means[1] > means[2]
    if transfer == 'knn':
        assert (train['cluster_vote'] == 1).all() and train['cluster_vote'].dtype == np.float32
        for cohort in COHORTS[1:]:
            ref, share = K.knn_transfer_labels(train['hidden'], train['cluster_id'], saved[cohort]['hidden'], 17)          # --transfer_k: feat_dim + 1
            np.testing.assert_array_equal(saved[cohort]['cluster_id'], ref)
            np.testing.assert_array_equal(saved[cohort]['cluster_vote'], share)
            assert saved[cohort]['cluster_id'].dtype == train['cluster_id'].dtype
