"""Gaussian mixtures on the GPU (csrc/dic_gmm.hip, gmm.py, the p2 / p4 gmm branches) against the numpy f64 yardstick of tests/test_gmm_host.py and sklearn.

The cases are the smallest shapes at which the kernels can still go wrong (tests/test_gmm_host.py: CASES): one workgroup (2 rows) and two (17), full-width
rows (D = 256), the ragged tail of a 16-row tile, the full grid of 256 workgroups with 17 rows each (4100), K = 1 and K = 32, truly soft responsibilities
(the overlap cases), a variance held up by reg_covar alone (same), duplicates, a strided input and zero-padded features.  test_gmm_host.py shows on the CPU
that every stopping decision and every label of every case is clear, so n_iter_, converged_ and the labels are held to equality.

test_one_em_pass prints the largest ratio of a deviation to its bound per case; DESIGN.md section 5 records them."""
import functools
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import gmm as G
from deep_interpolation_clustering_amd.gmm import GaussianMixture, gmm_sweep
from deep_interpolation_clustering_amd.info import COHORTS
from test_gmm_host import (CASES, EPS, N_INIT_CASES, REG, TOL, blobs, cov_of, fit_rtol, initial_labels, points, rel, winner, y_estep, yardstick)
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

ATTRS = ('weights_', 'means_', 'covariances_', 'precisions_', 'precisions_cholesky_', 'lower_bounds_', 'labels_')


def device_points(case):
    """The case's points on the device; 'strided' as a view with a row stride of 16 floats into a buffer whose other columns hold NaN."""
    X = torch.as_tensor(np.array(points(case)), device='cuda')
    if case != 'strided':
        return X
    buf = torch.full((X.shape[0], 16), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, 4:12] = X
    view = buf[:, 4:12]
    assert view.stride(0) == 16 and not view.is_contiguous()
    return view


def _padded(a, d, fill):
    out = torch.full((a.shape[0], d), fill, dtype=torch.float64, device='cuda')
    out[:, :a.shape[1]] = torch.as_tensor(a, device='cuda')
    return out.contiguous()


def _init_model(case, **kw):
    """The estimator started from the yardstick's initial M-step."""
    _, K, cov = CASES[case]
    y = yardstick(case)
    w, mu, var = y['init']
    return GaussianMixture(K, covariance_type=cov, tol=TOL, reg_covar=REG, weights_init=w, means_init=mu + y['c'], precisions_init=1.0 / cov_of(var, cov), **kw)


@functools.lru_cache(maxsize=None)
def device_fit(case):
    x = device_points(case)
    keep = x.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        model = _init_model(case).fit(x)
    assert not [c for c in caught if 'did not converge' in str(c.message)]          # (every case converges)
    assert torch.equal(x, keep)          # the input is only read
    return model


def log_bound(case, logp):
    """4 (D + 16) 2^-53 max(1, max |log p|): the same-sign-sum bound of a length-D f64 sum, taken on both sides and carried through the log-sum-exp."""
    d0 = points(case).shape[1]
    return 4.0 * (d0 + 16) * EPS * max(1.0, float(np.max(np.abs(logp))))


@pytest.mark.parametrize('case', list(CASES))
def test_one_em_pass(case):
    _, K, cov = CASES[case]
    y = yardstick(case)
    n, d0 = points(case).shape
    pts = G._Points(device_points(case), shift=y['c'])
    w0, mu0, var0 = y['init']
    w = torch.as_tensor(w0, device='cuda').reshape(1, K).contiguous()
    mu, var = _padded(mu0, pts.d, 0.0)[None].contiguous(), _padded(var0, pts.d, 1.0)[None].contiguous()
    M, logp, lse, logr, (w1, mu1, var1, nk1) = y['first']
    B = log_bound(case, logp)
    e = G.estep(pts, w[0], mu[0], var[0], lse=True, log_resp=True, labels=True, total=True)
    got_lse, got_logr = e['lse'].cpu().numpy(), e['log_resp'].cpu().numpy()
    ratios = {'lse': np.max(np.abs(got_lse - lse)) / B, 'log r': np.max(np.abs(got_logr - logr)) / B}
    assert np.array_equal(e['labels'].cpu().numpy(), logp.argmax(axis=1))
    assert abs(float(e['total'][0]) - lse.sum()) <= (B + n * EPS) * np.abs(lse).sum()
    status, lbs = G.em(pts, G.COV_TYPES[cov], REG, w, mu, var, TOL, 1)
    assert status[0, 0] == 1 and status[0, 1] == 1 and status[0, 2] == 0 and lbs.shape == (1, 1)
    assert abs(lbs[0, 0] - lse.mean()) <= (B + n * EPS) * np.abs(lse).mean() and status[0, 3] == lbs[0, 0]
    # the new parameters: (B + N 2^-53) times the absolute-value sums
    r, Xs, rate = np.exp(logr), y['Xs'], B + n * EPS
    b_n = rate * r.sum(axis=0)
    b_mu = rate * (r[:, :, None] * np.abs(Xs)[:, None, :]).sum(axis=0) / nk1[:, None]
    b_var = rate * (r[:, :, None] * (Xs * Xs)[:, None, :]).sum(axis=0) / nk1[:, None] + 2.0 * np.abs(mu1) * b_mu
    if cov == 'spherical':
        b_var = np.repeat(b_var.mean(axis=1)[:, None], d0, axis=1)
    got_w, got_mu, got_var = w[0].cpu().numpy(), mu[0, :, :d0].cpu().numpy(), var[0, :, :d0].cpu().numpy()
    ratios['n_k'] = np.max(np.abs(got_w - w1) * n / b_n)          # (w = n_k / N up to the normalisation, which is 1 to within K 2^-52)
    ratios['means'] = np.max(np.abs(got_mu - mu1) / np.maximum(b_mu, np.finfo(np.float64).tiny))
    ratios['variances'] = np.max(np.abs(got_var - var1) / np.maximum(b_var, np.finfo(np.float64).tiny))
    print(case, 'one EM pass: bound on log p', B, 'largest deviation / bound:', {k: float('%.3g' % v) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if pts.d > d0:          # the padding: means 0, and nothing else reads its variances
        assert torch.all(mu[0, :, d0:] == 0)


@pytest.mark.parametrize('case', list(CASES))
def test_whole_fit_equals_the_yardstick(case):
    _, K, cov = CASES[case]
    y = yardstick(case)
    m = device_fit(case)
    assert m.n_iter_ == y['n_iter'] and m.converged_ is True and y['converged']
    assert m.labels_.dtype == np.int32 and np.array_equal(m.labels_, y['labels'])
    w, mu, var = y['final']
    dev = {'lower_bounds': rel(m.lower_bounds_, y['lbs']), 'weights': rel(m.weights_, w), 'means': rel(m.means_, mu + y['c']),
           'covariances': rel(m.covariances_, cov_of(var, cov))}
    print(case, 'whole fit: n_iter', m.n_iter_, 'relative deviations', dev, 'allowed', fit_rtol(case))
    assert max(dev.values()) <= fit_rtol(case)
    assert m.lower_bound_ == m.lower_bounds_[-1] and m.n_features_in_ == points(case).shape[1]
    for name in ATTRS[:6]:
        assert getattr(m, name).dtype == np.float64
    assert m.covariances_.shape == ((K, points(case).shape[1]) if cov == 'diag' else (K,)) and m.means_.shape == (K, points(case).shape[1])
    np.testing.assert_allclose(m.precisions_, 1.0 / m.covariances_, rtol=1e-15)
    np.testing.assert_allclose(m.precisions_cholesky_ ** 2, m.precisions_, rtol=1e-15)
    if case == 'same_k1':
        np.testing.assert_allclose(m.covariances_, REG, rtol=1e-13, atol=0)


@pytest.mark.parametrize('case', list(CASES))
def test_two_calls_and_a_host_array_give_identical_bits(case):
    m = device_fit(case)
    again = _init_model(case).fit(device_points(case))
    host = _init_model(case).fit(np.array(points(case)))          # the contiguous (and, for d13, padded) copy; for `strided` the same points without the gaps
    for name in ATTRS:
        assert getattr(m, name).tobytes() == getattr(again, name).tobytes() == getattr(host, name).tobytes(), name
    assert m.n_iter_ == again.n_iter_ == host.n_iter_
    if case == 'strided':          # read where it lies
        view = device_points(case)
        assert G._Points(view).x.data_ptr() == view.data_ptr() and torch.isnan(view._base[:, :4]).all() and torch.isnan(view._base[:, 12:]).all()


@functools.lru_cache(maxsize=None)
def three_restarts(case):
    _, K, cov = CASES[case]
    pts = G._Points(device_points(case))
    m = GaussianMixture(K, covariance_type=cov, n_init=3)._fit_points(pts, init_labels=initial_labels(case, 3))
    return pts, m


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_pick_the_winner_and_do_not_depend_on_each_other(case):
    _, K, cov = CASES[case]
    pts, m = three_restarts(case)
    ys = [yardstick(case, r, 3) for r in range(3)]
    best = winner(case)
    assert [int(v) for v in m._status[:, 1]] == [y['n_iter'] for y in ys] and np.all(m._status[:, 0] == 1) and np.all(m._status[:, 2] == 1)
    assert m.lower_bound_ == m._status[best, 3] == np.max(m._status[:, 3]) and m.n_iter_ == ys[best]['n_iter']
    assert np.array_equal(m.labels_, ys[best]['labels'])
    w, mu, var = ys[best]['final']
    assert max(rel(m.weights_, w), rel(m.means_, mu + ys[best]['c']), rel(m.covariances_, cov_of(var, cov)), rel(m.lower_bounds_, ys[best]['lbs'])) <= fit_rtol(case)
    for r in range(3):
        # alone, and with max_iter cut at its own n_iter_: the same bytes -- a done restart is frozen while the others continue
        for max_iter in (100, ys[r]['n_iter']):
            solo = GaussianMixture(K, covariance_type=cov, n_init=1, max_iter=max_iter)._fit_points(pts, init_labels=initial_labels(case, 3)[r:r + 1])
            for part, alone in zip(m._all_parameters, solo._all_parameters):
                assert part[r].tobytes() == alone[0].tobytes()
            assert m._all_lower_bounds[r, :ys[r]['n_iter']].tobytes() == solo._all_lower_bounds[0, :ys[r]['n_iter']].tobytes()
            assert solo.converged_ and solo.n_iter_ == ys[r]['n_iter']
    assert np.all(np.isnan(m._all_lower_bounds[0, ys[0]['n_iter']:]))


def test_padding_adds_nothing_and_a_single_iteration_does_not_converge():
    y = yardstick('d13')
    m = device_fit('d13')
    assert m.means_.shape == (3, 13) and m.covariances_.shape == (3, 13)
    np.testing.assert_allclose(m.lower_bounds_, y['lbs'], rtol=fit_rtol('d13'), atol=0)          # (the log-determinant: 13 columns, not 16)
    with pytest.warns(UserWarning, match='Best performing initialization did not converge'):
        one = _init_model('overlap_k4', max_iter=1).fit(device_points('overlap_k4'))
    assert one.converged_ is False and one.n_iter_ == 1 and len(one.lower_bounds_) == 1
    assert one.lower_bounds_[0] == device_fit('overlap_k4').lower_bounds_[0]


@pytest.mark.parametrize('case,held', [('n1030_k4', lambda: blobs(333, 8, 6)), ('overlap_k4', lambda: blobs(517, 8, 11, n_centers=4, spread=1.2)),
                                       ('sph_d256_k5', lambda: blobs(131, 256, 14, n_centers=6, spread=0.15)), ('d13', lambda: blobs(77, 13, 15))])
def test_predict_and_scores_on_held_out_points(case, held):
    _, K, cov = CASES[case]
    m = device_fit(case)
    H = held()
    var = m.covariances_ if cov == 'diag' else np.repeat(m.covariances_[:, None], H.shape[1], axis=1)
    _, logp, lse, logr = y_estep(H.astype(np.float64) - m._shift, m.weights_, m._means_shifted, var)
    B = log_bound(case, logp)
    top = np.sort(logp, axis=1)
    decided = (top[:, -1] - top[:, -2]) > 1e-4 if K > 1 else np.ones(len(H), bool)
    pred, proba, scores, score = m.predict(H), m.predict_proba(torch.as_tensor(H, device='cuda')), m.score_samples(H), m.score(H)
    assert pred.shape == (len(H),) and proba.shape == (len(H), K) and proba.dtype == np.float64 and scores.dtype == np.float64
    assert decided.mean() > 0.98 and np.array_equal(pred[decided], logp.argmax(axis=1)[decided])
    assert np.max(np.abs(scores - lse)) <= B and np.max(np.abs(proba - np.exp(logr))) <= B
    assert np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 1e-12
    assert abs(score - lse.mean()) <= B + len(H) * EPS * np.abs(lse).mean()
    assert np.array_equal(pred[decided], proba.argmax(axis=1)[decided])
    n = len(H)
    assert m.bic(H) == -2 * score * n + m._n_parameters() * np.log(n) and m.aic(H) == -2 * score * n + 2 * m._n_parameters()
    with pytest.raises(ValueError, match='expecting %d features' % H.shape[1]):
        m.predict(H[:, :-1])


@pytest.mark.parametrize('case', ['n1030_k4', 'n4100_k7'])
def test_end_to_end_equals_sklearn(case):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov = CASES[case]
    X = np.array(points(case))
    ours = GaussianMixture(K, covariance_type=cov, init_params='kmeans', random_state=5).fit(X)
    ref = mix.GaussianMixture(K, covariance_type=cov, init_params='kmeans', random_state=5).fit(X.astype(np.float64))
    assert np.array_equal(ours.fit_predict(X), ours.labels_)
    assert np.array_equal(ours.labels_, ref.predict(X.astype(np.float64)))
    assert ours.n_iter_ == ref.n_iter_ and ours.converged_ == ref.converged_
    dev = max(rel(ours.weights_, ref.weights_), rel(ours.means_, ref.means_), rel(ours.covariances_, ref.covariances_), rel(ours.lower_bounds_, ref.lower_bounds_))
    print(case, 'end to end against sklearn: relative deviation', dev, 'allowed', fit_rtol(case))
    assert dev <= fit_rtol(case)


@pytest.mark.parametrize('init', ['k-means++', 'random_from_data', 'random'])
def test_other_initialisations_and_the_sweep(init):
    """The draws follow sklearn's order, so a seeded fit is repeatable and two restarts differ; the sweep gives the fits of its Ks."""
    X = device_points('overlap_k4')
    a = GaussianMixture(4, init_params=init, n_init=2, random_state=3).fit(X)
    b = GaussianMixture(4, init_params=init, n_init=2, random_state=np.random.RandomState(3)).fit(X)
    for name in ATTRS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()
    assert a._status[0, 3] != a._status[1, 3] and np.isfinite(a.lower_bound_) and abs(a.weights_.sum() - 1.0) < 1e-12
    sweep = gmm_sweep(X, [2, 4], init_params=init, n_init=2, random_state=3)
    assert sorted(sweep) == [2, 4] and sweep[4].means_.tobytes() == a.means_.tobytes() and sweep[2].means_.shape == (2, 8)
    assert sweep[2].bic(X) != sweep[4].bic(X)


def test_a_workspace_that_does_not_fit_raises_memory_error(monkeypatch):
    X = np.array(points('n255_k3'))
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (1000, 1 << 30))
    with pytest.raises(MemoryError, match=r'255 points needs (\d+) bytes on the device, 1000 are free') as err:
        GaussianMixture(3).fit(X)
    assert int(str(err.value).split('needs ')[1].split(' bytes')[0]) >= 16 * 8 * (3 * 129 + 1)


def test_p2_gmm_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import cluster_stats
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'gmm', '--k_max', '4', '--n_init', '2'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X, V = data['training']['hidden'], data['validation']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_gmm_aligned' / 'plot'
    table, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Gmm.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(table.columns) == ['k', 'lower_bound', 'bic', 'aic', 'n_iter', 'converged', 'valid_score'] + metrics and table.k.tolist() == [2, 3, 4]
    assert list(labels.columns) == ['k2', 'k3', 'k4'] and len(labels) == len(X)
    assert np.all(np.isfinite(table[['lower_bound', 'bic', 'aic', 'valid_score']].to_numpy())) and np.all(table.n_iter >= 1)
    n_par = np.array([k * 16 + k * 16 + k - 1 for k in (2, 3, 4)])
    np.testing.assert_allclose(table.bic - table.aic, n_par * (np.log(len(X)) - 2.0), rtol=1e-9)
    for row, k in enumerate((2, 3, 4)):
        lab = labels['k%d' % k].to_numpy()
        assert set(lab.tolist()) <= set(range(k))
        lab = np.unique(lab, return_inverse=True)[1]
        if lab.max() > 0:
            direct = [cluster_stats.silhouette_score(X, lab), cluster_stats.davies_bouldin_score(X, lab), cluster_stats.calinski_harabasz_score(X, lab)]
            np.testing.assert_allclose(table[metrics].to_numpy()[row], direct, rtol=1e-12, atol=0)
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy(), equal_nan=True)
    # a second run finds the files and does not recompute; overwrite=True does
    gm = p2.Gmm(4, str(plot.parent), metrics, n_init=2)
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Gmm.FILES]
    calls = []
    real = p2.gmm_sweep
    monkeypatch.setattr(p2, 'gmm_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = gm.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Gmm.FILES] == stamps and gm.fits_ is None
    assert np.array_equal(again.to_numpy(), table.to_numpy(), equal_nan=True)
    redo = gm.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and sorted(gm.fits_) == [2, 3, 4] and list(redo.columns) == list(table.columns)
    np.testing.assert_allclose(redo.valid_score, [gm.fits_[k].score(V) for k in (2, 3, 4)], rtol=0, atol=0)


def test_p4_gmm_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.GaussianMixture):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'GaussianMixture', Recording)
    args = p4.get_arguments(['--cluster_method', 'gmm', '--num_clusters', '3'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_gmm_aligned'
    saved = {cohort: np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1
    model = made[0]
    for cohort in COHORTS:
        s = saved[cohort]
        assert sorted(s) == ['cluster_id', 'cluster_prob', 'encounter_id', 'hidden'] and len(s['cluster_id']) == len(data[cohort]['hidden'])
        prob = s['cluster_prob']
        assert prob.dtype == np.float32 and prob.shape == (len(s['cluster_id']), 3) and np.max(np.abs(prob.sum(axis=1) - 1.0)) < 1e-6
        assert np.array_equal(s['cluster_id'], prob.argmax(axis=1))
        # every cohort is labelled by the one training model, in its aligned order
        assert np.array_equal(s['cluster_id'], model.predict(data[cohort]['hidden']))
        assert np.array_equal(prob, model.predict_proba(data[cohort]['hidden']).astype(np.float32))
    ids = np.asarray(saved['training']['cluster_id'])
    sbp = data['training']['ob'][:, 0, :].mean(1)
    means = [sbp[ids == i].mean() for i in range(3)]
    assert means[0] > means[1] > means[2]
    assert abs(model.weights_.sum() - 1.0) < 1e-12 and model.means_.shape == (3, 16)
    # an existing result is left alone
    stamps = [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
