"""Fuzzy c-means on the GPU (csrc/dic_fcm.hip, fcm.py, the p2 / p4 fcm branches) against the numpy f64 yardstick of tests/test_fcm_host.py.

The cases are the smallest shapes at which the kernels can still go wrong (tests/test_fcm_host.py: CASES): one workgroup (3 rows) and two (17), full-width
rows (D = 256), the ragged tail of a 16-row tile, the full grid of 256 workgroups with 17 rows each (4100), K = 2 and K = 32, zero-padded features,
duplicate rows, a strided input, and both forms of the memberships (the m == 2 short cut; exp / log at m = 1.2 and 1.05).  The initial centres are rows of
the points, so every first pass meets distances that are exactly 0.  test_fcm_host.py shows on the CPU that every stopping decision and every label of every
parity case is clear, so n_iter_, converged_ and the labels are held to equality; whole fits are held to 16 x the CPU's own pairwise / sequential figure
(test_fcm_host.BASE), never less than 1e-13."""
import functools
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import cluster_stats
from deep_interpolation_clustering_amd import fcm as F
from deep_interpolation_clustering_amd.fcm import FuzzyCMeans, fcm_sweep
from deep_interpolation_clustering_amd.info import COHORTS
from test_fcm_host import (ALL, CASES, COLLAPSE, MAX_ITER, N_INIT_CASES, TOL, fit_rtol, indices, initial_centers, points, winner, y_memberships, yardstick)
from test_gmm_host import blobs, rel
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
ATTRS = ('cluster_centers_', 'labels_', 'objectives_', 'center_separation_')
SCALARS = ('objective_', 'partition_coefficient_', 'partition_entropy_', 'modified_partition_coefficient_', 'xie_beni_', 'n_iter_', 'converged_')


def device_points(case):
    return torch.as_tensor(np.array(points(case)), device='cuda')


def _model(case, **kw):
    _, K, m = ALL[case]
    kw.setdefault('centers_init', initial_centers(case))
    return FuzzyCMeans(K, m=m, **kw)


@functools.lru_cache(maxsize=None)
def device_fit(case):
    x = device_points(case)
    keep = x.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        model = _model(case).fit(x)
    assert torch.equal(x, keep)          # the input is only read
    return model, [str(c.message) for c in caught]


def u_bound(d0, m):
    """A bound on |u - u'| for two f64 evaluations of the definition that differ in the order of their sums and in libm's last bits: every d2 is a sum of d0
    non-negative terms, so either evaluation is within (d0 + 2) 2^-53 of it, relatively; the ratio dmin / d2 carries two of them and a division, the power
    multiplies a relative error by p = 1 / (m - 1), and the normalisation by a sum of at most 32 non-negative terms adds less than the 16 in the factor.
    u <= 1, so the relative bound is an absolute one: 8 (d0 + 16) 2^-53 max(1, p)."""
    return 8.0 * (d0 + 16) * EPS * max(1.0, 1.0 / (m - 1.0))


def same_bytes(a, b):
    for name in ATTRS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    for name in SCALARS:
        assert getattr(a, name) == getattr(b, name), name
    assert a.coincident_centers_ == b.coincident_centers_


@pytest.mark.parametrize('case', list(CASES))
def test_one_iteration(case):
    _, K, m = CASES[case]
    y = yardstick(case)
    n, d0 = points(case).shape
    pts = F._Points(device_points(case), shift=y['c'])
    centers = F.shifted_centers(pts, initial_centers(case))
    assert centers.shape == (1, K, pts.d) and np.array_equal(centers[0, :, :d0].cpu().numpy(), y['V0'])
    d2, u, w, (J, S2, SE), V1 = y['first']
    out = F.memberships(pts, m, centers[0].contiguous(), u=True, labels=True, d2=True, sums=True)
    got_u, got_d2, got_labels, got_sums = (out[k].cpu().numpy() for k in ('u', 'd2', 'labels', 'sums'))
    rtol = fit_rtol(case)
    assert np.array_equal(got_d2 == 0, d2 == 0) and (d2 == 0).any(axis=1).sum() >= K          # the rows that are centres: exactly 0 on both sides
    assert np.array_equal(got_u[(d2 == 0).any(axis=1)], u[(d2 == 0).any(axis=1)])          # .. and their memberships exactly [d2 == 0] / count
    top = np.sort(u, axis=1)
    decided = top[:, -1] - top[:, -2] > 1e-9
    assert got_labels.dtype == np.int32 and np.array_equal(got_labels[decided], u.argmax(axis=1)[decided])
    dev = {'d2': rel(got_d2, d2), 'u': rel(got_u, u), 'J': abs(got_sums[0] - J) / J, 'S2': abs(got_sums[1] - S2) / S2, 'SE': abs(got_sums[2] - SE) / max(abs(SE), 1.0)}
    status, objs = F.iterate(pts, m, centers, TOL, 1)
    assert status[0, 0] == 1 and status[0, 1] == 1 and status[0, 2] == 0 and objs.shape == (1, 1)          # the first iteration never stops by tol
    assert objs[0, 0] == got_sums[0] == status[0, 3]          # the same pass, the same order: the same bits
    dev['centres'] = rel(centers[0, :, :d0].cpu().numpy(), V1)
    print(case, 'one iteration: relative deviations', {k: float('%.3g' % v) for k, v in dev.items()}, 'allowed', rtol)
    assert max(dev.values()) <= rtol, dev
    if pts.d > d0:          # the padding stays zero
        assert torch.all(centers[0, :, d0:] == 0)


@pytest.mark.parametrize('case', list(CASES))
def test_whole_fit_equals_the_yardstick(case):
    _, K, m = CASES[case]
    y = yardstick(case)
    model, caught = device_fit(case)
    assert not caught, caught          # (no parity case collapses)
    assert model.n_iter_ == y['n_iter'] and model.converged_ is True and y['converged']
    assert model.labels_.dtype == np.int32 and np.array_equal(model.labels_, y['labels'])
    got_u = model.memberships(device_points(case))
    dev = {'J': rel(model.objectives_, y['J']), 'centres': rel(model._centers_shifted, y['V']), 'u': rel(got_u, y['u'])}
    print(case, 'whole fit: n_iter', model.n_iter_, 'relative deviations', dev, 'allowed', fit_rtol(case))
    assert max(dev.values()) <= fit_rtol(case)
    pc, pe, mpc = indices(y, K)
    assert abs(model.partition_coefficient_ - pc) <= fit_rtol(case) * pc and abs(model.partition_entropy_ - pe) <= fit_rtol(case) * max(pe, 1.0)
    assert model.objective_ == model.objectives_[-1] and model.n_features_in_ == points(case).shape[1] and model.coincident_centers_ == []
    assert model.cluster_centers_.shape == (K, points(case).shape[1]) and model.cluster_centers_.dtype == np.float64
    np.testing.assert_allclose(model.cluster_centers_, y['V'] + y['c'], rtol=0, atol=fit_rtol(case) * np.abs(y['V']).max() + 4 * EPS * np.abs(y['c']).max())


def test_rows_on_one_two_and_three_equal_centres():
    X = np.array(blobs(40, 12, 21))
    p, q, r = X[5].astype(np.float64), X[17].astype(np.float64), X[30].astype(np.float64)
    C = np.stack([p, q, q, r, r, r])
    pts = F._Points(X)
    centers = F.shifted_centers(pts, C)
    for m in (2.0, 1.2):
        out = F.memberships(pts, m, centers, u=True, labels=True, d2=True)
        u, labels = out['u'].cpu().numpy(), out['labels'].cpu().numpy()
        assert np.array_equal(u[5], [1, 0, 0, 0, 0, 0]) and np.array_equal(u[17], [0, 0.5, 0.5, 0, 0, 0])
        assert np.array_equal(u[30], [0, 0, 0, 1 / 3, 1 / 3, 1 / 3]) and labels[[5, 17, 30]].tolist() == [0, 1, 3]
        assert np.max(np.abs(u.sum(axis=1) - 1.0)) <= 1e-14 and np.all(np.isfinite(u))
        # an iteration from these centres: equal centres get equal weights and stay equal
        moved = centers[None].clone()
        status, _ = F.iterate(pts, m, moved, TOL, 1)
        assert status[0, 1] == 1 and torch.equal(moved[0, 1], moved[0, 2]) and torch.equal(moved[0, 3], moved[0, 4]) and torch.equal(moved[0, 4], moved[0, 5])


@pytest.mark.parametrize('case', ['n17_k2', 'n1030_k4', 'd13', 'overlap_k4_m1.2', 'n257_d256_k5_m1.2'])
def test_two_calls_a_host_array_and_a_device_tensor_give_identical_bits(case):
    model, _ = device_fit(case)
    again = _model(case).fit(device_points(case))
    host = _model(case).fit(np.array(points(case)))
    same_bytes(model, again)
    same_bytes(model, host)
    X = device_points(case)
    assert model.memberships(X).tobytes() == again.memberships(np.array(points(case))).tobytes()
    assert model.transform(X).tobytes() == host.transform(X).tobytes() and np.array_equal(model.predict(X), model.labels_)


def test_a_strided_view_and_its_copy_give_identical_bits():
    X = torch.as_tensor(blobs(257, 8, 10), device='cuda')
    buf = torch.full((257, 16), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, 4:12] = X
    view = buf[:, 4:12]
    assert view.stride(0) == 16 and not view.is_contiguous()
    assert F._Points(view).x.data_ptr() == view.data_ptr()          # read where it lies
    init = X[[3, 100, 200]].double().cpu().numpy()[None]
    a = FuzzyCMeans(3, m=1.5, centers_init=init).fit(view)
    b = FuzzyCMeans(3, m=1.5, centers_init=init).fit(X)
    same_bytes(a, b)
    assert a.memberships(view).tobytes() == b.memberships(X).tobytes() and np.all(np.isfinite(a.cluster_centers_))
    assert torch.isnan(buf[:, :4]).all() and torch.isnan(buf[:, 12:]).all()


@functools.lru_cache(maxsize=None)
def three_restarts(case):
    _, K, m = CASES[case]
    return FuzzyCMeans(K, m=m, n_init=3, centers_init=initial_centers(case, 3)).fit(device_points(case))


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_pick_the_smallest_objective_and_do_not_depend_on_each_other(case):
    _, K, m = CASES[case]
    model = three_restarts(case)
    ys = [yardstick(case, r, 3) for r in range(3)]
    best = winner(case)
    assert [int(v) for v in model._status[:, 1]] == [y['n_iter'] for y in ys] and np.all(model._status[:, 0] == 1) and np.all(model._status[:, 2] == 1)
    assert model.objective_ == model._status[best, 3] == np.min(model._status[:, 3]) and model.n_iter_ == ys[best]['n_iter']
    assert np.array_equal(model.labels_, ys[best]['labels'])
    assert max(rel(model._centers_shifted, ys[best]['V']), rel(model.objectives_, ys[best]['J'])) <= fit_rtol(case)
    init = initial_centers(case, 3)
    for r in range(3):
        # alone, and with max_iter cut at its own n_iter_: the same bytes -- a done restart is frozen while the others continue
        for max_iter in (MAX_ITER, ys[r]['n_iter']):
            solo = FuzzyCMeans(K, m=m, max_iter=max_iter, centers_init=init[r:r + 1]).fit(device_points(case))
            assert model._all_centers[r].tobytes() == solo._all_centers[0].tobytes()
            assert model._all_objectives[r, :ys[r]['n_iter']].tobytes() == solo._all_objectives[0, :ys[r]['n_iter']].tobytes()
            assert solo.converged_ and solo.n_iter_ == ys[r]['n_iter']
    shortest = int(np.argmin([y['n_iter'] for y in ys]))
    assert np.all(np.isnan(model._all_objectives[shortest, ys[shortest]['n_iter']:MAX_ITER]))


def test_a_single_iteration_does_not_converge_and_ties_go_to_the_first():
    one = _model('n1030_k4', max_iter=1).fit(device_points('n1030_k4'))
    assert one.converged_ is False and one.n_iter_ == 1 and len(one.objectives_) == 1
    assert one.objectives_[0] == device_fit('n1030_k4')[0].objectives_[0]
    init = initial_centers('n1030_k4', 3)
    twice = FuzzyCMeans(4, n_init=2, centers_init=np.stack([init[1], init[1]])).fit(device_points('n1030_k4'))
    assert twice._status[0, 3] == twice._status[1, 3] and twice._all_centers[0].tobytes() == twice._all_centers[1].tobytes()
    assert twice._centers_shifted.tobytes() == twice._all_centers[0].tobytes()


@pytest.mark.parametrize('case,held', [('n1030_k4', lambda: blobs(333, 8, 6)), ('overlap_k4_m1.2', lambda: blobs(517, 8, 11, n_centers=4, spread=1.2)),
                                       ('n257_d256_k5', lambda: blobs(131, 256, 5)), ('d13', lambda: blobs(77, 13, 15)),
                                       ('n1030_k4_m1.05', lambda: blobs(333, 8, 6))])
def test_predict_memberships_and_transform_on_held_out_points(case, held):
    _, K, m = CASES[case]
    model, _ = device_fit(case)
    H = held()
    d2, u, _, _ = y_memberships(H.astype(np.float64) - model._shift, model._centers_shifted, m)
    top = np.sort(u, axis=1)
    decided = top[:, -1] - top[:, -2] > 1e-9
    pred, got_u, dist = model.predict(H), model.memberships(torch.as_tensor(H, device='cuda')), model.transform(H)
    assert pred.shape == (len(H),) and pred.dtype == np.int32 and got_u.shape == dist.shape == (len(H), K) and got_u.dtype == dist.dtype == np.float64
    assert decided.mean() > 0.98 and np.array_equal(pred[decided], u.argmax(axis=1)[decided])
    assert np.array_equal(pred[decided], got_u.argmax(axis=1)[decided])
    assert np.max(np.abs(got_u.sum(axis=1) - 1.0)) <= 1e-12
    B = u_bound(H.shape[1], m)
    print(case, 'held out: largest |u - u\'|', float(np.max(np.abs(got_u - u))), 'bound', B)
    assert np.max(np.abs(got_u - u)) <= B
    assert np.max(np.abs(dist - np.sqrt(d2)) / np.sqrt(d2)) <= 2.0 * (H.shape[1] + 16) * EPS
    assert np.array_equal(model.predict_proba(H), got_u)
    with pytest.raises(ValueError, match='expecting %d features' % H.shape[1]):
        model.predict(H[:, :-1])


@pytest.mark.parametrize('case', list(COLLAPSE))
def test_a_collapsed_fit_says_so(case):
    _, K, m = COLLAPSE[case]
    y = yardstick(case)
    with pytest.warns(UserWarning, match='choose a smaller m') as rec:
        model = _model(case).fit(device_points(case))
    assert model.coincident_centers_ and all(0 <= j < k < K for j, k in model.coincident_centers_)
    assert any(all(str(pair) in str(w.message) for pair in model.coincident_centers_) for w in rec)
    limit = F.COINCIDENT_FRACTION * np.sqrt((y['Xs'] ** 2).sum() / len(y['Xs']))
    assert all(model.center_separation_[j, k] < limit for j, k in model.coincident_centers_)
    # the centres are ill-conditioned here (1e-9 between the two orders of summation on the CPU): only J, PC and PE are compared
    pc, pe, _ = indices(y, K)
    dev = {'J': rel(model.objectives_[:min(model.n_iter_, y['n_iter'])], y['J'][:min(model.n_iter_, y['n_iter'])]),
           'PC': abs(model.partition_coefficient_ - pc) / pc, 'PE': abs(model.partition_entropy_ - pe) / pe}
    print(case, 'collapsed: n_iter', model.n_iter_, 'yardstick', y['n_iter'], 'coincident', model.coincident_centers_, 'relative deviations', dev)
    assert model.n_iter_ == y['n_iter'] and model.converged_ == y['converged']
    assert max(dev.values()) <= fit_rtol(case)
    if case == 'collapse_d256_k6':
        assert len(model.coincident_centers_) == K * (K - 1) // 2 and abs(model.partition_coefficient_ - 1.0 / K) < 1e-4
        assert abs(model.modified_partition_coefficient_) < 1e-3


def test_the_smaller_fuzzifier_does_not_warn():
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        model = _model('overlap_k4_m1.2').fit(device_points('overlap_k4_m1.2'))
    assert model.coincident_centers_ == [] and model.partition_coefficient_ > 0.8


@pytest.mark.parametrize('case', ['n1030_k4', 'overlap_k4_m1.2', 'collapse_k4'])
def test_the_indices_equal_their_formulas(case):
    _, K, m = ALL[case]
    model, _ = device_fit(case)
    X = device_points(case)
    u, d = model.memberships(X), model.transform(X)
    n = len(u)
    pc = (u * u).sum() / n
    pe = -(u * np.log(np.where(u > 0, u, 1.0))).sum() / n
    assert abs(model.partition_coefficient_ - pc) <= 1e-13 * pc and abs(model.partition_entropy_ - pe) <= 1e-13 * max(pe, 1.0)
    assert model.modified_partition_coefficient_ == (K * model.partition_coefficient_ - 1.0) / (K - 1.0)
    sep = np.sqrt(((model.cluster_centers_[:, None, :] - model.cluster_centers_[None, :, :]) ** 2).sum(axis=2))
    np.testing.assert_allclose(model.center_separation_, sep, rtol=1e-9, atol=1e-12 * np.abs(model.cluster_centers_).max())
    assert np.array_equal(model.center_separation_, model.center_separation_.T) and np.all(np.diag(model.center_separation_) == 0)
    closest = model.center_separation_[~np.eye(K, dtype=bool)].min()
    xb = ((u ** m) * d * d).sum() / (n * closest * closest)
    assert abs(model.xie_beni_ - xb) <= 1e-12 * xb
    labels = np.unique(model.predict(X), return_inverse=True)[1]
    s = cluster_stats.silhouette_samples(X, labels).double().cpu().numpy()
    top = np.sort(u, axis=1)
    for alpha in (1.0, 2.0):
        weight = (top[:, -1] - top[:, -2]) ** alpha
        fs = (weight * s).sum() / weight.sum()
        assert abs(model.fuzzy_silhouette(X, alpha=alpha) - fs) <= 1e-12
    assert -1.0 <= model.fuzzy_silhouette(X) <= 1.0
    hard = float(s.mean())
    print(case, 'PC', pc, 'PE', pe, 'XB', xb, 'fuzzy silhouette', model.fuzzy_silhouette(X), 'crisp', hard)


def test_equal_centres_give_an_infinite_xie_beni():
    X = device_points('n1030_k4')
    init = initial_centers('n1030_k4')
    init = np.stack([init[0, 0], init[0, 0], init[0, 1]])[None]
    with pytest.warns(UserWarning, match=r'\(0, 1\)'):
        model = FuzzyCMeans(3, centers_init=init).fit(X)
    assert model.xie_beni_ == float('inf') and model.coincident_centers_ == [(0, 1)] and model.center_separation_[0, 1] == 0
    assert np.array_equal(model.cluster_centers_[0], model.cluster_centers_[1])
    re = FuzzyCMeans(3, centers_init=init)
    with pytest.warns(UserWarning):
        re.fit(X).reorder([2, 0, 1])
    assert re.coincident_centers_ == [(1, 2)] and np.array_equal(re.cluster_centers_, model.cluster_centers_[[2, 0, 1]])
    assert np.array_equal(re.predict(X), re.labels_) and np.array_equal(re.center_separation_, model.center_separation_[np.ix_([2, 0, 1], [2, 0, 1])])
    assert np.max(np.abs(re.memberships(X) - model.memberships(X)[:, [2, 0, 1]])) <= 1e-15          # (sum_k is a tree over the lanes: its order moved)
    with pytest.raises(ValueError, match='permutation'):
        re.reorder([0, 0, 1])


@pytest.mark.parametrize('init', ['k-means++', 'kmeans', 'random'])
def test_the_initialisations_and_the_sweep(init):
    """Every draw comes from one stream, so a seeded fit is repeatable and two restarts differ; the sweep gives the fits of its Ks."""
    X = device_points('overlap_k4_m1.2')
    a = FuzzyCMeans(4, m=1.2, init=init, n_init=2, random_state=3).fit(X)
    b = FuzzyCMeans(4, m=1.2, init=init, n_init=2, random_state=np.random.RandomState(3)).fit(X)
    same_bytes(a, b)
    assert not np.array_equal(a._initial_centers[0], a._initial_centers[1]) and np.isfinite(a.objective_) and a.objective_ == np.min(a._status[:, 3])
    if init != 'kmeans':          # the initial centres are rows of the points
        rows = np.array(points('overlap_k4_m1.2')).astype(np.float64) - a._shift
        assert all((np.abs(rows - c).max(axis=1) == 0).any() for c in a._initial_centers.reshape(-1, 8))
    sweep = fcm_sweep(X, [2, 4], m=1.2, init=init, n_init=2, random_state=3)
    assert sorted(sweep) == [2, 4] and sweep[2].cluster_centers_.shape == (2, 8) and np.array_equal(a.fit_predict(X), a.labels_)
    given = FuzzyCMeans(4, m=1.2, n_init=5, init=a.cluster_centers_).fit(X)          # given centres: one restart
    assert given._status.shape[0] == 1 and rel(given.cluster_centers_, a.cluster_centers_) < 1e-2
    with pytest.raises(ValueError, match='init should have the shape'):
        FuzzyCMeans(3, init=a.cluster_centers_).fit(X)
    with pytest.raises(ValueError, match='n_samples >= n_clusters'):
        FuzzyCMeans(5).fit(X[:4])


def test_a_workspace_that_does_not_fit_raises_memory_error(monkeypatch):
    X = np.array(points('n255_k3'))
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (1000, 1 << 30))
    with pytest.raises(MemoryError, match=r'255 points needs (\d+) bytes on the device, 1000 are free') as err:
        FuzzyCMeans(3).fit(X)
    assert int(str(err.value).split('needs ')[1].split(' bytes')[0]) >= 16 * 8 * (3 * 65 + 3)


def test_p2_fcm_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'fcm', '--k_max', '3', '--n_init', '2', '--fcm_m', '1.2', '2'])
    args.restore_metric = ['ae_mse']
    np.random.seed(123)
    res = p2.main(args)
    X, V = data['training']['hidden'], data['validation']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_fcm_aligned' / 'plot'
    table, labels, centers = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Fcm.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(table.columns) == ['m', 'k', 'objective', 'partition_coefficient', 'modified_partition_coefficient', 'partition_entropy', 'xie_beni',
                                   'fuzzy_silhouette', 'n_iter', 'converged', 'n_coincident', 'valid_partition_coefficient'] + metrics
    assert table.m.tolist() == [1.2, 1.2, 2.0, 2.0] and table.k.tolist() == [2, 3, 2, 3]
    assert list(labels.columns) == ['m1.2_k2', 'm1.2_k3', 'm2_k2', 'm2_k3'] and len(labels) == len(X)
    assert all(np.issubdtype(labels[c].to_numpy().dtype, np.integer) for c in labels.columns)
    assert list(centers.columns) == ['m', 'k', 'cluster'] + ['x%d' % c for c in range(16)] and len(centers) == 2 * (2 + 3)
    assert np.all(np.isfinite(table[['objective', 'partition_coefficient', 'partition_entropy', 'valid_partition_coefficient']].to_numpy()))
    assert np.all(table.n_iter >= 2) and np.all((table.partition_coefficient > 1.0 / table.k - 1e-12) & (table.partition_coefficient <= 1.0))
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy(), equal_nan=True)
    # a second run finds the files and does not recompute; overwrite=True does, and its rows equal direct calls
    fc = p2.Fcm(3, str(plot.parent), metrics, n_init=2, ms=[1.2, 2.0])
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Fcm.FILES]
    calls = []
    real = p2.fcm_sweep
    monkeypatch.setattr(p2, 'fcm_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = fc.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Fcm.FILES] == stamps and fc.fits_ is None
    assert np.array_equal(again.to_numpy(), table.to_numpy(), equal_nan=True)
    redo = fc.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1, 1] and sorted(fc.fits_) == [(1.2, 2), (1.2, 3), (2.0, 2), (2.0, 3)] and list(redo.columns) == list(table.columns)
    written = pd.read_csv(plot / 'fcm_labels.csv')
    for row, (m, k) in enumerate(sorted(fc.fits_)):
        fit = fc.fits_[(m, k)]
        u = fit.memberships(V)
        assert redo.valid_partition_coefficient[row] == float((u * u).sum() / len(u)) and redo.objective[row] == fit.objective_
        assert redo.partition_coefficient[row] == fit.partition_coefficient_ and redo.xie_beni[row] == fit.xie_beni_
        assert redo.fuzzy_silhouette[row] == fit.fuzzy_silhouette(X) and redo.n_coincident[row] == len(fit.coincident_centers_)
        lab = written[p2.Fcm.column(m, k)].to_numpy()
        assert np.array_equal(lab, fit.labels_) and np.array_equal(lab, fit.predict(X)) and set(lab.tolist()) <= set(range(k))
        lab = np.unique(lab, return_inverse=True)[1]
        direct = [cluster_stats.silhouette_score(X, lab), cluster_stats.davies_bouldin_score(X, lab), cluster_stats.calinski_harabasz_score(X, lab)]
        np.testing.assert_allclose(redo[metrics].to_numpy()[row], direct, rtol=1e-12, atol=0)


def test_p4_fcm_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.FuzzyCMeans):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'FuzzyCMeans', Recording)
    args = p4.get_arguments(['--cluster_method', 'fcm', '--num_clusters', '3', '--fcm_m', '1.2'])
    args.restore_metric = ['ae_mse']
    np.random.seed(123)
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_fcm_aligned'
    saved = {cohort: np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1
    model = made[0]
    assert model.m == 1.2 and model.n_clusters == 3 and model.coincident_centers_ == []
    for cohort in COHORTS:
        s = saved[cohort]
        assert sorted(s) == ['cluster_id', 'cluster_prob', 'encounter_id', 'fcm_m', 'hidden'] and len(s['cluster_id']) == len(data[cohort]['hidden'])
        prob = s['cluster_prob']
        assert s['fcm_m'] == 1.2 and np.issubdtype(np.asarray(s['cluster_id']).dtype, np.integer)
        assert prob.dtype == np.float32 and prob.shape == (len(s['cluster_id']), 3) and np.max(np.abs(prob.sum(axis=1) - 1.0)) < 1e-6
        # every cohort is labelled by the one training model, in its aligned order
        assert np.array_equal(s['cluster_id'], model.predict(data[cohort]['hidden']))
        assert np.array_equal(prob, model.predict_proba(data[cohort]['hidden']).astype(np.float32))
    ids = np.asarray(saved['training']['cluster_id'])
    sbp = data['training']['ob'][:, 0, :].mean(1)
    means = [sbp[ids == i].mean() for i in range(3)]
    assert means[0] > means[1] > means[2]
    assert model.cluster_centers_.shape == (3, 16) and model.converged_
    # an existing result is left alone
    stamps = [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
    with pytest.raises(ValueError, match='--transfer knn applies to'):          # a centre-based method labels every cohort with its training model already
        a = p4.get_arguments(['--cluster_method', 'fcm', '--num_clusters', '3', '--transfer', 'knn'])
        a.restore_metric = ['ae_mse']
        p4.main(a)
