"""Full- and tied-covariance Gaussian mixtures on the GPU (csrc/dic_gmm_full.hip, gmm_full.py, the p2 / p4 branches) against the numpy f64 yardstick of
tests/test_gmm_full_host.py and sklearn.

The cases are those of test_gmm_full_host.py (CASES): seven fits of several iterations at 8 to 256 features, and the smallest at which a tile kernel can still go
wrong -- one workgroup (2 rows), a ragged 16-row tile (17), 255 / 257 rows, D0 = 13 (padded to 16), D = 4, D = 200 (predicated up to 208), K = 32, duplicated
rows and a strided view.  The host file shows on the CPU that every stopping decision and label of every case is clear, so n_iter_, converged_ and the labels
are held to equality; every array is held to fit_rtol(case) = 16 x the largest CPU-side deviation of BASE, never less than 1e-13, as max |a - b| / max |b|."""
import functools
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import gmm_full as GF
from deep_interpolation_clustering_amd.gmm import _Points
from deep_interpolation_clustering_amd.gmm_full import FullGaussianMixture, gmm_full_sweep
from deep_interpolation_clustering_amd.info import COHORTS
from test_gmm_full_host import (BASE, BLURRED, CASES, N_INIT_CASES, REG, TOL, blurred, corr_blobs, cov_of, fit_rtol, initial_labels, mild, points, slabs, winner,
                                y_estep, y_factor, y_factor_columns, y_mstep, yardstick)
from test_gmm_host import blobs, one_hot
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
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


def rel(a, b):
    """test_gmm_host.rel with 0 / 0 = 0 (the shifted mean of a single component is exactly 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(np.float64).tiny))


def factor_devs(case, C, P, ld):
    """The device's factor (numpy (Kc, d0, d0), (Kc, d0, d0), (Kc)) against LAPACK's on the device's own covariances, and the bound: 16 x (c), never less than
    1e-13.  (Against the yardstick's P and log_det the case tolerance holds, as for every other array: BASE measures the factors' answer to a change of C.)"""
    Pl, ldl = y_factor(C)
    return {'P | own C': rel(P, Pl), 'log_det | own C': float(np.max(np.abs(ld - ldl) / np.maximum(np.abs(ldl), 1.0)))}, max(16.0 * BASE[case][2], 1e-13)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def padded_vectors(a, d):
    out = torch.zeros(a.shape[:-1] + (d,), dtype=torch.float64, device='cuda')
    out[..., :a.shape[-1]] = dev(a)
    return out.contiguous()


def padded_squares(a, d):
    return GF._pad_square(a, d, 'cuda').contiguous()


def check_padding(t, d0):
    """(.., D, D) on the device: the identity outside the leading d0 x d0 block."""
    D = t.shape[-1]
    if D > d0:
        eye = torch.eye(D, dtype=torch.float64, device=t.device)
        assert torch.equal(t[..., d0:, :], eye[d0:, :].expand_as(t[..., d0:, :])) and torch.equal(t[..., :, d0:], eye[:, d0:].expand_as(t[..., :, d0:]))


def fit_from_labels(case, n_init=1, **kw):
    """(points, the fit of ``n_init`` restarts from the host file's initial labels); the device does the initial M-step itself."""
    _, K, cov = CASES[case]
    pts = _Points(device_points(case))
    model = FullGaussianMixture(K, covariance_type=cov, tol=TOL, reg_covar=REG, n_init=n_init, **kw)
    return pts, model._fit_points(pts, init_labels=initial_labels(case, n_init))


@functools.lru_cache(maxsize=None)
def device_fit(case):
    x = device_points(case)
    keep = x.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        model = fit_from_labels(case)[1]
    assert not [c for c in caught if 'did not converge' in str(c.message)]
    assert torch.equal(x, keep) or case == 'strided'          # the input is only read (the strided buffer holds NaN, which never equals itself)
    return model


@pytest.mark.parametrize('case', list(CASES))
def test_one_em_pass(case):
    _, K, cov = CASES[case]
    ct = GF.COV_TYPES[cov]
    y = yardstick(case)
    n, d0 = points(case).shape
    tol = fit_rtol(case)
    pts = _Points(device_points(case), shift=y['c'])
    labels0 = torch.as_tensor(initial_labels(case).astype(np.int32), device='cuda')
    status = GF.new_status(1, TOL, 1, 'cuda')
    par = GF.mstep(pts, K, ct, REG, labels=labels0, status=status)
    w0, mu0, C0, P0, ld0 = y['init']
    got = lambda name: par[name][0, :, :d0, :d0].cpu().numpy()
    init = {'weights': rel(par['w'][0].cpu().numpy(), w0), 'means': rel(par['mu'][0, :, :d0].cpu().numpy(), mu0), 'covariances': rel(got('cov'), C0),
            'P': rel(got('P'), P0), 'log_det': rel(par['log_det'][0].cpu().numpy(), ld0)}
    init_f, tol_f = factor_devs(case, got('cov'), got('P'), par['log_det'][0].cpu().numpy())
    # the E-step from the yardstick's own initial parameters
    M, logp, lse, logr, (w1, mu1, C1, P1, ld1, nk1) = y['first']
    e = GF.estep(pts, ct, dev(w0), padded_vectors(mu0, pts.d), padded_squares(P0, pts.d), dev(ld0), lse=True, log_resp=True, labels=True, total=True)
    est = {'lse': rel(e['lse'].cpu().numpy(), lse), 'log r': rel(e['log_resp'].cpu().numpy(), logr),
           'total': abs(float(e['total'][0]) - lse.sum()) / abs(lse.sum())}
    assert np.array_equal(e['labels'].cpu().numpy(), logp.argmax(axis=1))
    # one EM iteration from the device's initial parameters
    st, lbs = GF.em(pts, ct, REG, par, status, 1)
    assert st[0, 0] == 1 and st[0, 1] == 1 and st[0, 2] == 0 and st[0, 7] == 0 and lbs.shape == (1, 1) and st[0, 3] == lbs[0, 0]
    C, P = par['cov'][0], par['P'][0]
    first = {'lower bound': abs(lbs[0, 0] - lse.mean()) / abs(lse.mean()), 'weights': rel(par['w'][0].cpu().numpy(), w1),
             'means': rel(par['mu'][0, :, :d0].cpu().numpy(), mu1), 'covariances': rel(got('cov'), C1), 'P': rel(got('P'), P1),
             'log_det': rel(par['log_det'][0].cpu().numpy(), ld1)}
    first_f, _ = factor_devs(case, got('cov'), got('P'), par['log_det'][0].cpu().numpy())
    print(case, 'allowed', tol, 'initial M-step', init, 'E-step', est, 'first iteration', first, '| factors of the device\'s own C: allowed', tol_f, init_f, first_f)
    assert max(init.values()) <= tol and max(est.values()) <= tol and max(first.values()) <= tol
    assert max(init_f.values()) <= tol_f and max(first_f.values()) <= tol_f
    assert torch.equal(C, C.transpose(-1, -2))          # bit-symmetric
    assert torch.equal(P, torch.triu(P))          # exactly 0 below the diagonal
    check_padding(C, d0)
    check_padding(P, d0)
    assert torch.all(par['mu'][0, :, d0:] == 0)


@pytest.mark.parametrize('case', BLURRED)
def test_estep_alone_from_blurred_parameters(case):
    """Separated clusters at D = 256 / 64 leave no row soft; parameters blurred to the pooled covariance do (the host file asserts more than 2 %)."""
    _, K, cov = CASES[case]
    y = yardstick(case)
    pts = _Points(device_points(case), shift=y['c'])
    w, mu, P, ld = blurred(case)
    _, logp, lse, logr = y_estep(y['Xs'], w, mu, P, ld)
    e = GF.estep(pts, 2, dev(w), padded_vectors(mu, pts.d), padded_squares(P, pts.d), dev(ld), lse=True, log_resp=True, labels=True)
    got = e['log_resp'].cpu().numpy()
    devs = {'lse': rel(e['lse'].cpu().numpy(), lse), 'log r': rel(got, logr),
            'r': float(np.max(np.abs(np.exp(got) - np.exp(logr))))}
    print(case, 'blurred E-step', devs, 'allowed', fit_rtol(case))
    assert max(devs.values()) <= fit_rtol(case)
    top = np.sort(logp, axis=1)
    decided = top[:, -1] - top[:, -2] > 1e-4
    assert np.array_equal(e['labels'].cpu().numpy()[decided], logp.argmax(axis=1)[decided])


def sum_bound(n):
    """A sum of n f64 terms in any order deviates from another order by at most (n + 16) 2^-52 times the sum of the absolute values (to first order)."""
    return (n + 16) * 2.0 ** -52


@pytest.mark.parametrize('n,d', [(255, 8), (257, 8), (4100, 8), (257, 256)])
def test_scatter_alone(n, d):
    """The scatter and reduce kernels through the M-step from given responsibilities, K = 3: component 1 owns exactly the first and the last row of every
    slab, component 2 is empty, component 0 has the rest; then random responsibilities; then T, the call with every weight 1."""
    X = blobs(n, d, 21, n_centers=3, spread=2.0)
    pts = _Points(torch.as_tensor(X, device='cuda'))
    Xs = X.astype(np.float64) - pts.shift_host
    K, S = 3, slabs(n, 3)
    rows = ((n + S - 1) // S + 3) // 4 * 4
    edge = sorted({i for s in range(S) for i in (s * rows, min(n, (s + 1) * rows) - 1) if s * rows < n})
    assert (n > 256) == (S > 1)
    lab = np.zeros(n, dtype=np.int32)
    lab[edge] = 1
    rs = np.random.RandomState(n + d)
    u = rs.uniform(size=(n, K)) ** 4
    for name, r, kw in (('one-hot', one_hot(lab, K), {'labels': torch.as_tensor(lab[None], device='cuda')}),
                        ('random', u / u.sum(axis=1)[:, None], None)):
        kw = kw or {'resp': torch.as_tensor(r[None], device='cuda')}
        par = GF.mstep(pts, K, 2, REG, **kw)
        w, mu, C, nk = y_mstep(Xs, r, 'full')
        got = par['cov'][0].cpu().numpy()
        # S / n_k: the sum's bound twice (S and n_k); mu' mu'^T: each mean's bound times the other mean
        b_mu = sum_bound(n) * 2.0 * (r.T @ np.abs(Xs)) / nk[:, None]
        bound = 2.0 * sum_bound(n) * np.einsum('nk,ni,nj->kij', r, np.abs(Xs), np.abs(Xs)) / nk[:, None, None]
        bound = bound + np.abs(mu)[:, :, None] * b_mu[:, None, :] + b_mu[:, :, None] * np.abs(mu)[:, None, :] + 4 * EPS * np.abs(C)
        ratio = np.max(np.abs(got - C) / (bound + 1e-300))
        print(n, d, name, 'slabs', S, 'largest deviation / bound', ratio)
        assert ratio <= 1.0 and np.array_equal(got, np.swapaxes(got, -1, -2))
        assert rel(par['mu'][0].cpu().numpy(), mu) <= 1e-13 and rel(par['w'][0].cpu().numpy(), w) <= 1e-13
        if name == 'one-hot':          # the exactly empty component: S = 0, n_k = 10 * 2^-52, C = reg_covar I
            assert np.array_equal(got[2], REG * np.eye(d)) and float(par['w'][0, 2]) < 1e-15
            assert par['status'][0, 7] == 0 and np.allclose(par['P'][0, 2].cpu().numpy(), np.eye(d) / np.sqrt(REG), rtol=1e-14)
    tied = GF.mstep(pts, K, 3, REG, labels=torch.as_tensor(lab[None], device='cuda'))
    T = tied['total'].cpu().numpy()
    ratio = np.max(np.abs(T - Xs.T @ Xs) / (sum_bound(n) * (np.abs(Xs).T @ np.abs(Xs))))
    print(n, d, 'T: slabs', slabs(n, 1), 'largest deviation / bound', ratio)
    assert ratio <= 1.0 and np.array_equal(T, T.T)
    C = y_mstep(Xs, one_hot(lab, K), 'tied')[2]
    assert rel(tied['cov'][0].cpu().numpy(), C) <= 1e-12
    again = GF.mstep(pts, K, 3, REG, labels=torch.as_tensor(lab[None], device='cuda'), total=tied['total'], compute_total=False)          # T only read
    assert torch.equal(again['cov'], tied['cov']) and torch.equal(again['P'], tied['P'])


def random_spd(d, cond, seed):
    rs = np.random.RandomState(seed)
    Q = np.linalg.qr(rs.normal(size=(d, d)))[0]
    C = (Q * np.logspace(0.0, -np.log10(cond), d)) @ Q.T
    return 0.5 * (C + C.T)


@pytest.mark.parametrize('d0', [4, 12, 13, 64, 200, 256])
def test_factor_alone(d0):
    """Random SPD matrices, cond 10, 1e3 and 1e6, against LAPACK within 16 x the deviation of the header's column order from LAPACK, measured here on the CPU."""
    D = (d0 + 3) // 4 * 4
    Cs = np.stack([random_spd(d0, cond, 100 + d0 + i) for i, cond in enumerate((10.0, 1e3, 1e6))])
    P, ld, status = GF.factor(padded_squares(Cs, D)[None], d0)
    assert torch.all(status[:, 7] == 0) and torch.equal(P, torch.triu(P))
    check_padding(P, d0)
    Pl, ldl = y_factor(Cs)
    for i in range(3):
        Pc, ldc = y_factor_columns(Cs[i])
        c = max(rel(Pc, Pl[i]), abs(ldc - ldl[i]) / max(abs(ldl[i]), 1.0))
        got = P[0, i, :d0, :d0].cpu().numpy()
        devs = (rel(got, Pl[i]), abs(float(ld[0, i]) - ldl[i]) / max(abs(ldl[i]), 1.0))
        print('D0', d0, 'matrix', i, 'column order vs LAPACK', c, 'device vs LAPACK', devs, 'entries that differ from the column order', int((got != Pc).sum()))
        assert max(devs) <= max(16.0 * c, 1e-13)
        assert np.array_equal(got, Pc)          # the header's order, bit for bit (products and differences rounded separately, IEEE sqrt and division)


def test_a_zero_pivot_sets_the_flag_and_the_restart_beside_it_completes():
    good = random_spd(8, 100.0, 3)
    C = np.stack([np.zeros((8, 8)), good, np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0]), good])[:, None]          # 4 restarts of one matrix
    C[2, 0, 3, 3] = np.nan
    P, ld, status = GF.factor(dev(C), 8)
    assert status[:, 7].tolist() == [1.0, 0.0, 1.0, 0.0] and status[:, 0].tolist() == [1.0, 0.0, 1.0, 0.0]
    assert torch.isfinite(P).all() and torch.isfinite(ld).all() and torch.equal(P[1], P[3])
    assert rel(P[1, 0].cpu().numpy(), y_factor(good)[0]) <= 1e-13
    X = np.tile(blobs(1, 4, 9), (131, 1))
    with pytest.raises(ValueError, match='Fitting the mixture model failed because some components have ill-defined empirical covariance'):
        FullGaussianMixture(1, reg_covar=0.0).fit(X)
    with pytest.raises(ValueError, match='ill-defined empirical covariance'):
        FullGaussianMixture(1, covariance_type='tied', reg_covar=0.0, n_init=2).fit(X)
    assert FullGaussianMixture(1).fit(X).converged_          # (reg_covar holds it up)


@pytest.mark.parametrize('case', list(CASES))
def test_whole_fit_equals_the_yardstick(case):
    _, K, cov = CASES[case]
    y = yardstick(case)
    m = device_fit(case)
    d0 = points(case).shape[1]
    assert m.n_iter_ == y['n_iter'] and m.converged_ is True and y['converged']
    assert m.labels_.dtype == np.int32 and np.array_equal(m.labels_, y['labels'])
    w, mu, C, P, ld = y['final']
    devs = {'lower_bounds': rel(m.lower_bounds_, y['lbs']), 'weights': rel(m.weights_, w), 'means': rel(m.means_, mu + y['c']),
            'covariances': rel(m.covariances_, cov_of(C, cov)), 'precisions_cholesky': rel(m.precisions_cholesky_, cov_of(P, cov)),
            'log_det': rel(m._log_det, ld)}
    shaped = lambda a: a.reshape((-1, d0, d0))
    devs_f, tol_f = factor_devs(case, shaped(m.covariances_), shaped(m.precisions_cholesky_), m._log_det)
    print(case, 'whole fit: n_iter', m.n_iter_, 'relative deviations', devs, 'allowed', fit_rtol(case), '| factor of its own covariances', devs_f, 'allowed', tol_f)
    assert max(devs.values()) <= fit_rtol(case) and max(devs_f.values()) <= tol_f
    assert m.lower_bound_ == m.lower_bounds_[-1] and m.n_features_in_ == d0
    shape = (K, d0, d0) if cov == 'full' else (d0, d0)
    assert m.covariances_.shape == m.precisions_.shape == m.precisions_cholesky_.shape == shape and m.means_.shape == (K, d0)
    for name in ATTRS[:6]:
        assert getattr(m, name).dtype == np.float64
    assert np.allclose(m.precisions_ @ m.covariances_, np.eye(d0), atol=1e-6 * np.linalg.cond(cov_of(C, cov)).max())
    assert m._n_parameters() == GF.n_parameters(K, d0, cov)


@pytest.mark.parametrize('case', ['full_d64_k3', 'tied_corr_k4', 'n257_d13_k3', 'strided', 'd200_k2'])
def test_two_calls_and_every_input_form_give_identical_bits(case):
    m = device_fit(case)
    again = fit_from_labels(case)[1]
    _, K, cov = CASES[case]
    host = FullGaussianMixture(K, covariance_type=cov)._fit_points(_Points(np.array(points(case))), init_labels=initial_labels(case))
    for name in ATTRS:
        assert getattr(m, name).tobytes() == getattr(again, name).tobytes() == getattr(host, name).tobytes(), name
    assert m.n_iter_ == again.n_iter_ == host.n_iter_
    if case == 'strided':          # read where it lies
        view = device_points(case)
        assert _Points(view).x.data_ptr() == view.data_ptr() and torch.isnan(view._base[:, :4]).all() and torch.isnan(view._base[:, 12:]).all()


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_pick_the_winner_and_do_not_depend_on_each_other(case):
    _, K, cov = CASES[case]
    pts, m = fit_from_labels(case, n_init=3)
    ys = [yardstick(case, r, 3) for r in range(3)]
    best = winner(case)
    assert [int(v) for v in m._status[:, 1]] == [y['n_iter'] for y in ys] and np.all(m._status[:, 0] == 1) and np.all(m._status[:, 2] == 1)
    assert m.lower_bound_ == m._status[best, 3] == np.max(m._status[:, 3]) and m.n_iter_ == ys[best]['n_iter']
    assert np.array_equal(m.labels_, ys[best]['labels'])
    w, mu, C = ys[best]['final'][:3]
    assert max(rel(m.weights_, w), rel(m.means_, mu + ys[best]['c']), rel(m.covariances_, cov_of(C, cov)), rel(m.lower_bounds_, ys[best]['lbs'])) <= fit_rtol(case)
    for r in range(3):          # alone: the same bytes -- a done restart is frozen while the others continue
        solo = FullGaussianMixture(K, covariance_type=cov)._fit_points(pts, init_labels=initial_labels(case, 3)[r:r + 1])
        for name, part in m._all_parameters.items():
            assert part[r].tobytes() == solo._all_parameters[name][0].tobytes(), (r, name)
        assert m._all_lower_bounds[r, :ys[r]['n_iter']].tobytes() == solo._all_lower_bounds[0, :ys[r]['n_iter']].tobytes()
        assert solo.converged_ and solo.n_iter_ == ys[r]['n_iter']


@pytest.mark.parametrize('case,held', [('full_corr_k4', lambda: corr_blobs(517, 8, 11, 4, 1.2)), ('tied_d64_k4', lambda: mild(333, 64, 6, 4, 0.35, mix=0.0)),
                                       ('n257_d13_k3', lambda: blobs(77, 13, 15)), ('full_d256_k2', lambda: mild(131, 256, 14, 2, 0.10))])
def test_predict_and_scores_on_held_out_points_equal_sklearn(case, held):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov = CASES[case]
    m = device_fit(case)
    H = held()
    sk = mix.GaussianMixture(K, covariance_type=cov)
    sk.weights_, sk.means_, sk.covariances_, sk.precisions_cholesky_ = m.weights_, m.means_, m.covariances_, m.precisions_cholesky_
    H64 = H.astype(np.float64)
    want_scores, want_proba = sk.score_samples(H64), sk.predict_proba(H64)
    logp = sk._estimate_weighted_log_prob(H64)
    top = np.sort(logp, axis=1)
    decided = (top[:, -1] - top[:, -2]) > 1e-4 if K > 1 else np.ones(len(H), bool)
    pred, proba, scores, score = m.predict(H), m.predict_proba(torch.as_tensor(H, device='cuda')), m.score_samples(H), m.score(H)
    assert pred.shape == (len(H),) and proba.shape == (len(H), K) and proba.dtype == np.float64 and scores.dtype == np.float64
    assert decided.mean() > 0.98 and np.array_equal(pred[decided], sk.predict(H64)[decided])
    tol = fit_rtol(case)
    devs = (rel(scores, want_scores), float(np.max(np.abs(proba - want_proba))), abs(score - want_scores.mean()) / abs(want_scores.mean()))
    print(case, 'held-out points against sklearn', devs, 'allowed', tol)
    assert max(devs) <= tol and np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 1e-12
    n = len(H)
    assert m.bic(H) == -2 * score * n + m._n_parameters() * np.log(n) and m.aic(H) == -2 * score * n + 2 * m._n_parameters()
    with pytest.raises(ValueError, match='expecting %d features' % H.shape[1]):
        m.predict(H[:, :-1])
    # reorder: the components renumbered, the model the same
    order = np.roll(np.arange(K), 1)
    before = {name: getattr(m, name).copy() for name in ATTRS[:5]}
    labels = m.labels_.copy()
    m.reorder(order)
    try:
        assert np.array_equal(m.weights_, before['weights_'][order]) and np.array_equal(m.means_, before['means_'][order])
        if cov == 'full':
            assert np.array_equal(m.covariances_, before['covariances_'][order]) and np.array_equal(m.precisions_cholesky_, before['precisions_cholesky_'][order])
        else:
            assert np.array_equal(m.covariances_, before['covariances_'])
        assert np.array_equal(order[m.labels_], labels) and np.array_equal(order[m.predict(H)][decided], pred[decided])
        assert np.allclose(m.predict_proba(H), proba[:, order], rtol=0, atol=tol) and abs(m.score(H) - score) <= tol * abs(score)          # (k is summed in its new order)
    finally:
        inverse = np.empty_like(order)
        inverse[order] = np.arange(K)
        m.reorder(inverse)
    assert all(np.array_equal(getattr(m, name), before[name]) for name in before) and np.array_equal(m.labels_, labels)


@pytest.mark.parametrize('cov', ['full', 'tied'])
def test_the_sweep_equals_the_single_fits_and_seeded_fits_repeat(cov):
    X = device_points('full_corr_k4')
    sweep = gmm_full_sweep(X, [2, 4], covariance_type=cov, n_init=2, random_state=3)
    assert sorted(sweep) == [2, 4]
    for k in (2, 4):
        single = FullGaussianMixture(k, covariance_type=cov, n_init=2, random_state=3).fit(X)
        for name in ATTRS:
            assert getattr(sweep[k], name).tobytes() == getattr(single, name).tobytes(), (k, name)
    assert sweep[2].bic(X) != sweep[4].bic(X) and abs(sweep[4].weights_.sum() - 1.0) < 1e-12
    for init in ('k-means++', 'random_from_data', 'random'):
        a = FullGaussianMixture(3, covariance_type=cov, init_params=init, random_state=3).fit(X)
        b = FullGaussianMixture(3, covariance_type=cov, init_params=init, random_state=np.random.RandomState(3)).fit(X)
        assert a.means_.tobytes() == b.means_.tobytes() and np.isfinite(a.lower_bound_)


def test_given_initial_parameters_equal_sklearn():
    mix = pytest.importorskip('sklearn.mixture')
    case = 'full_corr_k4'
    X = np.array(points(case))
    for cov in ('full', 'tied'):
        ref0 = mix.GaussianMixture(4, covariance_type=cov, random_state=1, max_iter=2).fit(X.astype(np.float64))
        kw = dict(weights_init=ref0.weights_, means_init=ref0.means_, precisions_init=ref0.precisions_)
        ours = FullGaussianMixture(4, covariance_type=cov, **kw).fit(X)
        ref = mix.GaussianMixture(4, covariance_type=cov, **kw).fit(X.astype(np.float64))
        assert ours.n_iter_ == ref.n_iter_ and np.array_equal(ours.labels_, ref.predict(X.astype(np.float64)))
        d = max(rel(ours.weights_, ref.weights_), rel(ours.means_, ref.means_), rel(ours.covariances_, ref.covariances_), rel(ours.lower_bounds_, ref.lower_bounds_))
        print(cov, 'from given parameters against sklearn', d)
        assert d <= fit_rtol({'full': 'full_corr_k4', 'tied': 'tied_corr_k4'}[cov])          # (the same points; the given precisions are factored directly)


def test_a_workspace_that_does_not_fit_raises_memory_error(monkeypatch):
    X = np.array(points('n257_d13_k3'))
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (1000, 1 << 30))
    with pytest.raises(MemoryError, match=r'257 points needs (\d+) bytes on the device, 1000 are free') as err:
        FullGaussianMixture(3).fit(X)
    assert int(str(err.value).split('needs ')[1].split(' bytes')[0]) >= 8 * 257 * 3 + 8 * 3 * 2 * 16 * 16


def test_p2_gmm_full_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'gmm', '--k_max', '3', '--n_init', '2', '--gmm_covariance_type', 'full'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X = data['training']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_gmm_aligned' / 'plot'
    table, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Gmm.FILES)
    assert table.k.tolist() == [2, 3] and list(labels.columns) == ['k2', 'k3'] and len(labels) == len(X)
    assert np.all(np.isfinite(table[['lower_bound', 'bic', 'aic', 'valid_score']].to_numpy())) and np.all(table.n_iter >= 1)
    n_par = np.array([k * 16 * 17 // 2 + k * 16 + k - 1 for k in (2, 3)])
    np.testing.assert_allclose(table.bic - table.aic, n_par * (np.log(len(X)) - 2.0), rtol=1e-9)
    assert np.array_equal(res['ae_mse'].to_numpy(), table.to_numpy(), equal_nan=True)
    for k in (2, 3):
        assert set(labels['k%d' % k].tolist()) <= set(range(k))
    gm = p2.Gmm(3, str(plot.parent), ['Sihouette'], n_init=1, covariance_type='tied')
    redo = gm.train(data['training'], data['validation'], overwrite=True)
    assert sorted(gm.fits_) == [2, 3] and gm.fits_[3].covariances_.shape == (16, 16) and list(redo.k) == [2, 3]


def test_p4_gmm_full_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.FullGaussianMixture):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'FullGaussianMixture', Recording)
    args = p4.get_arguments(['--cluster_method', 'gmm', '--num_clusters', '3', '--gmm_covariance_type', 'full'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_gmm_aligned'
    saved = {cohort: np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1 and made[0].covariance_type == 'full' and made[0].covariances_.shape == (3, 16, 16)
    model = made[0]
    for cohort in COHORTS:
        s = saved[cohort]
        prob = s['cluster_prob']
        assert sorted(s) == ['cluster_id', 'cluster_prob', 'encounter_id', 'hidden'] and prob.dtype == np.float32 and prob.shape == (len(s['cluster_id']), 3)
        assert np.max(np.abs(prob.sum(axis=1) - 1.0)) < 1e-6 and np.array_equal(s['cluster_id'], prob.argmax(axis=1))
        assert np.array_equal(s['cluster_id'], model.predict(data[cohort]['hidden']))
    ids = np.asarray(saved['training']['cluster_id'])
    sbp = data['training']['ob'][:, 0, :].mean(1)
    means = [sbp[ids == i].mean() for i in range(3)]
    assert means[0] > means[1] > means[2]
