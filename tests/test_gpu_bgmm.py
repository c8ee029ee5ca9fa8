"""Bayesian Gaussian mixtures on the device (csrc/dic_bgmm.hip, bgmm.py) against the numpy f64 yardstick of tests/test_bgmm_host.py: the special functions,
one pass, whole fits, determinism and the independence of the restarts, the estimator surface, live sklearn, the sweep and the p2 / p4 branches."""
import functools
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import bgmm as B
from deep_interpolation_clustering_amd.bgmm import BayesianGaussianMixture, bgmm_sweep
from deep_interpolation_clustering_amd.info import COHORTS
from test_bgmm_host import (CASES, DP, N_INIT_CASES, SCIPY_DIGAMMA_DEV, SCIPY_GAMMALN_DEV, Model, cov_of, fit_arrays, fit_rtol, initial_labels, points,
                            one_hot, ref_digamma, ref_gammaln, special_arguments, special_dev, winner, y_estep, y_lower_bound, yardstick)
from test_gmm_host import EPS, REG, TOL, blobs, rel
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

ATTRS = ('weights_', 'means_', 'covariances_', 'precisions_', 'precisions_cholesky_', 'mean_precision_', 'degrees_of_freedom_', 'lower_bounds_', 'labels_')
TINY = np.finfo(np.float64).tiny


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


def _model(case, **kw):
    _, K, cov, prior = CASES[case]
    return BayesianGaussianMixture(K, covariance_type=cov, tol=TOL, reg_covar=REG, weight_concentration_prior_type=prior, **kw)


def _fit(case, x, **kw):
    """The estimator fitted from the yardstick's initial labels."""
    return _model(case, **kw)._fit_points(B._Points(x), init_labels=initial_labels(case))


@functools.lru_cache(maxsize=None)
def device_fit(case):
    x = device_points(case)
    keep = x.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        model = _fit(case, x)
    assert not [c for c in caught if 'did not converge' in str(c.message)]          # (every case converges)
    assert torch.equal(x, keep)          # the input is only read
    return model


def log_bound(case, logp):
    """4 (D + 16) 2^-53 max(1, max |log p|): the same-sign-sum bound of a length-D f64 sum, taken on both sides and carried through the log-sum-exp."""
    d0 = points(case).shape[1]
    return 4.0 * (d0 + 16) * EPS * max(1.0, float(np.max(np.abs(logp))))


def test_special_functions():
    """The device psi and lgamma against the long-double references of the host test: 8 x what scipy's own functions show against them."""
    x = special_arguments()
    psi, lg = B.special_probe(x)
    dg, dl = special_dev(psi, ref_digamma(x)), special_dev(lg, ref_gammaln(x))
    print('device digamma', dg, 'allowed', 8 * SCIPY_DIGAMMA_DEV, 'device lgamma', dl, 'allowed', 8 * SCIPY_GAMMALN_DEV)
    assert dg <= 8 * SCIPY_DIGAMMA_DEV and dl <= 8 * SCIPY_GAMMALN_DEV
    assert np.isnan(B.special_probe(np.array([0.0, -1.5]))[0]).all()          # (positive arguments only)


@pytest.mark.parametrize('case', list(CASES))
def test_one_pass(case):
    from scipy.special import digamma, gammaln
    _, K, cov, prior = CASES[case]
    y = yardstick(case)
    n, d0 = points(case).shape
    pts = B._Points(device_points(case), shift=y['c'])
    p0 = y['init']
    mu, var = _padded(p0.m, pts.d, 0.0)[None].contiguous(), _padded(p0.v, pts.d, 1.0)[None].contiguous()
    comp = torch.zeros((1, B.COMP_WORDS, K), dtype=torch.float64, device='cuda')
    comp[0, B.C_LC] = torch.as_tensor(p0.lc, device='cuda')
    M, logp, lse, logr, p1, lb1 = y['first']
    Bd = log_bound(case, logp)
    e = B.estep(pts, comp[0, B.C_LC].contiguous(), mu[0], var[0], lse=True, log_resp=True, labels=True, total=True)
    got_lse, got_logr = e['lse'].cpu().numpy(), e['log_resp'].cpu().numpy()
    ratios = {'lse': np.max(np.abs(got_lse - lse)) / Bd, 'log r': np.max(np.abs(got_logr - logr)) / Bd}
    assert np.array_equal(e['labels'].cpu().numpy(), logp.argmax(axis=1))
    assert abs(float(e['total'][0]) - lse.sum()) <= (Bd + n * EPS) * np.abs(lse).sum()
    # the priors of the fit, formed on the device
    model = _model(case)
    pri = model._priors(pts)
    yp = y['priors']
    np.testing.assert_allclose(pri.s0[:d0].cpu().numpy(), yp['s0'], rtol=(n + 16) * 2 * EPS, atol=0)
    assert pri.gamma0 == yp['g0'] and pri.kappa0 == yp['k0'] and pri.nu0 == yp['nu0'] and torch.all(pri.m0 == 0) and torch.all(pri.s0[d0:] == 0)
    status, lbs = B.em(pts, pri, REG, mu, var, comp, TOL, 1)
    assert status[0, 0] == 1 and status[0, 1] == 1 and status[0, 2] == 0 and lbs.shape == (1, 1) and status[0, 3] == lbs[0, 0]
    c = comp[0].cpu().numpy()
    # the sufficient statistics and the new parameters: (B + N 2^-53) times the absolute-value sums, carried through the M-step to first order
    r, Xs, rate = np.exp(logr), y['Xs'], Bd + n * EPS
    nk = p1.nk
    b_n = rate * r.sum(axis=0) + 4 * EPS * nk
    xb = p1.m * p1.kappa[:, None] / nk[:, None]
    b_xb = rate * (r[:, :, None] * np.abs(Xs)[:, None, :]).sum(axis=0) / nk[:, None]
    b_s = rate * (r[:, :, None] * (Xs * Xs)[:, None, :]).sum(axis=0) / nk[:, None] + 2.0 * np.abs(xb) * b_xb
    dd = xb * xb
    s_term = p1.v * p1.nu[:, None] - yp['s0'][None, :]          # n_k (s + ratio dd)
    if cov == 'spherical':
        b_s = np.repeat(b_s.mean(axis=1)[:, None], d0, axis=1)
        b_dd = np.repeat((2.0 * np.abs(xb) * b_xb).mean(axis=1)[:, None], d0, axis=1)
        dd = np.repeat(dd.mean(axis=1)[:, None], d0, axis=1)
    else:
        b_dd = 2.0 * np.abs(xb) * b_xb
    ratio = yp['k0'] / p1.kappa
    b_m = b_xb + np.abs(xb) * (b_n / p1.kappa)[:, None] + 4 * EPS * np.abs(p1.m)
    b_v = ((b_n / nk)[:, None] * np.abs(s_term) + nk[:, None] * (b_s + ratio[:, None] * b_dd + dd * (ratio * b_n / p1.kappa)[:, None])) / p1.nu[:, None] \
        + p1.v * (b_n / p1.nu)[:, None] + 8 * EPS * p1.v
    got_m, got_v = mu[0, :, :d0].cpu().numpy(), var[0, :, :d0].cpu().numpy()
    ratios['n_k'] = np.max(np.abs(c[B.C_NK] - nk) / b_n)
    ratios['kappa'] = np.max(np.abs(c[B.C_KAPPA] - p1.kappa) / b_n)
    ratios['nu'] = np.max(np.abs(c[B.C_NU] - p1.nu) / b_n)
    ratios['m'] = np.max(np.abs(got_m - p1.m) / np.maximum(b_m, TINY))
    ratios['v'] = np.max(np.abs(got_v - p1.v) / np.maximum(b_v, TINY))
    if prior == DP:
        b_b = np.concatenate([np.cumsum(b_n[::-1])[-2::-1], [0.0]]) + K * 2 * EPS * p1.conc[1]
        ratios['a'] = np.max(np.abs(c[B.C_A] - p1.conc[0]) / b_n)
        ratios['b'] = np.max(np.abs(c[B.C_B] - p1.conc[1]) / b_b)
    else:
        ratios['alpha'] = np.max(np.abs(c[B.C_A] - p1.conc) / b_n)
        assert np.all(c[B.C_B] == 0)
    # the lower bound of the iteration, to first order in the deviations above; psi and lgamma at 8 x scipy's own deviation per term
    lr_abs = np.where(np.isfinite(logr), np.abs(logr), 0.0)
    b_ent = Bd * (r * (lr_abs + 1.0)).sum() + (n + K) * 2 * EPS * (r * lr_abs).sum()
    ent = -(r * np.where(np.isfinite(logr), logr, 0.0)).sum()
    half = 0.5 * (p1.nu[:, None] - np.arange(d0)[None, :])
    psi_sum = 0.5 * digamma(half).sum(axis=1)
    sf = 8 * max(SCIPY_DIGAMMA_DEV, SCIPY_GAMMALN_DEV)
    b_ell = 0.5 * (b_v / p1.v).sum(axis=1) + 0.5 * d0 * b_n / p1.nu + (d0 + 16) * EPS * (0.5 * np.abs(np.log(p1.v)).sum(axis=1) + 0.5 * d0 * np.abs(np.log(p1.nu)))
    b_logw = b_n * np.abs(p1.ell + 0.5 * d0 * np.log(2.0) + psi_sum) + p1.nu * b_ell + (sf + (d0 + 16) * EPS) * np.maximum(1.0, np.abs(gammaln(half))).sum(axis=1) \
        + 8 * EPS * np.abs(p1.nu * p1.ell)
    b_kap = 0.5 * d0 * ((b_n / p1.kappa).sum() + (K + 4) * EPS * np.abs(np.log(p1.kappa)).sum())
    if prior == DP:
        a, b = p1.conc
        b_norm = (np.abs(digamma(a) - digamma(a + b)) * b_n + np.abs(digamma(b) - digamma(a + b)) * b_b).sum() \
            + (sf + K * EPS) * (np.maximum(1.0, np.abs(gammaln(a))) + np.maximum(1.0, np.abs(gammaln(b))) + np.maximum(1.0, np.abs(gammaln(a + b)))).sum()
    else:
        al = p1.conc
        b_norm = (np.abs(digamma(al.sum()) - digamma(al)) * b_n).sum() + (sf + K * EPS) * (np.maximum(1.0, np.abs(gammaln(al))).sum()
                                                                                             + max(1.0, abs(gammaln(al.sum()))))
    b_lb = b_ent + b_logw.sum() + b_kap + b_norm + 8 * EPS * abs(lb1)
    ratios['lower bound'] = abs(lbs[0, 0] - lb1) / b_lb
    # the sum r log r word on its own: the bound minus the terms the yardstick forms from the DEVICE's new parameters
    pd_ = Model(nu=c[B.C_NU], ell=c[B.C_L], lgsum=c[B.C_LGAMMA], kappa=c[B.C_KAPPA], conc=(c[B.C_A], c[B.C_B]) if prior == DP else c[B.C_A])
    rest = y_lower_bound(np.zeros((1, K)), pd_, prior, d0)          # (log r = 0: r log r = 0, only the parameter terms)
    got_ent = rest - lbs[0, 0]          # sum r log r = -(lb - rest)
    ratios['sum r log r'] = abs(got_ent - (-ent)) / (b_ent + (sf + (d0 + 16) * EPS) * (np.abs(c[B.C_NU] * c[B.C_L]).sum() + np.abs(c[B.C_LGAMMA]).sum()
                                                                                       + abs(rest)))
    print(case, 'one pass: bound on log p', Bd, 'largest deviation / bound:', {k: float('%.3g' % v) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if pts.d > d0:          # the padding: m = 0, v = 1
        assert torch.all(mu[0, :, d0:] == 0) and torch.all(var[0, :, d0:] == 1)


@pytest.mark.parametrize('case', list(CASES))
def test_whole_fit_equals_the_yardstick(case):
    _, K, cov, prior = CASES[case]
    y = yardstick(case)
    m = device_fit(case)
    d0 = points(case).shape[1]
    assert m.n_iter_ == y['n_iter'] and m.converged_ is True and y['converged']
    assert m.labels_.dtype == np.int32 and np.array_equal(m.labels_, y['labels'])
    assert m.active_components_.dtype == np.int64 and np.array_equal(m.active_components_, y['active'])
    got = (m.lower_bounds_, m.weights_, m.means_, m.covariances_, m.degrees_of_freedom_, m.mean_precision_)
    names = ('lower_bounds', 'weights', 'means', 'covariances', 'degrees_of_freedom', 'mean_precision')
    dev = {name: rel(a, b) for name, a, b in zip(names, got, fit_arrays(y, cov))}
    conc = y['final'].conc
    if prior == DP:
        assert isinstance(m.weight_concentration_, tuple) and len(m.weight_concentration_) == 2
        dev['a'], dev['b'] = rel(m.weight_concentration_[0], conc[0]), rel(m.weight_concentration_[1], conc[1])
    else:
        assert m.weight_concentration_.shape == (K,)
        dev['alpha'] = rel(m.weight_concentration_, conc)
    print(case, 'whole fit: n_iter', m.n_iter_, 'active', len(m.active_components_), 'relative deviations', dev, 'allowed', fit_rtol(case))
    assert max(dev.values()) <= fit_rtol(case)
    assert abs(m.weights_.sum() - 1.0) <= K * 2.0 ** -52
    assert m.lower_bound_ == m.lower_bounds_[-1] and m.n_features_in_ == d0
    for name in ATTRS[:8]:
        assert getattr(m, name).dtype == np.float64, name
    assert m.covariances_.shape == ((K, d0) if cov == 'diag' else (K,)) and m.means_.shape == (K, d0)
    assert m.weights_.shape == m.mean_precision_.shape == m.degrees_of_freedom_.shape == (K,)
    assert m.precisions_.shape == m.precisions_cholesky_.shape == m.covariances_.shape
    np.testing.assert_allclose(m.precisions_, 1.0 / m.covariances_, rtol=1e-15)
    assert m.weight_concentration_prior_ == 1.0 / K and m.mean_precision_prior_ == 1.0 and m.degrees_of_freedom_prior_ == d0
    np.testing.assert_allclose(m.mean_prior_, points(case).astype(np.float64).mean(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.atleast_1d(m.covariance_prior_), np.atleast_1d(cov_of(y['priors']['s0'][None, :], cov)[0]), rtol=1e-12)


@pytest.mark.parametrize('case', list(CASES))
def test_two_calls_and_a_host_array_give_identical_bits(case):
    m = device_fit(case)
    again = _fit(case, device_points(case))
    host = _fit(case, np.array(points(case)))          # the contiguous (and, for d13, padded) copy; for `strided` the same points without the gaps
    for name in ATTRS:
        assert getattr(m, name).tobytes() == getattr(again, name).tobytes() == getattr(host, name).tobytes(), name
    assert m.n_iter_ == again.n_iter_ == host.n_iter_ and np.array_equal(m.active_components_, host.active_components_)
    if case == 'strided':          # read where it lies
        view = device_points(case)
        assert B._Points(view).x.data_ptr() == view.data_ptr() and torch.isnan(view._base[:, :4]).all() and torch.isnan(view._base[:, 12:]).all()


@functools.lru_cache(maxsize=None)
def three_restarts(case):
    pts = B._Points(device_points(case))
    return pts, _model(case, n_init=3)._fit_points(pts, init_labels=initial_labels(case, 3))


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_pick_the_winner_and_do_not_depend_on_each_other(case):
    _, K, cov, prior = CASES[case]
    pts, m = three_restarts(case)
    ys = [yardstick(case, r, 3) for r in range(3)]
    best = winner(case)
    assert [int(v) for v in m._status[:, 1]] == [y['n_iter'] for y in ys] and np.all(m._status[:, 0] == 1) and np.all(m._status[:, 2] == 1)
    assert m.lower_bound_ == m._status[best, 3] == np.max(m._status[:, 3]) and m.n_iter_ == ys[best]['n_iter']
    assert np.array_equal(m.labels_, ys[best]['labels'])
    got = (m.lower_bounds_, m.weights_, m.means_, m.covariances_, m.degrees_of_freedom_, m.mean_precision_)
    assert max(rel(a, b) for a, b in zip(got, fit_arrays(ys[best], cov))) <= fit_rtol(case)
    for r in range(3):
        # alone, and with max_iter cut at its own n_iter_: the same bytes -- a done restart is frozen while the others continue
        for max_iter in (100, ys[r]['n_iter']):
            solo = _model(case, n_init=1, max_iter=max_iter)._fit_points(pts, init_labels=initial_labels(case, 3)[r:r + 1])
            for part, alone in zip(m._all_parameters, solo._all_parameters):
                assert part[r].tobytes() == alone[0].tobytes()
            assert m._all_lower_bounds[r, :ys[r]['n_iter']].tobytes() == solo._all_lower_bounds[0, :ys[r]['n_iter']].tobytes()
            assert solo.converged_ and solo.n_iter_ == ys[r]['n_iter']
    short = min(range(3), key=lambda r: ys[r]['n_iter'])
    assert np.all(np.isnan(m._all_lower_bounds[short, ys[short]['n_iter']:]))


def test_padding_adds_nothing_and_a_single_iteration_does_not_converge():
    y = yardstick('d13')
    m = device_fit('d13')
    assert m.means_.shape == (3, 13) and m.covariances_.shape == (3, 13)
    np.testing.assert_allclose(m.lower_bounds_, y['lbs'], rtol=fit_rtol('d13'), atol=0)          # (13 columns and 13 psi terms, not 16)
    # the same points in a 16-column buffer whose padding the caller wrote: the same bits
    X = np.array(points('d13'))
    wide = torch.zeros((len(X), 16), dtype=torch.float32, device='cuda')
    wide[:, :13] = torch.as_tensor(X, device='cuda')
    view = _fit('d13', wide[:, :13])
    for name in ATTRS:
        assert getattr(m, name).tobytes() == getattr(view, name).tobytes(), name
    with pytest.warns(UserWarning, match='Best performing initialization did not converge'):
        one = _fit('overlap_k9', device_points('overlap_k9'), max_iter=1)
    assert one.converged_ is False and one.n_iter_ == 1 and len(one.lower_bounds_) == 1
    assert one.lower_bounds_[0] == device_fit('overlap_k9').lower_bounds_[0]


@pytest.mark.parametrize('case,held', [('n1030_k12', lambda: blobs(333, 8, 6)), ('sph_k8', lambda: blobs(517, 8, 11, n_centers=4, spread=1.2)),
                                       ('sph_d256_k6', lambda: blobs(131, 256, 14, n_centers=6, spread=0.15)), ('d13', lambda: blobs(77, 13, 15)),
                                       ('overlap_k9_dd', lambda: blobs(400, 12, 12, n_centers=9, spread=1.5))])
def test_predict_and_scores_on_held_out_points(case, held):
    from scipy.special import digamma
    _, K, cov, prior = CASES[case]
    m = device_fit(case)
    H = held()
    d0 = H.shape[1]
    v = m.covariances_ if cov == 'diag' else np.repeat(m.covariances_[:, None], d0, axis=1)
    # the constants of the E-step from the fitted attributes, by the yardstick's formulas
    if prior == DP:
        a, b = m.weight_concentration_
        elogpi = digamma(a) - digamma(a + b) + np.hstack((0, np.cumsum(digamma(b) - digamma(a + b))[:-1]))
    else:
        elogpi = digamma(m.weight_concentration_) - digamma(m.weight_concentration_.sum())
    nu, kap = m.degrees_of_freedom_, m.mean_precision_
    psi = digamma(0.5 * (nu[:, None] - np.arange(d0)[None, :]))
    ell = -0.5 * np.log(v).sum(axis=1) - 0.5 * d0 * np.log(nu)
    lc = elogpi - 0.5 * d0 * np.log(2.0 * np.pi) + ell + 0.5 * (d0 * np.log(2.0) + psi.sum(axis=1) - d0 / kap)
    b_lc = (8 * SCIPY_DIGAMMA_DEV + (d0 + 16) * EPS) * (0.5 * np.maximum(1.0, np.abs(psi)).sum(axis=1) + 3 * K * np.maximum(1.0, np.abs(elogpi)) + np.abs(ell)
                                                       + 0.5 * np.abs(np.log(v)).sum(axis=1) + d0)
    assert np.all(np.abs(m._log_const - lc) <= b_lc), (np.abs(m._log_const - lc) / b_lc).max()
    _, logp, lse, logr = y_estep(H.astype(np.float64) - m._shift, Model(m=m._means_shifted, v=v, lc=m._log_const))
    Bd = log_bound(case, logp)
    top = np.sort(logp, axis=1)
    decided = (top[:, -1] - top[:, -2]) > 1e-4 if K > 1 else np.ones(len(H), bool)
    pred, proba, scores, score = m.predict(H), m.predict_proba(torch.as_tensor(H, device='cuda')), m.score_samples(H), m.score(H)
    assert pred.shape == (len(H),) and proba.shape == (len(H), K) and proba.dtype == np.float64 and scores.dtype == np.float64
    assert decided.mean() > 0.98 and np.array_equal(pred[decided], logp.argmax(axis=1)[decided])
    assert np.max(np.abs(scores - lse)) <= Bd and np.max(np.abs(proba - np.exp(logr))) <= Bd
    assert np.max(np.abs(proba.sum(axis=1) - 1.0)) <= 1e-12
    assert abs(score - lse.mean()) <= Bd + len(H) * EPS * np.abs(lse).mean()
    assert np.array_equal(pred[decided], proba.argmax(axis=1)[decided])
    assert not hasattr(m, 'bic') and not hasattr(m, 'aic')
    with pytest.raises(ValueError, match='expecting %d features' % d0):
        m.predict(H[:, :-1])


def test_reorder_permutes_every_per_component_attribute():
    case = 'n1030_k12'
    m = _fit(case, device_points(case))
    ref = device_fit(case)
    order = np.random.RandomState(0).permutation(12)
    m.reorder(order)
    X = np.array(points(case))
    inverse = np.argsort(order)
    assert np.array_equal(m.labels_, inverse[ref.labels_]) and np.array_equal(m.predict(X), m.labels_)
    assert np.array_equal(m.active_components_, np.sort(inverse[ref.active_components_]))
    for name in ('weights_', 'means_', 'covariances_', 'mean_precision_', 'degrees_of_freedom_'):
        assert np.array_equal(getattr(m, name), getattr(ref, name)[order]), name
    assert np.array_equal(m.weight_concentration_[1], ref.weight_concentration_[1][order])
    # (not the same bits: the sum over the components is a tree over the lanes, and the components changed lanes; 12 terms of at most 1, both ways)
    np.testing.assert_allclose(m.predict_proba(X), ref.predict_proba(X)[:, order], rtol=0, atol=4 * 12 * EPS)


@pytest.mark.parametrize('case', ['n1030_k12', 'sph_k8'])
def test_end_to_end_equals_sklearn(case):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov, prior = CASES[case]
    X = np.array(points(case))
    ours = BayesianGaussianMixture(K, covariance_type=cov, init_params='kmeans', random_state=0, weight_concentration_prior_type=prior).fit(X)
    ref = mix.BayesianGaussianMixture(n_components=K, covariance_type=cov, init_params='kmeans', random_state=0,
                                      weight_concentration_prior_type=prior).fit(X.astype(np.float64))
    assert np.array_equal(ours.fit_predict(X), ours.labels_)
    assert np.array_equal(ours.labels_, ref.predict(X.astype(np.float64)))
    assert ours.n_iter_ == ref.n_iter_ and ours.converged_ == ref.converged_
    dev = max(rel(ours.weights_, ref.weights_), rel(ours.means_, ref.means_), rel(ours.covariances_, ref.covariances_),
              rel(ours.lower_bounds_, ref.lower_bounds_), rel(ours.degrees_of_freedom_, ref.degrees_of_freedom_),
              rel(ours.mean_precision_, ref.mean_precision_))
    print(case, 'end to end against sklearn: n_iter', ours.n_iter_, 'relative deviation', dev, 'allowed', fit_rtol(case))
    assert dev <= fit_rtol(case)


def test_sweep_and_other_initialisations():
    """One fit per concentration from one upload; a larger concentration does not activate fewer components (sklearn on the CPU gives 5, 5 and 5 components
    with a training row at 0.001, 1 / 12 and 100 on these points, random_state 0); seeded fits are repeatable."""
    X = device_points('n1030_k12')
    calls = []
    real = B.prior_moments
    try:
        B.prior_moments = lambda pts: calls.append(pts) or real(pts)
        sweep = bgmm_sweep(X, [0.001, 1.0 / 12, 100.0], n_components=12, random_state=0)
    finally:
        B.prior_moments = real
    assert list(sweep) == [0.001, 1.0 / 12, 100.0] and len({id(p) for p in calls}) == 1
    active = [len(sweep[g].active_components_) for g in sweep]
    print('n1030_k12 sweep: active components', active)
    assert active[0] <= active[1] <= active[2] and all(isinstance(f, BayesianGaussianMixture) for f in sweep.values())
    assert [sweep[g].weight_concentration_prior_ for g in sweep] == list(sweep)
    alone = BayesianGaussianMixture(12, weight_concentration_prior=100.0, random_state=0).fit(X)
    for name in ATTRS:
        assert getattr(alone, name).tobytes() == getattr(sweep[100.0], name).tobytes(), name
    for init in ('k-means++', 'random_from_data', 'random'):
        a = BayesianGaussianMixture(6, init_params=init, n_init=2, random_state=3).fit(X)
        b = BayesianGaussianMixture(6, init_params=init, n_init=2, random_state=np.random.RandomState(3)).fit(X)
        for name in ATTRS:
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (init, name)
        assert np.isfinite(a.lower_bound_) and abs(a.weights_.sum() - 1.0) <= 6 * 2.0 ** -52


def test_given_priors_reach_the_kernels():
    """Priors other than the defaults: against live sklearn from the same initial labels."""
    mix = pytest.importorskip('sklearn.mixture')
    case = 'sph_k8'
    X = np.array(points(case))
    labels0 = initial_labels(case)[0]
    kw = dict(covariance_type='spherical', weight_concentration_prior=0.3, mean_precision_prior=0.5, mean_prior=X[:7].astype(np.float64).mean(axis=0),
              degrees_of_freedom_prior=9.5, covariance_prior=2.0)

    class FromLabels(mix.BayesianGaussianMixture):
        def _initialize_parameters(self, X, random_state):
            self._initialize(X, one_hot(labels0, 8))

    ref = FromLabels(n_components=8, **kw).fit(X.astype(np.float64))
    ours = BayesianGaussianMixture(8, **kw)._fit_points(B._Points(X), init_labels=labels0[None])
    assert ours.n_iter_ == ref.n_iter_ and np.array_equal(ours.labels_, ref.predict(X.astype(np.float64)))
    dev = max(rel(ours.weights_, ref.weights_), rel(ours.means_, ref.means_), rel(ours.covariances_, ref.covariances_),
              rel(ours.lower_bounds_, ref.lower_bounds_), rel(ours.degrees_of_freedom_, ref.degrees_of_freedom_),
              rel(ours.mean_precision_, ref.mean_precision_))
    print('given priors against sklearn: relative deviation', dev, 'allowed', fit_rtol(case))
    assert dev <= fit_rtol(case)


def test_p2_bgmm_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'bgmm', '--k_max', '6', '--n_init', '2', '--bgmm_concentration', '0.01', '10'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X, V = data['training']['hidden'], data['validation']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_bgmm_aligned' / 'plot'
    table, weights, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Bgmm.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(table.columns) == ['concentration', 'n_components', 'n_active', 'lower_bound', 'n_iter', 'converged', 'valid_score'] + metrics
    assert table.concentration.tolist() == [0.01, 10.0] and table.n_components.tolist() == [6, 6] and len(table) == 2
    assert list(weights.columns) == ['concentration', 'component', 'weight', 'n_k', 'mean_precision', 'degrees_of_freedom', 'active'] and len(weights) == 12
    assert list(labels.columns) == ['c0', 'c1'] and len(labels) == len(X)
    assert np.all(np.isfinite(table[['lower_bound', 'valid_score']].to_numpy())) and np.all(table.n_iter >= 1)
    for row, column in enumerate(labels.columns):
        lab = labels[column].to_numpy()
        assert sorted(set(lab.tolist())) == list(range(int(table.n_active[row])))          # consecutive ids
        w = weights[weights.concentration == table.concentration[row]]
        assert int(w.active.sum()) == table.n_active[row] and abs(w.weight.sum() - 1.0) < 1e-12 and w.component.tolist() == list(range(6))
        np.testing.assert_allclose(w.n_k.sum(), len(X), rtol=1e-9)
        np.testing.assert_array_equal(np.bincount(lab) > 0, True)
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy(), equal_nan=True)
    # a second run finds the files and does not recompute; overwrite=True does
    bg = p2.Bgmm(6, str(plot.parent), metrics, n_init=2, concentrations=[0.01, 10.0])
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Bgmm.FILES]
    calls = []
    real = p2.bgmm_sweep
    monkeypatch.setattr(p2, 'bgmm_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = bg.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Bgmm.FILES] == stamps and bg.fits_ is None
    assert np.array_equal(again.to_numpy(), table.to_numpy(), equal_nan=True)
    redo = bg.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and len(bg.fits_) == 2 and list(redo.columns) == list(table.columns)
    np.testing.assert_allclose(redo.valid_score, [f.score(V) for f in bg.fits_], rtol=0, atol=0)
    assert p2.Bgmm(6, str(plot.parent), metrics).concentrations == [1.0 / 6]


def test_p4_bgmm_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.BayesianGaussianMixture):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'BayesianGaussianMixture', Recording)
    args = p4.get_arguments(['--cluster_method', 'bgmm', '--num_clusters', '8'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_bgmm_aligned'
    saved = {cohort: np.load(out / ('%s_bgmm-K8.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1
    model = made[0]
    active = model.active_components_
    A = len(active)
    assert 1 <= A <= 8 and model.n_components == 8
    # the active components by descending sbp of their training encounters, as the branch orders them
    sbp = data['training']['ob'][:, 0, :].mean(1)
    columns = active[np.argsort([sbp[model.labels_ == k].mean() for k in active])[::-1]]
    for cohort in COHORTS:
        s = saved[cohort]
        assert sorted(s) == ['cluster_id', 'cluster_prob', 'encounter_id', 'hidden'] and len(s['cluster_id']) == len(data[cohort]['hidden'])
        prob = s['cluster_prob']
        assert prob.dtype == np.float32 and prob.shape == (len(s['cluster_id']), A)          # one column per active component
        assert set(np.asarray(s['cluster_id']).tolist()) <= set(range(A))          # active components only
        full = model.predict_proba(data[cohort]['hidden'])
        assert np.array_equal(prob, full[:, columns].astype(np.float32))
        assert np.array_equal(s['cluster_id'], full[:, columns].argmax(axis=1))
        # predict, where its component is active; the best active one otherwise
        pred = model.predict(data[cohort]['hidden'])
        hit = np.isin(pred, active)
        assert np.array_equal(columns[np.asarray(s['cluster_id'])][hit], pred[hit])
    ids = np.asarray(saved['training']['cluster_id'])
    assert sorted(set(ids.tolist())) == list(range(A))
    means = [sbp[ids == i].mean() for i in range(A)]
    assert all(means[i] > means[i + 1] for i in range(A - 1))
    # an existing result is left alone
    stamps = [(out / ('%s_bgmm-K8.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_bgmm-K8.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
