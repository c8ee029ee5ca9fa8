"""Full- and tied-covariance Gaussian mixtures, host side (no GPU): the numpy f64 yardstick of the definition in include/dic_hip.h against sklearn, the
conditions the GPU tests (tests/test_gpu_gmm_full.py) rely on, bic / aic, the ABI's and the Python argument errors, and the register use of the kernels."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import gmm_full as GF
from deep_interpolation_clustering_amd.gmm_full import FullGaussianMixture, n_parameters

import test_gmm_host as TG
from test_gmm_host import blobs, one_hot, rel

TOL, REG = 1e-3, 1e-6          # sklearn's defaults, used by every case


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def mild(n, d, seed, n_centers, spread, mix=0.5):
    """Correlated clusters: centres N(0, spread^2); the points of cluster c are z (I + mix G_c / sqrt(d)), z and G_c standard normal."""
    rs = np.random.RandomState(seed)
    centers = rs.normal(0.0, spread, size=(n_centers, d))
    A = np.stack([np.eye(d) + mix * rs.normal(size=(d, d)) / np.sqrt(d) for _ in range(n_centers)])
    which = rs.randint(n_centers, size=n)
    z = rs.normal(size=(n, d))
    return (centers[which] + np.einsum('nd,nde->ne', z, A[which])).astype(np.float32)


def corr_blobs(n, d, seed, n_centers, spread):
    """The same with z (0.5 I + G_c / sqrt(d)): ill-conditioned covariances, kept on purpose."""
    rs = np.random.RandomState(seed)
    centers = rs.normal(0.0, spread, size=(n_centers, d))
    A = np.stack([0.5 * np.eye(d) + rs.normal(size=(d, d)) / np.sqrt(d) for _ in range(n_centers)])
    which = rs.randint(n_centers, size=n)
    z = rs.normal(size=(n, d))
    return (centers[which] + np.einsum('nd,nde->ne', z, A[which])).astype(np.float32)


def _corr_k4():
    return corr_blobs(1030, 8, 11, 4, 1.2)


# name -> (points, K, covariance type).  The GPU tests run on exactly these.
CASES = {
    'full_d256_k2': (lambda: mild(2100, 256, 14, 2, 0.10), 2, 'full'),
    'full_d64_k3': (lambda: mild(1500, 64, 5, 3, 0.3), 3, 'full'),
    'full_d12_k9': (lambda: mild(4100, 12, 12, 9, 1.5), 9, 'full'),
    'full_corr_k4': (_corr_k4, 4, 'full'),
    'tied_corr_k4': (_corr_k4, 4, 'tied'),
    'tied_d64_k4': (lambda: mild(1500, 64, 6, 4, 0.35, mix=0.0), 4, 'tied'),
    'tied_d256_k5': (lambda: blobs(1500, 256, 14, n_centers=6, spread=0.15), 5, 'tied'),
    'n2_k1': (lambda: blobs(2, 4, 1), 1, 'full'),
    'n17_k2': (lambda: blobs(17, 4, 3), 2, 'full'),
    'n255_d64_k3': (lambda: blobs(255, 64, 4), 3, 'tied'),
    'n257_d13_k3': (lambda: blobs(257, 13, 15), 3, 'full'),
    'd4_k2': (lambda: blobs(300, 4, 2, n_centers=2), 2, 'full'),
    'd200_k2': (lambda: mild(900, 200, 7, 2, 0.10), 2, 'full'),
    'dup_k3': (TG._dup, 3, 'tied'),
    'strided': (lambda: blobs(257, 8, 10), 3, 'full'),
    'k32_d8': (lambda: blobs(4100, 8, 13, n_centers=32, spread=2.0), 32, 'full'),
}
WELL_CONDITIONED = ['full_d256_k2', 'full_d64_k3', 'full_d12_k9', 'd200_k2', 'k32_d8']          # n_k >= 2 D0 and cond(C_k) <= 1e4
OVERLAP = ['full_d12_k9', 'full_corr_k4', 'tied_corr_k4', 'tied_d64_k4', 'tied_d256_k5']          # > 2 % of the rows soft at the end of the fit
BLURRED = ['full_d256_k2', 'full_d64_k3']          # the soft path at high D: one E-step from blurred parameters
N_INIT_CASES = ['full_corr_k4', 'tied_corr_k4']

# The largest relative deviation (max |a - b| / max |b| per array: lower bounds, weights, means, covariances, and the factors P and log_det, which answer a
# change of C with up to cond(C) times that change) measured on the CPU, per case, between (a) the yardstick and sklearn 1.7.2 started from the same parameters,
# sklearn's own factor of its own covariances included, (b) the yardstick with numpy's pairwise / BLAS sums and with sequential ones (rows one after the other
# for n_k and mu', 32-row blocks one after the other for the scatter matrices), the factors of the initial M-step and of the first iteration included, and
# (c) the two factor routines -- LAPACK's and the header's column order -- on the fit's final covariances (P and log_det).  The GPU tests allow 16 x the largest
# of the three, never less than 1e-13.  Measured with numpy 2.2 / sklearn 1.7.2 on x86-64; the host tests hold the yardstick to 4 x these figures.
BASE = {
    'full_d256_k2': (4.24e-15, 1.56e-14, 8.66e-15), 'full_d64_k3': (4.37e-15, 2.94e-14, 6.79e-16), 'full_d12_k9': (1.04e-13, 2.29e-13, 6.11e-16),
    'full_corr_k4': (9.41e-14, 6.35e-14, 1.33e-14), 'tied_corr_k4': (6.42e-14, 7.42e-14, 9.62e-17), 'tied_d64_k4': (6.47e-14, 1.33e-14, 4.44e-16),
    'tied_d256_k5': (2.06e-13, 2.60e-13, 9.77e-16), 'n2_k1': (6.50e-10, 0.0, 2.01e-9), 'n17_k2': (9.93e-15, 8.42e-15, 4.61e-15),
    'n255_d64_k3': (2.67e-12, 1.12e-13, 2.01e-14), 'n257_d13_k3': (4.41e-14, 1.24e-13, 3.55e-15), 'd4_k2': (1.64e-13, 9.45e-13, 2.54e-17),
    'd200_k2': (8.45e-16, 6.81e-15, 1.27e-15), 'dup_k3': (4.68e-14, 7.23e-14, 1.37e-15), 'strided': (6.16e-14, 3.29e-13, 2.40e-15),
    'k32_d8': (1.05e-13, 1.61e-13, 5.76e-16),
}
# Without the factors among the arrays the same measurement gave (a) 5.9e-16 .. 2.1e-13 and (b) 0 .. 3.3e-13: the factors carry cond(C), 130 for `strided`.
# Iterations / largest cond(C) / soft share of the fits: full_d256_k2 6 / 22 / 0; full_d64_k3 8 / 28 / 0.003; full_d12_k9 3 / 19 / 0.040; full_corr_k4 5 / 3.4e3 /
# 0.033; tied_corr_k4 11 / 4.7 / 0.39; tied_d64_k4 4 / 2.3 / 0.42; tied_d256_k5 47 / 8.9 / 0.16; k32_d8 10 / 9.1 / 0.32; the small shapes 2 iterations each.
# n2_k1: two points give a covariance of rank 1 plus reg_covar, cond 5.5e7; the factor's entries of size 1e3 carry that condition number's share of an ulp.


def fit_rtol(case):
    return max(16.0 * max(BASE[case]), 1e-13)


@functools.lru_cache(maxsize=None)
def points(case):
    X = CASES[case][0]()
    X.setflags(write=False)
    return X


def _sum(a, axis, seq):
    return TG._sum(a, axis, seq)


def y_factor(C):
    """(P = L^-T, log_det) of (.., D, D) covariances with LAPACK's Cholesky and solve."""
    C = np.asarray(C)
    L = np.linalg.cholesky(C)
    P = np.swapaxes(np.linalg.solve(L, np.broadcast_to(np.eye(C.shape[-1]), C.shape)), -1, -2)
    P = np.triu(P)
    return P, np.log(np.diagonal(P, axis1=-2, axis2=-1)).sum(axis=-1)


def y_factor_columns(C):
    """One (D, D) covariance in the header's plain column order: (P, log_det), or None where a pivot is not a finite positive number."""
    C = np.asarray(C, dtype=np.float64)
    D = len(C)
    L = np.zeros((D, D))
    for j in range(D):
        s = C[j:, j].copy()
        for t in range(j):
            s = s - L[j:, t] * L[j, t]
        if not (s[0] > 0.0 and np.isfinite(s[0])):
            return None
        L[j, j] = np.sqrt(s[0])
        L[j + 1:, j] = s[1:] / L[j, j]
    P = np.zeros((D, D))
    for c in range(D - 1, -1, -1):
        P[c, c] = 1.0 / L[c, c]
        s = np.zeros(D - c - 1)          # columns c + 1 ..
        for t in range(c + 1, D):
            s[t - c - 1:] = s[t - c - 1:] + L[t, c] * P[t, t:]
        P[c, c + 1:] = -s / L[c, c]
    ld = 0.0
    for d in range(D):
        ld = ld + np.log(P[d, d])
    return P, ld


def y_estep(Xs, w, mu, P, log_det, seq=False):
    """The E-step of the definition on shifted f64 points, P (Kc, D, D), log_det (Kc): (M, log p, lse, log r)."""
    K = len(w)
    M = np.empty((len(Xs), K))
    for k in range(K):
        y = (Xs - mu[k]) @ P[k if len(P) > 1 else 0]
        M[:, k] = _sum(y * y, 1, seq)
    ld = log_det if len(log_det) == K else np.repeat(log_det, K)
    logp = np.log(w)[None, :] - 0.5 * (Xs.shape[1] * np.log(2.0 * np.pi) + M) + ld[None, :]
    mx = logp.max(axis=1)
    lse = mx + np.log(_sum(np.exp(logp - mx[:, None]), 1, seq))
    return M, logp, lse, logp - lse[:, None]


def scatter(Xs, wgt, seq=False):
    """sum_i wgt_i x_i x_i^T: one BLAS product, or 32-row blocks one after the other."""
    if not seq:
        return (wgt[:, None] * Xs).T @ Xs
    S = np.zeros((Xs.shape[1], Xs.shape[1]))
    for i in range(0, len(Xs), 32):
        S = S + (wgt[i:i + 32, None] * Xs[i:i + 32]).T @ Xs[i:i + 32]
    return S


def y_mstep(Xs, r, cov_type, reg=REG, seq=False):
    """The M-step of the definition: (w, mu', C (Kc, D, D), n_k)."""
    K, D = r.shape[1], Xs.shape[1]
    nk = _sum(r, 0, seq) + 10.0 * np.finfo(np.float64).eps
    mu = _sum(r[:, :, None] * Xs[:, None, :], 0, seq) / nk[:, None]
    if cov_type == 'full':
        C = np.stack([scatter(Xs, r[:, k], seq) / nk[k] - np.outer(mu[k], mu[k]) + reg * np.eye(D) for k in range(K)])
    else:
        m2 = np.zeros((D, D))
        for k in range(K):
            m2 = m2 + np.outer(nk[k] * mu[k], mu[k])
        C = ((scatter(Xs, np.ones(len(Xs)), seq) - m2) / _sum(nk, 0, True) + reg * np.eye(D))[None]
    w = nk / len(Xs)
    return w / _sum(w, 0, seq), mu, C, nk


def y_fit(X, K, cov_type, labels0, tol=TOL, reg=REG, max_iter=100, seq=False):
    """EM of the definition from the one-hot responsibilities of ``labels0``: a dict as test_gmm_host.y_fit's, the parameters (w, mu', C, P, log_det)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    c = X64.mean(axis=0)
    Xs = X64 - c
    w, mu, C, _ = y_mstep(Xs, one_hot(labels0, K), cov_type, reg, seq)
    P, ld = y_factor(C)
    out = {'c': c, 'Xs': Xs, 'init': (w, mu, C, P, ld), 'lbs': [], 'converged': False}
    lb = -np.inf
    for it in range(1, max_iter + 1):
        prev = lb
        M, logp, lse, logr = y_estep(Xs, w, mu, P, ld, seq)
        w, mu, C, nk = y_mstep(Xs, np.exp(logr), cov_type, reg, seq)
        P, ld = y_factor(C)
        if it == 1:
            out['first'] = (M, logp, lse, logr, (w, mu, C, P, ld, nk))
        lb = _sum(lse, 0, seq) / len(Xs)
        out['lbs'].append(lb)
        if abs(lb - prev) < tol:
            out['converged'] = True
            break
    out['n_iter'] = it
    out['final'] = (w, mu, C, P, ld)
    out['nk'] = nk
    out['lbs'] = np.array(out['lbs'])
    _, logp, lse, logr = y_estep(Xs, w, mu, P, ld, seq)
    out['logr'], out['lse'], out['labels'] = logr, lse, logp.argmax(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def initial_labels(case, n_init=1):
    """sklearn's KMeans(n_init=1) on the f64 points, ``n_init`` fits in a row from one RandomState(5): (n_init, N)."""
    sk = pytest.importorskip('sklearn.cluster')
    X, K = points(case), CASES[case][1]
    rs = np.random.RandomState(5)
    return np.stack([sk.KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X.astype(np.float64)).labels_ for _ in range(n_init)])


@functools.lru_cache(maxsize=None)
def yardstick(case, restart=0, n_init=1, seq=False):
    _, K, cov = CASES[case]
    return y_fit(points(case), K, cov, initial_labels(case, n_init)[restart], seq=seq)


def cov_of(C, cov_type):
    return C if cov_type == 'full' else C[0]


@functools.lru_cache(maxsize=None)
def sklearn_fit(case):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov = CASES[case]
    y = yardstick(case)
    w, mu, C, P, ld = y['init']
    prec = cov_of(P @ np.swapaxes(P, -1, -2), cov)
    return mix.GaussianMixture(K, covariance_type=cov, tol=TOL, reg_covar=REG, weights_init=w / w.sum() if K > 1 else np.ones(1), means_init=mu + y['c'],
                               precisions_init=prec).fit(points(case).astype(np.float64))


def sk_factor(sk):
    """sklearn's own factor of its own covariances, in the yardstick's shapes: (P (Kc, D, D), log_det (Kc))."""
    P = np.asarray(sk.precisions_cholesky_)
    P = P if P.ndim == 3 else P[None]
    return P, np.log(np.diagonal(P, axis1=-2, axis2=-1)).sum(axis=-1)


def deviations(case, other):
    """The relative deviations of ``other`` = (lower bounds, weights, means, covariances, P (Kc, D, D), log_det (Kc)) from the yardstick's."""
    _, _, cov = CASES[case]
    y = yardstick(case)
    w, mu, C, P, ld = y['final']
    lbs, ow, om, oc, op, old = other
    return max(rel(lbs, y['lbs']), rel(ow, w), rel(om, mu + y['c']), rel(oc, cov_of(C, cov)), rel(op, P), rel(old, ld))


def stage_deviations(case, other):
    """The factors of the initial M-step and of the first iteration, which the GPU tests compare too: ``other`` is another yardstick dict."""
    y = yardstick(case)
    return max(rel(other['init'][3], y['init'][3]), rel(other['init'][4], y['init'][4]), rel(other['first'][4][3], y['first'][4][3]),
               rel(other['first'][4][4], y['first'][4][4]))


@functools.lru_cache(maxsize=None)
def factor_deviation(case):
    """(c): the header's column order against LAPACK on the fit's final covariances."""
    C, P, ld = yardstick(case)['final'][2:]
    dev = 0.0
    for k in range(len(C)):
        Pc, ldc = y_factor_columns(C[k])
        dev = max(dev, rel(Pc, P[k]), abs(ldc - ld[k]) / max(abs(ld[k]), 1.0))
    return dev


def blurred(case):
    """Parameters that leave many rows soft at high D: the means of the initial labels, every covariance the pooled (tied) one: (w, mu', P (K, D, D), log_det)."""
    y = yardstick(case)
    K = CASES[case][1]
    w, mu, C, _ = y_mstep(y['Xs'], one_hot(initial_labels(case)[0], K), 'tied')
    P, ld = y_factor(C)
    return w, mu, np.repeat(P, K, axis=0), np.repeat(ld, K)


@pytest.mark.parametrize('case', list(CASES))
def test_yardstick_equals_sklearn(case):
    sk = sklearn_fit(case)
    y = yardstick(case)
    assert sk.n_iter_ == y['n_iter'] and sk.converged_ == y['converged'] and y['converged']
    assert np.array_equal(sk.predict(points(case).astype(np.float64)), y['labels'])
    dev = deviations(case, (sk.lower_bounds_, sk.weights_, sk.means_, sk.covariances_) + sk_factor(sk))
    print(case, 'n_iter', y['n_iter'], 'yardstick vs sklearn', dev)
    assert dev <= 4.0 * BASE[case][0]
    if case in OVERLAP:
        soft = float((np.exp(y['logr']).max(axis=1) < 0.99).mean())
        print(case, 'rows with a largest responsibility below 0.99:', soft)
        assert soft > 0.02


@pytest.mark.parametrize('case', list(CASES))
def test_pairwise_and_sequential_sums_agree(case):
    y, s = yardstick(case), yardstick(case, seq=True)
    assert s['n_iter'] == y['n_iter'] and np.array_equal(s['labels'], y['labels'])
    w, mu, C, P, ld = s['final']
    dev = max(deviations(case, (s['lbs'], w, mu + s['c'], cov_of(C, CASES[case][2]), P, ld)), stage_deviations(case, s))
    print(case, 'pairwise vs sequential', dev)
    assert dev <= (4.0 * BASE[case][1] if BASE[case][1] > 0.0 else 1e-14)          # (n2_k1: one block of rows either way, the same bits)


@pytest.mark.parametrize('case', list(CASES))
def test_the_two_factor_routines_agree(case):
    dev = factor_deviation(case)
    print(case, 'column order vs LAPACK', dev)
    assert dev <= 4.0 * BASE[case][2]


def test_factor_yardstick_refuses_a_zero_pivot():
    assert y_factor_columns(np.zeros((4, 4))) is None and y_factor_columns(np.diag([1.0, np.nan])) is None


@pytest.mark.parametrize('case', list(CASES))
def test_cases_meet_the_conditions(case):
    """What the GPU tests rely on: clear stopping decisions, clear labels, no vanishing component, and for the cases named well-conditioned enough rows per
    component and cond(C_k) <= 1e4.  (A change of seed must keep these.)"""
    y = yardstick(case)
    _, K, cov = CASES[case]
    steps = np.abs(np.diff(np.concatenate([[-np.inf], y['lbs']])))
    margin = float(np.min(np.abs(steps - TOL)))
    assert margin > 1e-6, (case, steps)
    gap = np.inf
    if K > 1:
        top = np.sort(y['logr'], axis=1)
        gap = float(np.min(top[:, -1] - top[:, -2]))
        assert gap > 1e-4
    assert y['final'][0].min() >= 1e-3
    conds = [float(np.linalg.cond(c)) for c in y['final'][2]]
    print(case, 'stop margin', margin, 'label gap', gap, 'smallest weight', y['final'][0].min(), 'smallest n_k', y['nk'].min(), 'largest cond', max(conds))
    if case in WELL_CONDITIONED:
        assert cov == 'full' and y['nk'].min() >= 2 * points(case).shape[1] and max(conds) <= 1e4


@pytest.mark.parametrize('case', BLURRED)
def test_blurred_parameters_leave_rows_soft(case):
    y = yardstick(case)
    logr = y_estep(y['Xs'], *blurred(case))[3]
    soft = float((np.exp(logr).max(axis=1) < 0.99).mean())
    print(case, 'soft rows from blurred parameters', soft)
    assert soft > 0.02


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_have_a_clear_winner(case):
    lbs = [yardstick(case, r, 3)['lbs'][-1] for r in range(3)]
    order = np.argsort(lbs)
    print(case, 'final lower bounds', lbs, 'winner (0-based)', order[-1])
    assert lbs[order[-1]] - lbs[order[-2]] > 1e-7
    for r in range(3):
        y = yardstick(case, r, 3)
        steps = np.abs(np.diff(np.concatenate([[-np.inf], y['lbs']])))
        assert np.min(np.abs(steps - TOL)) > 1e-6 and y['converged']


def winner(case):
    return int(np.argmax([yardstick(case, r, 3)['lbs'][-1] for r in range(3)]))


@pytest.mark.parametrize('cov', ['full', 'tied'])
def test_model_selection_equals_sklearn(cov):
    mix = pytest.importorskip('sklearn.mixture')
    X = points('full_corr_k4').astype(np.float64)
    sk = mix.GaussianMixture(4, covariance_type=cov, random_state=0).fit(X)
    assert n_parameters(4, 8, cov) == sk._n_parameters()
    ours = FullGaussianMixture(4, covariance_type=cov)
    ours.n_features_in_ = 8
    ours.score = sk.score          # (bic / aic are formulas on top of score)
    assert ours._n_parameters() == sk._n_parameters()
    assert ours.bic(X) == sk.bic(X) and ours.aic(X) == sk.aic(X)
    assert n_parameters(5, 13, 'full') == 5 * 13 * 14 // 2 + 5 * 13 + 4 and n_parameters(5, 13, 'tied') == 13 * 14 // 2 + 5 * 13 + 4


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    for cov in ('diag', 'spherical', 'banded'):
        with pytest.raises(ValueError, match="'full' or 'tied'"):
            FullGaussianMixture(2, covariance_type=cov)
    assert FullGaussianMixture(2).covariance_type == 'full' and FullGaussianMixture(2).get_params()['reg_covar'] == 1e-6
    for bad in (0, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='n_components'):
            FullGaussianMixture(bad)
        with pytest.raises(ValueError, match='n_init'):
            FullGaussianMixture(2, n_init=bad)
        with pytest.raises(ValueError, match='max_iter'):
            FullGaussianMixture(2, max_iter=bad)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        FullGaussianMixture(33)
    with pytest.raises(ValueError, match='init_params'):
        FullGaussianMixture(2, init_params='zeros')
    with pytest.raises(ValueError, match='tol and reg_covar'):
        FullGaussianMixture(2, reg_covar=-1.0)
    with pytest.raises(RuntimeError, match='not fitted'):
        FullGaussianMixture(2).predict(X)
    with pytest.raises(ValueError, match='normalized'):
        FullGaussianMixture(2, weights_init=[0.5, 0.6])._check_inits(8)
    with pytest.raises(ValueError, match="'means' should have the shape"):
        FullGaussianMixture(2, means_init=np.zeros((3, 8)))._check_inits(8)
    eye = np.eye(8)
    with pytest.raises(ValueError, match=r"'full precision' should have the shape of \(2, 8, 8\)"):
        FullGaussianMixture(2, precisions_init=eye)._check_inits(8)
    with pytest.raises(ValueError, match=r"'tied precision' should have the shape of \(8, 8\)"):
        FullGaussianMixture(2, covariance_type='tied', precisions_init=np.stack([eye, eye]))._check_inits(8)
    with pytest.raises(ValueError, match='symmetric, positive-definite'):
        FullGaussianMixture(2, precisions_init=np.stack([eye, -eye]))._check_inits(8)
    skew = eye.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match='symmetric, positive-definite'):
        FullGaussianMixture(2, covariance_type='tied', precisions_init=skew)._check_inits(8)
    rs = np.random.RandomState(0)
    A = rs.normal(size=(8, 8))
    prec = A @ A.T + np.eye(8)
    P, ld = FullGaussianMixture(2, covariance_type='tied', precisions_init=prec)._check_inits(8)['prec']
    assert np.allclose(P[0] @ P[0].T, prec, rtol=1e-12) and np.array_equal(P[0], np.triu(P[0])) and np.isclose(ld[0], 0.5 * np.linalg.slogdet(prec)[1])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            FullGaussianMixture(2).fit(X)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            GF.gmm_full_sweep(X, [2, 3], covariance_type='tied')


def test_module_does_not_import_scipy_or_sklearn():
    from deep_interpolation_clustering_amd import _gmm_base
    for module in (GF, _gmm_base):
        with open(module.__file__) as f:
            assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M), module.__name__


def test_drivers_accept_full_and_tied():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    for cov in ('full', 'tied', 'diag', 'spherical'):
        assert p2.get_arguments(['--cluster_method', 'gmm', '--gmm_covariance_type', cov]).gmm_covariance_type == cov
        assert p4.get_arguments(['--cluster_method', 'gmm', '--num_clusters', '3', '--gmm_covariance_type', cov]).gmm_covariance_type == cov
    assert p2.get_arguments(['--cluster_method', 'gmm']).gmm_covariance_type == 'diag'
    assert p4.get_arguments(['--cluster_method', 'gmm', '--num_clusters', '3']).gmm_covariance_type == 'diag'


NAMES = {'dic_gmm_full_workspace', 'dic_gmm_full_em_iter', 'dic_gmm_full_estep', 'dic_gmm_full_mstep', 'dic_gmm_full_factor'}


def test_header_and_signatures_agree():
    assert NAMES <= set(N.header_symbols()) and NAMES <= set(N.SIGNATURES)
    with open(N.HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name in NAMES:
        decl = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(decl.split(',')) == len(N.SIGNATURES[name][1]), name


def a256(words):
    return (8 * words + 255) // 256 * 256


def slabs(n, m):
    return max(1, min((n + 255) // 256, (128 + m - 1) // m))


def workspace_bytes(n, d, k, runs, cov):
    """The header's formula."""
    blocks, kc = min(256, (n + 63) // 64), k if cov == 2 else 1
    slab = runs * k * slabs(n, k) * d * d if cov == 2 else slabs(n, 1) * d * d
    return a256(runs * n * k) + a256(runs * blocks * (k * (d + 1) + 1)) + a256(runs * k) + a256(slab) + a256(runs * kc * d * d)


def test_workspace_formula(lib):
    for args in ((1000, 256, 4, 2, 2), (1000, 256, 4, 2, 3), (75000, 256, 10, 10, 2), (75000, 256, 32, 1, 3), (2, 4, 1, 1, 2), (257, 16, 3, 3, 2),
                 (4100, 8, 32, 1, 2), (16400, 200, 7, 2, 3)):
        assert lib.dic_gmm_full_workspace(*args) == workspace_bytes(*args), args
    for bad in ((1, 256, 4, 2, 2), (1 << 30, 256, 4, 2, 2), (1000, 260, 4, 2, 2), (1000, 0, 4, 2, 2), (1000, 256, 0, 2, 2), (1000, 256, 33, 2, 2),
                (1000, 256, 4, 0, 2), (1000, 256, 4, 2, 0), (1000, 256, 4, 2, 1), (1000, 256, 4, 2, 4)):
        assert lib.dic_gmm_full_workspace(*bad) == 0
    assert slabs(255, 1) == 1 and slabs(257, 1) == 2 and slabs(4100, 3) == 17 and slabs(75000, 10) == 13 and slabs(75000, 32) == 4


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_gmm_full_workspace(1000, 256, 4, 2, 2)

    def em(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=2, reg=1e-6, shift=fake, w=fake, mu=fake, C=fake, P=fake, ld=fake, T=None, status=fake,
           lbs=fake, stride=100, work=fake, nbytes=ws):
        return lib.dic_gmm_full_em_iter(X, ldx, n, d, d0, k, runs, cov, reg, shift, w, mu, C, P, ld, T, status, lbs, stride, work, nbytes, None)

    def es(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, cov=2, shift=fake, w=fake, mu=fake, P=fake, ld=fake, work=fake, nbytes=ws):
        return lib.dic_gmm_full_estep(X, ldx, n, d, d0, k, cov, shift, w, mu, P, ld, None, None, None, None, work, nbytes, None)

    def ms(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=2, reg=1e-6, shift=fake, labels=fake, resp=None, T=None, w=fake, mu=fake, C=fake, P=fake,
           ld=fake, status=fake, work=fake, nbytes=ws):
        return lib.dic_gmm_full_mstep(X, ldx, n, d, d0, k, runs, cov, reg, shift, labels, resp, T, 1, w, mu, C, P, ld, status, work, nbytes, None)

    for call in (em, es, ms):
        for kw in ({'X': None}, {'shift': None}, {'w': None}, {'mu': None}, {'P': None}, {'ld': None}, {'work': None}):
            assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
        assert call(n=1) == -1 and b'at least 2' in lib.dic_last_error_string()
        assert call(n=0) == -1 and call(ldx=128) == -1 and call(d=0) == -1 and call(k=0) == -1 and call(d0=0) == -1 and call(d0=257) == -1
        for cov in (0, 1, 4, -1):
            assert call(cov=cov) == -1 and b'cov_type' in lib.dic_last_error_string()
        assert call(ldx=252, d=250, d0=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
        assert call(k=33) == -2 and b'at most 32 components' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
        assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(work=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(nbytes=1000) == -3 and b'workspace' in lib.dic_last_error_string()
    for call in (em, ms):
        for kw in ({'C': None}, {'status': None}, {'runs': 0}, {'reg': -1.0}):
            assert call(**kw) == -1
        assert call(cov=3) == -1 and b'total scatter' in lib.dic_last_error_string()          # (tied without T)
    assert em(lbs=None) == -1 and em(stride=0) == -1
    assert ms(labels=None) == -1 and ms(resp=fake) == -1 and b'exactly one' in lib.dic_last_error_string()

    def fa(C=fake, runs=2, mats=4, d=256, d0=256, P=fake, ld=fake, status=fake, work=fake, nbytes=2 * 4 * 256 * 256 * 8):
        return lib.dic_gmm_full_factor(C, runs, mats, d, d0, P, ld, status, work, nbytes, None)

    for kw in ({'C': None}, {'P': None}, {'ld': None}, {'status': None}, {'work': None}, {'runs': 0}, {'mats': 0}, {'d': 0}, {'d0': 0}, {'d0': 257}):
        assert fa(**kw) == -1
    assert fa(d=260, d0=260) == -2 and fa(d=250, d0=250) == -2 and fa(mats=33) == -2 and fa(work=ctypes.c_void_p((1 << 20) + 8)) == -2
    assert fa(nbytes=2 * 4 * 256 * 256 * 8 - 1) == -3 and b'workspace' in lib.dic_last_error_string()


def test_gmm_full_kernels_do_not_spill_to_scratch():
    """The E-step keeps a 16 x 256 tile of differences in registers per wave: a register that went to scratch memory would be paid on every matrix
    instruction.  Require ScratchSize == 0 and no vector-register spills for every kernel of dic_gmm_full.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_gmm_full.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    assert sum('gf_pass_kernel' in n for n in names) == 4
    for kernel in ('gf_resp_kernel', 'gf_scatter_kernel', 'gf_params_kernel', 'gf_cov_kernel', 'gf_factor_kernel', 'gf_sum_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
