"""Bayesian Gaussian mixtures, host side (no GPU): the numpy f64 yardstick of csrc/dic_bgmm.hip's definition against sklearn, the conditions the GPU tests
(tests/test_gpu_bgmm.py) rely on, the reference of the special functions, the ABI's and the Python argument errors, and the register use of the kernels."""
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
from deep_interpolation_clustering_amd import bgmm as B
from deep_interpolation_clustering_amd.bgmm import BayesianGaussianMixture

import test_gmm_host as G
from test_gmm_host import REG, TOL, blobs, one_hot, rel

DP, DD = 'dirichlet_process', 'dirichlet_distribution'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def _k12():
    return blobs(1030, 8, 6)


def _k9():
    return blobs(4100, 12, 12, n_centers=9, spread=1.5)


def _sph8():
    return blobs(1030, 8, 11, n_centers=4, spread=1.2)


# name -> (points, K, covariance type, weight prior type).  The GPU tests run on exactly these.
CASES = {
    'n2_k1': (lambda: blobs(2, 4, 1), 1, 'diag', DP),
    'n17_k2': (lambda: blobs(17, 12, 3), 2, 'diag', DP),
    'n257_d256_k5': (lambda: blobs(257, 256, 5), 5, 'diag', DP),
    'n1030_k12': (_k12, 12, 'diag', DP),
    'n4100_k32': (lambda: blobs(4100, 8, 13, n_centers=7, spread=4.0), 32, 'diag', DP),
    'overlap_k9': (_k9, 9, 'diag', DP),
    'sph_k8': (_sph8, 8, 'spherical', DP),
    'sph_d256_k6': (lambda: blobs(1500, 256, 14, n_centers=6, spread=0.15), 6, 'spherical', DP),
    'dup_k3': (G._dup, 3, 'diag', DP),
    'strided': (lambda: blobs(257, 8, 10), 3, 'diag', DP),
    'd13': (lambda: blobs(300, 13, 15), 3, 'diag', DP),
    'n1030_k12_dd': (_k12, 12, 'diag', DD),
    'overlap_k9_dd': (_k9, 9, 'diag', DD),
    'sph_k8_dd': (_sph8, 8, 'spherical', DD),
}
N_INIT_CASES = ['n1030_k12', 'sph_k8']
# the components with weight > 1 / N of the cases that must empty some
N_HEAVY = {'n1030_k12': 5, 'n4100_k32': 7, 'sph_d256_k6': 1}

# The largest relative deviation (max |a - b| / max |b| per array: lower bounds, weights, means, covariances, degrees of freedom, mean precisions) measured
# on the CPU, per case, between (a) the yardstick and sklearn 1.7.2 started from the same initial labels, and (b) the yardstick with numpy's pairwise sums
# and with strictly sequential sums.  The host tests hold the yardstick to 4 x these figures; the GPU tests allow 16 x the larger of the two, and never less
# than 1e-13 (the rule of the plain mixtures, test_gmm_host.py).  Measured with numpy 2.2 / sklearn 1.7.2 on x86-64.
BASE = {
    'n2_k1': (7.18e-16, 0.0), 'n17_k2': (3.34e-16, 1.12e-16), 'n257_d256_k5': (1.92e-14, 5.27e-14), 'n1030_k12': (8.38e-14, 1.22e-13),
    'n4100_k32': (2.82e-14, 3.42e-13), 'overlap_k9': (1.97e-13, 2.24e-13), 'sph_k8': (3.18e-15, 1.94e-15), 'sph_d256_k6': (5.31e-15, 1.21e-14),
    'dup_k3': (1.01e-15, 6.54e-15), 'strided': (1.65e-15, 8.23e-15), 'd13': (1.48e-15, 3.58e-15), 'n1030_k12_dd': (8.38e-14, 1.18e-13),
    'overlap_k9_dd': (1.70e-13, 2.94e-13), 'sph_k8_dd': (2.84e-15, 1.93e-15),
}

# The largest deviation |a - b| / max(1, |b|) of scipy.special.digamma and gammaln from the long-double references below over special_arguments(),
# measured with scipy on x86-64 (80-bit long double).  Where |psi| < 1 -- around its root at 1.4616.. -- and where |lgamma| < 1 -- around its roots at 1 and
# 2 -- the deviation is absolute: a relative one is unbounded at a root.  The GPU test allows the device functions 8 x these figures.
SCIPY_DIGAMMA_DEV = 2.98e-16
SCIPY_GAMMALN_DEV = 4.02e-16


def fit_rtol(case):
    """The relative tolerance of a whole fit on the device against the yardstick (see BASE)."""
    return max(16.0 * max(BASE[case]), 1e-13)


@functools.lru_cache(maxsize=None)
def points(case):
    X = CASES[case][0]()
    X.setflags(write=False)
    return X


_sum = G._sum


class Model(dict):
    """The variational posterior of the yardstick: kappa, m (shifted), nu, v (K, D), conc ((a, b) or alpha), and what follows from them."""
    __getattr__ = dict.__getitem__


def y_priors(X64, K, cov_type):
    s0 = np.var(X64, axis=0, ddof=1)
    return dict(g0=1.0 / K, k0=1.0, nu0=float(X64.shape[1]), s0=s0 if cov_type == 'diag' else np.full(X64.shape[1], s0.mean()))


def y_mstep(Xs, r, cov_type, prior_type, pri, reg=REG, seq=False):
    """The M-step of the definition from responsibilities r: a Model with every constant of the next E-step."""
    from scipy.special import digamma, gammaln
    D = Xs.shape[1]
    nk = _sum(r, 0, seq) + 10.0 * np.finfo(np.float64).eps
    xb = _sum(r[:, :, None] * Xs[:, None, :], 0, seq) / nk[:, None]
    s = _sum(r[:, :, None] * (Xs * Xs)[:, None, :], 0, seq) / nk[:, None] - xb * xb + reg
    dd = xb * xb          # (m0 = 0 in shifted coordinates)
    if cov_type == 'spherical':
        s = np.repeat(_sum(s, 1, seq)[:, None] / D, D, axis=1)
        dd = np.repeat(_sum(dd, 1, seq)[:, None] / D, D, axis=1)
    kap = pri['k0'] + nk
    nu = pri['nu0'] + nk
    m = (nk[:, None] * xb) / kap[:, None]
    v = (pri['s0'][None, :] + nk[:, None] * (s + (pri['k0'] / kap)[:, None] * dd)) / nu[:, None]
    if prior_type == DP:
        conc = (1.0 + nk, pri['g0'] + np.hstack((np.cumsum(nk[::-1])[-2::-1], 0)))
        pab = digamma(conc[0] + conc[1])
        elogpi = digamma(conc[0]) - pab + np.hstack((0, np.cumsum(digamma(conc[1]) - pab)[:-1]))
    else:
        conc = pri['g0'] + nk
        elogpi = digamma(conc) - digamma(_sum(conc, 0, seq))
    ell = -0.5 * _sum(np.log(v), 1, seq) - 0.5 * D * np.log(nu)
    half = 0.5 * (nu[:, None] - np.arange(D)[None, :])
    loglam = D * np.log(2.0) + _sum(digamma(half), 1, seq)
    lgsum = _sum(gammaln(half), 1, seq)
    lc = elogpi - 0.5 * D * np.log(2.0 * np.pi) + ell + 0.5 * (loglam - D / kap)
    return Model(nk=nk, kappa=kap, m=m, nu=nu, v=v, conc=conc, elogpi=elogpi, ell=ell, loglam=loglam, lgsum=lgsum, lc=lc)


def y_estep(Xs, p, seq=False):
    """The E-step of the definition on shifted f64 points: (M, log p, lse, log r)."""
    diff = Xs[:, None, :] - p.m[None, :, :]
    M = _sum(diff * diff / p.v[None, :, :], 2, seq)
    logp = p.lc[None, :] - 0.5 * M
    mx = logp.max(axis=1)
    lse = mx + np.log(_sum(np.exp(logp - mx[:, None]), 1, seq))
    return M, logp, lse, logp - lse[:, None]


def y_entropy(logr, seq=False):
    """sum_i sum_k r log r, the rows' sums first, the product only where log r is finite."""
    r = np.exp(logr)
    t = np.where(np.isfinite(logr), r * np.where(np.isfinite(logr), logr, 0.0), 0.0)
    return _sum(_sum(t, 1, seq), 0, seq)


def y_lower_bound(logr, p, prior_type, D, seq=False):
    from scipy.special import betaln, gammaln
    logw = -(p.nu * p.ell + p.nu * D * 0.5 * np.log(2.0) + p.lgsum)
    if prior_type == DP:
        log_norm = -_sum(betaln(p.conc[0], p.conc[1]), 0, seq)
    else:
        log_norm = gammaln(_sum(p.conc, 0, seq)) - _sum(gammaln(p.conc), 0, seq)
    return -y_entropy(logr, seq) - _sum(logw, 0, seq) - log_norm - 0.5 * D * _sum(np.log(p.kappa), 0, seq)


def y_weights(prior_type, conc):
    """sklearn's ``_set_parameters``: stick breaking for the process."""
    if prior_type == DP:
        total = conc[0] + conc[1]
        w = conc[0] / total * np.hstack((1, np.cumprod((conc[1] / total)[:-1])))
        return w / np.sum(w)
    return conc / np.sum(conc)


def y_fit(X, K, cov_type, prior_type, labels0, tol=TOL, reg=REG, max_iter=100, seq=False):
    """The variational EM of the definition from the one-hot responsibilities of ``labels0``.  A dict: the shift c, the shifted points, the priors, the
    initial and the final Model, the first E-step (M, log p, lse, log r), the Model after the first M-step, the lower bounds, n_iter, converged, and the final
    E-step's log p, log r, lse and labels."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    c = X64.mean(axis=0)
    Xs = X64 - c
    D = Xs.shape[1]
    pri = y_priors(X64, K, cov_type)
    p = y_mstep(Xs, one_hot(labels0, K), cov_type, prior_type, pri, reg, seq)
    out = {'c': c, 'Xs': Xs, 'priors': pri, 'init': p, 'lbs': [], 'converged': False}
    lb = -np.inf
    for it in range(1, max_iter + 1):
        prev = lb
        M, logp, lse, logr = y_estep(Xs, p, seq)
        p = y_mstep(Xs, np.exp(logr), cov_type, prior_type, pri, reg, seq)
        lb = y_lower_bound(logr, p, prior_type, D, seq)
        if it == 1:
            out['first'] = (M, logp, lse, logr, p, lb)
        out['lbs'].append(lb)
        if abs(lb - prev) < tol:
            out['converged'] = True
            break
    out['n_iter'] = it
    out['final'] = p
    out['lbs'] = np.array(out['lbs'])
    _, logp, lse, logr = y_estep(Xs, p, seq)
    out['logp'], out['logr'], out['lse'], out['labels'] = logp, logr, lse, logp.argmax(axis=1)
    out['weights'] = y_weights(prior_type, p.conc)
    out['active'] = np.unique(out['labels'])
    return out


@functools.lru_cache(maxsize=None)
def initial_labels(case, n_init=1):
    """sklearn's KMeans(n_init=1) on the f64 points, ``n_init`` fits in a row from one RandomState(5): (n_init, N)."""
    sk = pytest.importorskip('sklearn.cluster')
    X, K = points(case), CASES[case][1]
    rs = np.random.RandomState(5)
    return np.stack([sk.KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X.astype(np.float64)).labels_ for _ in range(n_init)])


@functools.lru_cache(maxsize=None)
def yardstick(case, restart=0, n_init=1, seq=False, max_iter=100):
    _, K, cov, prior = CASES[case]
    return y_fit(points(case), K, cov, prior, initial_labels(case, n_init)[restart], seq=seq, max_iter=max_iter)


def cov_of(v, cov_type):
    return v if cov_type == 'diag' else v[:, 0]


@functools.lru_cache(maxsize=None)
def sklearn_fit(case):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov, prior = CASES[case]
    labels0 = initial_labels(case)[0]

    class FromLabels(mix.BayesianGaussianMixture):
        def _initialize_parameters(self, X, random_state):          # (the same initial labels: one-hot responsibilities through sklearn's _initialize)
            self._initialize(X, one_hot(labels0, K))

    return FromLabels(n_components=K, covariance_type=cov, tol=TOL, reg_covar=REG, max_iter=100, weight_concentration_prior_type=prior).fit(
        points(case).astype(np.float64))


def fit_arrays(y, cov_type):
    """(lower bounds, weights, means, covariances, degrees of freedom, mean precisions) of a yardstick fit, as sklearn names them."""
    p = y['final']
    return y['lbs'], y['weights'], p.m + y['c'], cov_of(p.v, cov_type), p.nu, p.kappa


def deviations(case, other):
    """The largest relative deviation of ``other`` = (lbs, weights, means, cov, dof, mean precision) from the yardstick's arrays."""
    return max(rel(a, b) for a, b in zip(other, fit_arrays(yardstick(case), CASES[case][2])))


@pytest.mark.parametrize('case', list(CASES))
def test_yardstick_equals_sklearn(case):
    sk = sklearn_fit(case)
    y = yardstick(case)
    assert sk.n_iter_ == y['n_iter'] and sk.converged_ == y['converged'] and y['converged']
    assert 2 <= y['n_iter'] <= 70
    assert np.array_equal(sk.predict(points(case).astype(np.float64)), y['labels'])
    dev = deviations(case, (sk.lower_bounds_, sk.weights_, sk.means_, sk.covariances_, sk.degrees_of_freedom_, sk.mean_precision_))
    print(case, 'n_iter', y['n_iter'], 'active', len(y['active']), 'yardstick vs sklearn', dev)
    assert dev <= max(4.0 * BASE[case][0], 1e-14)
    if case in N_HEAVY:
        assert int((y['weights'] > 1.0 / len(points(case))).sum()) == N_HEAVY[case]
    if case == 'overlap_k9':
        soft = float((np.exp(y['logr']).max(axis=1) < 0.99).mean())
        print(case, 'rows with a largest responsibility below 0.99:', soft)
        assert soft > 0.02


@pytest.mark.parametrize('case', list(CASES))
def test_pairwise_and_sequential_sums_agree(case):
    y, s = yardstick(case), yardstick(case, seq=True)
    assert s['n_iter'] == y['n_iter'] and np.array_equal(s['labels'], y['labels'])
    dev = deviations(case, fit_arrays(s, CASES[case][2]))
    print(case, 'pairwise vs sequential', dev)
    assert dev <= max(4.0 * BASE[case][1], 1e-14)


def _conditions(y, K):
    steps = np.abs(np.diff(np.concatenate([[-np.inf], y['lbs']])))
    margin = float(np.min(np.abs(steps - TOL)))
    assert margin > 0.01 * TOL, steps
    gap = np.inf
    if K > 1:
        for logp in (y['first'][1], y['logp']):          # (the first E-step, which the one-pass test checks, and the final one)
            top = np.sort(logp, axis=1)
            gap = min(gap, float(np.min(top[:, -1] - top[:, -2])))
        assert gap > 1e-9
    return margin, gap


@pytest.mark.parametrize('case', list(CASES))
def test_cases_meet_the_conditions(case):
    """What the GPU tests rely on: clear stopping decisions and clear labels.  (A change of seed must keep these.)"""
    margin, gap = _conditions(yardstick(case), CASES[case][1])
    print(case, 'stop margin', margin, 'label gap', gap)


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_have_a_clear_winner(case):
    lbs = [yardstick(case, r, 3)['lbs'][-1] for r in range(3)]
    order = np.argsort(lbs)
    print(case, 'final lower bounds', lbs, 'winner (0-based)', order[-1])
    assert lbs[order[-1]] - lbs[order[-2]] > 1e-7 * abs(lbs[order[-1]])
    for r in range(3):
        y = yardstick(case, r, 3)
        _conditions(y, CASES[case][1])
        assert y['converged']


def winner(case):
    return int(np.argmax([yardstick(case, r, 3)['lbs'][-1] for r in range(3)]))


# -- the special functions ------------------------------------------------------------------------------------------------------------------------------
def special_arguments():
    """4 096 arguments spaced geometrically in [0.5, 1e6] and the half-integers 0.5, 1.0, .. 200."""
    return np.concatenate([np.geomspace(0.5, 1e6, 4096), 0.5 * np.arange(1, 401)])


def ref_digamma(x):
    """psi(x), x > 0, in long double: 40 terms of the recurrence psi(x) = psi(x + 1) - 1 / x, then the asymptotic series at x + 40."""
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    s = sum(L(1) / (x + L(i)) for i in range(40))
    y = x + L(40)
    r2 = L(1) / (y * y)
    ser = r2 * (L(1) / 12 - r2 * (L(1) / 120 - r2 * (L(1) / 252 - r2 * (L(1) / 240 - r2 * (L(1) / 132 - r2 * (L(691) / 32760 - r2 * (L(1) / 12)))))))
    return np.log(y) - L(1) / (2 * y) - ser - s


def ref_gammaln(x):
    """lgamma(x), x > 0, in long double: lgamma(x) = lgamma(x + 40) - sum_i log(x + i), Stirling's series at x + 40."""
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    s = sum(np.log(x + L(i)) for i in range(40))
    y = x + L(40)
    r, r2 = L(1) / y, L(1) / (y * y)
    ser = r * (L(1) / 12 - r2 * (L(1) / 360 - r2 * (L(1) / 1260 - r2 * (L(1) / 1680 - r2 * (L(1) / 1188 - r2 * (L(691) / 360360 - r2 * (L(1) / 156)))))))
    half_log_2pi = np.log(8 * np.arctan(L(1))) / 2
    return (y - L(1) / 2) * np.log(y) - y + half_log_2pi + ser - s


def special_dev(got, ref):
    """max |got - ref| / max(1, |ref|), in long double."""
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(got - ref) / np.maximum(1, np.abs(ref))))


def test_scipy_special_functions_against_long_double():
    sp = pytest.importorskip('scipy.special')
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip('long double is no wider than double here')
    x = special_arguments()
    assert abs(float(ref_digamma(np.longdouble(1)) + np.longdouble('0.57721566490153286060651209'))) < 1e-18          # psi(1) = -gamma
    assert abs(float(ref_gammaln(np.longdouble(0.5)) - np.log(np.sqrt(4 * np.arctan(np.longdouble(1)))))) < 1e-17          # lgamma(1/2) = log sqrt(pi); 40 logarithms are summed
    dg, lg = special_dev(sp.digamma(x), ref_digamma(x)), special_dev(sp.gammaln(x), ref_gammaln(x))
    print('scipy digamma', dg, 'scipy gammaln', lg)
    assert dg <= SCIPY_DIGAMMA_DEV and lg <= SCIPY_GAMMALN_DEV
    assert SCIPY_DIGAMMA_DEV <= 2.0 ** -50 and SCIPY_GAMMALN_DEV <= 2.0 ** -50          # (a few units in the last place: the figures are no licence)


# -- arguments ------------------------------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    for cov in ('full', 'tied'):
        with pytest.raises(NotImplementedError, match='matrix-core'):
            BayesianGaussianMixture(2, covariance_type=cov)
    with pytest.raises(ValueError, match="'diag' or 'spherical'"):
        BayesianGaussianMixture(2, covariance_type='banded')
    with pytest.raises(NotImplementedError, match='warm_start'):
        BayesianGaussianMixture(2, warm_start=True)
    with pytest.raises(ValueError, match='n_components'):
        BayesianGaussianMixture(0)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        BayesianGaussianMixture(33)
    assert not hasattr(BayesianGaussianMixture(2), 'bic') and not hasattr(BayesianGaussianMixture(2), 'aic')
    assert BayesianGaussianMixture(2).covariance_type == 'diag'
    with pytest.raises(RuntimeError, match='not fitted'):
        BayesianGaussianMixture(2).predict(X)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            BayesianGaussianMixture(2).fit(X)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            B.bgmm_sweep(X, [0.1, 1.0], n_components=3)


def _sklearn_message(**kw):
    mix = pytest.importorskip('sklearn.mixture')
    with pytest.raises(ValueError) as e:
        mix.BayesianGaussianMixture(n_components=2, **kw).fit(np.random.RandomState(0).normal(size=(20, 3)))
    return str(e.value)


@pytest.mark.parametrize('kw', [dict(weight_concentration_prior=-1.0), dict(weight_concentration_prior=0), dict(mean_precision_prior=0.0),
                                dict(degrees_of_freedom_prior=-1.0), dict(covariance_type='spherical', covariance_prior=-1.0),
                                dict(degrees_of_freedom_prior=2.0), dict(degrees_of_freedom_prior=1.5), dict(mean_prior=[0.0, 0.0]),
                                dict(covariance_type='diag', covariance_prior=[1.0, 1.0]), dict(covariance_type='diag', covariance_prior=[1.0, -1.0, 1.0])],
                         ids=lambda kw: '-'.join('%s=%s' % kv for kv in kw.items()))
def test_bad_priors_raise_sklearns_messages(kw):
    """The constructor refuses what sklearn's parameter constraints refuse at fit; ``_check_priors`` what sklearn's ``_check_parameters`` refuses."""
    want = _sklearn_message(**kw)
    with pytest.raises(ValueError) as e:
        BayesianGaussianMixture(n_components=2, **kw)._check_priors(3)
    assert str(e.value) == want


def test_prior_type_message_and_defaults():
    with pytest.raises(ValueError, match="'weight_concentration_prior_type' parameter of BayesianGaussianMixture must be a str among"):
        BayesianGaussianMixture(2, weight_concentration_prior_type='x')
    m = BayesianGaussianMixture(4, degrees_of_freedom_prior=2.5)
    m._check_priors(3)          # (nu0 > D0 - 1 = 2)
    assert m.degrees_of_freedom_prior_ == 2.5 and m.weight_concentration_prior_ == 0.25 and m.mean_precision_prior_ == 1.0
    m = BayesianGaussianMixture(4)
    m._check_priors(7)
    assert m.degrees_of_freedom_prior_ == 7


def test_module_does_not_import_scipy_or_sklearn():
    with open(B.__file__) as f:
        assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M)


def test_drivers_accept_bgmm():
    from deep_interpolation_clustering_amd import _cluster_cli as cli
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    assert cli.METHODS[-1] == 'bgmm' and 'bgmm' in p2.BRANCHES and 'bgmm' in p4.Cluster.BRANCHES
    a = p2.get_arguments(['--cluster_method', 'bgmm', '--k_max', '5', '--bgmm_concentration', '0.01', '1', '--bgmm_prior_type', 'dirichlet_distribution'])
    assert a.cluster_method == 'bgmm' and a.bgmm_concentration == [0.01, 1.0] and a.bgmm_prior_type == DD
    assert p2.get_arguments(['--cluster_method', 'bgmm']).bgmm_concentration is None
    a = p4.get_arguments(['--cluster_method', 'bgmm', '--num_clusters', '6', '--bgmm_concentration', '0.5'])
    assert a.cluster_method == 'bgmm' and a.bgmm_concentration == 0.5 and a.bgmm_prior_type == DP


def test_header_and_signatures_agree():
    names = {'dic_bgmm_workspace', 'dic_bgmm_init', 'dic_bgmm_em_iter', 'dic_bgmm_estep', 'dic_bgmm_special_probe'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    with open(N.HEADER_PATH) as f:
        assert int(re.search(r'#define DIC_BGMM_COMP_WORDS (\d+)', f.read()).group(1)) == B.COMP_WORDS


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_bgmm_workspace(1000, 256, 4, 2)
    assert ws >= 2 * 63 * 8 * (4 * 513 + 2)
    for bad in ((1, 256, 4, 2), (1 << 30, 256, 4, 2), (1000, 260, 4, 2), (1000, 0, 4, 2), (1000, 256, 0, 2), (1000, 256, 33, 2), (1000, 256, 4, 0)):
        assert lib.dic_bgmm_workspace(*bad) == 0
    assert lib.dic_bgmm_workspace(75000, 256, 32, 1) == 256 * 8 * (32 * 513 + 2)

    def ini(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=0, prior=0, reg=1e-6, g0=0.25, k0=1.0, nu0=256.0, shift=fake, m0=fake, s0=fake,
            labels=fake, resp=None, mu=fake, var=fake, comp=fake, work=fake, nbytes=ws):
        return lib.dic_bgmm_init(X, ldx, n, d, d0, k, runs, cov, prior, reg, g0, k0, nu0, shift, m0, s0, labels, resp, mu, var, comp, work, nbytes, None)

    def em(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=0, prior=0, reg=1e-6, g0=0.25, k0=1.0, nu0=256.0, shift=fake, m0=fake, s0=fake, mu=fake,
           var=fake, comp=fake, status=fake, lbs=fake, stride=100, work=fake, nbytes=ws):
        return lib.dic_bgmm_em_iter(X, ldx, n, d, d0, k, runs, cov, prior, reg, g0, k0, nu0, shift, m0, s0, mu, var, comp, status, lbs, stride, work, nbytes,
                                    None)

    def es(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, shift=fake, lc=fake, mu=fake, var=fake, work=fake, nbytes=ws):
        return lib.dic_bgmm_estep(X, ldx, n, d, d0, k, shift, lc, mu, var, None, None, None, None, work, nbytes, None)

    for call in (ini, em, es):
        for kw in ({'X': None}, {'shift': None}, {'mu': None}, {'var': None}, {'work': None}):
            assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
        assert call(n=1) == -1 and b'at least 2' in lib.dic_last_error_string()
        assert call(n=0) == -1 and call(ldx=128) == -1 and call(d=0) == -1 and call(k=0) == -1 and call(d0=0) == -1 and call(d0=257) == -1
        assert call(ldx=252, d=250, d0=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
        assert call(k=33) == -2 and b'at most 32 components' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
        assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(work=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(nbytes=1000) == -3 and b'workspace' in lib.dic_last_error_string()
    assert es(lc=None) == -1
    for call in (ini, em):
        for kw in ({'m0': None}, {'s0': None}, {'comp': None}, {'runs': 0}, {'cov': 2}, {'cov': -1}, {'prior': 2}, {'prior': -1}, {'reg': -1.0}):
            assert call(**kw) == -1
        for kw in ({'g0': 0.0}, {'g0': -1.0}, {'g0': float('nan')}, {'k0': 0.0}, {'k0': float('inf')}, {'nu0': 255.0}, {'nu0': float('nan')},
                   {'d0': 200, 'nu0': 199.0}):
            assert call(**kw) == -1 and b'priors' in lib.dic_last_error_string()
    for kw in ({'status': None}, {'lbs': None}, {'stride': 0}):
        assert em(**kw) == -1
    for kw in ({'labels': None}, {'resp': fake}):
        assert ini(**kw) == -1
    assert b'exactly one' in lib.dic_last_error_string()
    assert lib.dic_bgmm_special_probe(None, 4, fake, fake) == -1 and lib.dic_bgmm_special_probe(fake, 4, None, None) == -1
    assert lib.dic_bgmm_special_probe(fake, 0, fake, fake) == -1


def test_bgmm_kernels_do_not_spill_to_scratch():
    """The pass keeps 64 f64 accumulators per thread, as the plain mixture's: require ScratchSize == 0 and no vector-register spills for every kernel of
    dic_bgmm.hip.  (Scalar registers parked in lanes of a vector register are reported as SGPR spills; that is not scratch.)"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_bgmm.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    assert sum('bg_pass_kernel' in n for n in names) == 4
    for kernel in ('bg_reduce_kernel', 'bg_finish_kernel', 'bg_sum_kernel', 'bg_probe_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
