"""Gaussian mixtures, host side (no GPU): the numpy f64 yardstick of csrc/dic_gmm.hip's definition against sklearn, the conditions the GPU tests
(tests/test_gpu_gmm.py) rely on, bic / aic, the ABI's and the Python argument errors, and the register use of the kernels."""
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
from deep_interpolation_clustering_amd import gmm as G
from deep_interpolation_clustering_amd.gmm import GaussianMixture, n_parameters

import test_ward_host as TW

TOL, REG = 1e-3, 1e-6          # sklearn's defaults, used by every case
EPS = 2.0 ** -53


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def blobs(n, d, seed, n_centers=5, spread=6.0):
    """test_ward_host.blobs with the centres' sigma as an argument; the default gives the same points."""
    rs = np.random.RandomState(seed)
    centers = rs.normal(0.0, spread, size=(n_centers, d))
    return (centers[rs.randint(n_centers, size=n)] + rs.normal(0.0, 1.0, size=(n, d))).astype(np.float32)


def _dup():
    X = blobs(200, 12, 7)
    X[160:] = X[:40]
    return X


def _overlap_k4():
    return blobs(1030, 8, 11, n_centers=4, spread=1.2)


def _overlap_d256():
    return blobs(1500, 256, 14, n_centers=6, spread=0.15)


# name -> (points, K, covariance type).  The GPU tests run on exactly these.
CASES = {
    'n2_k1': (lambda: blobs(2, 4, 1), 1, 'diag'),
    'n17_k2': (lambda: blobs(17, 12, 3), 2, 'diag'),
    'n255_k3': (lambda: blobs(255, 64, 4), 3, 'diag'),
    'n257_d256_k5': (lambda: blobs(257, 256, 5), 5, 'diag'),
    'n1030_k4': (lambda: blobs(1030, 8, 6), 4, 'diag'),
    'n4100_k7': (lambda: blobs(4100, 8, 8, n_centers=7), 7, 'diag'),
    'overlap_k4': (_overlap_k4, 4, 'diag'),
    'overlap_k9': (lambda: blobs(4100, 12, 12, n_centers=9, spread=1.5), 9, 'diag'),
    'overlap_k32': (lambda: blobs(4100, 8, 13, n_centers=32, spread=2.0), 32, 'diag'),
    'overlap_d256_k6': (_overlap_d256, 6, 'diag'),
    'sph_k4': (_overlap_k4, 4, 'spherical'),
    'sph_d256_k5': (_overlap_d256, 5, 'spherical'),
    'same_k1': (lambda: np.tile(blobs(1, 4, 9), (131, 1)), 1, 'diag'),
    'dup_k3': (_dup, 3, 'diag'),
    'strided': (lambda: blobs(257, 8, 10), 3, 'diag'),
    'd13': (lambda: blobs(300, 13, 15), 3, 'diag'),
}
OVERLAP = ['overlap_k4', 'overlap_k9', 'overlap_k32', 'overlap_d256_k6', 'sph_k4', 'sph_d256_k5']
N_INIT_CASES = ['overlap_k4', 'overlap_k32', 'sph_k4']

# The largest relative deviation (max |a - b| / max |b| per array: lower bounds, weights, means, variances) measured on the CPU, per case, between (a) the
# yardstick and sklearn 1.7.2 started from the same parameters, and (b) the yardstick with numpy's pairwise sums and with strictly sequential sums.  The GPU
# tests allow 16 x the larger of the two, and never less than 1e-13.  Measured with numpy 2.2 / sklearn 1.7.2 on x86-64; test_yardstick_equals_sklearn and
# test_pairwise_and_sequential_sums_agree hold the yardstick to 4 x these figures.
BASE = {
    'n2_k1': (1.08e-15, 0.0), 'n17_k2': (6.79e-16, 2.26e-16), 'n255_k3': (1.87e-15, 4.97e-15), 'n257_d256_k5': (1.01e-13, 3.38e-13),
    'n1030_k4': (2.15e-14, 2.78e-14), 'n4100_k7': (1.33e-12, 3.71e-12), 'overlap_k4': (7.23e-15, 9.13e-15), 'overlap_k9': (2.16e-13, 2.52e-13),
    'overlap_k32': (1.19e-13, 1.93e-13), 'overlap_d256_k6': (2.79e-14, 1.55e-14), 'sph_k4': (1.34e-15, 2.01e-15), 'sph_d256_k5': (1.40e-14, 1.29e-14),
    'same_k1': (7.11e-9, 2.22e-15), 'dup_k3': (1.02e-15, 6.67e-15), 'strided': (3.76e-15, 9.41e-15), 'd13': (1.25e-15, 3.64e-15),
}
# same_k1: sklearn, which does not shift, loses 7e-9 of the lower bound on identical rows.  The blob cases whose clusters lie far from the common mean lose up to
# 4e-12 of a variance either way: v = E[x'^2] - mu'^2 cancels two numbers of several hundred, and the order of the sum over the rows decides their last bits.


def fit_rtol(case):
    """The relative tolerance of a whole fit on the device against the yardstick (see BASE)."""
    return max(16.0 * max(BASE[case]), 1e-13)


@functools.lru_cache(maxsize=None)
def points(case):
    X = CASES[case][0]()
    X.setflags(write=False)
    return X


def _sum(a, axis, seq):
    """numpy's pairwise sum -- along a contiguous last axis: numpy adds the slices of any other axis one after the other -- or the strictly sequential one."""
    if seq:
        return np.take(np.cumsum(a, axis=axis), -1, axis=axis)
    return np.ascontiguousarray(np.moveaxis(a, axis, -1)).sum(axis=-1)


def y_estep(Xs, w, mu, var, seq=False):
    """The E-step of the definition on shifted f64 points: (M, log p, lse, log r)."""
    diff = Xs[:, None, :] - mu[None, :, :]
    M = _sum(diff * diff / var[None, :, :], 2, seq)
    logp = np.log(w)[None, :] - 0.5 * (Xs.shape[1] * np.log(2.0 * np.pi) + M) - 0.5 * _sum(np.log(var), 1, seq)[None, :]
    mx = logp.max(axis=1)
    lse = mx + np.log(_sum(np.exp(logp - mx[:, None]), 1, seq))
    return M, logp, lse, logp - lse[:, None]


def y_mstep(Xs, r, cov_type, reg=REG, seq=False):
    """The M-step of the definition: (w, mu', v (K, D), n_k)."""
    nk = _sum(r, 0, seq) + 10.0 * np.finfo(np.float64).eps
    mu = _sum(r[:, :, None] * Xs[:, None, :], 0, seq) / nk[:, None]
    var = _sum(r[:, :, None] * (Xs * Xs)[:, None, :], 0, seq) / nk[:, None] - mu * mu + reg
    if cov_type == 'spherical':
        var = np.repeat(_sum(var, 1, seq)[:, None] / Xs.shape[1], Xs.shape[1], axis=1)
    w = nk / len(Xs)
    return w / _sum(w, 0, seq), mu, var, nk


def one_hot(labels, K):
    r = np.zeros((len(labels), K))
    r[np.arange(len(labels)), labels] = 1.0
    return r


def y_fit(X, K, cov_type, labels0, tol=TOL, reg=REG, max_iter=100, seq=False):
    """EM of the definition from the one-hot responsibilities of ``labels0``.  A dict: the shift c, the initial and final (w, mu', var), the first E-step
    (M, log p, lse, log r) and the first M-step, the lower bounds, n_iter, converged, and the final E-step's log r and labels."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    c = X64.mean(axis=0)
    Xs = X64 - c
    w, mu, var, _ = y_mstep(Xs, one_hot(labels0, K), cov_type, reg, seq)
    out = {'c': c, 'Xs': Xs, 'init': (w, mu, var), 'lbs': [], 'converged': False}
    lb = -np.inf
    for it in range(1, max_iter + 1):
        prev = lb
        M, logp, lse, logr = y_estep(Xs, w, mu, var, seq)
        w, mu, var, nk = y_mstep(Xs, np.exp(logr), cov_type, reg, seq)
        if it == 1:
            out['first'] = (M, logp, lse, logr, (w, mu, var, nk))
        lb = _sum(lse, 0, seq) / len(Xs)
        out['lbs'].append(lb)
        if abs(lb - prev) < tol:
            out['converged'] = True
            break
    out['n_iter'] = it
    out['final'] = (w, mu, var)
    out['lbs'] = np.array(out['lbs'])
    _, logp, lse, logr = y_estep(Xs, w, mu, var, seq)
    out['logr'], out['lse'], out['labels'] = logr, lse, logp.argmax(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def initial_labels(case, n_init=1):
    """sklearn's KMeans(n_init=1) on the f64 points, ``n_init`` fits in a row from one RandomState(5): (n_init, N)."""
    sk = pytest.importorskip('sklearn.cluster')
    X, K, _ = points(case), CASES[case][1], None
    rs = np.random.RandomState(5)
    return np.stack([sk.KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X.astype(np.float64)).labels_ for _ in range(n_init)])


@functools.lru_cache(maxsize=None)
def yardstick(case, restart=0, n_init=1, seq=False, max_iter=100):
    _, K, cov = CASES[case]
    return y_fit(points(case), K, cov, initial_labels(case, n_init)[restart], seq=seq, max_iter=max_iter)


def cov_of(var, cov_type):
    return var if cov_type == 'diag' else var[:, 0]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def sklearn_fit(case):
    mix = pytest.importorskip('sklearn.mixture')
    _, K, cov = CASES[case]
    y = yardstick(case)
    w, mu, var = y['init']
    return mix.GaussianMixture(K, covariance_type=cov, tol=TOL, reg_covar=REG, weights_init=w / w.sum() if K > 1 else np.ones(1), means_init=mu + y['c'],
                               precisions_init=1.0 / cov_of(var, cov)).fit(points(case).astype(np.float64))


def deviations(case, other):
    """The relative deviations of (lower bounds, weights, means, variances) of ``other`` = (lbs, w, means, cov) from the yardstick's."""
    _, _, cov = CASES[case]
    y = yardstick(case)
    w, mu, var = y['final']
    lbs, ow, om, ov = other
    return max(rel(lbs, y['lbs']), rel(ow, w), rel(om, mu + y['c']), rel(ov, cov_of(var, cov)))


def test_blobs_default_spread_is_test_ward_hosts():
    assert np.array_equal(blobs(257, 8, 10), TW.blobs(257, 8, 10)) and np.array_equal(blobs(4100, 8, 8, n_centers=7), TW.blobs(4100, 8, 8, n_centers=7))
    assert np.array_equal(points('dup_k3'), TW.points('dup')) and np.array_equal(points('same_k1'), TW.points('same'))


@pytest.mark.parametrize('case', list(CASES))
def test_yardstick_equals_sklearn(case):
    sk = sklearn_fit(case)
    y = yardstick(case)
    assert sk.n_iter_ == y['n_iter'] and sk.converged_ == y['converged'] and y['converged']
    assert np.array_equal(sk.predict(points(case).astype(np.float64)), y['labels'])
    dev = deviations(case, (sk.lower_bounds_, sk.weights_, sk.means_, sk.covariances_))
    print(case, 'n_iter', y['n_iter'], 'yardstick vs sklearn', dev)
    assert dev <= max(4.0 * BASE[case][0], 1e-14)
    if case == 'same_k1':
        assert np.allclose(y['final'][2], REG, rtol=1e-13, atol=0)
    if case in OVERLAP:
        soft = float((np.exp(y['logr']).max(axis=1) < 0.99).mean())
        print(case, 'rows with a largest responsibility below 0.99:', soft)
        assert soft > 0.02


@pytest.mark.parametrize('case', list(CASES))
def test_pairwise_and_sequential_sums_agree(case):
    y, s = yardstick(case), yardstick(case, seq=True)
    assert s['n_iter'] == y['n_iter'] and np.array_equal(s['labels'], y['labels'])
    w, mu, var = s['final']
    dev = deviations(case, (s['lbs'], w, mu + s['c'], cov_of(var, CASES[case][2])))
    print(case, 'pairwise vs sequential', dev)
    assert dev <= max(4.0 * BASE[case][1], 1e-14)


@pytest.mark.parametrize('case', list(CASES))
def test_cases_meet_the_conditions(case):
    """What the GPU tests rely on: clear stopping decisions, clear labels, no vanishing component.  (A change of seed must keep these.)"""
    y = yardstick(case)
    steps = np.abs(np.diff(np.concatenate([[-np.inf], y['lbs']])))
    margin = float(np.min(np.abs(steps - TOL)))
    assert margin > 1e-6, (case, steps)
    gap = np.inf
    if CASES[case][1] > 1:
        top = np.sort(y['logr'], axis=1)
        gap = float(np.min(top[:, -1] - top[:, -2]))
        assert gap > 1e-4
    assert y['final'][0].min() >= 1e-3
    print(case, 'stop margin', margin, 'label gap', gap, 'smallest weight', y['final'][0].min())


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
    lbs = [yardstick(case, r, 3)['lbs'][-1] for r in range(3)]
    return int(np.argmax(lbs))


@pytest.mark.parametrize('cov', ['diag', 'spherical'])
def test_model_selection_equals_sklearn(cov):
    mix = pytest.importorskip('sklearn.mixture')
    X = points('overlap_k4').astype(np.float64)
    sk = mix.GaussianMixture(4, covariance_type=cov, random_state=0).fit(X)
    assert n_parameters(4, 8, cov) == sk._n_parameters()
    ours = GaussianMixture(4, covariance_type=cov)
    ours.n_features_in_ = 8
    ours.score = sk.score          # (bic / aic are formulas on top of score)
    assert ours._n_parameters() == sk._n_parameters()
    assert ours.bic(X) == sk.bic(X) and ours.aic(X) == sk.aic(X)
    assert n_parameters(5, 13, 'diag') == 5 * 13 + 5 * 13 + 4 and n_parameters(5, 13, 'spherical') == 5 + 5 * 13 + 4


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    for cov in ('full', 'tied'):
        with pytest.raises(NotImplementedError, match='Cholesky factors are a different kernel'):
            GaussianMixture(2, covariance_type=cov)
    with pytest.raises(ValueError, match="'diag' or 'spherical'"):
        GaussianMixture(2, covariance_type='banded')
    with pytest.raises(NotImplementedError, match='warm_start'):
        GaussianMixture(2, warm_start=True)
    with pytest.raises(NotImplementedError, match='sample is not implemented'):
        GaussianMixture(2).sample(3)
    for bad in (0, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='n_components'):
            GaussianMixture(bad)
        with pytest.raises(ValueError, match='n_init'):
            GaussianMixture(2, n_init=bad)
        with pytest.raises(ValueError, match='max_iter'):
            GaussianMixture(2, max_iter=bad)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        GaussianMixture(33)
    with pytest.raises(ValueError, match='init_params'):
        GaussianMixture(2, init_params='zeros')
    with pytest.raises(ValueError, match='tol and reg_covar'):
        GaussianMixture(2, tol=-1.0)
    with pytest.raises(ValueError, match='2-D'):
        GaussianMixture(2).fit(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match='at least 2 points'):
        GaussianMixture(1).fit(X[:1])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        GaussianMixture(2).fit(np.zeros((10, 260), np.float32))
    with pytest.raises(RuntimeError, match='not fitted'):
        GaussianMixture(2).predict(X)
    m = GaussianMixture(2, weights_init=[0.5, 0.6])
    with pytest.raises(ValueError, match='normalized'):
        m._check_inits(8)
    with pytest.raises(ValueError, match="'means' should have the shape"):
        GaussianMixture(2, means_init=np.zeros((3, 8)))._check_inits(8)
    with pytest.raises(ValueError, match='precision'):
        GaussianMixture(2, precisions_init=np.zeros((2, 8)))._check_inits(8)
    with pytest.raises(ValueError, match='precision'):
        GaussianMixture(2, covariance_type='spherical', precisions_init=np.ones((2, 8)))._check_inits(8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            GaussianMixture(2).fit(X)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            G.gmm_sweep(X, [2, 3])


def test_module_does_not_import_scipy_or_sklearn():
    from deep_interpolation_clustering_amd import _gmm_base
    for module in (G, _gmm_base):
        with open(module.__file__) as f:
            assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M), module.__name__


def test_drivers_accept_gmm():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p2.get_arguments(['--cluster_method', 'gmm', '--k_max', '5', '--gmm_covariance_type', 'spherical', '--n_init', '3'])
    assert a.cluster_method == 'gmm' and a.gmm_covariance_type == 'spherical' and a.n_init == 3
    assert p2.get_arguments(['--cluster_method', 'gmm']).gmm_covariance_type == 'diag'
    assert p4.get_arguments(['--cluster_method', 'gmm', '--num_clusters', '3']).cluster_method == 'gmm'


def test_header_and_signatures_agree():
    names = {'dic_gmm_workspace', 'dic_gmm_em_iter', 'dic_gmm_estep', 'dic_gmm_mstep_labels'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_gmm_workspace(1000, 256, 4, 2)
    assert ws >= 2 * 63 * 8 * (4 * 513 + 1)
    for bad in ((1, 256, 4, 2), (1 << 30, 256, 4, 2), (1000, 260, 4, 2), (1000, 0, 4, 2), (1000, 256, 0, 2), (1000, 256, 33, 2), (1000, 256, 4, 0)):
        assert lib.dic_gmm_workspace(*bad) == 0
    assert lib.dic_gmm_workspace(75000, 256, 32, 1) == 256 * 8 * (32 * 513 + 1)

    def em(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=0, reg=1e-6, shift=fake, w=fake, mu=fake, var=fake, status=fake, lbs=fake, stride=100,
           work=fake, nbytes=ws):
        return lib.dic_gmm_em_iter(X, ldx, n, d, d0, k, runs, cov, reg, shift, w, mu, var, status, lbs, stride, work, nbytes, None)

    def es(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, shift=fake, w=fake, mu=fake, var=fake, work=fake, nbytes=ws):
        return lib.dic_gmm_estep(X, ldx, n, d, d0, k, shift, w, mu, var, None, None, None, None, work, nbytes, None)

    def ms(X=fake, ldx=256, n=1000, d=256, d0=256, k=4, runs=2, cov=0, reg=1e-6, shift=fake, labels=fake, resp=None, w=fake, mu=fake, var=fake, work=fake,
           nbytes=ws):
        return lib.dic_gmm_mstep_labels(X, ldx, n, d, d0, k, runs, cov, reg, shift, labels, resp, w, mu, var, work, nbytes, None)

    for call in (em, es, ms):
        for kw in ({'X': None}, {'shift': None}, {'w': None}, {'mu': None}, {'var': None}, {'work': None}):
            assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
        assert call(n=1) == -1 and b'at least 2' in lib.dic_last_error_string()
        assert call(n=0) == -1 and call(ldx=128) == -1 and call(d=0) == -1 and call(k=0) == -1 and call(d0=0) == -1 and call(d0=257) == -1
        assert call(ldx=252, d=250, d0=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=258) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
        assert call(k=33) == -2 and b'at most 32 components' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
        assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(work=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(nbytes=1000) == -3 and b'workspace' in lib.dic_last_error_string()
    for kw in ({'status': None}, {'lbs': None}, {'runs': 0}, {'stride': 0}, {'cov': 2}, {'cov': -1}, {'reg': -1.0}):
        assert em(**kw) == -1
    for kw in ({'runs': 0}, {'cov': 2}, {'reg': -1.0}, {'labels': None}, {'resp': fake}):
        assert ms(**kw) == -1
    assert b'exactly one' in lib.dic_last_error_string()


def test_gmm_kernels_do_not_spill_to_scratch():
    """An EM pass runs once per iteration and restart with 64 f64 accumulators per thread: a register that went to scratch memory would be paid on every
    row.  Require ScratchSize == 0 and no vector-register spills for every kernel of dic_gmm.hip.  (The pass kernels park a few dozen scalar registers in
    lanes of a vector register, which the compiler reports as SGPR spills; that costs no memory traffic and is not scratch.)"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_gmm.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    assert sum('gm_pass_kernel' in n for n in names) == 4 and any('gm_mstep_kernel' in n for n in names) and any('gm_sum_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
