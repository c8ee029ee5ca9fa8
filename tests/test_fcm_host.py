"""Fuzzy c-means, host side (no GPU): the numpy f64 yardstick of csrc/dic_fcm.hip's definition against the textbook form of the memberships and the
centres, the conditions the GPU tests (tests/test_gpu_fcm.py) rely on, the ABI's and the Python argument errors, and the register use of the kernels."""
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
from deep_interpolation_clustering_amd import fcm as F
from deep_interpolation_clustering_amd.fcm import FuzzyCMeans

from test_gmm_host import _dup, _overlap_d256, _overlap_k4, _sum, blobs, rel

TOL, MAX_ITER = 1e-6, 300          # the estimator's defaults, used by every case

# name -> (points, K, m).  The GPU tests run on exactly these.  One workgroup (3 rows) and two (17), full-width rows (D = 256), the ragged tail of a 16-row
# tile, the full grid of 256 workgroups with 17 rows each (4100), K = 2 and K = 32, zero-padded features (13 -> 16), duplicate rows, and the exp / log path
# of the memberships (m = 1.2, m = 1.05) beside the m == 2 short cut.
CASES = {
    'n3_k2': (lambda: blobs(3, 4, 1), 2, 2.0),
    'n17_k2': (lambda: blobs(17, 12, 3), 2, 2.0),
    'n255_k3': (lambda: blobs(255, 64, 4), 3, 2.0),
    'n257_d256_k5': (lambda: blobs(257, 256, 5), 5, 2.0),
    'n1030_k4': (lambda: blobs(1030, 8, 6), 4, 2.0),
    'n4100_k7': (lambda: blobs(4100, 8, 8, n_centers=7), 7, 2.0),
    'd13': (lambda: blobs(300, 13, 15), 3, 2.0),
    'dup_k3': (_dup, 3, 2.0),
    'overlap_k4_m1.2': (_overlap_k4, 4, 1.2),
    'overlap_k32_m1.2': (lambda: blobs(4100, 8, 13, n_centers=32, spread=2.0), 32, 1.2),
    'n257_d256_k5_m1.2': (lambda: blobs(257, 256, 5), 5, 1.2),
    'n1030_k4_m1.05': (lambda: blobs(1030, 8, 6), 4, 1.05),
}
# the fits that collapse (centres run together at the centre of gravity, their memberships become equal): only J, PC and PE are compared there
COLLAPSE = {
    'collapse_d256_k6': (_overlap_d256, 6, 2.0),
    'collapse_k4': (_overlap_k4, 4, 2.0),
}
ALL = dict(CASES, **COLLAPSE)
N_INIT_CASES = ['n1030_k4', 'overlap_k4_m1.2', 'overlap_k32_m1.2']

# The largest relative deviation (max |a - b| / max |b| per array: the J history, the centres, the memberships of the kept centres) measured on the CPU, per
# case, between the yardstick with numpy's pairwise sums and with strictly sequential sums.  The GPU tests allow 16 x that figure, and never less than 1e-13.
# Measured with numpy 2.2 on x86-64; test_pairwise_and_sequential_sums_agree holds the yardstick to 4 x these figures.
BASE = {
    'n3_k2': 0.0, 'n17_k2': 3.12e-16, 'n255_k3': 1.05e-15, 'n257_d256_k5': 7.17e-14, 'n1030_k4': 3.03e-15, 'n4100_k7': 5.38e-14, 'd13': 7.94e-16,
    'dup_k3': 9.28e-16, 'overlap_k4_m1.2': 4.22e-15, 'overlap_k32_m1.2': 3.26e-14, 'n257_d256_k5_m1.2': 1.02e-15, 'n1030_k4_m1.05': 2.97e-13,
}


# The same figure for the two collapsing fits over the J history, PC and PE only: their centres are ill-conditioned (they deviated by 1e-9 between the two
# orders of summation) and are not compared.
COLLAPSE_BASE = {'collapse_d256_k6': 2.54e-14, 'collapse_k4': 1.54e-15}


def fit_rtol(case):
    """The relative tolerance of a whole fit on the device against the yardstick (see BASE, COLLAPSE_BASE)."""
    return max(16.0 * (BASE[case] if case in BASE else COLLAPSE_BASE[case]), 1e-13)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


@functools.lru_cache(maxsize=None)
def points(case):
    X = ALL[case][0]()
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def initial_rows(case, n_init=1):
    """The rows the initial centres are, (n_init, K), drawn in a row from one RandomState(0): the first pass always meets rows at distance 0."""
    rs = np.random.RandomState(0)
    return np.stack([rs.choice(len(points(case)), size=ALL[case][1], replace=False) for _ in range(n_init)])


def initial_centers(case, n_init=1):
    """(n_init, K, D) f64, unshifted: what the estimator takes as ``centers_init``."""
    return points(case).astype(np.float64)[initial_rows(case, n_init)]


def y_memberships(Xs, V, m, seq=False):
    """The memberships of the definition on shifted f64 points: (d2, u, w, log u with 0 where u == 0)."""
    diff = Xs[:, None, :] - V[None, :, :]
    d2 = _sum(diff * diff, 2, seq)
    dmin = d2.min(axis=1)
    pos = dmin > 0
    u = np.zeros_like(d2)
    with np.errstate(divide='ignore'):
        r = dmin[pos, None] / d2[pos]
        t = r if m == 2.0 else np.exp((1.0 / (m - 1.0)) * np.log(r))
    u[pos] = t / _sum(t, 1, seq)[:, None]
    zero = d2[~pos] == 0
    u[~pos] = zero / zero.sum(axis=1)[:, None]
    lg = np.log(np.where(u > 0, u, 1.0))
    w = u * u if m == 2.0 else np.where(u > 0, np.exp(m * lg), 0.0)
    return d2, u, w, lg


def y_sums(d2, u, w, lg, seq=False):
    """(J, S2, SE): over k, then over the rows."""
    return tuple(float(_sum(_sum(a, 1, seq), 0, seq)) for a in (w * d2, u * u, u * lg))


def y_update(Xs, w, V, seq=False):
    nk = _sum(w, 0, seq)
    sx = _sum(w[:, :, None] * Xs[:, None, :], 0, seq)
    safe = np.where(nk != 0, nk, 1.0)
    return np.where((nk != 0)[:, None], sx / safe[:, None], V), nk


def y_fit(X, m, V0, tol=TOL, max_iter=MAX_ITER, seq=False):
    """Fuzzy c-means of the definition from the (unshifted) centres ``V0``.  A dict: the shift c, the shifted points, the first pass (d2, u, w, (J, S2, SE),
    the centres after it), the J history, n_iter, converged, the kept centres (shifted), the centres that entered the last iteration, and the pass with the
    kept centres: u, d2, labels and its (J, S2, SE)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    c = X64.mean(axis=0)
    Xs = X64 - c
    V = np.asarray(V0, dtype=np.float64) - c
    out = {'c': c, 'Xs': Xs, 'V0': V.copy(), 'J': [], 'converged': False}
    for it in range(1, max_iter + 1):
        d2, u, w, lg = y_memberships(Xs, V, m, seq)
        J = y_sums(d2, u, w, lg, seq)
        entered = V
        V, nk = y_update(Xs, w, V, seq)
        if it == 1:
            out['first'] = (d2, u, w, J, V.copy())
        out['J'].append(J[0])
        if it >= 2 and abs(out['J'][-2] - J[0]) <= tol * out['J'][-2]:
            out['converged'] = True
            break
    out['n_iter'], out['V'], out['entered'], out['J'] = it, V, entered, np.array(out['J'])
    d2, u, w, lg = y_memberships(Xs, V, m, seq)
    out['u'], out['d2'], out['w'], out['labels'], out['sums'] = u, d2, w, u.argmax(axis=1), y_sums(d2, u, w, lg, seq)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(case, restart=0, n_init=1, seq=False, max_iter=MAX_ITER):
    return y_fit(points(case), ALL[case][2], initial_centers(case, n_init)[restart], seq=seq, max_iter=max_iter)


def indices(y, K):
    """(PC, PE, MPC) of a yardstick fit."""
    n = len(y['Xs'])
    pc = y['sums'][1] / n
    return pc, -y['sums'][2] / n, (K * pc - 1.0) / (K - 1.0)


def separation(V):
    """(the centre distances (K, K), the smallest one off the diagonal)."""
    diff = V[:, None, :] - V[None, :, :]
    sep = np.sqrt((diff * diff).sum(axis=2))
    return sep, float(sep[~np.eye(len(V), dtype=bool)].min())


def rms(y):
    return float(np.sqrt((y['Xs'] ** 2).sum() / len(y['Xs'])))


def deviation(case, other):
    """The largest relative deviation of ``other`` = (J history, kept centres (shifted), memberships of the kept centres) from the yardstick's."""
    y = yardstick(case)
    return max(rel(other[0], y['J']), rel(other[1], y['V']), rel(other[2], y['u']))


@pytest.mark.parametrize('case', list(CASES))
def test_yardstick_equals_the_textbook(case):
    """No third-party FCM is here, so the yardstick is held to the textbook: u_ik = 1 / sum_j (d_ik / d_jk)^(2 / (m - 1)) from scipy's distances, v_k the
    u^m-weighted mean, J never increasing, and at the end a fixed point up to what the stopping rule allows: with T one full iteration and n_k = sum_i u_ik^m,
    J(U, V) - J(U, T V) = sum_k n_k |V_k - (T V)_k|^2, and a fit that stopped had a decrease of at most tol J."""
    cdist = pytest.importorskip('scipy.spatial.distance').cdist
    _, K, m = CASES[case]
    y = yardstick(case)
    assert y['converged'] and 2 <= y['n_iter'] < MAX_ITER
    X64 = points(case).astype(np.float64)
    for V in (y['entered'], y['V']):
        d = cdist(X64, V + y['c'])
        assert d.min() > 0
        u = 1.0 / ((d[:, :, None] / d[:, None, :]) ** (2.0 / (m - 1.0))).sum(axis=2)
        if V is y['entered']:
            mean = ((u ** m)[:, :, None] * X64[:, None, :]).sum(axis=0) / (u ** m).sum(axis=0)[:, None]
            assert rel(y['V'] + y['c'], mean) <= 1e-11          # the kept centres: the update of the memberships that entered
        else:
            assert np.max(np.abs(u - y['u'])) <= 1e-11
    assert np.max(np.abs(y['u'].sum(axis=1) - 1.0)) <= 1e-14
    steps = np.diff(y['J'])
    assert np.all(steps <= 1e-13 * y['J'][:-1]), steps.max()
    assert y['sums'][0] <= y['J'][-1] * (1 + 1e-13)
    TV, nk = y_update(y['Xs'], y['w'], y['V'])
    residual = float((nk * ((TV - y['V']) ** 2).sum(axis=1)).sum())
    print(case, 'n_iter', y['n_iter'], 'fixed-point residual / (tol J)', residual / (TOL * y['J'][-1]))
    assert residual <= TOL * y['J'][-1]


@pytest.mark.parametrize('case', list(CASES))
def test_pairwise_and_sequential_sums_agree(case):
    y, s = yardstick(case), yardstick(case, seq=True)
    assert s['n_iter'] == y['n_iter'] and s['converged'] == y['converged'] and np.array_equal(s['labels'], y['labels'])
    dev = deviation(case, (s['J'], s['V'], s['u']))
    print(case, 'pairwise vs sequential', dev)
    assert dev <= max(4.0 * BASE[case], 1e-14)


@pytest.mark.parametrize('case', list(CASES))
def test_cases_meet_the_conditions(case):
    """What the parity tests rest on: no collapse (no coincident pair, PC >= 1 / K + 0.05), a first pass that meets rows at distance 0, clear stopping
    decisions and clear labels.  (A change of seed must keep these.)"""
    _, K, m = CASES[case]
    y = yardstick(case)
    sep, closest = separation(y['V'])
    pc, pe, mpc = indices(y, K)
    assert closest >= F.COINCIDENT_FRACTION * rms(y), (closest, rms(y))
    assert pc >= 1.0 / K + 0.05
    assert ((y['first'][0] == 0).sum(axis=1) >= 1).sum() >= K
    ratios = np.abs(np.diff(y['J'])) / y['J'][:-1]
    margin = float(np.min(np.abs(ratios / TOL - 1.0)))
    top = np.sort(y['u'], axis=1)
    gap = float(np.min(top[:, -1] - top[:, -2]))
    print(case, 'n_iter', y['n_iter'], 'closest / rms', closest / rms(y), 'PC', pc, 'stop margin', margin, 'label gap', gap)
    assert margin > 1e-4 and gap > 1e-9


@pytest.mark.parametrize('case', list(COLLAPSE))
def test_collapse_cases_collapse(case):
    _, K, m = COLLAPSE[case]
    y = yardstick(case)
    _, closest = separation(y['V'])
    pc, pe, _ = indices(y, K)
    print(case, 'n_iter', y['n_iter'], 'closest / rms', closest / rms(y), 'PC - 1 / K', pc - 1.0 / K)
    assert closest < F.COINCIDENT_FRACTION * rms(y) and pc < 1.0 / K + 0.05
    if case == 'collapse_d256_k6':          # every centre at the centre of gravity; in collapse_k4 only some of the centres coincide
        assert abs(pc - 1.0 / K) < 1e-4 and abs(pe - np.log(K)) < 1e-4
    s = yardstick(case, seq=True)
    assert s['n_iter'] == y['n_iter'] and s['converged'] == y['converged'] and y['converged']
    ratios = np.abs(np.diff(y['J'])) / y['J'][:-1]
    assert np.min(np.abs(ratios / TOL - 1.0)) > 1e-4          # clear stopping decisions here too
    spc, spe, _ = indices(s, K)
    dev = max(rel(s['J'], y['J']), abs(spc - pc) / pc, abs(spe - pe) / pe)
    print(case, 'pairwise vs sequential: J history, PC, PE', dev, 'centres', rel(s['V'], y['V']))
    assert dev <= max(4.0 * COLLAPSE_BASE[case], 1e-14)


def test_the_smaller_fuzzifier_does_not_collapse():
    """overlap_k4 collapses at m = 2 and not at m = 1.2: the advice of the warning."""
    y = yardstick('overlap_k4_m1.2')
    assert separation(y['V'])[1] > 10 * F.COINCIDENT_FRACTION * rms(y)


@pytest.mark.parametrize('case', N_INIT_CASES)
def test_three_restarts_have_a_clear_winner(case):
    last = [yardstick(case, r, 3)['J'][-1] for r in range(3)]
    order = np.argsort(last)
    print(case, 'final J', last, 'winner (0-based)', order[0])
    assert last[order[1]] - last[order[0]] > 1e-9 * last[order[0]]
    for r in range(3):
        y = yardstick(case, r, 3)
        ratios = np.abs(np.diff(y['J'])) / y['J'][:-1]
        assert np.min(np.abs(ratios / TOL - 1.0)) > 1e-4 and y['converged']
    assert len({yardstick(case, r, 3)['n_iter'] for r in range(3)}) > 1          # (a restart that is done waits for the others)


def winner(case):
    return int(np.argmin([yardstick(case, r, 3)['J'][-1] for r in range(3)]))


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    for bad in (0, 1, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='n_clusters'):
            FuzzyCMeans(bad)
    for bad in (0, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='n_init'):
            FuzzyCMeans(2, n_init=bad)
        with pytest.raises(ValueError, match='max_iter'):
            FuzzyCMeans(2, max_iter=bad)
    with pytest.raises(ValueError, match='outside the compiled limit'):
        FuzzyCMeans(33)
    for bad in (1.0, 0.5, -2.0, float('inf'), float('nan'), True, 'x', None):
        with pytest.raises(ValueError, match='fuzzifier'):
            FuzzyCMeans(2, m=bad)
    with pytest.raises(ValueError, match='tol'):
        FuzzyCMeans(2, tol=-1.0)
    with pytest.raises(ValueError, match='init must be'):
        FuzzyCMeans(2, init='zeros')
    with pytest.raises(TypeError):
        FuzzyCMeans(2, 2.0, 1e-6, 300, 1, 'random', None, np.zeros((1, 2, 8)))          # (centers_init is keyword-only)
    with pytest.raises(ValueError, match='2-D'):
        FuzzyCMeans(2).fit(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match='at least 2 points'):
        FuzzyCMeans(2).fit(X[:1])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        FuzzyCMeans(2).fit(np.zeros((10, 260), np.float32))
    with pytest.raises(RuntimeError, match='not fitted'):
        FuzzyCMeans(2).predict(X)
    with pytest.raises(RuntimeError, match='not fitted'):
        FuzzyCMeans(2).memberships(X)
    assert FuzzyCMeans.memberships is FuzzyCMeans.predict_proba
    p = FuzzyCMeans(3, m=1.5, n_init=2, init='random', random_state=4).get_params()
    assert p == dict(n_clusters=3, m=1.5, tol=1e-6, max_iter=300, n_init=2, init='random', random_state=4)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            FuzzyCMeans(2).fit(X)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            F.fcm_sweep(X, [2, 3])


def test_module_does_not_import_scipy_or_sklearn():
    with open(F.__file__) as f:
        assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M)


def test_drivers_accept_fcm():
    from deep_interpolation_clustering_amd import _cluster_cli
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    assert 'fcm' in _cluster_cli.METHODS and 'fcm' in p2.BRANCHES and 'fcm' in p4.Cluster.BRANCHES
    assert _cluster_cli.METHODS.index('fcm') == _cluster_cli.METHODS.index('gmm') + 1
    a = p2.get_arguments(['--cluster_method', 'fcm', '--k_max', '5', '--fcm_m', '1.2', '2', '--n_init', '3'])
    assert a.cluster_method == 'fcm' and a.fcm_m == [1.2, 2.0] and a.n_init == 3
    assert p2.get_arguments(['--cluster_method', 'fcm']).fcm_m == [2.0]
    b = p4.get_arguments(['--cluster_method', 'fcm', '--num_clusters', '3', '--fcm_m', '1.2'])
    assert b.cluster_method == 'fcm' and b.fcm_m == 1.2 and p4.get_arguments([]).fcm_m == 2.0


def test_header_and_signatures_agree():
    names = {'dic_fcm_workspace', 'dic_fcm_iter', 'dic_fcm_memberships'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_fcm_workspace(1000, 256, 4, 2)
    assert ws >= 2 * 63 * 8 * (4 * 257 + 3)
    for bad in ((1, 256, 4, 2), (1 << 30, 256, 4, 2), (1000, 260, 4, 2), (1000, 0, 4, 2), (1000, 256, 0, 2), (1000, 256, 33, 2), (1000, 256, 4, 0)):
        assert lib.dic_fcm_workspace(*bad) == 0
    assert lib.dic_fcm_workspace(75000, 256, 32, 1) == 256 * 8 * (32 * 257 + 3)

    def it(X=fake, ldx=256, n=1000, d=256, k=4, runs=2, m=2.0, shift=fake, centers=fake, status=fake, objs=fake, stride=100, work=fake, nbytes=ws):
        return lib.dic_fcm_iter(X, ldx, n, d, k, runs, m, shift, centers, status, objs, stride, work, nbytes, None)

    def mem(X=fake, ldx=256, n=1000, d=256, k=4, m=2.0, shift=fake, centers=fake, work=fake, nbytes=ws):
        return lib.dic_fcm_memberships(X, ldx, n, d, k, m, shift, centers, None, None, None, None, work, nbytes, None)

    for call in (it, mem):
        for kw in ({'X': None}, {'shift': None}, {'centers': None}, {'work': None}):
            assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
        for m in (1.0, 0.5, -1.0, float('inf'), float('nan')):
            assert call(m=m) == -1 and b'fuzzifier' in lib.dic_last_error_string()
        assert call(m=1.0, k=33) == -1          # the invalid argument before the unsupported shape
        assert call(n=1) == -1 and b'at least 2' in lib.dic_last_error_string()
        assert call(n=0) == -1 and call(ldx=128) == -1 and call(d=0) == -1 and call(k=0) == -1
        assert call(ldx=260, d=258) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=258) == -2 and b'multiples of 4' in lib.dic_last_error_string()
        assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
        assert call(k=33) == -2 and b'at most 32 components' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
        assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(work=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
        assert call(nbytes=1000) == -3 and b'workspace' in lib.dic_last_error_string()
    for kw in ({'status': None}, {'objs': None}, {'runs': 0}, {'stride': 0}):
        assert it(**kw) == -1


def test_fcm_kernels_do_not_spill_to_scratch():
    """A pass runs once per iteration and restart with up to 32 f64 accumulators per thread: a register that went to scratch memory would be paid on every
    row.  Require ScratchSize == 0 and no vector-register spills for every kernel of dic_fcm.hip.  (Scalar registers parked in lanes of a vector register
    are reported as SGPR spills; that costs no memory traffic and is not scratch.)"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_fcm.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    assert sum('fc_pass_kernel' in n for n in names) == 2 and any('fc_reduce_kernel' in n for n in names) and any('fc_sums_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
