"""Mean shift without a GPU: the numpy f64 yardstick of the definition in include/dic_hip.h (it shares no code with meanshift.py), the yardstick against
sklearn's MeanShift, the cases the GPU tests (tests/test_gpu_meanshift.py) run and the conditions that make equality demands on them fair, argument errors of
the estimator and of the new ABI calls, the p2 / p4 parsers, and the register budget of the kernels (compile only).

WHY EQUALITY IS FAIR.  Member sets, stopping decisions, suppressions and labels are comparisons of f64 quantities whose value depends on the summation order
at the 1e-13 level at most.  Every random case is therefore required to keep every such comparison at least GAP = 1e-9 (relative) away from its threshold, in
the yardstick, over all seeds and iterations; a case that does not gets another random seed, never a lower bar."""
import collections
import ctypes
import functools
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import meanshift as M

GAP = 1e-9
Result = collections.namedtuple('Result', 'centres labels seed_positions seed_counts seed_iterations n_iter first_members gaps bandwidth')


# ------------------------------------------------------------------------------------------------------------------------------------ the yardstick
def y_bin_seeds(X, h, min_bin_freq):
    """sklearn's get_bin_seeds, restated: bins of np.round(X / h) in first-appearance order, f32 grid coordinates times h."""
    sizes = collections.OrderedDict()
    for p in X:
        key = tuple(np.round(p / h))
        sizes[key] = sizes.get(key, 0) + 1
    seeds = np.array([k for k, f in sizes.items() if f >= min_bin_freq], dtype=np.float32)
    if len(seeds) == len(X):
        return X
    return seeds * np.float32(h)


def y_estimate_bandwidth(X32, quantile=0.3):
    X = np.asarray(X32, dtype=np.float64)
    k = max(1, int(len(X) * quantile))
    total = 0.0
    kth = np.empty(len(X))
    for i in range(len(X)):
        d = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
        kth[i] = np.partition(d, k - 1)[k - 1]
    total = kth.mean()
    return float(total)


def yardstick(X32, h, seeds=None, bin_seeding=False, min_bin_freq=1, cluster_all=True, max_iter=300):
    """The definition, seed by seed.  ``gaps``: the smallest relative distance of any comparison from its threshold (member, moved, centre, nearest, orphan)."""
    X = np.asarray(X32, dtype=np.float64)
    n = len(X)
    c = X.mean(axis=0)
    Xp = X - c
    t = h * h
    if seeds is None:
        seeds = y_bin_seeds(X, h, min_bin_freq) if bin_seeding else X
    seeds = np.asarray(seeds, dtype=np.float64)
    gaps = dict(member=np.inf, moved=np.inf, centre=np.inf, nearest=np.inf, orphan=np.inf)
    pos, counts, iters, first = [], [], [], np.zeros((len(seeds), n), dtype=bool)
    for q, s in enumerate(seeds):
        s = s.copy()
        done_iters, cnt = 0, 0
        shifts = 0
        while True:
            d2 = ((s - X) ** 2).sum(axis=1)
            gaps['member'] = min(gaps['member'], float(np.min(np.abs(d2 - t) / t)))
            m = d2 <= t
            if shifts == 0:
                first[q] = m
            shifts += 1
            cnt = int(m.sum())
            if cnt == 0:
                break
            new = c + Xp[m].sum(axis=0) / cnt
            moved = float(np.sqrt(((new - s) ** 2).sum()))
            gaps['moved'] = min(gaps['moved'], abs(moved - 1e-3 * h) / (1e-3 * h))
            s = new
            if moved <= 1e-3 * h or done_iters == max_iter:
                break
            done_iters += 1
        pos.append(s)
        counts.append(cnt)
        iters.append(done_iters)
    pos, counts, iters = np.array(pos), np.array(counts), np.array(iters)
    live = [(int(counts[q]), tuple(pos[q])) for q in range(len(seeds)) if counts[q] > 0]
    if not live:
        raise ValueError('No point was within bandwidth=%f of any seed.' % h)
    srt = np.array([p for _, p in sorted(live, reverse=True)])
    alive = np.ones(len(srt), dtype=bool)
    keep = []
    for i in range(len(srt)):
        if not alive[i]:
            continue
        d2 = ((srt[i] - srt) ** 2).sum(axis=1)
        others = np.arange(len(srt)) != i
        if others.any():
            gaps['centre'] = min(gaps['centre'], float(np.min(np.abs(d2[others] - t) / t)))
        alive &= ~(d2 <= t)
        keep.append(i)
    centres = srt[keep]
    d2 = np.stack([((cen - X) ** 2).sum(axis=1) for cen in centres], axis=1)          # (n, K)
    labels = d2.argmin(axis=1)
    best = d2[np.arange(n), labels]
    if len(centres) > 1:
        second = np.partition(d2, 1, axis=1)[:, 1]
        gaps['nearest'] = float(np.min((second - best) / second))
    if not cluster_all:
        gaps['orphan'] = float(np.min(np.abs(best - t) / t))
        labels = np.where(best > t, -1, labels)
    return Result(centres, labels.astype(np.int64), pos, counts, iters, int(iters.max()), first, gaps, h)


# ---------------------------------------------------------------------------------------------------------------------------------------- the cases
def blobs(n, d, k, seed, spread):
    rs = np.random.RandomState(seed)
    cen = rs.normal(size=(k, d)) * spread
    lab = rs.randint(k, size=n)
    return (cen[lab] + rs.normal(size=(n, d))).astype(np.float32)


def _quantile_case(n, d, k, seed, spread, quantile):
    X = blobs(n, d, k, seed, spread)
    return dict(X=X, h=y_estimate_bandwidth(X, quantile), kw={})


def _explicit_seeds(m, seed):
    X = blobs(400, 8, 3, seed, 4.0)
    rs = np.random.RandomState(seed + 100)
    seeds = X[rs.randint(len(X), size=m)].astype(np.float64) + rs.normal(size=(m, 8)) * 0.25
    if m > 1:
        seeds[rs.rand(m) < 0.2] += 1e3          # far from every point: count 0, dropped
    return dict(X=X, h=y_estimate_bandwidth(X, 0.2), kw=dict(seeds=seeds))


def _duplicates():
    X = blobs(150, 8, 3, 21, 4.0)
    X = np.concatenate([X, X[:90], X[:30]])
    return dict(X=X, h=y_estimate_bandwidth(blobs(150, 8, 3, 21, 4.0), 0.3), kw={})


def _lattice():
    rs = np.random.RandomState(5)
    X = rs.randint(0, 4, size=(300, 4)).astype(np.float32)
    return dict(X=X, h=2.0, kw={})          # pairs at d2 == 4 == t exactly: (2,0,0,0) and (1,1,1,1) steps


_BUILDERS = {
    'n2_d4': lambda: dict(X=np.array([[0, 0, 0, 0], [1, 0.5, 0, 0.25]], dtype=np.float32), h=0.75, kw={}),
    'n255_d8': lambda: _quantile_case(255, 8, 3, 0, 4.0, 0.2),
    'n256_d8': lambda: _quantile_case(256, 8, 3, 1, 4.0, 0.2),
    'n257_d8': lambda: _quantile_case(257, 8, 3, 2, 4.0, 0.2),
    'n300_d5': lambda: _quantile_case(300, 5, 3, 3, 4.0, 0.2),
    'n600_d256': lambda: _quantile_case(600, 256, 3, 4, 3.0, 0.3),
    'n1000_d4': lambda: _quantile_case(1000, 4, 5, 3, 5.0, 0.1),
    'seeds_m1': lambda: _explicit_seeds(1, 7),
    'seeds_m257': lambda: _explicit_seeds(257, 8),
    'duplicates': _duplicates,
    'lattice': _lattice,
}
RANDOM_CASES = [name for name in _BUILDERS if name != 'lattice']          # the lattice serves the one-shift mask test only
# (case, estimator keywords): every random case as it stands, and the variants
VARIANTS = [(name, ()) for name in RANDOM_CASES] + [
    ('n257_d8', (('cluster_all', False),)), ('n1000_d4', (('cluster_all', False),)),
    ('n300_d5', (('bin_seeding', True),)), ('n1000_d4', (('bin_seeding', True), ('min_bin_freq', 2))),
    ('n256_d8', (('max_iter', 0),)), ('n255_d8', (('max_iter', 2),)), ('n600_d256', (('max_iter', 1),)), ('n1000_d4', (('max_iter', 2), ('cluster_all', False))),
]
VARIANT_IDS = ['%s%s' % (n, ''.join('-%s=%s' % kv for kv in kw)) for n, kw in VARIANTS]


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    c['X'].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, kw=()):
    c = case(name)
    return yardstick(c['X'], c['h'], **{**c['kw'], **dict(kw)})


# ---------------------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('name,kw', VARIANTS, ids=VARIANT_IDS)
def test_conditions_of_the_cases(name, kw):
    r = reference(name, kw)
    print(name, kw, 'centres', len(r.centres), 'n_iter', r.n_iter, 'gaps', r.gaps)
    for what, g in r.gaps.items():
        assert g >= GAP, (what, g)


def test_shapes_of_the_cases():
    assert len(reference('n600_d256').centres) >= 2
    assert len(reference('n1000_d4').centres) == 5
    assert case('n2_d4')['X'].shape == (2, 4) and case('n300_d5')['X'].shape == (300, 5)
    r = reference('seeds_m257')
    assert case('seeds_m257')['kw']['seeds'].shape == (257, 8) and (r.seed_counts == 0).sum() >= 10 and (r.seed_counts > 0).sum() >= 100
    assert case('seeds_m1')['kw']['seeds'].shape == (1, 8) and len(reference('seeds_m1').centres) == 1
    assert reference('n256_d8', (('max_iter', 0),)).n_iter == 0 and reference('n255_d8', (('max_iter', 2),)).n_iter == 2
    assert reference('n600_d256', (('max_iter', 1),)).n_iter == 1 and reference('n600_d256').n_iter == 2          # (the variants cut fits that run longer)
    assert reference('n255_d8').n_iter > 2 and reference('n1000_d4').n_iter > 2
    assert (reference('n257_d8', (('cluster_all', False),)).labels == -1).any()
    X = case('lattice')['X']
    d2 = ((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1)
    assert (d2 == 4.0).sum() > 1000          # members AT the bandwidth
    dup = case('duplicates')['X']
    assert len(np.unique(dup, axis=0)) == 150 and len(dup) == 270


@pytest.mark.parametrize('name,kw', VARIANTS, ids=VARIANT_IDS)
def test_yardstick_against_sklearn(name, kw):
    cluster = pytest.importorskip('sklearn.cluster')
    c = case(name)
    r = reference(name, kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sk = cluster.MeanShift(bandwidth=c['h'], **{**c['kw'], **dict(kw)}).fit(c['X'].astype(np.float64))
    assert sk.cluster_centers_.shape == r.centres.shape
    scale = np.abs(sk.cluster_centers_).max()
    assert np.abs(sk.cluster_centers_ - r.centres).max() <= 1e-12 * scale
    assert np.array_equal(sk.labels_, r.labels)
    assert sk.n_iter_ == r.n_iter


@pytest.mark.parametrize('name,q', [('n255_d8', 0.2), ('n300_d5', 0.3), ('n600_d256', 0.3), ('n1000_d4', 0.1), ('n2_d4', 0.3)])
def test_estimate_bandwidth_yardstick_against_sklearn(name, q):
    cluster = pytest.importorskip('sklearn.cluster')
    X = case(name)['X']
    want = cluster.estimate_bandwidth(X.astype(np.float64), quantile=q)
    assert abs(y_estimate_bandwidth(X, q) - want) <= 1e-12 * want


def test_get_bin_seeds_equals_sklearn_and_the_yardstick():
    cluster = pytest.importorskip('sklearn.cluster')
    for name, freq in (('n300_d5', 1), ('n1000_d4', 2), ('n1000_d4', 1)):
        c = case(name)
        X = c['X'].astype(np.float64)
        got = M.get_bin_seeds(X, c['h'], freq)
        assert got.dtype == np.float32 and np.array_equal(got, y_bin_seeds(X, c['h'], freq))
        assert np.array_equal(got, cluster.get_bin_seeds(X, c['h'], freq))
    X = case('n2_d4')['X'].astype(np.float64)
    with pytest.warns(UserWarning, match='Binning data failed'):
        assert M.get_bin_seeds(X, 0.01) is X


# ------------------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    X = np.zeros((5, 4), np.float32)
    for bad in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='bandwidth must be > 0'):
            M.MeanShift(bandwidth=bad)
    with pytest.raises(ValueError, match='below 2\\^50'):
        M.MeanShift(bandwidth=2.0 ** 50)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='max_iter must be an int >= 0'):
            M.MeanShift(bandwidth=1.0, max_iter=bad)
    with pytest.raises(ValueError, match='min_bin_freq must be an int >= 1'):
        M.MeanShift(bandwidth=1.0, min_bin_freq=0)
    with pytest.raises(ValueError, match='mask_budget'):
        M.MeanShift(bandwidth=1.0, mask_budget=0)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        M.MeanShift(bandwidth=1.0).fit(np.zeros((5, 260), np.float32))
    with pytest.raises(ValueError, match='at least 1 point'):
        M.MeanShift(bandwidth=1.0).fit(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match='2-D'):
        M.MeanShift(bandwidth=1.0).fit(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match='quantile'):
        M.estimate_bandwidth(X, quantile=1.5)
    with pytest.raises(RuntimeError, match='not fitted'):
        M.MeanShift(bandwidth=1.0).predict(X)
    assert M.MeanShift().get_params()['max_iter'] == 300 and M.MeanShift().max_iter == 300
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU'):
            M.MeanShift(bandwidth=1.0).fit(X)


def test_module_does_not_import_scipy_or_sklearn():
    with open(M.__file__) as f:
        text = f.read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', text, flags=re.M)


NAMES = {'dic_meanshift_workspace': 2, 'dic_meanshift_prepare': 9, 'dic_meanshift_members': 16, 'dic_meanshift_shift': 15, 'dic_meanshift_nearest': 10}


def test_header_and_signatures_agree():
    assert set(NAMES) <= set(N.header_symbols()) and set(NAMES) <= set(N.SIGNATURES)
    for name, n_args in NAMES.items():
        assert len(N.SIGNATURES[name][1]) == n_args
    assert set(N.header_symbols()) == set(N.SIGNATURES)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    odd = ctypes.c_void_p((1 << 20) + 2)
    nb = ctypes.c_int64(0)

    def prepare(x=fake, ldx=8, n=1000, d=8, centre=fake, m_max=100, ws=fake, ws_bytes=1 << 40):
        return lib.dic_meanshift_prepare(x, ldx, n, d, centre, m_max, ws, ws_bytes, None)

    def members(x=fake, ldx=8, n=1000, d=8, centre=fake, seeds=fake, m=100, m_max=100, h=1.0, mask=fake, band=fake, cap=16, n_band=ctypes.byref(nb), ws=fake,
                ws_bytes=1 << 40):
        return lib.dic_meanshift_members(x, ldx, n, d, centre, seeds, m, m_max, h, mask, band, cap, n_band, ws, ws_bytes, None)

    def shift(x=fake, ldx=8, n=1000, d=8, c=fake, mask=fake, m=100, seeds=fake, h=1.0, max_iter=300, counts=fake, iters=fake, done=fake, sums=None):
        return lib.dic_meanshift_shift(x, ldx, n, d, c, mask, m, seeds, h, max_iter, counts, iters, done, sums, None)

    def nearest(x=fake, ldx=8, rows=None, n=1000, d=8, centres=fake, c=3, idx=fake, d2=fake):
        return lib.dic_meanshift_nearest(x, ldx, rows, n, d, centres, c, idx, d2, None)

    err = lib.dic_last_error_string
    assert lib.dic_meanshift_workspace(1000, 100) > 2 * 2 * (1000 + 256) * 288 and lib.dic_meanshift_workspace(0, 100) == 0
    assert lib.dic_meanshift_workspace(1000, 0) == 0 and lib.dic_meanshift_workspace(1 << 30, 100) == 0
    assert lib.dic_meanshift_workspace(75000, 75000) > lib.dic_meanshift_workspace(75000, 1000)
    for call in (prepare, members, shift, nearest):
        assert call(n=0) == -1 and call(d=0) == -1
        assert call(d=260, ldx=260) == -2 and b'at most 256' in err()
        assert call(d=6) == -2 and b'multiples of 4' in err()
        assert call(x=odd) == -2 and b'aligned' in err()
    for call in (prepare, members, shift):
        assert call(ldx=4) == -1 and call(x=None) == -1 and b'NULL' in err()
    for call in (members, shift):
        for h in (0.0, -1.0, float('nan')):
            assert call(h=h) == -1 and b'bandwidth' in err()
        assert call(m=0) == -1
    assert prepare(ws_bytes=1000) == -3 and members(ws_bytes=1000) == -3 and b'workspace' in err()
    assert prepare(m_max=0) == -1 and prepare(n=1 << 30) == -2 and prepare(centre=None) == -1 and prepare(ws=None) == -1
    assert members(m=101) == -1 and members(cap=-1) == -1 and members(h=2.0 ** 50) == -2 and b'2^50' in err()
    for kw in ({'seeds': None}, {'mask': None}, {'n_band': None}, {'ws': None}, {'centre': None}, {'band': None}):
        assert members(**kw) == -1 and b'NULL' in err(), kw
    assert members(band=None, cap=0, ws_bytes=1000) == -3          # (no band list is fine with capacity 0)
    for kw in ({'seeds': odd}, {'mask': odd}, {'band': odd}, {'ws': odd}):
        assert members(**kw) == -2 and b'aligned' in err(), kw
    assert shift(max_iter=-1) == -1
    for kw in ({'c': None}, {'mask': None}, {'seeds': None}, {'counts': None}, {'iters': None}, {'done': None}):
        assert shift(**kw) == -1 and b'NULL' in err(), kw
    for kw in ({'c': odd}, {'seeds': odd}, {'sums': odd}, {'mask': odd}):
        assert shift(**kw) == -2 and b'aligned' in err(), kw
    assert nearest(c=0) == -1
    assert nearest(rows=fake) == -1 and b'exactly one' in err()
    assert nearest(x=None) == -1 and b'exactly one' in err()
    assert nearest(centres=None) == -1 and nearest(idx=None, d2=None) == -1 and b'NULL' in err()
    assert nearest(x=None, rows=odd) == -2 and nearest(centres=odd) == -2 and b'aligned' in err()


# ------------------------------------------------------------------------------------------------------------------------------------------ parsers
def test_p2_parser_accepts_the_meanshift_flags_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    a = p2.get_arguments([])
    assert (a.cluster_method, a.k_max, a.select_eps, a.n_init, a.gap_b, a.opt_eps) == ('kmeans', 10, 'k_distance_graph', 10, 10, 1.9)
    assert a.select_opt_k == ['gap_sts', 'elbow'] and a.restore_metric == ['ae_mse', 'loss']
    assert a.internal_metrics == ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert (a.consensus_reps, a.consensus_p_item, a.hdbscan_min_cluster_size, a.gmm_covariance_type, a.metric_sample) == (100, 0.8, None, 'diag', 0)
    assert (a.snn_k, a.snn_eps, a.snn_min_samples) == (None, None, None)
    assert (a.meanshift_quantile, a.meanshift_bandwidth, a.meanshift_bin_seeding, a.meanshift_cluster_all) == ([0.1, 0.2, 0.3], None, False, 1)
    a = p2.get_arguments(['--cluster_method', 'meanshift', '--meanshift_quantile', '0.05', '0.25', '--meanshift_bin_seeding', '--meanshift_cluster_all', '0'])
    assert (a.cluster_method, a.meanshift_quantile, a.meanshift_bin_seeding, a.meanshift_cluster_all) == ('meanshift', [0.05, 0.25], True, 0)
    a = p2.get_arguments(['--cluster_method', 'meanshift', '--meanshift_bandwidth', '2.5', '4'])
    assert a.meanshift_bandwidth == [2.5, 4.0]
    for bad in (['--meanshift_quantile', 'x'], ['--meanshift_cluster_all', '2'], ['--meanshift_bandwidth', 'wide']):
        with pytest.raises(SystemExit):
            p2.get_arguments(bad)
    assert p2.Meanshift.COLUMNS == ['quantile', 'bandwidth', 'n_clusters', 'n_orphans', 'largest', 'smallest', 'n_iter', 'valid_distortion']
    assert p2.Meanshift.FILES == ('meanshift_bandwidth.csv', 'meanshift_labels.csv', 'meanshift_centers.csv')


def test_p4_parser_accepts_the_meanshift_flags_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p4.get_arguments([])
    assert (a.cluster_method, a.num_clusters, a.opt_eps, a.hdbscan_min_cluster_size, a.transfer, a.transfer_k, a.dl_cluster_label_type) == (
        'kmeans', 4, 1.9, None, 'centre', None, 'pred')
    assert a.restore_metric == ['ae_mse', 'loss', 'delta'] and (a.snn_k, a.snn_eps, a.snn_min_samples) == (None, None, None)
    assert (a.meanshift_bandwidth, a.meanshift_quantile, a.meanshift_bin_seeding, a.meanshift_cluster_all) == (None, None, False, 1)
    a = p4.get_arguments(['--cluster_method', 'meanshift', '--meanshift_bandwidth', '3.5', '--meanshift_cluster_all', '0'])
    assert (a.cluster_method, a.meanshift_bandwidth, a.meanshift_cluster_all) == ('meanshift', 3.5, 0)
    a = p4.get_arguments(['--cluster_method', 'meanshift', '--meanshift_quantile', '0.2'])
    assert a.meanshift_quantile == 0.2
    for bad in (['--meanshift_quantile', 'x'], ['--meanshift_bandwidth', '2', '3']):
        with pytest.raises(SystemExit):
            p4.get_arguments(bad)


# --------------------------------------------------------------------------------------------------------------------------------------- registers
def test_meanshift_kernels_do_not_spill_to_scratch():
    """The members epilogue runs 64 times per lane per tile beside 128 live accumulators, and the shift kernel's f64 accumulators are sized for four waves per SIMD: a
    register in scratch memory would be paid on every one.  Require ScratchSize == 0 and no vector-register spills for every kernel of dic_meanshift.hip, by
    name (the prep kernels of dic_pairtile.h the file instantiates included)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_meanshift.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'warning' not in res.stderr
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('ms_seed_prep_kernel', 'pt_mask_cols_kernel', 'ms_members_kernel', 'ms_recheck_kernel', 'ms_shift_kernelILi1ELi1E', 'ms_shift_kernelILi4ELi1E',
                   'ms_shift_kernelILi4ELi4E', 'ms_nearest_kernel', 'pt_prep_kernel', 'pt_block_max_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
