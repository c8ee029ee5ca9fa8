"""The local outlier factor without a GPU: the definition every layer is held to (include/dic_hip.h, lof.py), stated here in numpy on brute-force lists
(lexsort by (d2, index), sklearn's self-exclusion rule) and held to sklearn.neighbors.LocalOutlierFactor fed the same points as f64, to 1e-12 of the
largest value (the bar test_embedding_quality_host holds sklearn to; the two differ by about 1e-14).  Then lof.py's host side -- clamping, offsets,
labels, warnings and refusals, with the device fit replaced by the numpy definition -- the drivers' flags, the C ABI's argument checks and the kernels'
register use.  test_gpu_lof.py imports the definition and the point sets from here."""
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
from deep_interpolation_clustering_amd import lof as LOF

KS = (1, 5, 20, 35)
SHAPES = ((300, 8), (700, 64), (500, 256))
N_PLANTED = 5
TOL = 1e-12


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


# ------------------------------------------------------------------------------------------------------------------------- the definition, in numpy
def lists(X, Q=None, k=5):
    """``(dist (M, k) f64, idx (M, k) int64)``: the k rows of X with the smallest (d2, index) for every row of Q, in that order; with ``Q=None`` for every
    row of X with its own index left out: k + 1 are taken, the entry whose index is the row's own is dropped, the first column where it is not among them."""
    x = np.asarray(X, dtype=np.float64)
    self_join = Q is None
    q = x if self_join else np.asarray(Q, dtype=np.float64)
    d2 = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    ids = np.arange(len(x))
    order = np.lexsort((np.broadcast_to(ids, d2.shape), d2), axis=1)
    if self_join:
        o = order[:, :k + 1]
        keep = o != ids[:, None]
        keep[np.all(keep, axis=1), 0] = False
        o = o[keep].reshape(len(x), k)
    else:
        o = order[:, :k]
    return np.sqrt(np.take_along_axis(d2, o, 1)), o


def lof_fit(dist, idx, ks):
    """``{k: (nof, lrd, kdist)}`` of a fit from its self-excluded lists, every k on the prefix of the lists."""
    out = {}
    for k in ks:
        kd = dist[:, k - 1]
        reach = np.maximum(kd[idx[:, :k]], dist[:, :k])
        lrd = 1.0 / (reach.mean(1) + 1e-10)
        out[k] = (-(lrd[idx[:, :k]] / lrd[:, None]).mean(1), lrd, kd)
    return out


def lof_score(dist_q, idx_q, lrd, kd, k):
    """``score_samples`` of new rows from their lists against the fitted set and the fit's ``lrd`` and ``kdist`` at k."""
    reach = np.maximum(kd[idx_q[:, :k]], dist_q[:, :k])
    lrd_q = 1.0 / (reach.mean(1) + 1e-10)
    return -(lrd[idx_q[:, :k]] / lrd_q[:, None]).mean(1)


@functools.lru_cache(maxsize=None)
def cluster_sets():
    """``{(n, d): (X, Q)}`` f32: three Gaussian clusters with N_PLANTED planted outliers in the first rows, and 200 new points around the same centres."""
    rng = np.random.default_rng(0)
    out = {}
    for n, d in SHAPES:
        c = rng.normal(size=(3, d)) * 4
        X = (c[rng.integers(0, 3, n)] + rng.normal(size=(n, d))).astype(np.float32)
        X[:N_PLANTED] += 15 * rng.normal(size=(N_PLANTED, d)).astype(np.float32)
        Q = (c[rng.integers(0, 3, 200)] + 1.5 * rng.normal(size=(200, d))).astype(np.float32)
        out[(n, d)] = (X, Q)
    return out


@functools.lru_cache(maxsize=None)
def duplicates_set():
    """200 x 4 f32 with rows 50..59 copies of row 0: 11 copies of one point, more than k + 1 at k = 5."""
    X = np.random.default_rng(5).normal(size=(200, 4)).astype(np.float32)
    X[50:60] = X[0]
    return X


def numpy_fit_lists(X, ks, candidate_budget=None):
    """lof._fit_lists on the numpy definition, CPU tensors: lets the estimator's host side run without a GPU."""
    dist, idx = lists(np.asarray(X), k=ks[-1])
    fit = lof_fit(dist, idx, ks)
    return tuple(torch.as_tensor(np.stack([fit[k][c] for k in ks], axis=1)) for c in range(3))


@pytest.fixture
def host_fit(monkeypatch):
    monkeypatch.setattr(LOF, '_fit_lists', numpy_fit_lists)


# --------------------------------------------------------------------------------------------------------------------------------- against sklearn
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_definition_against_sklearn(shape):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X, Q = cluster_sets()[shape]
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    dist, idx = lists(X, k=max(KS))
    dist_q, idx_q = lists(X, Q, k=max(KS))
    mine = lof_fit(dist, idx, KS)
    for k in KS:
        nof, lrd, kd = mine[k]
        sk = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm='brute').fit(X64)
        err = np.abs(sk.negative_outlier_factor_ - nof).max() / np.abs(sk.negative_outlier_factor_).max()
        skn = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm='brute', novelty=True).fit(X64)
        s = skn.score_samples(Q64)
        err_q = np.abs(s - lof_score(dist_q, idx_q, lrd, kd, k)).max() / np.abs(s).max()
        skc = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm='brute', contamination=0.05).fit(X64)
        err_off = abs(LOF.offset_of(nof, 0.05) - skc.offset_) / abs(skc.offset_)
        print('%s k=%d: fit %.2e novelty %.2e offset %.2e' % (shape, k, err, err_q, err_off))
        assert err <= TOL and err_q <= TOL and err_off <= TOL
        assert set(np.argsort(nof)[:N_PLANTED].tolist()) == set(range(N_PLANTED))          # the planted outliers are the five smallest
        assert LOF.offset_of(nof, 'auto') == -1.5 == sk.offset_


def test_duplicates_keep_sklearns_values_and_warning(host_fit):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = duplicates_set()
    dist, idx = lists(X, k=5)
    nof = lof_fit(dist, idx, [5])[5][0]
    with pytest.warns(UserWarning) as theirs:
        sk = neighbors.LocalOutlierFactor(n_neighbors=5, algorithm='brute').fit(X.astype(np.float64))
    assert nof.min() < -1e9 and np.abs(sk.negative_outlier_factor_ - nof).max() / np.abs(sk.negative_outlier_factor_).max() <= TOL
    with pytest.warns(UserWarning) as ours:
        fit = LOF.LocalOutlierFactor(n_neighbors=5).fit(X)
    assert [str(w.message) for w in ours] == [str(w.message) for w in theirs] and 'Duplicate values are leading to incorrect results' in str(ours[0].message)
    assert np.array_equal(fit.negative_outlier_factor_, nof)
    with warnings.catch_warnings():          # a novelty fit does not warn (sklearn: "novelty must also be false")
        warnings.simplefilter('error')
        LOF.LocalOutlierFactor(n_neighbors=5, novelty=True).fit(X)


def test_clamping(host_fit):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = cluster_sets()[(300, 8)][0][:40]
    with pytest.warns(UserWarning) as theirs:
        sk = neighbors.LocalOutlierFactor(n_neighbors=50, algorithm='brute').fit(X.astype(np.float64))
    with pytest.warns(UserWarning) as ours:
        fit = LOF.LocalOutlierFactor(n_neighbors=50).fit(X)
    assert [str(w.message) for w in ours] == [str(w.message) for w in theirs] and 'will be set to (n_samples - 1) for estimation' in str(ours[0].message)
    assert fit.n_neighbors_ == sk.n_neighbors_ == 39
    assert np.abs(fit.negative_outlier_factor_ - sk.negative_outlier_factor_).max() <= TOL * np.abs(sk.negative_outlier_factor_).max()
    with pytest.warns(UserWarning, match=r'n_neighbors \(40\) is equal to the total number of samples \(40\)'):          # every clamp warns here
        assert LOF.LocalOutlierFactor(n_neighbors=40).fit(X).n_neighbors_ == 39
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert LOF.LocalOutlierFactor(n_neighbors=39).fit(X).n_neighbors_ == 39
    two = LOF.LocalOutlierFactor(n_neighbors=1).fit(X[:2])
    assert two.n_neighbors_ == 1 and two.negative_outlier_factor_.shape == (2,)


def test_estimator_host_side_against_sklearn(host_fit):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = cluster_sets()[(300, 8)][0]
    for k in (5, 20):
        sk = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm='brute', contamination=0.05)
        theirs = sk.fit_predict(X.astype(np.float64))
        assert np.abs(sk.negative_outlier_factor_ - sk.offset_).min() > 1e-9          # no label hangs on the last bits
        est = LOF.LocalOutlierFactor(n_neighbors=k, contamination=0.05)
        ours = est.fit_predict(X)
        assert ours.dtype == theirs.dtype and np.array_equal(ours, theirs) and set(ours.tolist()) == {1, -1}
        assert abs(est.offset_ - sk.offset_) <= TOL * abs(sk.offset_) and est.n_neighbors_ == k
        assert np.array_equal(LOF.LocalOutlierFactor(n_neighbors=k, contamination=0.05, novelty=True).fit(X).predict(), theirs)
    auto = LOF.LocalOutlierFactor().fit(X)
    assert auto.n_neighbors == 20 and auto.contamination == 'auto' and auto.novelty is False and auto.offset_ == -1.5


def test_sklearn_words_the_errors_the_same_way():
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = np.zeros((5, 4), np.float32)

    def words(exc):          # (sklearn's available_if wraps the worded AttributeError in a generic one)
        return str(exc.__cause__ if isinstance(exc, AttributeError) and exc.__cause__ is not None else exc)

    for kw in ({'contamination': 0.7}, {'contamination': 0.0}, {'contamination': 'most'}, {'contamination': 1}, {'n_neighbors': 0}):
        with pytest.raises(ValueError) as a:
            neighbors.LocalOutlierFactor(**kw).fit(X.astype(np.float64))
        with pytest.raises(ValueError) as b:
            LOF.LocalOutlierFactor(**kw).fit(X)
        assert str(b.value) == str(a.value), kw
    for novelty, names in ((False, ('predict', 'score_samples', 'decision_function')), (True, ('fit_predict',))):
        for name in names:
            with pytest.raises(AttributeError) as a:
                getattr(neighbors.LocalOutlierFactor(novelty=novelty), name)(X)
            with pytest.raises(AttributeError) as b:
                getattr(LOF.LocalOutlierFactor(novelty=novelty), name)(X)
            assert str(b.value) == words(a.value), name


def test_argument_errors():
    X = np.zeros((50, 4), np.float32)
    with pytest.raises(NotImplementedError, match='at most 1023 neighbours'):
        LOF.lof_sweep(np.zeros((1100, 4), np.float32), [5, 1024])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        LOF.lof_sweep(np.zeros((50, 260), np.float32), [5])
    with pytest.raises(NotImplementedError, match='at most 64 values of k'):
        LOF.lof_sweep(np.zeros((100, 4), np.float32), list(range(1, 66)))
    with pytest.raises(ValueError, match='Expected n_neighbors < n_samples_fit, but n_neighbors = 50, n_samples_fit = 50, n_samples = 50'):
        LOF.lof_sweep(X, [5, 50])
    with pytest.raises(ValueError, match='Expected n_neighbors > 0. Got 0'):
        LOF.lof_sweep(X, [0])
    with pytest.raises(ValueError, match='integer'):
        LOF.lof_sweep(X, [2.5])
    with pytest.raises(ValueError, match='at least one'):
        LOF.lof_sweep(X, [])
    with pytest.raises(ValueError, match='2-D'):
        LOF.lof_sweep(np.zeros(5, np.float32), [1])
    with pytest.raises(NotImplementedError, match='at most 1023 neighbours'):
        LOF.LocalOutlierFactor(n_neighbors=1024).fit(np.zeros((1100, 4), np.float32))
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        LOF.LocalOutlierFactor().fit(np.zeros((50, 260), np.float32))
    with pytest.raises(RuntimeError, match='not fitted'):
        LOF.LocalOutlierFactor(novelty=True).score_samples(X)
    # lof_from_lists refuses on the host whatever needs no device
    d, i = torch.zeros((6, 4), dtype=torch.float64), torch.zeros((6, 4), dtype=torch.int32)
    for args, match in (((d, i.double(), [2]), 'idx must be integers'), ((d, i[:, :3], [2]), r'\(n_rows, width\) both'), ((d.float(), i, [2]), 'float64'),
                        ((d, i, [2, 5]), 'the lists hold 4 neighbours, n_neighbors = 5'), ((d, i, [3, 2]), 'ascending'), ((d, i, [0]), 'n_neighbors > 0'),
                        ((d.numpy(), i, [2]), 'torch tensors')):
        with pytest.raises(ValueError, match=match):
            LOF.lof_from_lists(*args)
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU'):
            LOF.lof_from_lists(d, i, [2])
        with pytest.raises(RuntimeError, match='no CPU path'):
            LOF.lof_sweep(X, [5])


def test_drop_self_is_sklearns_rule():
    X = duplicates_set()
    x = X.astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    ids = np.arange(len(x))
    order = np.lexsort((np.broadcast_to(ids, d2.shape), d2), axis=1)[:, :6]
    raw_dist = np.sqrt(np.take_along_axis(d2, order, 1))
    dist, idx = LOF.drop_self(torch.as_tensor(raw_dist), torch.as_tensor(order.astype(np.int32)))
    ref_dist, ref_idx = lists(X, k=5)
    assert not (order[55] == 55).any()          # a row whose own index is not among its k + 1: the first column leaves
    assert np.array_equal(idx.numpy(), ref_idx) and np.array_equal(dist.numpy(), ref_dist) and idx.dtype == torch.int32


def test_module_does_not_import_scipy_or_sklearn():
    with open(LOF.__file__) as f:
        text = f.read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', text, flags=re.M)


def test_parsers_accept_the_outlier_flags():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    for mod in (p2, p4):
        a = mod.get_arguments([])
        assert a.outlier is None and a.outlier_k == [20] and a.outlier_contamination == 'auto'
        a = mod.get_arguments(['--cluster_method', 'ward', '--outlier', 'lof', '--outlier_k', '5', '20', '--outlier_contamination', '0.05'])
        assert (a.cluster_method, a.outlier, a.outlier_k, a.outlier_contamination) == ('ward', 'lof', [5, 20], 0.05)
        with pytest.raises(SystemExit):
            mod.get_arguments(['--outlier', 'iforest'])
        with pytest.raises(SystemExit):
            mod.get_arguments(['--outlier_contamination', 'most'])
        with open(mod.__file__) as f:          # nothing of the feature is loaded by a run without the flag
            assert not re.search(r'^(import|from)\s+\S*lof', f.read(), flags=re.M)


def test_header_and_signatures_agree():
    names = {'dic_lof_lrd', 'dic_lof_scores'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    assert set(N.header_symbols()) == set(N.SIGNATURES)
    assert len(N.SIGNATURES['dic_lof_lrd'][1]) == 10 and len(N.SIGNATURES['dic_lof_scores'][1]) == 10


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    odd = ctypes.c_void_p((1 << 20) + 4)          # 4-B aligned only
    odd2 = ctypes.c_void_p((1 << 20) + 2)

    def ks_of(*v):
        return (ctypes.c_int * len(v))(*v)

    def lrd(dist=fake, idx=fake, m=100, ld=40, kdist=fake, n=100, ks=ks_of(5, 20), nk=2, out=fake):
        return lib.dic_lof_lrd(dist, idx, m, ld, kdist, n, ks, nk, out, None)

    def scores(idx=fake, m=100, ld=40, lrd_fit=fake, n=100, lrd_rows=fake, ks=ks_of(5, 20), nk=2, out=fake):
        return lib.dic_lof_scores(idx, m, ld, lrd_fit, n, lrd_rows, ks, nk, out, None)

    for call, pointers, doubles in ((lrd, ('dist', 'idx', 'kdist', 'ks', 'out'), ('dist', 'kdist', 'out')),
                                    (scores, ('idx', 'lrd_fit', 'lrd_rows', 'ks', 'out'), ('lrd_fit', 'lrd_rows', 'out'))):
        for name in pointers:
            assert call(**{name: None}) == -1 and b'NULL' in lib.dic_last_error_string(), name
        assert call(nk=0) == -1 and b'expected 1 <= nk <= 64' in lib.dic_last_error_string()
        assert call(nk=-2) == -1
        assert call(ks=ks_of(*range(1, 66)), nk=65, ld=100) == -2 and b'at most 64 values of k' in lib.dic_last_error_string()
        for ks in (ks_of(20, 5), ks_of(5, 5), ks_of(0, 5), ks_of(-1, 5), ks_of(5, 41)):
            assert call(ks=ks) == -1 and b'ascending' in lib.dic_last_error_string(), list(ks)
        assert call(ks=ks_of(41), nk=1) == -1 and b'ld = 40' in lib.dic_last_error_string()
        for kw in ({'ld': 0}, {'ld': -4}, {'m': 0}, {'n': 0}, {'m': -1}):
            assert call(**kw) == -1 and b'positive sizes' in lib.dic_last_error_string(), kw
        for kw in ({'m': 1 << 30}, {'n': 1 << 30}):
            assert call(**kw) == -2 and b'2^30' in lib.dic_last_error_string(), kw
        for name in doubles:
            assert call(**{name: odd}) == -2 and b'aligned' in lib.dic_last_error_string(), name
        assert call(idx=odd2) == -2 and b'aligned' in lib.dic_last_error_string()


def test_lof_kernels_do_not_spill_to_scratch():
    """Both kernels keep LOF_U gathers in flight per lane and index the by-value ks table per lane: neither may cost a register in scratch memory.  Require
    ScratchSize == 0 and no vector-register spills for every kernel of dic_lof.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_lof.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('lof_lrd_kernel', 'lof_scores_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills) == 2
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
