"""CPU checks of the OPTICS pieces that need no GPU: the two label extractions of optics.py against sklearn's, the Python argument errors, the ABI's
argument checks and the register allocation of csrc/dic_optics.hip.  The graphs the extractions run on come from the numpy yardstick of
test_gpu_optics.py (``oracle_optics`` on ``dmat``), on its cases A, B, D and G, plus a synthetic reachability plot."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import optics
from deep_interpolation_clustering_amd.optics import OPTICS, cluster_optics_dbscan, cluster_optics_xi, optics_graph
from test_gpu_optics import case


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def synthetic_plot():
    """A reachability plot written by hand, as (ordering, reachability, predecessor) of 400 points: plateaus, runs that fall and rise by EXACTLY the factor
    1 - xi per point (xi = 0.05 and 0.2: 0.95 and 0.8 are not dyadic, the products round, and the steep tests are <= / >= on those very values), valleys of
    three depths, nested valleys, unreachable (inf) points inside and at the ends, predecessors partly outside their valley."""
    rng = np.random.default_rng(77)
    seg = [np.array([np.inf]), np.full(12, 4.0)]
    for factor, floor in ((0.95, 1.0), (0.8, 0.5), (0.95, 2.5)):
        down = 4.0 * factor ** np.arange(1, 60)
        down = down[down >= floor]
        flat = np.full(25, down[-1]) * (1 + 0.01 * rng.uniform(-1, 1, 25))
        inner = np.concatenate([flat[:8], flat[8] * 0.8 ** np.arange(1, 4), np.full(9, flat[8] * 0.8 ** 3), flat[8] * 0.8 ** np.arange(2, -1, -1), flat[8:]])
        up = down[::-1]
        seg += [down, inner, up, np.full(6, 4.0)]
    # a valley whose right rim is higher than its left one: the cluster's end is moved down to the left rim's level, and the predecessor correction
    # (which only looks at clusters that end no lower than they start) has trailing points to drop
    low = 3.0 * 0.8 ** np.arange(1, 6)
    seg += [np.array([np.inf, np.inf]), np.full(8, 3.0), low, np.full(20, low[-1]) * (1 + 0.01 * rng.uniform(-1, 1, 20)), low[::-1], 3.0 / 0.8 ** np.arange(0, 3),
            np.array([np.inf])]
    plot = np.concatenate(seg)[:400]
    plot = np.concatenate([plot, np.full(400 - len(plot), 3.5)])
    n = len(plot)
    ordering = rng.permutation(n)
    reach = np.empty(n)
    reach[ordering] = plot
    pred_pos = np.maximum(np.arange(n) - rng.integers(1, 40, n), 0)          # a predecessor comes earlier in the ordering: up to 39 places,
    far = rng.random(n) < 0.3                                                # or, for three points in ten, anywhere before
    pred_pos[far] = (rng.random(n) * np.arange(n)).astype(np.int64)[far]
    pred_pos[1:][plot[1:] > 1.2 * plot[:-1]] = 0                             # and every point of a steep rise is reached from the very first point
    pred = np.empty(n, dtype=np.int64)
    pred[ordering] = ordering[pred_pos]
    pred[ordering[np.isinf(plot)]] = -1
    return ordering, reach, pred


def graphs():
    out = {}
    for name in ('A', 'B', 'D', 'G'):
        _, k, _, (o_ord, o_core, o_reach, o_pred, _) = case(name)
        out[name] = (o_ord, o_core, o_reach, o_pred, k)
    o, r, p = synthetic_plot()
    out['synthetic'] = (o, r.copy(), r, p, 5)          # (any core distances do for the xi extraction; the dbscan one gets the reachabilities)
    return out


@pytest.mark.parametrize('name', ['A', 'B', 'D', 'G', 'synthetic'])
def test_xi_extraction_equals_sklearns(name):
    sk = pytest.importorskip('sklearn.cluster')
    o_ord, _, o_reach, o_pred, k = graphs()[name]
    n = len(o_ord)
    found = 0
    for xi in (0.01, 0.05, 0.2):
        for mcs in (None, max(2, n // 50), 0.03):
            for corr in (True, False):
                kw = dict(reachability=o_reach, predecessor=o_pred, ordering=o_ord, min_samples=k, min_cluster_size=mcs, xi=xi, predecessor_correction=corr)
                labels, hier = cluster_optics_xi(**kw)
                ref_labels, ref_hier = sk.cluster_optics_xi(**kw)
                assert labels.shape == (n,) and hier.ndim == 2 and hier.shape[1] == 2 and hier.dtype.kind == 'i' and labels.dtype.kind == 'i'
                np.testing.assert_array_equal(labels, ref_labels)
                np.testing.assert_array_equal(hier, np.asarray(ref_hier).reshape(-1, 2))
                found += len(hier)
    assert found >= 18          # (one cluster per setting on average at the least: the comparison is not of empty lists)
    # min_samples as a fraction
    kw = dict(reachability=o_reach, predecessor=o_pred, ordering=o_ord, min_samples=0.02)
    np.testing.assert_array_equal(cluster_optics_xi(**kw)[0], sk.cluster_optics_xi(**kw)[0])


def test_synthetic_plot_has_what_it_claims():
    o, r, p = synthetic_plot()
    plot = r[o]
    with np.errstate(invalid='ignore'):
        ratio = plot[:-1] / plot[1:]
    assert np.isinf(plot).sum() >= 4 and (ratio == 1).sum() >= 20
    for keep in (0.95, 0.8):          # runs of exactly the factor: some land on either side of the comparison after rounding
        assert (np.abs(ratio - keep) < 1e-12).sum() >= 3 and (np.abs(ratio - 1 / keep) < 1e-12).sum() >= 3
    labels, hier = cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=5, xi=0.05)
    inside = (hier[:, None, 0] >= hier[None, :, 0]) & (hier[:, None, 1] <= hier[None, :, 1])
    assert len(hier) >= 4 and (inside.sum() - len(hier)) >= 1          # nested clusters
    with_corr = cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=5, xi=0.05, predecessor_correction=True)[1]
    without = cluster_optics_xi(reachability=r, predecessor=p, ordering=o, min_samples=5, xi=0.05, predecessor_correction=False)[1]
    assert not np.array_equal(with_corr, without)          # the correction has something to correct


@pytest.mark.parametrize('name', ['A', 'B', 'D', 'G', 'synthetic'])
def test_dbscan_extraction_equals_sklearns(name):
    sk = pytest.importorskip('sklearn.cluster')
    o_ord, o_core, o_reach, _, _ = graphs()[name]
    fin = o_core[np.isfinite(o_core)]
    for eps in (np.quantile(fin, 0.1), np.median(fin), np.quantile(fin, 0.9), 2 * fin.max(), 0.5 * fin.min(), np.inf):
        kw = dict(reachability=o_reach, core_distances=o_core, ordering=o_ord, eps=float(eps))
        got = cluster_optics_dbscan(**kw)
        np.testing.assert_array_equal(got, sk.cluster_optics_dbscan(**kw))
        assert got.dtype.kind == 'i'


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError, match='2-D'):
        optics_graph(np.zeros(10, np.float32), 2)
    with pytest.raises(ValueError, match='2-D'):
        OPTICS(min_samples=2).fit(torch.zeros(4, 3, 2))
    for bad in (0, 1, -3, 1.5, -0.1, True, 'x', None):
        with pytest.raises(ValueError, match='min_samples must be an int >= 2 or a float'):
            optics_graph(X, bad)
    with pytest.raises(ValueError, match=r'min_samples must be no greater than the number of samples \(10\). Got 11'):
        optics_graph(X, 11)
    with pytest.raises(ValueError, match='no greater than the number of samples'):
        OPTICS(min_samples=11).fit(X)
    with pytest.raises(ValueError, match='max_eps'):
        optics_graph(X, 2, max_eps=-1.0)
    with pytest.raises(ValueError, match='max_eps'):
        optics_graph(X, 2, max_eps=float('nan'))
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        optics_graph(np.zeros((10, 260), np.float32), 2)
    with pytest.raises(NotImplementedError, match='pass the points'):
        OPTICS(metric='precomputed')
    for kw in ({'metric': 'manhattan'}, {'metric': 'cosine'}, {'p': 1}, {'metric': 'minkowski', 'p': 3}, {'metric_params': {'w': 1}}):
        with pytest.raises(NotImplementedError, match='only the euclidean metric'):
            OPTICS(**kw)
    OPTICS(metric='minkowski', p=2)
    with pytest.raises(ValueError, match='cluster_method'):
        OPTICS(cluster_method='kmeans')
    with pytest.raises(ValueError, match='Specify an epsilon smaller than 1.0. Got 2.0.'):
        OPTICS(max_eps=1.0, cluster_method='dbscan', eps=2.0).fit(X)
    with pytest.raises(ValueError, match='min_cluster_size must be no greater'):
        cluster_optics_xi(reachability=np.ones(5), predecessor=np.zeros(5, int), ordering=np.arange(5), min_samples=2, min_cluster_size=6)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            optics_graph(X, 3)
        with pytest.raises(RuntimeError, match='no CPU path'):
            OPTICS(min_samples=3).fit_predict(X)


def test_sizes_resolve_as_sklearns():
    assert optics._resolve_size(5, 100, 'min_samples') == 5
    assert optics._resolve_size(0.25, 100, 'min_samples') == 25
    assert optics._resolve_size(0.001, 100, 'min_samples') == 2
    assert optics._resolve_size(1.0, 100, 'min_samples') == 100
    assert optics._resolve_size(np.int64(7), 100, 'min_samples') == 7 and optics._resolve_size(np.float32(0.5), 100, 'min_samples') == 50
    x = np.array([0.1234567890123456, 2.5, np.inf, 0.0])
    np.testing.assert_array_equal(optics.around15(x), np.rint(x * 1e15) / 1e15)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_optics_workspace(1000, 256)
    assert ws > 0 and lib.dic_optics_workspace(1000, 260) == 0 and lib.dic_optics_workspace(0, 256) == 0 and lib.dic_optics_workspace(1 << 30, 256) == 0

    def call(X=fake, ldx=256, n=1000, d=256, core=fake, max_eps=float('inf'), ordering=fake, reach=fake, pred=fake, work=fake, nbytes=ws):
        return lib.dic_optics_order(X, ldx, n, d, core, max_eps, ordering, reach, pred, work, nbytes, None)

    for kw in ({'X': None}, {'core': None}, {'ordering': None}, {'reach': None}, {'pred': None}, {'work': None}):
        assert call(**kw) == -1
        assert b'NULL' in lib.dic_last_error_string()
    assert call(n=0) == -1 and call(ldx=128) == -1
    assert call(max_eps=-1.0) == -1 and b'max_eps' in lib.dic_last_error_string()
    assert call(max_eps=float('nan')) == -1
    assert call(ldx=252, d=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
    assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
    assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert call(core=ctypes.c_void_p((1 << 20) + 4)) == -2
    assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()


def test_workspace_is_linear_in_n(lib):
    sizes = [lib.dic_optics_workspace(n, 256) for n in (1, 255, 256, 257, 5000, 75000, 300000)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.dic_optics_workspace(75000, 256) <= 75000 + (1 << 14)          # a flag byte per point, 4 KB of workgroup minima, the slot
    assert lib.dic_optics_workspace(75000, 4) == lib.dic_optics_workspace(75000, 256)


def test_optics_kernels_do_not_spill_to_scratch():
    """A step is launched N times: registers that go to scratch memory would be paid 75 000 times.  Require ScratchSize == 0 and no spills for every kernel of
    dic_optics.hip (dic_exactd2.h included)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_optics.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    sspills = [int(v) for v in re.findall(r'SGPRs Spill: (\d+)', res.stderr)]
    assert any('op_step_kernel' in n for n in names) and any('op_init_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills) == len(sspills)
    assert max(scratch) == 0 and max(spills) == 0 and max(sspills) == 0, list(zip(names, scratch, spills, sspills))
