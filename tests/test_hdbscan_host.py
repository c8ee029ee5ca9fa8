"""CPU checks of the HDBSCAN pieces that need no GPU: the numpy restatements of hdbscan.py (single-linkage tree, condensed tree, label selection,
labelling at a cut) against sklearn's compiled ``make_single_linkage``, ``tree_to_labels`` and ``labelling_at_cut``, the parameter errors, the ABI's
argument checks and the register allocation of csrc/dic_hdbscan.hip.

The trees come from sklearn's own ``mst_from_mutual_reachability`` on the mutual-reachability matrix of ``dmat`` (test_gpu_optics.py's f64 difference-form
distances), sorted with ``kind='stable'`` -- the order hdbscan.py defines (its module docstring): point sets A, B, D, F of test_gpu_optics.py and two
quantised ones (integer coordinates, 400 x 4), where nearly every weight ties.  Labels must be equal; probabilities equal to 1e-15 absolute, because the
same operations run in the same order."""
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
from deep_interpolation_clustering_amd import hdbscan as H
from deep_interpolation_clustering_amd.hdbscan import HDBSCAN, condense_tree, hdbscan_mst, hdbscan_sizes, labelling_at_cut, single_linkage_tree, tree_to_labels
from test_gpu_optics import dmat, points

MIN_SAMPLES = {'A': 17, 'B': 5, 'D': 3, 'F': 7, 'Q1': 5, 'Q2': 9}
CASES = sorted(MIN_SAMPLES)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def quantised(seed):
    """400 x 4 with integer coordinates around three centres: a handful of distinct distances, so nearly every weight of the tree ties."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 6.0, (3, 4))
    return np.rint(centres[rng.integers(0, 3, 400)] + rng.normal(0, 1.5, (400, 4))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def walk(name):
    """sklearn's Prim on the case: ``(sklearn's MST records, ordering, reach, min_samples)``."""
    linkage = pytest.importorskip('sklearn.cluster._hdbscan._linkage')
    X = quantised({'Q1': 41, 'Q2': 42}[name]) if name.startswith('Q') else points(name)
    k = MIN_SAMPLES[name]
    D = dmat(X)
    core = np.sort(D, axis=1)[:, k - 1]
    mst = linkage.mst_from_mutual_reachability(np.maximum(np.maximum(D, core[:, None]), core[None, :]))
    ordering = np.concatenate([[0], mst['next_node']]).astype(np.int64)
    np.testing.assert_array_equal(mst['current_node'], ordering[:-1])          # sklearn's record holds the previous point of the walk
    reach = np.full(len(X), np.inf)
    reach[mst['next_node']] = mst['distance']
    return mst, ordering, reach, k


@functools.lru_cache(maxsize=None)
def trees(name):
    linkage = pytest.importorskip('sklearn.cluster._hdbscan._linkage')
    mst, ordering, reach, k = walk(name)
    ref = linkage.make_single_linkage(mst[np.argsort(mst['distance'], kind='stable')])
    return ref, single_linkage_tree(ordering, reach), k


def test_quantised_sets_tie_nearly_everywhere():
    for name in ('Q1', 'Q2'):
        w = walk(name)[0]['distance']
        ties = len(w) - len(np.unique(w))
        print('%s: %d of %d weights repeat an earlier one' % (name, ties, len(w)))
        assert ties >= 350


@pytest.mark.parametrize('name', CASES)
def test_single_linkage_tree_equals_sklearns(name):
    ref, got, _ = trees(name)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    for field in ('left_node', 'right_node', 'value', 'cluster_size'):
        np.testing.assert_array_equal(got[field], ref[field])


@pytest.mark.parametrize('name', CASES)
def test_labels_and_probabilities_equal_sklearns(name):
    tree = pytest.importorskip('sklearn.cluster._hdbscan._tree')
    ref_slt, slt, k = trees(name)
    w = np.sort(ref_slt['value'])
    inside = float(np.quantile(w[w > 0], 0.98))          # a cluster_selection_epsilon inside the range of the weights, above most splits
    n = len(slt) + 1
    found = set()
    for mcs in (k, 3 * k):
        cond = condense_tree(slt, mcs)
        ref_cond = tree._condense_tree(ref_slt, mcs)
        assert cond.dtype == ref_cond.dtype
        for field in ('parent', 'child', 'value', 'cluster_size'):
            np.testing.assert_array_equal(cond[field], ref_cond[field])
        for method in ('eom', 'leaf'):
            for eps in (0.0, inside):
                for single in (False, True):
                    for cap in (None, n // 4):
                        labels, prob = tree_to_labels(slt, mcs, method, single, eps, cap)
                        ref_labels, ref_prob = tree.tree_to_labels(ref_slt, mcs, method, single, eps, cap)
                        what = (name, mcs, method, eps, single, cap)
                        assert labels.shape == (n,) and labels.dtype.kind == 'i' and prob.dtype == np.float64
                        np.testing.assert_array_equal(labels, ref_labels, err_msg=str(what))
                        assert np.abs(prob - ref_prob).max() <= 1e-15, what
                        assert ((prob >= 0) & (prob <= 1)).all() and (prob[labels == -1] == 0).all()
                        found.add(labels.tobytes())
    assert len(found) >= 2          # (the settings do not all give the same clustering)


@pytest.mark.parametrize('name', CASES)
def test_labelling_at_cut_equals_sklearns(name):
    tree = pytest.importorskip('sklearn.cluster._hdbscan._tree')
    ref_slt, slt, k = trees(name)
    w = ref_slt['value']
    for cut in (0.0, float(w.min()), float(np.quantile(w, 0.3)), float(np.median(w)), float(np.quantile(w, 0.9)), float(w.max()), 2 * float(w.max())):
        for mcs in (1, 2, k, 3 * k):
            got = labelling_at_cut(slt, cut, mcs)
            np.testing.assert_array_equal(got, tree.labelling_at_cut(ref_slt, cut, mcs))
            assert got.dtype.kind == 'i'


def test_stable_and_unstable_sorts_can_differ():
    """What the module docstring says of sklearn's own sort, on case B: the two sort kinds order equal weights differently, and this module follows the
    stable one."""
    linkage = pytest.importorskip('sklearn.cluster._hdbscan._linkage')
    mst, ordering, reach, _ = walk('B')
    w = mst['distance']
    assert len(w) - len(np.unique(w)) >= 20
    stable = np.argsort(w, kind='stable')
    ties = np.flatnonzero(np.diff(w[stable]) == 0)
    assert (np.diff(stable)[ties] > 0).all()          # equal weights in the walk's order
    np.testing.assert_array_equal(single_linkage_tree(ordering, reach)['value'], linkage.make_single_linkage(mst[stable])['value'])


def test_two_points_and_zero_weights():
    # two points: one edge, no cluster of 2 points can split: everything is noise, or one cluster where that is allowed
    slt = single_linkage_tree(np.array([0, 1]), np.array([np.inf, 2.0]))
    assert slt.tolist() == [(0, 1, 2.0, 2)]
    labels, prob = tree_to_labels(slt, 2)
    assert labels.tolist() == [-1, -1] and prob.tolist() == [0.0, 0.0]
    labels, prob = tree_to_labels(slt, 2, allow_single_cluster=True)
    assert labels.tolist() == [0, 0] and prob.tolist() == [1.0, 1.0]
    # zero weights: lambda is inf there and the probability 1
    tree = pytest.importorskip('sklearn.cluster._hdbscan._tree')
    ordering = np.arange(12)
    reach = np.array([np.inf, 0, 0, 0, 3.0, 0, 0, 0, 5.0, 1.0, 1.0, 1.0])
    slt = single_linkage_tree(ordering, reach)
    mst = np.zeros(11, dtype=[('current_node', np.int64), ('next_node', np.int64), ('distance', np.float64)])
    mst['current_node'], mst['next_node'], mst['distance'] = ordering[:-1], ordering[1:], reach[1:]
    ref = pytest.importorskip('sklearn.cluster._hdbscan._linkage').make_single_linkage(mst[np.argsort(mst['distance'], kind='stable')])
    assert slt.tolist() == ref.tolist()
    for mcs in (2, 3, 4):
        for method in ('eom', 'leaf'):
            with np.errstate(all='ignore'):
                labels, prob = tree_to_labels(slt, mcs, method)
                ref_labels, ref_prob = tree.tree_to_labels(ref, mcs, method)
            np.testing.assert_array_equal(labels, ref_labels)
            np.testing.assert_array_equal(prob, ref_prob)


SK_MESSAGES = [
    ({'min_cluster_size': 1}, "The 'min_cluster_size' parameter of HDBSCAN must be an int in the range [2, inf). Got 1 instead."),
    ({'min_cluster_size': 2.5}, "The 'min_cluster_size' parameter of HDBSCAN must be an int in the range [2, inf). Got 2.5 instead."),
    ({'min_samples': 0}, "The 'min_samples' parameter of HDBSCAN must be an int in the range [1, inf) or None. Got 0 instead."),
    ({'cluster_selection_epsilon': -1.0}, "The 'cluster_selection_epsilon' parameter of HDBSCAN must be a float in the range [0.0, inf). Got -1.0 instead."),
    ({'max_cluster_size': 0}, "The 'max_cluster_size' parameter of HDBSCAN must be None or an int in the range [1, inf). Got 0 instead."),
    ({'cluster_selection_method': 'xi'}, "The 'cluster_selection_method' parameter of HDBSCAN must be a str among {'eom', 'leaf'}. Got 'xi' instead."),
    ({'allow_single_cluster': 'yes'},
     "The 'allow_single_cluster' parameter of HDBSCAN must be an instance of 'bool' or an instance of 'numpy.%s'. Got 'yes' instead." % np.bool_.__qualname__),
]


@pytest.mark.parametrize('kw, message', SK_MESSAGES)
def test_parameter_errors_are_sklearns(kw, message):
    X = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError, match=re.escape(message)):
        HDBSCAN(**kw).fit(X)
    sk = pytest.importorskip('sklearn.cluster')
    with pytest.raises(ValueError) as err:
        sk.HDBSCAN(**kw).fit(X.astype(np.float64))
    ours, theirs = message, str(err.value)
    if 'str among' in message:          # (sklearn prints a set: either order)
        ours, theirs = (s.replace("{'leaf', 'eom'}", "{'eom', 'leaf'}") for s in (ours, theirs))
    assert ours == theirs


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError, match='2-D'):
        hdbscan_mst(np.zeros(10, np.float32), 2)
    with pytest.raises(ValueError, match='2-D'):
        HDBSCAN().fit(torch.zeros(4, 3, 2))
    for bad in (0, -3, 1.5, True, 'x', None):
        with pytest.raises(ValueError, match='min_samples must be an int >= 1'):
            hdbscan_mst(X, bad)
    with pytest.raises(ValueError, match=re.escape('min_samples (11) must be at most the number of samples in X (10)')):
        hdbscan_mst(X, 11)
    with pytest.raises(ValueError, match=re.escape('min_samples (11) must be at most the number of samples in X (10)')):
        HDBSCAN(min_cluster_size=11).fit(X)          # (min_samples = None: min_cluster_size)
    with pytest.raises(ValueError, match='n_samples=1 while HDBSCAN requires more than one sample'):
        HDBSCAN().fit(X[:1])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        hdbscan_mst(np.zeros((10, 260), np.float32), 2)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        HDBSCAN().fit(np.zeros((10, 260), np.float32))
    with pytest.raises(NotImplementedError, match='pass the points'):
        HDBSCAN(metric='precomputed')
    for kw in ({'metric': 'manhattan'}, {'metric': 'cosine'}, {'metric_params': {'w': 1}}):
        with pytest.raises(NotImplementedError, match='only the euclidean metric'):
            HDBSCAN(**kw)
    with pytest.raises(NotImplementedError, match='alpha'):
        HDBSCAN(alpha=0.5)
    for centers in ('centroid', 'medoid', 'both'):
        with pytest.raises(NotImplementedError, match='store_centers'):
            HDBSCAN(store_centers=centers)
    with pytest.raises(ValueError, match="'min_cluster_size' parameter"):
        hdbscan_sizes(X, 3, [5, 1])
    with pytest.raises(ValueError, match='empty'):
        hdbscan_sizes(X, 3, [])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            hdbscan_mst(X, 3)
        with pytest.raises(RuntimeError, match='no CPU path'):
            HDBSCAN(min_cluster_size=3).fit_predict(X)


def test_module_does_not_import_sklearn():
    src = open(H.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+sklearn', src, flags=re.M)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_hdbscan_workspace(1000, 256)
    assert ws > 0 and lib.dic_hdbscan_workspace(1000, 260) == 0 and lib.dic_hdbscan_workspace(0, 256) == 0 and lib.dic_hdbscan_workspace(1 << 30, 256) == 0

    def call(X=fake, ldx=256, n=1000, d=256, core=fake, ordering=fake, reach=fake, pred=fake, work=fake, nbytes=ws):
        return lib.dic_hdbscan_mst(X, ldx, n, d, core, ordering, reach, pred, work, nbytes, None)

    for kw in ({'X': None}, {'core': None}, {'ordering': None}, {'reach': None}, {'pred': None}, {'work': None}):
        assert call(**kw) == -1
        assert b'NULL' in lib.dic_last_error_string()
    assert call(n=0) == -1 and call(ldx=128) == -1
    assert call(ldx=252, d=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
    assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
    assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert call(core=ctypes.c_void_p((1 << 20) + 4)) == -2
    assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()


def test_workspace_is_linear_in_n(lib):
    sizes = [lib.dic_hdbscan_workspace(n, 256) for n in (1, 255, 256, 257, 5000, 75000, 300000)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.dic_hdbscan_workspace(75000, 256) <= 75000 + (1 << 14)          # a flag byte per point, 4 KB of workgroup minima, the slot
    assert lib.dic_hdbscan_workspace(75000, 4) == lib.dic_hdbscan_workspace(75000, 256)


def test_hdbscan_kernels_do_not_spill_to_scratch():
    """A step is launched N - 1 times: registers that go to scratch memory would be paid 75 000 times.  Require ScratchSize == 0 and no spills for every
    kernel of dic_hdbscan.hip (dic_exactd2.h included)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_hdbscan.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    sspills = [int(v) for v in re.findall(r'SGPRs Spill: (\d+)', res.stderr)]
    assert any('hd_step_kernel' in n for n in names) and any('hd_init_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills) == len(sspills)
    assert max(scratch) == 0 and max(spills) == 0 and max(sspills) == 0, list(zip(names, scratch, spills, sspills))
