"""The host side of DBCV (dbcv.py: plain numpy on the walks' arrays) on hand-made trees, and the properties of the numpy restatement of the definition
(dbcv_reference.py) that test_gpu_dbcv.py holds the kernels to.  No GPU."""
import functools

import numpy as np
import pytest

from deep_interpolation_clustering_amd import dbcv
from dbcv_reference import N_NOISE, SIZES, blobs, dmat, reference, split_at_random, tree_rules

INF = np.inf


def rules(pred, reach):
    pred, reach = np.array(pred), np.array(reach, dtype=np.float64)
    dsc, internal = dbcv.sparseness(pred, reach)
    return dsc, internal.tolist(), dbcv.internal_edges(pred, internal).tolist()


def test_path_of_three_has_one_internal_node_and_falls_back_to_all_edges():
    dsc, internal, edges = rules([-1, 0, 1], [INF, 2.0, 5.0])
    assert internal == [False, True, False] and edges == [False, True, True] and dsc == 5.0
    assert dbcv.tree_degrees([-1, 0, 1]).tolist() == [1, 2, 1]


def test_star_has_its_centre_as_the_internal_node_and_all_edges():
    dsc, internal, edges = rules([-1, 0, 0, 0, 0], [INF, 1.0, 4.0, 3.0, 2.0])
    assert internal == [True, False, False, False, False] and edges == [False, True, True, True, True] and dsc == 4.0


def test_pair_has_its_first_member_as_the_internal_node():
    dsc, internal, edges = rules([-1, 0], [INF, 7.0])
    assert internal == [True, False] and edges == [False, True] and dsc == 7.0


def test_a_leaf_edge_that_is_the_maximum_is_ignored():
    # 0 - 1 - 2 - 3 with the leaf 4 hanging off 1 at the largest weight: internal nodes 1 and 2, the one internal edge is 1 - 2
    dsc, internal, edges = rules([-1, 0, 1, 2, 1], [INF, 1.0, 2.0, 3.0, 9.0])
    assert internal == [False, True, True, False, False] and edges == [False, False, True, False, False] and dsc == 2.0


def test_host_rules_equal_the_restatement_on_random_trees():
    rng = np.random.RandomState(3)
    for n in (2, 3, 4, 7, 30, 200):
        for _ in range(5):
            pred = np.array([-1] + [rng.randint(0, q) for q in range(1, n)])
            reach = np.concatenate([[INF], rng.rand(n - 1)])
            dsc, internal = dbcv.sparseness(pred, reach)
            r_dsc, r_internal = tree_rules(reach, pred)
            assert dsc == r_dsc and np.array_equal(internal, r_internal)


def test_validity_and_weighted_score():
    v = dbcv.cluster_validity([1.0, 4.0, 0.0, 0.0], [4.0, 1.0, 0.0, 2.0])
    assert v.tolist() == [0.75, -0.75, 0.0, 1.0]
    assert dbcv.weighted_score([2, 2, 2, 2], v, 16) == pytest.approx(0.125, abs=1e-16)


def test_partition_keeps_clusters_of_two_or_more_sorted_by_cluster_then_row():
    ids, sizes, order, seg_start, n_noise, n_singletons = dbcv.partition(np.array([7, -1, 3, 7, 9, 3, 3, -1]))
    assert ids.tolist() == [3, 7] and sizes.tolist() == [3, 2] and order.tolist() == [2, 5, 6, 0, 3] and seg_start.tolist() == [0, 3, 5]
    assert n_noise == 2 and n_singletons == 1
    with pytest.raises(ValueError):
        dbcv.partition(np.array([0, 0, 0, 1, -1]))          # cluster 1 is a singleton: one cluster left
    with pytest.raises(ValueError):
        dbcv.partition(np.array([0.0, 1.0]))


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case():
    X, labels = blobs(8)
    D = dmat(X)
    for arr in (X, labels, D):
        arr.setflags(write=False)
    return X, labels, D, reference(X, labels, D=D)


def test_scores_lie_in_the_unit_range_and_the_counts_are_right():
    _, _, _, ref = case()
    assert np.all(np.abs(ref['validity']) <= 1) and -1 <= ref['score'] <= 1
    assert ref['cluster_ids'].tolist() == [0, 1, 2, 3, 4] and ref['sizes'].tolist() == list(SIZES[:5])
    assert ref['n_noise'] == N_NOISE and ref['n_singletons'] == 1
    assert ref['score'] > 0.3          # separated blobs
    print('D = 8 blobs: DBCV %.4f, V %s' % (ref['score'], np.round(ref['validity'], 3)))


def test_a_blob_split_at_random_scores_lower_and_its_halves_are_invalid():
    X, labels, D, ref = case()
    cut = reference(X, split_at_random(labels, 0, 6), D=D)
    halves = cut['validity'][np.isin(cut['cluster_ids'], (0, 6))]
    print('split: DBCV %.4f against %.4f, halves %s' % (cut['score'], ref['score'], halves))
    assert cut['score'] < ref['score'] and np.all(halves < 0)


def test_noise_rows_lower_the_score_by_exactly_their_share():
    X, labels, D, ref = case()
    keep = labels != -1
    clean = reference(X[keep], labels[keep], d=X.shape[1], D=D[np.ix_(keep, keep)])
    np.testing.assert_array_equal(clean['validity'], ref['validity'])
    np.testing.assert_allclose(ref['score'], clean['score'] * keep.sum() / len(labels), rtol=1e-14, atol=0)


def test_a_singleton_changes_nothing_but_the_row_count():
    X, labels, D, ref = case()
    keep = labels != 5          # the singleton
    without = reference(X[keep], labels[keep], d=X.shape[1], D=D[np.ix_(keep, keep)])
    assert without['n_singletons'] == 0
    np.testing.assert_array_equal(without['validity'], ref['validity'])
    np.testing.assert_allclose(ref['score'], without['score'] * keep.sum() / len(labels), rtol=1e-14, atol=0)
    as_noise = reference(X, np.where(labels == 5, -1, labels), D=D)
    assert as_noise['score'] == ref['score'] and as_noise['n_noise'] == N_NOISE + 1


def test_the_exponent_defaults_to_the_column_count():
    X, labels, D, ref = case()
    assert reference(X, labels, d=8, D=D)['score'] == ref['score']
    assert reference(X, labels, d=3, D=D)['score'] != ref['score']
    assert dbcv._exponent(None, 8) == 8 and dbcv._exponent(3, 8) == 3
    with pytest.raises(ValueError):
        dbcv._exponent(0, 8)


def test_coincident_members_are_skipped_and_a_cluster_of_them_has_zero_core_distance():
    X, labels, D, ref = case()
    rows = np.flatnonzero(labels == 0)
    twins = [r for r in rows if (D[r, rows] == 0).sum() == 2]
    assert len(twins) == 2 and ref['core_distances_'][twins[0]] == ref['core_distances_'][twins[1]] > 0
    Y = np.concatenate([np.zeros((5, 4), np.float32), X[labels == 1][:40, :4], X[labels == 2][:30, :4]])
    lab = np.array([0] * 5 + [1] * 40 + [2] * 30)
    res = reference(Y, lab)
    assert np.all(res['core_distances_'][:5] == 0) and res['sparseness'][0] == 0 and res['validity'][0] == 1


# ---- the C entry points without a GPU ------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    from deep_interpolation_clustering_amd import _native as N
    lib = N.lib()
    assert lib.dic_dbcv_workspace(75000, 12) >= 75000 * 4 and lib.dic_dbcv_workspace(0, 1) == 0 and lib.dic_dbcv_workspace(10, 11) == 0
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ws = lib.dic_dbcv_workspace(1000, 3)

    def core(x=fake, ldx=16, n=1000, d=16, seg=fake, k=3, dpow=16.0, a=fake, work=fake, nbytes=ws):
        return lib.dic_dbcv_core(x, ldx, n, d, seg, k, dpow, a, work, nbytes, None)

    def sep(x=fake, ldx=16, n=1000, d=16, seg=fake, k=3, a=fake, flag=fake, rowsep=fake, rowarg=fake, work=fake, nbytes=ws):
        return lib.dic_dbcv_separation(x, ldx, n, d, seg, k, a, flag, rowsep, rowarg, work, nbytes, None)

    for call in (core, sep):
        for kw in ({'x': None}, {'seg': None}, {'work': None}, {'a': None}, {'n': 0}, {'k': 0}, {'k': 1001}, {'ldx': 12}):
            assert call(**kw) == -1, kw
        for kw in ({'d': 260, 'ldx': 260}, {'d': 6, 'ldx': 8}, {'n': 1 << 30, 'k': 3}, {'x': odd}, {'work': odd}):
            assert call(**kw) == -2, kw
        assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()
    assert core(dpow=0.5) == -1 and core(dpow=1e6) == -1
    assert sep(flag=None) == -1 and sep(rowsep=None) == -1 and sep(rowsep=odd) == -2 and sep(rowarg=ctypes.c_void_p(4098)) == -2


def test_dbcv_kernels_do_not_spill_to_scratch():
    """Both tile kernels hold a 4 x 4 micro-tile of f64 accumulators per thread (csrc/dic_dbcv.hip): require ScratchSize == 0 and no vector-register spills
    for every kernel of the file."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_dbcv.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('dbcv_core_kernel', 'dbcv_sep_kernel', 'dbcv_rowseg_kernel', 'dbcv_collist_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills) == 4
    assert max(scratch) == 0 and max(spills) == 0, (names, scratch, spills)
