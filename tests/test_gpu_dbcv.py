"""DBCV on the GPU (dbcv.py, csrc/dic_dbcv.hip) against the numpy restatement of the definition (dbcv_reference.py), and the p2 --validity dbcv files.

The data (``dbcv_reference.blobs``): 700 shuffled rows at D = 8 and D = 256 -- 47 noise rows and clusters of 300, 250, 97, 3, 2 and 1 members -- so that
segment boundaries fall inside a 64-row tile, the last tile is ragged, the fallback rules (a path of three, a pair) and a singleton occur, and one exact
duplicate pair lies in the largest cluster; a second case has a cluster made only of coincident rows.  At D = 256 the naive power (1 / d)^256 leaves f64's
range for a majority of the pairs (asserted).

The bars.  ``core_distances_``: rtol 1e-12 -- each term of S carries a relative error of about (d / 2) a few ulp = 1e-13, the terms are positive, the
-1 / d power shrinks it further; the terms the kernel leaves out are below 1e-17 of S (csrc/dic_dbcv.hip).  With the GPU's own ``a`` handed to the
restatement, the trees, the internal nodes and the arg-minima are discrete and must be IDENTICAL, and so must the sparseness, a maximum of ``a`` values and
distances: every coordinate is a multiple of 2^-10 below 32, so every d^2 is exact in f64 in any summation order and both sides hold the same bits
(``blobs`` has the count).  ``separation`` rtol 1e-12, ``validity`` and ``score`` atol 1e-10, as the restatement's own ``a`` differs by up to 1e-12."""
import functools

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import dbcv
from dbcv_reference import N_NOISE, SIZES, blobs, dmat, reference, split_at_random
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

DIMS = (8, 256)
FIELDS = ('score', 'cluster_ids', 'sizes', 'sparseness', 'separation', 'validity', 'nearest_cluster', 'core_distances_', 'internal_')


@functools.lru_cache(maxsize=None)
def case(D):
    """(X, labels, distance matrix, the restatement's result, the GPU's result) -- computed once, shared by every test, never written to."""
    X, labels = blobs(D)
    M = dmat(X)
    for arr in (X, labels, M):
        arr.setflags(write=False)
    return X, labels, M, reference(X, labels, D=M), dbcv.dbcv(X, labels)


def same_bits(a, b):
    for f in FIELDS:
        np.testing.assert_array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f)), err_msg=f)
    assert (a.n_noise, a.n_singletons) == (b.n_noise, b.n_singletons)


def test_the_naive_power_leaves_f64_for_most_pairs_at_256_features():
    _, _, M, ref, _ = case(256)
    far = M[M > 0]
    with np.errstate(over='ignore', under='ignore'):
        naive = (1.0 / far) ** 256
    lost = float(np.mean((naive == 0) | np.isinf(naive)))
    print('D = 256: distances %.3g .. %.3g, naive power lost for %.1f %% of the pairs; DBCV %.4f' % (far.min(), far.max(), 100 * lost, ref['score']))
    assert lost > 0.5 and np.all(np.isfinite(ref['core_distances_'][np.isfinite(ref['core_distances_'])]))


@pytest.mark.parametrize('D', DIMS)
def test_core_distances(D):
    _, labels, _, ref, got = case(D)
    kept = np.isin(labels, (0, 1, 2, 3, 4))
    assert np.all(np.isnan(got.core_distances_[~kept])) and np.all(got.core_distances_[kept] > 0)
    err = np.abs(got.core_distances_[kept] - ref['core_distances_'][kept]) / ref['core_distances_'][kept]
    print('D = %d: core distances, largest relative difference %.3g' % (D, err.max()))
    np.testing.assert_allclose(got.core_distances_[kept], ref['core_distances_'][kept], rtol=1e-12, atol=0)


@pytest.mark.parametrize('D', DIMS)
def test_trees_and_separation_with_the_gpus_own_core_distances(D):
    X, labels, M, _, got = case(D)
    ref = reference(X, labels, a=got.core_distances_, D=M)
    np.testing.assert_array_equal(got.internal_, ref['internal_'])
    np.testing.assert_array_equal(got.sparseness, ref['sparseness'])
    np.testing.assert_array_equal(got.nearest_cluster, ref['nearest_cluster'])
    print('D = %d: separation, largest relative difference %.3g' % (D, (np.abs(got.separation - ref['separation']) / ref['separation']).max()))
    np.testing.assert_allclose(got.separation, ref['separation'], rtol=1e-12, atol=0)
    # the fallback rules occurred: the path of three has one internal node, the pair its first member
    for c, n_internal in ((3, 1), (4, 1)):
        assert got.internal_[labels == c].sum() == n_internal
    assert got.internal_[np.flatnonzero(labels == 4)[0]] and not got.internal_[labels == 5].any() and not got.internal_[labels == -1].any()


@pytest.mark.parametrize('D', DIMS)
def test_validity_and_score(D):
    _, _, _, ref, got = case(D)
    assert got.cluster_ids.tolist() == [0, 1, 2, 3, 4] and got.sizes.tolist() == list(SIZES[:5])
    assert (got.n_noise, got.n_singletons) == (N_NOISE, 1)
    print('D = %d: DBCV %.6f (restatement %.6f), largest validity difference %.3g' % (D, got.score, ref['score'],
                                                                                      np.abs(got.validity - ref['validity']).max()))
    np.testing.assert_allclose(got.validity, ref['validity'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got.score, ref['score'], rtol=0, atol=1e-10)
    assert np.all(np.abs(got.validity) <= 1) and abs(got.score) <= 1


@pytest.mark.parametrize('D', DIMS)
def test_a_random_split_scores_lower(D):
    X, labels, M, ref, got = case(D)
    cut_labels = split_at_random(labels, 0, 6)
    cut, cut_ref = dbcv.dbcv(X, cut_labels), reference(X, cut_labels, D=M)
    print('D = %d: DBCV %.4f, after the split %.4f' % (D, got.score, cut.score))
    np.testing.assert_allclose(cut.score, cut_ref['score'], rtol=0, atol=1e-10)
    assert cut.score < got.score and np.all(cut.validity[np.isin(cut.cluster_ids, (0, 6))] < 0)


def test_a_cluster_of_coincident_rows():
    X, labels, _, _, _ = case(8)
    Y = np.concatenate([np.full((5, 8), 0.25, np.float32), X[labels == 1][:70], X[labels == 2][:60]])
    lab = np.array([4] * 5 + [9] * 70 + [2] * 60)
    got, ref = dbcv.dbcv(Y, lab), reference(Y, lab)
    assert got.cluster_ids.tolist() == [2, 4, 9]
    assert np.all(got.core_distances_[:5] == 0) and got.sparseness[1] == 0 and got.validity[1] == 1
    np.testing.assert_allclose(got.core_distances_, ref['core_distances_'], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got.nearest_cluster, ref['nearest_cluster'])
    np.testing.assert_allclose(got.score, ref['score'], rtol=0, atol=1e-10)


@pytest.mark.parametrize('D', DIMS)
def test_calls_tensors_and_sweeps_give_the_same_bits(D):
    X, labels, _, _, got = case(D)
    same_bits(dbcv.dbcv(X, labels), got)
    same_bits(dbcv.dbcv(torch.as_tensor(X, device='cuda'), labels), got)
    cut_labels = split_at_random(labels, 0, 6)
    sweep = dbcv.dbcv_sweep(X, {'whole': labels, 'cut': cut_labels})
    assert list(sweep) == ['whole', 'cut']
    same_bits(sweep['whole'], got)
    same_bits(sweep['cut'], dbcv.dbcv(X, cut_labels))
    score, per = dbcv.validity_index(X, labels, per_cluster=True)
    assert score == got.score == dbcv.validity_index(X, labels) and np.array_equal(per, got.validity)
    assert dbcv.validity_index(X, labels, d=3) != got.score


def test_errors():
    X, labels, _, _, _ = case(8)
    with pytest.raises(ValueError):
        dbcv.dbcv(X, np.where(labels == 0, 0, -1))          # one cluster
    with pytest.raises(ValueError):
        dbcv.dbcv(X, labels[:-1])
    with pytest.raises(NotImplementedError):
        dbcv.dbcv(np.zeros((10, 260), np.float32), np.arange(10) % 2)


def test_p2_validity_dbcv(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    X = data['training']['hidden']
    k = X.shape[1] + 1
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'hdbscan', '--hdbscan_min_cluster_size', str(k), str(3 * k), '--validity', 'dbcv'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_hdbscan_aligned' / 'plot'
    labels = pd.read_csv(plot / 'hdbscan_labels.csv')
    table, clusters = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Dbcv.FILES)          # (%.17g: exact)
    assert list(table.columns) == ['labelling', 'n_clusters', 'n_noise', 'n_singletons', 'dbcv']
    assert list(clusters.columns) == ['labelling', 'cluster', 'size', 'sparseness', 'separation', 'nearest_cluster', 'validity']
    assert table.labelling.tolist() == list(labels.columns) == ['mcs%d' % k, 'mcs%d' % (3 * k)]
    for row, name in enumerate(labels.columns):
        res = dbcv.dbcv(X, labels[name].to_numpy())
        assert table.dbcv[row] == res.score == dbcv.validity_index(X, labels[name].to_numpy())
        assert (int(table.n_clusters[row]), int(table.n_noise[row]), int(table.n_singletons[row])) == (len(res.cluster_ids), res.n_noise, res.n_singletons)
        part = clusters[clusters.labelling == name]
        assert part.cluster.tolist() == res.cluster_ids.tolist() and part['size'].tolist() == res.sizes.tolist()
        assert part.nearest_cluster.tolist() == res.nearest_cluster.tolist()
        for f in ('sparseness', 'separation', 'validity'):
            assert np.array_equal(part[f].to_numpy(), getattr(res, f))
        assert len(res.cluster_ids) >= 3 and -1 <= res.score <= 1
    # a second run leaves the files alone; overwrite=True writes them again
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Dbcv.FILES]
    p2.main(args)
    assert stamps == [(plot / name).stat().st_mtime_ns for name in p2.Dbcv.FILES]
    p2.Dbcv(str(plot.parent), 'hdbscan').train(data['training'], data['validation'], overwrite=True)
    assert all(a < (plot / name).stat().st_mtime_ns for a, name in zip(stamps, p2.Dbcv.FILES))
    again = pd.read_csv(plot / 'dbcv.csv', float_precision='round_trip')
    assert again.dbcv.tolist() == table.dbcv.tolist()
    # a method that writes no label file is logged and skipped
    assert p2.Dbcv(str(plot.parent), 'optics').train(data['training'], data['validation']) is None


def test_p4_validity_dbcv(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    base = ['--cluster_method', 'ward', '--num_clusters', '3']
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_ward_aligned'
    args = p4.get_arguments(base + ['--validity', 'dbcv'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert sorted(p.name for p in out.iterdir() if 'dbcv' in p.name) == sorted('%s_dbcv%s.csv' % (c, s) for c in data for s in ('', '_clusters'))
    for cohort in data:
        saved = np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item()
        res = dbcv.dbcv(data[cohort]['hidden'], np.asarray(saved['cluster_id']).astype(np.int64))
        table = pd.read_csv(out / ('%s_dbcv.csv' % cohort), float_precision='round_trip')
        assert table.labelling.tolist() == ['%s_3.npy' % cohort] and table.dbcv[0] == res.score and int(table.n_clusters[0]) == 3
        clusters = pd.read_csv(out / ('%s_dbcv_clusters.csv' % cohort), float_precision='round_trip')
        assert np.array_equal(clusters.validity.to_numpy(), res.validity) and clusters['size'].tolist() == res.sizes.tolist()
