"""GPU checks of consensus clustering (consensus.py, csrc/dic_consensus.hip).  The kernels are held, independently of k-means, to numpy integers on synthetic
label matrices: the histogram exactly, the distance matrix bit for bit, the row sums at 1e-12 (f64 sums of at most N terms in [0, 1] whose order differs from
numpy's: N * 2^-53 relative is 6e-14 at the largest N here).  The agglomeration is held exactly, heights included, to the numpy restatement of scipy's
nearest-neighbour chain in test_consensus_host.py (which that file holds to scipy): both sides evaluate one correctly rounded f64 expression per update and
break ties by index.  The tile edge of the pair pass is 128: N = 127, 129 and 257 sit around one and two tiles."""
import functools
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import consensus
from deep_interpolation_clustering_amd.consensus import BINS, ConsensusKMeans, average_linkage, consensus_pairs, cut_linkage
from deep_interpolation_clustering_amd.info import COHORTS
from test_consensus_host import distance, histogram, pair_counts, synthetic_labels, yardstick_linkage

pytestmark = pytest.mark.gpu

# name -> (N, H, K)
SHAPES = {'n2': (2, 1, 2), 'n255': (255, 4, 2), 'n257': (257, 7, 3), 'n300': (300, 33, 5), 'n513': (513, 100, 20), 'k254': (257, 255, 254),
          'n127': (127, 17, 4), 'n129': (129, 64, 4), 'never': (140, 20, 3), 'full': (200, 48, 6), 'same': (131, 10, 3)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(L (N, H) uint8, y (N,) 0-based labels for the row sums, K, agree, both, D, hist, rowsum) -- computed once, never modified."""
    n, h, k = SHAPES[name]
    seed = 1000 + n + h + k
    if name == 'full':
        L = synthetic_labels(n, h, k, seed, unsampled=0.0)
        assert not (L == 0xFF).any()
    elif name == 'same':
        L = np.repeat(synthetic_labels(1, h, k, seed), n, axis=0)
    else:
        L = synthetic_labels(n, h, k, seed)
    if name == 'never':
        L[37] = 0xFF          # a point no resample ever drew: both == 0 against everyone
    rng = np.random.default_rng(seed + 1)
    y = rng.integers(0, k, n)
    if k > 2:
        y[y == 1] = 0          # a cluster without members
    agree, both = pair_counts(L)
    d = distance(agree, both)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.where(both > 0, agree / np.maximum(both, 1), 0.0)
    np.fill_diagonal(m, 0.0)
    rowsum = np.stack([m[:, y == c].sum(axis=1) for c in range(k)], axis=1)
    for a in (L, y, agree, both, d, rowsum):
        a.setflags(write=False)
    return L, y, k, agree, both, d, histogram(agree, both), rowsum


@functools.lru_cache(maxsize=None)
def reference_linkage(name):
    Z = yardstick_linkage(case(name)[5])
    Z.setflags(write=False)
    return Z


def test_cases_have_what_they_claim():
    assert (case('never')[4][37] == 0).all() and (case('never')[5][37, :37] == 1.0).all()
    assert (case('same')[5] == 0).all()
    assert (case('n257')[4][np.triu_indices(257, 1)] == 0).any()          # pairs never sampled together
    assert len(np.unique(case('k254')[0])) >= 200
    h = case('n513')[6]
    assert (h[1:BINS] > 0).sum() >= 20          # the bins between the ends are used, not only 0 and 100


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_pair_pass_against_numpy_integers(name):
    L, y, k, agree, both, d_ref, hist_ref, rowsum_ref = case(name)
    n = len(L)
    hist, rowsum, D = consensus_pairs(L, y=y, want_distance=True, n_clusters=k)
    assert hist.dtype == np.uint64 and hist.shape == (BINS + 1,) and int(hist.sum()) == n * (n - 1) // 2
    np.testing.assert_array_equal(hist, hist_ref)
    assert D.is_cuda and D.dtype == torch.float64 and tuple(D.shape) == (n, n)
    d = D.cpu().numpy()
    assert np.array_equal(d, d_ref)          # bit-equal: one f64 division, one subtraction
    assert np.array_equal(d, d.T) and (np.diag(d) == 0).all()
    assert rowsum.shape == (n, k) and rowsum.dtype == np.float64
    np.testing.assert_allclose(rowsum, rowsum_ref, rtol=1e-12, atol=0)
    # a subset of the outputs: the same bits
    h1, r1, d1 = consensus_pairs(L)
    assert r1 is None and d1 is None and np.array_equal(h1, hist)
    h2, r2, d2 = consensus_pairs(L, want_distance=True, want_hist=False)
    assert h2 is None and r2 is None and np.array_equal(d2.cpu().numpy(), d)
    h3, r3, d3 = consensus_pairs(L, y=y, want_hist=False, n_clusters=k)
    assert h3 is None and d3 is None and np.array_equal(r3, rowsum)
    # a device tensor, already padded to a multiple of 16 columns
    Lp = torch.full((n, -(-L.shape[1] // 16) * 16), 0xFF, dtype=torch.uint8, device='cuda')
    Lp[:, :L.shape[1]] = torch.as_tensor(L, device='cuda')
    h4, r4, d4 = consensus_pairs(Lp, y=torch.as_tensor(y, device='cuda'), want_distance=True, n_clusters=k)
    assert np.array_equal(h4, hist) and np.array_equal(r4, rowsum) and np.array_equal(d4.cpu().numpy(), d)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_average_linkage_equals_the_yardstick_exactly(name):
    d_ref = case(name)[5]
    n = len(d_ref)
    ref = reference_linkage(name)
    Z = average_linkage(d_ref)
    assert Z.shape == (n - 1, 4) and Z.dtype == np.float64
    assert np.array_equal(Z, ref), int((Z != ref).any(axis=1).argmax())
    # from the kernel's own matrix, on the device; the caller's tensor survives unless it says otherwise
    _, _, D = consensus_pairs(case(name)[0], want_distance=True, want_hist=False)
    keep = D.clone()
    assert np.array_equal(average_linkage(D), ref) and torch.equal(D, keep)
    assert np.array_equal(average_linkage(D, overwrite=True), ref)
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
    except ImportError:
        return
    if n > 2:
        assert np.array_equal(Z, linkage(squareform(d_ref, checks=False), 'average'))


def test_cut_of_the_device_linkage():
    L, _, k, _, _, d_ref, _, _ = case('n300')
    labels = cut_linkage(average_linkage(d_ref), k)
    np.testing.assert_array_equal(labels, cut_linkage(reference_linkage('n300'), k))
    assert sorted(set(labels.tolist())) == list(range(1, k + 1))


def test_memory_guard_raises_before_any_launch(monkeypatch):
    n = 300
    d = np.zeros((n, n))
    calls = []
    lib = consensus.N.lib()

    class Spy:
        def __getattr__(self, name):
            if name in ('dic_linkage_average', 'dic_consensus_pairs'):
                calls.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(consensus.N, 'lib', lambda: Spy())
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (8 * n * n - 1, 1 << 40))
    with pytest.raises(MemoryError, match=str(8 * n * n)):
        average_linkage(d)
    with pytest.raises(MemoryError, match=str(8 * n * n)):
        consensus_pairs(case('n300')[0], want_distance=True)
    with pytest.raises(MemoryError, match='bytes'):
        ConsensusKMeans([2], reps=2).fit(np.zeros((n, 4), np.float32))
    assert not calls
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (8 * n * n, 1 << 40))
    assert average_linkage(d).shape == (n - 1, 4) and calls == ['dic_linkage_average']


def blobs(n=600, d=8, seed=5):
    rng = np.random.default_rng(seed)
    planted = rng.integers(0, 4, n)
    centres = rng.normal(0, 1, (4, d))
    centres *= 20.0 / np.linalg.norm(centres, axis=1, keepdims=True)
    return (centres[planted] + rng.normal(0, 0.3, (n, d))).astype(np.float32), planted


@functools.lru_cache(maxsize=None)
def blob_fit():
    X, planted = blobs()
    return X, planted, ConsensusKMeans([2, 3, 4, 5], reps=20).fit(X)


def test_end_to_end_on_four_blobs():
    X, planted, cc = blob_fit()
    n = len(X)
    assert sorted(cc.labels_) == [2, 3, 4, 5] and len(cc.resamples_) == 20 and all(len(r) == int(0.8 * n) for r in cc.resamples_)
    lab = cc.labels_[4]
    assert lab.dtype == np.int64 and lab.shape == (n,) and sorted(set(lab.tolist())) == [1, 2, 3, 4]
    # the planted partition, in canonical numbering
    _, first = np.unique(planted, return_index=True)
    canon = np.empty(4, dtype=np.int64)
    canon[np.argsort(first)] = np.arange(1, 5)
    np.testing.assert_array_equal(lab, canon[planted])
    areas = [cc.area_[k] for k in (2, 3, 4)]
    assert areas == sorted(areas)          # non-decreasing up to the planted K
    assert (cc.cluster_consensus_[4] == 1.0).all() and cc.cluster_consensus_[4].shape == (4,)
    item = cc.item_consensus_[4]
    assert item.shape == (n, 4) and (item[np.arange(n), lab - 1] == 1.0).all() and (item >= 0).all()
    for k in (2, 3, 4, 5):
        assert cc.cdf_[k].shape == (BINS + 1,) and cc.cdf_[k][-1] == 1.0 and int(cc.hist_[k].sum()) == n * (n - 1) // 2
        assert cc.linkage_[k].shape == (n - 1, 4) and cc.item_consensus_[k].shape == (n, k)
        np.testing.assert_array_equal(cc.labels_[k], cut_linkage(cc.linkage_[k], k))
    assert cc.delta_area_[2] == cc.area_[2] and cc.delta_area_[3] == (cc.area_[3] - cc.area_[2]) / cc.area_[2]


def _same_fit(a, b):
    for k in a.ks:
        assert np.array_equal(a.labels_[k], b.labels_[k]) and np.array_equal(a.cdf_[k], b.cdf_[k]) and np.array_equal(a.linkage_[k], b.linkage_[k])
        assert np.array_equal(a.hist_[k], b.hist_[k]) and np.array_equal(a.cluster_consensus_[k], b.cluster_consensus_[k], equal_nan=True)
        assert np.array_equal(a.item_consensus_[k], b.item_consensus_[k], equal_nan=True)


def test_same_seed_same_bits_and_tensor_equals_array():
    X, _, cc = blob_fit()
    _same_fit(cc, ConsensusKMeans([2, 3, 4, 5], reps=20).fit(X))
    _same_fit(cc, ConsensusKMeans([2, 3, 4, 5], reps=20).fit(torch.as_tensor(X, device='cuda')))
    other = ConsensusKMeans([3], reps=20, seed=1).fit(X)
    assert not all(np.array_equal(a, b) for a, b in zip(other.resamples_, cc.resamples_))


def test_label_matrix_layout():
    X, _, cc = blob_fit()
    res = cc.resamples_[:5]
    L = consensus.label_matrix(X, 3, res)
    assert L.is_cuda and L.dtype == torch.uint8 and tuple(L.shape) == (len(X), 16)
    Lh = L.cpu().numpy()
    assert (Lh[:, 5:] == 0xFF).all()
    for h, idx in enumerate(res):
        mask = np.zeros(len(X), bool)
        mask[idx] = True
        assert (Lh[~mask, h] == 0xFF).all() and (Lh[mask, h] < 3).all()


def _write_latents(root, sub, seed, n=(420, 300, 60), d=8):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (3, d))
    centres *= 15.0 / np.linalg.norm(centres, axis=1, keepdims=True)
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    out = {}
    for cohort, m in zip(COHORTS, n):
        lab = rng.integers(0, 3, m)
        h = (centres[lab] + rng.normal(0, 0.25, (m, d))).astype(np.float32)
        ob = rng.normal(100 + 10 * lab[:, None, None], 1.0, (m, 6, 12)).astype(np.float32)
        data = {'encounter_id': np.arange(m), 'hidden': h, 'ob': ob, 'padding_mask': np.ones((m, 6, 12), np.float32), 'planted': lab}
        np.save(os.path.join(root, sub, cohort + '.npy'), data)
        out[cohort] = data
    return out


def test_p2_then_p4_consensus_branches(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    feat2 = tmp_path / 'Results' / 'Pretrain' / 'out_feat'
    data = _write_latents(str(feat2), 'ae_mse', 11)
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'consensus', '--k_max', '4', '--consensus_reps', '12'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    plot = feat2 / 'ae_mse_consensus_aligned' / 'plot'
    raw = feat2 / 'raw_consensus_result'
    cdf, area = (pd.read_csv(plot / name, float_precision='round_trip') for name in ('consensus_cdf.csv', 'consensus_area.csv'))
    assert list(cdf.columns) == ['k', 'c', 'cdf'] and list(area.columns) == ['k', 'area', 'delta_area']
    assert len(cdf) == 3 * (BINS + 1) and area.k.tolist() == [2, 3, 4] and res['ae_mse'].k.tolist() == [2, 3, 4]
    np.testing.assert_array_equal(cdf.c.to_numpy()[:BINS + 1], np.arange(BINS + 1) / BINS)
    ref = ConsensusKMeans([2, 3, 4], reps=12).fit(data['training']['hidden'])
    np.testing.assert_array_equal(area.area.to_numpy(), [ref.area_[k] for k in (2, 3, 4)])
    np.testing.assert_array_equal(area.delta_area.to_numpy(), [ref.delta_area_[k] for k in (2, 3, 4)])
    np.testing.assert_array_equal(cdf.cdf.to_numpy()[(BINS + 1):2 * (BINS + 1)], ref.cdf_[3])
    tables = {}
    for cohort in ('training', 'validation'):
        t = pd.read_csv(raw / (cohort + '_consensus.csv'))
        assert list(t.columns) == ['k2', 'k3', 'k4'] and len(t) == len(data[cohort]['hidden'])
        assert all(sorted(set(t['k%d' % k].tolist())) == list(range(1, k + 1)) for k in (2, 3, 4))          # 1-based
        # K = 3 is the planted partition of either cohort
        pair = set(zip(t.k3.tolist(), data[cohort]['planted'].tolist()))
        assert len(pair) == 3
        tables[cohort] = t
    np.testing.assert_array_equal(tables['training'].k3.to_numpy(), ref.labels_[3])
    assert not (raw / 'testing_consensus.csv').exists()
    # a second run leaves the files alone
    co = p2.Consensus(4, str(plot.parent), str(raw), reps=12)
    stamps = [f.stat().st_mtime_ns for f in (plot / 'consensus_cdf.csv', raw / 'training_consensus.csv', raw / 'validation_consensus.csv')]
    again = co.train(data['training'], data['validation'])
    assert not co.fits_ and again.area.tolist() == area.area.tolist()
    assert [f.stat().st_mtime_ns for f in (plot / 'consensus_cdf.csv', raw / 'training_consensus.csv', raw / 'validation_consensus.csv')] == stamps

    # p4 reads Results/Clustering: the feature dump p3 would write there, p2's training labels, and NO validation file -- p4 computes that one itself
    feat4 = tmp_path / 'Results' / 'Clustering' / 'out_feat'
    os.makedirs(feat4 / 'ae_mse')
    os.makedirs(feat4 / 'raw_consensus_result')
    for cohort in COHORTS:
        np.save(feat4 / 'ae_mse' / (cohort + '.npy'), data[cohort])
    tables['training'].to_csv(feat4 / 'raw_consensus_result' / 'training_consensus.csv', index=False)
    a4 = p4.get_arguments(['--cluster_method', 'consensus', '--num_clusters', '3'])
    a4.restore_metric = ['ae_mse']
    p4.main(a4)
    made = pd.read_csv(feat4 / 'raw_consensus_result' / 'validation_consensus.csv')
    assert list(made.columns) == ['k3'] and len(set(zip(made.k3.tolist(), data['validation']['planted'].tolist()))) == 3
    for cohort, raw_col in (('training', tables['training'].k3.to_numpy()), ('validation', made.k3.to_numpy())):
        d = np.load(feat4 / 'ae_mse_consensus_aligned' / (cohort + '_3.npy'), allow_pickle=True).item()
        assert 'ob' not in d and 'padding_mask' not in d
        cid = d['cluster_id']
        assert sorted(set(cid.tolist())) == [0, 1, 2] and len(set(zip(cid.tolist(), raw_col.tolist()))) == 3          # a renumbering of the csv column
    # training clusters are numbered by descending sbp: planted 2 (sbp 120) is cluster 0
    d = np.load(feat4 / 'ae_mse_consensus_aligned' / 'training_3.npy', allow_pickle=True).item()
    np.testing.assert_array_equal(d['cluster_id'], 2 - data['training']['planted'])
    assert not (feat4 / 'ae_mse_consensus_aligned' / 'testing_3.npy').exists()
