"""CPU checks of the consensus clustering pieces that need no GPU: the numpy restatement of scipy's nearest-neighbour-chain average linkage (the yardstick
test_gpu_consensus.py holds the kernel to) against scipy itself, the host finish of a linkage (stable sort, relabelling), the cut, the CDF arithmetic, p4's
renumbering, and the ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import consensus
from deep_interpolation_clustering_amd.consensus import BINS, cdf_area, cut_linkage, delta_area

SHAPES = [(257, 7, 3), (300, 33, 5), (513, 100, 20)]          # (N, H, K); the first has pairs that were never sampled together


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def synthetic_labels(n, h, k, seed, flip=0.15, unsampled=0.20):
    """A label matrix (n, h) uint8 as k-means resamples would leave it: every row follows a planted label, 15 % of the entries are flipped to a random label,
    20 % are 0xFF (not in that resample)."""
    rng = np.random.default_rng(seed)
    planted = rng.integers(0, k, n)
    L = np.repeat(planted[:, None], h, axis=1)
    flips = rng.random((n, h)) < flip
    L[flips] = rng.integers(0, k, int(flips.sum()))
    L = L.astype(np.uint8)
    L[rng.random((n, h)) < unsampled] = 0xFF
    return L


def pair_counts(L):
    """(agree, both) (n, n) int64 of a label matrix, in integers."""
    sampled = L != 0xFF
    both = sampled.astype(np.int64) @ sampled.astype(np.int64).T
    agree = np.zeros_like(both)
    for c in np.unique(L[sampled]):
        m = (L == c).astype(np.int64)
        agree += m @ m.T
    return agree, both


def distance(agree, both):
    """d = 1.0 - (double)agree / (double)both, 1 where both == 0, 0 on the diagonal."""
    with np.errstate(invalid='ignore', divide='ignore'):
        d = 1.0 - agree.astype(np.float64) / both.astype(np.float64)
    d[both == 0] = 1.0
    np.fill_diagonal(d, 0.0)
    return d


def histogram(agree, both):
    iu = np.triu_indices(len(agree), 1)
    a, b = agree[iu], both[iu]
    t = np.where(b > 0, (BINS * a + b - 1) // np.maximum(b, 1), 0)
    return np.bincount(t, minlength=BINS + 1).astype(np.uint64)


def nn_chain_records(D):
    """The definition: scipy's nearest-neighbour chain for average linkage on a square matrix, every update one correctly rounded f64 expression; the raw
    records (x, y, height, size) in the order the merges happen."""
    D = np.array(D, dtype=np.float64)
    n = len(D)
    size = np.ones(n, dtype=np.int64)
    chain, rec = [], []
    for _ in range(n - 1):
        if not chain:
            chain = [int(np.flatnonzero(size > 0)[0])]
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y, cur = chain[-2], D[x, chain[-2]]
            else:
                y, cur = -1, np.inf
            row = np.where(size > 0, D[x], np.inf)
            row[x] = np.inf
            i = int(np.argmin(row))          # the first of the smallest: ascending i, strictly smaller wins
            if row[i] < cur:
                y, cur = i, row[i]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        chain = chain[:-2]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        rec.append((x, y, cur, nx + ny))
        size[x], size[y] = 0, nx + ny
        live = size > 0
        live[y] = False
        new = (float(nx) * D[live, x] + float(ny) * D[live, y]) / float(nx + ny)
        D[live, y] = new
        D[y, live] = new
    return np.array(rec, dtype=np.float64)


def yardstick_linkage(D):
    """Z of the definition: the records, stably sorted by height and relabelled as scipy relabels -- written out here independently of consensus._relabel."""
    rec = nn_chain_records(D)
    n = len(rec) + 1
    rec = rec[np.argsort(rec[:, 2], kind='stable')]
    name = {i: i for i in range(n)}          # point -> the name of its current cluster, through member lists
    members = {i: [i] for i in range(n)}
    Z = np.empty((n - 1, 4))
    for i, (x, y, h, _) in enumerate(rec):
        a, b = sorted((name[int(x)], name[int(y)]))
        both = members.pop(a) + members.pop(b)
        members[n + i] = both
        for p in both:
            name[p] = n + i
        Z[i] = (a, b, h, len(both))
    return Z


def partition_after(Z, k):
    """The partition after N - k merges as a list of frozensets, from member lists."""
    n = len(Z) + 1
    members = {i: [i] for i in range(n)}
    for i in range(n - k):
        members[n + i] = members.pop(int(Z[i, 0])) + members.pop(int(Z[i, 1]))
    return list(members.values())


@pytest.mark.parametrize('shape', SHAPES)
def test_yardstick_equals_scipy(shape):
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    from scipy.spatial.distance import squareform
    n, h, k = shape
    agree, both = pair_counts(synthetic_labels(n, h, k, seed=n + h))
    if shape == SHAPES[0]:
        assert (both[np.triu_indices(n, 1)] == 0).any()
    d = distance(agree, both)
    Z = yardstick_linkage(d)
    ref = hier.linkage(squareform(d, checks=False), 'average')
    assert np.array_equal(Z, ref)
    heights = Z[:, 2]
    assert (np.diff(heights) == 0).sum() >= 3          # tie-rich: the index rule decides merges
    # the package's host finish of the same records
    assert np.array_equal(consensus._relabel(nn_chain_records(d), n), ref)


@pytest.mark.parametrize('shape', SHAPES)
def test_cut_linkage_is_the_partition_after_n_minus_k_merges(shape):
    n, h, k = shape
    agree, both = pair_counts(synthetic_labels(n, h, k, seed=n + h))
    Z = yardstick_linkage(distance(agree, both))
    for kk in (1, 2, k, k + 3, n):
        labels = cut_linkage(Z, kk)
        assert labels.shape == (n,) and labels.dtype == np.int64
        parts = partition_after(Z, kk)
        assert len(parts) == kk and sorted(map(sorted, parts)) == sorted(sorted(np.flatnonzero(labels == c).tolist()) for c in range(1, kk + 1))
        # canonical numbering: 1-based, in order of first appearance by point index
        first = [int(np.flatnonzero(labels == c)[0]) for c in range(1, kk + 1)]
        assert labels[0] == 1 and first == sorted(first)
    with pytest.raises(ValueError):
        cut_linkage(Z, 0)
    with pytest.raises(ValueError):
        cut_linkage(Z, n + 1)


def test_cut_linkage_by_hand():
    # 5 points: (1, 3) merge, then (0, 4), then {1, 3} with 2, then all
    Z = np.array([[1, 3, 0.0, 2], [0, 4, 0.0, 2], [2, 5, 0.5, 3], [6, 7, 1.0, 5]], dtype=np.float64)
    assert cut_linkage(Z, 5).tolist() == [1, 2, 3, 4, 5]
    assert cut_linkage(Z, 4).tolist() == [1, 2, 3, 2, 4]
    assert cut_linkage(Z, 3).tolist() == [1, 2, 3, 2, 1]
    assert cut_linkage(Z, 2).tolist() == [1, 2, 2, 2, 1]
    assert cut_linkage(Z, 1).tolist() == [1, 1, 1, 1, 1]


def test_cdf_area_and_delta_area_by_hand():
    hist = np.zeros(BINS + 1, dtype=np.uint64)
    hist[0], hist[50], hist[BINS] = 2, 1, 1          # four pairs: consensus 0, 0, (0.49, 0.5], 1
    cdf, area = cdf_area(hist)
    assert cdf.shape == (BINS + 1,) and cdf.dtype == np.float64
    assert cdf[0] == 0.5 and (cdf[:50] == 0.5).all() and (cdf[50:BINS] == 0.75).all() and cdf[BINS] == 1.0
    assert area == (49 * 0.5 + 50 * 0.75 + 1.0) / BINS          # (dyadic values: the sum is exact)
    with pytest.raises(ValueError):
        cdf_area(np.zeros(BINS + 1, dtype=np.uint64))
    d = delta_area({2: 0.5, 3: 0.75, 4: 0.75, 6: 0.9375})
    assert d == {2: 0.5, 3: 0.5, 4: 0.0, 6: 0.25}
    # a perfectly clean consensus matrix (only 0 and 1) has a flat CDF between its ends
    hist = np.zeros(BINS + 1, dtype=np.uint64)
    hist[0], hist[BINS] = 30, 10
    cdf, area = cdf_area(hist)
    assert (cdf[:BINS] == 0.75).all() and area == (99 * 0.75 + 1.0) / BINS


@pytest.mark.parametrize('shape', SHAPES)
def test_histogram_counts_every_pair_once(shape):
    n, h, k = shape
    hist = histogram(*pair_counts(synthetic_labels(n, h, k, seed=n + h)))
    assert hist.dtype == np.uint64 and int(hist.sum()) == n * (n - 1) // 2
    cdf, area = cdf_area(hist)
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all() and 0 < area < 1


def test_consensus_summaries_by_hand():
    # 4 points, clusters {0, 1, 2} and {3}; rowsum[i, c] = sum of M(i, j) over j != i in c
    M = np.array([[0, 1, .5, .25], [1, 0, .5, 0], [.5, .5, 0, 0], [.25, 0, 0, 0]])
    y = np.array([0, 0, 0, 1])
    rowsum = np.stack([M[:, y == 0].sum(1), M[:, y == 1].sum(1)], axis=1)
    cluster, item = consensus.consensus_summaries(rowsum, y)
    assert cluster[0] == (1 + .5 + .5) / 3 and np.isnan(cluster[1])          # a singleton has no pair
    assert item[0, 0] == 0.75 and item[3, 0] == 0.25 / 3 and item[0, 1] == 0.25 and np.isnan(item[3, 1])


def test_python_argument_errors():
    with pytest.raises(ValueError, match='ks'):
        consensus.ConsensusKMeans([])
    with pytest.raises(ValueError, match='ks'):
        consensus.ConsensusKMeans([1, 2])
    with pytest.raises(ValueError, match='ks'):
        consensus.ConsensusKMeans([2, 2])
    with pytest.raises(ValueError, match='ks'):
        consensus.ConsensusKMeans([2, 300])
    with pytest.raises(ValueError, match='2-D'):
        consensus.ConsensusKMeans([2]).fit(np.zeros(10, np.float32))
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        consensus.ConsensusKMeans([2]).fit(np.zeros((10, 260), np.float32))
    with pytest.raises(ValueError, match='p_item'):
        consensus.draw_resamples(10, 5, 0.01, 0)
    with pytest.raises(ValueError, match='reps'):
        consensus.draw_resamples(10, 70000, 0.8, 0)
    a, b = consensus.draw_resamples(50, 3, 0.8, 7), consensus.draw_resamples(50, 3, 0.8, 7)
    assert len(a) == 3 and all(len(i) == 40 and len(set(i.tolist())) == 40 for i in a) and all((i == j).all() for i, j in zip(a, b))
    assert not (a[0] == a[1]).all()


class _P4Args:
    cluster_method, num_clusters, restore_metric, opt_eps, dl_cluster_label_type = 'consensus', 3, ['ae_mse'], 1.9, 'pred'


def test_p4_renumbering_by_hand():
    from deep_interpolation_clustering_amd.p4_clustering_final import Cluster
    # old 0 -> new 2, old 1 -> new 0, old 2 -> new 1
    raw = np.array([0, 1, 2, 2, 1, 0, 0])
    assert Cluster.renumber_consensus(raw, {0: 2, 1: 0, 2: 1}).tolist() == [2, 0, 1, 1, 0, 2, 2]
    assert raw.tolist() == [0, 1, 2, 2, 1, 0, 0]
    # a chain in which a naive in-place mapping would map twice: 0 -> 1 -> 2 -> 0
    assert Cluster.renumber_consensus(np.array([0, 1, 2]), {0: 1, 1: 2, 2: 0}).tolist() == [1, 2, 0]
    assert Cluster.renumber_consensus(np.array([2, 2, 0]), {0: 0, 1: 1, 2: 2}).tolist() == [2, 2, 0]


def _write_p4_inputs(root, labels_by_cohort, one_based):
    """A three-cluster feature dump whose sbp level (channel 0 of ob) is 100 + 10 * raw cluster, and the raw consensus csv files."""
    import pandas as pd
    from deep_interpolation_clustering_amd.info import COHORTS
    feat = os.path.join(root, 'Results', 'Clustering', 'out_feat')
    os.makedirs(os.path.join(feat, 'ae_mse'))
    os.makedirs(os.path.join(feat, 'raw_consensus_result'))
    rng = np.random.default_rng(3)
    for cohort in COHORTS:
        lab = labels_by_cohort[cohort]
        m = len(lab)
        ob = rng.normal(0, 0.1, (m, 2, 6)) + (100 + 10 * lab)[:, None, None]
        np.save(os.path.join(feat, 'ae_mse', cohort + '.npy'),
                {'encounter_id': np.arange(m), 'hidden': rng.normal(0, 1, (m, 4)).astype(np.float32), 'ob': ob, 'padding_mask': np.ones((m, 2, 6))})
        if cohort != 'testing':
            pd.DataFrame({'k2': np.ones(m, dtype=np.int64), 'k3': lab + (1 if one_based else 0)}).to_csv(
                os.path.join(feat, 'raw_consensus_result', cohort + '_consensus.csv'), index=False)
    return feat


@pytest.mark.parametrize('one_based', [True, False])
def test_p4_consensus_with_both_files_touches_no_gpu(tmp_path, monkeypatch, one_based):
    import torch
    from deep_interpolation_clustering_amd import kmeans, p4_clustering_final as p4

    def no_gpu(*a, **kw):
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(kmeans, '_device', no_gpu)
    monkeypatch.setattr(consensus, '_device', no_gpu)
    monkeypatch.setattr(torch.cuda, 'current_device', no_gpu)
    labels = {'training': np.array([0, 1, 2, 2, 1, 0, 1, 2]), 'validation': np.array([2, 2, 0, 1, 1]), 'testing': np.array([0, 1, 2])}
    feat = _write_p4_inputs(str(tmp_path), labels, one_based)
    monkeypatch.chdir(tmp_path)
    p4.main(_P4Args())
    # descending sbp: raw 2 (sbp 120) -> 0, raw 1 -> 1, raw 0 (sbp 100) -> 2: the cluster that maps to new id 0 is there
    out = os.path.join(feat, 'ae_mse_consensus_aligned')
    for cohort in ('training', 'validation'):
        d = np.load(os.path.join(out, cohort + '_3.npy'), allow_pickle=True).item()
        assert sorted(d) == ['cluster_id', 'encounter_id', 'hidden']
        assert d['cluster_id'].tolist() == (2 - labels[cohort]).tolist()
    assert not os.path.exists(os.path.join(out, 'testing_3.npy'))          # upstream leaves the test cohort out
    # an existing result is left alone
    stamp = os.stat(os.path.join(out, 'training_3.npy')).st_mtime_ns
    p4.main(_P4Args())
    assert os.stat(os.path.join(out, 'training_3.npy')).st_mtime_ns == stamp


def test_p4_optics_keeps_raising(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    labels = {'training': np.array([0, 1, 2]), 'validation': np.array([2, 0, 1]), 'testing': np.array([0, 1, 2])}
    _write_p4_inputs(str(tmp_path), labels, True)
    monkeypatch.chdir(tmp_path)
    args = _P4Args()
    args.cluster_method = 'optics'
    with pytest.raises(NotImplementedError, match='optics'):
        p4.main(args)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_consensus_pairs_workspace(1000, 100, 4)
    assert ws > 0 and lib.dic_consensus_pairs_workspace(1000, 100, 0) > 0
    assert lib.dic_consensus_pairs_workspace(1, 100, 4) == 0 and lib.dic_consensus_pairs_workspace(1000, 0, 4) == 0
    assert lib.dic_consensus_pairs_workspace(1000, 65536, 4) == 0 and lib.dic_consensus_pairs_workspace(1000, 100, 255) == 0
    assert lib.dic_consensus_pairs_workspace(1000, 100, -1) == 0

    def pairs(L=fake, ldl=112, n=1000, h=100, y=fake, k=4, hist=fake, rowsum=fake, D=fake, work=fake, nbytes=ws):
        return lib.dic_consensus_pairs(L, ldl, n, h, y, k, hist, rowsum, D, work, nbytes, None)

    assert pairs(L=None) == -1 and b'NULL' in lib.dic_last_error_string()
    assert pairs(hist=None, rowsum=None, D=None) == -1 and b'NULL' in lib.dic_last_error_string()
    assert pairs(y=None) == -1 and b'NULL' in lib.dic_last_error_string()
    assert pairs(work=None) == -1 and b'NULL' in lib.dic_last_error_string()
    assert pairs(n=1) == -1 and pairs(n=0) == -1 and pairs(h=0) == -1 and pairs(ldl=96) == -1
    assert pairs(ldl=104) == -1 and b'multiple of 16' in lib.dic_last_error_string()
    assert pairs(k=0) == -1 and pairs(k=255) == -1 and b'K=255' in lib.dic_last_error_string()
    assert pairs(ldl=65536, h=65536) == -2 and b'65535' in lib.dic_last_error_string()
    assert pairs(n=1 << 30) == -2
    assert pairs(L=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert pairs(D=ctypes.c_void_p((1 << 20) + 4)) == -2
    assert pairs(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()

    lws = lib.dic_linkage_average_workspace(1000)
    assert lws > 0 and lib.dic_linkage_average_workspace(1) == 0 and lib.dic_linkage_average_workspace(1 << 30) == 0
    assert lws <= 8 * 1000 + 1024          # O(N): sizes, chain, counters

    def link(D=fake, n=1000, rec=fake, work=fake, nbytes=lws):
        return lib.dic_linkage_average(D, n, rec, work, nbytes, None)

    for kw in ({'D': None}, {'rec': None}, {'work': None}):
        assert link(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
    assert link(n=1) == -1 and link(n=0) == -1 and link(n=-5) == -1
    assert link(n=1 << 30) == -2
    assert link(D=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert link(nbytes=lws - 1) == -3 and b'workspace' in lib.dic_last_error_string()


def test_header_and_signatures_agree():
    names = {'dic_consensus_pairs_workspace', 'dic_consensus_pairs', 'dic_linkage_average_workspace', 'dic_linkage_average'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    assert set(N.header_symbols()) == set(N.SIGNATURES)
    with open(N.HEADER_PATH) as f:
        assert '#define DIC_CONSENSUS_BINS %d' % BINS in f.read()


def test_package_does_not_import_scipy_or_sklearn():
    import re
    with open(consensus.__file__) as f:
        assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M)
