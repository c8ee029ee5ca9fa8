"""Exact neighbour lists on the GPU (knn.py: kneighbors, NearestNeighbors, knn_transfer_labels; csrc/dic_knn.hip: dic_knn_neighbors) against the numpy yardstick
of tests/test_knn_lists_host.py, which shares no code with them, and p4's --transfer knn.

Kernel and yardstick each sum D exact f64 squares, so both lie within (D + 2) 2^-53 relative of the true d^2 of the f32 points -- 2.9e-14 relative on d at
D = 256; the bar is 1e-13 relative on d, as in tests/test_gpu_knn.py, a yardstick distance of 0 asks for 0, and the indices must be equal (the host file
asserts that no row of a random case has two of its first k + 1 distances close enough for the two summation orders to disagree).  The lattice cases hold
small integers, exact in any order: they compare bit for bit."""
import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn as K
from deep_interpolation_clustering_amd.dbscan import DBSCAN
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.knn import CandidateBudgetError, NearestNeighbors, kneighbors, knn_transfer_labels, kth_neighbor_distance

import test_gpu_dbscan as TD
import test_knn_lists_host as H

pytestmark = pytest.mark.gpu

REL = 1e-13


def check(name, exact=False, **kw):
    X, Q, k = H.case(name)
    ref_d, ref_i, _ = H.yard(name)
    dist, idx = kneighbors(X, k, Q=Q, **kw)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and dist.shape == idx.shape == ref_d.shape
    zero = ref_d == 0
    err = np.abs(dist[~zero] - ref_d[~zero]) / ref_d[~zero]
    print('%s: max rel err %.3g, zeros %d, index mismatches %d' % (name, err.max() if err.size else 0.0, int(zero.sum()), int((idx != ref_i).sum())))
    assert np.all(dist[zero] == 0.0)
    if exact:
        np.testing.assert_array_equal(dist, ref_d)
    else:
        assert np.all(err <= REL), err.max()
    np.testing.assert_array_equal(idx, ref_i)
    assert idx.min() >= 0 and idx.max() < len(X)          # queries never appear as neighbours
    return dist, idx


@pytest.mark.parametrize('name', sorted(H.SELF))
def test_self_join(name):
    X, _, k = H.case(name)
    dist, idx = check(name)
    assert np.array_equal(idx[:, 0], np.arange(len(X))) and np.all(dist[:, 0] == 0)          # the self pair is an ordinary pair with d^2 = 0


@pytest.mark.parametrize('name', ['n1000_d32_k7', 'n600_d256_k257'])
def test_last_column_is_the_kth_distance_bit_for_bit(name):
    X, _, k = H.case(name)
    np.testing.assert_array_equal(kneighbors(X, k)[0][:, -1], kth_neighbor_distance(X, k))


@pytest.mark.parametrize('name', sorted(H.CROSS))
def test_cross_set(name):
    X, Q, k = H.case(name)
    dist, idx = check(name)
    assert dist[0, 0] == 0.0 and idx[0, 0] == min(3, len(X) - 1)          # the query that equals an index point finds it first, at exactly 0


@pytest.mark.parametrize('name', ['lattice_self', 'lattice_cross'])
def test_lattice_ties_compare_exactly(name):
    check(name, exact=True)


@pytest.mark.parametrize('name', ['dup_k10', 'dup_k60'])
def test_duplicated_points(name):
    dist, idx = check(name)
    assert (dist[100:140, :10] == 0).all()


@pytest.mark.parametrize('name', ['far_self', 'far_cross'])
def test_points_far_from_their_mean(name):
    check(name)


def test_budget_groups_and_repeat_calls():
    name = 'n1000_d32_k7'
    X, _, k = H.case(name)
    st = {}
    a = kneighbors(X, k, stats=st)
    assert st['groups'] == 1 and st['passes'] == 4 and st['max_list'] >= k and st['candidates'] >= k * len(X)
    budget = 12 * (st['candidates'] // 3)          # at least 3 groups
    assert budget >= st['budget_needed']
    st2 = {}
    b = check(name, candidate_budget=budget, stats=st2)
    assert st2['groups'] >= 3 and st2['candidates'] == st['candidates']
    c = kneighbors(X, k)
    d = kneighbors(torch.as_tensor(X, device='cuda'), k, return_device=True)
    assert d[0].is_cuda and d[1].is_cuda and d[1].dtype == torch.int32
    for u, v, w, t in zip(a, b, c, d):
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u, w)
        np.testing.assert_array_equal(u, t.cpu().numpy())
    # the cross join too
    X, Q, k = H.case('n70_m600')
    st = {}
    a = kneighbors(X, k, Q=Q, stats=st)
    st2 = {}
    b = check('n70_m600', candidate_budget=12 * (st['candidates'] // 3), stats=st2)
    assert st2['groups'] >= 3
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_budget_below_one_list():
    X, _, k = H.case('dup_k10')          # the duplicates' lists hold all 41 copies
    st = {}
    with pytest.raises(CandidateBudgetError) as e:
        kneighbors(X, k, candidate_budget=12 * 20, stats=st)
    assert e.value.needed == st['budget_needed'] >= 12 * 41 and st['max_list'] >= 41
    dist, idx = check('dup_k10', candidate_budget=e.value.needed)


def test_memory_stays_within_the_workspace_and_the_outputs():
    n, m, d, k = 20000, 6000, 64, 65
    x = torch.randn(n, d, device='cuda')
    q = torch.randn(m, d, device='cuda')
    centre = x.mean(0, keepdim=True).contiguous()
    L = N.lib()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    budget = 64 << 20
    nws = L.dic_knn_neighbors_workspace(n, m, d, budget)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    dist = torch.empty((m, k), dtype=torch.float64, device='cuda')
    idx = torch.empty((m, k), dtype=torch.int32, device='cuda')
    N.check(L.dic_knn_neighbors(N.ptr(x), d, n, N.ptr(q), d, m, N.ptr(centre), d, k, N.ptr(dist), N.ptr(idx), budget, None, N.ptr(ws), nws, N.stream_of(x)),
            'dic_knn_neighbors')
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    io = m * k * 12
    print('20 000 + 6 000 x 64: peak growth %.2f MB, workspace %.2f MB, outputs %.2f MB' % (grown / 2 ** 20, nws / 2 ** 20, io / 2 ** 20))
    assert grown <= nws + io + (1 << 20)
    assert nws + io < m * n * 8 // 4          # nothing M x N: the f64 matrix would be 960 MB
    i = idx.cpu().numpy()
    dd = dist.cpu().numpy()
    assert i.min() >= 0 and i.max() < n and (np.diff(dd, axis=1) >= 0).all() and np.isfinite(dd).all()
    ref = torch.cdist(q[:64].double(), x.double()).topk(k, dim=1, largest=False)          # a spot check of 64 rows
    assert np.allclose(dd[:64], ref.values.cpu().numpy(), rtol=1e-9, atol=0)


def _without_self(name):
    """The yardstick of kneighbors(None): k + 1 neighbours, the row's own index dropped, the first column where it is not among them (sklearn 1.7.2)."""
    X, _, k = H.case(name)
    d, i = H.kneighbors_exact(X, None, k + 1)
    keep = i != np.arange(len(X))[:, None]
    keep[keep.all(1), 0] = False
    return d[keep].reshape(len(X), k), i[keep].reshape(len(X), k)


@pytest.mark.parametrize('name', ['n257_d16_k4', 'dup_k10'])
def test_nearest_neighbors_without_self(name):
    X, _, k = H.case(name)
    ref_d, ref_i = _without_self(name)
    nn = NearestNeighbors(n_neighbors=k).fit(X)
    dist, idx = nn.kneighbors()
    np.testing.assert_array_equal(idx, ref_i)
    assert np.all(dist[ref_d == 0] == 0) and np.allclose(dist, ref_d, rtol=REL, atol=0)
    if name == 'dup_k10':          # the later copies do not find themselves among 11 zeros: their first column went
        assert (idx[130:140] != np.arange(130, 140)[:, None]).all() and (ref_i[130:140, 0] == 100).all()
    np.testing.assert_array_equal(nn.kneighbors(return_distance=False), ref_i)
    d3, i3 = nn.kneighbors(X[:9], n_neighbors=3)          # given queries keep themselves
    r3 = H.kneighbors_exact(X, X[:9], 3)
    np.testing.assert_array_equal(i3, r3[1])
    assert np.allclose(d3, r3[0], rtol=REL, atol=0)


def test_kneighbors_graph_is_the_yardsticks_csr():
    name = 'n257_d16_k4'
    X, _, k = H.case(name)
    ref_d, ref_i = _without_self(name)
    nn = NearestNeighbors(n_neighbors=k).fit(X)
    data, indices, indptr = nn.kneighbors_graph()
    np.testing.assert_array_equal(indptr, np.arange(0, len(X) * k + 1, k))
    np.testing.assert_array_equal(indices, ref_i.ravel())
    assert data.dtype == np.float64 and np.all(data == 1.0) and len(data) == len(X) * k
    data, indices, indptr = nn.kneighbors_graph(mode='distance')
    np.testing.assert_array_equal(indices, ref_i.ravel())
    assert np.allclose(data, ref_d.ravel(), rtol=REL, atol=0)
    Q = H.case('n300_m70')[1]
    data, indices, indptr = nn.kneighbors_graph(Q, n_neighbors=2, mode='distance')          # given queries: an (M, n_samples_fit) matrix
    r = H.kneighbors_exact(X, Q, 2)
    np.testing.assert_array_equal(indptr, np.arange(0, len(Q) * 2 + 1, 2))
    np.testing.assert_array_equal(indices, r[1].ravel())
    assert np.allclose(data, r[0].ravel(), rtol=REL, atol=0)


def test_transfer_labels_equal_the_host_vote():
    X, _, Q = H._labelled()
    y = DBSCAN(1.4, 9).fit(X).labels_          # real DBSCAN labels: three clusters, and a quarter of the points noise
    seen = set()
    assert (y == -1).sum() > 10 and len(set(y.tolist()) - {-1}) >= 2
    for k in (1, 5, 9):
        _, idx = H.kneighbors_exact(X, Q, k)
        ref, share = H.vote_exact(idx, y)
        lab, got = knn_transfer_labels(X, y, Q, k)
        assert lab.dtype == np.int32 and got.dtype == np.float32 and lab.shape == got.shape == (len(Q),)
        np.testing.assert_array_equal(lab, ref)
        np.testing.assert_array_equal(got, share)
        seen |= set(lab.tolist())
    assert seen == {-1, 0, 1, 2}          # noise is a class like any other: some query takes it
    X, y, Q, k = H._forced_tie()
    lab, share = knn_transfer_labels(X, y, Q, k)
    assert lab.tolist() == [-1] and share.tolist() == [0.5]          # two votes each for -1 and 2: the smaller label
    lab, share = knn_transfer_labels(torch.as_tensor(X, device='cuda'), y, torch.as_tensor(Q), 2)
    assert lab.tolist() == [2] and share.tolist() == [1.0]


@pytest.mark.parametrize('method', ['dbscan', 'hdbscan'])
def test_p4_knn_transfer(method, tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = TD._write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 37 if method == 'dbscan' else 35)
    monkeypatch.chdir(tmp_path)
    extra, stem = (['--opt_eps', '1.5'], '%s_eps-1.5') if method == 'dbscan' else ([], '%s_mcs-17')
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / ('ae_mse_%s_aligned' % method)

    def run(more):
        args = p4.get_arguments(['--cluster_method', method] + extra + more)
        args.restore_metric = ['ae_mse']
        p4.main(args)

    run(['--transfer', 'knn'])
    saved = {c: np.load(out / ((stem + '_knn.npy') % c), allow_pickle=True).item() for c in COHORTS}
    train = saved['training']
    assert sorted(train) == ['cluster_id', 'cluster_vote', 'encounter_id', 'hidden'] and (train['cluster_vote'] == 1).all()
    assert sorted(set(train['cluster_id'].tolist()) - {-1}) == [0, 1, 2] and (train['cluster_id'] == -1).any()
    k = train['hidden'].shape[1] + 1          # --transfer_k defaults to feat_dim + 1
    for cohort in COHORTS[1:]:
        s = saved[cohort]
        assert sorted(s) == ['cluster_id', 'cluster_vote', 'encounter_id', 'hidden'] and len(s['cluster_id']) == len(data[cohort]['hidden'])
        _, idx = H.kneighbors_exact(train['hidden'], s['hidden'], k)
        ref, share = H.vote_exact(idx, train['cluster_id'])
        np.testing.assert_array_equal(s['cluster_id'], ref)
        np.testing.assert_array_equal(s['cluster_vote'], share)
        assert s['cluster_id'].dtype == train['cluster_id'].dtype and s['cluster_vote'].dtype == np.float32
        assert (s['cluster_vote'] > 0).all() and (s['cluster_vote'] <= 1).all()
        assert set(s['cluster_id'].tolist()) >= {0, 1, 2}
    # the default is --transfer centre, and it writes what a run without the flag writes
    run([])
    plain = {c: (out / ((stem + '.npy') % c)).read_bytes() for c in COHORTS}
    for c in COHORTS:
        (out / ((stem + '.npy') % c)).unlink()
    run(['--transfer', 'centre'])
    assert all((out / ((stem + '.npy') % c)).read_bytes() == plain[c] for c in COHORTS)
    # another k goes through, and leaves the training cohort's labels as they are
    stamp = (out / ((stem + '_knn.npy') % 'training')).stat().st_mtime_ns
    for c in COHORTS[1:]:
        (out / ((stem + '_knn.npy') % c)).unlink()
    run(['--transfer', 'knn', '--transfer_k', '3'])
    assert (out / ((stem + '_knn.npy') % 'training')).stat().st_mtime_ns == stamp
    s = np.load(out / ((stem + '_knn.npy') % 'validation'), allow_pickle=True).item()
    _, idx = H.kneighbors_exact(train['hidden'], s['hidden'], 3)
    np.testing.assert_array_equal(s['cluster_id'], H.vote_exact(idx, train['cluster_id'])[0])
