"""HDBSCAN on the GPU (hdbscan.py, csrc/dic_hdbscan.hip) against a yardstick that shares no code with it, and the p2 / p4 --cluster_method hdbscan branches.

The yardstick: ``dmat`` (test_gpu_optics.py) -- the numpy f64 difference-form distance matrix of the f32 points -- and ``oracle_mst``, the loop of the
definition on it: Prim from point 0 over mr(p, q) = max(core[p], core[q], d(p, q)), strict updates, ties to the smallest index (sklearn's
``mst_from_mutual_reachability``, which ``test_convention_is_sklearns`` holds it to bit for bit).  Kernel and yardstick each sum D exact f64 squares, so both
lie within (D + 2) 2^-53 relative of the true d^2: core distances and finite weights compare at 1e-13 relative (the bar of test_gpu_knn.py), nothing is
rounded.  Ordering and predecessor compare EXACTLY; what keeps that honest is computed from the yardstick itself: wherever the loop chooses between two
distinct values -- the arg-min against the next distinct reachability outside the tree, a candidate mr against a differing finite reach[q] -- and wherever
the stable sort of the weights orders two distinct weights, they are at least 1e-10 apart relatively, three orders above the arithmetic's error, so both
sides must decide alike; equal values are equal bits on both sides (one distance function, symmetric) and go to the smaller index.  The total weight of the
tree is also held to scipy's minimum spanning tree of the yardstick's matrix, which no tie rule enters.  Labels compare with the host extraction of
hdbscan.py (held to sklearn's in test_hdbscan_host.py) applied to the yardstick's tree, and with sklearn's own fit wherever sklearn's result does not depend
on its unstable sort."""
import functools
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.hdbscan import HDBSCAN, hdbscan_mst, hdbscan_sizes, labelling_at_cut, single_linkage_tree, tree_to_labels
from test_gpu_optics import LINE_N, _write_latents, dmat, line, matrix, points

pytestmark = pytest.mark.gpu

REL = 1e-13
PROB = 1e-12          # ten times the weight bar: probabilities are quotients of reciprocals of weights
MARGIN = 1e-10


def oracle_mst(D, min_samples):
    """The definition as a loop over the matrix: ``(ordering, core, reach, pred, (arg-min margin, update margin, sort margin))``.  The first two margins are
    the smallest relative gaps the loop met between two DISTINCT values it had to order, the third the smallest relative gap between two distinct weights
    of the tree (inf where there was none)."""
    n = len(D)
    core = np.partition(D, min_samples - 1, axis=1)[:, min_samples - 1].copy()
    reach, pred = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    in_tree, ordering = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    pick_margin = update_margin = np.inf
    cur = 0
    for step in range(n - 1):
        in_tree[cur] = True
        mr = np.maximum(np.maximum(D[cur], core), core[cur])
        live = ~in_tree
        differ = live & np.isfinite(reach) & (reach != mr) & (np.minimum(reach, mr) > 0)
        if differ.any():
            update_margin = min(update_margin, float((np.abs(reach - mr)[differ] / np.minimum(reach, mr)[differ]).min()))
        better = live & (mr < reach)
        reach[better] = mr[better]
        pred[better] = cur
        vals = np.where(live, reach, np.inf)
        cur = int(np.argmin(vals))          # the first minimum: the smallest index
        lowest = vals[cur]
        above = vals[(vals > lowest) & np.isfinite(vals)]
        if above.size and lowest > 0:
            pick_margin = min(pick_margin, float((above.min() - lowest) / lowest))
        ordering[step + 1] = cur
    w = np.unique(reach[ordering[1:]])
    gaps = (np.diff(w) / np.where(w[:-1] > 0, w[:-1], np.inf))
    sort_margin = float(gaps[gaps > 0].min()) if (gaps > 0).any() else np.inf
    return ordering, core, reach, pred, (pick_margin, update_margin, sort_margin)


MIN_SAMPLES = {'A': 17, 'B': 5, 'C20': 20, 'C257': 257, 'D': 3, 'E': 9, 'F': 7}
CASES = sorted(MIN_SAMPLES)
HAVE_CLUSTERS = ('A', 'B', 'C20', 'D', 'E')


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, min_samples, oracle tuple) -- computed once, shared by every test, never written to."""
    X, k = points(name), MIN_SAMPLES[name]
    out = oracle_mst(matrix(name), k)
    for a in out[:4]:
        a.setflags(write=False)
    return X, k, out


def close(got, ref):
    """inf in the same places; finite values within 1e-13 relative."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.all(got[~fin] == ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= REL * ref[fin]), (err / np.maximum(ref[fin], 1e-300)).max()
    return float((err / np.maximum(ref[fin], 1e-300)).max()) if fin.any() else 0.0


def margins_hold(m):
    return all(v >= MARGIN for v in m)


@pytest.mark.parametrize('name', CASES)
def test_margins_of_the_cases(name):
    """The condition under which exact equality of ordering and predecessor is the right demand (module docstring)."""
    _, _, (o_ord, _, o_reach, _, (pick, update, sort)) = case(name)
    w = o_reach[o_ord[1:]]
    print('case %s: arg-min margin %.3g, update margin %.3g, sort margin %.3g, %d equal weights' % (name, pick, update, sort, len(w) - len(np.unique(w))))
    assert pick >= MARGIN and update >= MARGIN and sort >= MARGIN


@pytest.mark.parametrize('name', CASES)
def test_tree_equals_the_oracle(name):
    X, k, (o_ord, o_core, o_reach, o_pred, m) = case(name)
    assert margins_hold(m)          # a case that fails this is a wrong choice of input, not a reason to compare loosely
    stats = {}
    ordering, core, reach, pred = hdbscan_mst(X, k, stats=stats)
    assert ordering.dtype == np.int64 and pred.dtype == np.int64 and core.dtype == np.float64 and reach.dtype == np.float64
    assert stats['steps'] == len(X) - 1
    np.testing.assert_array_equal(np.sort(ordering), np.arange(len(X)))
    e_core, e_reach = close(core, o_core), close(reach, o_reach)
    print('case %s: N=%d D=%d min_samples=%d: max rel err core %.3g reach %.3g' % (name, len(X), X.shape[1], k, e_core, e_reach))
    assert np.isinf(reach[0]) and np.isfinite(reach[1:]).all()
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(pred, o_pred)
    np.testing.assert_array_equal(core, knn.kth_neighbor_distance(X, k))          # unrounded


@pytest.mark.parametrize('name', CASES)
def test_tree_is_a_minimum_spanning_tree(name):
    """Independent of every tie rule: pred / reach form a spanning tree of the mutual-reachability graph whose total weight is the minimum one's."""
    csgraph = pytest.importorskip('scipy.sparse.csgraph')
    sparse = pytest.importorskip('scipy.sparse')
    X, k, (_, o_core, o_reach, _, _) = case(name)
    ordering, core, reach, pred = hdbscan_mst(X, k)
    n = len(X)
    position = np.empty(n, dtype=np.int64)
    position[ordering] = np.arange(n)
    rest = np.arange(1, n)
    assert pred[0] == -1 and pred[rest].min() >= 0
    assert (position[pred[rest]] < position[rest]).all()          # every point hangs on an earlier one: n - 1 edges, no cycle, one component
    D = matrix(name)
    edge = np.maximum(np.maximum(D[rest, pred[rest]], o_core[rest]), o_core[pred[rest]])
    assert np.all(np.abs(reach[rest] - edge) <= REL * edge)          # the weights are the graph's
    # scipy sorts every edge it is given (8 s for the 18 million of case E), so it gets the edges no heavier than the heaviest weight of the YARDSTICK's walk only.
    # That loses nothing whatever that bound is worth: scipy's tree below spans all n points, so the graph of the edges <= bound is connected, so the full
    # graph's minimum spanning trees have no edge above the bound (a heavier edge could be exchanged for a path of lighter ones) and lie inside it.
    M = np.maximum(np.maximum(D, o_core[:, None]), o_core[None, :])
    i, j = np.nonzero(np.triu(M <= o_reach[1:].max(), 1))
    assert (M[i, j] > 0).all()          # (scipy reads a zero as no edge)
    tree = csgraph.minimum_spanning_tree(sparse.csr_matrix((M[i, j], (i, j)), shape=(n, n)))
    assert tree.nnz == n - 1
    best = float(tree.sum())
    total = float(reach[rest].sum())
    print('case %s: tree weight %.17g, scipy %.17g, relative difference %.3g' % (name, total, best, abs(total - best) / best))
    assert abs(total - best) <= 1e-12 * best


@pytest.mark.parametrize('name', CASES)
def test_labels_equal_the_extraction_on_the_oracle_tree(name):
    X, k, (o_ord, _, o_reach, _, m) = case(name)
    assert margins_hold(m)
    slt = single_linkage_tree(o_ord, o_reach)
    for mcs in (k, 3 * k):
        for method in ('eom', 'leaf'):
            fit = HDBSCAN(min_cluster_size=mcs, min_samples=k, cluster_selection_method=method).fit(X)
            ref_labels, ref_prob = tree_to_labels(slt, mcs, method)
            np.testing.assert_array_equal(fit.labels_, ref_labels)
            assert np.abs(fit.probabilities_ - ref_prob).max() <= PROB
            np.testing.assert_array_equal(fit.ordering_, o_ord)
            assert len(fit.single_linkage_tree_) == len(X) - 1 and fit.condensed_tree_['child'].max() >= len(X) - 1
            if mcs == k and method == 'eom':
                n_clusters, n_noise = int(ref_labels.max()) + 1, int((ref_labels == -1).sum())
                print('case %s: %d clusters, %d noise points' % (name, n_clusters, n_noise))
                assert (n_clusters >= 2 and n_noise > 0) or name not in HAVE_CLUSTERS          # (those inputs have clusters to find)
                cut = float(np.median(o_reach[1:]))
                np.testing.assert_array_equal(fit.dbscan_clustering(cut, k), labelling_at_cut(slt, cut, k))
    # one tree, several sizes
    fit, found = hdbscan_sizes(X, k, [k, 3 * k], cluster_selection_method='leaf')
    for mcs in (k, 3 * k):
        np.testing.assert_array_equal(found[mcs][0], tree_to_labels(slt, mcs, 'leaf')[0])


@pytest.mark.parametrize('name', CASES)
def test_labels_equal_sklearns_where_its_sort_does_not_matter(name):
    """sklearn sorts the tree's edges with an unstable sort; where its own functions give the same labels under both sort kinds, its fit on the distance
    matrix is the reference.  A case where they differ skips this one comparison and no other."""
    sk = pytest.importorskip('sklearn.cluster')
    from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
    from sklearn.cluster._hdbscan._tree import tree_to_labels as sk_tree_to_labels
    X, k, (o_ord, _, o_reach, _, m) = case(name)
    assert margins_hold(m)
    mst = np.zeros(len(X) - 1, dtype=MST_edge_dtype)
    mst['current_node'], mst['next_node'], mst['distance'] = o_ord[:-1], o_ord[1:], o_reach[o_ord[1:]]
    by_kind = {kind: sk_tree_to_labels(make_single_linkage(mst[np.argsort(mst['distance'], kind=kind)]), k)[0] for kind in ('quicksort', 'stable')}
    ours = HDBSCAN(min_cluster_size=k, min_samples=k).fit(X)
    np.testing.assert_array_equal(ours.labels_, by_kind['stable'])          # (this one holds whatever the sort kinds do)
    if not np.array_equal(by_kind['quicksort'], by_kind['stable']):
        pytest.skip('case %s: sklearn labels depend on the tie order of its unstable sort' % name)
    ref = sk.HDBSCAN(min_cluster_size=k, min_samples=k, metric='precomputed', algorithm='brute').fit(matrix(name).copy())          # (sklearn writes into it)
    np.testing.assert_array_equal(ours.labels_, ref.labels_)
    assert np.abs(ours.probabilities_ - ref.probabilities_).max() <= PROB


@pytest.mark.parametrize('name', ['B', 'D'])
def test_convention_is_sklearns(name):
    linkage = pytest.importorskip('sklearn.cluster._hdbscan._linkage')
    _, k, (o_ord, o_core, o_reach, _, _) = case(name)
    D = matrix(name)
    mst = linkage.mst_from_mutual_reachability(np.maximum(np.maximum(D, o_core[:, None]), o_core[None, :]))
    np.testing.assert_array_equal(mst['current_node'], o_ord[:-1])
    np.testing.assert_array_equal(mst['next_node'], o_ord[1:])
    np.testing.assert_array_equal(mst['distance'], o_reach[o_ord[1:]])


def exact(X, k):
    """Inputs whose distances are exact (or exactly equal) in both arithmetics: everything compares bit for bit."""
    o_ord, o_core, o_reach, o_pred, _ = oracle_mst(dmat(X), k)
    ordering, core, reach, pred = hdbscan_mst(X, k)
    np.testing.assert_array_equal(core, o_core)
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(reach, o_reach)
    np.testing.assert_array_equal(pred, o_pred)
    return ordering, core, reach, pred


@pytest.mark.parametrize('k', [7, 27])
def test_lattice_ties_compare_exactly(k):
    # integer lattice: every d^2 is a small integer and its root correctly rounded on both sides; whole shells of points tie at every step
    g = np.arange(7, dtype=np.float32)
    X = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    X = np.concatenate([X, np.zeros((len(X), 1), np.float32)], 1)
    _, core, reach, _ = exact(X, k)
    assert len(np.unique(reach)) <= 8 and len(np.unique(core)) <= 8          # 343 points, a handful of values: ties everywhere


@pytest.mark.parametrize('k', [2, 3])
def test_duplicated_points_compare_exactly(k):
    # every point twice, coordinates on a grid of eighths: every difference, square and sum is exact in f64 whatever the order of summation, and the root is
    # correctly rounded on both sides.  Zero weights (core 0 at k = 2: a point's copy joins at 0), and the two copies of a point tie in every comparison
    rng = np.random.default_rng(5)
    base = (rng.integers(-32, 33, (500, 12)) / 8.0).astype(np.float32)
    assert len(np.unique(base, axis=0)) == 500
    X = np.concatenate([base, base])[rng.permutation(1000)]
    _, core, reach, _ = exact(X, k)
    if k == 2:
        assert np.all(core == 0.0) and (reach == 0.0).sum() == 500
        fit = HDBSCAN(min_cluster_size=2, min_samples=2).fit(X)          # lambda = inf at the zero weights: the extraction runs through
        assert fit.labels_.shape == (1000,) and np.isfinite(fit.probabilities_).all()


def test_second_trip_of_the_row_loop_on_a_line():
    # as in test_gpu_optics.py: more rows than one trip of the step's row loop takes, on the input whose walk is known in closed form
    X, o_ord, o_reach, o_pred = line(300)
    ordering, core, reach, pred, _ = oracle_mst(dmat(X), 2)
    assert np.all(core == 1.0)
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(reach, o_reach)
    np.testing.assert_array_equal(pred, o_pred)
    X, o_ord, o_reach, o_pred = line(LINE_N)
    ordering, core, reach, pred = hdbscan_mst(X, 2)
    assert np.all(core == 1.0)
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(reach, o_reach)
    np.testing.assert_array_equal(pred, o_pred)


def _abi_call(x, core):
    L = N.lib()
    n, d = x.shape
    ordering = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    pred = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    reach = torch.zeros(n, dtype=torch.float64, device='cuda')
    ws = torch.empty(L.dic_hdbscan_workspace(n, d), dtype=torch.uint8, device='cuda')
    rc = L.dic_hdbscan_mst(N.ptr(x), d, n, d, N.ptr(core), N.ptr(ordering), N.ptr(reach), N.ptr(pred), N.ptr(ws), ws.numel(), N.stream_of(x))
    assert rc == 0
    torch.cuda.synchronize()
    return ordering.cpu().numpy(), reach.cpu().numpy(), pred.cpu().numpy()


def test_one_and_two_points_through_the_abi():
    # N = 1 at the C entry point (no step is launched): the point is the walk
    ordering, reach, pred = _abi_call(torch.zeros(1, 4, device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda'))
    assert ordering.tolist() == [0] and pred.tolist() == [-1] and np.isinf(reach[0])
    # N = 2: one step; the weight is max(core[0], core[1], d)
    x = torch.tensor([[0., 0., 0., 0.], [3., 4., 0., 0.]], device='cuda')
    for cores, weight in (([0.0, 0.0], 5.0), ([5.0, 5.0], 5.0), ([6.0, 1.0], 6.0), ([1.0, 7.5], 7.5)):
        ordering, reach, pred = _abi_call(x, torch.tensor(cores, dtype=torch.float64, device='cuda'))
        assert ordering.tolist() == [0, 1] and pred.tolist() == [-1, 0] and np.isinf(reach[0]) and reach[1] == weight
    ordering, core, reach, pred = exact(np.array([[0, 0, 0, 0], [3, 4, 0, 0]], np.float32), 2)
    assert list(ordering) == [0, 1] and list(pred) == [-1, 0] and reach[1] == core[0] == core[1] == 5.0
    assert hdbscan_mst(np.zeros((1, 4), np.float32), 1)[0].tolist() == [0]


def test_two_calls_and_a_device_tensor_give_identical_bits():
    X, k, _ = case('A')
    a = hdbscan_mst(X, k)
    b = hdbscan_mst(X, k)
    c = hdbscan_mst(torch.as_tensor(X, device='cuda'), k)
    for u, v, t in zip(a, b, c):
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u, t)
    X, k, _ = case('F')          # padded to a multiple of 4 on the way in
    for u, v in zip(hdbscan_mst(X, k), hdbscan_mst(torch.as_tensor(X, device='cuda'), k)):
        np.testing.assert_array_equal(u, v)


def test_memory_stays_within_the_workspace():
    n, d, k = 20000, 64, 65
    x = torch.randn(n, d, device='cuda')
    core = torch.as_tensor(knn.kth_neighbor_distance(x, k), device='cuda')
    L = N.lib()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    nws = L.dic_hdbscan_workspace(n, d)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    ordering = torch.empty(n, dtype=torch.int32, device='cuda')
    pred = torch.empty(n, dtype=torch.int32, device='cuda')
    reach = torch.empty(n, dtype=torch.float64, device='cuda')
    N.check(L.dic_hdbscan_mst(N.ptr(x), d, n, d, N.ptr(core), N.ptr(ordering), N.ptr(reach), N.ptr(pred), N.ptr(ws), nws, N.stream_of(x)), 'dic_hdbscan_mst')
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    io = n * 8 + n * 4 + n * 4          # the outputs (the points and the core distances were there before)
    print('20 000 x 64: peak growth %.2f MB, workspace %.2f MB' % (grown / 2 ** 20, nws / 2 ** 20))
    assert nws <= 2 * n + (1 << 16)          # O(N): flags, partials, slot
    assert grown <= nws + io + (64 << 20)
    assert nws + io + (64 << 20) < n * n * 8          # the f64 matrix this guards against: 3.2 GB
    o = ordering.cpu().numpy()
    np.testing.assert_array_equal(np.sort(o), np.arange(n))
    r, p, c = reach.cpu().numpy(), pred.cpu().numpy(), core.cpu().numpy()
    assert o[0] == 0 and np.isinf(r[0]) and np.isfinite(r[1:]).all() and p[0] == -1 and p[1:].min() >= 0
    assert (r[1:] >= np.maximum(c[1:], c[p[1:]])).all()          # a weight is no less than either end's core distance


def test_p2_hdbscan_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    X = data['training']['hidden']
    k = X.shape[1] + 1
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'hdbscan', '--hdbscan_min_cluster_size', str(k), str(3 * k)])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_hdbscan_aligned' / 'plot'
    walk, sizes, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Hdbscan.FILES)          # (%.17g: exact)
    assert list(walk.columns) == ['x', 'sample', 'source', 'dist'] and list(sizes.columns) == p2.Hdbscan.COLUMNS
    assert list(labels.columns) == ['mcs%d' % k, 'mcs%d' % (3 * k)] and len(walk) == len(labels) == len(X) and k == 17
    o_ord, o_core, o_reach, o_pred, m = oracle_mst(dmat(X), k)
    assert margins_hold(m)
    np.testing.assert_array_equal(walk.x.to_numpy(), np.arange(len(X)))
    np.testing.assert_array_equal(walk['sample'].to_numpy(), o_ord)
    np.testing.assert_array_equal(walk['source'].to_numpy(), o_pred[o_ord])
    close(walk.dist.to_numpy(), o_reach[o_ord])
    slt = single_linkage_tree(o_ord, o_reach)
    for row, mcs in enumerate((k, 3 * k)):
        ref = tree_to_labels(slt, mcs)[0]
        got = labels['mcs%d' % mcs].to_numpy()
        np.testing.assert_array_equal(got, ref)
        n_clusters = int(ref.max()) + 1
        assert (int(sizes.min_cluster_size[row]), int(sizes.n_clusters[row]), int(sizes.n_noise[row])) == (mcs, n_clusters, int((ref == -1).sum()))
        assert n_clusters >= 3 and -1 <= sizes.silhouette[row] <= sizes.denoise_silhouette[row] <= 1
    df = res['ae_mse']
    assert list(df.columns) == p2.Hdbscan.COLUMNS and np.allclose(df.to_numpy(), sizes.to_numpy(), rtol=1e-12, atol=0)
    # the default size is feat_dim + 1
    assert p2.get_arguments(['--cluster_method', 'hdbscan']).hdbscan_min_cluster_size is None
    # a second run finds the files and does not recompute; overwrite=True does
    hd = p2.Hdbscan(k, [k, 3 * k], str(plot.parent))
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Hdbscan.FILES]
    calls = []
    monkeypatch.setattr(p2, 'hdbscan_sizes', lambda *a, **kw: calls.append(1) or hdbscan_sizes(*a, **kw))
    again = hd.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Hdbscan.FILES] == stamps
    assert np.allclose(again.to_numpy(), sizes.to_numpy(), rtol=1e-12, atol=0) and hd.fit_ is None
    redo = hd.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and np.allclose(redo.to_numpy(), sizes.to_numpy(), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(hd.fit_.ordering_, o_ord)
    np.testing.assert_array_equal(pd.read_csv(plot / 'hdbscan_mst.csv', float_precision='round_trip').dist.to_numpy(), walk.dist.to_numpy())


def test_p4_hdbscan_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35)
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'hdbscan'])
    assert args.hdbscan_min_cluster_size is None          # feat_dim + 1
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_hdbscan_aligned'
    centres = {}
    for cohort in COHORTS:
        saved = np.load(out / ('%s_mcs-17.npy' % cohort), allow_pickle=True).item()
        ids, h = saved['cluster_id'], saved['hidden']
        assert sorted(saved) == ['cluster_id', 'encounter_id', 'hidden'] and len(ids) == len(data[cohort]['hidden'])
        assert sorted(set(ids.tolist()) - {-1}) == [0, 1, 2] and 0 < (ids == -1).sum() < len(ids) // 5
        centres[cohort] = np.stack([h[ids == i].mean(0) for i in range(3)])
        if cohort == 'training':          # the ids are in the order of descending systolic pressure
            sbp = data[cohort]['ob'][:, 0, :].mean(1)
            means = [sbp[ids == i].mean() for i in range(3)]
            assert means[0] > means[1] > means[2]
            k = h.shape[1] + 1
            raw = tree_to_labels(single_linkage_tree(*[oracle_mst(dmat(h), k)[i] for i in (0, 2)]), k)[0]
            assert np.array_equal(raw == -1, ids == -1) and len(set(zip(raw.tolist(), ids.tolist()))) == 4          # a renumbering of the oracle's labels
    for cohort in COHORTS[1:]:          # the same id is the same cluster in every cohort: the centres are 17 apart, the clusters 1 wide
        assert np.linalg.norm(centres[cohort] - centres['training'], axis=1).max() < 1.0
    assert np.linalg.norm(centres['training'][0] - centres['training'][1]) > 5.0
    # another size goes to another file
    args = p4.get_arguments(['--cluster_method', 'hdbscan', '--hdbscan_min_cluster_size', '40'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert all((out / ('%s_mcs-40.npy' % cohort)).exists() for cohort in COHORTS)
