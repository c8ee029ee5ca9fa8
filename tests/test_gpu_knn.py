"""k-th neighbour distances on the GPU (knn.py, csrc/dic_knn.hip) against oracles that share no code with them, and p2's k-distance branch
(p2_clustering_optK.py:102-120).

Small cases (N <= 4 000): numpy f64 difference form, ``np.sort(d2, 1)[:, k - 1]``.  Kernel and oracle each sum D exact f64 squares, so both lie within
(D + 2) 2^-53 relative of the true d^2 of the f32 points -- 2.9e-14 relative on d at D = 256; the bar is 1e-13 relative on d, and an oracle of 0 asks for 0.
Large cases: torch f64 on the GPU, norm form on centred data, row chunks, ``kthvalue``; the bar is that form's own worst case, computed from the data:
|ours^2 - oracle^2| <= 4 (D + 3) 2^-53 max|x - c|^2 + 2 (D + 2) 2^-53 oracle^2."""
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.knn import core_distances, k_distance_graph, kneedle_elbow, kth_neighbor_distance

pytestmark = pytest.mark.gpu

REL = 1e-13


def oracle_d2(X, k):
    """(N,) f64: the k-th smallest squared distance of every row, difference form in f64 (numpy, CPU)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(len(X))
    step = max(1, (1 << 24) // max(1, X.shape[0] * X.shape[1]))
    for s in range(0, len(X), step):
        diff = X[s:s + step, None, :] - X[None, :, :]
        d2 = np.einsum('ijk,ijk->ij', diff, diff)
        out[s:s + step] = np.sort(d2, 1)[:, k - 1]
    return out


def check_small(X, k, **kw):
    got = kth_neighbor_distance(X, k, **kw)
    ref = np.sqrt(oracle_d2(X, k))
    assert got.dtype == np.float64 and got.shape == (len(X),)
    zero = ref == 0
    err = np.abs(got[~zero] - ref[~zero]) / ref[~zero]
    print('k=%d N=%d D=%d: max rel err %.3g, zeros %d' % (k, len(X), X.shape[1], err.max() if err.size else 0.0, int(zero.sum())))
    assert np.all(got[zero] == 0.0)
    assert np.all(err <= REL), err.max()
    return got


def oracle_large(X, k, chunk=2048):
    """(oracle d (N,) f64 numpy, bar on d^2 (N,) f64 numpy): torch f64 norm form on centred data."""
    x = torch.as_tensor(X, device='cuda').double()
    x = x - x.mean(0, keepdim=True)
    sq = (x * x).sum(1)
    out = torch.empty(len(x), dtype=torch.float64, device='cuda')
    for s in range(0, len(x), chunk):
        d2 = sq[s:s + chunk, None] + sq[None, :] - 2.0 * (x[s:s + chunk] @ x.T)
        out[s:s + chunk] = torch.kthvalue(d2, k, dim=1).values
    d2 = out.clamp_min(0).cpu().numpy()
    D = X.shape[1]
    bar = 4 * (D + 3) * 2.0 ** -53 * float(sq.max()) + 2 * (D + 2) * 2.0 ** -53 * d2
    return np.sqrt(d2), bar


def blobs(n, d, k, spread, noise_frac, seed, box=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (k, d)) * (box or 4.0)
    m = int(n * (1 - noise_frac))
    X = centres[rng.integers(0, k, m)] + rng.normal(0, spread, (m, d))
    lo, hi = centres.min(0) - 1, centres.max(0) + 1
    noise = rng.uniform(lo, hi, (n - m, d))
    return rng.permutation(np.concatenate([X, noise])).astype(np.float32)


def reference_latents(n_clustered=11000, n_background=1000, seed=21):
    """The recipe of test_gpu_dbscan.test_reference_settings_latents: p1-like latents, clusters of two widths plus a diffuse background."""
    rng = np.random.default_rng(seed)
    k = 8
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(n_clustered, np.full(k, 1 / k))
    widths = np.array([0.05, 0.088] * 4)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)] + [rng.normal(0, 0.45, (n_background, 256))])
    return rng.permutation(X).astype(np.float32)


@pytest.mark.parametrize('d,k', [(256, 10), (8, 5), (6, 3)])
def test_blobs_with_noise(d, k):
    X = blobs(3000, d, 6, 0.1 if d == 256 else 0.15, 0.1, seed=d)
    got = check_small(X, k)
    assert got.min() > 0
    # a tensor on the device gives the same bits as the numpy array
    np.testing.assert_array_equal(kth_neighbor_distance(torch.as_tensor(X, device='cuda'), k), got)


def test_k_one_is_zero_and_k_n_is_the_farthest_point():
    X = blobs(1500, 16, 4, 0.2, 0.1, seed=2)
    got = kth_neighbor_distance(X, 1)
    assert got.shape == (1500,) and np.all(got == 0.0)
    check_small(X, len(X))
    check_small(X, len(X) - 1)
    check_small(X, 2)


def test_duplicates_give_exact_zeros_up_to_the_multiplicity():
    rng = np.random.default_rng(5)
    base = rng.normal(0, 1, (500, 12)).astype(np.float32)
    X = np.concatenate([base, base, base[:200], base[:200]])          # rows of base[:200] four times, of base[200:] twice
    perm = rng.permutation(len(X))
    X = X[perm]
    mult = np.concatenate([np.full(500, 2), np.full(500, 2), np.full(400, 4)])
    mult[:200] = 4
    mult[500:700] = 4
    mult = mult[perm]
    for k in (1, 2, 3, 4, 5):
        got = check_small(X, k)
        assert np.all(got[mult >= k] == 0.0) and np.all(got[mult < k] > 0.0)


def test_lattice_ties_compare_exactly():
    # integer lattice: every d^2 is a small integer, exact in every format, with massive ties -- the value at rank k is still unique
    g = np.arange(7, dtype=np.float32)
    X = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    X = np.concatenate([X, np.zeros((len(X), 1), np.float32)], 1)
    for k in (2, 7, 8, 27, 100, len(X)):
        ref = oracle_d2(X, k)
        assert np.all(ref == np.round(ref))
        np.testing.assert_array_equal(kth_neighbor_distance(X, k), np.sqrt(ref))


@pytest.mark.parametrize('n,d,k', [(1000, 32, 7), (257, 16, 4), (100, 8, 3), (5, 4, 5), (1, 4, 1)])
def test_sizes_off_the_tile_grid(n, d, k):
    rng = np.random.default_rng(n)
    X = rng.normal(0, 1, (n, d)).astype(np.float32)
    check_small(X, k)


def test_points_far_from_their_mean():
    # two clusters at +100 and -100 in every coordinate, width 0.01: the mean lies between them, the error bound of the tile products (~ 2^-12 |x|^2 = 40)
    # dwarfs every within-cluster d^2 (~ 0.003), every pair of a cluster is a candidate -- the case the exact phase exists for
    rng = np.random.default_rng(8)
    X = np.concatenate([100.0 + rng.normal(0, 0.01, (600, 16)), -100.0 + rng.normal(0, 0.01, (600, 16))])
    X = rng.permutation(X).astype(np.float32)
    stats = {}
    check_small(X, 10, stats=stats)
    assert stats['max_list'] >= 600
    check_small(X, 601)          # the first point of the other cluster


def test_reference_settings_latents():
    X = reference_latents()
    stats = {}
    got = kth_neighbor_distance(X, 256, stats=stats)
    ref, bar = oracle_large(X, 256)
    err = np.abs(got ** 2 - ref ** 2)
    print('12 000 x 256, k = 256: max |ours^2 - oracle^2| / bar = %.3g, max rel on d = %.3g, stats %r' % ((err / bar).max(), (np.abs(got - ref) / ref).max(), stats))
    assert np.all(err <= bar)
    assert stats['passes'] == 4 and stats['groups'] >= 1 and stats['candidates'] >= len(X)


def test_group_count_does_not_change_a_bit():
    X = reference_latents(2700, 300, seed=3)
    s0, s1 = {}, {}
    ref = kth_neighbor_distance(X, 64, stats=s0)
    assert s0['max_list'] > 1 and s0['budget_needed'] == 12 * s0['max_list']
    budget = max(s0['budget_needed'], 12 * s0['candidates'] // 7)
    got = kth_neighbor_distance(X, 64, candidate_budget=budget, stats=s1)
    print('default: %r, budget %d: %r' % (s0, budget, s1))
    assert s1['groups'] > 1 and s1['groups'] >= s0['groups']
    assert (s1['max_list'], s1['candidates']) == (s0['max_list'], s0['candidates'])
    np.testing.assert_array_equal(got, ref)
    # the smallest budget that works: one list at a time for the longest row
    np.testing.assert_array_equal(kth_neighbor_distance(X[:700], 64, candidate_budget=None), kth_neighbor_distance(X[:700], 64, candidate_budget=1 << 20))


def test_budget_below_one_list_reports_the_size_needed():
    X = reference_latents(2700, 300, seed=3)
    s0 = {}
    ref = kth_neighbor_distance(X, 64, stats=s0)
    with pytest.raises(knn.CandidateBudgetError, match='candidate_budget >= %d' % s0['budget_needed']) as ei:
        kth_neighbor_distance(X, 64, candidate_budget=s0['budget_needed'] - 12)
    assert ei.value.needed == s0['budget_needed']
    s1 = {}
    np.testing.assert_array_equal(kth_neighbor_distance(X, 64, candidate_budget=ei.value.needed, stats=s1), ref)
    assert s1['groups'] > 1
    # the C entry point itself
    L = N.lib()
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    small = s0['budget_needed'] - 12
    ws = torch.empty(L.dic_knn_workspace(n, d, small), dtype=torch.uint8, device='cuda')
    out = torch.empty(n, dtype=torch.float64, device='cuda')
    st = (N.C.c_int64 * 5)()
    rc = L.dic_knn_kth_distance(N.ptr(x), d, N.ptr(x.mean(0, keepdim=True)), n, d, 64, N.ptr(out), small, st, N.ptr(ws), ws.numel(), N.stream_of(x))
    assert rc == -3 and st[4] == s0['budget_needed'] and st[2] == s0['max_list']


@pytest.fixture(scope='module')
def candlist_rec():
    """scripts/record_knn_candlist_golden.py: the cases' inputs and how a run is reduced to what the fixture holds."""
    import runpy
    from types import SimpleNamespace
    return SimpleNamespace(**runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'scripts', 'record_knn_candlist_golden.py')))


CANDLIST_CASES = [('kth', 1537, 0, 20, 7), ('kth', 5, 0, 4, 5), ('lists', 700, 0, 36, 5), ('lists', 600, 300, 8, 4), ('lists', 256, 1, 4, 256),
                  ('ranks', 513, 0, 12, 9), ('ranks', 300, 0, 8, 1)]


@pytest.mark.parametrize('kind,n,m,d,k', CANDLIST_CASES)
def test_candidate_list_driver_equals_the_recorded_bits(candlist_rec, kind, n, m, d, k):
    """The k-th distances, the neighbour lists and the neighbour ranks against tests/golden/knn_candlist_parent.npz, BIT for bit (SHA-256 of the output
    bytes) and in all five stats words: what the last commit with three copies of the list protocol computed on an MI355X
    (scripts/record_knn_candlist_golden.py).  Each case at the default budget and at candidate_budget = budget_needed, the smallest legal one (the most
    groups).  k-th distance: 7 row blocks with a partial last one, and N = k = 5.  Lists: the self join; queries whose first row is no block boundary (the
    walk starts before the first listed row); a query block that starts at a boundary, k = N.  Ranks: two counting passes with absent and self targets and a
    last block of one row; one target."""
    assert (kind, n, m, d, k) in candlist_rec.CASES
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knn_candlist_parent.npz'))
    got = candlist_rec.run_case(knn, kind, n, m, d, k)
    assert len(got) == 2
    for name, value in got.items():
        print(name, value.tolist() if name.endswith('_stats') else '')
        assert value.dtype == golden[name].dtype and np.array_equal(value, golden[name]), name


def test_two_calls_are_bit_identical_and_core_distances_is_the_same_quantity():
    X = blobs(4000, 24, 5, 0.2, 0.15, seed=17)
    a = kth_neighbor_distance(X, 25)
    b = kth_neighbor_distance(X, 25)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(core_distances(X, 25), a)
    g = k_distance_graph(X, 25)
    np.testing.assert_array_equal(g['sorted_dist'], np.sort(a))
    assert (g['elbow_x'], g['elbow_y']) == kneedle_elbow(np.sort(a)) and g['k'] == 25


def test_memory_stays_within_the_workspace():
    n, d, k = 20000, 64, 65
    x = torch.randn(n, d, device='cuda')
    kth_neighbor_distance(x[:512], 5)          # (library and allocator warm)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = kth_neighbor_distance(x, k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    ws = N.lib().dic_knn_workspace(n, d, 0)
    io = n * d * 4 + n * 8 + d * 12          # a contiguous f32 copy of the points at most, the result, the centre (f64 and f32)
    print('20 000 x 64: peak growth %.1f MB, workspace %.1f MB' % (grown / 2 ** 20, ws / 2 ** 20))
    assert grown <= ws + io + (64 << 20)
    assert ws + io + (64 << 20) < n * n * 4          # the N x N f32 matrix this guards against: 1.6 GB
    assert np.isfinite(got).all() and got.min() > 0


def test_convention_is_sklearns():
    # sklearn is not the precision oracle (its kneighbors carries f32-level rounding); this checks that the oracle and upstream agree on the convention --
    # self included, k-th column -- within 4 f32 ulps of d (2.4e-7 relative; absolutely for the self distances)
    sk = pytest.importorskip('sklearn.neighbors')
    rng = np.random.default_rng(11)
    X = (rng.normal(0, 0.3, (4, 32))[rng.integers(0, 4, 2000)] + rng.normal(0, 0.1, (2000, 32))).astype(np.float32)
    tol = 4 * 2.0 ** -24
    for k in (1, 2, 8, 33):
        dist, ind = sk.NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)
        ref = np.sqrt(oracle_d2(X, k))
        dev = np.abs(dist[:, -1] - ref)
        print('k=%d: sklearn vs oracle max abs %.3g, max rel %.3g' % (k, dev.max(), (dev[ref > 0] / ref[ref > 0]).max() if (ref > 0).any() else 0.0))
        if k == 1:
            assert np.all(ref == 0) and np.all(dev <= tol)
        else:
            assert np.all(dev <= tol * ref)
        assert np.all(ind[:, 0] == np.arange(len(X)))          # the point itself is its first neighbour
        got = kth_neighbor_distance(X, k)
        assert np.all(np.abs(got - ref) <= REL * ref)


def _write_latents(root, sub, seed, n=(1500, 600, 600), d=16):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3.0, (3, d))
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    out = {}
    for cohort, m in zip(COHORTS, n):
        lab = rng.integers(0, 3, m)
        h = (centres[lab] + rng.normal(0, 0.25, (m, d))).astype(np.float32)
        h[: m // 20] = rng.uniform(-8, 8, (m // 20, d))
        ob = rng.normal(100 + 10 * lab[:, None, None], 1.0, (m, 6, 48)).astype(np.float32)
        pad = np.ones((m, 6, 48), np.float32)
        data = {'encounter_id': np.arange(m), 'hidden': h, 'ob': ob, 'padding_mask': pad}
        np.save(os.path.join(root, sub, cohort + '.npy'), data)
        out[cohort] = data
    return out


def test_p2_k_distance_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd.dbscan import dbscan_sweep
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    X = data['training']['hidden']
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'dbscan'])
    assert args.select_eps == 'k_distance_graph'
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_dbscan_aligned' / 'plot'
    kd, el = (pd.read_csv(plot / name, float_precision='round_trip') for name in ('k_distance.csv', 'k_distance_elbow.csv'))          # (%.17g: exact)
    assert list(kd.columns) == ['sample', 'dist'] and list(el.columns) == ['k', 'elbow_x', 'elbow_y']
    # k = min_samples - 1 = feat_dim, the curve sorted, equal to the oracle's
    k = X.shape[1]
    assert k == 16 and int(el.k[0]) == k
    dist = kd.dist.to_numpy()
    np.testing.assert_array_equal(kd['sample'].to_numpy(), np.arange(1, len(X) + 1))
    assert np.all(np.diff(dist) >= 0)
    ref = np.sort(np.sqrt(oracle_d2(X, k)))
    assert np.all(np.abs(dist - ref) <= REL * ref) and np.all(dist[ref == 0] == 0)
    # the elbow row is the knee of that column
    ex, ey = kneedle_elbow(dist)
    assert ex is not None and (int(el.elbow_x[0]), float(el.elbow_y[0])) == (ex, ey)
    # return value and dbscan_eps.csv: the eps table, as before
    df = res['ae_mse']
    eps_range = np.arange(.5, 5.1, .5)
    assert list(df.columns) == p2.Dbscan.COLUMNS and len(df) == len(eps_range)
    fits = dbscan_sweep(X, eps_range, X.shape[1] + 1)
    for row, (lab, core) in zip(df.itertuples(), fits):
        assert (row.n_core, row.n_noise) == (len(core), int((lab == -1).sum()))
    on_disk = pd.read_csv(plot / 'dbscan_eps.csv')
    np.testing.assert_allclose(on_disk.to_numpy(), df.to_numpy(), rtol=1e-12, equal_nan=True)
    # the object keeps the graph; a second run finds the table and does not recompute
    db = p2.Dbscan(eps_range[:1], X.shape[1] + 1, str(plot.parent))
    stamp = (plot / 'k_distance.csv').stat().st_mtime_ns
    calls = []
    monkeypatch.setattr(p2, 'k_distance_graph', lambda *a, **kw: calls.append(1) or k_distance_graph(*a, **kw))
    db.train(data['training'], data['validation'], 'k_distance_graph')
    assert db.k_distance_ is None and not calls and (plot / 'k_distance.csv').stat().st_mtime_ns == stamp
    db.train(data['training'], data['validation'], 'k_distance_graph', overwrite=True)
    assert calls == [1] and db.k_distance_['elbow_x'] == ex and db.k_distance_['k'] == k
    np.testing.assert_array_equal(db.k_distance_['sorted_dist'], dist)


def test_p2_other_select_eps_skips_the_graph(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 36, n=(600, 100, 100))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'dbscan', '--select_eps', 'none'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_dbscan_aligned' / 'plot'
    assert (plot / 'dbscan_eps.csv').exists() and len(res['ae_mse']) == 10
    assert not (plot / 'k_distance.csv').exists() and not (plot / 'k_distance_elbow.csv').exists()
