"""OPTICS on the GPU (optics.py, csrc/dic_optics.hip) against a yardstick that shares no code with it, and p2's --cluster_method optics branch
(p2_clustering_optK.py:86-88,171-223).

The yardstick: ``dmat`` -- the numpy f64 difference-form distance matrix of the f32 points -- and ``oracle_optics``, the loop of the definition on it
(sklearn's ``OPTICS(metric='precomputed').fit(dmat(X))``, which ``test_convention_is_sklearns`` holds it to bit for bit).  Kernel and yardstick each sum D
exact f64 squares, so both lie within (D + 2) 2^-53 relative of the true d^2: finite core and reachability distances compare at 1e-13 relative (the bar of
test_gpu_knn.py) plus 1e-15, the grid both are rounded to.  Ordering and predecessor compare EXACTLY; what keeps that honest is computed from the yardstick
itself: wherever the loop chooses between two distinct values -- the arg-min against the next distinct unprocessed reachability, a candidate r against a
differing finite reach[q], and with a finite max_eps every distance against max_eps -- they are at least 1e-10 apart relatively, three orders above the arithmetic's error, so both sides must decide alike; equal
values are equal bits on both sides (one distance function, symmetric) and go to the smaller index.  ``test_margins_of_the_cases`` asserts the margins."""
import functools
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.optics import OPTICS, cluster_optics_dbscan, cluster_optics_xi, optics_graph

pytestmark = pytest.mark.gpu

REL, GRID = 1e-13, 1e-15
MARGIN = 1e-10


def dmat(X):
    """(N, N) f64: the distances of the rows of X, difference form in f64 (numpy, CPU)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((len(X), len(X)))
    step = max(1, (1 << 24) // max(1, X.shape[0] * X.shape[1]))
    for s in range(0, len(X), step):
        diff = X[s:s + step, None, :] - X[None, :, :]
        out[s:s + step] = np.sqrt(np.einsum('ijk,ijk->ij', diff, diff))
    return out


def oracle_optics(D, min_samples, max_eps=np.inf):
    """The definition as a loop over the matrix: ``(ordering, core, reach, pred, (arg-min margin, update margin, max_eps margin))``.  The first two margins are
    the smallest relative gaps the loop met between two DISTINCT values it had to order (inf where it met none); the third is the smallest relative distance
    of any pair distance or unrounded core distance to a finite ``max_eps`` -- the ``d <= max_eps`` and ``core > max_eps`` decisions (inf for max_eps = inf)."""
    n = len(D)
    core = np.sort(D, axis=1)[:, min_samples - 1].copy()
    eps_margin = np.inf
    if np.isfinite(max_eps):
        eps_margin = float(min(np.abs(D - max_eps).min(), np.abs(core - max_eps).min()) / max_eps)
    core[core > max_eps] = np.inf
    core = np.around(core, 15)
    reach, pred = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    processed, ordering = np.zeros(n, dtype=bool), np.empty(n, dtype=np.int64)
    pick_margin = update_margin = np.inf
    for step in range(n):
        idx = np.flatnonzero(~processed)
        vals = reach[idx]
        p = idx[np.argmin(vals)]          # the first minimum: the smallest index
        lowest = vals.min()
        above = vals[(vals > lowest) & np.isfinite(vals)]
        if above.size and lowest > 0:
            pick_margin = min(pick_margin, (above.min() - lowest) / lowest)
        processed[p] = True
        ordering[step] = p
        if not np.isfinite(core[p]):
            continue
        q = np.flatnonzero(~processed & (D[p] <= max_eps))
        r = np.around(np.maximum(D[p, q], core[p]), 15)
        old = reach[q]
        differ = np.isfinite(old) & (old != r) & (np.minimum(old, r) > 0)
        if differ.any():
            update_margin = min(update_margin, float((np.abs(r - old)[differ] / np.minimum(old, r)[differ]).min()))
        better = r < old
        reach[q[better]] = r[better]
        pred[q[better]] = p
    return ordering, core, reach, pred, (pick_margin, update_margin, eps_margin)


def blobs(n, d, k, spread, noise_frac, seed, box=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (k, d)) * (box or 4.0)
    m = int(n * (1 - noise_frac))
    X = centres[rng.integers(0, k, m)] + rng.normal(0, spread, (m, d))
    lo, hi = centres.min(0) - 1, centres.max(0) + 1
    noise = rng.uniform(lo, hi, (n - m, d))
    return rng.permutation(np.concatenate([X, noise])).astype(np.float32)


def reference_latents(n_clustered=11000, n_background=1000, seed=21):
    rng = np.random.default_rng(seed)
    k = 8
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(n_clustered, np.full(k, 1 / k))
    widths = np.array([0.05, 0.088] * 4)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)] + [rng.normal(0, 0.45, (n_background, 256))])
    return rng.permutation(X).astype(np.float32)


@functools.lru_cache(maxsize=None)
def points(name):
    if name in ('A', 'G'):
        return blobs(1500, 16, 5, 0.2, 0.1, seed=3)
    if name == 'B':
        return blobs(1000, 8, 4, 0.15, 0.1, seed=8)
    if name in ('C20', 'C257'):
        return reference_latents(1800, 200, seed=21)
    if name == 'D':
        return np.random.default_rng(1).normal(0, 1, (257, 4)).astype(np.float32)          # off every tile grid
    if name == 'E':
        return blobs(6000, 8, 6, 0.15, 0.1, seed=6)          # more rows than one pass of the grid (256 workgroups x 16 waves)
    if name == 'F':
        return np.random.default_rng(1000).normal(0, 1, (1000, 6)).astype(np.float32)          # D % 4 != 0: padded
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _matrix(letter):
    return dmat(points({'C': 'C20', 'G': 'A'}.get(letter, letter)))


def matrix(name):
    return _matrix(name[0])


MIN_SAMPLES = {'A': 17, 'B': 5, 'C20': 20, 'C257': 257, 'D': 3, 'E': 9, 'F': 7, 'G': 17}
CASES = sorted(MIN_SAMPLES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, min_samples, max_eps, oracle tuple) -- computed once, shared by every test, never written to."""
    X, k = points(name), MIN_SAMPLES[name]
    max_eps = np.inf
    if name == 'G':          # 1.5 x the median core distance: a tenth of the points get no core distance, about as many are never reached -- the inf ties
        max_eps = 1.5 * float(np.median(case('A')[3][1]))
    out = oracle_optics(matrix(name), k, max_eps)
    for a in out[:4]:
        a.setflags(write=False)
    return X, k, max_eps, out


def close(got, ref):
    """inf in the same places; finite values within 1e-13 relative + 1e-15."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.all(got[~fin] == ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= REL * ref[fin] + GRID), (err / np.maximum(ref[fin], 1e-300)).max()
    return float((err / np.maximum(ref[fin], GRID)).max()) if fin.any() else 0.0


@pytest.mark.parametrize('name', CASES)
def test_margins_of_the_cases(name):
    """The condition under which exact equality of ordering and predecessor is the right demand (module docstring)."""
    pick, update, at_eps = case(name)[3][4]
    print('case %s: arg-min margin %.3g, update margin %.3g, max_eps margin %.3g' % (name, pick, update, at_eps))
    assert pick >= MARGIN and update >= MARGIN and at_eps >= MARGIN


@pytest.mark.parametrize('name', CASES)
def test_graph_equals_the_oracle(name):
    X, k, max_eps, (o_ord, o_core, o_reach, o_pred, (pick, update, at_eps)) = case(name)
    assert pick >= MARGIN and update >= MARGIN and at_eps >= MARGIN          # a case that fails this is a wrong choice of input, not a reason to compare loosely
    stats = {}
    ordering, core, reach, pred = optics_graph(X, k, max_eps, stats=stats)
    assert ordering.dtype == np.int64 and pred.dtype == np.int64 and core.dtype == np.float64 and reach.dtype == np.float64
    assert stats['steps'] == len(X) - 1
    np.testing.assert_array_equal(np.sort(ordering), np.arange(len(X)))
    e_core, e_reach = close(core, o_core), close(reach, o_reach)
    print('case %s: N=%d D=%d min_samples=%d: max rel err core %.3g reach %.3g; inf core %d, unreached %d'
          % (name, len(X), X.shape[1], k, e_core, e_reach, int(np.isinf(o_core).sum()), int(np.isinf(o_reach).sum())))
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(pred, o_pred)
    if name == 'G':
        assert np.isinf(o_core).sum() > 100 and np.isinf(o_reach).sum() > 100


HAVE_CLUSTERS = {'A', 'B', 'C20', 'D', 'E', 'G'}          # C257 and F are one cluster: their labels are compared all the same


@pytest.mark.parametrize('name', CASES)
def test_labels_equal_the_extraction_on_the_oracle_graph(name):
    X, k, max_eps, (o_ord, o_core, o_reach, o_pred, _) = case(name)
    fit = OPTICS(min_samples=k, max_eps=max_eps).fit(X)
    ref, hier = cluster_optics_xi(reachability=o_reach, predecessor=o_pred, ordering=o_ord, min_samples=k)
    np.testing.assert_array_equal(fit.labels_, ref)
    np.testing.assert_array_equal(fit.cluster_hierarchy_, hier)
    assert fit.labels_.max() >= 1 or name not in HAVE_CLUSTERS          # (those inputs have clusters to find)
    eps = float(np.median(o_core[np.isfinite(o_core)]))
    fit = OPTICS(min_samples=k, max_eps=max_eps, cluster_method='dbscan', eps=eps).fit(X)
    ref = cluster_optics_dbscan(reachability=o_reach, core_distances=o_core, ordering=o_ord, eps=eps)
    np.testing.assert_array_equal(fit.labels_, ref)
    assert not hasattr(fit, 'cluster_hierarchy_')
    assert ((ref == -1).any() and ref.max() >= 1) or name not in HAVE_CLUSTERS
    np.testing.assert_array_equal(OPTICS(min_samples=k, max_eps=max_eps, cluster_method='dbscan').fit_predict(X),
                                  cluster_optics_dbscan(reachability=o_reach, core_distances=o_core, ordering=o_ord, eps=max_eps))


def exact(X, k, max_eps=np.inf):
    """Inputs whose distances are exact (or exactly equal) in both arithmetics: everything compares bit for bit."""
    o_ord, o_core, o_reach, o_pred, _ = oracle_optics(dmat(X), k, max_eps)
    ordering, core, reach, pred = optics_graph(X, k, max_eps)
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
    # correctly rounded on both sides.  Zero distances (core 0 at k = 2), and the two copies of a point tie in every comparison they enter
    rng = np.random.default_rng(5)
    base = (rng.integers(-32, 33, (500, 12)) / 8.0).astype(np.float32)
    assert len(np.unique(base, axis=0)) == 500
    X = np.concatenate([base, base])[rng.permutation(1000)]
    _, core, reach, _ = exact(X, k)
    if k == 2:
        assert np.all(core == 0.0) and (reach == 0.0).sum() == 500


LINE_N = 16640          # 256 workgroups x 16 waves x 4 rows in flight = 16 384 rows per trip of a step's row loop: the smallest multiple of 256 above it


@functools.lru_cache(maxsize=None)
def line(n):
    """Points whose walk has a closed form: point j sits at ``(pos[j], 0, 0, 0)``, ``pos`` a seeded permutation of 0..n-1 with ``pos[0] = 0`` -- integers below
    2^24, so every coordinate and distance is exact.  With min_samples = 2 every core distance is 1.0, and OPTICS and Prim both walk the line left to right with
    no tie to break: the point at position i + 1 is reached at exactly 1.0, every other one at 2.0 or more.  ``(X, ordering, reach, pred)``, read-only."""
    rng = np.random.default_rng(16)
    pos = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    X = np.zeros((n, 4), dtype=np.float32)
    X[:, 0] = pos
    ordering = np.argsort(pos)          # the point at position i
    pred = np.full(n, -1, dtype=np.int64)
    pred[ordering[1:]] = ordering[:-1]
    reach = np.ones(n)
    reach[0] = np.inf
    for a in (X, ordering, reach, pred):
        a.setflags(write=False)
    return X, ordering, reach, pred


def test_second_trip_of_the_row_loop_on_a_line():
    # the oracle cases end at 6000 rows, one trip of the row loop; the matrix oracle is O(N^2), so the long input is one whose answer is known in closed form,
    # which the oracle confirms at 300 points first
    X, o_ord, o_reach, o_pred = line(300)
    ordering, core, reach, pred, _ = oracle_optics(dmat(X), 2)
    assert np.all(core == 1.0)
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(reach, o_reach)
    np.testing.assert_array_equal(pred, o_pred)
    X, o_ord, o_reach, o_pred = line(LINE_N)
    ordering, core, reach, pred = optics_graph(X, 2)
    assert np.all(core == 1.0)
    np.testing.assert_array_equal(ordering, o_ord)
    np.testing.assert_array_equal(reach, o_reach)
    np.testing.assert_array_equal(pred, o_pred)


def test_small_sets_and_min_samples_forms():
    rng = np.random.default_rng(2)
    X2 = rng.normal(0, 1, (2, 4)).astype(np.float32)
    ordering, core, reach, pred = exact(X2, 2)
    assert list(ordering) == [0, 1] and list(pred) == [-1, 0] and np.isinf(reach[0]) and reach[1] == core[0] == core[1]
    # min_samples = N: the core distance is the farthest point's
    X = rng.normal(0, 1, (40, 8)).astype(np.float32)
    o = oracle_optics(dmat(X), 40)
    got = optics_graph(X, 40)
    np.testing.assert_array_equal(got[0], o[0])
    np.testing.assert_array_equal(got[3], o[3])
    close(got[1], o[1])
    close(got[2], o[2])
    # a fraction: max(2, int(f N))
    a, b = optics_graph(X, 0.25), optics_graph(X, 10)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(optics_graph(X, 0.01), optics_graph(X, 2)):
        np.testing.assert_array_equal(u, v)
    fit = OPTICS(min_samples=0.25, min_cluster_size=0.2).fit(X)
    np.testing.assert_array_equal(fit.ordering_, b[0])
    # sklearn's errors
    with pytest.raises(ValueError, match=r'min_samples must be no greater than the number of samples \(40\). Got 41'):
        OPTICS(min_samples=41).fit(X)
    with pytest.raises(ValueError, match='Specify an epsilon smaller than 2.0. Got 3.0.'):
        OPTICS(min_samples=5, max_eps=2.0, cluster_method='dbscan', eps=3.0).fit(X)
    # one point: no integer min_samples fits it (sklearn: min_samples >= 2 > N), and a fraction resolves to 2 neighbours of a 1-point set
    X1 = X[:1]
    with pytest.raises(ValueError, match='no greater than the number of samples'):
        optics_graph(X1, 2)
    with pytest.raises(ValueError, match='n_neighbors <= n_samples_fit'):
        optics_graph(X1, 0.5)


def test_one_point_through_the_abi():
    # N = 1 at the C entry point (no step is launched): the point is the ordering
    L = N.lib()
    x = torch.zeros(1, 4, device='cuda')
    core = torch.zeros(1, dtype=torch.float64, device='cuda')
    ordering = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    pred = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    reach = torch.zeros(1, dtype=torch.float64, device='cuda')
    ws = torch.empty(L.dic_optics_workspace(1, 4), dtype=torch.uint8, device='cuda')
    rc = L.dic_optics_order(N.ptr(x), 4, 1, 4, N.ptr(core), float('inf'), N.ptr(ordering), N.ptr(reach), N.ptr(pred), N.ptr(ws), ws.numel(), N.stream_of(x))
    assert rc == 0
    assert ordering.item() == 0 and pred.item() == -1 and np.isinf(reach.item())


def test_two_calls_and_a_device_tensor_give_identical_bits():
    X, k, max_eps, _ = case('G')
    a = optics_graph(X, k, max_eps)
    b = optics_graph(X, k, max_eps)
    c = optics_graph(torch.as_tensor(X, device='cuda'), k, max_eps)
    for u, v, t in zip(a, b, c):
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u, t)
    X, k, _, _ = case('F')          # padded to a multiple of 4 on the way in
    for u, v in zip(optics_graph(X, k), optics_graph(torch.as_tensor(X, device='cuda'), k)):
        np.testing.assert_array_equal(u, v)


def test_core_distances_are_the_rounded_knn_distances():
    X, k, _, _ = case('A')
    fit = OPTICS(min_samples=k).fit(X)
    np.testing.assert_array_equal(fit.core_distances_, np.around(knn.core_distances(X, k), 15))
    X, k, max_eps, _ = case('G')
    ref = knn.core_distances(X, k)
    ref[ref > max_eps] = np.inf
    np.testing.assert_array_equal(OPTICS(min_samples=k, max_eps=max_eps).fit(X).core_distances_, np.around(ref, 15))


@pytest.mark.parametrize('name', ['B', 'D'])
def test_convention_is_sklearns(name):
    sk = pytest.importorskip('sklearn.cluster')
    X, k, max_eps, (o_ord, o_core, o_reach, o_pred, _) = case(name)
    ref = sk.OPTICS(min_samples=k, max_eps=max_eps, metric='precomputed').fit(matrix(name))
    np.testing.assert_array_equal(ref.ordering_, o_ord)
    np.testing.assert_array_equal(ref.core_distances_, o_core)
    np.testing.assert_array_equal(ref.reachability_, o_reach)
    np.testing.assert_array_equal(ref.predecessor_, o_pred)
    ours = OPTICS(min_samples=k, max_eps=max_eps).fit(X)
    np.testing.assert_array_equal(ours.labels_, ref.labels_)
    np.testing.assert_array_equal(ours.cluster_hierarchy_, ref.cluster_hierarchy_.reshape(-1, 2))


def test_memory_stays_within_the_workspace():
    n, d, k = 20000, 64, 65
    x = torch.randn(n, d, device='cuda')
    core = torch.as_tensor(np.around(knn.kth_neighbor_distance(x, k), 15), device='cuda')
    L = N.lib()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    nws = L.dic_optics_workspace(n, d)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    ordering = torch.empty(n, dtype=torch.int32, device='cuda')
    pred = torch.empty(n, dtype=torch.int32, device='cuda')
    reach = torch.empty(n, dtype=torch.float64, device='cuda')
    N.check(L.dic_optics_order(N.ptr(x), d, n, d, N.ptr(core), float('inf'), N.ptr(ordering), N.ptr(reach), N.ptr(pred), N.ptr(ws), nws, N.stream_of(x)),
            'dic_optics_order')
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    io = n * 8 + n * 4 + n * 4          # the outputs (the points and the core distances were there before)
    print('20 000 x 64: peak growth %.2f MB, workspace %.2f MB' % (grown / 2 ** 20, nws / 2 ** 20))
    assert nws <= 2 * n + (1 << 16)          # O(N): flags, partials, slot
    assert grown <= nws + io + (64 << 20)
    assert nws + io + (64 << 20) < n * n * 8          # the f64 matrix this guards against: 3.2 GB
    o = ordering.cpu().numpy()
    np.testing.assert_array_equal(np.sort(o), np.arange(n))
    r = reach.cpu().numpy()
    assert np.isinf(r[0]) and np.isfinite(r[1:]).all() and pred.cpu().numpy()[1:].min() >= 0


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


def test_p2_optics_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    X = data['training']['hidden']
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'optics'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_optics_aligned' / 'plot'
    rp, sm = (pd.read_csv(plot / name, float_precision='round_trip') for name in ('reachability_xi.csv', 'optics_xi.csv'))          # (%.17g: exact)
    assert list(rp.columns) == ['x', 'sample', 'dist', 'label'] and list(sm.columns) == ['min_samples', 'n_clusters', 'n_noise']
    k = X.shape[1] + 1
    assert k == 17 and int(sm.min_samples[0]) == k and len(rp) == len(X)          # every row: noise is not dropped
    o_ord, o_core, o_reach, o_pred, (pick, update, _) = oracle_optics(dmat(X), k)
    assert pick >= MARGIN and update >= MARGIN
    np.testing.assert_array_equal(rp.x.to_numpy(), np.arange(len(X)))
    sample = rp['sample'].to_numpy()
    np.testing.assert_array_equal(np.sort(sample), np.arange(len(X)))
    np.testing.assert_array_equal(sample, o_ord)
    close(rp.dist.to_numpy(), o_reach[o_ord])
    ref_labels, _ = cluster_optics_xi(reachability=o_reach, predecessor=o_pred, ordering=o_ord, min_samples=k, min_cluster_size=k, xi=.05)
    labels = rp.label.to_numpy()
    np.testing.assert_array_equal(labels, ref_labels[o_ord])
    n_clusters = len(set(labels.tolist())) - (1 if -1 in labels else 0)
    assert (int(sm.n_clusters[0]), int(sm.n_noise[0])) == (n_clusters, int((labels == -1).sum())) and n_clusters >= 3
    df = res['ae_mse']
    assert list(df.columns) == p2.Optics.COLUMNS and df.to_numpy().tolist() == sm.to_numpy().tolist()
    # a second run finds the table and does not recompute; overwrite=True does
    op = p2.Optics(k, 'xi', str(plot.parent))
    stamps = [(plot / name).stat().st_mtime_ns for name in ('reachability_xi.csv', 'optics_xi.csv')]
    calls = []
    monkeypatch.setattr(p2, 'OPTICS', lambda *a, **kw: calls.append(1) or OPTICS(*a, **kw))
    again = op.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in ('reachability_xi.csv', 'optics_xi.csv')] == stamps
    assert again.to_numpy().tolist() == sm.to_numpy().tolist() and op.fit_ is None
    redo = op.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and redo.to_numpy().tolist() == sm.to_numpy().tolist()
    np.testing.assert_array_equal(op.fit_.ordering_, o_ord)
    np.testing.assert_array_equal(pd.read_csv(plot / 'reachability_xi.csv', float_precision='round_trip').dist.to_numpy(), rp.dist.to_numpy())
    # the dbscan extraction of the same class
    od = p2.Optics(k, 'dbscan', str(plot.parent))
    dd = od.train(data['training'], data['validation'])
    rd = pd.read_csv(plot / 'reachability_dbscan.csv', float_precision='round_trip')
    np.testing.assert_array_equal(rd['sample'].to_numpy(), o_ord)
    np.testing.assert_array_equal(rd.label.to_numpy(), cluster_optics_dbscan(reachability=o_reach, core_distances=o_core, ordering=o_ord, eps=np.inf)[o_ord])
    assert int(dd.n_noise[0]) == int((rd.label.to_numpy() == -1).sum()) and (plot / 'optics_dbscan.csv').exists()
