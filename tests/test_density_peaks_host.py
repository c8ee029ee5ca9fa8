"""Density-peaks clustering: the definition of include/dic_hip.h restated in numpy from the f64 distance matrix (the yardstick tests/test_gpu_density_peaks.py
holds the GPU to), the fixed-seed cases with their tie margins asserted for EVERY row, and the host functions of density_peaks.py (centre selection, label
propagation, the halo rule, input checks) tested from given arrays.  Nothing here needs a GPU.

The yardstick is written independently of density_peaks.py: explicit loops in rank order where the module uses lexsort and pointer doubling."""
import functools

import numpy as np
import pytest

from deep_interpolation_clustering_amd import density_peaks as DP
from deep_interpolation_clustering_amd.dbscan import sq_threshold

MARGIN = 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------------- yardstick
def matrix(X, block=128):
    """(N, N) f64: the exact squared distances of the f32 rows in difference form (every difference of two f32 is exact in f64), built blockwise."""
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    n = len(x)
    out = np.empty((n, n))
    for s in range(0, n, block):
        diff = x[s:s + block, None, :] - x[None, :, :]
        out[s:s + block] = np.einsum('ijk,ijk->ij', diff, diff)
    return out


def y_dc(D2, percent):
    """dc='auto': the mean distance to the k-th neighbour, the point itself counted, k = max(1, int(N percent / 100))."""
    n = len(D2)
    k = max(1, int(n * (percent / 100.0)))
    return float(np.mean(np.sqrt(np.sort(D2, axis=1)[:, k - 1])))


def y_density(D2, density, dc=None, k=None):
    """rho (N): 'cutoff': the neighbours under DBSCAN's rule f32(d^2) <= t(dc), the point itself removed (int64); 'knn': 1 / (1 + kth / mean(kth))."""
    if density == 'cutoff':
        t = np.float32(sq_threshold(float(dc)))
        return (D2.astype(np.float32) <= t).sum(axis=1).astype(np.int64) - 1
    return y_density_from_kth(np.sqrt(np.sort(D2, axis=1)[:, k - 1]))


def y_density_from_kth(kth):
    return 1.0 / (1.0 + kth / np.mean(kth, dtype=np.float64))


def y_order(rho):
    """(order, rank) of the strict total order: denser = larger rho, then smaller index."""
    order = np.asarray(sorted(range(len(rho)), key=lambda i: (-rho[i], i)), dtype=np.int64)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return order, rank


def y_delta_parent(D2, rho):
    """(delta, parent, margin): parent = the minimiser of (d^2, rank) over the denser points, -1 and the largest distance for the densest; margin = the
    smallest relative gap between the smallest and second-smallest eligible distance over ALL rows that have two."""
    order, rank = y_order(rho)
    n = len(rho)
    delta, parent = np.empty(n), np.empty(n, dtype=np.int64)
    margin = np.inf
    for r, i in enumerate(order):
        if r == 0:
            delta[i], parent[i] = np.sqrt(D2[i].max()), -1
            continue
        row = D2[i, order[:r]]
        at = int(np.argmin(row))          # the FIRST minimum: the smallest rank among equal distances
        delta[i], parent[i] = np.sqrt(row[at]), order[at]
        if r > 1:
            two = np.sqrt(np.partition(row, 1)[:2])
            margin = min(margin, (two[1] - two[0]) / two[1] if two[1] > 0 else 0.0)
    return delta, parent, margin


def y_centres(rho, delta, K):
    """(centres in rank order, relative gap between gamma_(K) and gamma_(K+1)): the K largest gamma, ties to the smaller rank."""
    _, rank = y_order(rho)
    gamma = np.asarray(rho, dtype=np.float64) * delta
    by = sorted(range(len(rho)), key=lambda i: (-gamma[i], rank[i]))
    gap = (gamma[by[K - 1]] - gamma[by[K]]) / gamma[by[K - 1]] if K < len(rho) and gamma[by[K - 1]] > 0 else np.inf
    return np.asarray(sorted(by[:K], key=lambda i: rank[i]), dtype=np.int64), gap


def y_labels(rho, parent, centres):
    order, _ = y_order(rho)
    slot = {int(c): s for s, c in enumerate(centres)}
    labels = np.full(len(rho), -1, dtype=np.int64)
    for i in order:          # parents come first in rank order
        labels[i] = slot[int(i)] if int(i) in slot else labels[parent[i]]
    return labels


def y_halo(D2, rho, labels, dc, K):
    """(halo (N) bool, border2 (K) int64, ties): border2[c] = max rho_i + rho_j over the pairs of different labels within d_c, i in c; ties = the points
    with 2 rho_i == border2[label_i]."""
    t = np.float32(sq_threshold(float(dc)))
    pair = (D2.astype(np.float32) <= t) & (labels[:, None] != labels[None, :])
    s = np.where(pair, rho[:, None] + rho[None, :], 0)
    border2 = np.zeros(K, dtype=np.int64)
    for c in range(K):
        if (labels == c).any():
            border2[c] = s[labels == c].max(initial=0)
    return 2 * rho < border2[labels], border2, int((2 * rho == border2[labels]).sum())


# -------------------------------------------------------------------------------------------------------------------------------------------- cases
def blobs(n, d, k, seed, spread=4.0, sigma=1.0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, spread, (k, d))
    return (centres[rng.integers(0, k, n)] + rng.normal(0, sigma, (n, d))).astype(np.float32)


def lattice():
    """600 x 4: 240 distinct points of the integer lattice {0..3}^4, 120 of them twice and 120 three times, shuffled: every d^2 is an exact integer,
    duplicates give delta = 0, equal distances abound, and with dc = 1 the lattice neighbours lie exactly AT the cut-off (band pairs)."""
    rng = np.random.default_rng(5)
    grid = np.stack(np.meshgrid(*[np.arange(4)] * 4, indexing='ij'), axis=-1).reshape(-1, 4)
    pts = grid[rng.permutation(256)[:240]]
    rows = np.concatenate([pts[:120]] * 2 + [pts[120:]] * 3)
    return rows[rng.permutation(len(rows))].astype(np.float32)


def halo_case():
    """400 x 8: two overlapping blobs (a border between them) and a tight far clump of 12 points (a cluster without border pairs)."""
    rng = np.random.default_rng(13)
    a = rng.normal(0, 1.0, (200, 8))
    b = rng.normal(0, 1.0, (188, 8)) + np.r_[3.0, np.zeros(7)]
    far = rng.normal(0, 0.2, (12, 8)) + np.r_[0.0, 60.0, np.zeros(6)]
    rows = np.concatenate([a, b, far])
    return rows[rng.permutation(400)].astype(np.float32)


# name -> (points, K, percent for dc='auto' (None: dc given), dc, n_neighbors of the 'knn' density)
# (the blobs overlap, and h's d_c is given: a cluster WITHOUT border pairs must hold no point of rho = 0, or 2 rho would equal its border2 = 0)
CASES = {
    'a': (lambda: blobs(700, 8, 3, 1, spread=1.0), 3, 2.0, None, 12),          # three row blocks, a partial last one
    'b': (lambda: blobs(257, 256, 3, 2, spread=0.2), 3, 2.0, None, 6),         # full width; one point in the last block
    'c': (lambda: blobs(513, 6, 4, 3, spread=1.5), 4, 2.0, None, 10),          # zero-padded to 8
    'd': (lambda: blobs(4200, 16, 5, 5, spread=1.5), 5, 2.0, None, 20),        # 17 x 17 tiles on 256 workgroups: ranges cross row-block changes
    'e': (lattice, 4, None, 1.0, 7),
    'h': (halo_case, 3, None, 1.8, 8),
}
RANDOM = ('a', 'b', 'c', 'd', 'h')


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything of a case, computed once and shared (read only): points, matrix, and per density rho, delta, parent, centres, labels."""
    make, K, percent, dc, k = CASES[name]
    X = make()
    D2 = matrix(X)
    dc = y_dc(D2, percent) if dc is None else dc
    out = {'X': X, 'D2': D2, 'K': K, 'dc': dc, 'k': k, 'percent': percent}
    for density in ('cutoff', 'knn'):
        rho = y_density(D2, density, dc=dc, k=k)
        out[density] = solve(D2, rho, K)
    c = out['cutoff']
    c['halo'], c['border2'], c['halo_ties'] = y_halo(D2, c['rho'], c['labels'], dc, K)
    for v in out.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def solve(D2, rho, K):
    delta, parent, margin = y_delta_parent(D2, rho)
    centres, gap = y_centres(rho, delta, K)
    return {'rho': rho, 'delta': delta, 'parent': parent, 'margin': margin, 'centres': centres, 'gap': gap, 'labels': y_labels(rho, parent, centres)}


@pytest.mark.parametrize('name', RANDOM)
def test_cases_keep_their_tie_margins(name):
    """No row exempted: the nearest and second-nearest denser point, gamma_(K) and gamma_(K+1), and 2 rho against border2 are all away from a tie."""
    c = case(name)
    for density in ('cutoff', 'knn'):
        s = c[density]
        print('case %s %s: delta margin %.3g, gamma gap %.3g' % (name, density, s['margin'], s['gap']))
        assert s['margin'] > MARGIN and s['gap'] > MARGIN
    assert c['cutoff']['halo_ties'] == 0


def test_case_shapes_and_what_they_exercise():
    assert [case(n)['X'].shape for n in 'abceh'] == [(700, 8), (257, 256), (513, 6), (600, 4), (400, 8)] and CASES['d'][0]().shape == (4200, 16)
    e = case('e')
    assert np.array_equal(e['D2'], np.round(e['D2'])) and e['dc'] == 1.0 and 1.0 <= sq_threshold(1.0) < 1.000001
    assert (e['D2'] == 1.0).sum() > 0                                   # pairs exactly AT the cut-off: inside DBSCAN's 2^-20 band of the threshold
    mult = (e['D2'] == 0).sum(axis=1)
    assert set(mult.tolist()) == {2, 3}                                 # every point two or three times
    s = e['cutoff']
    assert (s['delta'] == 0).sum() >= 300 and np.unique(s['rho']).size < 40          # duplicates; integer densities tie everywhere
    h = case('h')['cutoff']
    assert h['halo'].any() and (h['border2'] == 0).any() and (h['border2'] > 0).any()          # a halo, and a cluster without border pairs
    assert np.bincount(h['labels'], minlength=3).min() >= 12


def test_lattice_tie_rules_in_the_yardstick():
    """Equal exact distances go to the denser point; equal densities to the smaller index."""
    e = case('e')
    s = e['cutoff']
    order, rank = y_order(s['rho'])
    assert all((s['rho'][a], -a) > (s['rho'][b], -b) for a, b in zip(order, order[1:]))
    ties = 0
    for i in range(600):
        p = s['parent'][i]
        if p < 0:
            continue
        denser = np.flatnonzero(rank < rank[i])
        best = denser[e['D2'][i, denser] == e['D2'][i, p]]
        ties += best.size > 1
        assert rank[p] == rank[best].min() and e['D2'][i, p] == e['D2'][i, denser].min()
    assert ties > 100


# ------------------------------------------------------------------------------------------------------------------ the module's host functions
@pytest.mark.parametrize('name', ['a', 'c', 'e', 'h'])
@pytest.mark.parametrize('density', ['cutoff', 'knn'])
def test_host_functions_equal_the_yardstick(name, density):
    c = case(name)
    s = c[density]
    order, rank = DP.density_order(s['rho'])
    y_ord, y_rank = y_order(s['rho'])
    assert np.array_equal(order, y_ord) and np.array_equal(rank, y_rank)
    centres = DP.select_centres(s['rho'], s['delta'], rank, n_clusters=c['K'])
    assert np.array_equal(centres, s['centres']) and centres[0] == order[0]
    assert np.array_equal(DP.propagate_labels(s['parent'], centres), s['labels'])
    if density == 'cutoff':
        assert np.array_equal(DP.halo_rule(s['rho'], s['labels'], s['border2']), s['halo'])


def test_thresholds_select_centres():
    s = case('a')['cutoff']
    order, rank = y_order(s['rho'])
    got = DP.select_centres(s['rho'], s['delta'], rank, rho_min=5, delta_min=2.0)
    want = [i for i in order if (s['rho'][i] > 5 and s['delta'][i] > 2.0) or rank[i] == 0]
    assert got.tolist() == want and len(want) >= 2
    # thresholds nothing passes: the densest point alone, and one cluster
    alone = DP.select_centres(s['rho'], s['delta'], rank, rho_min=10 ** 9, delta_min=1e300)
    assert alone.tolist() == [order[0]]
    assert (DP.propagate_labels(s['parent'], alone) == 0).all()
    only_delta = DP.select_centres(s['rho'], s['delta'], rank, delta_min=2.0)
    assert only_delta.tolist() == [i for i in order if s['delta'][i] > 2.0 or rank[i] == 0]
    with pytest.raises(ValueError):
        DP.select_centres(s['rho'], s['delta'], rank)
    with pytest.raises(ValueError):
        DP.select_centres(s['rho'], s['delta'], rank, n_clusters=2, rho_min=1)


def test_gamma_ties_go_to_the_smaller_rank():
    rho = np.array([4, 4, 2, 2, 1], dtype=np.int64)
    delta = np.array([9.0, 1.0, 2.0, 2.0, 4.0])          # gamma 36, 4, 4, 4, 4
    _, rank = DP.density_order(rho)
    assert DP.select_centres(rho, delta, rank, n_clusters=3).tolist() == [0, 1, 2]
    assert DP.select_centres(rho, delta, rank, n_clusters=5).tolist() == [0, 1, 2, 3, 4]
    assert DP.gamma_gap(rho * delta, 1) == 9.0 and DP.gamma_gap(rho * delta, 2) == 1.0 and DP.gamma_gap(rho * delta, 5) == np.inf


def test_a_parent_chain_of_length_n():
    n = 5000
    rng = np.random.default_rng(0)
    order = rng.permutation(n)
    parent = np.empty(n, dtype=np.int64)
    parent[order[0]] = -1
    parent[order[1:]] = order[:-1]          # every point's parent is the point one rank above
    assert (DP.propagate_labels(parent, order[:1]) == 0).all()
    centres = order[[0, 1000, 4999]]
    want = np.empty(n, dtype=np.int64)
    want[order] = np.where(np.arange(n) < 1000, 0, np.where(np.arange(n) < 4999, 1, 2))
    assert np.array_equal(DP.propagate_labels(parent, centres), want)
    with pytest.raises(ValueError):
        DP.propagate_labels(parent, order[1:2])          # the densest point is no centre
    parent[order[0]] = order[3]
    with pytest.raises(ValueError):
        DP.propagate_labels(parent, order[10:11])        # a cycle


def test_halo_rule_is_strict():
    rho = np.array([3, 4, 5, 0])
    assert DP.halo_rule(rho, np.array([0, 0, 0, 1]), np.array([8, 0])).tolist() == [True, False, False, False]


def test_argument_checks_need_no_gpu():
    X = np.zeros((10, 4), np.float32)
    with pytest.raises(ValueError, match='halo'):
        DP.DensityPeaks(2, density='knn', halo=True)
    with pytest.raises(ValueError):
        DP.DensityPeaks()
    with pytest.raises(ValueError):
        DP.DensityPeaks(2, rho_min=1)
    with pytest.raises(ValueError):
        DP.DensityPeaks(0)
    with pytest.raises(ValueError):
        DP.DensityPeaks(2, density='gaussian')
    with pytest.raises(ValueError):
        DP.DensityPeaks(2, dc=-1.0)
    with pytest.raises(ValueError):
        DP.DensityPeaks(2, percent=0)
    with pytest.raises(ValueError, match='n_clusters=11'):
        DP.DensityPeaks(11).fit(X)
    with pytest.raises(ValueError, match='n_clusters=11'):
        DP.density_peaks_sweep(X, [2, 11])
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        DP.DensityPeaks(2).fit(bad)
    with pytest.raises(NotImplementedError, match='256'):
        DP.DensityPeaks(2).fit(np.zeros((10, 257), np.float32))
    with pytest.raises(ValueError, match='2-D'):
        DP.DensityPeaks(2).fit(np.zeros(10, np.float32))
    with pytest.raises(RuntimeError, match='not fitted'):
        DP.DensityPeaks(2).predict(X)
    with pytest.raises(RuntimeError, match='not fitted'):
        DP.DensityPeaks(2).decision_graph()
    assert DP.density_peaks_sweep(X, []) == {}
    assert DP.DensityPeaks(3, halo=True).get_params()['halo'] is True
