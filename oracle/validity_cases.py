"""Seeded inputs for the validity-index tests (TEST INFRASTRUCTURE ONLY): labellings of the kinds the clustering branches hand to
cluster_stats.py, and K-cluster geometries from benign to ones on which the norm form of a distance cancels.  Plain NumPy; shared by
tests/test_cluster_stats_oracle.py (CPU) and tests/test_gpu_cluster_stats.py."""
import numpy as np

# name -> (seed, n, d, K).  Each at most 1300 x 20: cluster_stats_oracle.distance_matrix holds n x n x d doubles.
LABELLINGS = {
    'k64': (64, 1000, 20, 64),             # the last K of one 64-cluster block
    'k65': (65, 1000, 20, 65),             # one cluster into the second block
    'k70': (70, 1000, 8, 70),
    'k129': (129, 1200, 8, 129),           # two blocks and one cluster; a third of the clusters are singletons
    'k200': (200, 1300, 12, 200),
    'noise_class': (81, 1200, 8, 81),      # labels -1, 0..79 with -1 the largest class
    'gaps': (7, 600, 8, 7),                # label values 3 c - 4, c from 0..9 with three of them unused
    'k_is_n_minus_1': (119, 120, 4, 119),
    'd6': (6, 500, 6, 5),                  # a width that is zero-padded to 8 columns
    'd20': (20, 700, 20, 7),
}
MANY = [name for name, c in LABELLINGS.items() if c[3] > 64]


def _blobs(rng, n, d, k, centre_spread=3.0):
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)                                      # every cluster occurs
    cen = rng.normal(0, centre_spread, (k, d))
    return cen[lab] + rng.normal(0, 1, (n, d)), lab


def labelling_case(name):
    """(x (n, d) f32, labels (n,) int64): unit blobs with centre spread 3."""
    seed, n, d, k = LABELLINGS[name]
    rng = np.random.default_rng(seed)
    if name == 'k129':
        x, lab = _blobs(rng, n, d, k)
        single = np.arange(0, k, 3)                             # clusters 0, 3, 6, ..: their first point only
        extra = np.isin(lab, single) & (np.arange(n) >= k)
        lab[extra] = (lab[extra] + 1) % k                       # (1, 4, ..: never a singleton cluster)
        assert (np.bincount(lab, minlength=k) == 1).sum() == len(single) == 43
    elif name == 'noise_class':
        x, lab = _blobs(rng, n, d, 80)
        noise = rng.random(n) < 0.25
        noise[:80] = False
        x[noise] = rng.uniform(-4, 4, (int(noise.sum()), d))          # (scattered among the blobs; no wider than they are, so the largest diameter is a cluster's)
        lab = np.where(noise, -1, lab)
        assert np.bincount(lab + 1).argmax() == 0 and len(np.unique(lab)) == k
    elif name == 'gaps':
        x, lab = _blobs(rng, n, d, k)
        lab = 3 * np.array([0, 1, 2, 4, 5, 7, 9])[lab] - 4
    elif name == 'k_is_n_minus_1':
        x = rng.normal(0, 3, (n, d))
        lab = np.minimum(np.arange(n), n - 2)                   # the last two points share a cluster
        lab = lab[rng.permutation(n)]
    else:
        x, lab = _blobs(rng, n, d, k)
    return x.astype(np.float32), lab.astype(np.int64)


def merged_beyond_64(labels):
    """What a kernel that clamps the cluster index to 63 sees: clusters 64.. (in sorted order of the label values) become cluster 63."""
    _, inv = np.unique(labels, return_inverse=True)
    return np.minimum(inv, 63)


# name -> (centre spread, cluster spread, d) of K unit-free Gaussian clusters; 'duplicates' and 'near_pair' are built below.
TIGHTNESS = {
    'unit': (1.0, 1.0, 16),
    't1': (10.0, 1.0, 16),
    't0.1': (10.0, 0.1, 16),
    't0.01': (10.0, 0.01, 16),
    't0.001': (10.0, 0.001, 16),
    'wide_t0.01': (30.0, 0.01, 64),
}
BENIGN = ['unit', 't1', 't0.1']                                 # cluster spread >= a tenth of a unit: the matrix-core pass may keep these
HARD = ['t0.01', 't0.001', 'wide_t0.01', 'duplicates', 'near_pair']
GEOMETRIES = BENIGN + HARD
SHIFT = 1000.0


def geometry_case(name, n=1500, k=3, d=None, shifted=False, seed=0):
    """(x (n, d) f32, labels): k clusters of the named geometry; ``shifted``: + 1000 in every coordinate (the f32 grid is then 6e-5).
    'duplicates': cluster 0 is n_0 copies of one point, the others as 't1'.  'near_pair': clusters 0 and 1 are 0.2 apart and 20 from
    cluster 2 (further clusters: centre spread 10), all of spread 0.02; nine tenths of the points are outside the pair, so the mean
    all points are taken relative to lies 18 from it."""
    cs, t, d0 = TIGHTNESS.get(name, (10.0, {'duplicates': 1.0, 'near_pair': 0.02}.get(name), 16))
    d = d or d0
    rng = np.random.default_rng([seed, n, k, d, GEOMETRIES.index(name)])
    lab = rng.integers(0, k, n)
    if name == 'near_pair':
        lab = np.where(rng.random(n) < 0.9, rng.integers(2, k, n), rng.integers(0, 2, n))
    lab[:k] = np.arange(k)
    cen = rng.normal(0, cs, (k, d))
    noise = rng.normal(0, t, (n, d))
    if name == 'near_pair':
        u, w = rng.normal(0, 1, (2, d))
        cen[2] = 0
        cen[0] = 20.0 * u / np.linalg.norm(u)
        cen[1] = cen[0] + 0.2 * w / np.linalg.norm(w)
    if name == 'duplicates':
        noise[lab == 0] = 0
    x = cen[lab] + noise + (SHIFT if shifted else 0.0)
    return x.astype(np.float32), lab.astype(np.int64)
