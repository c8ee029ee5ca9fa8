"""Pin oracle/cluster_stats_oracle.py to the scores the reference's own classes produced (oracle/make_golden_stats.py:
internal_eval.DunnIndex / Sihouette / CHIndex / DBIndex and p2's two gap-statistic inertia definitions).  CPU only."""
import glob
import os

import numpy as np
import pytest

from oracle import cluster_stats_oracle as CO

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, 'cluster_stats_*.npz')))


def test_fixture_inventory():
    assert len(CASES) == 3


@pytest.mark.parametrize('name', CASES)
def test_oracle_matches_reference_scores(name):
    g = dict(np.load(os.path.join(GOLDEN, name)))
    x, lab = g['x'], g['labels']
    # the reference evaluates pairwise distances of float32 inputs in float32 for the inertia / Dunn terms: 1e-5 covers it
    np.testing.assert_allclose(CO.inertia_v1(x, lab), g['inertia_v1'], rtol=1e-5)
    np.testing.assert_allclose(CO.inertia_v2(x, lab), g['inertia_v2'], rtol=1e-5)
    np.testing.assert_allclose(CO.dunn(x, lab), g['dunn'], rtol=1e-5)
    np.testing.assert_allclose(CO.silhouette(x, lab), g['silhouette'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(CO.calinski_harabasz(x, lab), g['calinski_harabasz'], rtol=1e-5)
    np.testing.assert_allclose(CO.davies_bouldin(x, lab), g['davies_bouldin'], rtol=1e-5)


def test_pair_stats_consistency():
    rng = np.random.default_rng(0)
    x, lab = rng.normal(size=(50, 4)), rng.integers(0, 3, 50)
    _, K, S, Dmin, own_max = CO.pair_stats(x, lab)
    d = CO.distance_matrix(x)
    np.testing.assert_allclose(S.sum(1), d.sum(1), rtol=1e-12)
    assert (Dmin[np.arange(50), lab] == 0).all() and (own_max <= d.max(1) + 1e-12).all()


# ------------------------------------------------------------------------------------- the inputs of the GPU parity tests (oracle/validity_cases.py)
# Conditions on the INPUTS, checked without a GPU: the oracle the GPU tests compare with agrees with scikit-learn on every case, and the two ways a kernel
# could be wrong on them -- the norm form's cancellation on tight clusters, a cluster index clamped to one 64-cluster block -- move the indices by many
# times the bar the GPU tests hold them to (rtol 1e-5; the silhouette: + atol 1e-6).
from oracle import pairtile_emulation as PE  # noqa: E402
from oracle import validity_cases as VC  # noqa: E402

RTOL, SIL_ATOL = 1e-5, 1e-6
GEOMETRY_IDS = [(name, shifted) for name in VC.GEOMETRIES for shifted in (False, True)]


def sil_bar(value):
    return RTOL * abs(value) + SIL_ATOL


@pytest.mark.parametrize('name', list(VC.LABELLINGS))
def test_labelling_cases_are_what_they_claim(name):
    x, lab = VC.labelling_case(name)
    seed, n, d, k = VC.LABELLINGS[name]
    cnt = np.unique(lab, return_counts=True)[1]
    assert x.shape == (n, d) and x.dtype == np.float32 and n <= 1300 and d <= 20 and len(cnt) == k
    x2, lab2 = VC.labelling_case(name)
    assert np.array_equal(x, x2) and np.array_equal(lab, lab2)                  # seeded
    if name == 'k129':
        assert (cnt == 1).sum() == 43
    if name == 'noise_class':
        assert lab.min() == -1 and cnt[0] == cnt.max() and sorted(np.unique(lab)) == list(range(-1, 80))
    if name == 'gaps':
        assert set(np.unique(lab)) < {3 * c - 4 for c in range(10)}
    if name == 'k_is_n_minus_1':
        assert k == n - 1


@pytest.mark.parametrize('name', ['gaps', 'k129', 'k_is_n_minus_1'])
def test_the_one_matrix_oracle_equals_the_separate_functions(name):
    x, lab = VC.labelling_case(name)
    v = CO.validity_indices(x, lab)
    for key, fn in (('silhouette', CO.silhouette), ('dunn', CO.dunn), ('inertia_v1', CO.inertia_v1), ('inertia_v2', CO.inertia_v2)):
        np.testing.assert_allclose(v[key], fn(x, lab), rtol=1e-13, err_msg=key)
    _, K, S, _, _ = CO.pair_stats(x, lab)
    np.testing.assert_allclose(v['between'], np.stack([S[CO.encode(lab)[0] == c].sum(0) for c in range(K)]), rtol=1e-13)


@pytest.mark.parametrize('name', list(VC.LABELLINGS))
def test_oracle_matches_sklearn_on_the_labelling_cases(name):
    from sklearn import metrics
    x, lab = VC.labelling_case(name)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(CO.silhouette(x, lab), metrics.silhouette_score(x64, lab), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(CO.calinski_harabasz(x, lab), metrics.calinski_harabasz_score(x64, lab), rtol=1e-9)
    np.testing.assert_allclose(CO.davies_bouldin(x, lab), metrics.davies_bouldin_score(x64, lab), rtol=1e-9)


@pytest.mark.parametrize('name,shifted', GEOMETRY_IDS)
def test_oracle_matches_sklearn_on_the_geometry_cases(name, shifted):
    """scikit-learn takes its distances, between points and from points to centroids, from the norm form in f64: a d^2 is off by about 2^-53 |x|^2 there, which
    at |x|^2 = 1.6e7 of the shifted cases is 1e-4 of the tightest cluster's d^2.  So the figure it is held to is 2 x 2^-53 max |x|^2 / (the smallest non-zero
    mean squared cluster radius), and 1e-9 where that is less; the oracle takes differences."""
    from sklearn import metrics
    x, lab = VC.geometry_case(name, shifted=shifted)
    x64 = x.astype(np.float64)
    radius = np.array([((x64[lab == c] - x64[lab == c].mean(0)) ** 2).sum(1).mean() for c in range(3)])
    rtol = 1e-9 + 2 * 2.0 ** -53 * (x64 ** 2).sum(1).max() / radius[radius > 0].min()
    np.testing.assert_allclose(CO.silhouette(x, lab), metrics.silhouette_score(x64, lab), rtol=rtol, atol=1e-12)
    np.testing.assert_allclose(CO.calinski_harabasz(x, lab), metrics.calinski_harabasz_score(x64, lab), rtol=rtol)
    np.testing.assert_allclose(CO.davies_bouldin(x, lab), metrics.davies_bouldin_score(x64, lab), rtol=rtol)


@pytest.mark.parametrize('name,shifted', GEOMETRY_IDS)
def test_the_emulated_matrix_core_pass_moves_the_silhouette_only_on_the_hard_geometries(name, shifted):
    """Own-cluster sums replaced by what the pair-tile arithmetic gives (oracle/pairtile_emulation.py).  Benign cases (cluster spread >= 0.1): within a fifth
    of the bar -- the pass may stay on them.  Hard cases: at least 10 x the bar -- a GPU test at the bar notices the pass on them."""
    x, lab = VC.geometry_case(name, shifted=shifted)
    s64, s_own, s_all = PE.silhouettes(x, lab)
    np.testing.assert_allclose(s64, CO.silhouette(x, lab), rtol=1e-13)
    dev = abs(s_own - s64)
    print('%s%s: f64 %.8f, own-cluster sums emulated %.3g, all sums emulated %.3g, bar %.3g' % (name, ' shifted' if shifted else '', s64, dev, abs(s_all - s64), sil_bar(s64)))
    if name in VC.BENIGN:
        assert dev <= sil_bar(s64) / 5 and abs(s_all - s64) <= sil_bar(s64) / 5
    else:
        assert name in VC.HARD and dev >= 10 * sil_bar(s64)


@pytest.mark.parametrize('name', VC.MANY)
def test_clamping_the_cluster_index_moves_the_indices(name):
    """Clusters 64.. merged into cluster 63 (what a kernel that handles one 64-cluster block would see): CH, DB and Dunn in f64 move by >= 10 x rtol."""
    x, lab = VC.labelling_case(name)
    merged = VC.merged_beyond_64(lab)
    assert len(np.unique(merged)) == 64
    for fn in (CO.calinski_harabasz, CO.davies_bouldin, CO.dunn):
        a, b = fn(x, lab), fn(x, merged)
        assert abs(a - b) >= 10 * RTOL * abs(a), (fn.__name__, a, b)


def test_the_emulation_splits_and_bounds():
    """bf16 rounding to nearest even; hi + lo carries 16 bits; the approximate d^2 stays inside dic_pairtile.h's proven bound 2^-12 (n_i + n_j) and is near
    its typical 2^-17."""
    v = np.float32([1.00390625, 1.01171875, -1.00390625])                       # ties: to the even neighbour
    assert PE.bf16(v).tolist() == [1.0, 1.015625, -1.0]
    rng = np.random.default_rng(1)
    x = rng.normal(0, 3, (300, 20)).astype(np.float32)
    _, h, l, nrm = PE.planes(x)
    c = x - x.astype(np.float64).mean(0).astype(np.float32)
    assert np.abs(c - (h + l)[:, :20]).max() <= 2.0 ** -16 * np.abs(c).max()
    np.testing.assert_allclose(nrm, (c.astype(np.float64) ** 2).sum(1), rtol=1e-6)
    d2 = CO.distance_matrix(x) ** 2
    err = np.abs(PE.approx_d2(x).astype(np.float64) - d2) / (nrm[:, None] + nrm[None, :])
    assert err.max() < 2.0 ** -12 and 2.0 ** -22 < np.sqrt((err ** 2).mean()) < 2.0 ** -15


def test_routing_constant_is_the_sweeps():
    """cluster_stats.ROWSUM_SAFE_RATIO = 4 x the largest ratio at which the emulated silhouette, or an emulated total of own-cluster sums, reaches its bar
    (scripts/validity_sweep.py, recorded in profiles/validity_parity.json): the recorded sweep gives the constant, two of its runs around the crossing are
    recomputed, and the geometry cases fall on the side the GPU tests expect -- every hard one is refused, unit blobs are kept.  (The sums set the constant:
    the silhouette alone would put it at 4.9e-5, and 't0.1' would stay on the pass with its own-cluster sums 1e-4 off; that figure is kept for the centroid
    distances, which enter the silhouette only.)"""
    import json
    import runpy
    from deep_interpolation_clustering_amd import cluster_stats
    root = os.path.join(os.path.dirname(__file__), os.pardir)
    sweep = runpy.run_path(os.path.join(root, 'scripts', 'validity_sweep.py'))
    rec = json.load(open(os.path.join(root, 'profiles', 'validity_parity.json')))['emulation']
    crossing, value = sweep['constant'](rec['sweep'])
    assert crossing == rec['crossing_ratio'] and value == rec['ROWSUM_SAFE_RATIO'] == cluster_stats.ROWSUM_SAFE_RATIO
    assert 4 * crossing <= value <= 4.2 * crossing
    sil_crossing, sep_value = sweep['constant'](rec['sweep'], 'silhouette_over_bar')
    assert sil_crossing == rec['silhouette_crossing_ratio'] and sep_value == rec['ROWSUM_SAFE_SEPARATION'] == cluster_stats.ROWSUM_SAFE_SEPARATION
    assert 4 * sil_crossing <= sep_value <= 4.2 * sil_crossing <= value
    at = max((r for r in rec['sweep'] if r['deviation_over_bar'] >= 1.0), key=lambda r: r['ratio'])
    above = min((r for r in rec['sweep'] if r['ratio'] > at['ratio']), key=lambda r: r['ratio'])
    for r in (at, above):
        again = sweep['run'](r['step'], r['seed'], r['shifted'])
        np.testing.assert_allclose([again['ratio'], again['deviation']], [r['ratio'], r['deviation']], rtol=1e-6)
    for name, shifted in GEOMETRY_IDS:
        radius, sep, far = PE.geometry_ratios(*VC.geometry_case(name, shifted=shifted))
        assert name not in VC.HARD or radius < value * far / 100, (name, shifted, radius, sep, far)
        assert name != 'unit' or (radius >= 10 * value * far and sep >= 10 * sep_value * far)


def test_reference_draws_into_a_buffer_replay_numpys_global_stream():
    """p2's gap statistic draws its uniform reference sets from NumPy's GLOBAL legacy stream (p2_clustering_optK.py:372-375 upstream:
    np.random.random_sample(shape)).  global_uniform_into fills a reused buffer instead: same doubles, and the stream continues
    exactly where the original call would have left it (the k-means++ seeds that follow depend on it)."""
    import numpy as np
    from deep_interpolation_clustering_amd.p2_clustering_optK import global_uniform_into
    np.random.seed(123)
    want, after = np.random.random_sample((1000, 37)), np.random.random_sample(4)
    np.random.seed(123)
    np.random.standard_normal(3)                     # (a cached Gaussian in the legacy state must survive the detour)
    np.random.seed(123)
    buf = np.full((1000, 37), -1.0)
    got = global_uniform_into(buf)
    assert got is buf and np.array_equal(buf, want)
    assert np.array_equal(np.random.random_sample(4), after)
    np.random.seed(7)
    g1 = np.random.standard_normal(1)                # leaves has_gauss = 1
    global_uniform_into(buf)
    tail = np.random.standard_normal(2)
    np.random.seed(7)
    assert np.array_equal(np.random.standard_normal(1), g1)
    np.random.random_sample((1000, 37))
    assert np.array_equal(np.random.standard_normal(2), tail)
