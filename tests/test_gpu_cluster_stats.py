"""GPU parity of the K-sweep statistics (csrc/dic_pairdist.hip through cluster_stats.py / internal_eval.py) against the
reference's own scores (tests/golden/cluster_stats_*.npz), the CPU oracle, and scikit-learn.  ``-m gpu``."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import cluster_stats_oracle as CO
from oracle import validity_cases as VC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, 'cluster_stats_*.npz')))


@pytest.fixture(scope='module')
def cs():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from deep_interpolation_clustering_amd import cluster_stats
    return cluster_stats


@pytest.mark.parametrize('name', CASES)
def test_scores_match_reference(cs, name):
    g = dict(np.load(os.path.join(GOLDEN, name)))
    x, lab = g['x'], g['labels']
    st = cs.pair_stats(x, lab)
    np.testing.assert_allclose(cs.inertia_v1(x, lab, st), g['inertia_v1'], rtol=1e-5)
    np.testing.assert_allclose(cs.inertia_v2(x, lab, st), g['inertia_v2'], rtol=1e-5)
    # the intra-cluster-only pass (dic_cluster_intra_sums: what the gap statistic's reference sets run) gives the reference's inertias too
    np.testing.assert_allclose(cs.inertia_v1(x, lab), g['inertia_v1'], rtol=1e-5)
    np.testing.assert_allclose(cs.inertia_v2(x, lab), g['inertia_v2'], rtol=1e-5)
    np.testing.assert_allclose(cs.dunn_index(x, lab, st), g['dunn'], rtol=1e-5)
    np.testing.assert_allclose(cs.silhouette_score(x, lab, st), g['silhouette'], rtol=1e-5, atol=1e-6)
    # ... and from the sums-only pass on the matrix cores (dic_cluster_pair_rowsums: what p2's sweep runs when no Dunn index is asked for)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(cs, 'ROWSUM_MIN_POINTS', 0)
        np.testing.assert_allclose(cs.silhouette_score(x, lab, cs.pair_stats(x, lab, need_min=False, need_max=False)), g['silhouette'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cs.calinski_harabasz_score(x, lab), g['calinski_harabasz'], rtol=1e-5)
    np.testing.assert_allclose(cs.davies_bouldin_score(x, lab), g['davies_bouldin'], rtol=1e-5)


@pytest.mark.parametrize('n,d,k', [(1, 4, 1), (63, 4, 2), (64, 8, 1), (65, 36, 3), (1000, 256, 7), (1537, 20, 64), (300, 6, 5), (1000, 20, 65), (1200, 8, 129),
                                   (300, 4, 200)])
def test_pair_stats_match_oracle(cs, n, d, k):
    """Every S / Dmin / own_max entry against the float64 oracle: ragged tile edges, D not a multiple of the 32-wide
    staging chunk (and not of 4: zero padded), K at and past 64, 128 and at two thirds of the points, empty label values skipped by the encoder."""
    rng = np.random.default_rng(n * 1000 + d)
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    lab = rng.integers(0, k, n) * 3 - 4              # arbitrary label values; some may be unused
    st = cs.pair_stats(x, lab)
    olab, K, S, Dmin, own_max = CO.pair_stats(x, lab)
    assert st.K == K and np.array_equal(st.labels.cpu().numpy(), olab)
    np.testing.assert_allclose(st.S.cpu().numpy(), S, rtol=2e-6, atol=1e-5)
    np.testing.assert_allclose(st.Dmin.cpu().numpy(), Dmin, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(st.own_max.cpu().numpy(), own_max, rtol=2e-6, atol=1e-6)


def test_validity_indices_match_sklearn(cs):
    """The drop-in callables of internal_eval.py against scikit-learn on k-means-like data (2 000 x 256)."""
    from sklearn import metrics
    from deep_interpolation_clustering_amd.internal_eval import CHIndex, DBIndex, DunnIndex, Sihouette
    rng = np.random.default_rng(5)
    cen = rng.normal(0, 1.0, (4, 256))
    lab = rng.integers(0, 4, 2000)
    x = (cen[lab] + rng.normal(0, 1.0, (2000, 256))).astype(np.float32)
    lab[rng.integers(0, 2000, 100)] = rng.integers(0, 4, 100)        # some misassigned points
    np.testing.assert_allclose(Sihouette()(x, lab), metrics.silhouette_score(x, lab), rtol=1e-5)
    np.testing.assert_allclose(CHIndex()(x, lab), metrics.calinski_harabasz_score(x, lab), rtol=1e-5)
    np.testing.assert_allclose(DBIndex()(x, lab), metrics.davies_bouldin_score(x, lab), rtol=1e-5)
    np.testing.assert_allclose(DunnIndex()(x, lab), CO.dunn(x, lab), rtol=1e-5)
    with pytest.raises(ValueError):
        Sihouette()(x, np.zeros(2000, dtype=np.int64))


def test_full_size_properties(cs):
    """75 000 x 256 latents (BASELINE cfg2), K = 4: properties that need no O(N^2) oracle -- row sums of S against
    torch.cdist for sampled rows, symmetry of the cluster-to-cluster sums, the Dmin / own_max invariants."""
    from oracle.synth import latent_blobs
    x, lab = latent_blobs(11, 75000, 256, 4)
    xd = torch.tensor(x, device='cuda')
    st = cs.pair_stats(xd, lab)
    pick = torch.arange(0, 75000, 293, device='cuda')
    ref = torch.cdist(xd[pick].double(), xd.double())
    np.testing.assert_allclose(st.S[pick].double().sum(1).cpu().numpy(), ref.sum(1).cpu().numpy(), rtol=2e-6)
    onehot = torch.nn.functional.one_hot(st.labels, st.K).double()
    between = onehot.t() @ st.S.double()                       # [a][b] = sum_{i in a, j in b} d_ij
    np.testing.assert_allclose(between.cpu().numpy(), between.t().cpu().numpy(), rtol=1e-6)
    assert float(st.Dmin.gather(1, st.labels[:, None]).abs().max()) == 0.0          # every point is its own nearest
    lab_t = st.labels[pick]
    own = torch.where(st.labels[None, :] == lab_t[:, None], ref, torch.zeros_like(ref)).max(1).values
    np.testing.assert_allclose(st.own_max[pick].cpu().numpy(), own.cpu().numpy(), rtol=2e-6)
    s = cs.silhouette_score(xd, lab, st)
    assert -1.0 <= s <= 1.0


@pytest.mark.parametrize('n,d,k', [(63, 4, 2), (65, 36, 3), (1000, 256, 7), (1537, 20, 64), (300, 6, 5), (5000, 256, 1), (1000, 20, 65), (1200, 8, 129)])
def test_intra_only_pass_equals_own_column_of_the_full_pass(cs, n, d, k):
    """dic_cluster_intra_sums visits only the column tiles of the clusters a row tile's own rows belong to (sum_c n_c^2 of the N^2 pairs):
    every point's own-cluster sum must be BIT-identical to the own column of the full pass (same tiles, same summation order), for
    row tiles that straddle cluster boundaries, singleton clusters and K = 1."""
    rng = np.random.default_rng(n + d + k)
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)                       # every label occurs
    if k > 3:
        lab[lab == k - 1] = 0
        lab[k - 1] = k - 1                       # a singleton cluster
    full = cs.pair_stats(x, lab, need_min=True, need_max=False)          # (with Dmin: the difference-form kernel; sums only would take the matrix-core pass)
    intra = cs.pair_stats(x, lab, intra_only=True)
    own = full.S.gather(1, full.labels[:, None])[:, 0]
    assert torch.equal(intra.S_own, own)
    assert intra.S is None and torch.equal(intra.intra_sums(), full.intra_sums())


@pytest.mark.parametrize('n,d,k,spread', [(63, 4, 2, 1.0), (700, 36, 3, 1.0), (3000, 256, 7, 1.0), (1537, 20, 64, 1.0), (5000, 256, 1, 1.0), (2600, 256, 2, 30.0),
                                          (20000, 256, 4, 1.0), (513, 255, 2, 1.0)])
def test_intra_totals_on_the_matrix_cores_match_f64(cs, n, d, k, spread):
    """dic_cluster_intra_totals (centred hi / lo bf16 planes, norms folded into the MFMA inner product, block pairs I <= J only): every cluster's sum of pairwise
    distances against the f64 sum of the same pairs, for clusters smaller than a block, cluster ends inside a block, a singleton cluster, a width that needs
    zero-padding, and clusters far from the origin (``spread``: the norm form's cancellation is what the centring removes).  Measured <= 2e-7; the reference sums
    f32 distances (tests of the golden tables: rtol 1e-5).  Same result on a second call (no atomics)."""
    rng = np.random.default_rng(n + d + k)
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)
    if k > 3:
        lab[lab == k - 1] = 0
        lab[k - 1] = k - 1                       # a singleton cluster
    x = (rng.normal(0, 1, (n, d)) + spread * rng.normal(0, 1, (k, d))[lab]).astype(np.float32)
    st = cs.intra_totals(x, lab)
    assert st.S is None and st.S_own is None
    got = st.intra_sums().cpu().numpy()
    xd = torch.as_tensor(x, device='cuda', dtype=torch.float64)
    want = np.zeros(k)
    for c in range(k):
        xc = xd[torch.as_tensor(lab == c, device='cuda')]
        for lo in range(0, xc.shape[0], 128):          # (torch.cdist returned a third of this sum for 4096 x 5000 f64 rows on this image)
            want[c] += float((xc[lo:lo + 128, None, :] - xc[None, :, :]).square_().sum(-1).sqrt_().sum())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
    assert np.array_equal(cs.intra_totals(x, lab).intra_sums().cpu().numpy(), got)
    # and the two inertia definitions built on it agree with the per-point pass (dic_cluster_intra_sums)
    per_point = cs.pair_stats(x, lab, intra_only=True)
    np.testing.assert_allclose(cs.inertia_v1(x, lab), cs.inertia_v1(x, lab, per_point), rtol=2e-6)
    np.testing.assert_allclose(cs.inertia_v2(x, lab), cs.inertia_v2(x, lab, per_point), rtol=2e-6)


@pytest.mark.parametrize('n,d,k,spread', [(1, 4, 1, 1.0), (63, 4, 2, 1.0), (700, 36, 3, 1.0), (3000, 256, 7, 1.0), (1537, 20, 64, 1.0), (2600, 256, 2, 10.0),
                                          (70001, 256, 3, 1.0), (513, 255, 2, 1.0)])
def test_row_sums_on_the_matrix_cores_match_the_difference_form(cs, n, d, k, spread, monkeypatch):
    """dic_cluster_pair_rowsums (need_min = need_max = False: split bf16 planes relative to the mean, norms folded into the inner product, contiguous tile ranges per
    workgroup, slots added in order) against the direct-difference f32 pass (dic_cluster_pairdist): every S[i][c], with empty label values, a singleton cluster,
    clusters smaller than a block, more tiles than workgroups (70 001 points: slots that split a (row block, cluster) run between two workgroups).  Measured:
    1.1e-6 of the row's largest sum at 70 001 x 256 (the size the pass is used from: cluster_stats.ROWSUM_MIN_POINTS), up to 4.4e-6 on the tiny shapes forced
    through it here (63 points in 4 dimensions: few pairs, nothing averages).  The same result on a second call."""
    monkeypatch.setattr(cs, 'ROWSUM_MIN_POINTS', 0)
    rng = np.random.default_rng(n + d + k)
    lab = rng.integers(0, k, n)
    lab[:min(k, n)] = np.arange(min(k, n))
    if k > 3:
        lab[lab == k - 1] = 0
        lab[k - 1] = k - 1                       # a singleton cluster
    x = (rng.normal(0, 1, (n, d)) + spread * rng.normal(0, 1, (k, d))[lab]).astype(np.float32)
    want = cs.pair_stats(x, lab, need_min=True, need_max=False)
    got = cs.pair_stats(x, lab, need_min=False, need_max=False)
    assert got.Dmin is None and got.own_max is None and torch.equal(got.labels, want.labels)
    w, g_ = want.S.double(), got.S.double()
    scale = w.max(1, keepdim=True).values.clamp(min=1e-3)
    assert float(((g_ - w).abs() / scale).max()) <= (3e-6 if n >= 8192 else 1.5e-5)
    assert torch.equal(cs.pair_stats(x, lab, need_min=False, need_max=False).S, got.S)
    if n > k:
        np.testing.assert_allclose(cs.silhouette_score(x, lab, got), cs.silhouette_score(x, lab, want), rtol=1e-5, atol=2e-6 if n >= 8192 else 2e-5)


@pytest.fixture(scope='module')
def rec():
    """scripts/record_intra_golden.py: the cases' inputs and how an output is reduced to what the fixture holds."""
    import runpy
    from types import SimpleNamespace
    return SimpleNamespace(**runpy.run_path(os.path.join(os.path.dirname(GOLDEN), os.pardir, 'scripts', 'record_intra_golden.py')))


INTRA_TOTALS = [(700, 36, 3), (1537, 20, 64), (513, 255, 2), (5900, 8, 1)]
INTRA_ROWSUMS = [(700, 36, 3), (1537, 20, 64), (4400, 8, 3)]


@pytest.mark.parametrize('kind,n,d,k', [('totals',) + c for c in INTRA_TOTALS] + [('rowsums',) + c for c in INTRA_ROWSUMS])
def test_intra_passes_equal_the_recorded_bits(cs, rec, kind, n, d, k, monkeypatch):
    """dic_cluster_intra_totals / dic_cluster_pair_rowsums against tests/golden/intra_pairtile_parent.npz, BIT for bit: what the last commit with a tile loop of
    its own in dic_intra.hip computed on an MI355X (scripts/record_intra_golden.py).  The move onto dic_pairtile.h reorders no floating-point operation.  Totals:
    a cluster end inside a block, clusters smaller than a block and a singleton, a zero-padded width with a block of one row, 300 tiles on 256 workgroups (the
    strided assignment wraps).  Row sums (all bytes by SHA-256, and sampled rows): the same small shapes, and more than 256 tiles (contiguous ranges that split a
    (row block, cluster) run between two workgroups)."""
    assert (n, d, k) in (rec.TOTALS if kind == 'totals' else rec.ROWSUMS)
    monkeypatch.setattr(cs, 'ROWSUM_MIN_POINTS', 0)
    golden = np.load(os.path.join(GOLDEN, 'intra_pairtile_parent.npz'))
    got = (rec.totals_case if kind == 'totals' else rec.rowsums_case)(cs, n, d, k)
    assert got
    for name, value in got.items():
        assert value.dtype == golden[name].dtype and np.array_equal(value, golden[name]), name


def test_gap_table_equals_reference(tmp_path):
    """KM.compute_gap_internal_metric against the table the REFERENCE's own method produced (oracle/make_golden_gap.py; p2:353-410):
    every column at rtol 1e-5 AND the position of NumPy's global stream afterwards -- i.e. the draw order reference set -> that fit's
    k-means++ seeds -> next reference set (which this package overlaps with the GPU work on a worker thread) is upstream's."""
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from oracle.synth import latent_blobs
    g = np.load(os.path.join(GOLDEN, 'gap_table_blobs.npz'))
    X, _ = latent_blobs(int(g['seed']), int(g['N']), int(g['D']), int(g['G']))
    assert str(X.dtype) == str(g['x_dtype'])
    cols = [str(c) for c in g['columns']]
    km = p2.KM(int(g['k_max']), str(tmp_path), cols[5:], int(g['n_init']), int(g['gap_b']))
    np.random.seed(int(g['np_seed']))
    df = km.compute_gap_internal_metric(X, int(g['k_max']), n_references=int(g['gap_b']), version=1).astype(float)
    pos = np.random.random()
    assert list(df.columns) == cols
    ref = g['table']
    assert pos == float(g['stream_pos']), 'the global stream was consumed differently'
    for j, c in enumerate(cols):
        np.testing.assert_allclose(df[c].to_numpy(), ref[:, j], rtol=1e-5, atol=1e-5 if c == 'gap' else 0, err_msg=c)   # gap = ref - act


def test_segment_sum_matches_numpy():
    """dic_segment_sum_f64 (the per-cluster f64 sums behind the centroid scores and the gap statistic's distance sums; round 6: no one-hot dgemm) against
    NumPy: matrices and vectors, labels in file order, an empty cluster, K in the second and third block of 64 clusters (one launch per block) and far past
    them, more clusters than rows, labels outside [0, K) (ignored); deterministic run to run."""
    from deep_interpolation_clustering_amd import cluster_stats
    rng = np.random.default_rng(3)
    for n, d, K, stray in ((75000, 256, 20, 0), (1001, 7, 3, 0), (64, 1, 2, 0), (5000, 256, 1, 0), (1000, 7, 65, 0), (1000, 65, 128, 0), (3000, 64, 129, 0),
                           (5000, 3, 1000, 0), (63, 1, 70, 0), (1000, 7, 130, 1)):
        lab = rng.integers(0, K, n)
        if K > 2:
            lab[lab == 1] = 0                                   # cluster 1 stays empty
        if stray:
            lab[::7] = rng.choice([-1, -64, K, K + 63, 1 << 32, (1 << 32) + 5], lab[::7].size)        # (the last two: inside [0, K) once truncated to 32 bits)
        v = rng.normal(size=(n, d))
        ref = np.zeros((K, d))
        inside = (lab >= 0) & (lab < K)
        np.add.at(ref, lab[inside], v[inside])
        vt, lt = torch.tensor(v, device='cuda'), torch.tensor(lab, device='cuda')
        got = cluster_stats._segment_sum(vt, lt, K)
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-12, atol=1e-10)
        assert torch.equal(got, cluster_stats._segment_sum(vt, lt, K))
        g1 = cluster_stats._segment_sum(vt[:, 0], lt, K)
        np.testing.assert_allclose(g1.cpu().numpy(), ref[:, 0], rtol=1e-12, atol=1e-10)


# ------------------------------------------------------------------------------------------------ every labelling the branches produce, against f64
# The inputs come from oracle/validity_cases.py; tests/test_cluster_stats_oracle.py shows on the CPU that a cluster index clamped to one 64-cluster block
# and the norm form's cancellation on tight clusters each move these figures by >= 10 x the bars below.  The bars: rtol 1e-5 on every index (the bar of
# test_scores_match_reference and test_validity_indices_match_sklearn), + atol 1e-6 on the silhouette as there, atol 1e-9 where the f64 value is exactly 0.
RTOL, SIL_ATOL, ZERO_ATOL = 1e-5, 1e-6, 1e-9
DEFAULT_METRICS = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']          # p2's --internal_metrics default
NAMES = {'Sihouette': 'silhouette', 'Davies-Bouldin_Index': 'davies_bouldin', 'Calinski-Harabasz': 'calinski_harabasz', 'Dunn_Index': 'dunn'}


def device_reference(x, lab):
    """CO.validity_indices in chunked torch f64 on the device, for sizes whose n x n x d differences the host oracle cannot hold."""
    lab, K = CO.encode(lab)
    order = np.argsort(lab, kind='stable')
    xs = torch.as_tensor(x[order], device='cuda', dtype=torch.float64)
    n, d = xs.shape
    seg = np.searchsorted(lab[order], np.arange(K + 1))
    ls = torch.as_tensor(lab[order], device='cuda')
    S = torch.empty((n, K), dtype=torch.float64, device='cuda')
    Dmin = torch.empty_like(S)
    own_max = torch.empty(n, dtype=torch.float64, device='cuda')
    step = max(64, min(2048, (1 << 28) // (n * d)))                      # a chunk of differences: at most 2 GiB
    for lo in range(0, n, step):
        dist = (xs[lo:lo + step, None, :] - xs[None, :, :]).square_().sum(-1).sqrt_()
        for c in range(K):
            S[lo:lo + step, c] = dist[:, seg[c]:seg[c + 1]].sum(1)
            Dmin[lo:lo + step, c] = dist[:, seg[c]:seg[c + 1]].min(1).values
        own_max[lo:lo + step] = torch.where(ls[lo:lo + step, None] == ls[None, :], dist, torch.zeros_like(dist)).max(1).values
    cnt = torch.as_tensor(np.diff(seg), device='cuda', dtype=torch.float64)
    rows = torch.arange(n, device='cuda')
    intra = S[rows, ls] / (cnt[ls] - 1)
    mean_to = S / cnt
    mean_to[rows, ls] = float('inf')
    inter = mean_to.min(1).values
    sil = torch.nan_to_num((inter - intra) / torch.maximum(intra, inter), nan=0.0)
    between = torch.stack([S[seg[c]:seg[c + 1]].sum(0) for c in range(K)])
    bmin = torch.stack([Dmin[seg[c]:seg[c + 1]].min(0).values for c in range(K)])
    off = bmin[~torch.eye(K, dtype=torch.bool, device='cuda')]
    totals = between.diagonal()
    samples = np.empty(n)
    samples[order] = sil.cpu().numpy()
    return {'silhouette': float(sil.mean()), 'silhouette_samples': samples, 'calinski_harabasz': CO.calinski_harabasz(x, lab), 'davies_bouldin': CO.davies_bouldin(x, lab),
            'dunn': float(off[off != 0].min() / own_max.max()), 'inertia_v1': float((totals / (cnt * cnt)).mean()), 'inertia_v2': float((totals / (2 * cnt)).sum()),
            'between': between.cpu().numpy()}


def check_indices(cs, tag, x, lab, ref):
    """Every index on its own and from the shared pair pass ``_cluster_cli.metric_values`` builds (with and without the Dunn index: the min / max pass and the
    sums-only pass), the two inertias from each, and the cluster-to-cluster sums of the sums-only pass, against ``ref``.  Returns the sums-only PairStats."""
    from deep_interpolation_clustering_amd._cluster_cli import INDICES, build_metrics, metric_values
    xd = torch.as_tensor(x, device='cuda')
    got = {}
    for name in INDICES:
        got[NAMES[name] + ' alone'] = build_metrics([name])[0](xd, lab)
    for names in (list(INDICES), DEFAULT_METRICS):
        for name, value in zip(names, metric_values(xd, lab, build_metrics(names))):
            got['%s shared by %d' % (NAMES[name], len(names))] = value
    full, sums = cs.pair_stats(xd, lab), cs.pair_stats(xd, lab, need_min=False, need_max=False)
    for how, st in (('alone', None), ('min / max pass', full), ('sums-only pass', sums)):
        got['inertia_v1 ' + how], got['inertia_v2 ' + how] = cs.inertia_v1(xd, lab, st), cs.inertia_v2(xd, lab, st)
    bad = []
    for key in sorted(got):
        want = ref[key.split(' ')[0]]
        atol = SIL_ATOL if key.startswith('silhouette') else ZERO_ATOL if want == 0 else 0.0
        err = abs(got[key] - want)
        print('%s %-36s %.10g f64 %.10g |diff| %.3g allowed %.3g' % (tag, key, got[key], want, err, RTOL * abs(want) + atol))
        if not err <= RTOL * abs(want) + atol:
            bad.append((key, got[key], want, err))
    # B[a][b] = sum_{i in a} S[i][b] of the sums-only pass: per entry, the diagonal (the own-cluster sums, which a row-maximum scale hides) included
    onehot = torch.nn.functional.one_hot(sums.labels, sums.K).double()
    B = (onehot.t() @ sums.S.double()).cpu().numpy()
    want = ref['between']
    err = np.abs(B - want)
    allowed = RTOL * np.abs(want) + np.where(want == 0, ZERO_ATOL, 0.0)
    worst = np.unravel_index(np.argmax(err - allowed), err.shape)
    print('%s between-cluster sums (%s): worst entry %s %.10g f64 %.10g |diff| %.3g allowed %.3g' % (tag, sums.route, worst, B[worst], want[worst], err[worst], allowed[worst]))
    if not (err <= allowed).all():
        bad.append(('between%s' % (worst,), B[worst], want[worst], err[worst]))
    samples = cs.silhouette_samples(xd, lab, sums).cpu().numpy()
    print('%s silhouette per sample (%s): largest deviation %.3g' % (tag, sums.route, np.abs(samples - ref['silhouette_samples']).max()))
    assert not bad, bad
    return sums


@pytest.mark.parametrize('name', list(VC.LABELLINGS) + ['%s%s' % (g, s) for g in VC.GEOMETRIES for s in ('', '+1000')])
def test_validity_indices_match_f64_on_every_labelling(cs, name):
    """Sihouette, CHIndex, DBIndex, DunnIndex, inertia_v1 and inertia_v2 against the f64 oracle on the labelling cases (K = 64, 65, 70, 129 with singletons,
    200, a noise class, label values with gaps, K = n - 1, widths 6 and 20) and on the K = 3 geometry cases at 1 500 points, plain and shifted by 1000."""
    if name in VC.LABELLINGS:
        x, lab = VC.labelling_case(name)
    else:
        x, lab = VC.geometry_case(name.split('+')[0], shifted=name.endswith('+1000'))
    check_indices(cs, name, x, lab, CO.validity_indices(x, lab))


@pytest.mark.parametrize('shifted', [False, True], ids=['plain', '+1000'])
@pytest.mark.parametrize('geometry', VC.GEOMETRIES)
@pytest.mark.parametrize('n,k,d', [(8200, 3, 16), (8200, 3, 256), (1200, 70, 16)])
def test_validity_indices_match_f64_from_the_size_of_the_matrix_core_pass(cs, n, k, d, geometry, shifted):
    """The same indices where the sums-only pass may go to the matrix cores (8 200 points >= ROWSUM_MIN_POINTS, K = 3, 16 and 256 wide) and at K = 70 (1 200
    points, centre spread 10), over the whole sweep of geometries and their shifted twins, against chunked f64 on the device.  No routing constant is patched:
    whatever takes the matrix-core pass holds the bars there (unit blobs do take it), and the hard geometries must have been sent to the difference form; the
    device's classification is NumPy's."""
    from oracle import pairtile_emulation as PE
    x, lab = VC.geometry_case(geometry, n=n, k=k, d=d, shifted=shifted)
    sums = check_indices(cs, '%s%s n=%d K=%d d=%d' % (geometry, '+1000' if shifted else '', n, k, d), x, lab, device_reference(x, lab))
    radius, sep, far = PE.geometry_ratios(x, lab)
    safe = radius >= cs.ROWSUM_SAFE_RATIO * far and sep >= cs.ROWSUM_SAFE_SEPARATION * far
    assert sums.route == ('rowsums' if n >= cs.ROWSUM_MIN_POINTS and safe else 'pairdist')
    if n >= cs.ROWSUM_MIN_POINTS:
        assert sums.route == {'unit': 'rowsums'}.get(geometry, 'pairdist')


def test_the_matrix_core_pass_is_kept_where_it_holds_the_bar(cs, rec):
    """The routing of the sums-only pass (cluster_stats.rowsum_is_safe): the labellings the pass has been measured on -- the blobs of the golden fixtures and
    of the recorded-bits cases, unit spread at 70 001 points, the BASELINE cfg2 shape -- are classified safe and, from ROWSUM_MIN_POINTS points on, do go
    through the matrix cores; the hard geometries do not, at the size of the pass.  One labelling the pass used to take is now refused: centre spread 10
    against cluster spread 1 has a radius ratio of 0.014, below ROWSUM_SAFE_RATIO = 0.046 (4 x the emulation's crossing, set by the own-cluster sums at rtol
    1e-5).  It takes the difference form; a test that forces the pass still gets it."""
    from oracle.synth import latent_blobs

    def safe(x, lab):
        lab, K = CO.encode(lab)
        order = np.argsort(lab, kind='stable')
        return cs.rowsum_is_safe(torch.as_tensor(x[order], device='cuda'), torch.as_tensor(lab[order], device='cuda'), torch.as_tensor(np.bincount(lab), device='cuda'))

    for name in CASES:
        g = np.load(os.path.join(GOLDEN, name))
        assert safe(g['x'], g['labels']), name
    for case in rec.ROWSUMS:
        assert safe(*rec.points(*case)), case
    rng = np.random.default_rng(70001 + 256 + 3)
    lab = rng.integers(0, 3, 70001)
    for spread, route in ((1.0, 'rowsums'), (10.0, 'pairdist')):
        x = (rng.normal(0, 1, (70001, 256)) + spread * rng.normal(0, 1, (3, 256))[lab]).astype(np.float32)
        assert cs.pair_stats(x, lab, need_min=False, need_max=False).route == route, spread
    x, lab = latent_blobs(11, 75000, 256, 4)
    assert cs.pair_stats(x, lab, need_min=False, need_max=False).route == 'rowsums'
    assert cs.pair_stats(x, lab).route == 'pairdist' and cs.pair_stats(x[:5000], lab[:5000], need_min=False, need_max=False).route == 'pairdist'
    for geometry in VC.HARD:
        for shifted in (False, True):
            x, lab = VC.geometry_case(geometry, n=8200, shifted=shifted)
            assert not safe(x, lab) and cs.pair_stats(x, lab, need_min=False, need_max=False).route == 'pairdist', (geometry, shifted)


def test_too_few_and_too_many_clusters_raise_before_any_kernel(cs, monkeypatch):
    """scikit-learn's ValueError for one cluster and for as many clusters as points comes from the label count alone: no library call is made."""
    from deep_interpolation_clustering_amd.internal_eval import CHIndex, DBIndex, Sihouette
    x = torch.as_tensor(np.random.default_rng(0).normal(size=(200, 8)).astype(np.float32), device='cuda')

    def no_kernel():
        raise AssertionError('a kernel was asked for')
    monkeypatch.setattr(cs.N, 'lib', no_kernel)
    for lab in (np.zeros(200, dtype=np.int64), np.arange(200)):
        for index in (Sihouette(), CHIndex(), DBIndex()):
            with pytest.raises(ValueError, match='Number of labels is %d' % len(np.unique(lab))):
                index(x, lab)


def test_p2_meanshift_branch_past_64_clusters(tmp_path):
    """p2's Meanshift branch picks K itself: 70 tight blobs in a 600-point cohort give 70 clusters, and the default --internal_metrics of the table are the
    f64 oracle's on the branch's own labels."""
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    rng = np.random.default_rng(70)
    cen = rng.normal(0, 3.0, (70, 8))
    comp = np.concatenate([np.arange(70), rng.integers(0, 70, 530)])
    x = (cen[comp] + rng.normal(0, 0.05, (600, 8))).astype(np.float32)
    valid = (cen[rng.integers(0, 70, 100)] + rng.normal(0, 0.05, (100, 8))).astype(np.float32)
    args = p2.get_arguments(['--cluster_method', 'meanshift', '--meanshift_bandwidth', '1.0'])
    assert args.internal_metrics == DEFAULT_METRICS
    ms = p2.Meanshift(str(tmp_path), args.internal_metrics, args.meanshift_quantile, args.meanshift_bandwidth)
    table = ms.train({'hidden': x}, {'hidden': valid})
    labels = ms.fits_[0].labels_
    assert table.n_clusters[0] == 70 and table.n_orphans[0] == 0 and len(np.unique(labels)) == 70
    assert all(len(np.unique(comp[labels == c])) == 1 for c in range(70))          # one blob per cluster
    ref = CO.validity_indices(x, labels)
    for name in DEFAULT_METRICS:
        print(name, table[name][0], ref[NAMES[name]])
        np.testing.assert_allclose(table[name][0], ref[NAMES[name]], rtol=RTOL, atol=SIL_ATOL if name == 'Sihouette' else 0, err_msg=name)
