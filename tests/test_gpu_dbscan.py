"""DBSCAN on the GPU (dbscan.py, csrc/dic_dbscan.hip) against sklearn's fit on the precomputed distance matrix -- the path upstream takes
(p2_clustering_optK.py:82-85,90-168, p4_clustering_final.py:181-236).  Labels and core indices must be identical."""
import functools
import os

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import cluster_stats
from deep_interpolation_clustering_amd.dbscan import DBSCAN, _Counts, _device_points, dbscan_sweep, sq_threshold
from deep_interpolation_clustering_amd.info import COHORTS

pytestmark = pytest.mark.gpu

sk_cluster = pytest.importorskip('sklearn.cluster')
sk_metrics = pytest.importorskip('sklearn.metrics')


def sk_dbscan(X, eps, min_samples):
    db = sk_cluster.DBSCAN(eps, min_samples=min_samples, metric='precomputed').fit(sk_metrics.pairwise_distances(X))
    return db.labels_.astype(np.int64), db.core_sample_indices_.astype(np.int64)


def audit(X, eps_values, rel=1e-6):
    """No pair's f64 distance lies within ``rel`` of any eps (so that the reference's own rounding cannot decide a test)."""
    X = X.astype(np.float64)
    sq = (X ** 2).sum(1)
    for s in range(0, len(X), 2048):
        d = np.sqrt(np.maximum(sq[s:s + 2048, None] + sq[None, :] - 2.0 * X[s:s + 2048] @ X.T, 0.0))
        for e in eps_values:
            assert not np.any(np.abs(d - float(e)) <= rel * float(e)), 'a pair at distance ~ eps %r' % (e,)


def check(X, eps, min_samples, **kw):
    db = DBSCAN(eps, min_samples, **kw).fit(X)
    lab, core = sk_dbscan(X, eps, min_samples)
    np.testing.assert_array_equal(db.core_sample_indices_, core)
    np.testing.assert_array_equal(db.labels_, lab)
    np.testing.assert_array_equal(db.components_, X[core])
    return db


def blobs(n, d, k, spread, noise_frac, seed, box=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (k, d)) * (box or 4.0)
    m = int(n * (1 - noise_frac))
    X = centres[rng.integers(0, k, m)] + rng.normal(0, spread, (m, d))
    lo, hi = centres.min(0) - 1, centres.max(0) + 1
    noise = rng.uniform(lo, hi, (n - m, d))
    return rng.permutation(np.concatenate([X, noise])).astype(np.float32)


@pytest.mark.parametrize('d,eps,ms', [(256, 2.5, 10), (8, 0.55, 5)])
def test_blobs_with_noise(d, eps, ms):
    X = blobs(3000, d, 6, 0.1 if d == 256 else 0.15, 0.1, seed=d)
    audit(X, [eps])
    db = check(X, eps, ms)
    assert len(set(db.labels_)) > 3 and (db.labels_ == -1).any()


def test_chains_need_many_passes():
    rng = np.random.default_rng(3)
    parts = []
    for c in range(3):
        t = np.arange(700)[:, None] * 0.1
        base = np.zeros((700, 16))
        base[:, 0] = t[:, 0]
        base[:, 1] = 5.0 * c + 0.3 * np.sin(t[:, 0])
        parts.append(base + rng.normal(0, 0.003, base.shape))
    X = rng.permutation(np.concatenate(parts)).astype(np.float32)
    audit(X, [0.15])
    stats = {}
    (lab, core), = dbscan_sweep(X, [0.15], 2, stats=stats)
    ref_lab, ref_core = sk_dbscan(X, 0.15, 2)
    np.testing.assert_array_equal(core, ref_core)
    np.testing.assert_array_equal(lab, ref_lab)
    assert len(set(lab)) == 3
    assert stats['components_passes'][0] >= 3


def test_border_point_of_two_clusters_takes_smallest_id():
    # two dense lines, a non-core point between them within eps of a core point of each; the second cluster is found first in index order
    # (min_samples 10: the middle points of each line are core, the bridge point has 4 + 4 + 1 neighbours and is not)
    a = np.stack([np.arange(10) * 0.1, np.zeros(10)], 1)
    b = np.stack([np.arange(10) * 0.1, np.full(10, 1.0)], 1)
    mid = np.array([[0.45, 0.5]])
    X = np.concatenate([b, a, mid, [[20.0, 20.0]]]).astype(np.float32)
    X = np.concatenate([X, np.zeros((len(X), 2), np.float32)], 1)
    eps = 0.55
    audit(X, [eps])
    db = check(X, eps, 10)
    assert db.labels_[-2] == 0 and db.labels_[15] == 1 and db.labels_[5] == 0 and db.labels_[-1] == -1
    assert 20 not in db.core_sample_indices_


def test_duplicates_and_min_samples_one():
    rng = np.random.default_rng(5)
    base = rng.normal(0, 1, (400, 12)).astype(np.float32)
    X = np.concatenate([base, base[:150], base[:40]])
    X = X[rng.permutation(len(X))]
    for eps, ms in [(1.3, 3), (1.3, 1), (0.05, 1)]:
        check(X, eps, ms)


def test_everything_noise_and_one_cluster():
    X = blobs(1500, 32, 3, 0.2, 0.0, seed=9, box=1.0)
    db = check(X, 1e-3, 2)
    assert (db.labels_ == -1).all() and len(db.core_sample_indices_) == 0
    db = check(X, 1e3, 5)
    assert (db.labels_ == 0).all()


def test_reference_settings_latents():
    # p1-like latents: 12 000 x 256, clusters of two widths (pair distances ~1.13 and ~2.0) plus a diffuse background, min_samples = 257 (p2: feat_dim
    # + 1), eps from p2's range (np.float64, as p2 passes them) between the distance bulks, so that the audit holds
    rng = np.random.default_rng(21)
    k = 8
    centres = rng.normal(0, 0.35, (k, 256))
    sizes = rng.multinomial(11000, np.full(k, 1 / k))
    widths = np.array([0.05, 0.088] * 4)
    X = np.concatenate([centres[c] + rng.normal(0, widths[c], (s, 256)) for c, s in enumerate(sizes)] + [rng.normal(0, 0.45, (1000, 256))])
    X = rng.permutation(X).astype(np.float32)
    eps_range = np.arange(.5, 5.1, .5)
    eps_list = [eps_range[2], eps_range[4], eps_range[6]]          # 1.5, 2.5, 3.5
    audit(X, eps_list)
    fits = dbscan_sweep(X, eps_list, 257)
    for e, (lab, core) in zip(eps_list, fits):
        ref_lab, ref_core = sk_dbscan(X, e, 257)
        np.testing.assert_array_equal(core, ref_core)
        np.testing.assert_array_equal(lab, ref_lab)
    assert any(len(set(l)) > 2 for l, _ in fits)


def test_lattice_ties_and_eps_types():
    # integer lattice, eps = spacing: every lattice neighbour sits exactly on eps
    g = np.arange(7, dtype=np.float32)
    X = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    X = np.concatenate([X, np.zeros((len(X), 1), np.float32)], 1)
    stats = {}
    (lab, core), = dbscan_sweep(X, [1.0], 5, stats=stats)
    ref_lab, ref_core = sk_dbscan(X, 1.0, 5)
    np.testing.assert_array_equal(core, ref_core)
    np.testing.assert_array_equal(lab, ref_lab)
    assert stats['band_pairs'][0] > 0
    # spacing f32(0.3): a float eps 0.3 compares in f32 (f32(0.3) <= 0.3 holds), an np.float64 0.3 in f64 (it does not)
    s = np.float32(0.3)
    v = np.array([-s, 0, s], np.float32)
    Y = np.stack(np.meshgrid(v, v, v, v, indexing='ij'), -1).reshape(-1, 4).astype(np.float32)
    assert np.sqrt(np.float32(s * s)) <= 0.3 and not np.sqrt(np.float32(s * s)) <= np.float64(0.3)
    assert sq_threshold(0.3) != sq_threshold(np.float64(0.3))
    outs = []
    for eps in (0.3, np.float64(0.3)):
        stats = {}
        (lab, core), = dbscan_sweep(Y, [eps], 3, stats=stats)
        ref_lab, ref_core = sk_dbscan(Y, eps, 3)
        np.testing.assert_array_equal(core, ref_core)
        np.testing.assert_array_equal(lab, ref_lab)
        assert stats['band_pairs'][0] > 0
        outs.append(len(core))
    assert outs[0] == len(Y) and outs[1] == 0


def test_band_overflow_reruns_exactly():
    X = blobs(2500, 16, 4, 0.2, 0.1, seed=13)
    eps = 0.8
    audit(X, [eps])
    ref = DBSCAN(eps, 6).fit(X)
    assert sum(ref.stats_['band_pairs']) > 1
    tiny = DBSCAN(eps, 6, band_capacity=1).fit(X)
    assert tiny.stats_['counts_reruns'] == 1
    np.testing.assert_array_equal(tiny.labels_, ref.labels_)
    np.testing.assert_array_equal(tiny.core_sample_indices_, ref.core_sample_indices_)
    lab, core = sk_dbscan(X, eps, 6)
    np.testing.assert_array_equal(ref.labels_, lab)
    # the C entry point itself reports the overflow
    L = N.lib()
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    ws = torch.empty(L.dic_dbscan_workspace(n, d), dtype=torch.uint8, device='cuda')
    counts = torch.empty((1, n), dtype=torch.int32, device='cuda')
    band = torch.empty((1, 4), dtype=torch.int32, device='cuda')
    centre = x.mean(0, keepdim=True)
    nb = N.C.c_int64(0)
    thr = (N.C.c_float * 1)(sq_threshold(eps))
    rc = L.dic_dbscan_counts(N.ptr(x), d, N.ptr(centre), n, d, thr, 1, N.ptr(counts), N.ptr(band), 1, N.C.byref(nb), N.ptr(ws), ws.numel(), N.stream_of(x))
    assert rc == -3 and nb.value > 1


@functools.lru_cache(maxsize=None)
def centred_points(n):
    """(X (n, 8) f32, exact f64 squared distances (n, n)): 40 points at the origin, the others on the 2^-12 grid at radius 0.2 .. 0.99 as +- pairs and one
    triple a, b, -(a + b), shuffled, a point of the origin last.  Every coordinate sum is exactly 0, so the centre the kernel gets is the origin itself and the
    zero vector -- which is also what a padding point holds -- is a real point; on the grid the f64 squared distances are exact."""
    rng = np.random.default_rng(2 + n)          # (a seed at which the audit below holds for every case)
    m = (n - 40 - 3) // 2
    assert 40 + 3 + 2 * m == n
    v = rng.normal(0, 1, (m + 2, 8))
    v = np.round(v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.2, 0.99, (m + 2, 1)) * 0.5 * 4096) / 4096
    a, b, half = v[0], v[1], v[2:]
    rest = rng.permutation(np.concatenate([2 * half, -2 * half, [a, b, -(a + b)], np.zeros((39, 8))]))
    X = np.concatenate([rest, np.zeros((1, 8))])
    assert X.shape == (n, 8) and not X.sum(0).any() and np.linalg.norm(X, axis=1).max() <= 1.0 and (X.astype(np.float32) == X).all()
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    d2.setflags(write=False)
    return X.astype(np.float32), d2


def brute_dbscan(d2, eps, min_samples):
    """sklearn's _dbscan_inner on the neighbour rule f32(d^2) <= sq_threshold(eps): (neighbour counts, labels, core indices)."""
    nb = d2.astype(np.float32) <= np.float32(sq_threshold(eps))
    counts = nb.sum(1)
    core = counts >= min_samples
    lab = np.full(len(d2), -1, np.int64)
    cid = 0
    for i in np.flatnonzero(core):
        if lab[i] >= 0:
            continue
        lab[i] = cid
        stack = [i]
        while stack:
            for q in np.flatnonzero(nb[stack.pop()] & (lab < 0)):
                lab[q] = cid
                if core[q]:
                    stack.append(q)
        cid += 1
    return counts, lab, np.flatnonzero(core).astype(np.int64)


def padding_eps(n_eps):
    """n_eps values from 1e-3, which isolates every point that has no duplicate, to 1e6, which makes every pair a neighbour (alone: the latter)."""
    return [1e6] if n_eps == 1 else [1e-3] + [float(e) for e in np.linspace(0.25, 1.0, n_eps - 2)] + [1e6]


# 257: two row blocks, 255 padding points in the last one; 513: the last point alone in its row block.  D = 8: zero-padded columns.
@pytest.mark.parametrize('n,n_eps', [(257, 1), (257, 4), (257, 10), (257, 16), (513, 10)])
def test_padding_points_are_never_neighbours(n, n_eps):
    X, d2 = centred_points(n)
    eps = padding_eps(n_eps)
    audit(X, eps)
    ref = [brute_dbscan(d2, e, 5) for e in eps]
    assert (ref[-1][0] == n).all() and (n_eps == 1 or (ref[0][0][np.any(X != 0, axis=1)] == 1).all())
    fits = dbscan_sweep(X, eps, 5)
    for (_, ref_lab, ref_core), (lab, core) in zip(ref, fits):
        np.testing.assert_array_equal(core, ref_core)
        np.testing.assert_array_equal(lab, ref_lab)
    counts = _Counts(_device_points(X), [sq_threshold(e) for e in eps]).counts.cpu().numpy()
    assert (counts[-1] == n).all()
    np.testing.assert_array_equal(counts, np.stack([c for c, _, _ in ref]))


def test_sweep_equals_fits_and_repeats():
    X = blobs(2000, 24, 5, 0.2, 0.15, seed=17)
    eps_list = [0.7, 0.9, 1.0, 1.8]
    audit(X, eps_list)
    a = dbscan_sweep(X, eps_list, 4)
    b = dbscan_sweep(X, eps_list, 4)
    for e, (la, ca), (lb, cb) in zip(eps_list, a, b):
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ca, cb)
        db = DBSCAN(e, 4).fit(X)
        np.testing.assert_array_equal(db.labels_, la)
        np.testing.assert_array_equal(db.core_sample_indices_, ca)
        lab, core = sk_dbscan(X, e, 4)
        np.testing.assert_array_equal(la, lab)


@pytest.mark.parametrize('n,k', [(3000, 80), (20000, 300)])
def test_silhouette_more_than_64_clusters(n, k):
    rng = np.random.default_rng(n)
    X = rng.normal(0, 1, (n, 16)).astype(np.float32)
    lab = rng.integers(-1, k - 1, n)
    X += (lab[:, None] % 7) * 0.5
    got = cluster_stats.silhouette_score(X, lab)
    ref = sk_metrics.silhouette_score(X, lab)
    assert abs(got - ref) <= 1e-5, (got, ref)


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


def test_p2_dbscan_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    audit(data['training']['hidden'], list(np.arange(.5, 5.1, .5)))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'dbscan'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    df = res['ae_mse']
    csv = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_dbscan_aligned' / 'plot' / 'dbscan_eps.csv'
    assert csv.exists()
    X = data['training']['hidden']
    eps_range = np.arange(.5, 5.1, .5)
    D = sk_metrics.pairwise_distances(X)
    assert len(df) == len(eps_range)
    for row, eps in zip(df.itertuples(), eps_range):
        db = sk_cluster.DBSCAN(eps, min_samples=X.shape[1] + 1, metric='precomputed').fit(D)
        lab = db.labels_
        ncl = len(set(lab)) - (1 if -1 in lab else 0)
        assert (row.n_core, row.n_clusters, row.n_noise) == (len(db.core_sample_indices_), ncl, int((lab == -1).sum()))
        if ncl > 1:
            keep = lab != -1
            assert abs(row.silhouette - sk_metrics.silhouette_score(X, lab)) <= 1e-5
            assert abs(row.denoise_silhouette - sk_metrics.silhouette_score(X[keep], lab[keep])) <= 1e-5
        else:
            assert np.isnan(row.silhouette)
    assert (df.n_clusters > 1).any()


def _align_train(lab, ob, pad, feat):
    lab = lab.copy()
    pad0 = pad[:, 0, :]
    per_enc = np.sum(ob[:, 0, :] * pad0, axis=1) / np.sum(pad0, axis=1)
    k = len(set(lab)) - (1 if -1 in lab else 0)
    members = [np.where(lab == i) for i in range(k)]
    order = np.argsort([np.average(per_enc[m]) for m in members])[::-1]
    amap = {int(prev): cur for cur, prev in enumerate(order)}
    for old, new in amap.items():
        lab[members[old]] = new
    return lab, [np.mean(feat[lab == i], axis=0) for i in range(k)]


def _align_center(feat, lab, centres):
    lab = lab.copy()
    k = len(set(lab)) - (1 if -1 in lab else 0)
    oc = [np.mean(feat[lab == i], axis=0) for i in range(k)]
    idx = np.argmin(sk_metrics.pairwise_distances(oc, centres), axis=1)
    assert len(set(idx)) == k
    members = [np.where(lab == i) for i in range(k)]
    for o, nw in enumerate(idx):
        lab[members[o]] = nw
    return lab


def test_p4_dbscan_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 37)
    for cohort in data.values():
        audit(cohort['hidden'], [1.5])
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'dbscan', '--opt_eps', '1.5'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    outdir = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_dbscan_aligned'
    centres = None
    for cohort in COHORTS:
        d = data[cohort]
        X = d['hidden']
        lab = sk_cluster.DBSCAN(1.5, min_samples=X.shape[1], metric='precomputed').fit(sk_metrics.pairwise_distances(X)).labels_
        if cohort == 'training':
            ref, centres = _align_train(lab, d['ob'], d['padding_mask'], X)
        else:
            ref = _align_center(X, lab, centres)
        got = np.load(outdir / '{}_eps-1.5.npy'.format(cohort), allow_pickle=True).item()
        assert 'ob' not in got and 'padding_mask' not in got
        np.testing.assert_array_equal(got['cluster_id'], ref)
    assert len(set(ref)) >= 3
