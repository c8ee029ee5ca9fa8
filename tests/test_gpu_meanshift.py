"""Mean shift on the GPU (csrc/dic_meanshift.hip, meanshift.py, the p2 / p4 meanshift branches) against the numpy f64 yardstick of
tests/test_meanshift_host.py and sklearn.

Member sets, counts, iteration counts and labels are demanded EQUAL: test_meanshift_host.py::test_conditions_of_the_cases keeps every comparison of every
case 1e-9 (relative) away from its threshold, four orders above the f64 summation-order noise.  With equal member sets a centre is one f64 mean of at most N
terms of magnitude <= R = max |x'| on either side: the coordinates may differ by 2 * (N 2^-53 R) for the two sums plus the roundings of the division and of
the addition of c (2^-53 R each), inside the 4 N 2^-53 R allowed."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import meanshift as M
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.meanshift import MeanShift, estimate_bandwidth, mean_shift_sweep
from test_gpu_optics import _write_latents
from test_meanshift_host import GAP, VARIANT_IDS, VARIANTS, blobs, case, reference, y_estimate_bandwidth

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def spread_of(X):
    X = np.asarray(X, dtype=np.float64)
    return float(np.abs(X - X.mean(axis=0)).max())


def unpack(mask, n):
    """(M, words) int32 device mask -> ((M, n) bool members, (M, tail) bool bits past the last point)."""
    words = mask.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder='little').astype(bool)
    return bits[:, :n], bits[:, n:]


def pack(member):
    m, n = member.shape
    words = (n + 31) // 32
    bits = np.zeros((m, words * 32), dtype=np.uint8)
    bits[:, :n] = member
    return np.packbits(bits, axis=1, bitorder='little').view(np.uint32).view(np.int32).reshape(m, words)


def device_members(X, seeds, h, capacity):
    """One dic_meanshift_members call: (status, band pairs reported, members, tail bits)."""
    pts = M._Points(X)
    s = pts.rows64(seeds, 'seeds')
    m = s.shape[0]
    ws = pts.workspace(m, 0)
    mask = torch.full((m, pts.words), -1, dtype=torch.int32, device=s.device)          # (every word must be overwritten)
    band = torch.empty((max(capacity, 1), 4), dtype=torch.int32, device=s.device)
    nb = ctypes.c_int64(-1)
    rc = N.lib().dic_meanshift_members(N.ptr(pts.x), pts.x.stride(0), pts.n, pts.d, N.ptr(pts.centre), N.ptr(s), m, m, float(h), N.ptr(mask), N.ptr(band),
                                       capacity, ctypes.byref(nb), N.ptr(ws), ws.numel(), N.stream_of(s))
    torch.cuda.synchronize()
    return (rc, int(nb.value)) + unpack(mask, pts.n)


# ----------------------------------------------------------------------------------------------------------------------------------- ABI: members
def test_members_on_the_lattice_with_pairs_at_exactly_the_bandwidth_and_the_band_protocol():
    c = case('lattice')
    X = c['X']
    far = np.array([[1e3, 0, 0, 0], [-50, -50, -50, -50], [3, 3, 3, 40]], dtype=np.float64)
    seeds = np.concatenate([X.astype(np.float64), far])
    d2 = ((seeds[:, None, :] - X[None, :, :].astype(np.float64)) ** 2).sum(-1)          # small integers: exact
    want = d2 <= c['h'] ** 2
    assert (d2 == 4.0).sum() > 1000 and not want[len(X):].any()
    rc, nb, got, tail = device_members(X, seeds, c['h'], 1)                       # a band list that is too small: the needed size comes back
    assert rc == -3 and nb >= (d2 == 4.0).sum() and b'capacity' in N.lib().dic_last_error_string()
    rc, nb2, got, tail = device_members(X, seeds, c['h'], nb)
    assert rc == 0 and nb2 == nb
    assert np.array_equal(got, want)
    assert tail.shape[1] == 20 and not tail.any()


@pytest.mark.parametrize('name', ['seeds_m257', 'n257_d8', 'n600_d256'])
def test_members_equal_the_yardstick(name):
    c, r = case(name), reference(name)
    seeds = c['kw'].get('seeds', c['X'].astype(np.float64))
    rc, nb, got, tail = device_members(c['X'], seeds, c['h'], 1 << 16)
    assert rc == 0 and nb >= 0
    assert np.array_equal(got, r.first_members)
    assert not tail.any()
    if name == 'seeds_m257':
        assert (~got.any(axis=1)).sum() >= 10          # the far seeds: rows of zeros


# ------------------------------------------------------------------------------------------------------------------------------------- ABI: shift
@pytest.mark.parametrize('m,n,d', [(17, 257, 8), (257, 1000, 256), (257, 257, 20), (17, 1000, 64)])
def test_shift_kernel_against_torch_f64(m, n, d):
    """The first f64 MFMA of the repository, at the ABI: a random 0/1 mask against ``mask.double() @ (X.double() - c)`` in torch f64 on the host.  Either side
    adds at most N terms of magnitude <= max |x'|, N roundings: 2 N 2^-53 max|x'| per coordinate, doubled for the two sides.  D = 8, 20 / 64 and 256 take the
    kernel's three accumulator widths."""
    rs = np.random.RandomState(m + n + d)
    X = (rs.normal(size=(n, d)) * 3 + rs.normal(size=d) * 10).astype(np.float32)
    member = rs.rand(m, n) < 0.05 + rs.rand(m, 1) * 0.55
    member[[0, m // 2, m - 1]] = False                                             # rows without a member
    member[1] = True
    seeds = rs.normal(size=(m, d)) * 3
    frozen = [2, m - 2]                                                            # done before the call: left alone
    dev = torch.device('cuda')
    x = torch.as_tensor(X, device=dev)
    c = x.double().mean(dim=0).contiguous()
    want = torch.as_tensor(member).double() @ (torch.as_tensor(X).double() - c.cpu())
    bound = 2 * (2 * n * U * float((torch.as_tensor(X).double() - c.cpu()).abs().max()))
    mask = torch.as_tensor(pack(member), device=dev)
    outs = []
    for _ in range(2):
        s = torch.as_tensor(seeds, device=dev).contiguous()
        counts = torch.full((m,), -7, dtype=torch.int32, device=dev)
        iters = torch.zeros(m, dtype=torch.int32, device=dev)
        done = torch.zeros(m, dtype=torch.int32, device=dev)
        done[frozen] = 1
        sums = torch.full((m, d), float('nan'), dtype=torch.float64, device=dev)
        N.check(N.lib().dic_meanshift_shift(N.ptr(x), x.stride(0), n, d, N.ptr(c), N.ptr(mask), m, N.ptr(s), 1.0, 300, N.ptr(counts), N.ptr(iters), N.ptr(done),
                                            N.ptr(sums), N.stream_of(x)), 'dic_meanshift_shift')
        outs.append([t.cpu().numpy() for t in (s, counts, iters, done, sums)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)                                # two calls: identical bits
    s, counts, iters, done, sums = outs[0]
    live = np.setdiff1d(np.arange(m), frozen)
    cnt = member.sum(axis=1)
    err = np.abs(sums[live] - want.numpy()[live]).max()
    print('shift', (m, n, d), 'largest deviation of a sum', err, 'allowed', bound)
    assert err <= bound
    assert np.array_equal(counts[live], cnt[live])
    empty = live[cnt[live] == 0]
    full = live[cnt[live] > 0]
    assert len(empty) == 3 and np.array_equal(s[empty], seeds[empty]) and (done[empty] == 1).all() and (iters[empty] == 0).all()
    assert np.array_equal(s[full], c.cpu().numpy() + sums[full] / cnt[full, None])          # the rule, from the kernel's own sums: bit for bit
    assert (done[full] == 0).all() and (iters[full] == 1).all()                    # (they moved far: not finished)
    assert np.array_equal(s[frozen], seeds[frozen]) and (counts[frozen] == -7).all() and (iters[frozen] == 0).all() and np.isnan(sums[frozen]).all()


def test_shift_stops_by_the_rule():
    """moved <= 1e-3 h finishes a seed without counting the iteration; so does a seed that has completed max_iter iterations."""
    X = case('n255_d8')['X']
    n, d = X.shape
    dev = torch.device('cuda')
    x = torch.as_tensor(X, device=dev)
    c = x.double().mean(dim=0).contiguous()
    member = np.zeros((3, n), dtype=bool)
    member[:, :40] = True
    mean = X[:40].astype(np.float64).mean(axis=0)
    seeds = np.stack([mean + 1e-7, mean + 1.0, mean + 1.0])
    s = torch.as_tensor(seeds, device=dev).contiguous()
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    iters = torch.as_tensor(np.array([0, 4, 5], dtype=np.int32), device=dev)
    done = torch.zeros(3, dtype=torch.int32, device=dev)
    mask = torch.as_tensor(pack(member), device=dev)
    N.check(N.lib().dic_meanshift_shift(N.ptr(x), x.stride(0), n, d, N.ptr(c), N.ptr(mask), 3, N.ptr(s), 1.0, 5, N.ptr(counts), N.ptr(iters), N.ptr(done), None,
                                        N.stream_of(x)), 'dic_meanshift_shift')
    assert done.cpu().tolist() == [1, 0, 1] and iters.cpu().tolist() == [0, 5, 5] and counts.cpu().tolist() == [40, 40, 40]
    assert np.abs(s.cpu().numpy() - mean).max() <= 4 * 40 * U * spread_of(X)


# ---------------------------------------------------------------------------------------------------------------------- estimator against the yardstick
@functools.lru_cache(maxsize=None)
def device_fit(name, kw=()):
    c = case(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return MeanShift(bandwidth=c['h'], **{**c['kw'], **dict(kw)}).fit(np.array(c['X']))


def assert_same_fit(fit, r, X):
    tol = 4 * len(X) * U * spread_of(X)
    assert fit.cluster_centers_.shape == r.centres.shape and fit.cluster_centers_.dtype == np.float64
    assert np.array_equal(fit.seed_counts_, r.seed_counts)
    assert np.array_equal(fit.seed_iterations_, r.seed_iterations)
    assert fit.n_iter_ == r.n_iter
    assert np.array_equal(fit.labels_, r.labels)
    err = np.abs(fit.cluster_centers_ - r.centres).max()
    print('largest deviation of a centre coordinate', err, 'allowed', tol)
    assert err <= tol


@pytest.mark.parametrize('name,kw', VARIANTS, ids=VARIANT_IDS)
def test_estimator_equals_the_yardstick(name, kw):
    fit = device_fit(name, kw)
    assert_same_fit(fit, reference(name, kw), case(name)['X'])
    assert fit.bandwidth_ == case(name)['h'] and fit.n_features_in_ == case(name)['X'].shape[1]


@pytest.mark.parametrize('name', ['n600_d256', 'n1000_d4'])
def test_estimator_equals_sklearn(name):
    cluster = pytest.importorskip('sklearn.cluster')
    c = case(name)
    fit = device_fit(name)
    sk = cluster.MeanShift(bandwidth=c['h']).fit(c['X'].astype(np.float64))
    assert np.array_equal(sk.labels_, fit.labels_) and sk.n_iter_ == fit.n_iter_
    assert np.abs(sk.cluster_centers_ - fit.cluster_centers_).max() <= 4 * len(c['X']) * U * spread_of(c['X'])


# --------------------------------------------------------------------------------------------------------------------------------------- plumbing
def same_bits(a, b):
    return (np.array_equal(a.cluster_centers_, b.cluster_centers_) and np.array_equal(a.labels_, b.labels_) and np.array_equal(a.seed_counts_, b.seed_counts_)
            and np.array_equal(a.seed_iterations_, b.seed_iterations_) and np.array_equal(a.seed_positions_, b.seed_positions_))


def test_results_do_not_depend_on_the_mask_budget():
    c = case('n1000_d4')
    small = MeanShift(bandwidth=c['h'], mask_budget=1).fit(np.array(c['X']))
    assert small.stats_['groups'] >= 3 and device_fit('n1000_d4').stats_['groups'] == 1
    assert same_bits(small, device_fit('n1000_d4'))


def test_device_tensor_strided_view_and_two_fits_give_identical_bits():
    c = case('n257_d8')
    ref = device_fit('n257_d8')
    X = np.array(c['X'])
    assert same_bits(MeanShift(bandwidth=c['h']).fit(X), ref)                                                     # two fits
    assert same_bits(MeanShift(bandwidth=c['h']).fit(torch.as_tensor(X, device='cuda')), ref)                    # a device tensor
    wide = torch.zeros((len(X), 16), dtype=torch.float32, device='cuda')
    wide[:, :8] = torch.as_tensor(X)
    wide[:, 8:] = 7.0
    view = wide[:, :8]
    from deep_interpolation_clustering_amd.ward import _usable_view
    assert _usable_view(view) and not view.is_contiguous()
    assert same_bits(MeanShift(bandwidth=c['h']).fit(view), ref)                                                 # read where it lies


def test_predict_sweep_and_bandwidth():
    c = case('n300_d5')
    fit = device_fit('n300_d5')
    other = blobs(333, 5, 3, 3, 4.0)[100:] + np.float32(0.5)
    d2 = ((other[:, None, :].astype(np.float64) - reference('n300_d5').centres[None]) ** 2).sum(-1)
    srt = np.sort(d2, axis=1)
    assert ((srt[:, 1] - srt[:, 0]) / srt[:, 1]).min() >= GAP                      # (the condition that makes equality fair)
    assert np.array_equal(fit.predict(other), d2.argmin(axis=1))
    assert np.array_equal(fit.predict(torch.as_tensor(other, device='cuda')), d2.argmin(axis=1))
    orphans = fit.predict(other, orphans=True)
    assert np.array_equal(orphans, np.where(d2.min(axis=1) > c['h'] ** 2, -1, d2.argmin(axis=1)))
    hs = [c['h'], 1.3 * c['h']]
    sweep = mean_shift_sweep(np.array(c['X']), hs)
    assert sorted(sweep) == sorted(hs)
    for h in hs:
        assert same_bits(sweep[h], MeanShift(bandwidth=h).fit(np.array(c['X'])))
    for name, q in (('n300_d5', 0.2), ('n600_d256', 0.3), ('n2_d4', 0.3)):
        want = y_estimate_bandwidth(case(name)['X'], q)
        assert abs(estimate_bandwidth(np.array(case(name)['X']), q) - want) <= 1e-13 * want
    auto = MeanShift().fit(np.array(c['X']))                                      # bandwidth=None: the quantile-0.3 estimate
    assert abs(auto.bandwidth_ - y_estimate_bandwidth(c['X'], 0.3)) <= 1e-13 * auto.bandwidth_


def test_errors_on_the_device(monkeypatch):
    X = np.array(case('n255_d8')['X'])
    with pytest.raises(ValueError, match='No point was within bandwidth=0.500000 of any seed'):
        MeanShift(bandwidth=0.5, seeds=np.full((3, 8), 1e4)).fit(X)
    with pytest.raises(ValueError, match=r'seeds must be of shape \(n, 8\)'):
        MeanShift(bandwidth=0.5, seeds=np.zeros((3, 7))).fit(X)
    with pytest.raises(ValueError, match='expecting 8 features'):
        device_fit('n255_d8').predict(np.zeros((4, 5), np.float32))
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **kw: (1000, 1 << 30))
    with pytest.raises(MemoryError, match=r'255 points with 255 seeds per pass needs (\d+) bytes on the device, 1000 are free') as err:
        MeanShift(bandwidth=4.0).fit(X)
    assert int(str(err.value).split('needs ')[1].split(' bytes')[0]) >= 2 * 2 * (255 + 255 + 256) * 288 * 2


# -------------------------------------------------------------------------------------------------------------------------------------- p2 and p4
def test_p2_meanshift_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'meanshift', '--meanshift_quantile', '0.2', '0.3'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X, V = data['training']['hidden'], data['validation']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_meanshift_aligned' / 'plot'
    table, labels, centers = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Meanshift.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(table.columns) == p2.Meanshift.COLUMNS + metrics and table['quantile'].tolist() == [0.2, 0.3]
    assert list(labels.columns) == ['bw0', 'bw1'] and len(labels) == len(X)
    assert list(centers.columns) == ['bandwidth', 'cluster'] + ['x%d' % c for c in range(16)]
    for row, q in enumerate((0.2, 0.3)):
        h = table.bandwidth[row]
        assert h == estimate_bandwidth(X, q)
        fit = MeanShift(bandwidth=h).fit(X)
        assert np.array_equal(labels['bw%d' % row].to_numpy(), fit.labels_)
        mine = centers[centers.bandwidth == h]
        assert mine.cluster.tolist() == list(range(len(fit.cluster_centers_))) and np.array_equal(mine.iloc[:, 2:].to_numpy(), fit.cluster_centers_)
        sizes = np.bincount(fit.labels_)
        assert (table.n_clusters[row], table.n_orphans[row], table.largest[row], table.smallest[row], table.n_iter[row]) == (
            len(sizes), 0, sizes.max(), sizes.min(), fit.n_iter_)
        dist = np.sqrt(((V.astype(np.float64) - fit.cluster_centers_[fit.predict(V)]) ** 2).sum(axis=1)).mean()
        assert table.valid_distortion[row] == dist
        assert np.all(np.isfinite(table[metrics].to_numpy()[row]))
    assert table.n_clusters.min() >= 3
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy(), equal_nan=True)
    # a second run finds the files and does not refit; overwrite=True does
    ms = p2.Meanshift(str(plot.parent), metrics, quantiles=[0.2, 0.3])
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Meanshift.FILES]
    calls = []
    real = p2.mean_shift_sweep
    monkeypatch.setattr(p2, 'mean_shift_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = ms.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Meanshift.FILES] == stamps and ms.fits_ is None
    assert np.array_equal(again.to_numpy(), table.to_numpy(), equal_nan=True)
    redo = ms.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and len(ms.fits_) == 2 and np.array_equal(redo.to_numpy(), table.to_numpy(), equal_nan=True)


@pytest.mark.parametrize('cluster_all', [1, 0])
def test_p4_meanshift_branch(tmp_path, monkeypatch, cluster_all):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.MeanShift):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'MeanShift', Recording)
    args = p4.get_arguments(['--cluster_method', 'meanshift', '--meanshift_bandwidth', '2.5', '--meanshift_cluster_all', str(cluster_all)])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_meanshift_aligned'
    saved = {cohort: np.load(out / ('%s_meanshift-bw2.5.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1
    model = made[0]
    k = len(model.cluster_centers_)
    assert k >= 3
    for cohort in COHORTS:
        s = saved[cohort]
        assert sorted(s) == ['cluster_id', 'encounter_id', 'hidden'] and len(s['cluster_id']) == len(data[cohort]['hidden'])
        assert np.array_equal(s['cluster_id'], model.predict(data[cohort]['hidden'], orphans=not cluster_all))
        if cohort != 'training':          # (every training outlier is a seed and ends as a centre of its own; the other cohorts' outliers are orphans)
            assert (np.asarray(s['cluster_id']) == -1).any() == (not cluster_all)
    # the training labels are the estimator's own, re-numbered by descending sbp
    ids = np.asarray(saved['training']['cluster_id'])
    assert np.array_equal(ids, model.labels_)
    plain = MeanShift(bandwidth=2.5, cluster_all=bool(cluster_all)).fit(data['training']['hidden'])
    pad0 = data['training']['padding_mask'][:, 0, :]
    sbp = np.sum(data['training']['ob'][:, 0, :] * pad0, axis=1) / np.sum(pad0, axis=1)          # (generate_align_map's expression)
    order = np.argsort([np.average(sbp[plain.labels_ == i]) for i in range(k)])[::-1]
    rank = np.empty(k, dtype=np.int64)
    rank[order] = np.arange(k)
    assert np.array_equal(ids, np.where(plain.labels_ >= 0, rank[np.maximum(plain.labels_, 0)], -1))
    assert np.array_equal(model.cluster_centers_, plain.cluster_centers_[order])
    means = [np.average(sbp[ids == i]) for i in range(k)]
    assert all(a > b for a, b in zip(means, means[1:]))
    # an existing result is left alone
    stamps = [(out / ('%s_meanshift-bw2.5.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_meanshift-bw2.5.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
