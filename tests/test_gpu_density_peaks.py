"""Density-peaks clustering on the GPU (csrc/dic_dpeaks.hip, density_peaks.py, the p2 / p4 densitypeaks branches) against the numpy f64 yardstick of
tests/test_density_peaks_host.py.

Parents, centres, labels, halo and the integer densities are demanded EQUAL: test_density_peaks_host.py keeps every decision of the random cases 1e-9 away
from a tie, and on the lattice case every d^2 is an exact integer, so delta and parent are demanded bit for bit there, tie rules included.  A distance is the
root of a sum of D non-negative f64 terms that the GPU and numpy add in different orders: (D + 16) 2^-52 d per distance, the bound test_gpu_kmedoids.py derives."""
import ctypes as C

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.density_peaks import DensityPeaks, density_peaks_sweep
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.meanshift import estimate_bandwidth
from test_density_peaks_host import MARGIN, RANDOM, case, solve, y_density, y_density_from_kth, y_order
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
DEV = 'cuda'


def dist_bound(d, D):
    return (D + 16) * 2 * U * d


def padded(X):
    x = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float32), device=DEV)
    return torch.nn.functional.pad(x, (0, (-x.shape[1]) % 4)).contiguous()


def prepared(xs):
    L = N.lib()
    n, d = xs.shape
    ws = torch.empty(int(L.dic_dpeaks_workspace(n, d)), dtype=torch.uint8, device=DEV)
    centre = xs.double().mean(dim=0).float().contiguous()
    N.check(L.dic_dpeaks_prepare(N.ptr(xs), xs.stride(0), n, d, N.ptr(centre), N.ptr(ws), ws.numel(), N.stream_of(xs)), 'dic_dpeaks_prepare')
    return ws


def raw_delta(xs, ws, capacity):
    """One dic_dpeaks_delta call: (rc, delta, parent, cand rows read back, n_cand, stats)."""
    n, d = xs.shape
    delta = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    parent = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    cand = torch.zeros((max(capacity, 1), 4), dtype=torch.int32, device=DEV)
    nc, st = C.c_int64(-1), (C.c_int64 * 2)()
    rc = N.lib().dic_dpeaks_delta(N.ptr(xs), xs.stride(0), n, d, N.ptr(cand), capacity, N.ptr(delta), N.ptr(parent), C.byref(nc), st, N.ptr(ws), ws.numel(),
                                  N.stream_of(xs))
    torch.cuda.synchronize()
    return rc, delta.cpu().numpy(), parent.cpu().numpy(), cand.cpu().numpy()[:max(0, min(int(nc.value), capacity))], int(nc.value), [int(v) for v in st]


def sorted_case(name):
    c = case(name)
    s = c['cutoff']
    order, rank = y_order(s['rho'])
    return c, s, order, rank, padded(c['X'][order])


# -------------------------------------------------------------------------------------------------------------------------------------- ABI: delta
@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e'])
def test_delta_and_parent_against_the_yardstick(name):
    c, s, order, rank, xs = sorted_case(name)
    n, D = xs.shape
    ws = prepared(xs)
    rc, delta, parent, cand, nc, stats = raw_delta(xs, ws, 64 * n)
    assert rc == 0 and 0 < nc <= 64 * n
    want_parent = np.where(s['parent'][order] >= 0, rank[np.maximum(s['parent'][order], 0)], -1)          # rank space
    want_delta = s['delta'][order]
    assert np.array_equal(parent, want_parent)
    err, bound = np.abs(delta - want_delta), dist_bound(want_delta, D)
    assert (err <= bound).all()
    pos = bound > 0
    print('delta %s: worst deviation / bound = %.3f, candidates %d (%.2f per row, longest %d)' % (
        name, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0, nc, nc / n, stats[1]))
    if name == 'e':          # every d^2 an exact integer: bit for bit, the tie rule included
        assert np.array_equal(delta, want_delta)
    # the list: eligible pairs only, each once, every row's true minimiser among them, the exact d^2 in the entry, stats consistent
    rows, cols = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64)
    assert (cols < rows).all() and (cols >= 0).all() and (rows < n).all()
    keys = rows * n + cols
    assert np.unique(keys).size == nc
    assert np.isin(np.arange(1, n) * n + want_parent[1:], keys).all()
    d2 = np.ascontiguousarray(cand[:, 2:4]).view(np.float64).ravel()
    ref = c['D2'][order[rows], order[cols]]
    assert (np.abs(d2 - ref) <= (D + 16) * 2 * U * ref).all()
    per_row = np.bincount(rows, minlength=n)
    assert stats == [nc, int(per_row.max())] and per_row[0] == 0 and (per_row[1:] >= 1).all()
    # two calls give the same bits (the list in any order)
    rc2, delta2, parent2, cand2, nc2, stats2 = raw_delta(xs, ws, 64 * n)
    assert rc2 == 0 and delta2.tobytes() == delta.tobytes() and parent2.tobytes() == parent.tobytes() and (nc2, stats2) == (nc, stats)

    def canon(a):
        return a[np.lexsort((a[:, 1], a[:, 0]))]
    assert np.array_equal(canon(cand2), canon(cand))


def test_capacity_protocol():
    c, s, order, rank, xs = sorted_case('e')
    ws = prepared(xs)
    rc, delta, parent, _, need, _ = raw_delta(xs, ws, 1)
    assert rc == -3 and need > 1                                              # DIC_ERR_WORKSPACE with the needed count
    assert b'candidate' in N.lib().dic_last_error_string()
    rc, delta, parent, cand, nc, stats = raw_delta(xs, ws, need)
    assert rc == 0 and nc == need and len(cand) == need
    assert np.array_equal(delta, s['delta'][order])
    rc0, *_, need0, _ = raw_delta(xs, ws, 0)
    assert rc0 == -3 and need0 == need


def test_one_and_two_points():
    x = padded(np.array([[1.0, 2.0, 3.0, 4.0], [4.0, 6.0, 3.0, 4.0]], np.float32))
    ws = prepared(x[:1])
    rc, delta, parent, cand, nc, stats = raw_delta(x[:1].contiguous(), ws, 4)
    assert (rc, delta.tolist(), parent.tolist(), nc, stats) == (0, [0.0], [-1], 0, [0, 0])
    ws = prepared(x)
    rc, delta, parent, cand, nc, stats = raw_delta(x, ws, 4)
    assert (rc, delta.tolist(), parent.tolist(), nc, stats) == (0, [5.0, 5.0], [-1, 0], 1, [1, 1])
    assert cand[0, :2].tolist() == [1, 0] and np.ascontiguousarray(cand[:, 2:4]).view(np.float64).ravel().tolist() == [25.0]
    m = DensityPeaks(1, dc=1.0).fit(x.cpu().numpy()[:1])
    assert m.labels_.tolist() == [0] and m.parent_.tolist() == [-1] and m.rho_.tolist() == [0]
    m = DensityPeaks(2, dc=1.0).fit(x.cpu().numpy())
    assert m.labels_.tolist() == [0, 1] and m.parent_.tolist() == [-1, 0] and m.delta_.tolist() == [5.0, 5.0] and m.center_indices_.tolist() == [0, 1]


def test_argument_validation_touches_no_gpu():
    L = N.lib()
    x = padded(np.zeros((8, 8), np.float32))
    ws = prepared(x)
    delta, parent = torch.empty(8, dtype=torch.float64, device=DEV), torch.empty(8, dtype=torch.int32, device=DEV)
    cand = torch.empty((64, 4), dtype=torch.int32, device=DEV)
    nc, st = C.c_int64(0), (C.c_int64 * 2)()

    def call(xp=N.ptr(x), ldx=8, n=8, d=8, dp=N.ptr(delta), wsp=N.ptr(ws)):
        return L.dic_dpeaks_delta(xp, ldx, n, d, N.ptr(cand), 64, dp, N.ptr(parent), C.byref(nc), st, wsp, ws.numel(), None)
    assert call() == 0
    assert call(xp=None) == -1 and call(dp=None) == -1 and call(wsp=None) == -1          # NULL pointers
    assert call(n=0) == -1                                                                # N < 1
    assert call(d=6) == -2 and call(d=260, ldx=260) == -2                                 # D % 4, D > 256
    assert L.dic_dpeaks_workspace(0, 8) == 0 and L.dic_dpeaks_workspace(8, 260) == 0
    assert L.dic_dpeaks_prepare(None, 8, 8, 8, N.ptr(x), N.ptr(ws), ws.numel(), None) == -1
    assert L.dic_dpeaks_prepare(N.ptr(x), 8, 8, 8, N.ptr(x), N.ptr(ws), 16, None) == -3
    lab = torch.zeros(8, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.dic_dpeaks_border(8, 8, 1.0, None, N.ptr(lab), 1, None, 0, N.ptr(out), N.ptr(ws), ws.numel(), None) == -1
    assert L.dic_dpeaks_border(0, 8, 1.0, N.ptr(lab), N.ptr(lab), 1, None, 0, N.ptr(out), N.ptr(ws), ws.numel(), None) == -1
    assert L.dic_dpeaks_border(8, 6, 1.0, N.ptr(lab), N.ptr(lab), 1, None, 0, N.ptr(out), N.ptr(ws), ws.numel(), None) == -2


# ------------------------------------------------------------------------------------------------------------------------------------- the module
def same_model(m, c, s, D, halo):
    X = c['X']
    assert np.array_equal(m.order_, y_order(s['rho'])[0])
    assert np.array_equal(m.parent_, s['parent'])
    err, bound = np.abs(m.delta_ - s['delta']), dist_bound(s['delta'], D)
    assert (err <= bound).all()
    assert np.array_equal(m.gamma_, m.rho_.astype(np.float64) * m.delta_)
    assert np.array_equal(m.center_indices_, s['centres']) and np.array_equal(m.cluster_centers_, X[s['centres']])
    assert np.array_equal(m.core_labels_, s['labels'])
    assert m.n_candidates_ >= len(X) - 1 and m.n_features_in_ == X.shape[1]
    rho, delta, gamma = m.decision_graph()
    assert rho is m.rho_ and delta is m.delta_ and gamma is m.gamma_
    if halo:
        assert np.array_equal(m.halo_, s['halo']) and np.array_equal(m.border_density_, s['border2'] / 2.0)
        assert np.array_equal(m.labels_, np.where(s['halo'], -1, s['labels']))
    else:
        assert not m.halo_.any() and m.border_density_ is None and np.array_equal(m.labels_, s['labels'])
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'e', 'h'])
def test_cutoff_fits_equal_the_yardstick(name):
    c = case(name)
    s = c['cutoff']
    halo = name in 'eh'
    m = DensityPeaks(c['K'], dc=c['dc'], halo=halo).fit(c['X'])
    assert m.rho_.dtype == np.int64 and np.array_equal(m.rho_, s['rho']) and m.dc_ == c['dc']
    worst = same_model(m, c, s, c['X'].shape[1], halo)
    if name == 'e':
        assert np.array_equal(m.delta_, s['delta'])
    print('cutoff %s: worst delta deviation / bound = %.3f, halo %d, border2 %s, candidates %d' % (
        name, worst, int(m.halo_.sum()), None if not halo else (2 * m.border_density_).astype(int).tolist(), m.n_candidates_))


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'e', 'h'])
def test_knn_fits_equal_the_yardstick(name):
    c = case(name)
    kth = knn.kth_neighbor_distance(c['X'], c['k'])
    rho = y_density_from_kth(kth)
    s = solve(c['D2'], rho, c['K'])          # the yardstick from the densities the definition names: the k-th distances of dic_knn_kth_distance
    if name in RANDOM:
        assert s['margin'] > MARGIN and s['gap'] > MARGIN
    m = DensityPeaks(c['K'], density='knn', n_neighbors=c['k']).fit(c['X'])
    assert m.rho_.tobytes() == rho.tobytes() and m.dc_ is None          # bit for bit
    worst = same_model(m, c, s, c['X'].shape[1], False)
    if name == 'e':
        assert np.array_equal(m.delta_, s['delta'])
    print('knn %s: worst delta deviation / bound = %.3f, candidates %d' % (name, worst, m.n_candidates_))


def test_auto_dc_is_the_percent_rule():
    c = case('a')
    X = c['X']
    m = DensityPeaks(3, percent=2.0).fit(X)
    assert m.dc_ == estimate_bandwidth(X, quantile=0.02)
    want = c['dc']          # the yardstick's mean k-th distance: every distance within (D + 16) 2^-52, the mean of N of them within N 2^-53 more
    assert abs(m.dc_ - want) <= (X.shape[1] + 16 + len(X)) * 2 * U * want
    assert np.array_equal(m.rho_, y_density(c['D2'], 'cutoff', dc=m.dc_))
    # thresholds in place of n_clusters
    t = DensityPeaks(rho_min=5, delta_min=1.5, dc=c['dc']).fit(X)
    s = c['cutoff']
    order, rank = y_order(s['rho'])
    assert (np.abs(s['delta'] - 1.5) > 1e-9).all()
    assert t.center_indices_.tolist() == [i for i in order if (s['rho'][i] > 5 and s['delta'][i] > 1.5) or rank[i] == 0]


def test_same_bytes_from_host_array_device_tensor_and_strided_view():
    c = case('c')          # 6 features: the host array and the device tensor are padded copies
    X = c['X']
    kw = dict(dc=c['dc'], halo=True)
    ref = DensityPeaks(c['K'], **kw).fit(X)
    wide = torch.zeros((len(X), 12), dtype=torch.float32, device=DEV)
    wide[:, :8] = padded(X)
    for other in (torch.as_tensor(X, device=DEV), wide[:, :8]):          # (the view: 8 columns of 12, used in place)
        m = DensityPeaks(c['K'], **kw).fit(other)
        for name in ('rho_', 'delta_', 'parent_', 'gamma_', 'order_', 'center_indices_', 'labels_', 'core_labels_', 'halo_', 'border_density_'):
            assert getattr(m, name).tobytes() == getattr(ref, name).tobytes(), name
        assert np.array_equal(m.cluster_centers_[:, :6], ref.cluster_centers_)


def test_sweep_equals_separate_fits_with_one_device_computation(monkeypatch):
    c = case('h')
    X = c['X']
    L = N.lib()
    calls = []
    real = L.dic_dpeaks_delta
    monkeypatch.setattr(L, 'dic_dpeaks_delta', lambda *a: calls.append(1) or real(*a), raising=False)
    fits = density_peaks_sweep(X, [2, 3, 4, 5], dc=c['dc'], halo=True)
    assert calls == [1] and sorted(fits) == [2, 3, 4, 5]
    gam = np.sort(fits[2].gamma_)[::-1]
    for k in (2, 3, 4, 5):
        one = DensityPeaks(k, dc=c['dc'], halo=True).fit(X)
        for name in ('rho_', 'delta_', 'parent_', 'center_indices_', 'labels_', 'core_labels_', 'halo_', 'border_density_'):
            assert getattr(fits[k], name).tobytes() == getattr(one, name).tobytes(), (k, name)
        assert fits[k].gamma_gap_ == gam[k - 1] / gam[k] == one.gamma_gap_
    assert len(calls) == 5
    assert np.array_equal(fits[3].labels_, np.where(c['cutoff']['halo'], -1, c['cutoff']['labels']))


def test_predict_is_the_nearest_centre():
    c = case('a')
    m = DensityPeaks(c['K'], dc=c['dc']).fit(c['X'])
    Q = np.random.default_rng(9).normal(0, 2.0, (333, 8)).astype(np.float32)
    d2 = ((Q.astype(np.float64)[:, None, :] - m.cluster_centers_.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    two = np.sort(d2, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) > 1e-9 * two[:, 1]).all()
    got = m.predict(Q)
    assert got.dtype == np.int64 and np.array_equal(got, d2.argmin(axis=1))
    assert np.array_equal(m.predict(c['X'][m.center_indices_]), np.arange(c['K']))
    with pytest.raises(ValueError, match='features'):
        m.predict(np.zeros((3, 9), np.float32))


# -------------------------------------------------------------------------------------------------------------------------------------- p2 and p4
def test_p2_densitypeaks_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'densitypeaks', '--k_max', '4', '--dp_halo', '1', '--dp_percent', '3'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X = data['training']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_densitypeaks_aligned' / 'plot'
    decision, table, labels = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Densitypeaks.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(decision.columns) == ['index', 'rho', 'delta', 'gamma', 'parent'] and len(decision) == len(X)
    assert list(table.columns) == ['k', 'gamma_gap', 'sizes', 'n_halo'] + metrics and table.k.tolist() == [2, 3, 4]
    assert list(labels.columns) == ['k2', 'k3', 'k4'] and len(labels) == len(X)
    fits = density_peaks_sweep(X, [2, 3, 4], percent=3.0, halo=True)
    one = fits[2]
    assert np.array_equal(decision['index'].to_numpy(), np.arange(len(X))) and np.array_equal(decision.rho.to_numpy(), one.rho_)
    assert np.array_equal(decision.delta.to_numpy(), one.delta_) and np.array_equal(decision.gamma.to_numpy(), one.gamma_)          # (%.17g: exact)
    assert np.array_equal(decision.parent.to_numpy(), one.parent_)
    for row, k in enumerate((2, 3, 4)):
        assert np.array_equal(labels['k%d' % k].to_numpy(), fits[k].labels_)
        assert table.gamma_gap[row] == fits[k].gamma_gap_ and table.n_halo[row] == int(fits[k].halo_.sum())
        assert [int(v) for v in table.sizes[row].split()] == np.bincount(fits[k].core_labels_, minlength=k).tolist()
        assert np.all(np.isfinite(table[metrics].to_numpy(dtype=np.float64)[row]))
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy())
    # a second run finds the files and does not compute again
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Densitypeaks.FILES]
    p2.main(args)
    assert [(plot / name).stat().st_mtime_ns for name in p2.Densitypeaks.FILES] == stamps


@pytest.mark.parametrize('transfer', ['centre', 'knn'])
def test_p4_densitypeaks_branch(tmp_path, monkeypatch, transfer):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p4.get_arguments(['--cluster_method', 'densitypeaks', '--num_clusters', '3', '--dp_percent', '3', '--transfer', transfer])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_densitypeaks_aligned'
    tag = '_knn' if transfer == 'knn' else ''
    saved = {cohort: np.load(out / ('%s_3%s.npy' % (cohort, tag)), allow_pickle=True).item() for cohort in COHORTS}
    X = data['training']['hidden']
    plain = DensityPeaks(3, percent=3.0).fit(X)
    pad0 = data['training']['padding_mask'][:, 0, :]
    sbp = np.sum(data['training']['ob'][:, 0, :] * pad0, axis=1) / np.sum(pad0, axis=1)          # (generate_align_map's expression)
    order = np.argsort([np.average(sbp[plain.labels_ == i]) for i in range(3)])[::-1]
    slot = np.empty(3, dtype=np.int64)
    slot[order] = np.arange(3)
    ids = np.asarray(saved['training']['cluster_id'])
    at = np.asarray(saved['training']['center_index'])
    assert np.array_equal(ids, slot[plain.labels_]) and np.array_equal(at, plain.center_indices_[order])          # slots ordered by sbp
    assert np.array_equal(ids[at], np.arange(3))
    means = [np.average(sbp[ids == i]) for i in range(3)]
    assert all(a > b for a, b in zip(means, means[1:]))
    plain.reorder(order)
    for cohort in COHORTS[1:]:
        s = saved[cohort]
        feat = data[cohort]['hidden']
        assert len(s['cluster_id']) == len(feat) and 'center_index' not in s
        if transfer == 'knn':
            lab, vote = knn.knn_transfer_labels(X, ids.astype(np.int64), feat, X.shape[1] + 1)
            assert np.array_equal(s['cluster_id'], lab) and np.array_equal(s['cluster_vote'], vote)
        else:
            assert np.array_equal(s['cluster_id'], plain.predict(feat)) and 'cluster_vote' not in s
    # an existing result is left alone
    stamps = [(out / ('%s_3%s.npy' % (cohort, tag))).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_3%s.npy' % (cohort, tag))).stat().st_mtime_ns for cohort in COHORTS] == stamps
