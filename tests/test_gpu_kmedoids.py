"""k-medoids on the GPU (csrc/dic_kmedoids.hip, kmedoids.py, the p2 / p4 kmedoids branches) against the numpy f64 yardstick of tests/test_kmedoids_host.py.

Medoids, labels, iteration counts and swap sequences are demanded EQUAL: test_kmedoids_host.py keeps every decision of every case 1e-6 TD away from a tie.
Values are held to derived rounding bounds.  A distance is the root of a sum of D non-negative f64 terms; the GPU and numpy add them in different orders:
(D + 16) 2^-52 d per distance covers both sides' summation, the two roots and the squares.  A sum over the N points of terms that are 1-Lipschitz in the
distances that enter them (d, dn, ds) is off by the sum of those per-distance bounds plus N 2^-53 sum |terms| for the order of the summation."""
import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import kmedoids as KM
from deep_interpolation_clustering_amd.info import COHORTS
from deep_interpolation_clustering_amd.kmedoids import KMedoids, kmedoids_sweep
from test_gpu_optics import _write_latents
from test_kmedoids_host import (CASE_STARTS, blobs, case, dist_matrix, duplicates, matrix, reference, start_of, y_assign, y_build, y_delta, y_first_sums, y_gains,
                                y_pam)

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def dist_bound(d, D):
    return (D + 16) * 2 * U * d


def fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def sum_bound(Dm, med, D):
    """(N,) per candidate c: the bound of a Delta(c, .), g(c) or first-sum entry -- every distance that enters, and N 2^-53 sum |terms| for the summation."""
    _, dn, ds = y_assign(Dm, med)
    n = len(Dm)
    enter = Dm.sum(axis=0) + dn.sum() + fin(ds).sum()
    terms = dn.sum() + np.where(np.isfinite(ds), ds - dn, 0.0).sum() + (Dm.sum(axis=0) if not np.isfinite(ds).all() else 0.0)
    return dist_bound(enter, D) + n * U * terms


def td_bound(td, n, D):
    return dist_bound(td, D) + n * U * td


def device_assign(pts, med):
    m = torch.as_tensor(np.asarray(med), dtype=torch.int32, device=pts.x.device)
    pts.assign(m)
    return m


# -------------------------------------------------------------------------------------------------------------------------------------- ABI: assign
@pytest.mark.parametrize('name', ['a', 'c', 'd'])
def test_assign_against_the_yardstick(name):
    X, k, _ = case(name)
    Dm = matrix(name)
    worst = 0.0
    for med in (start_of(name, 'random'), start_of(name, 'build'), start_of(name, 'random')[:1]):
        pts = KM._Points(X, len(med))
        device_assign(pts, med)
        n, dn, ds = y_assign(Dm, med)
        got_n, got_dn, got_ds, got_td = (t.cpu().numpy() for t in (pts.nearest, pts.dn, pts.ds, pts.td))
        assert np.array_equal(got_n, n)
        assert np.array_equal(np.isfinite(got_ds), np.isfinite(ds)) and (len(med) > 1 or np.isinf(got_ds).all())
        e_dn, e_ds = np.abs(got_dn - dn), np.abs(fin(got_ds) - fin(ds))
        b_dn, b_ds = dist_bound(dn, X.shape[1]), dist_bound(fin(ds), X.shape[1])
        assert (e_dn <= b_dn).all() and (e_ds <= b_ds).all()
        assert (got_dn[np.asarray(med)] == 0.0).all()
        b_td = td_bound(dn.sum(), len(X), X.shape[1])
        assert abs(got_td[0] - dn.sum()) <= b_td
        ratios = [float((e_dn[b_dn > 0] / b_dn[b_dn > 0]).max()), abs(got_td[0] - dn.sum()) / b_td]
        if len(med) > 1:
            ratios.append(float((e_ds / b_ds).max()))
        worst = max(worst, *ratios)
    print('assign %s: largest deviation / bound = %.3g' % (name, worst))


def test_assign_of_other_points_is_predict():
    X, k, _ = case('a')
    Q = blobs(101, 8, 3, 2.0, 77)
    med = start_of('a', 'build')
    pts = KM._Points(X, k)
    m = torch.as_tensor(med, dtype=torch.int32, device=pts.x.device)
    nearest, dn, ds, td = pts.assign(m, torch.as_tensor(Q, device=pts.x.device))
    d = np.sqrt(((Q.astype(np.float64)[:, None, :] - X.astype(np.float64)[med][None, :, :]) ** 2).sum(-1))
    assert np.array_equal(nearest.cpu().numpy(), d.argmin(axis=1))
    assert (np.abs(dn.cpu().numpy() - d.min(axis=1)) <= dist_bound(d.min(axis=1), 8)).all()
    assert abs(td.item() - d.min(axis=1).sum()) <= td_bound(d.min(axis=1).sum(), 101, 8)


# --------------------------------------------------------------------------------------------------------------------------------------- ABI: exact
@pytest.mark.parametrize('name', ['a', 'd'])
def test_exact_table_against_the_yardstick(name):
    X, k, _ = case(name)
    Dm = matrix(name)
    n, D = X.shape
    med = start_of(name, 'random')
    pts = KM._Points(X, k)
    device_assign(pts, med)
    L, st = N.lib(), N.stream_of(pts.x)
    worst = 0.0
    tables = []
    for rep in range(2):
        out = torch.full((n, k), float('nan'), dtype=torch.float64, device=pts.x.device)
        N.check(L.dic_kmedoids_exact(N.ptr(pts.x), pts.x.stride(0), n, pts.d, None, n, None, 2, N.ptr(pts.nearest), N.ptr(pts.dn), N.ptr(pts.ds), k, N.ptr(out), st),
                'dic_kmedoids_exact')
        tables.append(out.cpu().numpy())
    assert np.array_equal(tables[0], tables[1])                # the same bits from call to call
    want = y_delta(Dm, med)
    bound = sum_bound(Dm, med, D)[:, None]
    assert (np.abs(tables[0] - want) <= bound).all()
    worst = float((np.abs(tables[0] - want) / bound).max())
    # BUILD's g and the first step's sums through the same kernel
    for mode, ref in ((1, y_gains(Dm, y_assign(Dm, med)[1])), (0, y_first_sums(Dm))):
        out = torch.full((n,), float('nan'), dtype=torch.float64, device=pts.x.device)
        N.check(L.dic_kmedoids_exact(N.ptr(pts.x), pts.x.stride(0), n, pts.d, None, n, None, mode, None, N.ptr(pts.dn), None, k, N.ptr(out), st), 'dic_kmedoids_exact')
        assert (np.abs(out.cpu().numpy() - ref) <= bound[:, 0]).all()
    # a candidate list with a device-side count, and the pick
    cand = torch.as_tensor([5, 3, n - 1, 0, 7], dtype=torch.int32, device=pts.x.device)
    count = torch.as_tensor([3], dtype=torch.int32, device=pts.x.device)
    part = torch.full((5, k), float('nan'), dtype=torch.float64, device=pts.x.device)
    N.check(L.dic_kmedoids_exact(N.ptr(pts.x), pts.x.stride(0), n, pts.d, N.ptr(cand), 5, N.ptr(count), 2, N.ptr(pts.nearest), N.ptr(pts.dn), N.ptr(pts.ds), k,
                                 N.ptr(part), st), 'dic_kmedoids_exact')
    got = part.cpu().numpy()
    assert np.array_equal(got[:3], tables[0][[5, 3, n - 1]]) and np.isnan(got[3:]).all()
    rec = torch.zeros(4, dtype=torch.float64, device=pts.x.device)
    N.check(L.dic_kmedoids_pick(N.ptr(cand), 5, N.ptr(count), N.ptr(part), k, N.ptr(rec), st), 'dic_kmedoids_pick')
    sub = tables[0][[5, 3, n - 1]]
    at = np.unravel_index(np.argmin(sub), sub.shape)
    assert rec.cpu().tolist() == [float([5, 3, n - 1][at[0]]), float(at[1]), float(sub[at]), 3.0]
    print('exact %s: largest deviation / bound = %.3g' % (name, worst))


@pytest.mark.parametrize('m,cols', [(448, 10), (5000, 32), (1025, 1), (3, 7)])
def test_pick_on_long_lists_in_any_order(m, cols):
    """The arg-min over a candidate list of the length full-size data gives (hundreds of entries per search), in shuffled order, with the smallest value
    also planted as a tie at other (c, i): the smallest c, then the smallest i, wins."""
    dev = torch.device('cuda')
    L = N.lib()
    for seed in range(8):
        rs = np.random.RandomState(1000 * m + seed)
        cand = rs.permutation(4 * m)[:m].astype(np.int32)
        table = rs.uniform(-5.0, 40000.0, (m, cols))
        low = -7.0 - seed
        spots = [(rs.randint(m), rs.randint(cols)) for _ in range(1 + seed % 3)]
        for j, i in spots:
            table[j, i] = low
        want = min((int(cand[j]), i) for j, i in spots)
        count = rs.randint(1, m + 1) if seed == 7 else m      # a device-side count below the capacity
        if count < m:
            live = [(int(cand[j]), i) for j, i in spots if j < count]
            flat = table[:count]
            at = np.unravel_index(np.argmin(flat), flat.shape)
            want = min(live) if live else (int(cand[at[0]]), int(at[1]))
            low = float(flat[at])
        t_cand, t_table = torch.as_tensor(cand, device=dev), torch.as_tensor(table, device=dev)
        t_count = torch.as_tensor([count], dtype=torch.int32, device=dev)
        rec = torch.full((4,), float('nan'), dtype=torch.float64, device=dev)
        N.check(L.dic_kmedoids_pick(N.ptr(t_cand), m, N.ptr(t_count), N.ptr(t_table), cols, N.ptr(rec), N.stream_of(rec)), 'dic_kmedoids_pick')
        assert rec.cpu().tolist() == [float(want[0]), float(want[1]), low, float(count)], (seed, spots)
    none = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(L.dic_kmedoids_pick(N.ptr(t_cand), m, N.ptr(none), N.ptr(t_table), cols, N.ptr(rec), N.stream_of(rec)), 'dic_kmedoids_pick')
    assert rec.cpu().tolist() == [-1.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------------------- ABI: delta pass
def pass_cases():
    out = [(name, case(name)[0], start_of(name, 'random')) for name in ('a', 'c', 'd')]
    for n in (255, 256, 257, 513):
        for d in (4, 256):
            X = blobs(n, d, 3, 3.0 if d == 4 else 0.5, 100 + n + d)
            out.append(('n%d_d%d' % (n, d), X, y_build(dist_matrix(X), 2)[0]))          # two medoids for three blobs: one slot is large, one small
    return out


PASS_CASES = pass_cases()


@pytest.mark.parametrize('name,X,med', PASS_CASES, ids=[c[0] for c in PASS_CASES])
def test_delta_pass_is_within_its_bound_and_the_bound_is_useful(name, X, med):
    Dm = matrix(name) if name in 'acd' else dist_matrix(X)
    n, k = len(X), len(med)
    lab, dn, ds = y_assign(Dm, med)
    sizes = np.bincount(lab, minlength=k)
    if n == 513:
        assert sizes.max() > 256 > sizes.min()                 # a slot of more than one column block, and one of less
    if name == 'c':
        assert sizes.max() > 256
    td = dn.sum()
    pts = KM._Points(X, k + 1)                                 # (a workspace for more slots than the pass uses)
    device_assign(pts, med)
    figures = []
    for mode, want in ((2, y_delta(Dm, med)), (1, y_gains(Dm, dn)[:, None]), (0, y_first_sums(Dm)[:, None])):
        pts.g.fill_(float('nan')); pts.e.fill_(float('nan')); pts.r.fill_(float('nan'))
        pts.delta_pass(k, mode)
        g, e = pts.g.cpu().numpy(), pts.e.cpu().numpy()
        r = pts.r.cpu().numpy().ravel()[:n * k].reshape(n, k) if mode == 2 else np.zeros((n, 1))
        approx = g[:, None] + r
        assert np.isfinite(approx).all() and np.isfinite(e).all() and (e >= 0).all()
        err = np.abs(approx - want)
        assert (err <= e[:, None]).all(), (mode, float((err / e[:, None]).max()))
        scale = td if mode else want.min()                    # (the first step has no TD yet: the smallest sum, the TD it leads to)
        assert e.max() <= 2.0 ** -8 * scale, (mode, e.max() / scale)
        figures.append((mode, float((err / e[:, None]).max()), float(e.max() / scale)))
    print('delta pass %s: (mode, largest error / E, largest E / TD) = %s' % (name, figures))


def test_select_keeps_the_exact_minimum_and_leaves_medoids_out():
    X, k, _ = case('a')
    Dm = matrix('a')
    med = start_of('a', 'random')
    pts = KM._Points(X, k)
    m = device_assign(pts, med)
    c, i, dl, cnt = pts.search(m, 2)
    want = y_delta(Dm, med)
    want[med] = np.inf
    at = np.unravel_index(np.argmin(want), want.shape)
    assert (c, i) == (int(at[0]), int(at[1])) and abs(dl - want[at]) <= sum_bound(Dm, med, X.shape[1])[c]
    listed = pts.list.cpu().numpy()[:cnt]
    assert 1 <= cnt == pts.count.item() and c in listed and not set(listed) & set(med) and len(set(listed)) == cnt


# -------------------------------------------------------------------------------------------------------------------------------------------- fits
def same_fit(fit, ref, Dm, n, D, start):
    assert np.array_equal(fit.medoid_indices_, ref.medoids)
    assert np.array_equal(fit.labels_, ref.labels)
    assert (fit.n_iter_, fit.converged_) == (ref.n_iter, ref.converged)
    assert [s[:4] for s in fit.swaps_] == [s[:4] for s in ref.swaps]
    med = list(start)
    for mine, theirs in zip(fit.swaps_, ref.swaps):
        assert abs(mine[4] - theirs[4]) <= sum_bound(Dm, med, D)[theirs[3]]
        med[theirs[1]] = theirs[3]
    assert abs(fit.inertia_ - ref.td) <= td_bound(ref.td, n, D)
    assert len(fit.n_exact_) == ref.n_iter + (1 if ref.converged else 0) and min(fit.n_exact_, default=1) >= 1


@pytest.mark.parametrize('name,start', CASE_STARTS)
def test_fits_equal_the_yardstick(name, start):
    X, k, seed = case(name)
    ref = reference(name, start)
    fit = KMedoids(k, init='build').fit(X) if start == 'build' else KMedoids(k, init='random', random_state=seed).fit(X)
    assert fit.initial_medoid_indices_.tolist() == start_of(name, start)
    same_fit(fit, ref, matrix(name), len(X), X.shape[1], start_of(name, start))
    assert np.array_equal(fit.cluster_centers_, X[ref.medoids])
    print('fit %s from %s: candidates sent to the exact stage per iteration = %s, BUILD = %s' % (name, start, fit.n_exact_, fit.build_n_exact_))
    if (name, start) == ('c', 'random'):
        # decisions of this run lie closer (1.8e-5 TD) than the approximate stage can tell apart (2^-12): the exact stage must have had a choice to make
        assert max(fit.n_exact_) > 1


def test_max_iter_stops_early_without_convergence():
    X, k, seed = case('b')
    ref = y_pam(matrix('b'), start_of('b', 'random'), max_iter=1)
    fit = KMedoids(k, init=np.asarray(start_of('b', 'random')), max_iter=1).fit(X)
    assert not fit.converged_ and fit.n_iter_ == 1 and not ref.converged
    same_fit(fit, ref, matrix('b'), len(X), X.shape[1], start_of('b', 'random'))
    none = KMedoids(k, init=np.asarray(start_of('b', 'random')), max_iter=0).fit(X)
    assert not none.converged_ and none.n_iter_ == 0 and none.medoid_indices_.tolist() == start_of('b', 'random')


def test_tie_rules_on_duplicated_rows():
    X, _ = duplicates()
    Dm = dist_matrix(X)
    fit = KMedoids(3).fit(X)
    med = y_build(Dm, 3)[0]
    assert fit.initial_medoid_indices_.tolist() == med
    same_fit(fit, y_pam(Dm, med), Dm, len(X), 4, med)
    fit = KMedoids(3, init=[60, 61, 62]).fit(X)                # the originals of the three medoids are candidates with Delta = 0 exactly
    same_fit(fit, y_pam(Dm, [60, 61, 62]), Dm, len(X), 4, [60, 61, 62])


def test_k_1_and_k_n():
    X = blobs(20, 4, 2, 1.0, 13)
    Dm = dist_matrix(X)
    best = int(np.argmin(Dm.sum(axis=0)))
    fit = KMedoids(1).fit(X)
    assert fit.medoid_indices_.tolist() == [best] and fit.converged_ and fit.n_iter_ == 0 and (fit.labels_ == 0).all()
    other = (best + 1) % 20
    fit = KMedoids(1, init=[other]).fit(X)
    same_fit(fit, y_pam(Dm, [other]), Dm, 20, 4, [other])
    assert fit.medoid_indices_.tolist() == [best]
    fit = KMedoids(20).fit(X)
    assert sorted(fit.medoid_indices_.tolist()) == list(range(20)) and fit.converged_ and fit.inertia_ == 0.0 and fit.n_exact_ == [0]
    assert np.array_equal(fit.medoid_indices_[fit.labels_], np.arange(20))
    assert fit.medoid_indices_.tolist() == y_build(Dm, 20)[0]


def test_same_bytes_from_host_array_device_tensor_and_strided_view():
    X, k, seed = case('a')
    dev = torch.device('cuda')
    wide = torch.zeros((len(X), 24), dtype=torch.float32, device=dev)
    wide[:, 4:12] = torch.as_tensor(X, device=dev)
    view = wide[:, 4:12]
    assert KM._usable_view(view) and not view.is_contiguous()
    fits = [KMedoids(k, init='random', random_state=seed).fit(src) for src in (X, X, torch.as_tensor(X, device=dev), view)]
    keep = lambda f: (f.medoid_indices_.tobytes(), f.labels_.tobytes(), np.float64(f.inertia_).tobytes(), repr(f.swaps_), f.n_exact_, f.cluster_centers_.tobytes())
    assert all(keep(f) == keep(fits[0]) for f in fits[1:])


def test_sweep_equals_separate_fits():
    X, _, _ = case('e')
    ks = [2, 3, 5, 8]
    sweep = kmedoids_sweep(X, ks)
    build = y_build(matrix('e'), 8)[0]
    for k in ks:
        one = KMedoids(k).fit(X)
        assert sweep[k].initial_medoid_indices_.tolist() == one.initial_medoid_indices_.tolist() == build[:k]
        assert np.array_equal(sweep[k].medoid_indices_, one.medoid_indices_) and np.array_equal(sweep[k].labels_, one.labels_)
        assert sweep[k].inertia_ == one.inertia_ and sweep[k].swaps_ == one.swaps_ and sweep[k].n_iter_ == one.n_iter_
    assert sweep[8].inertia_ < sweep[5].inertia_ < sweep[3].inertia_ < sweep[2].inertia_
    rnd = kmedoids_sweep(X, [3, 4], init='random', random_state=5)
    assert np.array_equal(rnd[3].medoid_indices_, KMedoids(3, init='random', random_state=5).fit(X).medoid_indices_)


def test_predict_transform_and_kmedoids_pp():
    X, k, _ = case('b')
    Dm = matrix('b')
    Q = blobs(203, 20, 5, 1.0, 91)
    fit = KMedoids(k).fit(X)
    d = np.sqrt(((Q.astype(np.float64)[:, None, :] - X.astype(np.float64)[fit.medoid_indices_][None, :, :]) ** 2).sum(-1))
    assert np.array_equal(fit.predict(Q), d.argmin(axis=1)) and fit.predict(Q).dtype == np.int64
    assert np.array_equal(fit.predict(X), fit.labels_) and np.array_equal(fit.fit_predict(X), fit.labels_)
    t = fit.transform(Q)
    assert t.shape == d.shape and t.dtype == np.float64 and (np.abs(t - d) <= dist_bound(d, 20)).all()
    with pytest.raises(ValueError, match='expecting 20 features'):
        fit.predict(np.zeros((4, 5), np.float32))
    pp = KMedoids(k, init='k-medoids++', random_state=3).fit(X)
    start = pp.initial_medoid_indices_.tolist()
    assert len(set(start)) == k
    same_fit(pp, y_pam(Dm, start), Dm, len(X), 20, start)
    again = KMedoids(k, init='k-medoids++', random_state=3).fit(X)
    assert again.initial_medoid_indices_.tolist() == start and np.array_equal(again.medoid_indices_, pp.medoid_indices_)
    order = np.arange(k)[::-1]
    before = (fit.medoid_indices_.copy(), fit.labels_.copy())
    fit.reorder(order)
    assert np.array_equal(fit.medoid_indices_, before[0][order]) and np.array_equal(fit.medoid_indices_[fit.labels_], before[0][before[1]])
    assert np.array_equal(fit.predict(X), fit.labels_)


# -------------------------------------------------------------------------------------------------------------------------------------- p2 and p4
def test_p2_kmedoids_branch(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    data = _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    args = p2.get_arguments(['--cluster_method', 'kmedoids', '--k_max', '4'])
    args.restore_metric = ['ae_mse']
    res = p2.main(args)
    X = data['training']['hidden']
    plot = tmp_path / 'Results' / 'Pretrain' / 'out_feat' / 'ae_mse_kmedoids_aligned' / 'plot'
    table, labels, medoids = (pd.read_csv(plot / name, float_precision='round_trip') for name in p2.Kmedoids.FILES)
    metrics = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert list(table.columns) == ['k', 'inertia', 'n_iter', 'converged'] + metrics and table.k.tolist() == [2, 3, 4]
    assert list(labels.columns) == ['k2', 'k3', 'k4'] and len(labels) == len(X)
    assert list(medoids.columns) == ['k', 'cluster', 'medoid_index', 'encounter_id'] and len(medoids) == 2 + 3 + 4
    for row, k in enumerate((2, 3, 4)):
        fit = KMedoids(k).fit(X)
        assert np.array_equal(labels['k%d' % k].to_numpy(), fit.labels_)
        mine = medoids[medoids.k == k]
        assert mine.cluster.tolist() == list(range(k)) and np.array_equal(mine.medoid_index.to_numpy(), fit.medoid_indices_)
        assert np.array_equal(mine.encounter_id.to_numpy(), data['training']['encounter_id'][fit.medoid_indices_])
        assert np.array_equal(X[mine.medoid_index.to_numpy()], fit.cluster_centers_)          # the medoid rows are rows of the training latents
        assert (table.inertia[row], table.n_iter[row], table.converged[row]) == (fit.inertia_, fit.n_iter_, 1)
        assert np.all(np.isfinite(table[metrics].to_numpy()[row]))
    assert table.inertia.is_monotonic_decreasing
    df = res['ae_mse']
    assert list(df.columns) == list(table.columns) and np.array_equal(df.to_numpy(), table.to_numpy())
    # --metric_sample is honoured: the table's metrics are those of the sampled points
    sampled = p2.Kmedoids(4, str(tmp_path / 'sampled'), metrics, metric_sample=100).train(data['training'], data['validation'])
    assert np.array_equal(sampled[['k', 'inertia', 'n_iter', 'converged']].to_numpy(), table[['k', 'inertia', 'n_iter', 'converged']].to_numpy())
    assert not np.array_equal(sampled[metrics].to_numpy(), table[metrics].to_numpy())
    # a second run finds the files and does not refit; overwrite=True does
    kd = p2.Kmedoids(4, str(plot.parent), metrics)
    stamps = [(plot / name).stat().st_mtime_ns for name in p2.Kmedoids.FILES]
    calls = []
    real = p2.kmedoids_sweep
    monkeypatch.setattr(p2, 'kmedoids_sweep', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    again = kd.train(data['training'], data['validation'])
    assert not calls and [(plot / name).stat().st_mtime_ns for name in p2.Kmedoids.FILES] == stamps and kd.fits_ is None
    assert np.array_equal(again.to_numpy(), table.to_numpy())
    redo = kd.train(data['training'], data['validation'], overwrite=True)
    assert calls == [1] and sorted(kd.fits_) == [2, 3, 4] and np.array_equal(redo.to_numpy(), table.to_numpy())


def test_p4_kmedoids_branch(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    made = []

    class Recording(p4.KMedoids):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(p4, 'KMedoids', Recording)
    args = p4.get_arguments(['--cluster_method', 'kmedoids', '--num_clusters', '3'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = tmp_path / 'Results' / 'Clustering' / 'out_feat' / 'ae_mse_kmedoids_aligned'
    saved = {cohort: np.load(out / ('%s_3.npy' % cohort), allow_pickle=True).item() for cohort in COHORTS}
    assert len(made) == 1
    model = made[0]
    X = data['training']['hidden']
    for cohort in COHORTS:
        s = saved[cohort]
        want = ['cluster_id', 'encounter_id', 'hidden'] + (['medoid_index'] if cohort == 'training' else [])
        assert sorted(s) == sorted(want) and len(s['cluster_id']) == len(data[cohort]['hidden'])
        assert np.array_equal(s['cluster_id'], model.predict(data[cohort]['hidden']))
    ids = np.asarray(saved['training']['cluster_id'])
    at = np.asarray(saved['training']['medoid_index'])
    assert np.array_equal(ids, model.labels_) and np.array_equal(at, model.medoid_indices_)
    assert np.array_equal(X[at], model.cluster_centers_) and np.array_equal(ids[at], np.arange(3))          # slot j's medoid is a training row labelled j
    # the slots are the estimator's own, re-numbered by descending sbp
    plain = KMedoids(3).fit(X)
    pad0 = data['training']['padding_mask'][:, 0, :]
    sbp = np.sum(data['training']['ob'][:, 0, :] * pad0, axis=1) / np.sum(pad0, axis=1)          # (generate_align_map's expression)
    order = np.argsort([np.average(sbp[plain.labels_ == i]) for i in range(3)])[::-1]
    rank = np.empty(3, dtype=np.int64)
    rank[order] = np.arange(3)
    assert np.array_equal(ids, rank[plain.labels_]) and np.array_equal(at, plain.medoid_indices_[order])
    means = [np.average(sbp[ids == i]) for i in range(3)]
    assert all(a > b for a, b in zip(means, means[1:]))
    # an existing result is left alone
    stamps = [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS]
    p4.main(args)
    assert [(out / ('%s_3.npy' % cohort)).stat().st_mtime_ns for cohort in COHORTS] == stamps
