"""csrc/dic_agreement.hip and agreement.py on the GPU, held to the numpy statement of the definition (agreement_reference.py) on the seeded inputs of
test_agreement_host.py: tables, marginals and integer sums equal (hence pair confusion, Rand, ARI and FMI), MI, the entropies and EMI within the derived
bars; one ragged batch bit for bit against its single-pair calls; the boundaries of the table kernel; the input forms; p2 and p4 end to end."""
import functools

import numpy as np
import pytest
import torch
from sklearn.metrics import cluster as skc

from deep_interpolation_clustering_amd import agreement
from agreement_reference import AVERAGES, CASES, SPECIAL, Reference, reference
from test_gpu_optics import _write_latents

pytestmark = pytest.mark.gpu

N_BATCH = 3000


def held_to(ref, s, what):
    """One pair's device sums against the reference: integers equal, floats within their bars (printed before they are asserted)."""
    assert np.array_equal(s.table, ref.sums.table) and np.array_equal(s.a, ref.sums.a) and np.array_equal(s.b, ref.sums.b), what
    assert (s.sum_squares, s.sum_a2, s.sum_b2, s.n) == (ref.sums.sum_squares, ref.sums.sum_a2, ref.sums.sum_b2, ref.sums.n), what
    diffs = {'mi': abs(s.mi - ref.sums.mi), 'h_a': abs(s.h_a - ref.sums.h_a), 'h_b': abs(s.h_b - ref.sums.h_b), 'emi': abs(s.emi - ref.sums.emi)}
    print(what, {k: '%.3g of %.3g' % (v, ref.bars[k]) for k, v in diffs.items()})
    for k, v in diffs.items():
        assert v <= ref.bars[k], (what, k, v, ref.bars[k])


@pytest.mark.parametrize('name', list(CASES))
def test_every_case_against_the_definition(name):
    a, b = CASES[name]
    ref = reference(name)
    s, classes = agreement._pair(a, b, need_emi=True, return_tables=True)
    assert np.array_equal(classes[0], ref.classes_a) and np.array_equal(classes[1], ref.classes_b)
    held_to(ref, s, name)
    sc = agreement.PairScores(s)
    assert np.array_equal(sc.pair_confusion_matrix(), skc.pair_confusion_matrix(a, b))
    assert (sc.rand(), sc.ari(), sc.fmi()) == (skc.rand_score(a, b), skc.adjusted_rand_score(a, b), skc.fowlkes_mallows_score(a, b))
    for avg in AVERAGES:
        for index, sk in (('nmi', skc.normalized_mutual_info_score), ('ami', skc.adjusted_mutual_info_score)):
            want = sk(a, b, average_method=avg)
            if name in SPECIAL:
                assert sc.index(index, avg) == want, (index, avg)
            else:
                assert abs(sc.index(index, avg) - want) <= ref.index_bar(lambda r: r.index(index, avg)), (index, avg)
    # the public single-pair functions are this machinery
    assert agreement.adjusted_rand_score(a, b) == sc.ari() and agreement.adjusted_mutual_info_score(a, b) == sc.ami()
    assert agreement.expected_mutual_information(a, b) == s.emi and agreement.mutual_info_score(a, b) == sc.mi()
    assert agreement.homogeneity_completeness_v_measure(a, b) == sc.hcv() and agreement.entropy(a) == pytest.approx(skc.entropy(a), abs=1e-12)
    t, ca, cb = agreement.contingency_matrix(a, b)
    assert np.array_equal(t, skc.contingency_matrix(a, b)) and t.dtype == np.int64 and np.array_equal(ca, np.unique(a))


@pytest.mark.parametrize('name', ['noise_800', 'noncontiguous_500'])
def test_noise_drop_against_the_definition(name):
    a, b = CASES[name]
    ref = Reference(a, b, drop=True)
    s, classes = agreement._pair(a, b, noise='drop', need_emi=True, return_tables=True)
    t, ca, cb = agreement._compact(s, classes[0], classes[1])
    assert np.array_equal(t, ref.table) and np.array_equal(ca, ref.classes_a) and np.array_equal(cb, ref.classes_b) and s.n == ref.n
    keep = (a != -1) & (b != -1)
    sc = agreement.PairScores(s)
    assert sc.ari() == skc.adjusted_rand_score(a[keep], b[keep]) == agreement.adjusted_rand_score(a, b, noise='drop')
    assert (sc.k_a, sc.k_b) == (len(ref.classes_a), len(ref.classes_b))
    for k in ('mi', 'h_a', 'h_b', 'emi'):
        assert abs(getattr(s, k) - getattr(ref.sums, k)) <= ref.bars[k], k
    assert abs(sc.ami() - skc.adjusted_mutual_info_score(a[keep], b[keep])) <= ref.index_bar(lambda r: r.ami())


# ---- one ragged batch ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch():
    rng = np.random.RandomState(21)
    base = rng.randint(0, 3, N_BATCH)
    lab = {'one': np.zeros(N_BATCH, dtype=np.int64), 'k2': rng.randint(0, 2, N_BATCH), 'k3': base,
           'k7': np.where(rng.rand(N_BATCH) < 0.5, base, rng.randint(0, 7, N_BATCH)), 'k64': rng.randint(0, 64, N_BATCH), 'k65': rng.randint(0, 65, N_BATCH),
           'k127': np.arange(N_BATCH) % 127, 'k128': rng.permutation(N_BATCH) % 128, 'k129': rng.permutation(N_BATCH) % 129, 'k200': rng.randint(0, 200, N_BATCH),
           'singletons': rng.permutation(N_BATCH), 'noisy': np.where(rng.rand(N_BATCH) < 0.2, -1, base * 5 + 100)}
    for v in lab.values():
        v.setflags(write=False)
    return lab, agreement.agreement_matrix(lab, indices=agreement.INDICES, return_tables=True)


def test_the_batch_has_every_pair_and_the_diagonal_and_repeats_its_bits():
    lab, res = batch()
    L = len(lab)
    assert L == 12 and len(res.pairs) == 66 and res.names == list(lab) and res.n.tolist() == [N_BATCH] * 66
    assert sorted(set(res.n_clusters.ravel().tolist())) == [1, 2, 3, 4, 7, 64, 65, 127, 128, 129, 200, N_BATCH]
    again = agreement.agreement_matrix(lab, indices=agreement.INDICES)
    for name in list(agreement.INDICES) + ['homogeneity', 'completeness']:
        m = res[name]
        assert not np.isnan(m).any() and np.array_equal(m, again[name]), name
        if name not in ('homogeneity', 'completeness'):
            assert np.array_equal(m, m.T), name
        if name in ('ari', 'rand', 'fmi'):          # (integer arithmetic: exactly 1 -- but sklearn's FMI is 0.0 where no two rows share a cluster)
            assert np.diag(m).tolist() == [0.0 if name == 'fmi' and key == 'singletons' else 1.0 for key in lab], name
    # the diagonal is the same kernels on the pair (i, i), nothing hard-wired: MI = H up to their bars, so the normalised indices are 1 up to the propagated bar
    for l, v in enumerate(lab.values()):
        own = Reference(v, v)
        for name in ('ami', 'nmi', 'vmeasure'):
            assert abs(res[name][l, l] - 1.0) <= own.index_bar(lambda r: r.index(name)), (res.names[l], name, res[name][l, l])
    assert np.array_equal(res.homogeneity, res.completeness.T)
    # a labelling of one class against everything: sklearn's special cases
    assert res.ami[0, 0] == 1.0 and res.nmi[0, 0] == 1.0 and np.all(res.ami[0, 1:] == 0.0) and np.all(res.nmi[0, 1:] == 0.0)
    # the singletons determine every labelling
    assert np.all(res.homogeneity[1:-2, -2] == pytest.approx(1.0, abs=1e-12))


def test_every_entry_of_the_batch_equals_its_own_single_pair_call():
    lab, res = batch()
    names = list(lab)
    for i in range(len(names)):
        for j in range(i, len(names)):
            a, b = lab[names[i]], lab[names[j]]
            s, _ = agreement._pair(a, b, need_emi=True)
            sc = agreement.PairScores(s)
            for name in agreement.INDICES:
                assert res[name][i, j] == sc.index(name), (names[i], names[j], name)
    assert res.ari[2, 3] == skc.adjusted_rand_score(lab['k3'], lab['k7']) and res.fmi[4, 5] == skc.fowlkes_mallows_score(lab['k64'], lab['k65'])


def test_pairs_subsets_and_tables_of_the_batch():
    lab, res = batch()
    picks = [('k7', 'k3'), (4, 5), ('singletons', 'k200'), ('one', 'noisy'), (9, 9)]
    sub = agreement.agreement_matrix(lab, indices=('ari', 'ami', 'vmeasure'), pairs=picks, return_tables=True)
    assert sub.pairs == [(2, 3), (4, 5), (9, 10), (0, 11)]
    for i, j in sub.pairs + [(9, 9)]:
        for name in ('ari', 'ami', 'vmeasure', 'homogeneity', 'completeness'):
            assert sub[name][i, j] == res[name][i, j] and sub[name][j, i] == res[name][j, i], (i, j, name)
    assert np.isnan(sub.ari[0, 1])
    for q, (i, j) in enumerate(sub.pairs):
        a, b = lab[res.names[i]], lab[res.names[j]]
        assert np.array_equal(sub.tables[q], skc.contingency_matrix(a, b)) and np.array_equal(sub.tables[q], res.tables[res.pairs.index((i, j))])
    ca, cb, jac = sub.matching[0]          # (k3 against k7: half of k7 copies k3)
    assert ca.tolist() == [0, 1, 2] and cb.tolist() == [0, 1, 2] and np.all(jac > 0.3)
    for pick in (('k3', 'k7'), ('k64', 'k65'), ('k200', 'singletons'), ('k128', 'k129'), ('noisy', 'k7')):          # (held to the definition, with its bars)
        s, _ = agreement._pair(lab[pick[0]], lab[pick[1]], need_emi=True, return_tables=True)
        held_to(Reference(lab[pick[0]], lab[pick[1]]), s, '%s x %s' % pick)


# ---- boundaries ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tables_on_both_sides_of_the_lds_budget():
    assert agreement.LDS_CELLS == 128 * 128
    rng = np.random.RandomState(3)
    n = 5000
    for ka, kb in ((127, 129), (128, 128), (128, 129), (129, 128)):          # (16383 and 16384 cells: counted in LDS; 16512: in global memory)
        assert (ka * kb <= agreement.LDS_CELLS) == ((ka, kb) in ((127, 129), (128, 128)))
        a, b = np.concatenate([np.arange(ka), rng.randint(0, ka, n - ka)]), np.concatenate([np.arange(kb), rng.randint(0, kb, n - kb)])
        t, _, _ = agreement.contingency_matrix(a, b)
        assert t.shape == (ka, kb) and np.array_equal(t, skc.contingency_matrix(a, b)), (ka, kb)


@pytest.mark.parametrize('n', [1, 255, 4095, 4096, 4097, 8192 + 5])
def test_row_counts_around_the_row_chunk(n):
    rng = np.random.RandomState(n)
    a, b = rng.randint(0, 5, n), rng.randint(-1, 3, n)
    t, ca, cb = agreement.contingency_matrix(a, b)
    assert np.array_equal(t, skc.contingency_matrix(a, b)) and t.sum() == n
    assert agreement.adjusted_rand_score(a, b) == skc.adjusted_rand_score(a, b)
    t, _, _ = agreement.contingency_matrix(np.arange(n), b)          # (n x 4 cells: beyond the LDS budget from n = 4097 on)
    assert np.array_equal(t, skc.contingency_matrix(np.arange(n), b))


def test_noise_drop_with_a_pair_that_keeps_no_rows():
    x, y, z = np.array([-1, -1, 0, 1] * 50), np.array([0, 1, -1, -1] * 50), np.array([0, 0, 0, 1] * 50)
    res = agreement.agreement_matrix({'x': x, 'y': y, 'z': z}, indices=agreement.INDICES, noise='drop', return_tables=True)
    assert res.n.tolist() == [0, 100, 100] and res.n_clusters.tolist() == [[0, 0], [2, 2], [2, 1]]
    for name in agreement.INDICES:
        assert np.isnan(res[name][0, 1]) and np.isnan(res[name][1, 0]) and not np.isnan(res[name][0, 2]), name
    assert res.ari[0, 2] == 1.0 and res.ami[0, 2] == pytest.approx(1.0, abs=1e-12) and res.ami[1, 2] == 0.0
    assert res.tables[0].shape == (0, 0) and res.tables[1].tolist() == [[50, 0], [0, 50]] and res.classes[1][0].tolist() == [0, 1]
    assert np.isnan(agreement.adjusted_mutual_info_score(x, y, noise='drop'))
    kept = agreement.agreement_matrix({'x': x, 'y': y, 'z': z}, noise='class')
    assert kept.n.tolist() == [200] * 3 and kept.ari[0, 1] == skc.adjusted_rand_score(x, y)


def test_input_forms_give_identical_results():
    lab, res = batch()
    names = ['k3', 'k7', 'noisy', 'k65']
    rows = np.stack([lab[n] for n in names])
    want = agreement.agreement_matrix({n: lab[n] for n in names}, indices=agreement.INDICES)
    dev = torch.device('cuda', torch.cuda.current_device())
    for form in (rows, rows.astype(np.int32), torch.as_tensor(rows, device=dev), torch.as_tensor(rows.astype(np.int32), device=dev), torch.as_tensor(rows),
                 {n: torch.as_tensor(np.array(lab[n]), device=dev) for n in names}):
        got = agreement.agreement_matrix(form, indices=agreement.INDICES)
        assert got.names == (names if isinstance(form, dict) else [0, 1, 2, 3])
        for name in agreement.INDICES:
            assert np.array_equal(got[name], want[name]), (type(form), name)
    assert want.ari[0, 1] == res.ari[2, 3]


# ---- the programs ----------------------------------------------------------------------------------------------------------------------------------------------
def test_p2_agreement_of_two_methods(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    _write_latents(str(tmp_path / 'Results' / 'Pretrain' / 'out_feat'), 'ae_mse', 35)
    monkeypatch.chdir(tmp_path)
    feat = tmp_path / 'Results' / 'Pretrain' / 'out_feat'
    args = p2.get_arguments(['--cluster_method', 'ward', '--k_max', '4'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    assert not (feat / 'ae_mse_ward_aligned' / 'plot' / 'agreement.csv').exists()          # (nothing changes without the flag)
    args = p2.get_arguments(['--cluster_method', 'kmedoids', '--k_max', '4', '--agreement', 'ari', 'ami', '--agreement_scope', 'all'])
    args.restore_metric = ['ae_mse']
    p2.main(args)
    plot = feat / 'ae_mse_kmedoids_aligned' / 'plot'
    labels = {'%s:%s' % (m, c): v.to_numpy() for m in ('ward', 'kmedoids')
              for c, v in pd.read_csv(feat / ('ae_mse_%s_aligned' % m) / 'plot' / ('%s_labels.csv' % m)).items()}
    assert list(labels) == ['ward:k2', 'ward:k3', 'ward:k4', 'kmedoids:k2', 'kmedoids:k3', 'kmedoids:k4']
    long = pd.read_csv(plot / 'agreement.csv', float_precision='round_trip')          # (%.17g: exact)
    assert list(long.columns) == ['labelling_a', 'labelling_b', 'n', 'clusters_a', 'clusters_b', 'ari', 'ami'] and len(long) == 15
    for row in long.itertuples():
        a, b = labels[row.labelling_a], labels[row.labelling_b]
        assert row.n == 1500 and (row.clusters_a, row.clusters_b) == (len(np.unique(a)), len(np.unique(b)))
        assert row.ari == skc.adjusted_rand_score(a, b)
        assert abs(row.ami - skc.adjusted_mutual_info_score(a, b)) <= Reference(a, b).index_bar(lambda r: r.ami())
    files = ['agreement.csv', 'agreement_ari.csv', 'agreement_ami.csv']
    for name in ('ari', 'ami'):
        square = pd.read_csv(plot / ('agreement_%s.csv' % name), index_col=0, float_precision='round_trip')
        assert list(square.columns) == list(square.index) == list(labels)
        m = square.to_numpy()
        assert np.array_equal(m, m.T)
        for l, v in enumerate(labels.values()):          # (a unit diagonal: exactly for ARI, within the propagated bar for AMI -- it is computed, not hard-wired)
            assert m[l, l] == 1.0 if name == 'ari' else abs(m[l, l] - 1.0) <= Reference(v, v).index_bar(lambda r: r.ami())
        assert [m[list(labels).index(r.labelling_a), list(labels).index(r.labelling_b)] for r in long.itertuples()] == long[name].tolist()
    stamps = [(plot / f).stat().st_mtime_ns for f in files]
    p2.main(args)          # (a second run leaves the files alone)
    assert stamps == [(plot / f).stat().st_mtime_ns for f in files]


def test_p4_agreement_of_two_methods(tmp_path, monkeypatch):
    import pandas as pd
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    data = _write_latents(str(tmp_path / 'Results' / 'Clustering' / 'out_feat'), 'ae_mse', 35, n=(400, 150, 150))
    monkeypatch.chdir(tmp_path)
    feat = tmp_path / 'Results' / 'Clustering' / 'out_feat'
    args = p4.get_arguments(['--cluster_method', 'ward', '--num_clusters', '3'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    assert not list((feat / 'ae_mse_ward_aligned').glob('*agreement*'))
    args = p4.get_arguments(['--cluster_method', 'kmedoids', '--num_clusters', '4', '--agreement', 'ari', 'ami'])
    args.restore_metric = ['ae_mse']
    p4.main(args)
    out = feat / 'ae_mse_kmedoids_aligned'
    for cohort in data:
        a = np.asarray(np.load(feat / 'ae_mse_ward_aligned' / ('%s_3.npy' % cohort), allow_pickle=True).item()['cluster_id']).astype(np.int64)
        b = np.asarray(np.load(out / ('%s_4.npy' % cohort), allow_pickle=True).item()['cluster_id']).astype(np.int64)
        long = pd.read_csv(out / ('%s_agreement.csv' % cohort), float_precision='round_trip')
        assert list(long.columns) == ['labelling_a', 'labelling_b', 'n', 'clusters_a', 'clusters_b', 'ari', 'ami'] and len(long) == 1
        assert (long.labelling_a[0], long.labelling_b[0], long.n[0]) == ('ward/%s_3' % cohort, 'kmedoids/%s_4' % cohort, len(a))
        assert long.ari[0] == skc.adjusted_rand_score(a, b)
        assert abs(long.ami[0] - skc.adjusted_mutual_info_score(a, b)) <= Reference(a, b).index_bar(lambda r: r.ami())
    stamp = (out / 'training_agreement.csv').stat().st_mtime_ns
    p4.main(args)
    assert stamp == (out / 'training_agreement.csv').stat().st_mtime_ns
