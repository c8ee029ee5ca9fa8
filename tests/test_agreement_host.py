"""The agreement definitions of include/dic_hip.h as numpy (agreement_reference.py) held to sklearn.metrics.cluster on the seeded inputs, the host
arithmetic of agreement.py over them, the errors, ``noise='drop'``, the p2 / p4 collectors on hand-written label files (the device stages replaced by the
numpy statement) and the C entry points' argument checks.  No GPU."""
import numpy as np
import pytest
from sklearn.metrics import cluster as skc
from sklearn.metrics.cluster._expected_mutual_info_fast import expected_mutual_information as sk_emi

from deep_interpolation_clustering_amd import _cluster_cli as cli
from deep_interpolation_clustering_amd import agreement
from agreement_reference import AVERAGES, CASES, SPECIAL, U, Reference, host_device_sums, host_encode, reference

GENERAL = [name for name in CASES if name not in SPECIAL]


@pytest.fixture
def on_host(monkeypatch):
    """agreement.py with the numpy statement in place of the upload and of the three kernels."""
    monkeypatch.setattr(agreement, '_encode', host_encode)
    monkeypatch.setattr(agreement, 'device_sums', host_device_sums)


@pytest.mark.parametrize('name', list(CASES))
def test_integer_indices_equal_sklearn_exactly(name):
    a, b = CASES[name]
    ref = reference(name)
    table = skc.contingency_matrix(a, b)
    assert np.array_equal(ref.table, table) and ref.table.dtype == np.int64
    assert np.array_equal(ref.classes_a, np.unique(a)) and np.array_equal(ref.classes_b, np.unique(b))
    assert np.array_equal(ref.scores.pair_confusion_matrix(), skc.pair_confusion_matrix(a, b))
    assert ref.scores.rand() == skc.rand_score(a, b)
    assert ref.scores.ari() == skc.adjusted_rand_score(a, b)
    assert ref.scores.fmi() == skc.fowlkes_mallows_score(a, b)


def test_ari_uses_python_ints_where_int64_overflows():
    """tp * tn leaves int64 for two near-equal halves of N = 100 000 rows (at 75 000 it stays 15 % inside): sums of that size, not a table."""
    rng = np.random.RandomState(5)
    a = rng.randint(0, 2, 100000)
    b = np.where(rng.rand(100000) < 0.05, 1 - a, a)
    t = skc.contingency_matrix(a, b).astype(np.int64)
    ma, mb = t.sum(1), t.sum(0)
    s = agreement.PairSums(a=ma, b=mb, sum_squares=int((t ** 2).sum()), sum_a2=int((ma ** 2).sum()), sum_b2=int((mb ** 2).sum()), n=100000, mi=0.0, h_a=0.0,
                           h_b=0.0, emi=0.0, table=t)
    sc = agreement.PairScores(s)
    (tn, fp), (fn, tp) = sc.pair_confusion_matrix().tolist()
    assert tp * tn > 2 ** 63
    assert sc.ari() == skc.adjusted_rand_score(a, b) and sc.rand() == skc.rand_score(a, b) and sc.fmi() == skc.fowlkes_mallows_score(a, b)


@pytest.mark.parametrize('name', GENERAL)
def test_mi_entropies_and_emi_lie_within_their_bars_of_sklearn(name):
    a, b = CASES[name]
    ref = reference(name)
    diffs = {'mi': abs(ref.scores.mi() - skc.mutual_info_score(a, b)), 'h_a': abs(ref.sums.h_a - skc.entropy(a)), 'h_b': abs(ref.sums.h_b - skc.entropy(b)),
             'emi': abs(ref.sums.emi - sk_emi(skc.contingency_matrix(a, b, sparse=True), len(a)))}
    print(name, {k: '%.3g of %.3g' % (v, ref.bars[k]) for k, v in diffs.items()})
    for k, v in diffs.items():
        assert v <= ref.bars[k], (k, v, ref.bars[k])


@pytest.mark.parametrize('name', GENERAL)
def test_normalised_indices_lie_within_the_propagated_bars_of_sklearn(name):
    a, b = CASES[name]
    ref = reference(name)
    for avg in AVERAGES:
        for index, sk in (('nmi', skc.normalized_mutual_info_score), ('ami', skc.adjusted_mutual_info_score)):
            got, bar = ref.scores.index(index, avg), ref.index_bar(lambda sc: sc.index(index, avg))
            assert abs(got - sk(a, b, average_method=avg)) <= bar, (index, avg, got, bar)
    for beta in (1.0, 0.5):
        want = skc.homogeneity_completeness_v_measure(a, b, beta=beta)
        for k in range(3):
            got, bar = ref.scores.hcv(beta)[k], ref.index_bar(lambda sc: sc.hcv(beta)[k])
            assert abs(got - want[k]) <= bar, (beta, k, got, bar)


@pytest.mark.parametrize('name', SPECIAL)
def test_special_cases_return_what_sklearn_returns(name):
    a, b = CASES[name]
    sc = reference(name).scores
    for avg in AVERAGES:
        assert sc.nmi(avg) == skc.normalized_mutual_info_score(a, b, average_method=avg)
        assert sc.ami(avg) == skc.adjusted_mutual_info_score(a, b, average_method=avg)
    assert sc.hcv() == skc.homogeneity_completeness_v_measure(a, b)
    assert sc.mi() == skc.mutual_info_score(a, b) and sc.entropies() == (skc.entropy(a), skc.entropy(b))
    if name == 'n2_constant':
        assert sc.nmi() == sc.ami() == 1.0
    if name == 'n2_constant_split':
        assert sc.ami() == 0.0 and sc.nmi() == 0.0


def test_the_clamps_of_ami_hold_the_sign():
    s = reference('planted_64').sums
    eps = np.finfo('float64').eps
    flat = agreement.PairScores(agreement.PairSums(**dict(s.__dict__, mi=s.emi, h_a=s.emi, h_b=s.emi)))
    assert flat.ami() == 1.0          # (0 / 0 -> eps / eps)
    below = agreement.PairScores(agreement.PairSums(**dict(s.__dict__, mi=s.emi - 1e-18)))
    assert below.ami() == pytest.approx(eps / (0.5 * (s.h_a + s.h_b) - s.emi), rel=1e-12)


@pytest.mark.parametrize('name', ['noise_800', 'noncontiguous_500'])
def test_noise_drop_is_sklearn_on_the_kept_rows(name):
    a, b = CASES[name]
    keep = (a != -1) & (b != -1)
    assert 0 < keep.sum() < len(a)
    ref = Reference(a, b, drop=True)
    assert ref.n == keep.sum() and -1 not in ref.classes_a and -1 not in ref.classes_b
    assert np.array_equal(ref.table, skc.contingency_matrix(a[keep], b[keep]))
    assert ref.scores.ari() == skc.adjusted_rand_score(a[keep], b[keep]) and ref.scores.fmi() == skc.fowlkes_mallows_score(a[keep], b[keep])
    assert abs(ref.scores.ami() - skc.adjusted_mutual_info_score(a[keep], b[keep])) <= ref.index_bar(lambda sc: sc.ami())


def test_errors_are_raised_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **kw):
        raise AssertionError('GPU work before the input was checked')
    monkeypatch.setattr(agreement, '_encode', no_gpu)
    monkeypatch.setattr(agreement, 'device_sums', no_gpu)
    a = np.array([0, 1, 1, 2])
    for bad, match in (((a, a[:3]), 'unequal lengths'), ((a[:0], a[:0]), 'empty'), ((a, a.astype(np.float64)), 'integers')):
        with pytest.raises(ValueError, match=match):
            agreement.adjusted_rand_score(*bad)
    with pytest.raises(ValueError, match='no labellings'):
        agreement.agreement_matrix({})
    with pytest.raises(ValueError, match='unknown index'):
        agreement.agreement_matrix({'a': a, 'b': a}, indices=('ari', 'jaccard'))
    with pytest.raises(ValueError, match='average_method'):
        agreement.adjusted_mutual_info_score(a, a, average_method='harmonic')
    with pytest.raises(ValueError, match='average_method'):
        agreement.normalized_mutual_info_score(a, a, average_method='harmonic')
    with pytest.raises(ValueError, match='not there'):
        agreement.agreement_matrix({'a': a, 'b': a}, pairs=[('a', 'c')])
    with pytest.raises(ValueError, match='not there'):
        agreement.agreement_matrix(np.stack([a, a]), pairs=[(0, 2)])
    with pytest.raises(ValueError, match='noise'):
        agreement.agreement_matrix({'a': a, 'b': a}, noise='ignore')
    with pytest.raises(ValueError, match=r'\(L, N\)'):
        agreement.agreement_matrix(a)
    with pytest.raises(ValueError, match='integers'):
        import torch
        agreement.agreement_matrix(torch.zeros((2, 4)))


def test_agreement_matrix_on_the_host_statement(on_host):
    """The batch machinery with the kernels replaced: names, pairs, symmetric matrices, a diagonal from the same path, the per-pair figures, tables and
    matching, ``pairs=`` subsets and a pair that ``noise='drop'`` empties."""
    labellings = {name: CASES['planted_257'][k] for k, name in enumerate(('a', 'b'))}
    labellings['c'] = np.arange(257) % 7
    labellings['one'] = np.zeros(257, dtype=np.int64)
    res = agreement.agreement_matrix(labellings, indices=('ari', 'ami', 'nmi', 'rand', 'fmi', 'vmeasure'), return_tables=True)
    assert res.names == ['a', 'b', 'c', 'one'] and res.pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert res.n.tolist() == [257] * 6 and res.n_clusters.tolist() == [[3, 4], [3, 7], [3, 1], [4, 7], [4, 1], [7, 1]]
    for name in ('ari', 'ami', 'nmi', 'rand', 'fmi', 'vmeasure'):
        m = res[name]
        assert m.shape == (4, 4) and np.array_equal(m, m.T) and m is getattr(res, name)
        for l, v in enumerate(labellings.values()):          # (the diagonal is computed: exactly 1 from integers, 1 within the propagated bar otherwise)
            assert m[l, l] == 1.0 if name in ('ari', 'rand', 'fmi') else abs(m[l, l] - 1.0) <= Reference(v, v).index_bar(lambda r: r.index(name))
        assert res.values[name].tolist() == [m[i, j] for i, j in res.pairs]
    assert res.ari[0, 1] == skc.adjusted_rand_score(labellings['a'], labellings['b'])
    assert res.ami[0, 3] == 0.0 and res.nmi[0, 3] == 0.0 and res.ami[3, 3] == 1.0
    h, c, v = skc.homogeneity_completeness_v_measure(labellings['a'], labellings['b'])
    assert res.homogeneity[0, 1] == pytest.approx(h, abs=1e-14) and res.completeness[0, 1] == pytest.approx(c, abs=1e-14)
    assert res.homogeneity[1, 0] == res.completeness[0, 1] and res.completeness[1, 0] == res.homogeneity[0, 1] and res.vmeasure[0, 1] == pytest.approx(v, abs=1e-14)
    assert np.array_equal(res.tables[0], skc.contingency_matrix(labellings['a'], labellings['b']))
    ca, cb, jac = res.matching[0]
    t = res.tables[0]
    want = t / (t.sum(1)[:, None] + t.sum(0)[None, :] - t)
    assert ca.tolist() == [0, 1, 2] and cb.tolist() == want.argmax(1).tolist() and np.array_equal(jac, want.max(1))
    # pairs= by name and by index, in either orientation: the entries of the full matrix
    sub = agreement.agreement_matrix(labellings, pairs=[('b', 'a'), (2, 3)])
    assert sub.pairs == [(0, 1), (2, 3)] and sub.ari[0, 1] == res.ari[0, 1] and sub.ami[2, 3] == res.ami[2, 3] and np.isnan(sub.ari[0, 2])
    # the single-pair functions are the same machinery
    assert agreement.adjusted_mutual_info_score(labellings['a'], labellings['b']) == res.ami[0, 1]
    t, ia, ib = agreement.contingency_matrix(labellings['a'], labellings['c'])
    assert np.array_equal(t, res.tables[1]) and ia.tolist() == [0, 1, 2] and ib.tolist() == list(range(7))
    assert agreement.entropy(labellings['c']) == pytest.approx(skc.entropy(labellings['c']), abs=1e-14)
    # a pair that keeps no rows
    x, y = np.array([-1, -1, 0, 1]), np.array([0, 1, -1, -1])
    emptied = agreement.agreement_matrix({'x': x, 'y': y, 'z': np.array([0, 0, 0, 1])}, noise='drop')
    assert emptied.n.tolist() == [0, 2, 2] and np.isnan(emptied.ari[0, 1]) and np.isnan(emptied.ami[0, 1]) and emptied.ari[0, 2] == 1.0
    assert emptied.n_clusters.tolist() == [[0, 0], [2, 2], [2, 1]]
    assert np.isnan(agreement.adjusted_rand_score(x, y, noise='drop'))


# ---- the p2 / p4 collectors -----------------------------------------------------------------------------------------------------------------------------------
def _label_files(root, n=40):
    import os
    import pandas as pd
    rng = np.random.RandomState(2)
    made = {}
    for method, columns in (('ward', ['k2', 'k3']), ('hdbscan', ['mcs5'])):
        plot = os.path.join(root, 'ae_mse_%s_aligned' % method, 'plot')
        os.makedirs(plot)
        made[method] = pd.DataFrame({c: rng.randint(-1 if method == 'hdbscan' else 0, 3, n) for c in columns})
        made[method].to_csv(os.path.join(plot, '%s_labels.csv' % method), index=False)
    os.makedirs(os.path.join(root, 'ae_mse_gmm_aligned', 'plot'))
    pd.DataFrame({'k2': rng.randint(0, 2, n - 1)}).to_csv(os.path.join(root, 'ae_mse_gmm_aligned', 'plot', 'gmm_labels.csv'), index=False)          # (short)
    os.makedirs(os.path.join(root, 'raw_consensus_result'))
    made['consensus'] = pd.DataFrame({'k2': rng.randint(1, 3, n)})
    made['consensus'].to_csv(os.path.join(root, 'raw_consensus_result', 'training_consensus.csv'), index=False)
    return made


def test_p2_collects_the_training_labellings_and_writes_the_tables(tmp_path, on_host):
    import pandas as pd
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    root = str(tmp_path)
    made = _label_files(root)
    train = {'encounter_id': np.arange(40)}
    got = cli.training_labellings(root, 'ae_mse', cli.METHODS, 40)
    assert list(got) == ['hdbscan:mcs5', 'ward:k2', 'ward:k3', 'consensus:k2']          # (METHODS' order; the short gmm file is skipped)
    assert np.array_equal(got['ward:k3'], made['ward']['k3'].to_numpy())
    assert list(cli.training_labellings(root, 'ae_mse', ['ward'], 40, consensus=False)) == ['ward:k2', 'ward:k3']
    out = str(tmp_path / 'ae_mse_ward_aligned')
    branch = p2.Agreement(out, 'ward', ['ari', 'ami'], 'all', 'class')
    assert branch.FILES == ('agreement.csv', 'agreement_ari.csv', 'agreement_ami.csv') and branch.metric == 'ae_mse' and branch.out_feat == root
    df = branch.train(train, None)
    assert list(df.columns) == ['labelling_a', 'labelling_b', 'n', 'clusters_a', 'clusters_b', 'ari', 'ami'] and len(df) == 6
    long = pd.read_csv(tmp_path / 'ae_mse_ward_aligned' / 'plot' / 'agreement.csv', float_precision='round_trip')
    assert long.labelling_a.tolist() == ['hdbscan:mcs5'] * 3 + ['ward:k2'] * 2 + ['ward:k3'] and long.n.tolist() == [40] * 6
    assert long.ari[3] == skc.adjusted_rand_score(made['ward']['k2'], made['ward']['k3'])
    assert long.ami[3] == pytest.approx(skc.adjusted_mutual_info_score(made['ward']['k2'], made['ward']['k3']), abs=1e-13)
    square = pd.read_csv(tmp_path / 'ae_mse_ward_aligned' / 'plot' / 'agreement_ari.csv', index_col=0, float_precision='round_trip')
    assert list(square.columns) == list(square.index) == list(got) and np.array_equal(np.diag(square.to_numpy()), np.ones(4))
    assert square.loc['ward:k2', 'ward:k3'] == square.loc['ward:k3', 'ward:k2'] == long.ari[3]
    # left alone on a second run; scope 'method' in another directory sees its own file only; one labelling: nothing written
    stamps = [(tmp_path / 'ae_mse_ward_aligned' / 'plot' / f).stat().st_mtime_ns for f in branch.FILES]
    again = branch.train(train, None)
    assert stamps == [(tmp_path / 'ae_mse_ward_aligned' / 'plot' / f).stat().st_mtime_ns for f in branch.FILES] and again.ari.tolist() == df.ari.tolist()
    own = p2.Agreement(str(tmp_path / 'ae_mse_hdbscan_aligned'), 'hdbscan', ['rand'], 'method', 'drop')
    assert own.train(train, None) is None and not (tmp_path / 'ae_mse_hdbscan_aligned' / 'plot' / 'agreement.csv').exists()
    args = p2.get_arguments(['--agreement', 'ari', 'vmeasure', '--agreement_noise', 'drop'])
    assert args.agreement == ['ari', 'vmeasure'] and args.agreement_scope == 'all' and args.agreement_noise == 'drop'
    assert p2.get_arguments([]).agreement is None


def test_p4_collects_the_label_files_of_one_cohort(tmp_path, on_host):
    import os
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    rng = np.random.RandomState(4)
    ids = np.arange(100, 130)
    for method, stem, other in (('ward', 'training_3', ids), ('kmedoids', 'training_3', ids), ('kmedoids', 'training_4', ids), ('gmm', 'training_3', ids[::-1].copy())):
        d = tmp_path / ('ae_mse_%s_aligned' % method)
        os.makedirs(d, exist_ok=True)
        np.save(d / (stem + '.npy'), {'encounter_id': other, 'cluster_id': rng.randint(0, 3, 30), 'hidden': np.zeros((30, 2), np.float32)})
    np.save(tmp_path / 'ae_mse_ward_aligned' / 'training_lof.npy', {'encounter_id': ids, 'lof': np.ones(30)})          # (no cluster_id)
    np.save(tmp_path / 'ae_mse_ward_aligned' / 'training_tsne.npy', np.zeros((30, 2)))          # (no dict)
    np.save(tmp_path / 'ae_mse_ward_aligned' / 'validation_3.npy', {'encounter_id': ids, 'cluster_id': rng.randint(0, 3, 30)})          # (another cohort)
    got = cli.cohort_labellings(str(tmp_path), 'ae_mse', cli.METHODS, 'training', ids)
    assert list(got) == ['ward/training_3', 'kmedoids/training_3', 'kmedoids/training_4']          # (gmm: other encounters)
    assert list(cli.cohort_labellings(str(tmp_path), 'ae_mse', ['kmedoids'], 'training', ids)) == ['kmedoids/training_3', 'kmedoids/training_4']
    rows, squares = cli.agreement_summary(got, ['ari', 'nmi'])
    assert [r[:2] for r in rows] == [('ward/training_3', 'kmedoids/training_3'), ('ward/training_3', 'kmedoids/training_4'),
                                     ('kmedoids/training_3', 'kmedoids/training_4')]
    assert rows[0][5] == skc.adjusted_rand_score(got['ward/training_3'], got['kmedoids/training_3']) and squares['nmi'].shape == (3, 3)
    args = p4.get_arguments(['--agreement', 'ami', '--agreement_scope', 'method'])
    assert args.agreement == ['ami'] and args.agreement_scope == 'method' and args.agreement_noise == 'class' and p4.get_arguments([]).agreement is None


# ---- the C entry points without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    from deep_interpolation_clustering_amd import _native as N
    lib = N.lib()
    assert lib.dic_agreement_lds_cells() == agreement.LDS_CELLS
    assert lib.dic_agreement_workspace(10) == 80 and lib.dic_agreement_workspace(0) == 0 and lib.dic_agreement_workspace(3) == 32
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)

    def tables(codes=fake, ld=100, L=3, n=100, drop=None, desc=fake, P=3, out=fake, cells=50):
        return lib.dic_agreement_tables(codes, ld, L, n, drop, desc, P, out, cells, None)

    def sums(t=fake, cells=50, desc=fake, L=3, P=3, marg=fake, total=20, isums=fake, fsums=fake):
        return lib.dic_agreement_sums(t, cells, desc, L, P, marg, total, isums, fsums, None)

    def emi(marg=fake, total=20, desc=fake, L=3, P=3, units=9, isums=fake, lf=fake, lf_len=101, out=fake, ws=fake, nbytes=1024):
        return lib.dic_agreement_emi(marg, total, desc, L, P, units, isums, lf, lf_len, out, ws, nbytes, None)

    for kw in ({'codes': None}, {'desc': None}, {'out': None}, {'n': 0}, {'ld': 99}, {'L': 0}, {'P': 0}, {'cells': 0}):
        assert tables(**kw) == -1, kw
    for kw in ({'codes': odd}, {'out': odd}, {'drop': odd}, {'desc': odd}, {'n': 1 << 31, 'ld': 1 << 31}, {'P': 1 << 24}):
        assert tables(**kw) == -2, kw
    for kw in ({'t': None}, {'marg': None}, {'isums': None}, {'fsums': None}, {'desc': None}, {'cells': 0}, {'total': 1}, {'P': 0}):
        assert sums(**kw) == -1, kw
    for kw in ({'t': odd}, {'marg': odd}, {'fsums': odd}, {'L': 1 << 24}):
        assert sums(**kw) == -2, kw
    for kw in ({'marg': None}, {'lf': None}, {'out': None}, {'ws': None}, {'isums': None}, {'units': 0}, {'lf_len': 1}, {'total': 1}):
        assert emi(**kw) == -1, kw
    for kw in ({'lf': odd}, {'ws': ctypes.c_void_p(4104)}, {'units': 1 << 26}):
        assert emi(**kw) == -2, kw
    assert emi(nbytes=0) == -3 and b'workspace' in lib.dic_last_error_string()


def test_agreement_kernels_do_not_spill_to_scratch():
    """The EMI kernel holds a cell's constants and an f64 exp and log per lane (csrc/dic_agreement.hip): require ScratchSize == 0 and no vector-register
    spills for every kernel of the file."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_agreement.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('agreement_tables_kernel', 'agreement_sums_kernel', 'agreement_emi_kernel', 'agreement_emi_finish_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills) == 4
    assert max(scratch) == 0 and max(spills) == 0, (names, scratch, spills)
