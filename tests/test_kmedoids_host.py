"""k-medoids (PAM) without a GPU: the numpy f64 yardstick of the definition in include/dic_hip.h on the full distance matrix, the conditions that make
demanding EQUAL medoids, labels and swap sequences of the GPU fair, brute force at a size where every medoid pair can be enumerated, the tie rules, the ABI's
argument checks, the Python argument errors and the p2 / p4 parsers.

The yardstick: d(o, c) = sqrt(sum_k (x_ok - x_ck)^2) in f64; n, dn, ds, TD; BUILD; SWAP by steepest descent, ties to the smaller c then the smaller slot.
Every decision of every case is required to be clear by GAP * TD = 1e-6 TD -- about 10^6 times the f64 summation noise of the sums involved (N 2^-53 TD) --
so an implementation that adds the same terms in another order takes the same decisions."""
import ctypes
import functools
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import kmedoids as KM

GAP = 1e-6
INF = float('inf')


# ----------------------------------------------------------------------------------------------------------------------------------- the yardstick
def dist_matrix(X32):
    """(N, N) f64: the Euclidean distances of the f32 rows, the differences formed in f64 (exact), row blocks to bound the memory."""
    X = np.asarray(X32, dtype=np.float64)
    n = len(X)
    out = np.empty((n, n))
    for i0 in range(0, n, 64):
        out[i0:i0 + 64] = np.sqrt(((X[i0:i0 + 64, None, :] - X[None, :, :]) ** 2).sum(-1))
    return out


def y_assign(Dm, med):
    """n (ties to the smaller slot), dn, ds (+inf at K = 1) of every row of Dm (rows: points, columns: all points) against the medoid columns."""
    d = Dm[:, med]
    n = np.argmin(d, axis=1)                                   # (numpy: the first minimum)
    dn = d[np.arange(len(d)), n]
    if len(med) == 1:
        return n, dn, np.full(len(d), INF)
    rest = d.copy()
    rest[np.arange(len(d)), n] = INF
    return n, dn, rest.min(axis=1)


def y_first_sums(Dm):
    return Dm.sum(axis=0)


def y_gains(Dm, dn):
    """g(c) of every c."""
    return (np.minimum(Dm, dn[:, None]) - dn[:, None]).sum(axis=0)


def y_delta(Dm, med):
    """Delta(c, i) of every c (the medoids' rows too) and every slot: (N, K)."""
    n, dn, ds = y_assign(Dm, med)
    g = y_gains(Dm, dn)
    rem = np.minimum(Dm, ds[:, None]) - np.minimum(Dm, dn[:, None])          # (o, c)
    out = np.empty((Dm.shape[0], len(med)))
    for i in range(len(med)):
        out[:, i] = g + rem[n == i].sum(axis=0)
    return out


def _pick(values, forbidden):
    """(index of the smallest value among the allowed ones -- the first one --, the gap to the next DIFFERENT candidate's value, how many attain it)."""
    v = np.array(values, dtype=np.float64)
    v[list(forbidden)] = INF
    best = int(np.argmin(v))
    ties = int((v == v[best]).sum())
    rest = v.copy()
    rest[best] = INF
    return best, float(rest.min() - v[best]), ties


def y_build(Dm, K):
    """(medoids, gaps relative to the one-medoid TD, ties per step)."""
    med, gaps, ties = [], [], []
    scale = None
    for step in range(K):
        if step == 0:
            vals = y_first_sums(Dm)
        else:
            vals = y_gains(Dm, y_assign(Dm, med)[1])
        c, gap, t = _pick(vals, med)
        if scale is None:
            scale = vals[c]
        med.append(c)
        gaps.append(gap / scale if scale > 0 else INF)
        ties.append(t)
    return med, gaps, ties


class Fit:
    pass


def y_pam(Dm, init, max_iter=300):
    """SWAP from the medoids ``init``: medoids, labels, TD, n_iter, converged, swaps [(iteration, slot, out, in, Delta)], and per iteration the gap of the
    choice and of the stopping decision relative to TD, and the number of (c, i) that attain the smallest Delta."""
    med = [int(v) for v in init]
    f = Fit()
    f.swaps, f.choice_gaps, f.stop_gaps, f.ties = [], [], [], []
    f.converged, f.n_iter = False, 0
    for it in range(max_iter):
        td = y_assign(Dm, med)[1].sum()
        delta = y_delta(Dm, med)
        delta[med] = INF
        if not np.isfinite(delta).any():                     # K = N: no candidate
            f.converged = True
            break
        flat = delta.ravel()                                   # row-major: the first minimum is the smaller c, then the smaller slot
        at = int(np.argmin(flat))
        c, i = divmod(at, len(med))
        best = flat[at]
        rest = flat.copy()
        rest[at] = INF
        f.ties.append(int((flat == best).sum()))
        f.choice_gaps.append(float(rest.min() - best) / td if td > 0 else INF)
        f.stop_gaps.append(abs(float(best)) / td if td > 0 else INF)
        if not best < 0:
            f.converged = True
            break
        f.swaps.append((it, i, med[i], c, float(best)))
        med[i] = c
        f.n_iter = it + 1                                      # iterations that swapped: the search that stops is not counted
    f.medoids = np.asarray(med, dtype=np.int64)
    f.labels, dn, _ = y_assign(Dm, med)
    f.td = float(dn.sum())
    return f


# ---------------------------------------------------------------------------------------------------------------------------------------- the cases
def blobs(n, d, k, sep, seed):
    r = np.random.RandomState(seed)
    c = r.randn(k, d) * sep
    lab = r.randint(k, size=n)
    return (c[lab] + r.randn(n, d)).astype(np.float32) + 3.0


CASES = {'a': (300, 8, 3, 2.0, 1), 'b': (517, 20, 5, 1.0, 2), 'c': (1030, 256, 4, 0.3, 3), 'd': (259, 4, 2, 1.5, 4), 'e': (770, 12, 8, 1.2, 5)}
ITERATIONS = {'a': (1, 3), 'b': (2, 7), 'c': (3, 6), 'd': (1, 3), 'e': (3, 9)}          # iterations that swapped: from BUILD, from the random start
STARTS = ('build', 'random')
CASE_STARTS = [(name, start) for name in CASES for start in STARTS]


@functools.lru_cache(maxsize=None)
def case(name):
    n, d, k, sep, seed = CASES[name]
    X = blobs(n, d, k, sep, seed)
    X.setflags(write=False)
    return X, k, seed


@functools.lru_cache(maxsize=None)
def matrix(name):
    Dm = dist_matrix(case(name)[0])
    Dm.setflags(write=False)
    return Dm


@functools.lru_cache(maxsize=None)
def build_of(name):
    return y_build(matrix(name), case(name)[1])


def start_of(name, start):
    X, k, seed = case(name)
    if start == 'build':
        return list(build_of(name)[0])
    return [int(v) for v in np.random.RandomState(seed).choice(len(X), k, replace=False)]


@functools.lru_cache(maxsize=None)
def reference(name, start, max_iter=300):
    return y_pam(matrix(name), start_of(name, start), max_iter)


@functools.lru_cache(maxsize=None)
def duplicates():
    """60 points and, behind them, copies of the three BUILD medoids of the 60 (rows 60, 61, 62): every copy ties with its original exactly."""
    base = blobs(60, 4, 3, 2.0, 7)
    b = y_build(dist_matrix(base), 3)[0]
    X = np.concatenate([base, base[b]])
    X.setflags(write=False)
    return X, b


# -------------------------------------------------------------------------------------------------------------------------- conditions of the cases
@pytest.mark.parametrize('name', list(CASES))
def test_build_choices_are_clear(name):
    med, gaps, ties = build_of(name)
    assert len(set(med)) == case(name)[1]
    assert min(gaps) >= GAP and max(ties) == 1, (gaps, ties)


@pytest.mark.parametrize('name,start', CASE_STARTS)
def test_swap_choices_and_the_stopping_decision_are_clear(name, start):
    r = reference(name, start)
    assert r.converged
    assert min(r.choice_gaps) >= GAP and min(r.stop_gaps) >= GAP and max(r.ties) == 1, (r.choice_gaps, r.stop_gaps)
    assert r.n_iter == ITERATIONS[name][STARTS.index(start)]
    assert len(r.swaps) == r.n_iter >= 1 and all(s[4] < 0 for s in r.swaps)
    tds = [y_assign(matrix(name), start_of(name, start))[1].sum()]
    for s in r.swaps:                                          # every swap lowers TD by its Delta
        tds.append(tds[-1] + s[4])
    assert abs(tds[-1] - r.td) <= 1e-9 * r.td


def test_case_c_has_decisions_inside_the_approximate_stages_error():
    """What makes case c from the random start the test of the exact stage: a decision gap below the pair-tile bound's relative 2^-12."""
    r = reference('c', 'random')
    assert min(min(r.choice_gaps), min(r.stop_gaps)) < 2.0 ** -12


# ------------------------------------------------------------------------------------------------------------------------------------ brute force
def test_yardstick_against_brute_force_at_n_12():
    X = blobs(12, 3, 2, 1.5, 11)
    Dm = dist_matrix(X)
    td_of = lambda m: Dm[:, list(m)].min(axis=1).sum()
    all_pairs = {m: td_of(m) for m in itertools.combinations(range(12), 2)}
    assert len(all_pairs) == 66
    for init in (y_build(Dm, 2)[0], [0, 1], [5, 11]):
        r = y_pam(Dm, init)
        assert r.converged
        assert abs(r.td - td_of(r.medoids)) <= 1e-12 * r.td
        assert min(all_pairs.values()) <= r.td * (1 + 1e-12)
        for slot in range(2):                                  # no single swap improves the result
            for c in range(12):
                if c not in r.medoids:
                    m = list(r.medoids)
                    m[slot] = c
                    assert td_of(m) >= r.td * (1 - 1e-12)
        # Delta is the change of TD of the swap it stands for
        delta = y_delta(Dm, list(init))
        for c in range(12):
            if c in init:
                continue
            for slot in range(2):
                m = list(init)
                m[slot] = c
                assert abs(delta[c, slot] - (td_of(m) - td_of(init))) <= 1e-12 * td_of(init)


def test_build_prefix_property():
    Dm = matrix('e')
    full = y_build(Dm, 8)[0]
    for k in (1, 2, 5):
        assert y_build(Dm, k)[0] == full[:k]


def test_tie_rules_on_duplicated_rows():
    X, b = duplicates()
    Dm = dist_matrix(X)
    med, _, ties = y_build(Dm, 3)
    assert max(ties) == 2                                      # a duplicated best candidate ..
    for m in med:
        equal = np.flatnonzero((X == X[m]).all(axis=1))
        assert m == equal.min()                                # .. gives the smaller index
    # a duplicate of a medoid never swaps in: start from the copies, whose originals are then candidates with Delta(original, slot of the copy) = 0 exactly
    r = y_pam(Dm, [60, 61, 62])
    assert r.converged
    current = [60, 61, 62]
    for _, slot, out, cin, dl in r.swaps:
        assert not any((X[cin] == X[m]).all() for m in current)
        current[slot] = cin
    assert y_delta(Dm, [60, 61, 62])[b[0], 0] == 0.0


def test_k_1_and_k_n():
    X = blobs(40, 4, 2, 1.0, 13)
    Dm = dist_matrix(X)
    best = int(np.argmin(Dm.sum(axis=0)))
    assert y_build(Dm, 1)[0] == [best]
    r = y_pam(Dm, [best])
    assert r.converged and r.n_iter == 0 and not r.swaps and (r.labels == 0).all()
    other = (best + 1) % 40
    r = y_pam(Dm, [other])                                     # at K = 1 Delta(c, 0) = sum_o d(o, c) - TD: one swap to the best, then stop
    assert r.converged and r.n_iter == 1 and r.swaps[0][1:4] == (0, other, best) and r.medoids.tolist() == [best]
    r = y_pam(Dm, list(range(40)))
    assert r.converged and r.n_iter == 0 and r.td == 0.0 and r.labels.tolist() == list(range(40))
    assert sorted(y_build(Dm, 40)[0]) == list(range(40))


# ------------------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    X = np.zeros((5, 4), np.float32)
    for bad in (0, -1):
        with pytest.raises(ValueError, match='n_clusters must be >= 1'):
            KM.KMedoids(bad)
    for bad in (1.5, True, None):
        with pytest.raises(ValueError, match='n_clusters must be an int'):
            KM.KMedoids(bad)
    with pytest.raises(ValueError, match='n_clusters must be <= %d' % N.MAX_CLUSTERS):
        KM.KMedoids(N.MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match='n_samples'):
        KM.KMedoids(6).fit(X)
    with pytest.raises(ValueError, match='n_samples'):
        KM.kmedoids_sweep(X, [2, 6])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        KM.KMedoids(2).fit(np.zeros((5, 260), np.float32))
    with pytest.raises(ValueError, match='NaN'):
        KM.KMedoids(2).fit(np.array([[0, 1, 2, np.nan]] * 5, np.float32))
    with pytest.raises(ValueError, match='2-D'):
        KM.KMedoids(2).fit(np.zeros(5, np.float32))
    with pytest.raises(ValueError, match='at least 1 point'):
        KM.KMedoids(1).fit(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match='init must be one of'):
        KM.KMedoids(2, init='pam')
    with pytest.raises(ValueError, match='duplicate'):
        KM.KMedoids(2, init=[1, 1])
    with pytest.raises(ValueError, match='out of range'):
        KM.KMedoids(2, init=[-1, 1])
    with pytest.raises(ValueError, match='out of range'):
        KM.KMedoids(2, init=[0, 5]).fit(X)
    with pytest.raises(ValueError, match='row indices'):
        KM.KMedoids(2, init=[0, 1, 2])
    with pytest.raises(ValueError, match='row indices'):
        KM.KMedoids(2, init=[0.5, 1.0])
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='max_iter must be an int >= 0'):
            KM.KMedoids(2, max_iter=bad)
    with pytest.raises(RuntimeError, match='not fitted'):
        KM.KMedoids(2).predict(X)
    p = KM.KMedoids(3).get_params()
    assert (p['n_clusters'], p['init'], p['max_iter'], p['random_state']) == (3, 'build', 300, None)
    assert KM.kmedoids_sweep(X, []) == {}
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU'):
            KM.KMedoids(2).fit(X)


def test_module_does_not_import_scipy_or_sklearn():
    with open(KM.__file__) as f:
        text = f.read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', text, flags=re.M)


NAMES = {'dic_kmedoids_workspace': 2, 'dic_kmedoids_prepare': 9, 'dic_kmedoids_assign': 15, 'dic_kmedoids_delta_pass': 13, 'dic_kmedoids_select': 13,
         'dic_kmedoids_exact': 14, 'dic_kmedoids_pick': 7}


def test_header_and_signatures_agree():
    assert set(NAMES) <= set(N.header_symbols()) and set(NAMES) <= set(N.SIGNATURES)
    for name, n_args in NAMES.items():
        assert len(N.SIGNATURES[name][1]) == n_args
    assert set(N.header_symbols()) == set(N.SIGNATURES)
    with open(N.HEADER_PATH) as f:                           # the definition is stated in the header
        text = f.read()
    for phrase in ('k-medoids (PAM)', 'BUILD:', 'SWAP:', 'ties to the smaller c, then the smaller i'):
        assert phrase in text, phrase


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    odd = ctypes.c_void_p((1 << 20) + 2)
    big = 1 << 42

    def prepare(x=fake, ldx=8, n=1000, d=8, centre=fake, k=4, ws=fake, ws_bytes=big):
        return lib.dic_kmedoids_prepare(x, ldx, n, d, centre, k, ws, ws_bytes, None)

    def assign(q=fake, ldq=8, rows=500, d=8, x=fake, ldx=8, n=1000, med=fake, k=4, nearest=fake, dn=fake, ds=fake, dist=None, td=fake):
        return lib.dic_kmedoids_assign(q, ldq, rows, d, x, ldx, n, med, k, nearest, dn, ds, dist, td, None)

    def delta(n=1000, k_max=4, k=4, mode=2, nearest=fake, dn=fake, ds=fake, g=fake, r=fake, e=fake, ws=fake, ws_bytes=big):
        return lib.dic_kmedoids_delta_pass(n, k_max, k, mode, nearest, dn, ds, g, r, e, ws, ws_bytes, None)

    def select(n=1000, k_max=4, cols=4, g=fake, r=fake, e=fake, med=fake, n_med=4, lst=fake, count=fake, ws=fake, ws_bytes=big):
        return lib.dic_kmedoids_select(n, k_max, cols, g, r, e, med, n_med, lst, count, ws, ws_bytes, None)

    def exact(x=fake, ldx=8, n=1000, d=8, cand=fake, m=10, count=None, mode=2, nearest=fake, dn=fake, ds=fake, k=4, out=fake):
        return lib.dic_kmedoids_exact(x, ldx, n, d, cand, m, count, mode, nearest, dn, ds, k, out, None)

    def pick(cand=fake, m=10, count=None, table=fake, cols=4, out=fake):
        return lib.dic_kmedoids_pick(cand, m, count, table, cols, out, None)

    err = lib.dic_last_error_string
    K = N.MAX_CLUSTERS
    assert lib.dic_kmedoids_workspace(1000, 4) > 2 * 2 * (1024 + 4 * 256) * 288
    assert lib.dic_kmedoids_workspace(0, 4) == 0 and lib.dic_kmedoids_workspace(1000, 0) == 0 and lib.dic_kmedoids_workspace(1000, K + 1) == 0
    assert lib.dic_kmedoids_workspace(1 << 30, 4) == 0
    assert lib.dic_kmedoids_workspace(75000, 10) > lib.dic_kmedoids_workspace(75000, 4) > lib.dic_kmedoids_workspace(1000, 4)
    for call in (prepare, assign, exact):
        assert call(n=0) == -1 and call(d=0) == -1 and call(k=0) == -1
        wide = {'ldq': 260} if call is assign else {}
        assert call(d=260, ldx=260, **wide) == -2 and b'at most 256' in err()
        assert call(d=6) == -2 and b'multiples of 4' in err()
        assert call(x=odd) == -2 and b'aligned' in err()
        assert call(ldx=4) == -1 and call(x=None) == -1 and b'NULL' in err()
        assert call(k=K + 1) == -2
    assert prepare(ws_bytes=1000) == -3 and delta(ws_bytes=1000) == -3 and select(ws_bytes=1000) == -3 and b'workspace' in err()
    assert prepare(n=1 << 30) == -2 and prepare(centre=None) == -1 and prepare(ws=None) == -1 and prepare(centre=odd) == -2
    # assign
    assert assign(rows=0) == -1 and assign(ldq=4) == -1 and assign(q=None) == -1 and assign(med=None) == -1
    assert assign(nearest=None, dn=None, ds=None, td=None) == -1 and assign(dn=None) == -1 and b'td needs dn' in err()
    assert assign(nearest=None, dn=None, ds=None, td=None, dist=fake, k=K + 1) == -2          # (the distances alone are an output too)
    for kw in ({'q': odd}, {'dn': odd}, {'ds': odd}, {'td': odd}, {'nearest': odd}, {'med': odd}, {'dist': odd}):
        assert assign(**kw) == -2 and b'aligned' in err(), kw
    # delta pass
    assert delta(n=0) == -1 and delta(k=0) == -1 and delta(k=5) == -1 and delta(mode=3) == -1 and delta(mode=-1) == -1
    assert delta(k_max=K + 1, k=4) == -2 and delta(n=1 << 30) == -2
    for kw in ({'g': None}, {'e': None}, {'ws': None}, {'dn': None}, {'ds': None}, {'nearest': None}, {'r': None}):
        assert delta(**kw) == -1 and b'NULL' in err(), kw
    assert delta(mode=1, nearest=None, ds=None, r=None, ws_bytes=1000) == -3          # (BUILD needs dn alone; the first step not even that)
    assert delta(mode=0, nearest=None, dn=None, ds=None, r=None, ws_bytes=1000) == -3
    assert delta(mode=1, dn=None) == -1
    for kw in ({'g': odd}, {'r': odd}, {'e': odd}, {'dn': odd}, {'ds': odd}, {'nearest': odd}, {'ws': odd}):
        assert delta(**kw) == -2 and b'aligned' in err(), kw
    # select
    assert select(n=0) == -1 and select(cols=5) == -1 and select(cols=-1) == -1 and select(n_med=-1) == -1 and select(n_med=K + 1) == -1
    for kw in ({'g': None}, {'e': None}, {'r': None}, {'med': None}, {'lst': None}, {'count': None}, {'ws': None}):
        assert select(**kw) == -1 and b'NULL' in err(), kw
    assert select(cols=0, r=None, n_med=0, med=None, ws_bytes=1000) == -3
    for kw in ({'g': odd}, {'r': odd}, {'e': odd}, {'med': odd}, {'lst': odd}, {'count': odd}, {'ws': odd}):
        assert select(**kw) == -2 and b'aligned' in err(), kw
    # exact
    assert exact(m=0) == -1 and exact(mode=3) == -1 and exact(cand=None, m=1001) == -1 and b'candidate list' in err()
    for kw in ({'out': None}, {'dn': None}, {'ds': None}, {'nearest': None}):
        assert exact(**kw) == -1 and b'NULL' in err(), kw
    assert exact(mode=1, dn=None) == -1 and exact(n=1 << 30) == -2 and exact(m=1 << 30) == -2
    for kw in ({'out': odd}, {'dn': odd}, {'ds': odd}, {'nearest': odd}, {'cand': odd}, {'count': odd}):
        assert exact(**kw) == -2 and b'aligned' in err(), kw
    # pick
    assert pick(m=0) == -1 and pick(cols=0) == -1 and pick(cols=K + 1) == -1 and pick(m=1 << 30) == -2
    assert pick(table=None) == -1 and pick(out=None) == -1 and b'NULL' in err()
    for kw in ({'table': odd}, {'out': odd}, {'cand': odd}, {'count': odd}):
        assert pick(**kw) == -2 and b'aligned' in err(), kw


# ------------------------------------------------------------------------------------------------------------------------------------------ parsers
def test_p2_parser_accepts_kmedoids_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    a = p2.get_arguments([])
    assert (a.cluster_method, a.k_max, a.metric_sample) == ('kmeans', 10, 0)
    a = p2.get_arguments(['--cluster_method', 'kmedoids', '--k_max', '6'])
    assert (a.cluster_method, a.k_max) == ('kmedoids', 6)
    assert p2.Kmedoids.FILES == ('kmedoids_k.csv', 'kmedoids_labels.csv', 'kmedoids_medoids.csv')
    assert p2.Kmedoids.COLUMNS[:4] == ['k', 'inertia', 'n_iter', 'converged']
    assert p2.Kmedoids.MEDOID_COLUMNS == ['k', 'cluster', 'medoid_index', 'encounter_id']
    with pytest.raises(SystemExit):
        p2.get_arguments(['--cluster_method', 'kmedoid'])


def test_p4_parser_accepts_kmedoids_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p4.get_arguments([])
    assert (a.cluster_method, a.num_clusters) == ('kmeans', 4)
    a = p4.get_arguments(['--cluster_method', 'kmedoids', '--num_clusters', '3'])
    assert (a.cluster_method, a.num_clusters) == ('kmedoids', 3)
    with pytest.raises(SystemExit):
        p4.get_arguments(['--cluster_method', 'pam'])


# --------------------------------------------------------------------------------------------------------------------------------------- registers
def test_kmedoids_kernels_do_not_spill_to_scratch():
    """The delta epilogue runs 128 times per lane per tile beside 128 live accumulators: a register in scratch memory would be paid on every one.  Require
    ScratchSize == 0 and no vector-register spills for every kernel of dic_kmedoids.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_kmedoids.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'warning' not in res.stderr
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('km_delta_kernelILi0E', 'km_delta_kernelILi1E', 'km_delta_kernelILi2E', 'km_exact_kernelILi2E', 'km_assign_kernel', 'km_scatter_kernelILi2E',
                   'km_reduce_kernelILi2E', 'km_pick_kernel', 'pt_prep_kernel', 'pt_block_max_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
