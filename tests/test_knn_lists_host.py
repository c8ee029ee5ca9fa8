"""Neighbour lists, host side (no GPU): the numpy f64 yardstick of dic_knn_neighbors' definition against sklearn, the conditions the GPU tests
(tests/test_gpu_knn_lists.py) rely on, the vote yardstick against KNeighborsClassifier, the Python and ABI argument errors, and the kernels' register use.

Yardstick: d^2 in f64 difference form (every difference of two f32 is exact in f64; D squares summed), the k smallest keys (d^2, j) by ``np.lexsort``.

Yardstick against sklearn.  ``NearestNeighbors(algorithm='brute')`` on f64 input takes the NORM form |x|^2 + |y|^2 - 2 x.y on the raw (uncentred) points, so
the bar is not the 1e-13 of tests/test_gpu_knn.py alone but that plus the norm form's own rounding, computed from the data as test_gpu_knn.oracle_large does:
    |sk^2 - yard^2| <= 4 (D + 3) 2^-53 max|x|^2  +  (2 (D + 2) + 4) 2^-53 yard^2
-- each of |x|^2, |y|^2, x.y is a sum of D products (<= (D + 1) 2^-53 relative of the sum of magnitudes, <= max|x|^2 each, x.y counted twice), two more
additions; the second term is the difference form's own (D + 2) 2^-53, twice, and the square root and the squaring back (4 ulp).  On d itself that is
1e-13 relative wherever the points are not far from the origin compared with their distances."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn as K

EPS = 2.0 ** -53
GAP = 1e-12          # the GPU tests compare indices: no two of a row's first k + 1 yardstick d^2 may be closer than this, relative


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def kneighbors_exact(X, Q, k, with_d2=False):
    """``(dist (M, k) f64, idx (M, k) int32)``: the k rows of X with the smallest (d^2, j) for every row of Q (of X when Q is None), sorted by that key.
    ``with_d2``: also the first min(k + 1, N) sorted d^2 of every row."""
    X64 = np.asarray(X, dtype=np.float64)
    Q64 = X64 if Q is None else np.asarray(Q, dtype=np.float64)
    n, m = len(X64), len(Q64)
    dist, idx, head = np.empty((m, k)), np.empty((m, k), np.int32), np.empty((m, min(k + 1, n)))
    jj = np.arange(n)
    step = max(1, (1 << 24) // max(1, n * X64.shape[1]))
    for s in range(0, m, step):
        diff = Q64[s:s + step, None, :] - X64[None, :, :]
        d2 = np.einsum('ijk,ijk->ij', diff, diff)
        order = np.lexsort((np.broadcast_to(jj, d2.shape), d2), axis=1)
        srt = np.take_along_axis(d2, order, 1)
        dist[s:s + step] = np.sqrt(srt[:, :k])
        idx[s:s + step] = order[:, :k]
        head[s:s + step] = srt[:, :head.shape[1]]
    return (dist, idx, head) if with_d2 else (dist, idx)


def vote_exact(idx, labels, k=None):
    """``(labels (M,) int32, share (M,) f32)``: the most frequent label among labels[idx[q]], the smallest label on equal votes, and its share of the votes."""
    labels = np.asarray(labels)
    classes = np.unique(labels)
    tally = (labels[idx][:, :, None] == classes[None, None, :]).sum(1)
    win = tally.argmax(1)          # the first maximum: the smallest label
    return classes[win].astype(np.int32), (tally.max(1).astype(np.float32) / np.float32(idx.shape[1]))


def blobs(n, d, n_centres, spread, noise_frac, seed, offset=0.0):
    """The recipe of tests/test_gpu_knn.py: gaussian blobs plus uniform background noise, shuffled."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (n_centres, d)) * 4.0
    m = int(n * (1 - noise_frac))
    X = centres[rng.integers(0, n_centres, m)] + rng.normal(0, spread, (m, d))
    noise = rng.uniform(centres.min(0) - 1, centres.max(0) + 1, (n - m, d))
    return (rng.permutation(np.concatenate([X, noise])) + offset).astype(np.float32)


def _cross(n, m, d, seed, **kw):
    P = blobs(n + m, d, 3, 0.5, 0.1, seed, **kw)
    X, Q = P[:n].copy(), P[n:].copy()
    Q[0] = X[min(3, n - 1)]          # a query equal to an index point
    return X, Q


def lattice():
    g = np.arange(6, dtype=np.float32)
    P = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    return np.concatenate([P, np.zeros((len(P), 1), np.float32)], 1)          # 6^3 points, D = 4


def duplicates():
    X = blobs(200, 12, 3, 0.5, 0.1, 7)
    X[100:140] = X[17]          # 40 copies of one point (41 with the original)
    return X


# name -> (X, Q or None, k).  Random cases: the GPU tests compare them by index, test_conditions_of_the_random_cases holds the seeds to that.
SELF = {'n1000_d32_k7': (1000, 32, 7), 'n257_d16_k4': (257, 16, 4), 'n100_d8_k3': (100, 8, 3), 'n5_d4_k5': (5, 4, 5), 'n1_d4_k1': (1, 4, 1),
        'n600_d256_k257': (600, 256, 257)}
CROSS = {'n300_m70': (300, 70, 5), 'n256_m256': (256, 256, 5), 'n70_m600': (70, 600, 5), 'n1000_m1': (1000, 1, 5), 'n1_m5': (1, 5, 1)}
RANDOM = sorted(SELF) + sorted(CROSS) + ['far_self', 'far_cross']
TIES = ['lattice_self', 'lattice_cross', 'dup_k10', 'dup_k60']


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SELF:
        n, d, k = SELF[name]
        return blobs(n, d, 4, 0.5, 0.1, 100 + n), None, k
    if name in CROSS:
        n, m, k = CROSS[name]
        return _cross(n, m, 16, 200 + n + m) + (k,)
    if name == 'far_self':          # points far from their mean: offset 1e3, spread 1
        return blobs(400, 16, 3, 1.0, 0.1, 31, offset=1e3), None, 6
    if name == 'far_cross':
        return _cross(300, 90, 16, 32, offset=1e3) + (6,)
    if name == 'lattice_self':
        return lattice(), None, 9
    if name == 'lattice_cross':
        L = lattice()
        return L, np.concatenate([L[::5], L[::7] + np.float32(0.5)]).astype(np.float32), 9
    if name in ('dup_k10', 'dup_k60'):
        return duplicates(), None, int(name[5:])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def yard(name):
    """(dist, idx, first k + 1 sorted d^2) of a case: computed once, shared by every test; read-only."""
    X, Q, k = case(name)
    out = kneighbors_exact(X, Q, k, with_d2=True)
    for a in out:
        a.setflags(write=False)
    return out


def rel_gaps(head):
    """(M,) the smallest relative gap between consecutive entries of each row (inf for a single entry)."""
    if head.shape[1] < 2:
        return np.full(len(head), np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = (head[:, 1:] - head[:, :-1]) / head[:, 1:]
    return np.where(np.isnan(g), 0.0, g).min(1)


@pytest.mark.parametrize('name', RANDOM)
def test_conditions_of_the_random_cases(name):
    X, Q, k = case(name)
    dist, idx, head = yard(name)
    gaps = rel_gaps(head)
    print('%s: smallest relative gap of the first k + 1 d^2 over %d rows: %.3g' % (name, len(gaps), gaps.min()))
    assert gaps.min() > GAP          # every row is compared by index: none is left out
    assert dist.shape == idx.shape == (len(X if Q is None else Q), k) and (np.diff(dist, axis=1) >= 0).all()
    if Q is None:
        assert (idx[:, 0] == np.arange(len(X))).all() and (dist[:, 0] == 0).all()
    else:
        assert dist[0, 0] == 0 and idx[0, 0] == min(3, len(X) - 1)


@pytest.mark.parametrize('name', TIES)
def test_tie_cases_have_ties(name):
    X, Q, k = case(name)
    dist, idx, head = yard(name)
    assert (rel_gaps(head) == 0).any()
    if name.startswith('lattice'):          # small integers (quarter-integers for the shifted queries): every d^2 exact in any summation order
        assert np.array_equal(head * 4, np.round(head * 4))
    tied = dist[:, 1:] == dist[:, :-1]
    assert (np.diff(idx.astype(np.int64), axis=1)[tied] > 0).all()          # ties are in index order


@pytest.mark.parametrize('name', RANDOM + TIES)
def test_yardstick_against_sklearn(name):
    neighbors = pytest.importorskip('sklearn.neighbors')
    X, Q, k = case(name)
    dist, idx, head = yard(name)
    X64 = X.astype(np.float64)
    Q64 = X64 if Q is None else Q.astype(np.float64)
    sk_d, sk_i = neighbors.NearestNeighbors(n_neighbors=k, algorithm='brute').fit(X64).kneighbors(Q64)
    D = X.shape[1]
    nmax = max((X64 ** 2).sum(1).max(), (Q64 ** 2).sum(1).max())
    bar = 4 * (D + 3) * EPS * nmax + (2 * (D + 2) + 4) * EPS * dist ** 2          # on d^2: the module docstring
    err = np.abs(sk_d ** 2 - dist ** 2)
    print('%s: worst |sk^2 - yard^2| / bar = %.3g' % (name, (err / bar).max()))
    assert (err <= bar).all()
    # indices: on every row whose consecutive d^2 differ by more than the two roundings
    width = 4 * (D + 3) * EPS * nmax + (2 * (D + 2) + 4) * EPS * head
    clear = ((head[:, 1:] - head[:, :-1]) > width[:, 1:] + width[:, :-1]).all(1) if head.shape[1] > 1 else np.ones(len(head), bool)
    print('%s: %d of %d rows compared by index' % (name, int(clear.sum()), len(clear)))
    if name in RANDOM:
        assert clear.mean() > 0.5
    assert np.array_equal(sk_i[clear], idx[clear])


def _labelled(seed=5):
    """Blobs that carry DBSCAN-like labels: three clusters 0..2 whose outer shell (the quarter of the points farthest from their centre) is noise, -1;
    queries from the same recipe."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 4.0, (3, 8))
    lab = rng.integers(0, 3, 500)
    off = rng.normal(0, 0.6, (500, 8))
    r = np.linalg.norm(off, axis=1)
    P = (centres[lab] + off).astype(np.float32)
    lab[r > np.quantile(r, 0.75)] = -1
    return P[:380], lab[:380], P[380:]


def _forced_tie():
    """One query at the origin, k = 4: two votes for label 2 (distance 1), two for label -1 (distance 1.5), label 0 far away: -1, the smaller, wins."""
    X = np.zeros((7, 4), np.float32)
    X[0, 0], X[1, 0], X[2, 1], X[3, 1] = 1, -1, 1.5, -1.5
    X[4:, 2] = (5, 6, 7)
    return X, np.array([2, 2, -1, -1, 0, 0, 0]), np.zeros((1, 4), np.float32), 4


def test_vote_yardstick_against_sklearn():
    neighbors = pytest.importorskip('sklearn.neighbors')
    X, y, Q = _labelled()
    for k in (1, 5, 9):
        _, idx = kneighbors_exact(X, Q, k)
        lab, share = vote_exact(idx, y)
        ref = neighbors.KNeighborsClassifier(n_neighbors=k, algorithm='brute').fit(X.astype(np.float64), y).predict(Q.astype(np.float64))
        assert np.array_equal(lab, ref) and (lab == -1).any() and set(lab.tolist()) == {-1, 0, 1, 2}
        assert share.dtype == np.float32 and (share > 0).all() and (share <= 1).all() and (k > 1 or (share == 1).all())
    X, y, Q, k = _forced_tie()
    _, idx = kneighbors_exact(X, Q, k)
    lab, share = vote_exact(idx, y)
    ref = neighbors.KNeighborsClassifier(n_neighbors=k, algorithm='brute').fit(X.astype(np.float64), y).predict(Q.astype(np.float64))
    assert sorted(idx[0].tolist()) == [0, 1, 2, 3] and lab.tolist() == ref.tolist() == [-1] and share.tolist() == [0.5]


def test_argument_errors():
    X = np.zeros((5, 4), np.float32)
    with pytest.raises(ValueError, match='Expected n_neighbors > 0. Got 0'):
        K.kneighbors(X, 0)
    with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit, but n_neighbors = 6, n_samples_fit = 5, n_samples = 5'):
        K.kneighbors(X, 6)
    with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit, but n_neighbors = 6, n_samples_fit = 5, n_samples = 2'):
        K.kneighbors(X, 6, Q=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match='X has 3 features, but NearestNeighbors is expecting 4 features as input'):
        K.kneighbors(X, 2, Q=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match='2-D'):
        K.kneighbors(np.zeros(5, np.float32), 2)
    with pytest.raises(ValueError, match='candidate_budget'):
        K.kneighbors(X, 2, candidate_budget=0)
    with pytest.raises(NotImplementedError, match='at most 1024 neighbours'):
        K.kneighbors(np.zeros((1100, 4), np.float32), 1025)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        K.kneighbors(np.zeros((5, 260), np.float32), 2)
    nn = K.NearestNeighbors()
    assert nn.n_neighbors == 5
    with pytest.raises(RuntimeError, match='not fitted'):
        nn.kneighbors()
    with pytest.raises(ValueError, match='Expected n_neighbors > 0. Got 0'):
        K.NearestNeighbors(0).fit(X)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        K.NearestNeighbors().fit(np.zeros((5, 260), np.float32))
    nn.fit(X)
    with pytest.raises(ValueError, match='Expected n_neighbors < n_samples_fit, but n_neighbors = 5, n_samples_fit = 5, n_samples = 5'):
        nn.kneighbors()          # the point itself does not count: 5 neighbours need 6 points
    with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit, but n_neighbors = 6, n_samples_fit = 5, n_samples = 5'):
        nn.kneighbors(X, n_neighbors=6)
    with pytest.raises(ValueError, match='Expected n_neighbors > 0. Got 0'):
        nn.kneighbors(X, n_neighbors=0)
    with pytest.raises(ValueError, match='X has 8 features, but NearestNeighbors is expecting 4 features as input'):
        nn.kneighbors(np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match='Unsupported mode'):
        nn.kneighbors_graph(X, mode='weights')
    with pytest.raises(ValueError, match='inconsistent numbers of samples'):
        K.knn_transfer_labels(X, np.zeros(4, np.int64), X, 2)
    with pytest.raises(ValueError, match='integers'):
        K.knn_transfer_labels(X, np.zeros(5, np.float64), X, 2)
    with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit'):
        K.knn_transfer_labels(X, np.zeros(5, np.int64), X, 6)
    with pytest.raises(NotImplementedError, match='at most 1024 neighbours'):
        K.knn_transfer_labels(np.zeros((1100, 4), np.float32), np.zeros(1100, np.int64), X, 1025)
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU path'):
            K.kneighbors(X, 2)


def test_sklearn_words_the_errors_the_same_way():
    neighbors = pytest.importorskip('sklearn.neighbors')
    X = np.zeros((5, 4))
    sk = neighbors.NearestNeighbors(n_neighbors=5, algorithm='brute').fit(X)
    ours = K.NearestNeighbors(5).fit(X.astype(np.float32))
    for call in (lambda nn: nn.kneighbors(), lambda nn: nn.kneighbors(X, n_neighbors=6), lambda nn: nn.kneighbors(X, n_neighbors=0),
                 lambda nn: nn.kneighbors(np.zeros((2, 8)))):
        with pytest.raises(ValueError) as a:
            call(sk)
        with pytest.raises(ValueError) as b:
            call(ours)
        assert str(b.value).rstrip('.') in str(a.value)


def test_module_does_not_import_scipy_or_sklearn():
    with open(K.__file__) as f:
        top = re.findall(r'^(?:import|from)\s+(\S+)', f.read(), flags=re.M)          # (kneedle_elbow's scipy.signal import is inside the function, as before)
    assert top and not any(m.split('.')[0] in ('scipy', 'sklearn') for m in top)
    import inspect
    for fn in (K.kneighbors, K.NearestNeighbors, K.knn_transfer_labels):
        assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', inspect.getsource(fn), flags=re.M)


def test_p4_parser_accepts_the_transfer_flags():
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p4.get_arguments([])
    assert a.transfer == 'centre' and a.transfer_k is None and a.cluster_method == 'kmeans'
    a = p4.get_arguments(['--cluster_method', 'hdbscan', '--transfer', 'knn', '--transfer_k', '9'])
    assert (a.cluster_method, a.transfer, a.transfer_k) == ('hdbscan', 'knn', 9)
    assert p4.get_arguments(['--cluster_method', 'dbscan', '--transfer', 'knn']).transfer_k is None          # feat_dim + 1
    with pytest.raises(SystemExit):
        p4.get_arguments(['--transfer', 'nearest'])


def test_p4_refuses_knn_transfer_for_other_methods(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    monkeypatch.chdir(tmp_path)
    for method in ('kmeans', 'ward', 'gmm', 'consensus', 'dl'):
        args = p4.get_arguments(['--cluster_method', method, '--transfer', 'knn'])
        with pytest.raises(ValueError, match='--transfer knn applies to --cluster_method dbscan and hdbscan only'):
            p4.main(args)
    assert not (tmp_path / 'Results').exists()


def test_header_and_signatures_agree():
    names = {'dic_knn_neighbors_workspace', 'dic_knn_neighbors'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    assert len(N.SIGNATURES['dic_knn_neighbors'][1]) == 16 and len(N.SIGNATURES['dic_knn_neighbors_workspace'][1]) == 4


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_knn_neighbors_workspace(1000, 200, 16, 0)
    assert ws > 2 * 2 * (1200 + 256) * 288 * 2          # at least the four planes of the stacked set
    assert lib.dic_knn_neighbors_workspace(1000, 0, 16, 0) == lib.dic_knn_workspace(1000, 16, 0)
    assert lib.dic_knn_neighbors_workspace(1000, 200, 16, 1 << 20) < ws          # the budget sizes the lists
    for bad in ((0, 0, 16, 0), (1000, -1, 16, 0), (1 << 29, 1 << 29, 16, 0), (1000, 0, 0, 0), (1000, 0, 260, 0)):
        assert lib.dic_knn_neighbors_workspace(*bad) == 0

    def call(X=fake, ldx=16, n=1000, Q=fake, ldq=16, m=200, centre=fake, d=16, k=5, dist=fake, idx=fake, budget=0, work=fake, nbytes=ws):
        return lib.dic_knn_neighbors(X, ldx, n, Q, ldq, m, centre, d, k, dist, idx, budget, None, work, nbytes, None)

    for kw in ({'X': None}, {'centre': None}, {'dist': None}, {'idx': None}, {'work': None}):
        assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
    for kw in ({'k': 0}, {'k': -3}, {'k': 1001}, {'n': 0}, {'m': 0}, {'ldx': 8}, {'ldq': 8}, {'d': 0}):
        assert call(**kw) in (-1, -2), kw
    assert call(k=0) == -1 and b'expected 1 <= k <= N' in lib.dic_last_error_string()
    assert call(k=1001) == -1 and b'expected 1 <= k <= N' in lib.dic_last_error_string()
    assert call(n=2000, k=1025, nbytes=1 << 40) == -2 and b'at most 1024 neighbours' in lib.dic_last_error_string()
    assert call(ldx=6, ldq=6, d=6) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=18) == -2 and call(ldq=18) == -2
    assert call(ldx=260, ldq=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
    assert call(n=1 << 29, m=1 << 29) == -2 and b'2^30' in lib.dic_last_error_string()
    for kw in ({'X': ctypes.c_void_p((1 << 20) + 4)}, {'Q': ctypes.c_void_p((1 << 20) + 4)}, {'work': ctypes.c_void_p((1 << 20) + 8)},
               {'dist': ctypes.c_void_p((1 << 20) + 4)}):
        assert call(**kw) == -2 and b'aligned' in lib.dic_last_error_string()
    assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()
    # the self join: Q = NULL, M and ldq ignored; its workspace is the smaller one
    ws_self = lib.dic_knn_neighbors_workspace(1000, 0, 16, 0)
    assert call(Q=None, m=12345, ldq=0, nbytes=ws_self - 1) == -3 and call(Q=None, k=1001, nbytes=ws_self) == -1


def test_neighbour_list_kernels_do_not_spill_to_scratch():
    """The exact stage runs once per row with its keys in LDS, and the list passes reuse the counting and gather tile kernels, which leave the product loop
    a handful of registers: a register in scratch memory would be paid on every tile.  Require ScratchSize == 0 and no vector-register spills for every
    kernel of dic_knn.hip, the three new ones by name."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_knn.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('knl_exact_kernel', 'kn_window_kernel', 'pt_mask_cols_kernel', 'kn_count_kernel', 'kn_gather_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
