"""Shared-nearest-neighbour clustering, host side (no GPU): the numpy yardstick of the definition in include/dic_hip.h (dic_snn_similarity), written twice,
the cases the GPU tests (tests/test_gpu_snn.py) run and the conditions that make them worth running, the yardstick against sklearn's DBSCAN on the dense
dissimilarity, the Python and ABI argument errors, the parsers, and the kernels' register use.

Yardstick.  Lists: ``test_knn_lists_host.kneighbors_exact`` (f64 difference form, the k smallest (d^2, j)).  Similarity, form (a): Python sets per row; form
(b): the membership matrix M (N x N, 0/1), G = M M^T in f32 (sums of at most 1024 ones: exact below 2^24), read at ``idx`` and masked by mutuality.
Labels: union-find over the strong core-core edges, clusters numbered by their smallest core index, border points by (sim descending, j ascending).
Everything is an integer, so the GPU tests demand equality."""
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
from deep_interpolation_clustering_amd import snn as S
from test_knn_lists_host import GAP, kneighbors_exact


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


# ---------------------------------------------------------------------------------------------------------------------------------- the yardstick
def sim_sets(idx, rows=None):
    """Form (a): ``sim[rows]`` (all rows when None) from Python sets."""
    n, k = idx.shape
    sets = [set(r.tolist()) for r in idx]
    rows = range(n) if rows is None else rows
    out = np.zeros((len(rows), k), np.int32)
    for a, i in enumerate(rows):
        for c in range(k):
            j = int(idx[i, c])
            if j != i and i in sets[j]:
                out[a, c] = len(sets[i] & sets[j])
    return out


def membership(idx):
    n = len(idx)
    M = np.zeros((n, n), np.float32)
    M[np.arange(n)[:, None], idx] = 1
    return M


def mutual_mask(idx, M=None):
    """(N, k) bool: j = idx[i, c] is another point and has i in its own list."""
    M = membership(idx) if M is None else M
    ii = np.arange(len(idx))[:, None]
    return (M[idx, ii] > 0) & (idx != ii)


def sim_matrix(idx):
    """Form (b): M M^T read at idx, masked by mutuality."""
    n, k = idx.shape
    M = membership(idx)
    G = M @ M.T
    assert k < 2 ** 24
    return np.where(mutual_mask(idx, M), G[np.arange(n)[:, None], idx], 0).astype(np.int32)


def snn_labels_exact(idx, sim, eps, min_samples):
    """``(labels int64, core indices int64, density int32, border ties)``: ``border ties`` = the border points whose largest sim is shared by two cores."""
    n, k = idx.shape
    strong = sim >= eps
    density = strong.sum(1).astype(np.int32)
    core = density >= min_samples
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in np.flatnonzero(core):
        for j in idx[i][strong[i] & core[idx[i]]]:
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)          # the root is the smallest index
    labels = np.full(n, -1, np.int64)
    roots = np.array([find(i) for i in np.flatnonzero(core)], dtype=np.int64)
    ranks = {r: q for q, r in enumerate(np.unique(roots))}
    labels[core] = [ranks[r] for r in roots]
    ties = 0
    for i in np.flatnonzero(~core):
        ok = strong[i] & core[idx[i]]
        if ok.any():
            s, j = sim[i][ok], idx[i][ok]
            best = j[s == s.max()]
            ties += len(best) > 1
            labels[i] = labels[best.min()]
    return labels, np.flatnonzero(core).astype(np.int64), density, int(ties)


# ---------------------------------------------------------------------------------------------------------------------------------------- the cases
def blobs3(n, d, seed):
    """Three gaussian blobs of unequal spread (0.4, 0.8, 1.2), a tenth of the points uniform noise, one triple of exact duplicates; shuffled."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 1, (3, d)) * 6.0 / np.sqrt(d / 8.0)
    m = n - n // 10
    which = rng.integers(0, 3, m)
    X = centres[which] + rng.normal(0, 1, (m, d)) * np.array([0.4, 0.8, 1.2])[which, None] / np.sqrt(d / 8.0)
    noise = rng.uniform(centres.min(0) - 2, centres.max(0) + 2, (n - m, d))
    X = rng.permutation(np.concatenate([X, noise])).astype(np.float32)
    a, b, c = rng.choice(n, 3, replace=False)
    X[b] = X[c] = X[a]
    return X


def chain(seed=3):
    """Two noisy parallel lines of 200 points each, 50 apart, rows shuffled."""
    rng = np.random.default_rng(seed)
    P = np.zeros((400, 4))
    P[:, 0] = np.tile(np.arange(200.0), 2)
    P[200:, 1] = 50.0
    P += rng.normal(0, 0.05, P.shape)
    return rng.permutation(P).astype(np.float32)


# name -> (N, D, k, eps, min_samples, clustering case?).  eps / min_samples of the cases that only check the similarity and one labelling are this file's choice
CASES = {
    'n2_k2': (2, 4, 2, 2, 1, False),
    'n5_k5': (5, 4, 5, 5, 2, False),
    'n65_d8_k8': (65, 8, 8, 4, 4, True),
    'n130_d256_k16': (130, 256, 16, 7, 6, True),
    'n1030_d12_k64': (1030, 12, 64, 24, 32, True),
    'n1600_d8_k257': (1600, 8, 257, 150, 200, True),
    'n1200_d8_k1024': (1200, 8, 1024, 980, 300, False),
    'chain400_k6': (400, 4, 6, 3, 2, True),
}
BLOBS = ['n65_d8_k8', 'n130_d256_k16', 'n1030_d12_k64', 'n1600_d8_k257']
CLUSTERING = [c for c in CASES if CASES[c][5]]
SEEDS = {'n65_d8_k8': 1, 'n130_d256_k16': 2, 'n1030_d12_k64': 3, 'n1600_d8_k257': 4, 'n1200_d8_k1024': 5}


@functools.lru_cache(maxsize=None)
def points(name):
    n, d = CASES[name][:2]
    if name == 'chain400_k6':
        X = chain()
    elif name in SEEDS:
        X = blobs3(n, d, SEEDS[name])
    else:
        X = np.random.default_rng(n).normal(0, 1, (n, d)).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def lists(name):
    """(idx (N, k), the k + 1 nearest (N, min(k + 1, N)), their sorted d^2): computed once, shared, read-only."""
    X, k = points(name), CASES[name][2]
    _, wide, head = kneighbors_exact(X, None, min(k + 1, len(X)), with_d2=True)
    idx, head = np.ascontiguousarray(wide[:, :k]), np.ascontiguousarray(head[:, :wide.shape[1]])
    for a in (idx, wide, head):
        a.setflags(write=False)
    return idx, wide, head


@functools.lru_cache(maxsize=None)
def yard(name, eps=None, min_samples=None):
    """(idx, sim, labels, core indices, density, border ties) of a case (at another eps / min_samples if given): computed once, shared, read-only."""
    idx = lists(name)[0]
    sim = sim_matrix(idx) if eps is None and min_samples is None else yard(name)[1]
    e, ms = CASES[name][3:5]
    out = (idx, sim) + snn_labels_exact(idx, sim, e if eps is None else eps, ms if min_samples is None else min_samples)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def strong_core_graph(name):
    idx, sim, labels, core_idx, density, _ = yard(name)
    core = np.zeros(len(idx), bool)
    core[core_idx] = True
    eps = CASES[name][3]
    return [idx[i][(sim[i] >= eps) & core[idx[i]]] if core[i] else [] for i in range(len(idx))], core


def eccentricity(adj, start):
    depth = {start: 0}
    frontier = [start]
    while frontier:
        nxt = []
        for a in frontier:
            for b in adj[a]:
                if int(b) not in depth:
                    depth[int(b)] = depth[a] + 1
                    nxt.append(int(b))
        frontier = nxt
    far = max(depth, key=depth.get)
    return far, depth[far]


# ------------------------------------------------------------------------------------------------------------------- the conditions on the yardstick
@pytest.mark.parametrize('name', list(CASES))
def test_conditions_of_the_cases(name):
    n, d, k, eps, ms, clustering = CASES[name]
    X = points(name)
    idx, wide, head = lists(name)
    _, sim, labels, core_idx, density, ties = yard(name)
    assert X.shape == (n, d) and idx.shape == sim.shape == (n, k)
    # the first k + 1 exact d^2 of every row are apart by GAP, exact duplicates excepted (settled by index in the yardstick and on the GPU alike)
    with np.errstate(divide='ignore', invalid='ignore'):
        gap = (head[:, 1:] - head[:, :-1]) / head[:, 1:]
    close = ~(gap > GAP)
    same = (X[wide[:, 1:]] == X[wide[:, :-1]]).all(-1)
    assert (same | ~close).all() and (np.diff(wide.astype(np.int64), axis=1)[close] > 0).all()
    n_clusters = labels.max() + 1
    border = (labels >= 0) & ~np.isin(np.arange(n), core_idx)
    non_mutual = int(((sim == 0) & (idx != np.arange(n)[:, None])).sum())
    print('%s: %d clusters, sizes %s, %d noise, %d border (%d ties), %d cores, %d non-mutual entries, sim max %d'
          % (name, n_clusters, np.bincount(labels[labels >= 0]).tolist(), (labels < 0).sum(), border.sum(), ties, len(core_idx), non_mutual, sim.max()))
    if name == 'n5_k5':
        assert (sim[idx != np.arange(n)[:, None]] == n).all() and (sim[idx == np.arange(n)[:, None]] == 0).all()
    if name not in ('n5_k5', 'n2_k2'):
        assert non_mutual > 0
    if clustering:
        assert n_clusters >= 2
    if name in BLOBS:
        assert (labels < 0).any() and border.any()
        assert sum((X == X[i]).all(1).sum() == 3 for i in range(n)) == 3          # the triple
    if n >= 130 and name != 'chain400_k6':          # (every point of the chain is a core point at its eps and min_samples: it has no border at all)
        assert ties >= 1
    if name == 'chain400_k6':
        adj, core = strong_core_graph(name)
        for root in np.unique(labels[core_idx]):
            start = int(core_idx[labels[core_idx] == root][0])
            far, _ = eccentricity(adj, start)
            assert eccentricity(adj, far)[1] >= 50          # (a lower bound of the diameter: the eccentricity of one vertex)


# ------------------------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('name', list(CASES))
def test_the_two_yardstick_forms_agree(name):
    idx, sim = yard(name)[:2]
    rows = range(len(idx)) if idx.size <= 70000 else range(0, len(idx), 7)          # (form (a) is per row: a seventh of the rows of the two large cases)
    assert np.array_equal(sim_sets(idx, rows), sim[list(rows)])


@pytest.mark.parametrize('name', list(CASES))
def test_similarity_is_symmetric(name):
    idx, sim = yard(name)[:2]
    n = len(idx)
    dense = np.zeros((n, n), np.int32)
    dense[np.arange(n)[:, None], idx] = sim
    assert np.array_equal(dense, dense.T) and (np.diag(dense) == 0).all()
    assert sim.min() >= 0 and sim.max() <= idx.shape[1]


def _components(adj_dense):
    n = len(adj_dense)
    lab = np.full(n, -1)
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = s
        stack = [s]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(adj_dense[a]):
                if lab[b] < 0:
                    lab[b] = s
                    stack.append(b)
    return np.unique(lab, return_inverse=True)[1]          # numbered by the smallest member


@pytest.mark.parametrize('name', [c for c in CASES if c != 'n1200_d8_k1024'])
def test_min_samples_zero_is_jarvis_patrick(name):
    n, _, k, eps = CASES[name][:4]
    idx, sim, labels, core_idx, density, _ = yard(name, eps, 0)
    dense = np.zeros((n, n), bool)
    dense[np.arange(n)[:, None], idx] = sim >= eps
    assert len(core_idx) == n and (labels >= 0).all()
    assert np.array_equal(labels, _components(dense))
    assert (np.bincount(labels)[labels[density == 0]] == 1).all()          # isolated points are singleton clusters


@pytest.mark.parametrize('name', CLUSTERING)
def test_yardstick_against_sklearn_dbscan_on_the_dense_dissimilarity(name):
    cluster = pytest.importorskip('sklearn.cluster')
    n, _, k, eps, ms, _ = CASES[name]
    idx, sim, labels, core_idx, _, _ = yard(name)
    dis = np.full((n, n), float(k + 1))
    ii = np.arange(n)[:, None]
    mutual = mutual_mask(idx)          # the other pairs stay at k + 1
    dis[np.broadcast_to(ii, idx.shape)[mutual], idx[mutual]] = (k - sim[mutual]).astype(np.float64)
    np.fill_diagonal(dis, 0.0)
    sk = cluster.DBSCAN(eps=k - eps, min_samples=ms + 1, metric='precomputed').fit(dis)          # (sklearn counts the point itself)
    assert np.array_equal(sk.core_sample_indices_, core_idx)
    assert np.array_equal(sk.labels_[core_idx], labels[core_idx])          # border points: sklearn assigns them first-come, not compared
    assert ((sk.labels_ >= 0) == (labels >= 0)).all()


# ------------------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors():
    X = np.zeros((5, 4), np.float32)
    for call in (lambda **kw: S.snn_graph(X, **kw), lambda **kw: S.snn_sweep(X, eps_values=[2], min_samples=1, **kw),
                 lambda **kw: S.SNN(eps=2, min_samples=1, **kw).fit(X)):
        with pytest.raises(ValueError, match='n_neighbors must be >= 2'):
            call(n_neighbors=1)
        with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples_fit, but n_neighbors = 6, n_samples_fit = 5, n_samples = 5'):
            call(n_neighbors=6)
        with pytest.raises(ValueError, match='candidate_budget'):
            call(n_neighbors=3, candidate_budget=0)
        with pytest.raises(ValueError, match='integer'):
            call(n_neighbors=2.5)
    with pytest.raises(NotImplementedError, match='at most 1024 neighbours'):
        S.snn_graph(np.zeros((1100, 4), np.float32), 1025)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        S.snn_graph(np.zeros((5, 260), np.float32), 2)
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        S.SNN(2, 1, 1).fit(torch.zeros(5, 260))
    with pytest.raises(ValueError, match='2-D'):
        S.snn_graph(np.zeros(5, np.float32), 2)
    for eps in (0, 4, 1.5):
        with pytest.raises(ValueError, match='eps must'):
            S.snn_sweep(X, 3, [2, eps], 1)
        with pytest.raises(ValueError, match='eps must'):
            S.SNN(3, eps, 1).fit(X)
    for ms in (-1, 0.5):
        with pytest.raises(ValueError, match='min_samples must be an integer >= 0'):
            S.snn_sweep(X, 3, [2], ms)
    idx = np.zeros((5, 3), np.int32)
    with pytest.raises(ValueError, match='one shape'):
        S.snn_labels(idx, np.zeros((5, 2), np.int32), 1, 1)
    with pytest.raises(ValueError, match='2-D'):
        S.snn_labels(idx.ravel(), idx.ravel(), 1, 1)
    with pytest.raises(ValueError, match='integers'):
        S.snn_labels(idx, idx.astype(np.float32), 1, 1)
    with pytest.raises(ValueError, match='expected 2 <= n_neighbors <= n_samples'):
        S.snn_labels(np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32), 1, 1)
    with pytest.raises(NotImplementedError, match='at most 1024 neighbours'):
        S.snn_labels(torch.zeros((1100, 1025), dtype=torch.int32), torch.zeros((1100, 1025), dtype=torch.int32), 1, 1)
    with pytest.raises(ValueError, match='eps must lie in'):
        S.snn_labels(torch.zeros((5, 3), dtype=torch.int32), torch.zeros((5, 3), dtype=torch.int32), 4, 1)
    with pytest.raises(ValueError, match='min_samples'):
        S.snn_labels(idx, idx, 1, -1)
    with pytest.raises(AttributeError, match='not fitted'):
        S.SNN().similarity_
    if not torch.cuda.is_available():          # and no quiet CPU path
        with pytest.raises(RuntimeError, match='no CPU path'):
            S.snn_graph(X, 2)
        with pytest.raises(RuntimeError, match='no CPU path'):
            S.snn_labels(idx, idx, 1, 1)


def test_module_does_not_import_scipy_or_sklearn():
    with open(S.__file__) as f:
        text = f.read()
    assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', text, flags=re.M)


def test_header_and_signatures_agree():
    names = {'dic_snn_similarity', 'dic_snn_components_pass'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)
    assert len(N.SIGNATURES['dic_snn_similarity'][1]) == 5 and len(N.SIGNATURES['dic_snn_components_pass'][1]) == 11
    assert set(N.header_symbols()) == set(N.SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    odd = ctypes.c_void_p((1 << 20) + 2)

    def similarity(idx=fake, n=1000, k=16, sim=fake):
        return lib.dic_snn_similarity(idx, n, k, sim, None)

    def components(idx=fake, sim=fake, n=1000, k=16, eps=8, density=fake, ms=4, labels=fake, border=fake, changed=fake):
        return lib.dic_snn_components_pass(idx, sim, n, k, eps, density, ms, labels, border, changed, None)

    for call in (similarity, components):
        for kw in ({'idx': None}, {'sim': None}):
            assert call(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
        for kw in ({'k': 1}, {'k': 0}, {'k': -5}, {'k': 1001}, {'n': 0}, {'n': -1}):
            assert call(**kw) == -1 and b'expected 2 <= k <= N' in lib.dic_last_error_string(), kw
        assert call(n=2000, k=1025) == -2 and b'at most 1024 neighbours' in lib.dic_last_error_string()
        assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
        for kw in ({'idx': odd}, {'sim': odd}):
            assert call(**kw) == -2 and b'aligned' in lib.dic_last_error_string()
    for kw in ({'density': None}, {'labels': None}, {'border': None}, {'changed': None}):
        assert components(**kw) == -1 and b'NULL' in lib.dic_last_error_string()
    for kw in ({'eps': 0}, {'eps': 17}, {'eps': -1}, {'ms': -1}):
        assert components(**kw) == -1 and b'expected 1 <= eps <= k' in lib.dic_last_error_string(), kw
    for kw in ({'density': odd}, {'labels': odd}, {'border': odd}, {'changed': odd}):
        assert components(**kw) == -2 and b'aligned' in lib.dic_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------------------------ parsers
def test_p2_parser_accepts_the_snn_flags_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    a = p2.get_arguments([])
    assert (a.cluster_method, a.k_max, a.select_eps, a.n_init, a.gap_b, a.opt_eps) == ('kmeans', 10, 'k_distance_graph', 10, 10, 1.9)
    assert a.select_opt_k == ['gap_sts', 'elbow'] and a.restore_metric == ['ae_mse', 'loss']
    assert a.internal_metrics == ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']
    assert (a.consensus_reps, a.consensus_p_item, a.hdbscan_min_cluster_size, a.gmm_covariance_type, a.metric_sample) == (100, 0.8, None, 'diag', 0)
    assert (a.snn_k, a.snn_eps, a.snn_min_samples) == (None, None, None)
    a = p2.get_arguments(['--cluster_method', 'snn', '--snn_k', '20', '--snn_eps', '4', '9', '--snn_min_samples', '0'])
    assert (a.cluster_method, a.snn_k, a.snn_eps, a.snn_min_samples) == ('snn', 20, [4, 9], 0)
    with pytest.raises(SystemExit):
        p2.get_arguments(['--snn_eps', '2.5'])
    assert p2.snn_default_eps(257) == [51, 77, 103, 128, 154, 180, 206]
    assert p2.snn_default_eps(17) == [3, 5, 7, 8, 10, 12, 14] and p2.snn_default_eps(2) == [1, 2]          # deduplicated, inside [1, k]
    assert p2.Snn.COLUMNS[:6] == p2.Dbscan.COLUMNS and p2.Snn.COLUMNS[6:] == ['k', 'min_samples']


def test_p4_parser_accepts_the_snn_flags_and_keeps_the_old_defaults():
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    a = p4.get_arguments([])
    assert (a.cluster_method, a.num_clusters, a.opt_eps, a.hdbscan_min_cluster_size, a.transfer, a.transfer_k, a.dl_cluster_label_type) == (
        'kmeans', 4, 1.9, None, 'centre', None, 'pred')
    assert a.restore_metric == ['ae_mse', 'loss', 'delta'] and (a.snn_k, a.snn_eps, a.snn_min_samples) == (None, None, None)
    a = p4.get_arguments(['--cluster_method', 'snn', '--snn_k', '20', '--snn_eps', '9', '--snn_min_samples', '5', '--transfer', 'knn'])
    assert (a.cluster_method, a.snn_k, a.snn_eps, a.snn_min_samples, a.transfer) == ('snn', 20, 9, 5, 'knn')
    with pytest.raises(SystemExit):
        p4.get_arguments(['--snn_eps', '4', '9'])          # a single eps


def test_p4_still_refuses_knn_transfer_for_kmeans_and_admits_snn(tmp_path, monkeypatch):
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match='--transfer knn applies to --cluster_method dbscan and hdbscan only'):
        p4.main(p4.get_arguments(['--cluster_method', 'kmeans', '--transfer', 'knn']))
    assert not (tmp_path / 'Results').exists()
    args = p4.get_arguments(['--cluster_method', 'snn', '--transfer', 'knn'])
    args.restore_metric = ['ae_mse']
    with pytest.raises(FileNotFoundError):          # past the refusal: it goes on to read the latents, which are not there
        p4.main(args)


# --------------------------------------------------------------------------------------------------------------------------------------- registers
def test_snn_kernels_do_not_spill_to_scratch():
    """The similarity kernel runs log2 k LDS probes per list entry, N k^2 entries: a register in scratch memory would be paid on every one.  Require
    ScratchSize == 0 and no vector-register spills for every kernel of dic_snn.hip, by name."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_snn.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert 'warning' not in res.stderr
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    for kernel in ('snn_similarity_kernel', 'snn_label_kernel', 'snn_jump_kernel'):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) == len(spills) == 3
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))
