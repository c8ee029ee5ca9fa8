"""Ward linkage, host side (no GPU): the numpy yardstick of csrc/dic_ward.hip's definition against scipy, the cuts against scipy and sklearn, the gap
condition of the test inputs, the ABI's and the Python argument errors, and the register use of the kernels."""
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
from deep_interpolation_clustering_amd import ward as W
from deep_interpolation_clustering_amd.consensus import cut_linkage
from deep_interpolation_clustering_amd.ward import Ward, cut_many, ward_linkage

GAP = 1e-10          # DESIGN.md section 5's OPTICS rule: a decision is an exact tie or separated by more than this, relative


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build(verbose=False)
    return N.lib()


def blobs(n, d, seed, n_centers=5):
    rs = np.random.RandomState(seed)
    centers = rs.normal(0.0, 6.0, size=(n_centers, d))
    return (centers[rs.randint(n_centers, size=n)] + rs.normal(0.0, 1.0, size=(n, d))).astype(np.float32)


def _dup():
    X = blobs(200, 12, 7)
    X[160:] = X[:40]
    return X


# name -> (points, has exact ties).  The GPU tests (tests/test_gpu_ward.py) run on exactly these.
CASES = {
    'n2': (lambda: blobs(2, 4, 1), False),
    'n3': (lambda: blobs(3, 4, 2), False),
    'n17': (lambda: blobs(17, 12, 3), False),
    'n255': (lambda: blobs(255, 64, 4), False),
    'n257': (lambda: blobs(257, 256, 5), False),
    'n1030': (lambda: blobs(1030, 8, 6), False),
    'n4100': (lambda: blobs(4100, 8, 8, n_centers=7), False),
    'dup': (_dup, True),
    'same': (lambda: np.tile(blobs(1, 4, 9), (131, 1)), True),
    'strided': (lambda: blobs(257, 8, 10), False),
}
BLOB_CASES = [c for c in CASES if c != 'same']


@functools.lru_cache(maxsize=None)
def points(case):
    X = CASES[case][0]()
    X.setflags(write=False)
    return X


def yardstick_ward(X):
    """The definition in numpy: f64 sums, one division per new centroid, scipy's chain and tie rules.  Returns (records (N - 1, 4) in merge order, gaps): per
    chain step (best, second, d_prev or None) -- the two smallest candidates and the distance to the previous chain element, where that element is not the
    best candidate itself."""
    X = np.asarray(X, dtype=np.float32)
    n = len(X)
    S = X.astype(np.float64)
    C = S.copy()
    size = np.zeros(n, dtype=np.int64) + 1
    chain, rec, gaps = [], [], []
    for _ in range(n - 1):
        if not chain:
            chain = [int(np.flatnonzero(size > 0)[0])]
        while True:
            x = chain[-1]
            live = np.flatnonzero(size > 0)
            live = live[live != x]
            diff = C[x][None, :] - C[live]
            nx, nq = float(size[x]), size[live].astype(np.float64)
            d2 = ((2.0 * (nx * nq)) / (nx + nq)) * (diff * diff).sum(axis=1)
            j = int(np.argmin(d2))          # the first of the smallest: ascending index
            best, y = float(d2[j]), int(live[j])
            second = float(np.partition(d2, 1)[1]) if len(d2) > 1 else np.inf
            d_prev = None
            if len(chain) > 1:
                prev = chain[-2]
                cur = float(d2[np.searchsorted(live, prev)])
                if y != prev:
                    d_prev = cur
                if not best < cur:          # the previous chain element wins a tie
                    y, best = prev, cur
            gaps.append((float(d2[j]), second, d_prev))
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        chain = chain[:-2]
        a, b = min(x, y), max(x, y)
        na, nb = int(size[a]), int(size[b])
        rec.append((a, b, np.sqrt(best), na + nb))
        S[b] = S[a] + S[b]
        C[b] = S[b] / float(na + nb)
        size[a], size[b] = 0, na + nb
    return np.array(rec, dtype=np.float64), gaps


def relabelled(rec):
    """scipy's Z of raw records: stable sort by height, merged clusters named n, n + 1, .., from member lists (independent of consensus._relabel)."""
    n = len(rec) + 1
    rec = rec[np.argsort(rec[:, 2], kind='stable')]
    name = list(range(n))
    members = {i: [i] for i in range(n)}
    Z = np.empty((n - 1, 4))
    for i, (x, y, h, _) in enumerate(rec):
        a, b = sorted((name[int(x)], name[int(y)]))
        both = members.pop(a) + members.pop(b)
        members[n + i] = both
        for p in both:
            name[p] = n + i
        Z[i] = (a, b, h, len(both))
    return Z


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """(records, Z, gaps) of a case, computed once per session."""
    rec, gaps = yardstick_ward(points(case))
    return rec, relabelled(rec), gaps


@functools.lru_cache(maxsize=None)
def scipy_linkage(case):
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    return hier.linkage(points(case).astype(np.float64), 'ward')


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize('case', list(CASES))
def test_yardstick_equals_scipy(case):
    ref = scipy_linkage(case)
    _, Z, _ = yardstick(case)
    assert np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]])
    zero = ref[:, 2] == 0
    assert np.all(Z[zero, 2] == 0)
    np.testing.assert_allclose(Z[~zero, 2], ref[~zero, 2], rtol=1e-12, atol=0)
    if case == 'dup':
        assert zero.sum() == 40
    if case == 'same':
        assert zero.all()


@pytest.mark.parametrize('case', list(CASES))
def test_cases_meet_the_gap_condition(case):
    """Every decision of the chain is an exact tie at 0 or separated by more than 1e-10 relative: only then is "the same merges" a fair demand of a kernel
    whose reduction tree differs from numpy's."""
    _, _, gaps = yardstick(case)
    worst = np.inf
    for best, second, d_prev in gaps:
        for lo, hi in ((best, second),) + (() if d_prev is None else ((min(best, d_prev), max(best, d_prev)),)):
            if hi == 0 and lo == 0:
                continue          # an exact tie at 0: the index rule / the previous-element rule decides, on equal bits
            if np.isinf(hi):
                continue          # a single candidate
            rel = (hi - lo) / hi
            worst = min(worst, rel)
            assert rel > GAP, (case, lo, hi)
    print(case, 'smallest relative gap', worst, 'steps', len(gaps), 'of at most', 3 * (len(points(case)) - 1))
    assert len(gaps) <= 3 * (len(points(case)) - 1)


@pytest.mark.parametrize('case', ['n17', 'n255', 'n1030', 'dup', 'same'])
def test_package_relabel_and_cuts_equal_scipy(case):
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    from deep_interpolation_clustering_amd.consensus import _relabel
    rec, Z, _ = yardstick(case)
    n = len(Z) + 1
    assert np.array_equal(_relabel(rec, n), Z)
    ks = [k for k in (1, 2, 3, 5, 7, 16, n) if k <= n]
    many = cut_many(Z, ks)
    assert sorted(many) == sorted(set(ks))
    for k in ks:
        lab = many[k]
        assert lab.shape == (n,) and lab.dtype == np.int64
        assert np.array_equal(lab, cut_linkage(Z, k) - 1)
        first = [int(np.flatnonzero(lab == c)[0]) for c in range(k)]
        assert first == sorted(first) and lab[0] == 0
        if not CASES[case][1]:
            assert same_partition(lab, hier.fcluster(scipy_linkage(case), k, 'maxclust'))


@pytest.mark.parametrize('case', ['n17', 'n255', 'n1030'])
def test_cuts_equal_sklearn(case):
    sk = pytest.importorskip('sklearn.cluster')
    _, Z, _ = yardstick(case)
    X = points(case).astype(np.float64)
    for k in (2, 3, 5, 7):
        theirs = sk.AgglomerativeClustering(n_clusters=k, linkage='ward').fit(X).labels_
        assert same_partition(cut_many(Z, [k])[k], theirs)


def test_cut_many_by_hand():
    # 5 points: (1, 3) merge, then (0, 4), then {1, 3} with 2, then all
    Z = np.array([[1, 3, 0.0, 2], [0, 4, 0.0, 2], [2, 5, 0.5, 3], [6, 7, 1.0, 5]], dtype=np.float64)
    got = cut_many(Z, [5, 4, 3, 2, 1])
    assert got[5].tolist() == [0, 1, 2, 3, 4]
    assert got[4].tolist() == [0, 1, 2, 1, 3]
    assert got[3].tolist() == [0, 1, 2, 1, 0]
    assert got[2].tolist() == [0, 1, 1, 1, 0]
    assert got[1].tolist() == [0, 0, 0, 0, 0]
    assert cut_many(Z, []) == {}
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match='K must be in 1..5'):
            cut_many(Z, [2, bad])
    with pytest.raises(ValueError, match='ints'):
        cut_many(Z, [2.5])


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError, match='2-D'):
        ward_linkage(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match='2-D'):
        Ward().fit(torch.zeros(4, 3, 2))
    with pytest.raises(ValueError, match='at least 2 points'):
        ward_linkage(X[:1])
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        ward_linkage(np.zeros((10, 260), np.float32))
    with pytest.raises(NotImplementedError, match='at most 256 features'):
        Ward().fit(np.zeros((10, 260), np.float32))
    with pytest.raises(NotImplementedError, match='pass the points'):
        Ward(metric='precomputed')
    for metric in ('manhattan', 'cosine'):
        with pytest.raises(NotImplementedError, match='only the euclidean metric'):
            Ward(metric=metric)
    with pytest.raises(NotImplementedError, match="linkage='ward'"):
        Ward(linkage='average')
    for bad in (0, -2, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='ints >= 1'):
            Ward(n_clusters=bad)
        with pytest.raises(ValueError, match='ints >= 1'):
            Ward(ks=[2, bad])
    with pytest.raises(ValueError, match='K must be in 1..10'):
        Ward(n_clusters=11).fit(X)
    with pytest.raises(ValueError, match='K must be in 1..10'):
        Ward(ks=range(2, 12)).fit(X)
    assert Ward(ks=range(2, 6)).ks == [2, 3, 4, 5] and Ward(ks=range(2, 6)).n_clusters == 5
    assert Ward(n_clusters=3, ks=[2, 7]).ks == [2, 3, 7] and Ward().n_clusters == 2
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ward_linkage(X)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            Ward(n_clusters=3).fit(X)


def test_module_does_not_import_scipy_or_sklearn():
    with open(W.__file__) as f:
        assert not re.search(r'^\s*(import|from)\s+(scipy|sklearn)', f.read(), flags=re.M)


def test_drivers_accept_ward():
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    assert p2.get_arguments(['--cluster_method', 'ward', '--k_max', '5']).cluster_method == 'ward'
    assert p4.get_arguments(['--cluster_method', 'ward', '--num_clusters', '3']).cluster_method == 'ward'
    assert 'need not be its nearest centre' in p4.Cluster._ward.__doc__


def test_header_and_signatures_agree():
    names = {'dic_ward_workspace', 'dic_ward_linkage'}
    assert names <= set(N.header_symbols()) and names <= set(N.SIGNATURES)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_ward_workspace(1000, 256)
    assert ws > 0 and lib.dic_ward_workspace(1000, 260) == 0 and lib.dic_ward_workspace(1, 256) == 0 and lib.dic_ward_workspace(1 << 30, 256) == 0
    assert lib.dic_ward_workspace(1000, 0) == 0

    def call(X=fake, ldx=256, n=1000, d=256, rec=fake, work=fake, nbytes=ws):
        return lib.dic_ward_linkage(X, ldx, n, d, rec, work, nbytes, None)

    for kw in ({'X': None}, {'rec': None}, {'work': None}):
        assert call(**kw) == -1
        assert b'NULL' in lib.dic_last_error_string()
    assert call(n=1) == -1 and b'at least 2' in lib.dic_last_error_string()
    assert call(n=0) == -1 and call(n=-3) == -1 and call(ldx=128) == -1 and call(d=0) == -1
    assert call(ldx=252, d=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=258, d=256) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
    assert call(n=1 << 30) == -2 and b'2^30' in lib.dic_last_error_string()
    assert call(X=ctypes.c_void_p((1 << 20) + 4)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert call(work=ctypes.c_void_p((1 << 20) + 8)) == -2 and b'aligned' in lib.dic_last_error_string()
    assert call(rec=ctypes.c_void_p((1 << 20) + 4)) == -2
    assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()


def test_workspace_is_linear_in_n(lib):
    sizes = [lib.dic_ward_workspace(n, 256) for n in (2, 255, 256, 257, 5000, 75000, 300000)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    per_point = 2 * 8 * 256 + 4 + 4          # S and C in f64, the size, the chain slot
    for n in (5000, 75000, 300000):
        assert n * per_point <= lib.dic_ward_workspace(n, 256) <= n * per_point + (1 << 14)          # + 8 KB of workgroup minima, the state, the alignment
    assert abs(lib.dic_ward_workspace(150000, 64) - lib.dic_ward_workspace(75000, 64) - 75000 * (2 * 8 * 64 + 8)) <= 4 * 256          # (four aligned arrays)
    assert lib.dic_ward_workspace(75000, 8) < lib.dic_ward_workspace(75000, 256)


def test_ward_kernels_do_not_spill_to_scratch():
    """A step is launched up to 3 (N - 1) times, 225 000 at the cohort size: registers that go to scratch memory would be paid every time.  Require
    ScratchSize == 0 and no spills for every kernel of dic_ward.hip."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_ward.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', res.stderr)]
    sspills = [int(v) for v in re.findall(r'SGPRs Spill: (\d+)', res.stderr)]
    assert any('wd_step_kernel' in n for n in names) and any('wd_init_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills) == len(sspills)
    assert max(scratch) == 0 and max(spills) == 0 and max(sspills) == 0, list(zip(names, scratch, spills, sspills))
