"""CPU checks of the k-distance pieces that need no GPU: the knee of a curve (knn.kneedle_elbow), the ABI's argument checks, the Python argument errors and the
register allocation of csrc/dic_knn.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd import knn
from deep_interpolation_clustering_amd.knn import kneedle_elbow


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def hockey_stick(n, corner, low_slope=0.0):
    """y over x = 1..n: ``low_slope`` per sample up to x = corner, then a straight rise of 1 in all to x = n."""
    x = np.arange(1, n + 1, dtype=np.float64)
    base = low_slope * np.minimum(x, corner)
    return base + np.where(x > corner, (x - corner) / (n - corner), 0.0)


# Why the corner: flipped, the curve rises (normalised slope > 1) up to the corner and is flat (or nearly) behind it, so D = yt - xn has its first maximum at
# the corner and falls by one sample step per sample after it -- below the threshold within two samples, whatever the rounding of that step.
@pytest.mark.parametrize('n,corner,low_slope', [(1001, 701, 1e-4), (1001, 101, 1e-4), (1001, 901, 1e-4), (1001, 701, 0.0), (400, 57, 0.0)])
def test_hockey_stick_corner(n, corner, low_slope):
    y = hockey_stick(n, corner, low_slope)
    ex, ey = kneedle_elbow(y)
    assert ex == corner
    assert ey == y[corner - 1]
    assert isinstance(ex, int) and isinstance(ey, float)


def test_plateau_at_the_end_is_what_the_definition_says():
    # a hockey stick (corner at x = 300) that ends in a plateau of equal values from x = 600 on: flipped, the plateau comes first, yt = 0 there, D = -xn falls
    # from D[0] = 0 -- index 0 is D's first maximum (greater_equal, ends clipped) and D is below its threshold two samples on: the knee is x[N - 1 - 0] = N.
    x = np.arange(1, 1001, dtype=np.float64)
    y = np.clip((x - 300) / 300.0, 0.0, 1.0)
    ex, ey = kneedle_elbow(y)
    assert (ex, ey) == (1000, 1.0)


def test_exp_curve_against_the_analytic_knee():
    # y = e^t over t in [0, 6], 2000 samples: the knee is where the normalised slope is 1, 6 e^t / (e^6 - 1) = 1
    t = np.linspace(0.0, 6.0, 2000)
    y = np.exp(t)
    t_star = np.log((np.exp(6.0) - 1.0) / 6.0)
    x_star = 1.0 + t_star / 6.0 * 1999
    ex, ey = kneedle_elbow(y)
    assert abs(ex - x_star) <= 1.0, (ex, x_star)
    assert ey == y[ex - 1]
    assert abs(ey - np.exp(t_star)) <= np.exp(t_star) * 6.0 / 1999 * 1.01          # within one sample of the analytic value


def test_constant_and_short_curves_have_no_knee():
    assert kneedle_elbow(np.full(50, 3.25)) == (None, None)
    assert kneedle_elbow([1.0, 2.0]) == (None, None)
    assert kneedle_elbow([1.0]) == (None, None)
    assert kneedle_elbow([]) == (None, None)


def test_two_bends_return_the_first_detected():
    # two hockey sticks on top of each other: flat, rise to 0.4 over x = 300..400, flat to x = 700, rise to 1 at x = 1000 (normalised slope 2).  The walk
    # runs over the FLIPPED curve, so it meets the later bend first: D rises along the last rise, peaks where the flat part ends (x = 700) and falls by one
    # sample step per sample along it -- detected there, the earlier bend is never reached.
    x = np.arange(1, 1001, dtype=np.float64)
    y = np.where(x <= 300, 0.0, np.where(x <= 400, 0.4 * (x - 300) / 100, np.where(x <= 700, 0.4, 0.4 + 0.6 * (x - 700) / 300)))
    assert kneedle_elbow(y) == (700, 0.4)


def test_equals_kneed_where_it_is_installed():
    kneed = pytest.importorskip('kneed')
    rng = np.random.default_rng(4)
    curves = [hockey_stick(1001, 701, 1e-4), np.exp(np.linspace(0, 6, 2000)), np.sort(rng.gamma(2.0, 1.0, 5000)),
              np.sort(np.concatenate([np.zeros(40), rng.normal(2.0, 0.05, 3000), rng.uniform(2.2, 9.0, 150)]))]
    for y in curves:
        x = np.arange(1, len(y) + 1)
        kl = kneed.KneeLocator(x, y, S=1.0, curve='convex', direction='increasing')
        ex, ey = kneedle_elbow(y)
        assert ex == kl.elbow and (ey == kl.elbow_y or (ey is None and kl.elbow_y is None))


def test_abi_rejects_bad_arguments_without_gpu(lib):
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    stats = (ctypes.c_int64 * 5)()
    ws = lib.dic_knn_workspace(1000, 256, 0)
    assert ws > 0 and lib.dic_knn_workspace(1000, 260, 0) == 0 and lib.dic_knn_workspace(0, 256, 0) == 0

    def call(X=fake, ldx=256, centre=fake, n=1000, d=256, k=5, kth=fake, work=fake, nbytes=ws):
        return lib.dic_knn_kth_distance(X, ldx, centre, n, d, k, kth, 0, stats, work, nbytes, None)

    for kw in ({'X': None}, {'centre': None}, {'kth': None}, {'work': None}):
        assert call(**kw) == -1
        assert b'NULL' in lib.dic_last_error_string()
    assert call(ldx=252, d=250) == -2 and b'multiples of 4' in lib.dic_last_error_string()
    assert call(ldx=260, d=260) == -2 and b'at most 256' in lib.dic_last_error_string()
    assert call(k=0) == -2 and b'k=0' in lib.dic_last_error_string()
    assert call(k=1001) == -2 and b'k=1001' in lib.dic_last_error_string() and b'N=1000' in lib.dic_last_error_string()
    assert call(k=-3) == -2
    assert call(nbytes=ws - 1) == -3 and b'workspace' in lib.dic_last_error_string()
    assert lib.dic_knn_kth_distance(fake, 256, fake, 1000, 256, 5, fake, 0, None, fake, ws - 1, None) == -3          # stats may be NULL


def test_workspace_is_monotone(lib):
    sizes = [lib.dic_knn_workspace(n, 256, 0) for n in (1, 255, 256, 257, 5000, 75000, 300000)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_budget = [lib.dic_knn_workspace(75000, 256, b) for b in (12, 1 << 20, 64 << 20, 384 << 20, 1 << 31)]
    assert all(a < b for a, b in zip(by_budget, by_budget[1:]))
    assert lib.dic_knn_workspace(75000, 256, 0) == lib.dic_knn_workspace(75000, 256, 384 << 20)          # <= 0: the default
    assert lib.dic_knn_workspace(75000, 256, -1) == lib.dic_knn_workspace(75000, 256, 0)
    # the budget never buys more than every pair of the call
    assert lib.dic_knn_workspace(100, 8, 1 << 40) == lib.dic_knn_workspace(100, 8, 12 * 100 * 100)
    # and next to the planes it is the only part that is not O(N): without it the workspace stays far below an N x N f32 matrix
    assert lib.dic_knn_workspace(75000, 256, 12) < 75000 * 75000 * 4 // 100


# (N, M, D, m, candidate_budget): (dic_knn_workspace(N, D, b), dic_knn_neighbors_workspace(N, M, D, b), dic_knn_ranks_workspace(N, D, m, b)), as the library
# computed them before the three entry points moved onto the shared candidate-list driver (csrc/dic_candlist.h).
WORKSPACES_BEFORE_CANDLIST = {
    (1, 0, 4, 1, 0): (636928, 636928, 636416),
    (1, 1, 4, 1, 1): (636928, 638976, 636416),                          # a budget below one entry: one entry
    (256, 0, 8, 9, 0): (2049280, 2049280, 6046976),
    (256, 1, 4, 1, 7): (1263360, 1267712, 1263104),
    (257, 300, 36, 8, 11): (1267712, 2005760, 1267200),                 # 11 bytes: one 8-byte entry of the ranks, none of the 12-byte ones
    (257, 0, 256, 1023, 1048576): (2060288, 2060288, 10654464),
    (1537, 0, 20, 7, 18444): (4440064, 4440064, 4439552),
    (600, 300, 8, 4, 4611686018427387904): (6430976, 12571136, 2110976),          # a budget above N^2 entries: every pair
    (100, 5, 8, 16, 1280001): (999168, 1024256, 2204416),
    (75000, 0, 256, 10, 0): (588086016, 588086016, 597718784),
    (75000, 25000, 256, 17, 67108864): (252541952, 314143232, 271807232),
    (300000, 1, 16, 3, -1): (739837696, 739840768, 739837184),
}


def test_workspace_sizes_are_those_before_the_shared_driver(lib):
    """The workspace layouts are part of the C ABI's contract with callers that size their own buffers: the move of the list protocol into
    csrc/dic_candlist.h changes none of them.  Host arithmetic, no device: N = 1, a full block, one row past it, the default budget (0 and negative), budgets
    below one entry and above every pair."""
    for (n, m, d, t, b), want in WORKSPACES_BEFORE_CANDLIST.items():
        got = (lib.dic_knn_workspace(n, d, b), lib.dic_knn_neighbors_workspace(n, m, d, b), lib.dic_knn_ranks_workspace(n, d, t, b))
        assert got == want, (n, m, d, t, b)


def test_python_argument_errors():
    X = np.zeros((10, 8), np.float32)
    with pytest.raises(ValueError, match='n_neighbors <= n_samples_fit'):
        knn.kth_neighbor_distance(X, 11)
    with pytest.raises(ValueError, match='n_neighbors'):
        knn.kth_neighbor_distance(X, 0)
    with pytest.raises(ValueError, match='2-D'):
        knn.kth_neighbor_distance(np.zeros(10, np.float32), 1)
    with pytest.raises(ValueError, match='2-D'):
        knn.kth_neighbor_distance(torch.zeros(4, 3, 2), 1)
    with pytest.raises(ValueError, match='candidate_budget'):
        knn.kth_neighbor_distance(X, 2, candidate_budget=0)
    with pytest.raises(ValueError):
        knn.core_distances(X, 11)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            knn.kth_neighbor_distance(X, 3)
        with pytest.raises(RuntimeError, match='no CPU path'):
            knn.k_distance_graph(X, 3)


def test_knn_kernels_do_not_spill_to_scratch():
    """The tile kernels run at 256 registers per lane with 128 of them accumulators; thresholds or counters that the compiler cannot keep in registers go to
    scratch memory inside the pair loop.  Require ScratchSize == 0 and no spills for every kernel of dic_knn.hip (dic_pairtile.h included)."""
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
    assert sum('kn_count_kernel' in n for n in names) == 2 and any('kn_gather_kernel' in n for n in names) and any('kn_exact_kernel' in n for n in names)
    assert len(scratch) == len(names) == len(spills)
    assert max(scratch) == 0 and max(spills) == 0, list(zip(names, scratch, spills))


def _walk_by_the_book(y, S=1.0):
    """The definition as a plain loop, the way kneed's find_knee walks it (online=False)."""
    from scipy.signal import argrelextrema
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    x = np.arange(1, n + 1, dtype=np.float64)
    xn = (x - x[0]) / (x[-1] - x[0])
    yn = (y - y.min()) / (y.max() - y.min())
    D = np.flip(yn.max() - yn) - xn
    maxima = argrelextrema(D, np.greater_equal)[0]
    minima = argrelextrema(D, np.less_equal)[0]
    Tmx = D[maxima] - S * np.abs(np.diff(xn).mean())
    threshold, candidate, m = 0.0, None, 0
    for i in range(n):
        if i < maxima[0]:
            continue
        if xn[i] == 1.0:
            break
        if (maxima == i).any():
            threshold, candidate = Tmx[m], i
            m += 1
        if (minima == i).any():
            threshold = 0.0
        if D[i + 1] < threshold:
            return int(x[n - 1 - candidate]), float(y[n - 1 - candidate])
    return None, None


def test_vectorised_walk_equals_the_loop():
    rng = np.random.default_rng(12)
    curves = [np.sort(rng.gamma(2.0, 1.0, 3000)), np.sort(rng.normal(0, 1, 800)), np.sort(rng.uniform(0, 1, 500)) ** 3,
              np.sort(np.concatenate([np.zeros(40), rng.normal(2.0, 0.05, 2000), rng.uniform(2.2, 9.0, 100)])),
              np.cumsum(rng.uniform(0, 1, 700) * np.linspace(0.01, 1, 700) ** 2), np.round(np.sort(rng.gamma(2.0, 1.0, 600)), 1),
              np.sort(rng.integers(0, 6, 300)).astype(float), hockey_stick(300, 200), np.linspace(0, 1, 50), np.linspace(0, 1, 50) ** 0.5]
    found = 0
    for y in curves:
        for S in (1.0, 0.0, 5.0):
            got = kneedle_elbow(y, S)
            assert got == _walk_by_the_book(y, S)
            found += got[0] is not None
    assert found >= 12
