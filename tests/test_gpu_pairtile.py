"""The approximate squared distance a_ij of the shared pair-tile loop (csrc/dic_pairtile.h) against f64, through the probe entry point
(csrc/dic_pairtile_probe.hip: the consumers' plane preparation and tile loop unchanged, every accumulator stored).  DBSCAN, the k-th neighbour distances, the
neighbour lists, mean shift and k-medoids decide on a_ij in registers, so the finished clusterings show an error in it only where a pair happens to lie within
the bound of a threshold; here every a_ij is looked at.

ORACLE: d^2 of the f32 points x (not of the centred v), numpy f64, difference form (test_pairtile_host.d2_f64).  BARS, none taken from a GPU measurement:
  bound         |a_ij - d^2_ij| < 2^-12 (nrm_i + bmax[J]) strictly, all i, j < N, with the DEVICE's nrm and bmax -- the sentence the consumers are built on;
  accumulation  |a_ij - t_ij| <= 2^-13.2 (n_i + n_j), t = test_pairtile_host.emulate fed the device's nrm: item (3) of the header's proof;
  norms         |nrm_i - sum v^2| <= 10 2^-24 sum v^2 (item (4)), bmax[b] == the largest nrm of block b exactly, 0 for the padding rows.
Lattice inputs (small integers: every product and partial sum exact) must come out bit for bit; ranges of the tile list on any number of workgroups must
reproduce the default launch bit for bit (dic_knn.hip: "a fixed function of (i, j)").

Every numeric case prints and appends one line to pairtile_bound.jsonl beside the trajectory tests' record (test_gpu_traj.DEV_LOG): the largest |a - d^2| / B0 and |a - t| / (2^-13.2 (n_i + n_j)).  The last
clean run, condensed: profiles/pairtile_bound.json."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd import _native as N
from test_gpu_traj import DEV_LOG
from test_pairtile_host import PT_T, aligned_residual, centred, d2_f64, emulate

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(DEV_LOG), 'pairtile_bound.jsonl')          # beside traj_deviation.jsonl
PAD = 2.0 ** 120                                                                 # PT_PAD_NORM: what the consumers without an index mask pass
ACC = 2.0 ** -13.2


def probe(X, centre, pad_norm=0.0, tile0=0, ntiles=0, grid=0):
    """One call of dic_pairtile_probe.  X: numpy (N, D) or a CUDA f32 tensor with unit column stride (its row stride is passed as ldx).
    Returns a (nblk 256, nblk 256) f32, visits (nblk, nblk), nrm (N + 256), bmax (nblk) as numpy arrays; a starts as NaN, visits as 0."""
    L = N.lib()
    x = X if torch.is_tensor(X) else torch.as_tensor(np.ascontiguousarray(X, dtype=np.float32), device='cuda')
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1
    n, d = x.shape
    c = torch.as_tensor(np.ascontiguousarray(centre, dtype=np.float32).reshape(1, d), device='cuda')
    nblk = (n + PT_T - 1) // PT_T
    a = torch.full((nblk * PT_T, nblk * PT_T), float('nan'), dtype=torch.float32, device='cuda')
    visits = torch.zeros((nblk, nblk), dtype=torch.int32, device='cuda')
    nrm = torch.full((n + PT_T,), float('nan'), dtype=torch.float32, device='cuda')
    bmax = torch.full((nblk,), float('nan'), dtype=torch.float32, device='cuda')
    ws = torch.empty(L.dic_pairtile_probe_workspace(n, d), dtype=torch.uint8, device='cuda')
    assert ws.numel() > 0
    N.check(L.dic_pairtile_probe(N.ptr(x), x.stride(0), N.ptr(c), n, d, pad_norm, tile0, ntiles, grid, N.ptr(a), N.ptr(visits), N.ptr(nrm), N.ptr(bmax),
                                 N.ptr(ws), ws.numel(), N.stream_of(x)), 'pairtile_probe')
    torch.cuda.synchronize()
    return SimpleNamespace(a=a.cpu().numpy(), visits=visits.cpu().numpy(), nrm=nrm.cpu().numpy(), bmax=bmax.cpu().numpy(), n=n, nblk=nblk)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def record(case, **measured):
    line = json.dumps(dict(case=case, **measured))
    print('[pairtile-bound]', line)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, 'a') as f:
            f.write(line + '\n')
    except OSError:
        pass


def check_norms(X, centre, r):
    n = r.n
    s = (centred(X, centre).astype(np.float64) ** 2).sum(1)
    nrm = r.nrm.astype(np.float64)
    assert np.all(np.abs(nrm[:n] - s) <= 10 * 2.0 ** -24 * s), float((np.abs(nrm[:n] - s) / np.maximum(s, 1e-300)).max())
    assert np.all(r.nrm[n:] == 0.0)
    for b in range(r.nblk):
        assert r.bmax[b] == r.nrm[b * PT_T:(b + 1) * PT_T].max(), b


def check_numerics(case, X, centre, r):
    """The three bars of the module docstring on the result r of probe(X, centre); records and returns the two ratios."""
    X = np.asarray(X, dtype=np.float32)
    n = r.n
    check_norms(X, centre, r)
    assert np.all(r.visits == 1)
    nrm = r.nrm[:n].astype(np.float64)
    a = r.a[:n, :n].astype(np.float64)
    b0 = 2.0 ** -12 * (nrm[:, None] + np.repeat(r.bmax.astype(np.float64), PT_T)[None, :n])
    acc_bar = ACC * (nrm[:, None] + nrm[None, :])
    e_bound = np.abs(a - d2_f64(X))
    e_acc = np.abs(a - emulate(X, centre, nrm=r.nrm[:n]))
    bound_ratio, acc_ratio = float((e_bound / b0).max()), float((e_acc / acc_bar).max())
    record(case, N=n, D=X.shape[1], bound_ratio=bound_ratio, accumulation_ratio=acc_ratio)
    assert np.all(e_bound < b0), bound_ratio                 # (comparisons with NaN are false: an unwritten entry fails here)
    assert np.all(e_acc <= acc_bar), acc_ratio
    return bound_ratio, acc_ratio


def gaussian(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1, (n, d)).astype(np.float32)
    return X, X.mean(0, keepdims=True)


def lattice(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (n, d)).astype(np.float32), np.zeros((1, d), np.float32)


# ---------------------------------------------------------------------------------------------------------------------------- exact lattice
@pytest.mark.parametrize('n', [1, 5, 255, 256, 257, 600])
def test_lattice_is_exact(n):
    """Integer coordinates in [-8, 8], D = 8, centre 0: h = v, l = 0, norms <= 512 in two bf16 pieces, every product and partial sum an integer below 2^24.
    a_ij == d^2_ij bit for bit; a wrong index map, swizzle or stale slab shows as a wrong integer.  The padding rows and columns are exact as well."""
    X, c = lattice(n, 8, seed=n)
    d2 = d2_f64(X).astype(np.float32)
    nrm = (X.astype(np.float64) ** 2).sum(1).astype(np.float32)
    for pad in (PAD, 0.0):
        r = probe(X, c, pad_norm=pad)
        assert np.all(r.visits == 1)
        np.testing.assert_array_equal(r.nrm[:n], nrm)
        np.testing.assert_array_equal(bits(r.a[:n, :n]), bits(d2))
        m = r.a.shape[0] - n                                       # padding points
        np.testing.assert_array_equal(r.a[:n, n:], np.broadcast_to((nrm + np.float32(pad))[:, None], (n, m)))          # (n_i + 2^120 rounds to 2^120)
        np.testing.assert_array_equal(r.a[n:, :n], np.broadcast_to(nrm[None, :], (m, n)))
        np.testing.assert_array_equal(r.a[n:, n:], np.full((m, m), pad, np.float32))


def test_default_grid_walks_two_one_and_no_tiles():
    """N = 4100: 17 x 17 = 289 tiles on the default 256 workgroups: two tiles each on the first 144, one on the next, none on the rest."""
    X, c = lattice(4100, 16, seed=3)
    r = probe(X, c, pad_norm=PAD)
    assert r.nblk == 17 and np.all(r.visits == 1)
    np.testing.assert_array_equal(bits(r.a[:4100, :4100]), bits(d2_f64(X).astype(np.float32)))
    assert np.all(r.a[:4100, 4100:] == np.float32(PAD)) and not np.isnan(r.a).any()


# ---------------------------------------------------------------------------------------------------------------------------- padding
def test_padding_rows_and_columns():
    X, c = gaussian(300, 36, seed=11)
    n = 300
    for pad in (PAD, 0.0):
        r = probe(X, c, pad_norm=pad)
        check_norms(X, c, r)
        nrm, bmax = r.nrm[:n].astype(np.float64), r.bmax.astype(np.float64)
        a = r.a.astype(np.float64)
        assert not np.isnan(a).any()
        if pad:
            assert np.all(r.a[:n, n:] == np.float32(PAD))          # real rows: exactly 2^120, above every threshold a caller admits
        else:
            assert np.all(np.abs(a[:n, n:] - nrm[:, None]) < 2.0 ** -12 * (nrm[:, None] + bmax[-1]))
        assert np.all(r.a[n:, n:] == np.float32(pad))
        # padding rows (zero vectors of norm 0 as operand i) against real columns
        assert np.all(np.abs(a[n:, :n] - nrm[None, :]) < 2.0 ** -12 * np.repeat(bmax, PT_T)[None, :n])


# ---------------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize('d,wide', [(4, False), (8, False), (36, False), (36, True), (128, False), (252, False), (256, False)])
def test_shapes(d, wide):
    """N(0, 1) points around their mean.  wide: the points are a column slice of a (N, D + 4) tensor (ldx = D + 4, rows still 16-B aligned) whose other
    columns hold 1e30 -- a read past D would show in every norm."""
    X, c = gaussian(300, d, seed=100 + d)
    if wide:
        full = torch.full((300, d + 4), 1e30, dtype=torch.float32, device='cuda')
        full[:, :d] = torch.as_tensor(X)
        x = full[:, :d]
        assert x.stride(0) == d + 4
        r = probe(x, c)
    else:
        r = probe(X, c)
    assert not np.isnan(r.a).any()
    check_numerics('gaussian%s' % (' ldx=D+4' if wide else ''), X, c, r)


# ---------------------------------------------------------------------------------------------------------------------------- ranges of the tile list
def test_ranges_and_grids_reproduce_the_default_launch():
    """N = 600: 3 x 3 tiles.  Every (tile0, ntiles) range on every grid: the walked tiles are visited once and hold the bits of the default launch, everything
    else is untouched.  One workgroup walking all nine tiles crosses two row-block changes (the e_prev / e_cur / e_nxt hand-off); (4, 2) starts inside a
    row block; with grid 4 over 9 tiles (3 per workgroup) and in every range shorter than the grid, workgroups have no tile at all."""
    X, c = gaussian(600, 36, seed=5)
    full = probe(X, c, pad_norm=PAD)
    assert np.all(full.visits == 1) and not np.isnan(full.a).any()
    check_numerics('gaussian N=600', X, c, full)
    for tile0, ntiles in [(0, 9), (3, 3), (4, 2), (8, 1)]:
        walked = np.zeros(9, bool)
        walked[tile0:tile0 + ntiles] = True
        walked = walked.reshape(3, 3)
        mask = np.kron(walked, np.ones((PT_T, PT_T), bool))
        for grid in (1, 2, 4, 9):
            r = probe(X, c, pad_norm=PAD, tile0=tile0, ntiles=ntiles, grid=grid)
            what = (tile0, ntiles, grid)
            np.testing.assert_array_equal(r.visits, walked.astype(np.int32), err_msg=str(what))
            assert np.isnan(r.a[~mask]).all(), what
            np.testing.assert_array_equal(bits(r.a[mask]), bits(full.a[mask]), err_msg=str(what))
            np.testing.assert_array_equal(bits(r.nrm), bits(full.nrm))


# ---------------------------------------------------------------------------------------------------------------------------- numerics
DIMS = [256, 8]


@pytest.mark.parametrize('d', DIMS)
def test_aligned_residuals(d):
    """The input test_pairtile_host qualifies: a kernel that loses the lo.hi or hi.lo products or the second norm piece is off by more than 4 B0 here."""
    X, c = aligned_residual(300, d)
    check_numerics('aligned residuals', X, c, probe(X, c))


@pytest.mark.parametrize('d', DIMS)
def test_two_clusters_far_from_their_mean(d):
    """test_gpu_knn.test_points_far_from_their_mean's recipe: the norms (~ 1e4 D) dwarf the within-cluster d^2 (~ 2e-4 D), all of the bound is cancellation."""
    rng = np.random.default_rng(8)
    X = np.concatenate([100.0 + rng.normal(0, 0.01, (300, d)), -100.0 + rng.normal(0, 0.01, (300, d))])
    X = rng.permutation(X).astype(np.float32)
    c = X.mean(0, keepdims=True)
    check_numerics('two clusters at +-100, width 0.01', X, c, probe(X, c))


@pytest.mark.parametrize('d', DIMS)
def test_exact_duplicates(d):
    rng = np.random.default_rng(9)
    base = rng.normal(0, 1, (560, d)).astype(np.float32)
    perm = rng.permutation(600)
    X = np.concatenate([base, np.repeat(base[7:8], 40, 0)])[perm]
    dup = np.flatnonzero((X == base[7]).all(1))
    assert len(dup) == 41
    c = X.mean(0, keepdims=True)
    r = probe(X, c)
    check_numerics('40 exact duplicates', X, c, r)
    sub = r.a[np.ix_(dup, dup)].astype(np.float64)
    b0 = 2.0 ** -12 * (r.nrm[dup].astype(np.float64)[:, None] + r.bmax.astype(np.float64)[dup // PT_T][None, :])
    assert np.all(np.abs(sub) < b0)          # d^2 = 0
    assert np.all(bits(sub) == bits(sub)[0, 0])          # and one value: the same planes give the same sum wherever the pair sits


@pytest.mark.parametrize('d', DIMS)
def test_one_large_block_among_small_ones(d):
    """Rows 256 .. 511 at scale 1e3, the others at 1e-2: nmax_J differs by ten orders of magnitude between column blocks -- the bound's per-block term."""
    rng = np.random.default_rng(10)
    X = rng.normal(0, 1, (600, d))
    X[:256] *= 1e-2
    X[256:512] *= 1e3
    X[512:] *= 1e-2
    X = X.astype(np.float32)
    c = X.mean(0, keepdims=True)
    check_numerics('one block at 1e3 among blocks at 1e-2', X, c, probe(X, c))


@pytest.mark.parametrize('d', DIMS)
def test_power_of_two_scaling_is_exact(d):
    """a(2^s X, 2^s c) == 2^(2s) a(X, c) bit for bit, s = +-16: nothing in the range the callers use is flushed or saturated."""
    X, c = gaussian(600, d, seed=12)
    base = probe(X, c)
    check_numerics('gaussian N=600', X, c, base)
    for s in (16, -16):
        f = np.float32(2.0 ** s)
        r = probe(X * f, c * f)
        np.testing.assert_array_equal(bits(r.a), bits(base.a * f * f), err_msg='s=%d' % s)
        np.testing.assert_array_equal(bits(r.nrm), bits(base.nrm * f * f))
        check_numerics('gaussian N=600 scaled by 2^%d' % s, X * f, c * f, r)
