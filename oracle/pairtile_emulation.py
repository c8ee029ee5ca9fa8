"""NumPy emulation of the pair-tile arithmetic (csrc/dic_pairtile.h) as dic_cluster_pair_rowsums uses it (TEST INFRASTRUCTURE ONLY).

What the kernels do to a pair (i, j), restated step by step:

  * v = fl32(x - centre), one centre for all points (the f64 mean rounded to f32);
  * every coordinate splits as h = bf16(v), l = bf16(v - h), round to nearest even; operand j carries -2 h, -2 l (exact);
  * n = the f32 norm of v: per group of four coordinates fma(v0, v0, fma(v1, v1, fma(v2, v2, v3 v3))), the 64 groups of a 256-wide row
    added by an xor butterfly (1, 2, 4, .. 32), every step rounded to f32; n as three bf16 pieces n0 + n1 + n2;
  * a_ij, the approximate d^2, is ONE f32 accumulator: for every 16 coordinates three MFMAs in this order, hi_j . hi_i, lo_j . hi_i,
    hi_j . lo_i (lo . lo is dropped), then one MFMA of the norm columns (n0_i + n1_i + n2_i + n0_j + n1_j + n2_j).  A product of two
    bf16 values is exact in f32; the sum of an MFMA's 16 products is taken here as exact and the addition to the accumulator as ONE
    rounding to f32 (the order inside the instruction is not documented: this is the optimistic reading, 3 D / 16 + 1 roundings);
  * d_ij = sqrt_f32(max(a_ij, 0)), i == j masked; the row sums are added here in f64 (the kernel adds 64 terms, then slots, in f32:
    a relative 1e-7 on a sum, far below what is studied here).

So this file emulates the cancellation of the norm form, which is what moves the silhouette on tight clusters, and not the last bits
of the summation."""
import numpy as np

from . import cluster_stats_oracle as CO


def bf16(v):
    """f32 -> the nearest bf16 (ties to even), returned as f32."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(v))


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # (the product is exact in f64)


def planes(x, centre=None):
    """(v, h, l, n): the centred f32 points, their bf16 pieces and the f32 norms of pt_prep_row."""
    x = np.asarray(x, dtype=np.float32)
    if centre is None:
        centre = x.astype(np.float64).mean(0).astype(np.float32)
    n_pts, d = x.shape
    v = np.zeros((n_pts, 256), np.float32)
    v[:, :d] = x - np.asarray(centre, np.float32)
    h = bf16(v)
    l = bf16(v - h)
    g = v.reshape(n_pts, 64, 4)
    nrm = _fma32(g[..., 0], g[..., 0], _fma32(g[..., 1], g[..., 1], _fma32(g[..., 2], g[..., 2], g[..., 3] * g[..., 3])))
    for o in (1, 2, 4, 8, 16, 32):
        nrm = nrm + nrm[:, np.arange(64) ^ o]                   # f32 + f32 -> f32, both lanes of a pair get the same sum
    width = -(-d // 16) * 16
    return v[:, :width], h[:, :width], l[:, :width], np.ascontiguousarray(nrm[:, 0])


def approx_d2(x, centre=None):
    """(N, N) f32: a_ij for every ordered pair, i the row (operand i), j the column."""
    v, h, l, nrm = planes(x, centre)
    n_pts = len(v)
    acc = np.zeros((n_pts, n_pts), np.float32)
    h64, l64 = h.astype(np.float64), l.astype(np.float64)
    for c0 in range(0, v.shape[1], 16):                          # (all-zero chunks of a padded row add exact zeros)
        hi, li = h64[:, c0:c0 + 16], l64[:, c0:c0 + 16]
        hj, lj = -2.0 * hi, -2.0 * li
        for a, b in ((hi, hj), (hi, lj), (li, hj)):
            acc = (acc.astype(np.float64) + a @ b.T).astype(np.float32)
    n0 = bf16(nrm)
    n1 = bf16(nrm - n0)
    n2 = bf16((nrm - n0) - n1)
    ns = n0.astype(np.float64) + n1.astype(np.float64) + n2.astype(np.float64)
    return (acc.astype(np.float64) + ns[:, None] + ns[None, :]).astype(np.float32)


def row_sums(x, labels):
    """(labels 0..K-1, K, S (N, K) f64): S[i][c] = sum_{j in c, j != i} sqrt_f32(max(a_ij, 0))."""
    lab, K = CO.encode(labels)
    dist = np.sqrt(np.maximum(approx_d2(x), np.float32(0)))
    np.fill_diagonal(dist, 0)
    S = np.stack([dist[:, lab == c].sum(1, dtype=np.float64) for c in range(K)], axis=1)
    return lab, K, S


def silhouette_from_sums(lab, K, S):
    """cluster_stats_oracle.silhouette's reduction, from given sums."""
    cnt = np.bincount(lab, minlength=K).astype(np.float64)
    rows = np.arange(len(lab))
    with np.errstate(divide='ignore', invalid='ignore'):
        intra = S[rows, lab] / (cnt[lab] - 1)
        mean_to = S / cnt
        mean_to[rows, lab] = np.inf
        inter = mean_to.min(1)
        sil = (inter - intra) / np.maximum(intra, inter)
    return np.nan_to_num(sil)


def compare(x, labels):
    """{'f64', 'own', 'all': the mean silhouette in f64, with the own-cluster sums emulated, with all sums emulated; 'own_sums': the largest relative deviation
    of a cluster's total of own-cluster sums, sum_{i, j in c} d_ij (what the inertias are made of), over the clusters where it is not zero}."""
    lab, K, S64, _, _ = CO.pair_stats(x, labels)
    _, _, Se = row_sums(x, labels)
    rows = np.arange(len(lab))
    Sown = S64.copy()
    Sown[rows, lab] = Se[rows, lab]
    out = {name: float(silhouette_from_sums(lab, K, S).mean()) for name, S in (('f64', S64), ('own', Sown), ('all', Se))}
    t64, te = (np.bincount(lab, weights=S[rows, lab], minlength=K) for S in (S64, Se))
    out['own_sums'] = float((np.abs(te - t64)[t64 > 0] / t64[t64 > 0]).max())
    return out


def silhouettes(x, labels):
    """(f64, own-cluster sums emulated, all sums emulated): the three mean silhouettes of one labelling."""
    c = compare(x, labels)
    return c['f64'], c['own'], c['all']


def geometry_ratios(x, labels):
    """The three f64 quantities the routing of cluster_stats.pair_stats compares: (smallest mean squared radius of a cluster of two or
    more points, smallest squared distance of two centroids, largest mean over a cluster of the squared distance from the mean of all points)."""
    lab, K = CO.encode(labels)
    x = np.asarray(x, dtype=np.float64)
    cnt = np.bincount(lab, minlength=K)
    cen = np.stack([x[lab == c].mean(0) for c in range(K)])
    r2 = np.array([((x[lab == c] - cen[c]) ** 2).sum(1).mean() for c in range(K)])
    sep = ((cen[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
    sep[np.arange(K), np.arange(K)] = np.inf
    far = ((x - x.mean(0)) ** 2).sum(1)
    far = max(far[lab == c].mean() for c in range(K))
    return float(r2[cnt > 1].min()) if (cnt > 1).any() else float('inf'), float(sep.min()), float(far)
