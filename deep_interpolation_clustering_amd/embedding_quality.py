"""Is a two-dimensional map of the latents to be believed?  Trustworthiness, continuity (Venna and Kaski 2001) and the share of neighbours kept, for maps of
any size: the figures that rank the maps of ``tsne.tsne_sweep`` -- KL is not comparable across perplexities, because P itself changes; these are.

    T(k) = 1 - 2 / (N k (2N - 3k - 1)) * sum_i sum_{j in U_i} (rank_X(i, j) - k)
        U_i: the k nearest MAP neighbours of i that are not among its k nearest INPUT-space neighbours; rank_X(i, j): where j stands among the input-space
        neighbours of i.  Low T: the map shows neighbours that are none (false neighbours).  ``sklearn.manifold.trustworthiness(X, Y, n_neighbors=k)``.
    C(k): the same with the two spaces swapped -- the input-space neighbours missing from the map's k nearest, ranked in the map.  Low C: the map tears
        neighbourhoods apart.  ``sklearn.manifold.trustworthiness(Y, X, n_neighbors=k)``.
    kept(k) = mean_i |kNN_X(i) n kNN_Y(i)| / k.

Neighbours and ranks are the package's (include/dic_hip.h: dic_knn_neighbors, dic_knn_ranks): the order of a row is by (d2, index), d2 the f64 difference-form
squared distance of the f32 coordinates, the row's own index dropped; rank(i, j) = 1 + #{l != i : (d2(i, l), l) < (d2(i, j), j)}.  MAP PRECISION: the map is
f64 and the neighbour machinery is f32, so the map-side lists and ranks are those of the map ROUNDED TO f32 -- at |Y| around 50 a grid of 4e-6; two map points
closer than that tie and the smaller index comes first.

sklearn builds the N x N distance matrix and a full argsort (45 GB in f64 at 75 000 points).  Here nothing N x N is stored: one ``kneighbors`` self join per
space at max(ks) + 1, and one ``neighbor_ranks`` call per space, for the entries of the other space's lists that are missing from this space's own (an entry
present in the list has its position as rank and needs no kernel).  Every smaller k comes from prefixes of the sorted lists; the sums are integers, so every
k of a sweep has the bits of its stand-alone call.  ``quality_from_lists`` -- lists and ranks in, (T, C, kept) out -- is pure numpy.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from .knn import MAX_NEIGHBORS, _shape_of, kneighbors, neighbor_ranks


# ------------------------------------------------------------------------------------------------------------------------------------ pure numpy
def check_ks(ks, n):
    """The sorted distinct ks as ints; sklearn's refusal of ``n_neighbors >= n_samples / 2`` (the normaliser 2N - 3k - 1 must stay positive)."""
    if isinstance(ks, (numbers.Integral, np.integer)):
        ks = (ks,)
    out = []
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
            raise ValueError('n_neighbors must be an integer, got %r' % (k,))
        if k < 1:
            raise ValueError('Expected n_neighbors > 0. Got %d' % k)
        if k >= n / 2:
            raise ValueError('n_neighbors (%d) should be less than n_samples / 2 (%s)' % (k, n / 2))
        out.append(int(k))
    if not out:
        raise ValueError('ks must name at least one n_neighbors')
    return sorted(set(out))


def positions_in(own, other):
    """(N, k) int64: for every entry of ``other`` its 1-based position in the same row of ``own`` (both (N, k) index lists, entries of a row distinct), 0 where
    the row of ``own`` does not hold it."""
    own, other = np.asarray(own), np.asarray(other)
    pos = np.zeros(other.shape, dtype=np.int64)
    for r0 in range(0, len(own), 4096):
        eq = other[r0:r0 + 4096, :, None] == own[r0:r0 + 4096, None, :]
        pos[r0:r0 + 4096] = np.where(eq.any(2), eq.argmax(2) + 1, 0)
    return pos


def merged_ranks(own, other, ranks):
    """(N, k) int64: the rank, in the space of the lists ``own``, of every entry of ``other``: its position where ``own`` holds it (a sorted list without
    the row's own index: position = rank), else the entry of ``ranks`` (from ``neighbor_ranks``; read only there)."""
    pos = positions_in(own, other)
    r = np.where(pos > 0, pos, np.asarray(ranks, dtype=np.int64))
    if (r <= 0).any():
        raise ValueError('a list entry has neither a position nor a rank')
    return r


def quality_from_lists(idx_x, idx_y, rank_x, rank_y, ks):
    """``{k: (T, C, kept)}`` from the sorted neighbour lists of the two spaces and the ranks of the entries each space's list lacks.

    ``idx_x``, ``idx_y`` (N, K): the K nearest neighbours of every point in the input space and on the map, the point itself dropped, sorted by
    (distance, index); K >= max(ks).  ``rank_x`` (N, K): rank_X(i, idx_y[i, c]), read only where idx_x[i] does not hold idx_y[i, c] (anything elsewhere);
    ``rank_y`` likewise with the spaces swapped.  A point is among the k nearest of a space iff its rank there is <= k, so with r = the merged ranks
        T(k) = 1 - 2 / (N k (2N - 3k - 1)) sum over the first k columns of max(r_x - k, 0),   kept(k) = #{r_x <= k in the first k columns} / (N k),
    and C(k) from r_y.  The sums are integers: no summation order, and a k of a sweep has the bits of its own call."""
    idx_x, idx_y = np.asarray(idx_x), np.asarray(idx_y)
    if idx_x.ndim != 2 or idx_x.shape != idx_y.shape:
        raise ValueError('idx_x and idx_y must be (n_samples, K) both, got %s and %s' % (idx_x.shape, idx_y.shape))
    n, width = idx_x.shape
    ks = check_ks(ks, n)
    if ks[-1] > width:
        raise ValueError('the lists hold %d neighbours, n_neighbors = %d needs as many' % (width, ks[-1]))
    rx = merged_ranks(idx_x, idx_y, rank_x)
    ry = merged_ranks(idx_y, idx_x, rank_y)
    out = {}
    for k in ks:
        norm = 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
        ex, ey = rx[:, :k] - k, ry[:, :k] - k
        t = 1.0 - norm * float(int(ex[ex > 0].sum()))
        c = 1.0 - norm * float(int(ey[ey > 0].sum()))
        out[k] = (t, c, float(int((ex <= 0).sum())) / float(n * k))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------- device
def drop_own(idx):
    """The (N, k + 1) raw self-join lists without the row's own index, (N, k), still sorted: the k nearest OTHER points.  Where the own index is not among
    the k + 1 (k + 1 or more duplicates of the point sort before it) all of them are other points and the last is dropped -- so that position = rank
    always.  (t-SNE's ``drop_self`` follows sklearn's ``kneighbors(X=None)`` there and drops the first.)  A torch tensor, on its device."""
    n, k1 = idx.shape
    keep = idx != torch.arange(n, dtype=idx.dtype, device=idx.device)[:, None]
    keep[keep.all(dim=1), k1 - 1] = False
    return idx[keep].reshape(n, k1 - 1)


def _own_lists(Z, k, raw_idx=None):
    """The k nearest others of every row of ``Z`` (device, int32).  ``raw_idx``: raw self-join lists at least k + 1 wide, whose first k + 1 columns are the
    lists of a join of their own."""
    if raw_idx is None or raw_idx.shape[1] < k + 1:
        raw_idx = kneighbors(Z, k + 1, return_device=True)[1]
    return drop_own(raw_idx[:, :k + 1].contiguous())


def _missing_ranks(Z, own, other, stats=None):
    """(N, k) int32 numpy: rank in the space of ``Z`` of the entries of ``other`` that ``own`` (the lists of ``Z``) lacks, 0 elsewhere.  The missing entries
    of a row are moved to the front (a stable sort: one kernel pass serves 8 targets, and a row lacks few), ranked by one ``neighbor_ranks`` call and put back."""
    n, k = own.shape
    missing = ~(other[:, :, None] == own[:, None, :]).any(dim=2) if n * k * k <= (1 << 28) else torch.cat(
        [~(other[r:r + 65536, :, None] == own[r:r + 65536, None, :]).any(dim=2) for r in range(0, n, 65536)])
    m = int(missing.sum(dim=1).max())
    ranks = torch.zeros((n, k), dtype=torch.int32, device=own.device)
    if stats is not None:
        stats.update(targets=int(missing.sum()), targets_per_row_max=m)
    if m == 0:
        return ranks.cpu().numpy()
    order = torch.sort((~missing).to(torch.int8), dim=1, stable=True).indices[:, :m]          # the columns of the missing entries first, in their order
    front = torch.gather(missing, 1, order)
    targets = torch.where(front, torch.gather(other, 1, order), torch.full_like(order, -1, dtype=other.dtype)).to(torch.int32).contiguous()
    st = {}
    got = neighbor_ranks(Z, targets, stats=st, return_device=True)
    if stats is not None:
        stats.update(st)
    ranks.scatter_(1, order, torch.where(front, got, torch.zeros_like(got)))
    return ranks.cpu().numpy()


def _on_device(Z):
    z = torch.as_tensor(Z)
    if not z.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('deep_interpolation_clustering_amd.embedding_quality runs only on an MI355X; there is no CPU path by design')
        z = z.to('cuda')
    return z.to(torch.float32).contiguous()          # (the map: rounded to f32 here -- module docstring)


def embedding_quality(X, Y, ks=(5, 10, 30), stats=None, _x_raw_idx=None):
    """``{k: (trustworthiness, continuity, neighbors_kept)}`` of the map ``Y`` (N, d) of the points ``X`` (N, D) for every k of ``ks``, from ONE computation
    (module docstring): numpy arrays or tensors, D and d <= 256, every k < N / 2 and <= 1023.  The map is rounded to f32.  ``stats`` (a dict, optional)
    receives ``x`` and ``y``: per space the targets ranked by the kernel and ``neighbor_ranks``' own figures."""
    n, _ = _shape_of(X)
    ny, _ = _shape_of(Y)
    if ny != n:
        raise ValueError('Found input variables with inconsistent numbers of samples: [%d, %d]' % (n, ny))
    ks = check_ks(ks, n)
    kmax = ks[-1]
    if kmax + 1 > MAX_NEIGHBORS:
        raise NotImplementedError('embedding_quality: at most %d neighbours (got %d)' % (MAX_NEIGHBORS - 1, kmax))
    x, y = _on_device(X), _on_device(Y)
    lx, ly = _own_lists(x, kmax, _x_raw_idx), _own_lists(y, kmax)
    sx, sy = {}, {}
    rank_x = _missing_ranks(x, lx, ly, sx)          # the map's neighbours, ranked in the input space
    rank_y = _missing_ranks(y, ly, lx, sy)          # the input space's neighbours, ranked on the map
    if stats is not None:
        stats.update(x=sx, y=sy)
    return quality_from_lists(lx.cpu().numpy(), ly.cpu().numpy(), rank_x, rank_y, ks)


def _single(X, Y, n_neighbors, which):
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (numbers.Integral, np.integer)):
        raise ValueError('n_neighbors must be an integer, got %r' % (n_neighbors,))
    return embedding_quality(X, Y, (n_neighbors,))[int(n_neighbors)][which]


def trustworthiness(X, Y, n_neighbors=5):
    """``sklearn.manifold.trustworthiness(X, Y, n_neighbors=n_neighbors)`` for the euclidean metric (module docstring)."""
    return _single(X, Y, n_neighbors, 0)


def continuity(X, Y, n_neighbors=5):
    """Trustworthiness with the two spaces swapped: ``sklearn.manifold.trustworthiness(Y, X, n_neighbors=n_neighbors)`` (module docstring)."""
    return _single(X, Y, n_neighbors, 1)


def neighbors_kept(X, Y, n_neighbors=5):
    """The mean share of a point's ``n_neighbors`` nearest input-space neighbours that are among its ``n_neighbors`` nearest on the map."""
    return _single(X, Y, n_neighbors, 2)
