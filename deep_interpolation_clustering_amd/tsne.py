"""Exact t-SNE of the latents on the MI355X (``sklearn.manifold.TSNE(method='exact')`` on neighbour-based affinities): the two-dimensional map every
``plot/<method>_labels.csv`` of p2 can be drawn on.  The p2 / p4 ``--embed tsne`` branches.

The definition is stated once, in include/dic_hip.h (dic_tsne_perplexity); in short: the conditional p_j|i over the ``int(3 perplexity + 1)`` nearest
neighbours of i (``knn.kneighbors``, the point itself left out) at the precision beta_i whose entropy is log(perplexity), found by sklearn's bracket-and-bisect
search; P = (p_j|i + p_i|j) / total as a symmetric CSR; then sklearn's gradient descent on KL(P || Q), Q the Student-t affinities of the (N, 2) map: 250
iterations with P exaggerated at momentum 0.5, the rest at momentum 0.8, gains as ``_gradient_descent`` keeps them, progress checked every 50 iterations.

sklearn's default for 75 000 points is Barnes-Hut on the CPU: approximate (``angle``) and many minutes.  Here the repulsion is the exact sum over all N^2
pairs, every iteration, in f64 (csrc/dic_tsne.hip): one all-pairs pass over the map and one sparse pass over P per iteration, no tree and no angle.  Every
sum has a fixed order, there are no floating-point atomics, and two fits give the same bits.  f64 is not a luxury: the exaggerated phase amplifies a relative
gradient error of 1e-7 to O(1) of the map within 50 iterations (scripts/tsne_probe.py), so f32 pair terms would make the map depend on the summation order.

Not provided: more than two components, Barnes-Hut / FFT variants, metrics other than euclidean, and a re-optimised ``transform`` -- ``transform`` is a
placement of new points among the fitted ones, not a fit.  The package imports neither sklearn nor scipy.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import _native as N
from .dbscan import MAX_DIM
from .knn import MAX_NEIGHBORS, _shape_of, kneighbors

EXPLORATION_ITER = 250          # sklearn's _EXPLORATION_MAX_ITER: the iterations with P exaggerated, at momentum 0.5
N_ITER_CHECK = 50               # sklearn's _N_ITER_CHECK
ENTROPY_TOL = 1e-10             # csrc/dic_tsne.hip: TS_ENTROPY_TOL
MAX_STEPS = 200                 # csrc/dic_tsne.hip: TS_MAX_STEPS


# ------------------------------------------------------------------------------------------------------------------------------------------ checks
def n_neighbors_of(perplexity, n):
    """sklearn's ``min(n_samples - 1, int(3. * perplexity + 1))``."""
    return min(n - 1, int(3.0 * perplexity + 1))


def _check(n, d, perplexity, n_components=2):
    """The refusals that need no GPU: raised before any device work."""
    if n_components != 2:
        raise ValueError('tsne: n_components must be 2 (the kernels hold a two-dimensional map), got %r' % (n_components,))
    if isinstance(perplexity, bool) or not isinstance(perplexity, (numbers.Real, np.floating, np.integer)) or not perplexity > 0 or not math.isfinite(perplexity):
        raise ValueError('perplexity must be a positive number, got %r' % (perplexity,))
    if perplexity >= n - 1:
        raise ValueError('perplexity must be less than n_samples - 1 (its %d neighbours leave the point itself out), got perplexity=%g, n_samples=%d'
                         % (int(3.0 * perplexity + 1), perplexity, n))
    if int(3.0 * perplexity + 1) + 1 > MAX_NEIGHBORS:
        raise ValueError('perplexity=%g needs lists of int(3 perplexity + 1) + 1 = %d neighbours; kneighbors gives at most %d'
                         % (perplexity, int(3.0 * perplexity + 1) + 1, MAX_NEIGHBORS))
    if d > MAX_DIM:
        raise ValueError('tsne: at most %d features (got %d)' % (MAX_DIM, d))


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('deep_interpolation_clustering_amd.tsne runs only on an MI355X; there is no CPU path by design')
    return torch.device('cuda', torch.cuda.current_device())


def _f64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, device=dev).to(torch.float64).contiguous()


# -------------------------------------------------------------------------------------------------------------------------------------- affinities
def drop_self(dist, idx):
    """The (N, k + 1) self-join lists without the point itself, (N, k), as sklearn's ``kneighbors(X=None)`` leaves it out: the entry whose index is the
    row's own is dropped; where it is not among them (k + 1 or more duplicates of the point sort before it) the first entry is.  Device tensors."""
    n, k1 = idx.shape
    keep = idx != torch.arange(n, dtype=idx.dtype, device=idx.device)[:, None]
    keep[keep.all(dim=1), 0] = False
    return dist[keep].reshape(n, k1 - 1), idx[keep].reshape(n, k1 - 1)


def conditional_probabilities(d2, perplexity):
    """``(beta (M,), p (M, k))`` f64 device tensors from the (M, k) squared distances ``d2`` (device, f64): the row minimum is subtracted here and
    dic_tsne_perplexity finds every row's precision."""
    d2 = d2.to(torch.float64)
    r = (d2 - d2.amin(dim=1, keepdim=True)).contiguous()
    m, k = r.shape
    beta = torch.empty(m, dtype=torch.float64, device=r.device)
    p = torch.empty_like(r)
    N.check(N.lib().dic_tsne_perplexity(N.ptr(r), m, k, float(perplexity), N.ptr(beta), N.ptr(p), N.stream_of(r)), 'dic_tsne_perplexity')
    return beta, p


def symmetrise(idx, p):
    """The CSR ``(indptr (N + 1) int64, indices int32 ascending within a row, data f64)`` of (p_j|i + p_i|j) / total from the lists ``idx`` (N, k) and
    their conditional ``p`` (N, k), on their device.  One sort of the 2 N k keys i N + j; a key occurs at most twice (the entries of a list are distinct),
    and a sum of two addends is the same in either order, so P_ij and P_ji have the same bits."""
    n, k = idx.shape
    dev = idx.device
    rows = torch.arange(n, dtype=torch.int64, device=dev).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    keys, order = torch.sort(torch.cat([rows * n + cols, cols * n + rows]))
    vals = torch.cat([p.reshape(-1), p.reshape(-1)])[order]
    del rows, cols, order
    first = torch.ones(keys.shape[0], dtype=torch.bool, device=dev)
    first[1:] = keys[1:] != keys[:-1]
    twin = torch.zeros_like(vals)
    twin[:-1] = torch.where(first[1:], torch.zeros_like(vals[1:]), vals[1:])
    data = (vals + twin)[first]
    keys = keys[first]
    ri = torch.div(keys, n, rounding_mode='floor')
    indices = (keys - ri * n).to(torch.int32)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(ri, minlength=n), 0)
    return indptr, indices, (data / data.sum()).contiguous()


def _lists(X, k1):
    """The raw self-join lists of ``k1`` neighbours (the point itself among them), on the device."""
    return kneighbors(X, k1, return_device=True)


def _joint(X, perplexity, lists=None):
    """``(graph, beta)`` on the device.  ``lists``: raw self-join lists at least ``k + 1`` wide (``tsne_sweep``); their first k + 1 columns are the lists of a
    join of their own, so every perplexity of a sweep gets the bits of its stand-alone fit."""
    n, d = _shape_of(X)
    _check(n, d, perplexity)
    k = n_neighbors_of(perplexity, n)
    dist, idx = _lists(X, k + 1) if lists is None else lists
    dist, idx = drop_self(dist[:, :k + 1], idx[:, :k + 1])
    beta, p = conditional_probabilities(dist * dist, perplexity)
    return symmetrise(idx, p), beta


def joint_probabilities(X, perplexity, return_device=False):
    """The symmetric affinities P of ``X`` (numpy array or tensor, (N, D), D <= 256) as the CSR triple ``(indptr, indices, data)``: one ``kneighbors`` self
    join, the perplexity kernel and one sort (module docstring).  numpy, or device tensors with ``return_device=True``."""
    n, d = _shape_of(X)
    _check(n, d, perplexity)
    graph, _ = _joint(X, perplexity)
    return graph if return_device else tuple(t.cpu().numpy() for t in graph)


def _graph_on(P, dev):
    indptr, indices, data = P
    return (torch.as_tensor(indptr, device=dev).to(torch.int64).contiguous(), torch.as_tensor(indices, device=dev).to(torch.int32).contiguous(),
            _f64(data, dev))


def _plogp(data):
    """sum P log P over the stored entries (0 log 0 = 0), on the host: numpy's pairwise sum, the same bits every time."""
    v = data.cpu().numpy()
    v = v[v > 0]
    return float(np.sum(v * np.log(v)))


# ---------------------------------------------------------------------------------------------------------------------------------------- descent
class _Descent:
    """The device state of one descent: the graph, the two map buffers, update and gains, and the workspace the two kernels share."""

    def __init__(self, graph, Y):
        self.indptr, self.indices, self.data = graph
        self.n = Y.shape[0]
        dev = Y.device
        L = N.lib()
        self.ws = torch.empty(max(16, L.dic_tsne_repulsion_workspace(self.n)), dtype=torch.uint8, device=dev)
        self.partials = torch.empty((max(1, L.dic_tsne_step_partials(self.n)), 2), dtype=torch.float64, device=dev)
        self.Y, self.Ynext = Y, torch.empty_like(Y)
        self.update, self.gains = torch.zeros_like(Y), torch.ones_like(Y)
        self.plogp = _plogp(self.data)

    def _repulsion(self):
        N.check(N.lib().dic_tsne_repulsion(N.ptr(self.Y), self.n, N.ptr(self.ws), self.ws.numel(), N.stream_of(self.Y)), 'dic_tsne_repulsion')

    def _step(self, exaggeration, momentum, lr, update, grad):
        N.check(N.lib().dic_tsne_step(N.ptr(self.indptr), N.ptr(self.indices), N.ptr(self.data), self.n, self.indices.numel(), N.ptr(self.Y), N.ptr(self.ws),
                                      self.ws.numel(), float(exaggeration), float(momentum), float(lr), N.ptr(self.update if update else None),
                                      N.ptr(self.gains if update else None), N.ptr(self.Ynext if update else None), N.ptr(grad), N.ptr(self.partials),
                                      N.stream_of(self.Y)), 'dic_tsne_step')

    def step(self, exaggeration, momentum, lr):
        """One iteration: the gradient at Y, the update, Y <- Y + update.  ``read()`` afterwards gives the error and gradient norm AT the old Y."""
        self._repulsion()
        self._step(exaggeration, momentum, lr, True, None)
        self.Y, self.Ynext = self.Ynext, self.Y

    def gradient(self, exaggeration):
        grad = torch.empty_like(self.Y)
        self._repulsion()
        self._step(exaggeration, 0.0, 0.0, False, grad)
        return grad

    def read(self, exaggeration):
        """``(kl, |grad|, Z)`` of the last kernel pass, the partials added on the host (numpy's pairwise sum)."""
        part = self.partials.cpu().numpy()
        z = float(self.ws[:8].view(torch.float64).cpu().numpy()[0])
        e = float(exaggeration)
        kl = e * (self.plogp + math.log(e) + float(np.sum(part[:, 1])) + math.log(z))
        return kl, math.sqrt(float(np.sum(part[:, 0]))), z


def tsne_gradient(Y, P, exaggeration=1.0):
    """``(kl, grad (N, 2) f64 numpy, Z)`` of the map ``Y`` (N, 2) under the affinities ``P`` (a symmetric CSR triple, as ``joint_probabilities`` gives it)
    with P multiplied by ``exaggeration``: one repulsion pass over all pairs and the attractive pass over P, no update -- sklearn's ``_kl_divergence``."""
    dev = _device()
    Yd = _f64(Y, dev)
    if Yd.dim() != 2 or Yd.shape[1] != 2:
        raise ValueError('Y must be (n_samples, 2), got shape %s' % (tuple(Yd.shape),))
    graph = _graph_on(P, dev)
    if graph[0].shape[0] != Yd.shape[0] + 1:
        raise ValueError('P has %d rows, Y has %d' % (graph[0].shape[0] - 1, Yd.shape[0]))
    run = _Descent(graph, Yd)
    grad = run.gradient(exaggeration)
    kl, _, z = run.read(exaggeration)
    return kl, grad.cpu().numpy(), z


def tsne_descend(Y, P, n_iter, exaggeration=1.0, momentum=0.8, learning_rate=200.0):
    """The (N, 2) f64 numpy map after ``n_iter`` iterations of the update rule from ``Y`` (update 0, gains 1) under the affinities ``P`` at a fixed
    ``exaggeration``, ``momentum`` and ``learning_rate``, no checks: the repulsion and step kernels as ``TSNE.fit`` runs them within one phase."""
    dev = _device()
    Yd = _f64(Y, dev).clone()
    if Yd.dim() != 2 or Yd.shape[1] != 2:
        raise ValueError('Y must be (n_samples, 2), got shape %s' % (tuple(Yd.shape),))
    run = _Descent(_graph_on(P, dev), Yd)
    for _ in range(int(n_iter)):
        run.step(exaggeration, momentum, learning_rate)
    return run.Y.cpu().numpy()


# -------------------------------------------------------------------------------------------------------------------------------------------- init
def pca_init(X, dev):
    """sklearn's ``init='pca'``: the scores of the two leading principal components, the sign of a component fixed by ``svd_flip`` (its entry of largest
    magnitude positive), divided by the standard deviation of the first column and multiplied by 1e-4.  The D x D covariance and the scores are torch f64
    on the device; the eigenvectors come from numpy's ``eigh`` on the host."""
    x = _f64(X, dev)
    xc = x - x.mean(dim=0, keepdim=True)
    w, v = np.linalg.eigh((xc.T @ xc).cpu().numpy())
    comp = v[:, np.argsort(w)[::-1][:2]].T.copy()          # (2, D)
    if comp.shape[0] < 2:
        comp = np.vstack([comp, np.zeros_like(comp)])          # (D = 1: a flat second column)
    at = np.argmax(np.abs(comp), axis=1)
    sign = np.sign(comp[np.arange(2), at])
    comp *= np.where(sign == 0, 1.0, sign)[:, None]
    Y = xc @ torch.as_tensor(comp.T.copy(), device=dev)
    return (Y / Y[:, 0].std(unbiased=False) * 1e-4).contiguous()


def _random_state(rs):
    if rs is None or rs is np.random:
        return np.random.mtrand._rand
    if isinstance(rs, (numbers.Integral, np.integer)):
        return np.random.RandomState(rs)
    return rs


class TSNE:
    """``sklearn.manifold.TSNE(n_components=2, method='exact', ...)`` on neighbour-based affinities (module docstring).  ``X``: a numpy array or a device
    tensor, (N, D), D <= 256.  After ``fit``: ``embedding_`` (N, 2) f64, ``kl_divergence_``, ``n_iter_`` (the iterations done: sklearn reports the index of
    the last one), ``learning_rate_``, ``kl_history_`` (a list of (iteration, kl) at every check, every 50 iterations, and at the last iteration; during
    the exaggerated phase the error is that of the exaggerated P, as sklearn's), ``betas_`` (N,), ``affinities_`` (the CSR triple indptr, indices, data).
    A gradient norm at or below ``min_grad_norm`` at a check ends the fit; ``n_iter_without_progress`` applies after the exaggerated phase.  An array
    ``init`` is used in f64 as it is.

    ``transform(Q)`` is a PLACEMENT, not a fit: nothing is optimised and the fitted map does not move.  Every query is put at the p-weighted mean of the
    map positions of its ``int(3 perplexity + 1)`` nearest training points, the weights the conditional p of the same perplexity search on the query's
    distances to them.  It is deterministic, and a query that coincides with a training point need not land on it."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, n_iter_without_progress=300,
                 min_grad_norm=1e-7, init='pca', random_state=None):
        if n_components != 2:
            raise ValueError('tsne: n_components must be 2 (the kernels hold a two-dimensional map), got %r' % (n_components,))
        if isinstance(init, str) and init not in ('pca', 'random'):
            raise ValueError("init must be 'pca', 'random' or an (n_samples, 2) array, got %r" % (init,))
        if not (learning_rate == 'auto' or (isinstance(learning_rate, (numbers.Real, np.floating, np.integer)) and learning_rate > 0)):
            raise ValueError("learning_rate must be 'auto' or a positive number, got %r" % (learning_rate,))
        if not early_exaggeration >= 1:
            raise ValueError('early_exaggeration must be >= 1, got %r' % (early_exaggeration,))
        if int(max_iter) < EXPLORATION_ITER:
            raise ValueError('max_iter must be >= %d (the exaggerated phase), got %r' % (EXPLORATION_ITER, max_iter))
        self.n_components, self.perplexity, self.early_exaggeration, self.learning_rate = n_components, perplexity, early_exaggeration, learning_rate
        self.max_iter, self.n_iter_without_progress, self.min_grad_norm, self.init, self.random_state = max_iter, n_iter_without_progress, min_grad_norm, init, random_state

    def _initial(self, X, n, dev):
        if isinstance(self.init, str):
            if self.init == 'pca':
                return pca_init(X, dev)
            return _f64(1e-4 * _random_state(self.random_state).standard_normal((n, 2)), dev)
        Y = _f64(self.init, dev).clone()
        if tuple(Y.shape) != (n, 2):
            raise ValueError('init must be (n_samples, 2) = (%d, 2), got shape %s' % (n, tuple(Y.shape)))
        return Y

    def fit(self, X, y=None, _lists=None):
        n, d = _shape_of(X)
        _check(n, d, self.perplexity, self.n_components)
        if not isinstance(self.init, str) and tuple(np.shape(self.init)) != (n, 2):
            raise ValueError('init must be (n_samples, 2) = (%d, 2), got shape %s' % (n, tuple(np.shape(self.init))))
        dev = X.device if isinstance(X, torch.Tensor) and X.is_cuda else _device()
        lists = kneighbors(X, n_neighbors_of(self.perplexity, n) + 1, return_device=True) if _lists is None else _lists
        graph, beta = _joint(X, self.perplexity, lists)
        self._raw_idx = lists[1]          # the raw self-join lists: ``quality`` takes the input-space neighbours from them
        ee = float(self.early_exaggeration)
        lr = max(n / ee / 4.0, 50.0) if self.learning_rate == 'auto' else float(self.learning_rate)
        run = _Descent(graph, self._initial(X, n, dev))
        max_iter = int(self.max_iter)
        history = []
        done, best, best_at, kl = 0, math.inf, 0, math.nan
        stopped = False
        for first, last, e, momentum, patience in ((0, EXPLORATION_ITER, ee, 0.5, EXPLORATION_ITER), (EXPLORATION_ITER, max_iter, 1.0, 0.8,
                                                                                                      int(self.n_iter_without_progress))):
            best, best_at = math.inf, first
            for i in range(first, last):
                run.step(e, momentum, lr)
                done = i + 1
                check = (i + 1) % N_ITER_CHECK == 0
                if check or i == last - 1:
                    kl, gnorm, _ = run.read(e)
                    history.append((i + 1, kl))
                if check:
                    if kl < best:
                        best, best_at = kl, i
                    elif i - best_at > patience:
                        break
                    if gnorm <= self.min_grad_norm:
                        stopped = True
                        break
            if stopped:
                break
        self.embedding_ = run.Y.cpu().numpy()
        self._Y = run.Y
        self._X = X
        self.kl_divergence_, self.n_iter_, self.learning_rate_, self.kl_history_ = kl, done, lr, history
        self.betas_ = beta.cpu().numpy()
        self.affinities_ = tuple(t.cpu().numpy() for t in graph)
        self.n_samples_fit_, self.n_features_in_ = n, d
        return self

    def quality(self, ks=(5,)):
        """``{k: (trustworthiness, continuity, neighbors_kept)}`` of the fitted map against the training points (embedding_quality.py: the map rounded to
        f32; every k < n_samples / 2) -- the figures that compare maps across perplexities, initialisations and methods, which KL does not.  The
        input-space neighbours come from the lists the fit (or its ``tsne_sweep``) joined, where they are wide enough: max(ks) <= int(3 perplexity + 1);
        the result is that of ``embedding_quality(X, embedding_, ks)`` either way."""
        if not hasattr(self, '_Y'):
            raise RuntimeError("This TSNE instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")
        from .embedding_quality import embedding_quality
        return embedding_quality(self._X, self.embedding_, ks, _x_raw_idx=self._raw_idx)

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_

    def transform(self, Q):
        """(M, 2) f64 numpy: the placement of the rows of ``Q`` on the fitted map (class docstring) -- not a fit."""
        if not hasattr(self, '_Y'):
            raise RuntimeError("This TSNE instance is not fitted yet. Call 'fit' with appropriate arguments before using this estimator.")
        m, d = _shape_of(Q)
        if d != self.n_features_in_:
            raise ValueError('X has %d features, but TSNE is expecting %d features as input.' % (d, self.n_features_in_))
        k = n_neighbors_of(self.perplexity, self.n_samples_fit_)
        dist, idx = kneighbors(self._X, k, Q=Q, return_device=True)
        _, p = conditional_probabilities(dist * dist, self.perplexity)
        return (p[:, :, None] * self._Y.to(p.device)[idx.long()]).sum(dim=1).cpu().numpy()


def tsne_sweep(X, perplexities, **kw):
    """{perplexity: fitted ``TSNE``} from ONE neighbour join, at the largest perplexity: the sorted lists of a smaller perplexity are prefixes of it, so
    every fit has the bits of its stand-alone fit.  ``kw``: the other arguments of ``TSNE``.  Every fit answers ``quality(ks)`` from the same join (the
    lists of the largest perplexity serve every map's input-space side), so the maps of a sweep can be ranked: KL cannot, P changes with the perplexity."""
    perplexities = list(perplexities)
    if not perplexities:
        raise ValueError('perplexities must name at least one perplexity')
    n, d = _shape_of(X)
    for u in perplexities:
        _check(n, d, u, kw.get('n_components', 2))
    fits = {u: TSNE(perplexity=u, **kw) for u in perplexities}          # (argument errors before any GPU work)
    lists = _lists(X, n_neighbors_of(max(perplexities), n) + 1)
    return {u: fits[u].fit(X, _lists=lists) for u in perplexities}
