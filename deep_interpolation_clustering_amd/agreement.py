"""Agreement of labellings with each other on the MI355X: sklearn.metrics.cluster's contingency table, pair confusion matrix, Rand, adjusted Rand,
Fowlkes-Mallows, mutual information, entropy, expected mutual information, NMI, AMI and homogeneity / completeness / V-measure (sklearn 1.7.2's names and
definitions), for ALL pairs of a set of labellings at once.

include/dic_hip.h states the definitions, the grouping of every floating-point expression and the order of every sum.  The label matrix is uploaded and
encoded once; csrc/dic_agreement.hip then runs three stages with the pairs as the second grid dimension: the contingency tables (integer atomics: exact),
per table the marginals, the integer sums, MI and the entropies, and the expected mutual information of the permutation model -- a sum of hypergeometric
terms over every cell of every table, the hot path (minutes to an hour for a sweep on the CPU).  ``ln m!`` is one host table (``math.lgamma``), uploaded
once; the device evaluates no lgamma.

Everything that is a function of integers -- pair confusion, Rand, ARI, FMI -- is formed here on the host from the device's integer sums with sklearn's own
expressions (Python ints where sklearn uses them: tp * tn leaves int64 from about N = 78 000), so it equals sklearn bit for bit.  NMI, AMI and V-measure are sklearn's
host expressions, special cases included, over the device's MI, EMI and entropies.

The single-pair functions are calls of ``agreement_matrix``'s machinery with one pair.  Labels are any integers; -1 is a class like any other
(``noise='class'``, sklearn's behaviour) or, with ``noise='drop'``, a row that says -1 in either labelling of a pair is left out of THAT pair.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import _native as N
from .utils import logger

NOISE = -1
INDICES = ('ari', 'ami', 'nmi', 'rand', 'fmi', 'vmeasure')
AVERAGE_METHODS = ('min', 'geometric', 'arithmetic', 'max')
NOISE_MODES = ('class', 'drop')
LDS_CELLS = 16384          # dic_agreement_lds_cells(): a table of at most this many cells is counted in LDS (test_agreement_host.py holds the two together)
EMI_COLS = 64              # columns per EMI work unit (include/dic_hip.h)
_CHUNK_CELLS = 1 << 27     # table cells per launch group (512 MB of int32): more pairs run as several groups, each pair with the bits of its own call
_EPS = float(np.finfo('float64').eps)


@functools.lru_cache(maxsize=4)
def log_factorials(n):
    """(n + 1,) f64, read-only: ``lf[m] = ln m!`` as ``math.lgamma(m + 1.0)`` -- THE table of the EMI kernel and of the tests' restatement."""
    lf = np.array([math.lgamma(m + 1.0) for m in range(int(n) + 1)], dtype=np.float64)
    lf.setflags(write=False)
    return lf


# ---- input ------------------------------------------------------------------------------------------------------------------------------------------------
def _is_integer_dtype(x):
    if torch.is_tensor(x):
        return x.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    return np.issubdtype(x.dtype, np.integer)


def _rows_of(labellings):
    """``(names, rows)``: the labellings as a list of 1-D integer arrays (or the rows of a tensor) of one length.  Every check of the input that needs no GPU."""
    if isinstance(labellings, dict):
        names, rows = list(labellings.keys()), [v if torch.is_tensor(v) else np.asarray(v) for v in labellings.values()]
    else:
        x = labellings if torch.is_tensor(labellings) else np.asarray(labellings)
        if x.ndim != 2:
            raise ValueError('labellings must be a {name: labels} dict or an (L, N) array, got shape %s' % (tuple(x.shape),))
        names, rows = list(range(x.shape[0])), [x[l] for l in range(x.shape[0])]
    if not rows:
        raise ValueError('no labellings given')
    for name, r in zip(names, rows):
        if r.ndim != 1:
            raise ValueError('labelling %r must be 1-D, got shape %s' % (name, tuple(r.shape)))
        if not _is_integer_dtype(r):
            raise ValueError('labelling %r must hold integers, got %s' % (name, r.dtype))
        if len(r) != len(rows[0]):
            raise ValueError('labellings of unequal lengths: %r has %d rows, %r has %d' % (names[0], len(rows[0]), name, len(r)))
    if len(rows[0]) == 0:
        raise ValueError('empty labellings')
    if len(rows[0]) >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 rows')
    return names, rows


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _encode(rows):
    """``(codes (L, N) int32 device tensor, classes)``: per labelling its sorted distinct ids and every row's index into them."""
    dev = _device()
    codes = torch.empty((len(rows), len(rows[0])), dtype=torch.int32, device=dev)
    classes = []
    for l, r in enumerate(rows):
        if torch.is_tensor(r):
            ids, inv = torch.unique(r.to(dev).long(), sorted=True, return_inverse=True)
            codes[l] = inv.to(torch.int32)
            classes.append(ids.cpu().numpy().astype(np.int64))
        else:
            ids, inv = np.unique(r.astype(np.int64), return_inverse=True)
            codes[l] = torch.as_tensor(inv.reshape(-1).astype(np.int32), device=dev)
            classes.append(ids.astype(np.int64))
    return codes, classes


def _resolve_pairs(names, pairs):
    """Index pairs ``(i, j)``, i <= j, from ``pairs`` (indices or names); None: every unordered pair and the diagonal."""
    L = len(names)
    if pairs is None:
        return [(i, j) for i in range(L) for j in range(i, L)]
    where = {name: l for l, name in enumerate(names)}
    out = []
    for pair in pairs:
        if len(pair) != 2:
            raise ValueError('a pair is two labellings, got %r' % (pair,))
        ij = []
        for e in pair:
            if e in where:
                ij.append(where[e])
            elif isinstance(e, (int, np.integer)) and not isinstance(e, bool) and 0 <= e < L:
                ij.append(int(e))
            else:
                raise ValueError('pair %r names a labelling that is not there: %r' % (pair, e))
        out.append((min(ij), max(ij)))
    if not out:
        raise ValueError('no pairs given')
    return out


def _check_indices(indices):
    indices = [indices] if isinstance(indices, str) else list(indices)
    for name in indices:
        if name not in INDICES:
            raise ValueError('unknown index %r: expected one of %s' % (name, ', '.join(INDICES)))
    return indices


def _check_average(average_method):
    if average_method not in AVERAGE_METHODS:
        raise ValueError('unknown average_method %r: expected one of %s' % (average_method, ', '.join(AVERAGE_METHODS)))
    return average_method


def _check_noise(noise):
    if noise not in NOISE_MODES:
        raise ValueError("noise must be 'class' or 'drop', got %r" % (noise,))
    return noise == 'drop'


# ---- device -------------------------------------------------------------------------------------------------------------------------------------------------
class PairSums(object):
    """What the device returns for one pair: ``a``, ``b`` (the marginals, int64), ``sum_squares``, ``sum_a2``, ``sum_b2``, ``n`` (Python ints), ``mi``,
    ``h_a``, ``h_b``, ``emi`` (floats as the kernels left them; ``emi`` None where it was not asked for) and ``table`` ((Ka, Kb) int64, or None)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _groups(sizes, budget):
    """Consecutive runs of pairs whose table cells sum to at most ``budget`` (a single larger pair runs alone)."""
    out, start, total = [], 0, 0
    for p, s in enumerate(sizes):
        if p > start and total + s > budget:
            out.append((start, p))
            start, total = p, 0
        total += s
    out.append((start, len(sizes)))
    return out


def device_sums(codes, n_classes, pairs, drop_codes=None, need_emi=True, return_tables=False, lf=None, timings=None):
    """The three stages for ``pairs`` (index pairs into the rows of ``codes``, an (L, N) int32 device tensor of codes in [0, n_classes[l])): a list of
    ``PairSums``.  ``drop_codes``: per labelling the code to leave out (-1: none), or None.  ``lf``: a device tensor of ``log_factorials(N)``.  ``timings``: a dict that
    receives the host-clock seconds of each stage ('tables', 'sums', 'emi'), each ending in a device synchronise (scripts/agreement_bench.py); None: no
    synchronise between the stages."""
    import time

    def lap(stage, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[stage] = timings.get(stage, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    lib = N.lib()
    dev = codes.device
    L, n_rows = codes.shape
    stream = N.stream_of(codes)
    drop_d = None if drop_codes is None else torch.as_tensor(np.asarray(drop_codes, dtype=np.int32), device=dev)
    if need_emi and lf is None:
        lf = torch.as_tensor(np.array(log_factorials(n_rows)), device=dev)          # (a copy: the cached table is read-only)
    ka = np.array([n_classes[i] for i, _ in pairs], dtype=np.int64)
    kb = np.array([n_classes[j] for _, j in pairs], dtype=np.int64)
    out = []
    for p0, p1 in _groups((ka * kb).tolist(), _CHUNK_CELLS):
        P = p1 - p0
        cells, margs, units = ka[p0:p1] * kb[p0:p1], ka[p0:p1] + kb[p0:p1], ka[p0:p1] * ((kb[p0:p1] + EMI_COLS - 1) // EMI_COLS)
        toff, moff, poff = (np.concatenate([[0], np.cumsum(v)]) for v in (cells, margs, units))
        desc = np.zeros((P, 8), dtype=np.int64)
        desc[:, 0], desc[:, 1] = [i for i, _ in pairs[p0:p1]], [j for _, j in pairs[p0:p1]]
        desc[:, 2], desc[:, 3], desc[:, 4], desc[:, 5], desc[:, 6] = ka[p0:p1], kb[p0:p1], toff[:-1], moff[:-1], poff[:-1]
        desc_d = torch.as_tensor(desc, device=dev)
        tables = torch.empty(int(toff[-1]), dtype=torch.int32, device=dev)
        marg = torch.zeros(int(moff[-1]), dtype=torch.int64, device=dev)
        isums = torch.zeros((P, 4), dtype=torch.int64, device=dev)
        fsums = torch.full((P, 3), float('nan'), dtype=torch.float64, device=dev)
        t0 = lap('setup', time.perf_counter())
        N.check(lib.dic_agreement_tables(N.ptr(codes), codes.stride(0), L, n_rows, N.ptr(drop_d), N.ptr(desc_d), P, N.ptr(tables), tables.numel(), stream),
                'dic_agreement_tables')
        t0 = lap('tables', t0)
        N.check(lib.dic_agreement_sums(N.ptr(tables), tables.numel(), N.ptr(desc_d), L, P, N.ptr(marg), marg.numel(), N.ptr(isums), N.ptr(fsums), stream),
                'dic_agreement_sums')
        t0 = lap('sums', t0)
        emi = None
        if need_emi:
            emi_d = torch.full((P,), float('nan'), dtype=torch.float64, device=dev)
            ws = torch.empty(max(16, lib.dic_agreement_workspace(int(poff[-1]))), dtype=torch.uint8, device=dev)
            N.check(lib.dic_agreement_emi(N.ptr(marg), marg.numel(), N.ptr(desc_d), L, P, int(units.max()), N.ptr(isums), N.ptr(lf), lf.numel(), N.ptr(emi_d),
                                          N.ptr(ws), ws.numel(), stream), 'dic_agreement_emi')
            lap('emi', t0)
            emi = emi_d.cpu().numpy()
        marg_h, isums_h, fsums_h = marg.cpu().numpy(), isums.cpu().numpy(), fsums.cpu().numpy()
        tables_h = tables.cpu().numpy() if return_tables else None
        for q in range(P):
            a = marg_h[moff[q]:moff[q] + ka[p0 + q]]
            b = marg_h[moff[q] + ka[p0 + q]:moff[q + 1]]
            out.append(PairSums(a=a, b=b, sum_squares=int(isums_h[q, 0]), sum_a2=int(isums_h[q, 1]), sum_b2=int(isums_h[q, 2]), n=int(isums_h[q, 3]),
                                mi=float(fsums_h[q, 0]), h_a=float(fsums_h[q, 1]), h_b=float(fsums_h[q, 2]), emi=None if emi is None else float(emi[q]),
                                table=None if tables_h is None else tables_h[toff[q]:toff[q + 1]].reshape(ka[p0 + q], kb[p0 + q]).astype(np.int64)))
    return out


# ---- host: sklearn's expressions over the device's sums -----------------------------------------------------------------------------------------------------
def _generalized_average(U, V, average_method):
    if average_method == 'min':
        return min(U, V)
    if average_method == 'geometric':
        return np.sqrt(U * V)
    if average_method == 'arithmetic':
        return np.mean([U, V])
    return max(U, V)


class PairScores(object):
    """sklearn's indices of one pair from its ``PairSums``; the class counts are those of the pair's own table (a class emptied by ``noise='drop'`` is none)."""

    def __init__(self, s):
        self.s = s
        self.n = s.n
        self.k_a, self.k_b = int(np.count_nonzero(s.a)), int(np.count_nonzero(s.b))

    def pair_confusion_matrix(self):
        n, sq = np.int64(self.s.n), np.int64(self.s.sum_squares)
        C = np.empty((2, 2), dtype=np.int64)
        C[1, 1] = sq - n
        C[0, 1] = np.int64(self.s.sum_b2) - sq
        C[1, 0] = np.int64(self.s.sum_a2) - sq
        C[0, 0] = n ** 2 - C[0, 1] - C[1, 0] - sq
        return C

    def rand(self):
        C = self.pair_confusion_matrix()
        numerator, denominator = C.diagonal().sum(), C.sum()
        if numerator == denominator or denominator == 0:
            return 1.0
        return float(numerator / denominator)

    def ari(self):
        (tn, fp), (fn, tp) = self.pair_confusion_matrix()
        tn, fp, fn, tp = int(tn), int(fp), int(fn), int(tp)          # (Python ints: tp * tn leaves int64)
        if fn == 0 and fp == 0:
            return 1.0
        return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))

    def fmi(self):
        n = np.int64(self.s.n)
        tk, pk, qk = np.int64(self.s.sum_squares) - n, np.int64(self.s.sum_b2) - n, np.int64(self.s.sum_a2) - n
        return float(np.sqrt(tk / pk) * np.sqrt(tk / qk)) if tk != 0.0 else 0.0

    def mi(self):
        if self.k_a == 1 or self.k_b == 1:
            return 0.0
        return float(np.clip(self.s.mi, 0.0, None))

    def entropies(self):
        return (0.0 if self.k_a == 1 else self.s.h_a), (0.0 if self.k_b == 1 else self.s.h_b)

    def emi(self):
        return self.s.emi

    def nmi(self, average_method='arithmetic'):
        if self.k_a == self.k_b == 1:
            return 1.0
        mi = self.mi()
        if mi == 0:
            return 0.0
        h_a, h_b = self.entropies()
        return float(mi / _generalized_average(h_a, h_b, average_method))

    def ami(self, average_method='arithmetic'):
        if self.k_a == self.k_b == 1:
            return 1.0
        if self.k_a == 1 or self.k_b == 1:
            return 0.0
        mi, emi = self.mi(), self.s.emi
        h_a, h_b = self.entropies()
        denominator = _generalized_average(h_a, h_b, average_method) - emi
        denominator = min(denominator, -_EPS) if denominator < 0 else max(denominator, _EPS)
        numerator = mi - emi
        numerator = min(numerator, -_EPS) if numerator < 0 else max(numerator, _EPS)
        return float(numerator / denominator)

    def hcv(self, beta=1.0):
        """(homogeneity, completeness, V-measure) with a as the classes and b as the clusters."""
        h_a, h_b = self.entropies()
        mi = self.mi()
        homogeneity = mi / h_a if h_a else 1.0
        completeness = mi / h_b if h_b else 1.0
        if homogeneity + completeness == 0.0:
            v = 0.0
        else:
            v = (1 + beta) * homogeneity * completeness / (beta * homogeneity + completeness)
        return float(homogeneity), float(completeness), float(v)

    def index(self, name, average_method='arithmetic'):
        if name in ('ami', 'nmi'):
            return getattr(self, name)(average_method)
        return self.hcv()[2] if name == 'vmeasure' else getattr(self, name)()


def jaccard_matching(table, classes_a, classes_b):
    """For every cluster of a: ``(cluster_a, best cluster of b, Jaccard)`` -- the cluster of b with the largest |A and B| / |A or B| (the first among equals),
    as three arrays.  Host arithmetic on the table."""
    table = np.asarray(table, dtype=np.int64)
    if table.size == 0:          # (a pair that noise='drop' left without rows)
        return np.asarray(classes_a), np.asarray(classes_b), np.zeros(0)
    a, b = table.sum(1), table.sum(0)
    union = a[:, None] + b[None, :] - table
    jac = np.where(union > 0, table / np.where(union > 0, union, 1), 0.0)
    best = jac.argmax(1)
    return np.asarray(classes_a), np.asarray(classes_b)[best], jac[np.arange(len(a)), best]


class Agreement(object):
    """The result of ``agreement_matrix``: ``names``; ``pairs`` (index pairs i < j, the off-diagonal pairs that were computed, in order); one (L, L)
    symmetric f64 matrix per requested index, as ``result[index]`` and as an attribute (NaN where a pair was not asked for); with 'vmeasure' also the
    matrices ``homogeneity`` and ``completeness``, entry [i, j] taking labelling i as the classes and j as the clusters; ``n`` (the rows counted) and
    ``n_clusters`` ((P, 2)) per entry of ``pairs``; ``values[index]`` the (P,) entries of ``pairs``.  With ``return_tables``: ``tables``, ``classes`` (per
    pair the (classes_a, classes_b) of its table) and ``matching`` (``jaccard_matching`` of the table)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getitem__(self, index):
        return self.matrices[index]

    def __getattr__(self, name):
        matrices = self.__dict__.get('matrices', {})
        if name in matrices:
            return matrices[name]
        raise AttributeError(name)


def _compact(s, classes_a, classes_b):
    """The pair's own table: rows and columns that ``noise='drop'`` emptied are no classes of it."""
    keep_a, keep_b = s.a > 0, s.b > 0
    return s.table[np.ix_(keep_a, keep_b)], classes_a[keep_a], classes_b[keep_b]


def _scores(labellings, pairs, noise, need_emi, return_tables):
    drop = _check_noise(noise)
    names, rows = _rows_of(labellings)
    index_pairs = _resolve_pairs(names, pairs)
    codes, classes = _encode(rows)
    drop_codes = [0 if drop and c[0] == NOISE else -1 for c in classes] if drop else None
    sums = device_sums(codes, [len(c) for c in classes], index_pairs, drop_codes, need_emi=need_emi, return_tables=return_tables)
    for (i, j), s in zip(index_pairs, sums):
        if s.n == 0:
            logger.info('agreement of {} and {}: no rows left without noise'.format(names[i], names[j]))
    return names, classes, index_pairs, sums


def agreement_matrix(labellings, indices=('ari', 'ami'), pairs=None, noise='class', return_tables=False, average_method='arithmetic'):
    """The ``Agreement`` of every pair of ``labellings`` (a ``{name: (N,) ints}`` dict, an (L, N) array or a device tensor; uploaded and encoded once).
    ``indices``: any of ``INDICES``.  ``pairs``: None for all L (L - 1) / 2 unordered pairs and the diagonal, or a list of ``(i, j)`` / ``(name, name)``.
    ``noise``: 'class' (-1 is a class, sklearn's behaviour) or 'drop' (per pair, the rows where either labelling says -1 are left out; a pair left with no
    rows gives NaN for every index and is logged).  Every entry has the bits of its own single-pair call."""
    indices = _check_indices(indices)
    _check_average(average_method)
    names, classes, index_pairs, sums = _scores(labellings, pairs, noise, 'ami' in indices, return_tables)
    L = len(names)
    wanted = indices + (['homogeneity', 'completeness'] if 'vmeasure' in indices else [])
    matrices = {name: np.full((L, L), np.nan) for name in wanted}
    off = [p for p, (i, j) in enumerate(index_pairs) if i != j]
    values = {name: np.full(len(off), np.nan) for name in wanted}
    slot = {p: q for q, p in enumerate(off)}
    for p, ((i, j), s) in enumerate(zip(index_pairs, sums)):
        if s.n == 0:
            continue
        sc = PairScores(s)
        got = {name: sc.index(name, average_method) for name in indices}
        for name, v in got.items():
            matrices[name][i, j] = matrices[name][j, i] = v
        if 'vmeasure' in indices:
            h, c, _ = sc.hcv()
            matrices['homogeneity'][i, j] = matrices['completeness'][j, i] = got['homogeneity'] = h
            matrices['completeness'][i, j] = matrices['homogeneity'][j, i] = got['completeness'] = c
        if p in slot:
            for name, v in got.items():
                values[name][slot[p]] = v
    res = Agreement(names=names, pairs=[index_pairs[p] for p in off], matrices=matrices, values=values, indices=indices,
                    n=np.array([sums[p].n for p in off], dtype=np.int64),
                    n_clusters=np.array([(np.count_nonzero(sums[p].a), np.count_nonzero(sums[p].b)) for p in off], dtype=np.int64).reshape(len(off), 2))
    if return_tables:
        compact = [_compact(sums[p], classes[index_pairs[p][0]], classes[index_pairs[p][1]]) for p in off]
        res.tables = [t for t, _, _ in compact]
        res.classes = [(ca, cb) for _, ca, cb in compact]
        res.matching = [jaccard_matching(t, ca, cb) for t, ca, cb in compact]
    return res


# ---- single pairs: the batch machinery with one pair ---------------------------------------------------------------------------------------------------------
def _pair(a, b, noise='class', need_emi=False, return_tables=False):
    a, b = (v if torch.is_tensor(v) else np.asarray(v) for v in (a, b))
    names, classes, _, sums = _scores({0: a, 1: b}, [(0, 1)], noise, need_emi, return_tables)
    return sums[0], classes


def _scored(a, b, noise, need_emi=False):
    s, _ = _pair(a, b, noise, need_emi)
    return None if s.n == 0 else PairScores(s)


def contingency_matrix(a, b, noise='class'):
    """``(table int64 (Ka, Kb), classes_a, classes_b)``: table[i, j] rows have class classes_a[i] in a and classes_b[j] in b."""
    s, classes = _pair(a, b, noise, return_tables=True)
    return _compact(s, classes[0], classes[1])


def pair_confusion_matrix(a, b, noise='class'):
    return PairScores(_pair(a, b, noise)[0]).pair_confusion_matrix()


def _single(name):
    def f(a, b, noise='class'):
        sc = _scored(a, b, noise)
        return float('nan') if sc is None else getattr(sc, name)()
    return f


rand_score = _single('rand')
adjusted_rand_score = _single('ari')
fowlkes_mallows_score = _single('fmi')
mutual_info_score = _single('mi')


def entropy(labels):
    """sklearn's ``entropy`` of one labelling (natural logarithm)."""
    labels = labels if torch.is_tensor(labels) else np.asarray(labels)
    sc = _scored(labels, labels, 'class')
    return sc.entropies()[0]


def expected_mutual_information(a, b, noise='class'):
    """The expected mutual information of the two labellings' marginals under the permutation model (sklearn's ``expected_mutual_information`` of their
    contingency table)."""
    sc = _scored(a, b, noise, need_emi=True)
    return float('nan') if sc is None else sc.emi()


def normalized_mutual_info_score(a, b, average_method='arithmetic', noise='class'):
    _check_average(average_method)
    sc = _scored(a, b, noise)
    return float('nan') if sc is None else sc.nmi(average_method)


def adjusted_mutual_info_score(a, b, average_method='arithmetic', noise='class'):
    _check_average(average_method)
    sc = _scored(a, b, noise, need_emi=True)
    return float('nan') if sc is None else sc.ami(average_method)


def homogeneity_completeness_v_measure(a, b, beta=1.0, noise='class'):
    if beta < 0:
        raise ValueError('beta must be >= 0, got %r' % (beta,))
    sc = _scored(a, b, noise)
    return (float('nan'),) * 3 if sc is None else sc.hcv(beta)
