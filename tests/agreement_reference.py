"""A numpy statement of the agreement definitions of include/dic_hip.h (tables by ``np.add.at``; MI, the entropies and EMI as plain sums over the same
``ln m!`` table and with the grouping the header fixes), the seeded inputs of the two agreement test files and the error bars they share.  No GPU.

THE BARS (2^-53 = u, the unit roundoff of f64; every bar is relative to the sum of the ABSOLUTE terms, which is what a sum's rounding errors scale with):
  EMI: ((8 lf[N] + 16) + n_terms) u sum|term|.  A term's exponent is nine table values of magnitude up to lf[N] added in some order: each of the 8 adds
      rounds by at most u lf[N] absolutely, which exp turns into that RELATIVE error of the term; 16 u covers the roundings of exp, the logs, the quotient
      and the products; the outer sum of n_terms terms adds at most n_terms u sum|term| whatever its order.
  MI: (nnz + 8) u sum|term| -- nnz terms in any order, 8 u for a term's own roundings.   Entropies: (K + 8) u sum|term| likewise.
  NMI / AMI / V-measure: sklearn's expression is monotone in each of MI, EMI, H(a), H(b) away from a zero denominator, so its range over the box of the four
      bars is attained at a corner: the bar is the largest |f(corner) - f(centre)| over the 16 corners plus 8 u |f| for the expression's own roundings.
"""
import functools
import itertools

import numpy as np

from deep_interpolation_clustering_amd import agreement

U = 2.0 ** -53


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------------------
def encode(labels):
    ids, inv = np.unique(np.asarray(labels).astype(np.int64), return_inverse=True)
    return ids, inv.reshape(-1)


def table_of(a, b, drop=False):
    """``(table int64 (Ka, Kb), classes_a, classes_b)`` by np.add.at; ``drop``: rows with -1 in either labelling are left out and emptied classes removed."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    if drop:
        keep = (a != -1) & (b != -1)
        a, b = a[keep], b[keep]
    ca, ia = encode(a)
    cb, ib = encode(b)
    t = np.zeros((len(ca), len(cb)), dtype=np.int64)
    np.add.at(t, (ia, ib), 1)
    return t, ca, cb


def mi_of(t):
    """``(MI, nnz, sum|term|)`` with the header's grouping, the nonzero cells of the row-major table in ascending order."""
    a, b, n = t.sum(1), t.sum(0), int(t.sum())
    logN = np.log(np.float64(n))
    total, absum, nnz = 0.0, 0.0, 0
    for i, j in zip(*np.nonzero(t)):
        v = np.float64(t[i, j])
        cnm = v / np.float64(n)
        log_outer = (-np.log(np.float64(int(a[i]) * int(b[j]))) + logN) + logN
        term = cnm * (np.log(v) - logN) + cnm * log_outer
        if abs(term) < 2.0 ** -52:
            term = 0.0
        total += term
        absum += abs(term)
        nnz += 1
    return float(total), nnz, float(absum)


def entropy_of(counts):
    """``(H, K, sum|term|)`` of the positive counts."""
    c = np.asarray(counts, dtype=np.int64)
    c = c[c > 0]
    n = np.float64(c.sum())
    terms = (c / n) * (np.log(c.astype(np.float64)) - np.log(n))
    total = 0.0
    for v in terms:
        total += v
    return float(-total), len(c), float(np.abs(terms).sum())


def emi_of(a, b, lf=None):
    """``(EMI, n_terms, sum|term|)`` of the marginals: every cell, n = max(1, a_i + b_j - N) .. min(a_i, b_j), the nine table values in the header's order."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    N = int(a.sum())
    lf = agreement.log_factorials(N) if lf is None else lf
    Nd, logN, lfN = np.float64(N), np.log(np.float64(N)), lf[N]
    total, absum, n_terms = 0.0, 0.0, 0
    cells = {}
    for ai in a[a > 0].tolist():          # (EMI depends on the marginals only: equal cells are evaluated once and added as often as they occur, in cell order)
        for bj in b[b > 0].tolist():
            key = (ai, bj)
            if key not in cells:
                n = np.arange(max(1, ai + bj - N), min(ai, bj) + 1)
                c0 = ((lf[ai] + lf[bj]) + lf[N - ai]) + lf[N - bj]
                g = (((c0 - (lf[n] + lfN)) - lf[ai - n]) - lf[bj - n]) - lf[N - ai - bj + n]
                nd = n.astype(np.float64)
                t2 = ((logN + np.log(nd)) - np.log(np.float64(ai))) - np.log(np.float64(bj))
                terms = ((nd / Nd) * t2) * np.exp(g)
                s = 0.0
                for v in terms.tolist():
                    s += v
                cells[key] = (s, len(n), float(np.abs(terms).sum()))
            s, k, ab = cells[key]
            total += s
            n_terms += k
            absum += ab
    return float(total), n_terms, float(absum)


def emi_bar(N, n_terms, absum):
    return ((8.0 * agreement.log_factorials(N)[N] + 16.0) + n_terms) * U * absum


def sum_bar(count, absum):
    return (count + 8.0) * U * absum


class Reference(object):
    """Everything the definition gives for one pair, with its bars: ``table``, ``classes``, ``sums`` (an ``agreement.PairSums``), ``scores`` (the host
    expressions of agreement.py over these sums) and ``bars`` {'mi', 'emi', 'h_a', 'h_b'}."""

    def __init__(self, a, b, drop=False):
        self.table, self.classes_a, self.classes_b = table_of(a, b, drop)
        t = self.table
        ma, mb, n = t.sum(1), t.sum(0), int(t.sum())
        self.n = n
        if n == 0:
            return
        mi, nnz, mi_abs = mi_of(t)
        ha, ka, ha_abs = entropy_of(ma)
        hb, kb, hb_abs = entropy_of(mb)
        emi, n_terms, emi_abs = emi_of(ma, mb)
        self.bars = {'mi': sum_bar(nnz, mi_abs), 'h_a': sum_bar(ka, ha_abs), 'h_b': sum_bar(kb, hb_abs), 'emi': emi_bar(n, n_terms, emi_abs)}
        self.sums = agreement.PairSums(a=ma, b=mb, sum_squares=int((t ** 2).sum()), sum_a2=int((ma ** 2).sum()), sum_b2=int((mb ** 2).sum()), n=n, mi=mi,
                                       h_a=ha, h_b=hb, emi=emi, table=t)
        self.scores = agreement.PairScores(self.sums)

    def index_bar(self, f):
        """The bar of ``f(scores)`` (an NMI / AMI / V-measure expression of a ``PairScores``): the corners of the box of the four bars."""
        s, centre = self.sums, f(self.scores)
        worst = 0.0
        for signs in itertools.product((-1.0, 1.0), repeat=4):
            moved = agreement.PairSums(**dict(s.__dict__, mi=s.mi + signs[0] * self.bars['mi'], emi=s.emi + signs[1] * self.bars['emi'],
                                              h_a=s.h_a + signs[2] * self.bars['h_a'], h_b=s.h_b + signs[3] * self.bars['h_b']))
            worst = max(worst, abs(f(agreement.PairScores(moved)) - centre))
        return worst + 8 * U * abs(centre)


@functools.lru_cache(maxsize=None)
def reference(name, drop=False):
    a, b = CASES[name]
    return Reference(a, b, drop)


# ---- the inputs, all seeded ------------------------------------------------------------------------------------------------------------------------------------
def planted(n, seed):
    """3 classes against a 60 % copy mixed with 4 random classes."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 3, n)
    return a, np.where(rng.rand(n) < 0.6, a, rng.randint(0, 4, n))


def _cases():
    rng = np.random.RandomState(7)
    cases = {'n2_identical': (np.array([0, 1]), np.array([0, 1])), 'n2_swapped': (np.array([0, 1]), np.array([1, 0])),
             'n2_constant': (np.array([0, 0]), np.array([0, 0])), 'n2_constant_split': (np.array([3, 3]), np.array([0, 1]))}
    for n in (63, 64, 65, 257, 3000):
        cases['planted_%d' % n] = planted(n, n)
    cases['singletons_300'] = (np.arange(300), rng.randint(0, 5, 300))
    big_a = np.array([0] * 900 + [1] * 100)
    big_b = np.array([0] * 850 + [1] * 150)
    flip = rng.choice(1000, 60, replace=False)
    big_b = big_b.copy()
    big_b[flip] = 1 - big_b[flip]
    cases['two_large_1000'] = (big_a, big_b)          # (a_0 + b_0 > N: the lower limit of n lies above 1)
    cases['independent_2000'] = (rng.randint(0, 6, 2000), rng.randint(0, 7, 2000))
    cases['many_3000'] = (rng.randint(0, 200, 3000), rng.randint(0, 190, 3000))          # (38 000 cells: beyond the LDS budget)
    ids = np.array([5, 9, 1000, -1])
    cases['noncontiguous_500'] = (ids[rng.randint(0, 4, 500)], ids[::-1][np.where(rng.rand(500) < 0.7, rng.randint(0, 4, 500), 2)])
    a, b = planted(800, 11)
    cases['noise_800'] = (np.where(rng.rand(800) < 0.1, -1, a), np.where(rng.rand(800) < 0.1, -1, b))
    for a, b in cases.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return cases


CASES = _cases()
SPECIAL = ('n2_identical', 'n2_swapped', 'n2_constant', 'n2_constant_split')          # (sklearn's exact returns are demanded of these)
AVERAGES = ('min', 'geometric', 'arithmetic', 'max')


# ---- the device stages on the host: what the tests without a GPU put in place of agreement._encode and agreement.device_sums ---------------------------------
def host_encode(rows):
    encoded = [encode(np.asarray(r)) for r in rows]
    return np.stack([inv.astype(np.int32) for _, inv in encoded]), [ids for ids, _ in encoded]


def host_device_sums(codes, n_classes, pairs, drop_codes=None, need_emi=True, return_tables=False, lf=None):
    out = []
    for i, j in pairs:
        a, b = codes[i].astype(np.int64), codes[j].astype(np.int64)
        keep = np.ones(len(a), dtype=bool) if drop_codes is None else (a != drop_codes[i]) & (b != drop_codes[j])
        t = np.zeros((n_classes[i], n_classes[j]), dtype=np.int64)
        np.add.at(t, (a[keep], b[keep]), 1)
        ma, mb, n = t.sum(1), t.sum(0), int(t.sum())
        mi, ha, hb, emi = (mi_of(t)[0], entropy_of(ma)[0], entropy_of(mb)[0], emi_of(ma, mb)[0] if need_emi else None) if n else (0.0, 0.0, 0.0, 0.0)
        out.append(agreement.PairSums(a=ma, b=mb, sum_squares=int((t ** 2).sum()), sum_a2=int((ma ** 2).sum()), sum_b2=int((mb ** 2).sum()), n=n, mi=mi,
                                      h_a=ha, h_b=hb, emi=emi, table=t if return_tables else None))
    return out
