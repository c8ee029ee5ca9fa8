"""The reference of the pair-tile loop's approximate d^2 (csrc/dic_pairtile.h) and the conditions on the inputs tests/test_gpu_pairtile.py feeds it.  CPU only.

``emulate`` is the header's arithmetic with every sum and product in f64: v = fl32(x - c), h = bf16(v), l = bf16(v - h), the three bf16 pieces of an f32
norm, t_ij = sum pieces_i + sum pieces_j - 2 sum_k (h_i h_j + l_i h_j + h_i l_j).  It leaves out only the f32 rounding of the accumulation (item (3) of the
header's proof, at most 2^-13.2 (n_i + n_j) = 0.44 2^-12 (n_i + n_j)), so it must stay within the rest of the bound, items (1), (2) and (4):
(0.11 + 0.19 + 0.01) B0 = 0.31 B0; the bar here is 0.25 B0.

``drop`` removes exactly one term.  It exists to QUALIFY INPUTS: on N(0, 1) data the bf16 residuals of a lost ``lo.hi`` product cancel and the error stays
near 2 B0, which a GPU test on such data might or might not notice.  On the aligned-residual input every residual v - h has the same sign and the same
relative size (0.98 2^-8 of the value), so the lost products add up.  The tests below hold that input to: unmutated <= 0.25 B0, every mutant > 4 B0 -- which
makes "a kernel that loses a term fails the GPU bound on this input" a checked statement (4 B0 of error less 0.44 B0 of accumulation rounding is far above
the bound of 1 B0)."""
import json

import numpy as np
import pytest
import torch

PT_T = 256                      # rows of a block: nmax_J of the bound is per 256-row block
DROPS = ('lo.hi', 'hi.lo', 'norm1')


def bf16(a):
    """Round-to-nearest-even to bfloat16, returned as float64 (a: float32 array)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float64).numpy()


def d2_f64(X, Y=None, chunk_elems=1 << 24):
    """(N, M) f64: squared distances of the f32 points in f64, difference form."""
    X = np.asarray(X, dtype=np.float64)
    Y = X if Y is None else np.asarray(Y, dtype=np.float64)
    out = np.empty((len(X), len(Y)))
    step = max(1, chunk_elems // max(1, Y.shape[0] * Y.shape[1]))
    for s in range(0, len(X), step):
        diff = X[s:s + step, None, :] - Y[None, :, :]
        out[s:s + step] = np.einsum('ijk,ijk->ij', diff, diff)
    return out


def centred(X, centre):
    """v = fl32(x - c), the f32 vectors the planes are made of."""
    return np.asarray(X, dtype=np.float32) - np.asarray(centre, dtype=np.float32).reshape(1, -1)


def norm_pieces(nrm):
    """The three bf16 pieces of an f32 norm, as f64 arrays (n0, n1, n2): n0 = bf16(n), n1 = bf16(n - n0), n2 = bf16(n - n0 - n1), the differences exact in f32."""
    nrm = np.asarray(nrm, dtype=np.float32)
    n0 = bf16(nrm)
    r1 = (nrm - n0.astype(np.float32)).astype(np.float32)
    n1 = bf16(r1)
    r2 = (r1 - n1.astype(np.float32)).astype(np.float32)
    return n0, n1, bf16(r2)


def emulate(X, centre, drop=None, nrm=None):
    """(N, N) f64: the approximate d^2 of the pair-tile loop without the f32 rounding of its accumulation.  ``nrm``: the f32 norms to split (default: the f64
    sum of v^2 rounded to f32; the GPU test passes the device's own).  ``drop``: None or one of DROPS -- the term a mutant loses ('lo.hi': l_i h_j,
    'hi.lo': h_i l_j, 'norm1': the second piece of both norms)."""
    assert drop is None or drop in DROPS
    v = centred(X, centre)
    if nrm is None:
        nrm = (v.astype(np.float64) ** 2).sum(1).astype(np.float32)
    h = bf16(v)
    l = bf16((v - h.astype(np.float32)).astype(np.float32))
    n0, n1, n2 = norm_pieces(nrm)
    s = n0 + n2 + (0.0 if drop == 'norm1' else n1)
    dot = h @ h.T
    if drop != 'lo.hi':
        dot = dot + l @ h.T
    if drop != 'hi.lo':
        dot = dot + h @ l.T
    return s[:, None] + s[None, :] - 2.0 * dot


def b0(nrm, n):
    """(n, n) f64: B0_ij = 2^-12 (n_i + nmax_J), nmax_J the largest norm of j's 256-row block."""
    nrm = np.asarray(nrm, dtype=np.float64)[:n]
    nblk = (n + PT_T - 1) // PT_T
    bmax = np.array([nrm[b * PT_T:(b + 1) * PT_T].max() for b in range(nblk)])
    return 2.0 ** -12 * (nrm[:, None] + np.repeat(bmax, PT_T)[None, :n])


def aligned_residual(n, d, seed=0):
    """Points whose bf16 residuals all have one sign: every coordinate is a power of two times (1 + 0.98 2^-8), so h = the power of two and
    l = +0.98 2^-8 of it (to bf16 precision).  Centre 0."""
    rng = np.random.default_rng(seed)
    X = (rng.choice([0.5, 1.0, 2.0], (n, d)) * (1 + 0.98 * 2.0 ** -8)).astype(np.float32)
    return X, np.zeros((1, d), np.float32)


def ratio(t, d2, bound):
    return float((np.abs(t - d2) / bound).max())


def condense(lines):
    """profiles/pairtile_bound.json from the lines of one run's pairtile_bound.jsonl (tests/test_gpu_pairtile.py): per case and D the two ratios, and the
    worst of each over the run."""
    recs = [json.loads(s) for s in lines if s.strip()]
    worst = {k: max(recs, key=lambda r: r[k]) for k in ('bound_ratio', 'accumulation_ratio')}
    return {
        '_note': 'tests/test_gpu_pairtile.py on one MI355X, one run, condensed by tests/test_pairtile_host.condense.  bound_ratio = max |a - d2| / '
                 '(2^-12 (nrm_i + bmax[J])) over all i, j < N (bar: < 1); accumulation_ratio = max |a - t| / (2^-13.2 (n_i + n_j)), t the f64 emulation '
                 'of the split (bar: <= 1).',
        'worst': {k: {'value': float('%.4g' % r[k]), 'case': r['case'], 'N': r['N'], 'D': r['D']} for k, r in worst.items()},
        'cases': [{'case': r['case'], 'N': r['N'], 'D': r['D'], 'bound_ratio': float('%.4g' % r['bound_ratio']),
                   'accumulation_ratio': float('%.4g' % r['accumulation_ratio'])} for r in recs],
    }


def test_condense_keeps_the_worst_case():
    out = condense(['{"case": "a", "N": 3, "D": 8, "bound_ratio": 0.5, "accumulation_ratio": 0.01}', '',
                    '{"case": "b", "N": 4, "D": 256, "bound_ratio": 0.25, "accumulation_ratio": 0.02}'])
    assert out['worst']['bound_ratio'] == {'value': 0.5, 'case': 'a', 'N': 3, 'D': 8}
    assert out['worst']['accumulation_ratio']['case'] == 'b' and len(out['cases']) == 2


def test_bf16_split_is_what_the_header_says():
    rng = np.random.default_rng(1)
    v = (rng.normal(0, 1, 4096) * 2.0 ** rng.integers(-20, 20, 4096)).astype(np.float32)
    h = bf16(v)
    l = bf16((v - h.astype(np.float32)).astype(np.float32))
    assert np.all(np.abs(v - h) <= 2.0 ** -8 * np.abs(v))
    assert np.all(np.abs(v - h - l) <= 2.0 ** -16 * np.abs(v))
    n0, n1, n2 = norm_pieces(np.abs(v))
    assert np.all(n0 + n1 + n2 == np.abs(v).astype(np.float64))          # three pieces of 8 bits hold the 24 bits of an f32


@pytest.mark.parametrize('d', [256, 8])
def test_aligned_residual_input_qualifies(d):
    X, c = aligned_residual(300, d)
    d2 = d2_f64(X)
    nrm = (centred(X, c).astype(np.float64) ** 2).sum(1).astype(np.float32)
    bound = b0(nrm, len(X))
    r = ratio(emulate(X, c), d2, bound)
    print('D=%d: unmutated max |t - d2| / B0 = %.4f' % (d, r))
    assert r <= 0.25
    for drop in DROPS:
        rm = ratio(emulate(X, c, drop=drop), d2, bound)
        print('D=%d: without %s: %.2f' % (d, drop, rm))
        assert rm > 4.0, (drop, rm)


@pytest.mark.parametrize('d', [256, 8])
def test_gaussian_input_does_not_qualify_but_stays_inside(d):
    """The reason the aligned-residual input exists: on N(0, 1) data a lost cross product stays within a few B0 (the residuals cancel).  Only the unmutated
    bar is asserted here; the mutants' ratios are printed."""
    rng = np.random.default_rng(2)
    X = rng.normal(0, 1, (300, d)).astype(np.float32)
    c = X.mean(0, keepdims=True)
    d2 = d2_f64(X)
    nrm = (centred(X, c).astype(np.float64) ** 2).sum(1).astype(np.float32)
    bound = b0(nrm, len(X))
    r = ratio(emulate(X, c), d2, bound)
    print('D=%d: unmutated %.4f; mutants %s' % (d, r, ['%.2f' % ratio(emulate(X, c, drop=m), d2, bound) for m in DROPS]))
    assert r <= 0.25
