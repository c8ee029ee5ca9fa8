#!/usr/bin/env python3
"""Records what dic_cluster_intra_totals and dic_cluster_pair_rowsums compute, bit for bit, for the cases of
tests/test_gpu_cluster_stats.py::test_intra_passes_equal_the_recorded_bits:

    DIC_LIB_PATH=<libdic_hip.so of the commit to record> python3 scripts/record_intra_golden.py [out.npz]

(default: tests/golden/intra_pairtile_parent.npz, recorded on one MI355X from the last commit whose dic_intra.hip carried its own copy of the tile loop).  The file
holds outputs only; the inputs are regenerated from np.random.default_rng.  Totals are kept whole (K f64 each).  Row sums S (n, K) f32 are kept as the SHA-256
of all their bytes plus every ROW_STRIDE-th row, so that a difference also says where it is."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
OUT = os.path.join(ROOT, 'tests', 'golden', 'intra_pairtile_parent.npz')

# (n, d, k).  Totals: a cluster end inside a block; clusters smaller than a block and a singleton; zero-padded width and a block of one row; 24 blocks = 300
# tiles, more than 256 workgroups (the strided assignment wraps).
TOTALS = [(700, 36, 3), (1537, 20, 64), (513, 255, 2), (5900, 8, 1)]
# Row sums: 18 row blocks x >= 18 column blocks is more than 256 tiles (contiguous ranges that split a (row block, cluster) run between two workgroups).
ROWSUMS = [(700, 36, 3), (1537, 20, 64), (4400, 8, 3)]
ROW_STRIDE = {(700, 36, 3): 1, (1537, 20, 64): 16, (4400, 8, 3): 2}


def points(n, d, k):
    """The labelling of test_intra_totals_on_the_matrix_cores_match_f64 (every label occurs; a singleton cluster when k > 3), spread 1."""
    rng = np.random.default_rng(n + d + k)
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)
    if k > 3:
        lab[lab == k - 1] = 0
        lab[k - 1] = k - 1
    x = (rng.normal(0, 1, (n, d)) + rng.normal(0, 1, (k, d))[lab]).astype(np.float32)
    return x, lab


def totals_case(cs, n, d, k):
    """{name: array} of dic_cluster_intra_totals on case (n, d, k)."""
    x, lab = points(n, d, k)
    return {'totals_%d_%d_%d' % (n, d, k): cs.intra_totals(x, lab).intra_sums().cpu().numpy()}


def rowsums_case(cs, n, d, k):
    """{name: array} of dic_cluster_pair_rowsums on case (n, d, k); the caller has set cs.ROWSUM_MIN_POINTS = 0."""
    x, lab = points(n, d, k)
    S = np.ascontiguousarray(cs.pair_stats(x, lab, need_min=False, need_max=False).S.cpu().numpy())
    assert S.dtype == np.float32 and S.shape == (n, k)
    tag = 'rowsums_%d_%d_%d' % (n, d, k)
    return {tag + '_sha256': np.frombuffer(hashlib.sha256(S.tobytes()).digest(), np.uint8), tag + '_rows': S[::ROW_STRIDE[(n, d, k)]].copy()}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from deep_interpolation_clustering_amd import _native, cluster_stats as cs
    cs.ROWSUM_MIN_POINTS = 0
    rec = {}
    for case in TOTALS:
        rec.update(totals_case(cs, *case))
    for case in ROWSUMS:
        rec.update(rowsums_case(cs, *case))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez(out, **rec)
    print('recorded %d arrays, %d bytes, from %s -> %s' % (len(rec), os.path.getsize(out), _native.LIB_PATH, out))
