#!/usr/bin/env python3
"""Records what dic_knn_kth_distance, dic_knn_neighbors and dic_knn_ranks compute and report, bit for bit, for the cases of
tests/test_gpu_knn.py::test_candidate_list_driver_equals_the_recorded_bits:

    DIC_LIB_PATH=<libdic_hip.so of the commit to record> python3 scripts/record_knn_candlist_golden.py [out.npz]

(default: tests/golden/knn_candlist_parent.npz, recorded on one MI355X from the last commit in which each of the three entry points carried its own copy of
the list protocol).  The file holds, per case, the five stats words and the SHA-256 of the output bytes, twice: at the default candidate budget and at
candidate_budget = budget_needed of that run, the smallest legal budget, which gives the most groups.  The inputs are regenerated from
np.random.default_rng."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
OUT = os.path.join(ROOT, 'tests', 'golden', 'knn_candlist_parent.npz')

# The smallest shapes at which the shared driver can go wrong.
CASES = [
    ('kth', 1537, 0, 20, 7),          # (N, -, D, k): 7 row blocks, the last one partial
    ('kth', 5, 0, 4, 5),
    ('lists', 700, 0, 36, 5),         # (N, M, D, k), M = 0: the self join
    ('lists', 600, 300, 8, 4),        # the first query row, 600, is no block boundary: the walk starts at row 512, before it
    ('lists', 256, 1, 4, 256),        # the query block starts exactly at a boundary
    ('ranks', 513, 0, 12, 9),         # (N, -, D, m): two counting passes, a last block of one row
    ('ranks', 300, 0, 8, 1),
]


def inputs(kind, n, m, d, k):
    rng = np.random.default_rng([n, m, d, k])
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    if kind == 'lists':
        return x, (rng.normal(0, 1, (m, d)).astype(np.float32) if m else None)
    if kind == 'ranks':
        t = rng.integers(-1, n, (n, k))          # absent targets (-1) among them
        t[::7, 0] = np.arange(n)[::7]            # the row itself
        t[3::11, -1] = -1
        return x, t
    return x, None


def run_case(knn, kind, n, m, d, k):
    """{name: array} of case (kind, n, m, d, k): stats (2, 5) int64 and sha256 (2, 32) uint8, row 0 at the default budget, row 1 at budget_needed."""
    x, other = inputs(kind, n, m, d, k)

    def once(budget):
        st = {}
        if kind == 'kth':
            out = (knn.kth_neighbor_distance(x, k, candidate_budget=budget, stats=st),)
        elif kind == 'lists':
            out = knn.kneighbors(x, k, Q=other, candidate_budget=budget, stats=st)
        else:
            out = (knn.neighbor_ranks(x, other, candidate_budget=budget, stats=st),)
        h = hashlib.sha256()
        for a in out:
            h.update(np.ascontiguousarray(a).tobytes())
        return [st[name] for name in knn.STAT_NAMES], np.frombuffer(h.digest(), np.uint8)

    s0, h0 = once(None)
    needed = s0[knn.STAT_NAMES.index('budget_needed')]
    assert needed > 0, (kind, n, m, d, k)
    s1, h1 = once(needed)
    tag = '%s_%d_%d_%d_%d' % (kind, n, m, d, k)
    return {tag + '_stats': np.array([s0, s1], np.int64), tag + '_sha256': np.stack([h0, h1])}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from deep_interpolation_clustering_amd import _native, knn
    rec = {}
    for case in CASES:
        rec.update(run_case(knn, *case))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez(out, **rec)
    for name in sorted(rec):
        if name.endswith('_stats'):
            print(name, rec[name].tolist())
    print('recorded %d arrays, %d bytes, from %s -> %s' % (len(rec), os.path.getsize(out), _native.LIB_PATH, out))
