#!/usr/bin/env python3
"""The sweep behind cluster_stats.ROWSUM_SAFE_RATIO, on the CPU:

    python3 scripts/validity_sweep.py          # rewrites the 'emulation' section of profiles/validity_parity.json

Three Gaussian clusters with centre spread 10 in 16 dimensions, 1 500 points, the cluster spread t going down from 1.8 to 0.0075 in steps of 10^(1/8), three
seeds, plain and shifted by 1000.  For each: the ratio the routing looks at (oracle.pairtile_emulation.geometry_ratios: smallest mean squared cluster radius /
largest mean squared distance of a cluster from the mean of all points; the centroids are far apart here) and the deviation of the emulated silhouette
(own-cluster sums replaced, and all sums replaced: the larger) from f64 in units of the silhouette's bar, rtol 1e-5 + atol 1e-6, and the largest relative
deviation of a cluster's total of own-cluster sums (the shared pass also feeds the inertias) in units of its bar, rtol 1e-5.  The crossing is the LARGEST ratio
of any run in which either reaches its bar (ROWSUM_SAFE_RATIO, for the cluster radii), or in which the silhouette does (ROWSUM_SAFE_SEPARATION, for the centroid
distances: they enter the silhouette alone);
a constant is 4 x its crossing (the factor tests/test_gpu_step_grads.py puts over an emulated floor), rounded up to two digits."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
OUT = os.path.join(ROOT, 'profiles', 'validity_parity.json')
N, D, K, CENTRE_SPREAD, MARGIN = 1500, 16, 3, 10.0, 4
STEPS, SEEDS, FIRST_STEP = 16, (0, 1, 2), -6          # cluster spreads 1.8 .. 0.0075
RTOL, ATOL = 1e-5, 1e-6


def sweep_points(step, seed, shifted):
    t = 10.0 ** (-0.5 - (step + FIRST_STEP) / 8)
    rng = np.random.default_rng([seed, step])
    lab = rng.integers(0, K, N)
    lab[:K] = np.arange(K)
    x = rng.normal(0, CENTRE_SPREAD, (K, D))[lab] + rng.normal(0, t, (N, D)) + (1000.0 if shifted else 0.0)
    return t, x.astype(np.float32), lab


def run(step, seed, shifted):
    """{cluster spread, ratio, f64 silhouette, deviation / bar} of one point of the sweep."""
    from oracle import pairtile_emulation as PE
    t, x, lab = sweep_points(step, seed, shifted)
    c = PE.compare(x, lab)
    radius, sep, far = PE.geometry_ratios(x, lab)
    s64, dev = c['f64'], max(abs(c['own'] - c['f64']), abs(c['all'] - c['f64']))
    return {'step': step, 'seed': seed, 'shifted': bool(shifted), 'cluster_spread': t, 'ratio': min(radius, sep) / far, 'silhouette_f64': s64,
            'deviation': dev, 'own_sums_deviation': c['own_sums'], 'silhouette_over_bar': dev / (RTOL * abs(s64) + ATOL), 'deviation_over_bar': max(dev / (RTOL * abs(s64) + ATOL), c['own_sums'] / RTOL)}


def constant(rows, key='deviation_over_bar'):
    """(crossing, MARGIN x crossing rounded up to two digits) of the runs in which ``key`` reaches 1."""
    crossing = max(r['ratio'] for r in rows if r[key] >= 1.0)
    digits = 10.0 ** (math.floor(math.log10(MARGIN * crossing)) - 1)
    return crossing, math.ceil(MARGIN * crossing / digits) * digits


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    rows = [run(step, seed, sh) for step in range(STEPS) for seed in SEEDS for sh in (False, True)]
    crossing, value = constant(rows)
    sil_crossing, sil_value = constant(rows, 'silhouette_over_bar')
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc['emulation'] = {'what': __doc__.split('\n\n')[2].replace('\n', ' '), 'n': N, 'd': D, 'K': K, 'centre_spread': CENTRE_SPREAD, 'rtol': RTOL, 'atol': ATOL,
                        'margin': MARGIN, 'crossing_ratio': crossing, 'ROWSUM_SAFE_RATIO': value,
                        'silhouette_crossing_ratio': sil_crossing, 'ROWSUM_SAFE_SEPARATION': sil_value, 'sweep': rows}
    json.dump(doc, open(OUT, 'w'), indent=1)
    print('crossing %.4g -> ROWSUM_SAFE_RATIO %.3g, the silhouette alone %.4g -> ROWSUM_SAFE_SEPARATION %.3g (%d runs) -> %s' % (crossing, value, sil_crossing, sil_value, len(rows), OUT))
