#!/usr/bin/env python3
"""Records what the two Gaussian mixture front ends (gmm.py, gmm_full.py) publish, bit for bit, for the cases of
tests/test_gpu_gmm_frontend.py::test_front_ends_equal_the_recorded_bits:

    python3 scripts/record_gmm_frontend_golden.py [out.npz]

(default: tests/golden/gmm_frontend_parent.npz, recorded on one MI355X from the last commit in which each front end carried its own copy of the constructor
checks, the draws, the EM poll loop and the winner rule).  Per case of the host test files' ``CASES`` and per ``init_params``: a fit with n_init = 2 and
random_state = 3, its fitted attributes, and predict / predict_proba / score_samples / score / bic / aic on the first half of the rows, before and after
``reorder`` with the reversed permutation; then one sweep over K = 2, 3 per family.  A fit that raises is recorded as 'Class: message'.  The points are
regenerated from the host test files' seeds."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
OUT = os.path.join(ROOT, 'tests', 'golden', 'gmm_frontend_parent.npz')

# (family, case of that family's host test file): the smallest shapes that reach each path of the front ends
CASES = [
    ('gmm', 'n17_k2'),              # 17 x 12 diag
    ('gmm', 'd13'),                 # 300 x 13: padded features
    ('gmm', 'strided'),             # a view read in place
    ('gmm', 'sph_k4'),              # spherical
    ('gmm_full', 'n17_k2'),         # 17 x 4 full
    ('gmm_full', 'n257_d13_k3'),    # full, padded
    ('gmm_full', 'n255_d64_k3'),    # tied
    ('gmm_full', 'dup_k3'),         # tied, duplicated rows
]
INITS = ('kmeans', 'k-means++', 'random', 'random_from_data')
SWEEPS = [('gmm', 'd13'), ('gmm_full', 'dup_k3')]          # (the second is tied: the total scatter matrix is reused by K = 3)
ATTRS = ('weights_', 'means_', 'covariances_', 'precisions_', 'precisions_cholesky_', 'lower_bounds_', 'labels_', 'n_iter_', 'converged_', '_status')
N_INIT, SEED = 2, 3


def _family(family):
    """(the host test file's CASES, the estimator class, the sweep) of 'gmm' or 'gmm_full'."""
    if os.path.join(ROOT, 'tests') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if family == 'gmm':
        import test_gmm_host as host
        from deep_interpolation_clustering_amd.gmm import GaussianMixture as cls, gmm_sweep as sweep
    else:
        import test_gmm_full_host as host
        from deep_interpolation_clustering_amd.gmm_full import FullGaussianMixture as cls, gmm_full_sweep as sweep
    return host.CASES, cls, sweep


def device_points(X, strided):
    """The points on the device; ``strided``: as a view with a row stride of 16 floats into a buffer whose other columns hold NaN."""
    import torch
    x = torch.as_tensor(np.array(X), device='cuda')
    if not strided:
        return x
    buf = torch.full((x.shape[0], 16), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, 4:4 + x.shape[1]] = x
    return buf[:, 4:4 + x.shape[1]]


def _queries(model, half, tag):
    return {tag + 'predict': model.predict(half), tag + 'predict_proba': model.predict_proba(half), tag + 'score_samples': model.score_samples(half),
            tag + 'score': model.score(half), tag + 'bic': model.bic(half), tag + 'aic': model.aic(half)}


def _fitted(model, tag):
    return {tag + name: getattr(model, name) for name in ATTRS}


def run_case(family, case, init):
    """{name: array} of one fit; {'<tag>error': 'Class: message'} where the fit or a query raises."""
    cases, cls, _ = _family(family)
    make, K, cov = cases[case]
    x = device_points(make(), case == 'strided')
    tag = '%s/%s/%s/' % (family, case, init)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # ('did not converge' is recorded as converged_)
        try:
            model = cls(K, covariance_type=cov, n_init=N_INIT, init_params=init, random_state=SEED).fit(x)
            out.update(_fitted(model, tag))
            half = x[:x.shape[0] // 2]
            out.update(_queries(model, half, tag))
            model.reorder(np.arange(K)[::-1])
            out.update(_queries(model, half, tag + 'reordered/'))
            out[tag + 'reordered/labels_'] = model.labels_
        except Exception as e:          # noqa: BLE001 (whatever the parent raised is the expected behaviour)
            out = {tag + 'error': '%s: %s' % (type(e).__name__, e)}
    return {k: np.asarray(v) for k, v in out.items()}


def run_sweep(family, case):
    cases, _, sweep = _family(family)
    make, _, cov = cases[case]
    x = device_points(make(), False)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for K, model in sweep(x, [2, 3], covariance_type=cov, n_init=N_INIT, random_state=SEED).items():
            out.update(_fitted(model, '%s/sweep_%s/K%d/' % (family, case, K)))
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == '__main__':
    rec = {}
    for family, case in CASES:
        for init in INITS:
            rec.update(run_case(family, case, init))
    for family, case in SWEEPS:
        rec.update(run_sweep(family, case))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **rec)
    for name in sorted(rec):
        if name.endswith(('n_iter_', 'error')):
            print(name, rec[name].tolist())
    print('recorded %d arrays, %d bytes -> %s' % (len(rec), os.path.getsize(out), out))
