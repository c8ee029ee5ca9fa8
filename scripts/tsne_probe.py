"""Why t-SNE's kernels are f64, and what a correct fit of the test data looks like: a CPU probe on the numpy definition of tests/test_tsne_host.py, on the
data of tests/test_gpu_tsne.py (600 x 16, three blobs, perplexity 30).  No GPU is used.

(1) Sensitivity of the exaggerated trajectory.  The definition is run from the test's ``init`` three times: as it is, with every gradient entry multiplied by
    1 + 1e-15 N(0, 1) (rounding-order noise: what another summation order does) and by 1 + 1e-7 N(0, 1) (what f32 pair terms would do).  Printed: the largest
    deviation from the unperturbed map relative to max|Y|, at iterations 5, 10, 20, 50, 100.  The two values at iteration 20 bracket the bound of
    test_trajectory_against_the_definition.
(2) The spread of a correct fit.  ``--runs`` runs of ``--iters`` iterations from the test's random init, each with its own 1e-15 perturbation: the final KL,
    the trustworthiness (5 neighbours) and the share of points whose five nearest map neighbours all carry the point's blob label.  Written to
    tests/golden/tsne_spread.json; test_full_fit_quality holds the GPU fit to it.  Where sklearn is installed its own exact fit is run once for scale
    (``TSNE(method='exact', init='random')``; it is NOT a bound of any test).

    python scripts/tsne_probe.py [--runs 5] [--iters 500] [--no_write]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from deep_interpolation_clustering_amd import tsne as T  # noqa: E402
from test_tsne_host import blobs, cond_p, dense_objective, descend, joint_dense, neighbour_lists, same_blob_share, trustworthiness  # noqa: E402

PERPLEXITY, EXAGGERATION, INIT_SEED = 30.0, 12.0, 0


def data():
    X, lab = blobs()
    dist, idx = neighbour_lists(X, T.n_neighbors_of(PERPLEXITY, len(X)))
    p, _, _ = cond_p(dist ** 2, PERPLEXITY)
    return X, lab, joint_dense(idx, p)


def random_init(n, seed=INIT_SEED):
    """``TSNE(init='random', random_state=seed)``'s map."""
    return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2))


def trajectories(Pd, Y0, lr, marks=(5, 10, 20, 50, 100)):
    """{iteration: (max|Y|, deviation at 1e-15, deviation at 1e-7)}: the definition stepped with the two perturbations beside the plain run."""
    states = []
    for pert, seed in ((0.0, 1), (1e-15, 1), (1e-7, 1)):
        states.append({'Y': Y0.copy(), 'U': np.zeros_like(Y0), 'G': np.ones_like(Y0), 'pert': pert, 'rng': np.random.default_rng(seed)})
    out = {}
    for it in range(max(marks)):
        for s in states:
            _, g, _, _ = dense_objective(s['Y'], Pd, EXAGGERATION)
            if s['pert']:
                g = g * (1.0 + s['pert'] * s['rng'].standard_normal(g.shape))
            s['G'] = np.maximum(np.where(s['U'] * g < 0.0, s['G'] + 0.2, s['G'] * 0.8), 0.01)
            s['U'] = 0.5 * s['U'] - lr * (g * s['G'])
            s['Y'] = s['Y'] + s['U']
        if it + 1 in marks:
            scale = np.abs(states[0]['Y']).max()
            out[it + 1] = (float(scale), float(np.abs(states[1]['Y'] - states[0]['Y']).max() / scale), float(np.abs(states[2]['Y'] - states[0]['Y']).max() / scale))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--no_write', action='store_true')
    a = ap.parse_args()
    X, lab, Pd = data()
    n = len(X)
    lr = max(n / EXAGGERATION / 4.0, 50.0)
    Y0 = random_init(n)

    out = {'n': n, 'd': int(X.shape[1]), 'perplexity': PERPLEXITY, 'iters': a.iters, 'learning_rate': lr}
    traj = trajectories(Pd, Y0, lr)
    for it, (scale, lo, hi) in traj.items():
        print('iteration %3d: max|Y| %.3e; deviation / max|Y| with 1e-15 gradient noise %.3e, with 1e-7 %.3e' % (it, scale, lo, hi), flush=True)
    out['trajectory'] = {str(it): {'scale': v[0], 'deviation_1e-15': v[1], 'deviation_1e-7': v[2]} for it, v in traj.items()}

    kls, trusts, shares = [], [], []
    for run in range(a.runs):
        t = time.perf_counter()
        Y, kl = descend(Y0, Pd, a.iters, lr, EXAGGERATION, pert=1e-15, seed=100 + run)
        kl = dense_objective(Y, Pd, 1.0)[0] if a.iters <= T.EXPLORATION_ITER else kl
        kls.append(kl)
        trusts.append(trustworthiness(X, Y, 5))
        shares.append(same_blob_share(Y, lab, 5))
        print('run %d: kl %.6f trustworthiness %.6f same-blob share %.4f (%.1f s)' % (run, kl, trusts[-1], shares[-1], time.perf_counter() - t), flush=True)
    out.update(kl=kls, trustworthiness=trusts, same_blob_share=shares, kl_spread=max(kls) - min(kls), trustworthiness_spread=max(trusts) - min(trusts))
    try:
        from sklearn.manifold import TSNE, trustworthiness as sk_trust
        fit = TSNE(method='exact', init='random', random_state=INIT_SEED, perplexity=PERPLEXITY, max_iter=max(a.iters, 250)).fit(X)
        out['sklearn_exact'] = {'kl': float(fit.kl_divergence_), 'trustworthiness': float(sk_trust(X, fit.embedding_, n_neighbors=5))}
        print('sklearn exact: kl %.6f trustworthiness %.6f' % (out['sklearn_exact']['kl'], out['sklearn_exact']['trustworthiness']), flush=True)
    except ImportError:
        pass
    if not a.no_write:
        with open(os.path.join(ROOT, 'tests', 'golden', 'tsne_spread.json'), 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
