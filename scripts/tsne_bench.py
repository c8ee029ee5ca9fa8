"""Exact t-SNE of p2 / p4 (--embed tsne) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/kmedoids_bench.py's
recipe), perplexity 30.  Writes profiles/tsne_bench.json and prints it as one JSON line.

Host-clock figures (the best of 3 windows of ``--reps`` repetitions after a warm-up, a window ending in a device synchronise): one repulsion pass
(``dic_tsne_repulsion``: the pair kernel and the two small kernels that add Z), one step kernel (``dic_tsne_step``), the neighbour join and the construction
of P (``joint_probabilities``: ``kneighbors``, the perplexity kernel, the sort), and the whole ``--iters``-iteration fit with its final KL.

The repulsion pass is set against its own instruction-count floor, not against a threshold: the compiled pair loop issues PAIR_OPS = 15 vector instructions per
pair (2 subtractions, 2 fma for 1 + d^2, 2 conversions and the f32 reciprocal, 4 fma of the two Newton steps, the q sum, q^2 and 2 fma of the force; 63 per
four pairs with the loop's own three), N^2 pairs, 64 lanes per instruction at 16 lanes per SIMD and clock, 4 SIMDs on each of the 256 CUs at the 2.4 GHz peak
clock, every instruction counted at the full rate.  The pass visits both (i, j) and (j, i);
using the symmetry is a recorded follow-up.

For scale, sklearn's ``TSNE(method='barnes_hut')`` is timed once on the first ``--sklearn_n`` points on this host's CPUs (0: skip; skipped when sklearn is
not installed).

    python scripts/tsne_bench.py [--n 75000] [--perplexity 30] [--iters 1000] [--reps 5] [--sklearn_n 20000]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import tsne as T  # noqa: E402
from kmedoids_bench import best_of_windows, latents  # noqa: E402

PAIR_OPS = 15
LANES_PER_CLOCK = 256 * 4 * 16
PEAK_CLOCK_HZ = 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sklearn_n', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsne_bench.json'))
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    T.TSNE(perplexity=10.0, max_iter=250).fit(x[:2048])          # warm-up: code objects, the allocator
    out = {'metric': 'tsne', 'n': n, 'd': d, 'perplexity': a.perplexity, 'iters': a.iters, 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'splits': int(N.lib().dic_tsne_splits(n))}

    torch.cuda.synchronize()
    t = time.perf_counter()
    graph = T.joint_probabilities(x, a.perplexity, return_device=True)
    torch.cuda.synchronize()
    out['join_and_p_s'] = time.perf_counter() - t
    out['nnz'] = int(graph[1].numel())
    out['longest_row'] = int((graph[0][1:] - graph[0][:-1]).max())

    # a map of the size the descent works on after the exaggerated phase, not the 1e-4 start
    Y = torch.as_tensor(10.0 * torch.randn((n, 2), dtype=torch.float64, generator=torch.Generator().manual_seed(0)), device='cuda')
    run = T._Descent(graph, Y)
    out['repulsion_ms'] = 1e3 * best_of_windows(run._repulsion, a.reps)
    out['step_ms'] = 1e3 * best_of_windows(lambda: run._step(1.0, 0.8, 200.0, True, None), a.reps)
    floor = n * n * PAIR_OPS / (LANES_PER_CLOCK * PEAK_CLOCK_HZ)
    out['repulsion_floor_ms'] = 1e3 * floor
    out['repulsion_over_floor'] = out['repulsion_ms'] / out['repulsion_floor_ms']
    out['pair_ops'] = PAIR_OPS
    print('n = %d: join + P %.2f s (%d entries, longest row %d); repulsion pass %.3f ms = %.2f x its instruction floor of %.3f ms; step kernel %.3f ms'
          % (n, out['join_and_p_s'], out['nnz'], out['longest_row'], out['repulsion_ms'], out['repulsion_over_floor'], out['repulsion_floor_ms'],
             out['step_ms']), flush=True)

    torch.cuda.synchronize()
    t = time.perf_counter()
    fit = T.TSNE(perplexity=a.perplexity, max_iter=a.iters).fit(x)
    torch.cuda.synchronize()
    out['fit_s'] = time.perf_counter() - t
    out['n_iter'], out['kl'], out['learning_rate'] = fit.n_iter_, fit.kl_divergence_, fit.learning_rate_
    out['kl_history'] = fit.kl_history_
    print('fit: %d iterations in %.2f s, kl %.6f' % (fit.n_iter_, out['fit_s'], fit.kl_divergence_), flush=True)

    if a.sklearn_n:
        try:
            from sklearn.manifold import TSNE
            sub = X[:a.sklearn_n]
            t = time.perf_counter()
            sk = TSNE(method='barnes_hut', perplexity=a.perplexity, max_iter=a.iters, init='pca').fit(sub)
            out['sklearn_barnes_hut'] = {'n': len(sub), 'iters': a.iters, 'seconds': time.perf_counter() - t, 'kl': float(sk.kl_divergence_),
                                         'cpus': len(os.sched_getaffinity(0))}
            t = time.perf_counter()
            ours = T.TSNE(perplexity=a.perplexity, max_iter=a.iters).fit(x[:a.sklearn_n])
            torch.cuda.synchronize()
            out['same_subset'] = {'n': len(sub), 'seconds': time.perf_counter() - t, 'kl': ours.kl_divergence_}
            print('sklearn barnes_hut on %d points (%d threads allowed): %.1f s, kl %.4f; this package on the same points: %.2f s, kl %.4f'
                  % (len(sub), out['sklearn_barnes_hut']['cpus'], out['sklearn_barnes_hut']['seconds'], out['sklearn_barnes_hut']['kl'],
                     out['same_subset']['seconds'], out['same_subset']['kl']), flush=True)
        except ImportError:
            out['sklearn_barnes_hut'] = None
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
