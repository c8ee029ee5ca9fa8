"""The agreement indices (agreement.py, csrc/dic_agreement.hip) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/kmedoids_bench.py's recipe), labelled by the package's own fits -- k-means at K = 2..10 from four seeds and at K = 32 from two, DBSCAN at three
eps (noise labels), one Ward tree cut at K = 2..10, 100 and 300 (the labellings with hundreds of clusters), and the common refinement of the two K = 32
fits and one K = 10 fit.  Writes
profiles/agreement_bench.json and prints it as one JSON line.

For ALL pairs of the labellings and the diagonal: host-clock seconds of each stage (tables, sums, EMI), each ending in a device synchronise, after a
warm-up on a slice -- the best of ``--repeats`` sweeps per stage, every sweep recorded -- and of the whole ``agreement_matrix`` call with all six indices (encoding, upload and host arithmetic included).

Beside the EMI kernel stands its f64 INSTRUCTION-COUNT FLOOR.  Every term n of every cell costs the exponent g: eight f64 adds and a compare, 9 lane
instructions.  A LIVE term (g >= -746) costs an exp, a log and eight more multiplies / adds; a polynomial exp or log in f64 is at least 20 fmas with its
range reduction, so 48 more.  The chip retires CUs x 64 f64 lane instructions per clock.  The terms are counted on the host from the marginals (all pairs);
the live share is counted exactly on the sampled pairs and taken for all.

Outside baseline: sklearn.metrics.cluster on this host's CPUs over a fixed (seeded) sample of the same pairs, one call per pair and index, beside the
largest difference per index between sklearn and this package on those pairs.

    python scripts/agreement_bench.py [--n 75000] [--sample 24] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from deep_interpolation_clustering_amd import agreement, dbscan, knn, ward  # noqa: E402
from deep_interpolation_clustering_amd.kmeans import KMeans  # noqa: E402
from kmedoids_bench import latents  # noqa: E402

CLOCK_HZ = 2.4e9          # the MI355X's peak engine clock (scripts/dbcv_bench.py)
G_INSTR, LIVE_INSTR = 9, 48


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def label_set(X, x):
    lab = {}
    for seed in range(4):
        for k in range(2, 11):
            lab['kmeans%d:k%d' % (seed, k)] = np.asarray(KMeans(n_clusters=k, n_init=1, random_state=seed).fit(X).predict(X)).astype(np.int64)
    fine = [np.asarray(KMeans(n_clusters=32, n_init=1, random_state=seed).fit(X).predict(X)).astype(np.int64) for seed in (0, 1)]
    for seed, v in enumerate(fine):
        lab['kmeans%d:k32' % seed] = v
    kd = knn.kth_neighbor_distance(x, 20)
    eps = [float(np.percentile(kd, q)) for q in (50, 80, 95)]
    for e, (labels, _) in zip(eps, dbscan.dbscan_sweep(x, eps, 20)):
        lab['dbscan:eps%.4f' % e] = np.asarray(labels).astype(np.int64)
    for k, v in ward.cut_many(ward.ward_linkage(x), list(range(2, 11)) + [100, 300]).items():
        lab['ward:k%d' % k] = np.asarray(v).astype(np.int64)
    _, lab['refinement:k32xk32xk10'] = np.unique((fine[0] * 32 + fine[1]) * 10 + lab['kmeans2:k10'], return_inverse=True)
    return lab


def emi_terms(a, b, n):
    """The number of terms of the EMI sum of two marginals."""
    a, b = a[a > 0][:, None], b[b > 0][None, :]
    return int((np.minimum(a, b) - np.maximum(1, a + b - n) + 1).sum())


def live_terms(a, b, n, lf):
    """(terms, live terms) of one pair, the exponent evaluated as the kernel does."""
    terms = live = 0
    seen = {}
    for ai in a[a > 0].tolist():
        for bj in b[b > 0].tolist():
            if (ai, bj) not in seen:
                m = np.arange(max(1, ai + bj - n), min(ai, bj) + 1)
                g = (((((lf[ai] + lf[bj]) + lf[n - ai]) + lf[n - bj]) - (lf[m] + lf[n])) - lf[ai - m]) - lf[bj - m] - lf[n - ai - bj + m]
                seen[(ai, bj)] = (len(m), int((g >= -746.0).sum()))
            t, v = seen[(ai, bj)]
            terms += t
            live += v
    return terms, live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--sample', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'agreement_bench.json'))
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {'metric': 'agreement', 'n': n, 'd': d, 'device': torch.cuda.get_device_name(0), 'cus': cus, 'clock_hz': CLOCK_HZ}
    lab = label_set(X, x)
    names = list(lab)
    counts = {name: int(len(np.unique(v))) for name, v in lab.items()}
    out['labellings'], out['clusters'] = len(names), counts
    print('%d labellings, clusters %s' % (len(names), sorted(counts.values())), flush=True)

    def save():
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')

    agreement.agreement_matrix({k: v[:3000] for k, v in lab.items()}, indices=agreement.INDICES)          # warm-up: code objects, the allocator
    _, rows = agreement._rows_of(lab)
    pairs = agreement._resolve_pairs(names, None)
    out['pairs'] = len(pairs)
    out['encode_s'], (codes, classes) = timed(lambda: agreement._encode(rows))
    lf = torch.as_tensor(np.array(agreement.log_factorials(n)), device=x.device)
    runs = []
    for _ in range(a.repeats):          # every run is the whole sweep; the best of them per stage, all of them recorded
        runs.append({})
        _, sums = timed(lambda: agreement.device_sums(codes, [len(c) for c in classes], pairs, need_emi=True, lf=lf, timings=runs[-1]))
    stages = {k: min(r[k] for r in runs) for k in runs[0]}
    out['stage_runs_s'] = runs
    out.update({'%s_s' % k: v for k, v in stages.items()})
    out['whole_s'], res = timed(lambda: agreement.agreement_matrix(lab, indices=agreement.INDICES))
    out['table_cells'] = int(sum(len(classes[i]) * len(classes[j]) for i, j in pairs))
    out['emi_terms'] = int(sum(emi_terms(s.a, s.b, s.n) for s in sums))
    print('%d pairs: encode %.3f s, tables %.4f s, sums %.4f s, EMI %.4f s, whole call %.3f s' % (len(pairs), out['encode_s'], stages['tables'],
                                                                                                  stages['sums'], stages['emi'], out['whole_s']), flush=True)
    save()
    # the sample: seeded, off-diagonal, always with the pair of the two labellings of the most clusters
    rng = np.random.RandomState(0)
    off = [p for p, (i, j) in enumerate(pairs) if i != j]
    by_size = sorted(range(len(names)), key=lambda l: -len(classes[l]))
    sample = sorted(set(rng.choice(off, min(a.sample, len(off)), replace=False).tolist() + [pairs.index((min(by_size[:2]), max(by_size[:2])))]))
    from sklearn.metrics import cluster as skc
    sk = {'ari': skc.adjusted_rand_score, 'ami': skc.adjusted_mutual_info_score, 'nmi': skc.normalized_mutual_info_score, 'rand': skc.rand_score,
          'fmi': skc.fowlkes_mallows_score, 'vmeasure': skc.v_measure_score}
    sk_s = {k: 0.0 for k in sk}
    worst = {k: 0.0 for k in sk}
    terms = live = 0
    lf_h = agreement.log_factorials(n)
    for p in sample:
        i, j = pairs[p]
        for k, f in sk.items():
            t = time.perf_counter()
            want = f(lab[names[i]], lab[names[j]])
            sk_s[k] += time.perf_counter() - t
            worst[k] = max(worst[k], abs(float(res[k][i, j]) - want))
        t, v = live_terms(sums[p].a, sums[p].b, sums[p].n, lf_h)
        terms, live = terms + t, live + v
    i, j = min(by_size[:2]), max(by_size[:2])
    t = time.perf_counter()
    want = skc.adjusted_mutual_info_score(lab[names[i]], lab[names[j]])
    out['largest_pair'] = {'labellings': [names[i], names[j]], 'clusters': [len(classes[i]), len(classes[j])], 'sklearn_ami_s': time.perf_counter() - t,
                           'ami_difference': abs(float(res['ami'][i, j]) - want)}
    out['sample'] = {'pairs': len(sample), 'cpus': len(os.sched_getaffinity(0)), 'sklearn_s_per_pair': {k: v / len(sample) for k, v in sk_s.items()},
                     'sklearn_s_all_pairs_extrapolated': {k: v / len(sample) * len(off) for k, v in sk_s.items()}, 'largest_difference': worst,
                     'emi_terms': terms, 'emi_live_terms': live}
    share = live / max(terms, 1)
    out['emi_live_share'] = share
    out['emi_floor_s'] = out['emi_terms'] * (G_INSTR + share * LIVE_INSTR) / (cus * 64.0 * CLOCK_HZ)
    out['emi_over_floor'] = stages['emi'] / out['emi_floor_s']
    print('sklearn on %d pairs: %s s per pair; largest differences %s' % (len(sample), {k: round(v / len(sample), 4) for k, v in sk_s.items()},
                                                                          {k: float('%.3g' % v) for k, v in worst.items()}), flush=True)
    print('EMI: %.3g terms, %.1f %% live; floor %.5f s, kernel %.5f s (x%.1f)' % (out['emi_terms'], 100 * share, out['emi_floor_s'], stages['emi'],
                                                                                  out['emi_over_floor']), flush=True)
    save()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
