"""DBCV (dbcv.py, csrc/dic_dbcv.hip) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output (scripts/kmedoids_bench.py's recipe),
for a k-means K = 4 labelling (no noise, four large segments) and for one DBSCAN labelling with noise (eps = the 80th percentile of the 20th-neighbour
distance, min_samples 20).  Writes profiles/dbcv_bench.json and prints it as one JSON line.

Per labelling, host-clock seconds of one call after a warm-up on a slice, each ending in a device synchronise: ``dic_dbcv_core``, the spanning-tree walks
(one ``dic_hdbscan_mst`` per cluster, N - K launches), ``dic_dbcv_separation``, and the whole ``dbcv.dbcv`` (upload, sort, host rules and segment minima
included).  Beside each pass stands its f64 INSTRUCTION-COUNT FLOOR: a pair costs D subtractions and D fmas in f64, 2 D lane instructions, and the chip
retires CUs x 64 f64 lane instructions per clock; the core pass evaluates every ordered pair inside a segment twice (m, then S), the separation pass every
pair of a row with an INTERNAL row of another segment once (before its skip rule).  Symmetry (d(o, p) = d(p, o)) is not used: it would halve both counts.  In the same run
the DBSCAN counting pass of that eps is timed, the pass this project already makes over all pairs on the matrix cores.

Outside baseline: the numpy definition (tests/dbcv_reference.py, dense matrix) on the first ``--numpy_n`` points with their k-means labels on this host's
CPUs (0: skip), beside this package on the same points, and the difference of the two scores.

    python scripts/dbcv_bench.py [--n 75000] [--numpy_n 4000]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from deep_interpolation_clustering_amd import dbcv, dbscan, knn  # noqa: E402
from deep_interpolation_clustering_amd.kmeans import KMeans  # noqa: E402
from kmedoids_bench import latents  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


CLOCK_HZ = 2.4e9          # the MI355X's peak engine clock: 256 CUs x 64 f64 lane instructions x 2.4 GHz = the 78.6 TFLOP/s of its data sheet (an fma = 2)


def floor_seconds(pairs, d):
    """``pairs`` ordered pairs at 2 d f64 lane instructions each over CUs x 64 lanes per clock."""
    return pairs * 2.0 * d / (torch.cuda.get_device_properties(0).multi_processor_count * 64.0 * CLOCK_HZ)


def labelling(x, labels):
    n_rows, d = x.shape
    ids, sizes, order, seg_start, n_noise, n_singletons = dbcv.partition(labels)
    xs = x.index_select(0, torch.as_tensor(order, device=x.device)).contiguous()
    seg_d = torch.as_tensor(seg_start, dtype=torch.int32, device=x.device)
    rec = {'rows': n_rows, 'kept_rows': int(len(order)), 'clusters': int(len(ids)), 'largest_cluster': int(sizes.max()), 'n_noise': n_noise,
           'n_singletons': n_singletons}
    rec['core_s'], a = timed(lambda: dbcv.device_core_distances(xs, seg_d, d))
    rec['walks_s'], (reach, pred) = timed(lambda: dbcv.device_walks(xs, seg_start, a))
    reach, pred = reach.cpu().numpy(), pred.cpu().numpy().astype(np.int64)
    internal = np.zeros(len(order), dtype=bool)
    for s in range(len(ids)):
        internal[seg_start[s]:seg_start[s + 1]] = dbcv.sparseness(pred[seg_start[s]:seg_start[s + 1]], reach[seg_start[s]:seg_start[s + 1]])[1]
    internal_d = torch.as_tensor(internal.astype(np.uint8), device=x.device)
    rec['internal_rows'] = int(internal.sum())
    rec['separation_s'], _ = timed(lambda: dbcv.device_separation(xs, seg_d, a, internal_d))
    rec['whole_s'], res = timed(lambda: dbcv.dbcv(x, labels))
    inside = float((sizes.astype(np.float64) ** 2).sum())
    per_segment = np.add.reduceat(internal.astype(np.float64), seg_start[:-1])
    rec['core_pairs'], rec['separation_pairs'] = 2.0 * inside, float(len(order)) * float(internal.sum()) - float((sizes * per_segment).sum())
    rec['core_floor_s'], rec['separation_floor_s'] = floor_seconds(rec['core_pairs'], d), floor_seconds(rec['separation_pairs'], d)
    rec['core_over_floor'] = rec['core_s'] / rec['core_floor_s']
    rec['separation_over_floor'] = rec['separation_s'] / rec['separation_floor_s']
    rec['dbcv'], rec['validity'] = res.score, res.validity.tolist()
    print('%d clusters, %d noise: core %.3f s (floor %.3f s, x%.2f); walks %.3f s; separation %.3f s (floor %.3f s, x%.2f); whole %.3f s; DBCV %.4f' % (
        rec['clusters'], n_noise, rec['core_s'], rec['core_floor_s'], rec['core_over_floor'], rec['walks_s'], rec['separation_s'],
        rec['separation_floor_s'], rec['separation_over_floor'], rec['whole_s'], res.score), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--numpy_n', type=int, default=4000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dbcv_bench.json'))
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    out = {'metric': 'dbcv', 'n': n, 'd': d, 'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'clock_hz': CLOCK_HZ}
    km = KMeans(n_clusters=4, n_init=2, random_state=0).fit(X)
    km_labels = np.asarray(km.predict(X)).astype(np.int64)
    dbcv.dbcv(x[:3000], km_labels[:3000])          # warm-up: code objects, the allocator
    out['kmeans4'] = labelling(x, km_labels)

    def save():
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    save()
    eps = float(np.percentile(knn.kth_neighbor_distance(x, 20), 80))
    db_labels = dbscan.dbscan_sweep(x, [eps], 20)[0][0]
    thr = [dbscan.sq_threshold(eps)]
    dbscan._Counts(x, thr)
    out['dbscan_eps'] = eps
    out['dbscan_counts_s'], _ = timed(lambda: dbscan._Counts(x, thr))
    print('DBSCAN counting pass at eps %.4f: %.3f s' % (eps, out['dbscan_counts_s']), flush=True)
    out['dbscan'] = labelling(x, db_labels)
    save()
    if a.numpy_n:
        from dbcv_reference import reference
        m = min(a.numpy_n, n)
        t = time.perf_counter()
        ref = reference(X[:m], km_labels[:m])
        np_s = time.perf_counter() - t
        ours_s, ours = timed(lambda: dbcv.dbcv(x[:m], km_labels[:m]))
        out['numpy'] = {'n': m, 'seconds': np_s, 'cpus': len(os.sched_getaffinity(0)), 'dbcv': ref['score']}
        out['same_subset'] = {'n': m, 'seconds': ours_s, 'dbcv': ours.score, 'difference': abs(ours.score - ref['score'])}
        print('numpy definition on %d points: %.2f s; this package on the same points: %.4f s; scores %.3e apart' % (m, np_s, ours_s,
                                                                                                                   out['same_subset']['difference']), flush=True)
    save()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
