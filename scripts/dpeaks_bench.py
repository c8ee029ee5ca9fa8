"""Density peaks of p2 / p4 (--cluster_method densitypeaks) at full size on one MI355X: 75 000 x 256 synthetic latents shaped like p1's output
(scripts/kmedoids_bench.py's recipe), density='cutoff' with the --percent rule.

Host-clock figures (the best of 3 windows of ``--reps`` repetitions after a warm-up, a window ending in a device synchronise): ``dic_dbscan_counts`` with one
threshold (plane preparation and the host read of the band count included: it is also density peaks' own density call), ``dic_dpeaks_prepare``, the bound +
candidate passes together (``dic_dpeaks_delta`` with capacity 0 returns behind them, after reading the count), the whole ``dic_dpeaks_delta`` (the exact stage
is the difference) and ``dic_dpeaks_border``.  Device times PER KERNEL -- the bound pass, the candidate pass, the exact-stage kernels, the halo pass, and
``db_count_kernel`` of the same run for the ratio -- come from one profiled repetition of each call (torch.profiler's kernel records).  The counting pass
at d_c carries a long band list when d_c lies inside the bulk of the pair distances, so a second one at ``--eps`` (next to no band pairs) is timed too.  Candidates per row: mean
and longest.  As a CPU figure, the numpy definition of tests/test_density_peaks_host.py on ``--cpu_n`` of the points.  One JSON line at the end.

    python scripts/dpeaks_bench.py [--n 75000] [--percent 2.0] [--k 10] [--reps 5] [--eps 0.5] [--cpu_n 4000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
from torch.autograd import DeviceType
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from deep_interpolation_clustering_amd import _native as N  # noqa: E402
from deep_interpolation_clustering_amd import density_peaks as DP  # noqa: E402
from deep_interpolation_clustering_amd.dbscan import _Counts, sq_threshold  # noqa: E402
from deep_interpolation_clustering_amd.meanshift import estimate_bandwidth  # noqa: E402
from kmedoids_bench import best_of_windows, latents  # noqa: E402

KERNELS = ('db_count_kernel', 'dp_bound_kernel', 'dp_cand_kernel', 'dp_exact_kernel', 'dp_parent_kernel', 'dp_far_kernel', 'dp_finish_kernel',
           'dp_border_kernel', 'dp_band_border_kernel')


def kernel_ms(fn):
    """{kernel: device ms} of one call of ``fn``, summed per kernel name."""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        for k in KERNELS:
            if k in e.name:
                out[k] = out.get(k, 0.0) + float(getattr(e, 'device_time_total', 0.0) or 0.0) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=75000)
    ap.add_argument('--percent', type=float, default=2.0)
    ap.add_argument('--k', type=int, default=10, help='clusters of the cut whose labels the halo pass takes')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eps', type=float, default=0.5, help='eps of a second DBSCAN counting pass with next to no band pairs (scripts/kmedoids_bench.py uses it)')
    ap.add_argument('--cpu_n', type=int, default=4000, help='points of the numpy definition on the CPU (0: skip)')
    a = ap.parse_args()
    X = latents(a.n)
    x = torch.as_tensor(X, device='cuda')
    n, d = x.shape
    L, st = N.lib(), N.stream_of(x)
    DP.DensityPeaks(4, halo=True).fit(x[:2048])          # warm-up: code objects, the LDS attribute, the allocator
    out = {'metric': 'density_peaks', 'n': n, 'd': d, 'reps': a.reps, 'percent': a.percent}

    t = time.perf_counter()
    dc = estimate_bandwidth(x, quantile=a.percent / 100.0)
    out['dc'], out['dc_s'] = dc, time.perf_counter() - t
    thr = sq_threshold(dc)
    out['dbscan_counts_ms'] = 1e3 * best_of_windows(lambda: _Counts(x, [thr]), a.reps)
    light = sq_threshold(a.eps)
    out['dbscan_counts_light_ms'] = 1e3 * best_of_windows(lambda: _Counts(x, [light]), a.reps)
    out['band_pairs_light'] = _Counts(x, [light]).n_band
    cp = _Counts(x, [thr])
    rho = cp.counts[0].cpu().numpy().astype(np.int64) - 1
    order, rank = DP.density_order(rho)
    xs = x[torch.as_tensor(order, device=x.device)].contiguous()
    ws = torch.empty(int(L.dic_dpeaks_workspace(n, d)), dtype=torch.uint8, device=x.device)
    centre = xs.double().mean(dim=0).float().contiguous()

    def prepare():
        N.check(L.dic_dpeaks_prepare(N.ptr(xs), xs.stride(0), n, d, N.ptr(centre), N.ptr(ws), ws.numel(), st), 'dic_dpeaks_prepare')
    out['prepare_ms'] = 1e3 * best_of_windows(prepare, a.reps)
    delta = torch.empty(n, dtype=torch.float64, device=x.device)
    parent = torch.empty(n, dtype=torch.int32, device=x.device)
    nc, stats = C.c_int64(0), (C.c_int64 * 2)()

    def delta_call(cand, cap):
        return L.dic_dpeaks_delta(N.ptr(xs), xs.stride(0), n, d, N.ptr(cand), cap, N.ptr(delta), N.ptr(parent), C.byref(nc), stats, N.ptr(ws), ws.numel(), st)
    assert delta_call(None, 0) == -3          # the two passes and the count: nothing else runs
    cap = int(nc.value)
    cand = torch.empty((cap, 4), dtype=torch.int32, device=x.device)
    out['passes_ms'] = 1e3 * best_of_windows(lambda: delta_call(None, 0), a.reps)
    out['delta_ms'] = 1e3 * best_of_windows(lambda: N.check(delta_call(cand, cap), 'dic_dpeaks_delta'), a.reps)
    out['exact_stage_ms'] = out['delta_ms'] - out['passes_ms']
    out['candidates'], out['longest_row'], out['candidates_per_row'] = int(stats[0]), int(stats[1]), int(stats[0]) / n

    ds, ps = delta.cpu().numpy(), parent.cpu().numpy().astype(np.int64)
    dl = np.empty(n)
    dl[order] = ds
    par = np.empty(n, dtype=np.int64)
    par[order] = np.where(ps >= 0, order[np.maximum(ps, 0)], -1)
    centres = DP.select_centres(rho, dl, rank, n_clusters=a.k)
    labels = DP.propagate_labels(par, centres)
    lab = torch.as_tensor(labels.astype(np.int32), device=x.device)
    rho_d = torch.as_tensor(rho.astype(np.int32), device=x.device)
    b2 = torch.empty(a.k, dtype=torch.int32, device=x.device)

    def border():
        N.check(L.dic_dpeaks_border(n, d, thr, N.ptr(lab), N.ptr(rho_d), a.k, N.ptr(cp.band), cp.n_band, N.ptr(b2), N.ptr(cp.ws), cp.ws.numel(), st),
                'dic_dpeaks_border')
    out['border_ms'] = 1e3 * best_of_windows(border, a.reps)
    out['band_pairs'] = cp.n_band
    out['halo'] = int(DP.halo_rule(rho, labels, b2.cpu().numpy()).sum())
    out['sizes'] = np.bincount(labels, minlength=a.k).tolist()

    km = {}
    for fn in (lambda: _Counts(x, [thr]), lambda: N.check(delta_call(cand, cap), 'dic_dpeaks_delta'), border):
        km.update(kernel_ms(fn))
    out['kernel_ms'] = km
    out['db_count_kernel_light_ms'] = kernel_ms(lambda: _Counts(x, [light])).get('db_count_kernel')
    passes = ('dp_bound_kernel', 'dp_cand_kernel', 'dp_border_kernel')
    for name, base in (('over_db_count_kernel', km.get('db_count_kernel')), ('over_db_count_kernel_light', out['db_count_kernel_light_ms'])):
        if base:
            out[name] = {k: km[k] / base for k in passes if k in km}
    print('d_c = %.4g (percent %.3g): dic_dbscan_counts %.2f ms; prepare %.2f ms; bound + candidate passes %.2f ms; whole dic_dpeaks_delta %.2f ms (exact stage '
          '%.2f ms); halo pass %.2f ms (%d band pairs)' % (dc, a.percent, out['dbscan_counts_ms'], out['prepare_ms'], out['passes_ms'], out['delta_ms'],
                                                          out['exact_stage_ms'], out['border_ms'], cp.n_band), flush=True)
    print('kernels (device ms): %s; over db_count_kernel: %s' % ({k: round(v, 3) for k, v in km.items()},
                                                                 {k: round(v, 3) for k, v in out.get('over_db_count_kernel', {}).items()}), flush=True)
    print('dic_dbscan_counts at eps %.3g (%d band pairs): %.2f ms, db_count_kernel %.3f ms; the passes over it: %s'
          % (a.eps, out['band_pairs_light'], out['dbscan_counts_light_ms'], out['db_count_kernel_light_ms'] or float('nan'),
             {k: round(v, 3) for k, v in out.get('over_db_count_kernel_light', {}).items()}), flush=True)
    print('candidates: %d = %.3f per row, longest row %d; K = %d: sizes %s, halo %d' % (out['candidates'], out['candidates_per_row'], out['longest_row'], a.k,
                                                                                     out['sizes'], out['halo']), flush=True)
    if a.cpu_n:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_density_peaks_host import matrix, solve, y_density, y_halo
        sub = X[:a.cpu_n]
        t = time.perf_counter()
        D2 = matrix(sub, block=16)
        t_matrix = time.perf_counter() - t
        t = time.perf_counter()
        r = y_density(D2, 'cutoff', dc=dc)
        s = solve(D2, r, min(a.k, a.cpu_n))
        y_halo(D2, r, s['labels'], dc, min(a.k, a.cpu_n))
        t_rest = time.perf_counter() - t
        out['cpu'] = {'n': a.cpu_n, 'matrix_s': t_matrix, 'definition_s': t_rest, 'cpus': len(os.sched_getaffinity(0))}
        print('numpy definition on %d points on the CPU (%d threads allowed): matrix %.2f s, rho / delta / parent / labels / halo %.2f s'
              % (a.cpu_n, out['cpu']['cpus'], t_matrix, t_rest), flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
