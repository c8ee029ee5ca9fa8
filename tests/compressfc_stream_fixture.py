"""Writes tests/golden/compressfc_stream.json: a SHA-256 of the raw bytes of every output of the four row-streaming kernels of the CompressFC node
(dic_bnhead_bwd_reduce, dic_bnhead_fwd, dic_fc_bwd / dic_fc_bwd_bnhead, dic_row_proj_stats) at the row counts where their load pipelines can go wrong.
Run it on the GPU from the root of a checkout of the commit whose bits are to be pinned, with that checkout's library built:
    python tests/compressfc_stream_fixture.py [out.json]
tests/test_gpu_compressfc_stream.py calls digests() on the current tree and compares.  Inputs come from a seeded CPU generator and are moved to the
device afterwards, so they do not depend on the machine; the grid caps below are those of the 256-CU MI355X the library is compiled for."""
import hashlib
import json
import os
import sys

import torch

K, FI = 128, 256
# bnhead kernels: 16 rows per workgroup and trip.  1..128 rows: one workgroup, 0 to 8 trips per lane; 129: two workgroups; 70 037: the reduce kernel's
# 512-workgroup cap (stride 8 192, 8 or 9 trips, a ragged end) and 548 workgroups of the forward (stride 8 768, 7 or 8 trips)
BN_ROWS = (1, 5, 16, 17, 100, 128, 129, 1000, 70037)
BN_HEADS = ((6, 1), (2, 0))                   # (C, ReLU)
BN_DROPS = (0.0, 0.2)
# fc_bwd: 32-row tiles, at most 256 workgroups.  One tile (partial, full, two); one workgroup walks two tiles; four or three tiles and a 13-row last tile
FC_ROWS = (31, 32, 33, 32 * 256 + 1, 32 * 256 * 3 + 45)
# row_proj_stats: 32-row tiles, at most 768 workgroups (a multiple of 8 once there are 8 tiles).  One tile; 21 tiles on 16 workgroups; one workgroup
# walks two tiles; four or three tiles and a 13-row last tile
RP_ROWS = (31, 32, 33, 32 * 20 + 5, 32 * 768 + 1, 32 * 768 * 3 + 45)
RNG_STATE = (0x123456789ABCDE, 7)             # (seed, call counter) of the in-kernel dropout hash


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _gen(seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return g


def _tail_params(g, c, n, dev):
    """Unit-scale z and dv, rstd > 0, and the parameters of BatchNorm1d(128) -> Linear(128, c)."""
    z = torch.randn(n, K, generator=g).to(torch.bfloat16)
    dv = torch.randn(n, c, generator=g)
    mean, rstd = torch.randn(K, generator=g) * 0.3, 0.5 + torch.rand(K, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    w2, b2 = 0.1 * torch.randn(c, K, generator=g), 0.1 * torch.randn(c, generator=g)
    return [t.to(dev) for t in (z, dv, mean, rstd, gamma, beta, w2, b2)]


def digests():
    from deep_interpolation_clustering_amd import _native as N
    L, P = N.lib(), N.ptr
    dev = torch.device('cuda', 0)
    rng = torch.tensor(RNG_STATE, dtype=torch.int64, device=dev)
    out = {}
    for c, relu in BN_HEADS:
        for n in BN_ROWS:
            z, dv, mean, rstd, gamma, beta, w2, b2 = _tail_params(_gen(1000 * c + n), c, n, dev)
            st = N.stream_of(z)
            for p in BN_DROPS:
                key = 'C%d_relu%d_p%g_N%d' % (c, relu, p, n)
                r = P(rng) if p > 0 else None
                v = torch.zeros(n, c, device=dev)
                N.check(L.dic_bnhead_fwd(P(z), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(b2), n, K, c, relu, p, r, P(v), st), 'dic_bnhead_fwd')
                out['bnhead_fwd/' + key + '/v'] = _sha(v)
                sums = torch.zeros((2 + c) * K + c, device=dev)
                ws = torch.zeros(L.dic_bnhead_bwd_workspace(n, K, c), dtype=torch.uint8, device=dev)
                N.check(L.dic_bnhead_bwd_reduce(P(z), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(dv), n, K, c, relu, p, r, P(sums), P(ws), ws.numel(), st),
                        'dic_bnhead_bwd_reduce')
                out['bnhead_bwd_reduce/' + key + '/sums'] = _sha(sums)
                out['bnhead_bwd_reduce/' + key + '/partials'] = _sha(ws)
    c = 6
    for n in FC_ROWS:
        g = _gen(50000 + n)
        z, dv, mean, rstd, gamma, beta, w2, _ = _tail_params(g, c, n, dev)
        x = (torch.randn(n, FI, generator=g)).to(torch.bfloat16).to(dev)
        w1 = (torch.randn(K, FI, generator=g) * 0.06).to(torch.bfloat16).to(dev)
        dz = torch.randn(n, K, generator=g).to(torch.bfloat16).to(dev)
        sum_da, sum_dax = (torch.randn(K, generator=g) * 0.1 * n).to(dev), (torch.randn(K, generator=g) * 0.1 * n).to(dev)
        cnt = torch.tensor([float(n)], device=dev)
        st = N.stream_of(x)
        ws = torch.zeros(L.dic_fc_bwd_workspace(n, FI, K), dtype=torch.uint8, device=dev)
        for with_dx in (True, False):
            dx = torch.zeros(n, FI, device=dev, dtype=torch.bfloat16) if with_dx else None
            dw = torch.zeros(K, FI, device=dev)
            N.check(L.dic_fc_bwd(P(dz), P(x), P(w1), n, FI, K, P(dx), P(dw), P(ws), ws.numel(), st), 'dic_fc_bwd')
            key = 'fc_bwd/N%d_dx%d' % (n, with_dx)
            if with_dx:
                out[key + '/dx'] = _sha(dx)
            out[key + '/dw'] = _sha(dw)
        for p, with_dx in ((0.0, True), (0.2, True), (0.0, False), (0.2, False)):
            dx = torch.zeros(n, FI, device=dev, dtype=torch.bfloat16) if with_dx else None
            dw = torch.zeros(K, FI, device=dev)
            N.check(L.dic_fc_bwd_bnhead(P(z), P(dv), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(sum_da), P(sum_dax), P(cnt), c, 1, p, P(rng) if p > 0 else None,
                                        P(x), P(w1), n, FI, K, P(dx), P(dw), P(ws), ws.numel(), st), 'dic_fc_bwd_bnhead')
            key = 'fc_bwd_bnhead/N%d_p%g_dx%d' % (n, p, with_dx)
            if with_dx:
                out[key + '/dx'] = _sha(dx)
            out[key + '/dw'] = _sha(dw)
    for n in RP_ROWS:
        g = _gen(90000 + n)
        x = torch.randn(n, FI, generator=g).to(torch.bfloat16).to(dev)
        w1 = (torch.randn(K, FI, generator=g) * 0.06).to(torch.bfloat16).to(dev)
        b1 = (torch.randn(K, generator=g) * 0.1).to(torch.bfloat16).to(dev)
        zo = torch.zeros(n, K, device=dev, dtype=torch.bfloat16)
        sums = torch.zeros(2 * K + 1, device=dev, dtype=torch.float64)
        ws = torch.zeros(L.dic_row_proj_stats_workspace(n, K), dtype=torch.uint8, device=dev)
        N.check(L.dic_row_proj_stats(P(x), P(w1), P(b1), n, FI, K, P(zo), P(sums), P(ws), ws.numel(), N.stream_of(x)), 'dic_row_proj_stats')
        out['row_proj_stats/N%d/z' % n] = _sha(zo)
        out['row_proj_stats/N%d/sums' % n] = _sha(sums)
    torch.cuda.synchronize()
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.getcwd())
    res = digests()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join('tests', 'golden', 'compressfc_stream.json')
    with open(path, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write('\n')
    print(len(res), 'digests ->', path)
