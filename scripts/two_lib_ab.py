#!/usr/bin/env python3
"""Interleaved A/B of one entry point between TWO builds of libdic_hip.so in one process (boxes drift by several per cent within a run, so builds are
timed alternately, several rounds, each figure the mean of ten launches; the first `warm` alternations, while clocks and caches settle, are shown but not
counted):
DIC_AB_LIB=<second .so> python3 scripts/two_lib_ab.py {fwd_proj|fwd_xproj|bwd|dx|bnhead_reduce|bnhead_fwd|fc_bwd|rowproj_stats} [B] [rounds] [warm]
(the last four: the row streams of the CompressFC node over 24 * B rows; checksums are exact f64 sums of the outputs' magnitudes and must agree)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch  # noqa: E402

import bench  # noqa: E402
from deep_interpolation_clustering_amd import _native as N  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else 'fwd_proj'
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
warm = int(sys.argv[4]) if len(sys.argv) > 4 else 3
LA = N.lib()
LB = C.CDLL(os.path.abspath(os.environ['DIC_AB_LIB']))
for name, (res, args) in N.SIGNATURES.items():
    if hasattr(LB, name):
        fn = getattr(LB, name)
        fn.restype, fn.argtypes = res, args
R, H = 24, 128
dev, bf, P = 'cuda', torch.bfloat16, N.ptr
torch.manual_seed(0)
CFC_MODES = ('bnhead_reduce', 'bnhead_fwd', 'fc_bwd', 'rowproj_stats')      # the four row streams of the CompressFC node, rows = R * B
if what in CFC_MODES:
    rows, K, FI, Cc = R * B, 128, 256, 6
    z = torch.randn(rows, K, device=dev).to(bf)
    xin = torch.randn(rows, FI, device=dev).to(bf)
    dv = torch.randn(rows, Cc, device=dev)
    mean, rstd = torch.randn(K, device=dev) * 0.3, 0.5 + torch.rand(K, device=dev)
    gamma, beta = 1.0 + 0.2 * torch.randn(K, device=dev), 0.2 * torch.randn(K, device=dev)
    w2, b2 = 0.1 * torch.randn(Cc, K, device=dev), 0.1 * torch.randn(Cc, device=dev)
    w1, b1 = (torch.randn(K, FI, device=dev) * 0.06).to(bf), (torch.randn(K, device=dev) * 0.1).to(bf)
    st = N.stream_of(z)
    if what == 'bnhead_reduce':
        sums = torch.zeros((2 + Cc) * K + Cc, device=dev)
        ws = torch.zeros(LA.dic_bnhead_bwd_workspace(rows, K, Cc), dtype=torch.uint8, device=dev)

        def call(L):
            return lambda: N.check(L.dic_bnhead_bwd_reduce(P(z), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(dv), rows, K, Cc, 1, 0.0, None, P(sums), P(ws), ws.numel(), st), what)
        chk = lambda: (sums.double().abs().sum().item(), ws.view(torch.float32).double().abs().sum().item())
    elif what == 'bnhead_fwd':
        v = torch.zeros(rows, Cc, device=dev)

        def call(L):
            return lambda: N.check(L.dic_bnhead_fwd(P(z), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(b2), rows, K, Cc, 1, 0.0, None, P(v), st), what)
        chk = lambda: (v.double().abs().sum().item(),)
    elif what == 'fc_bwd':
        sda, sdx, cnt = torch.randn(K, device=dev) * 0.1 * rows, torch.randn(K, device=dev) * 0.1 * rows, torch.tensor([float(rows)], device=dev)
        dxo, dw = torch.zeros(rows, FI, device=dev, dtype=bf), torch.zeros(K, FI, device=dev)
        ws = torch.zeros(LA.dic_fc_bwd_workspace(rows, FI, K), dtype=torch.uint8, device=dev)

        def call(L):
            return lambda: N.check(L.dic_fc_bwd_bnhead(P(z), P(dv), P(mean), P(rstd), P(gamma), P(beta), P(w2), P(sda), P(sdx), P(cnt), Cc, 1, 0.0, None, P(xin), P(w1), rows, FI, K,
                                                       P(dxo), P(dw), P(ws), ws.numel(), st), what)
        chk = lambda: (dxo.double().abs().sum().item(), dw.double().abs().sum().item())
    else:
        zo, sums = torch.zeros(rows, K, device=dev, dtype=bf), torch.zeros(2 * K + 1, device=dev, dtype=torch.float64)
        ws = torch.zeros(LA.dic_row_proj_stats_workspace(rows, K), dtype=torch.uint8, device=dev)

        def call(L):
            return lambda: N.check(L.dic_row_proj_stats(P(xin), P(w1), P(b1), rows, FI, K, P(zo), P(sums), P(ws), ws.numel(), st), what)
        chk = lambda: (zo.double().abs().sum().item(), sums.abs().sum().item())
else:
    Bp = (B + 63) // 64 * 64
    out = torch.empty(R + 2, B, 2 * H, device=dev, dtype=bf)
    hn, cn = torch.empty(2, B, H, device=dev), torch.empty(2, B, H, device=dev)
    gates, cs = torch.empty(R, Bp, 2, 4, H, device=dev, dtype=bf), torch.empty(R + 1, Bp, 2, H, device=dev, dtype=bf)
    whh = (torch.randn(2, 4 * H, H, device=dev) * 0.08).to(bf)
    st = N.stream_of(out)
    if what == 'fwd_proj' or what == 'bwd':
        x = torch.randn(R, B, 32, device=dev).to(bf)
        wih = (torch.randn(2, 4 * H, 32, device=dev) * 0.1).to(bf)

        def call(L):
            return lambda: N.check(L.dic_lstm_fwd_proj(P(x), P(wih), P(whh), None, None, R, B, H, 32, P(out[1]), None, P(hn), P(cn), P(gates), P(cs), 0, 0, 1, st), what)
    else:
        x = (torch.randn(R, B, 256, device=dev) * 0.5).to(bf)
        wih = (torch.randn(8 * H, 256, device=dev) * 0.06).to(bf)
        bias = (torch.randn(8 * H, device=dev) * 0.1).to(bf)

        def call(L):
            return lambda: N.check(L.dic_lstm_fwd_xproj(P(x), P(wih), P(whh), P(bias), None, None, R, B, H, 256, P(out[1]), None, P(hn), P(cn), P(gates), P(cs), 0, 1, st), what)
    if what == 'dx':
        rows = R * B
        dg = (torch.randn(rows, 1024, device=dev) * 0.3).to(bf)
        wt = (torch.randn(256, 1024, device=dev) * 0.06).to(bf)
        dxo = torch.empty(rows, 256, device=dev, dtype=bf)

        def call(L):
            return lambda: N.check(L.dic_lstm_dx_tile(P(dg), P(wt), rows, 1024, 256, P(dxo), st), what)
        chk = lambda: (dxo.float().abs().sum().item(),)
    elif what == 'bwd':
        # the 64-row backward on the state a forward saved: lstm_bwd8 (dic_lstm_bwd)
        x = torch.randn(R, B, 32, device=dev).to(bf)
        wih = (torch.randn(2, 4 * H, 32, device=dev) * 0.1).to(bf)
        N.check(LA.dic_lstm_fwd_proj(P(x), P(wih), P(whh), None, None, R, B, H, 32, P(out[1]), None, P(hn), P(cn), P(gates), P(cs), 0, 0, 1, st), 'fwd')
        whh_t = whh.transpose(1, 2).contiguous()
        dout = (torch.randn(R, B, 2 * H, device=dev) * 0.1).to(bf)
        dgx = torch.empty(R, B, 2, 4, H, device=dev, dtype=bf)
        dh0, dc0, db = torch.empty(2, B, H, device=dev), torch.empty(2, B, H, device=dev), torch.empty(2, 4 * H, device=dev)
        ws = torch.empty(max(16, LA.dic_lstm_bwd_workspace(B)), dtype=torch.uint8, device=dev)

        def call(L):
            return lambda: N.check(L.dic_lstm_bwd(P(whh_t), P(gates), P(cs), None, P(dout), None, None, R, B, H, P(dgx), P(dh0), P(dc0), P(db), P(ws), ws.numel(), 0, 0, st), what)
        chk = lambda: (dgx.float().abs().sum().item(), dh0.abs().sum().item(), dc0.abs().sum().item())
    elif True:
        chk = lambda: (out[1:R + 1].float().abs().sum().item(), gates.float().abs().sum().item(), cs[:R].float().abs().sum().item())
a, b = call(LA), call(LB)
a(); sa = chk()
b(); sb = chk()
print('checksums A', sa, 'B', sb)
if what in CFC_MODES:
    assert sa == sb, 'the two libraries disagree: %r against %r' % (sa, sb)       # (these four are held bit for bit)
ta, tb = [], []
for _ in range(warm + rounds):
    ta.append(bench.time_kernel(a, 10) * 1e3)
    tb.append(bench.time_kernel(b, 10) * 1e3)
print(what, 'B = %d, warm-up alternations (not counted): A' % B, ' '.join('%.1f' % t for t in ta[:warm]), ' B', ' '.join('%.1f' % t for t in tb[:warm]))
ta, tb = ta[warm:], tb[warm:]
print(what, 'A (in-tree lib) us:', ' '.join('%.1f' % t for t in ta), ' median %.1f' % sorted(ta)[len(ta) // 2])
print(what, 'B (DIC_AB_LIB)  us:', ' '.join('%.1f' % t for t in tb), ' median %.1f' % sorted(tb)[len(tb) // 2])
print(what, 'slowest A %.1f %s fastest B %.1f' % (max(ta), '<' if max(ta) < min(tb) else '>=', min(tb)))
