"""The persistent form of lstm_fwdx8 (csrc/dic_lstm32.hip: one workgroup per CU walks the 32-row tiles w, w + W, w + 2 W, ... of its direction, weights loaded
once, the x tiles of consecutive tiles staged as one sequence).  The other LSTM tests run at most a dozen tiles per direction -- one tile per workgroup --
and never enter the tile loop; the batch here gives every workgroup five or four tiles, the last of them ragged.

The kernel has no four-wave twin, so the check is slice invariance: batch rows are independent, so the full batch in one launch and the same rows in
consecutive slices of at most one tile per workgroup must give the same bits everywhere.  The whole path is held to what the commit before the persistent
form computed: tests/golden/persistent_traj.json, written by tests/persistent_traj_fixture.py on that commit."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
H, I = 128, 256


def _shapes():
    half = torch.cuda.get_device_properties(0).multi_processor_count // 2       # W: workgroups per direction
    return half, 2 * half * 64 + 70                                              # B = 16 454 on 256 CUs: 516 tiles of 32 rows, 6 live rows in tile 514, none in 515


def _run(N, L, x, wih, whh, bias, h0, c0, bm, relu_x, save):
    """One dic_lstm_fwd_xproj launch on freshly poisoned outputs (boundary rows on).  Returns out (R+2,B,2H), out_r, hn, cn, gates, cs."""
    R, B = x.shape[0], x.shape[1]
    dev, bf, P = x.device, torch.bfloat16, N.ptr
    Bp = (B + 63) // 64 * 64
    out = torch.full((R + 2, B, 2 * H), 7.0, device=dev, dtype=bf)
    out_r = torch.full((R, B, 2 * H), 7.0, device=dev, dtype=bf)
    st_shape = (B, 2, H) if bm else (2, B, H)
    hn, cn = torch.full(st_shape, 7.0, device=dev), torch.full(st_shape, 7.0, device=dev)
    gates = torch.full((R, Bp, 2, 4, H), 7.0, device=dev, dtype=bf) if save else None
    cs = torch.full((R, Bp, 2, H), 7.0, device=dev, dtype=bf) if save else None
    N.check(L.dic_lstm_fwd_xproj(P(x), P(wih), P(whh), P(bias), P(h0), P(c0), R, B, H, I, P(out[1]), P(out_r), P(hn), P(cn), P(gates), P(cs),
                                 int(bm) | 2, int(relu_x), N.stream_of(x)), 'dic_lstm_fwd_xproj')
    return out, out_r, hn, cn, gates, cs


@pytest.mark.parametrize('relu_x,init,bm,save', [(1, True, 0, True), (0, True, 1, True), (1, False, 0, True), (0, False, 1, True), (1, True, 1, False)])
@pytest.mark.parametrize('R', [1, 2, 3, 5])
def test_persistent_decoder_forward_is_invariant_under_batch_slicing(R, relu_x, init, bm, save):
    """R = 1 and R = 2 are shorter than the x pipeline is deep (a tile's x tiles are requested during the previous tile); save=False is the inference
    path without saved state."""
    from deep_interpolation_clustering_amd import _native as N
    L = N.lib()
    half, B = _shapes()
    dev, bf = torch.device('cuda'), torch.bfloat16
    torch.manual_seed(1000 * R + 10 * relu_x + init)
    x = (torch.randn(R, B, I, device=dev) * 0.5).to(bf)
    wih = (torch.randn(8 * H, I, device=dev) * 0.06).to(bf)
    whh = (torch.randn(2, 4 * H, H, device=dev) * 0.08).to(bf)
    bias = (torch.randn(8 * H, device=dev) * 0.1).to(bf)
    st_shape = (B, 2, H) if bm else (2, B, H)
    h0 = torch.randn(st_shape, device=dev) * 0.5 if init else None
    c0 = torch.randn(st_shape, device=dev) * 0.5 if init else None
    bdim = 0 if bm else 1
    out, out_r, hn, cn, gates, cs = _run(N, L, x, wih, whh, bias, h0, c0, bm, relu_x, save)
    torch.cuda.synchronize()
    nbt = 2 * ((B + 63) // 64)
    assert nbt > 4 * half                     # some workgroup walks five tiles
    if save:                                  # per (step, tile): 32 rows x 1024 gate values / 256 cell states, lane-native: (.., hh, r, j), r = row of the tile
        gv, cv = gates.view(R, nbt, -1, 32, 4), cs.view(R, nbt, -1, 32, 4)
    rows = half * 32                          # one tile per workgroup at most
    for lo in range(0, B, rows):
        hi = min(lo + rows, B)
        sl = lambda s: None if s is None else s.narrow(bdim, lo, hi - lo).contiguous()
        o, o_r, h, c, g, s = _run(N, L, x[:, lo:hi].contiguous(), wih, whh, bias, sl(h0), sl(c0), bm, relu_x, save)
        assert torch.equal(o, out[:, lo:hi]), ('out and boundary rows', lo)
        assert torch.equal(o_r, out_r[:, lo:hi]), ('out_r', lo)
        assert torch.equal(h, hn.narrow(bdim, lo, hi - lo)), ('h_n', lo)
        assert torch.equal(c, cn.narrow(bdim, lo, hi - lo)), ('c_n', lo)
        if save:
            n = hi - lo
            snbt = 2 * ((n + 63) // 64)
            g, s = g.view(R, snbt, -1, 32, 4), s.view(R, snbt, -1, 32, 4)
            for j in range((n + 31) // 32):
                live = min(32, n - 32 * j)
                assert torch.equal(g[:, j, :, :live], gv[:, lo // 32 + j, :, :live]), ('gates', lo, j)
                assert torch.equal(s[:, j, :, :live], cv[:, lo // 32 + j, :, :live]), ('cell states', lo, j)
    assert not bool((out == 7.0).all(-1).any())       # every row was written: time slots, boundary rows
    assert not bool((out_r == 7.0).all(-1).any())
    assert torch.equal(out_r, torch.relu(out[1:R + 1]))



def test_joint_step_leaves_the_parameters_the_tiled_kernels_left(golden_dir):
    """One joint bf16 step at B = 16 454, R = 24 through Stepper: loss, gradient norm and the f64 sum of all parameters after the update, exactly those of the
    commit before (the fixture was written on 256 CUs; the batch is fixed to it, so on another part this is still the same computation)."""
    spec = importlib.util.spec_from_file_location('persistent_traj_fixture', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'persistent_traj_fixture.py'))
    fx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fx)
    with open(os.path.join(golden_dir, 'persistent_traj.json')) as f:
        want = json.load(f)
    got = fx.one_step()
    print('got', got, 'want', want)
    for k in ('loss', 'gnorm', 'param_sum'):
        assert got[k] == want[k], (k, got[k], want[k])
