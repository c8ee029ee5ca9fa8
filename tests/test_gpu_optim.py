"""Fused clip + Adam(amsgrad) over the flat bucket (csrc/dic_optim.hip, flat_adam.py) against torch.optim.Adam +
torch.nn.utils.clip_grad_norm_ -- the tail of the reference's training step (pretrain_trainer.py:228-229, utils.py:83).

Besides the three trajectory-level tests at the top, the three C entry points (``dic_grad_norm_clip``, ``dic_adam_amsgrad_step``,
``dic_accumulate_many``) are called through ``_native`` at the sizes production runs them at and every output array is compared with the float64
restatement of the formulas in oracle/optim_oracle.py (pinned to torch's float64 optimiser by tests/test_optim_oracle.py); then the update of
the real ``Stepper`` on the real ``Net`` is checked step by step, teacher-forced (``forced_step``).

THE BARS.  u = 2^-24 is the unit roundoff of f32 (one correctly rounded operation: relative error <= u; hipcc divides and takes square roots
correctly rounded by default); a result in the subnormal range has absolute error <= 2^-150 instead, so every bar below is ``k u S + k 2^-149``.
Contraction of a multiply and an add into one fma only removes roundings.  The oracle is handed the f32 hyper-parameters the kernel receives,
widened to f64; 1 - b1 and 1 - b2 are exact in f32 (Sterbenz), so the kernel and the oracle use the same numbers.  None of the counts comes
from a GPU run.

  total       (``dic_grad_norm_clip``)  nblk = dic_grad_norm_workspace(n) / 8 workgroups of 256 threads; a thread adds L = ceil(n / (256 nblk))
              squares in one f32 fma chain of non-negative addends: L roundings, the sum of squares within L u relative.  The wave, workgroup
              and ``reduce_partials_32x8`` stages are f64 (free).  The square root halves the error, the cast to f32 adds u:
              |total / total64 - 1| <= (L/2 + 1) u.
  coef        bit for bit min(1, max_norm / (total + 1e-6f)) evaluated in f32 on the kernel's own ``total`` (torch's formula); within 3 u of the
              f64 oracle's (the cast of total, the add, the divide).  max_norm makes the clip active (half the norm), inactive (twice the
              norm) and sits exactly at the boundary: total + 1e-6f itself (coef = 1 exactly) and the next f32 below it (coef < 1).
  returned g  bit for bit float32(g) * float32(coef).
  m           g_s = fl(g c) [1]; g' = fma(wd, p, g_s) [2]; d = fl(g' - m) [3]; e = fl(d (1 - b1)) [4]; m' = fl(m + e) [5].  Every intermediate
              is at most S_m = |m| + |g c| + |wd p| in magnitude, so |m' - m64'| <= 5 u S_m.
  v, vmax     g' carries [1] and [2]: 2 u relative to |g c| + |wd p|, so 4 u on its square; a = fl((1 - b2) g') [5], fl(a g') [6],
              v' = fma(b2, v, .) [7]: |v' - v64'| <= 7 u S_v with S_v = |v| + (1 - b2)(|g c| + |wd p|)^2.  vmax' = max(vmax, v') selects: the same
              7 u S_v (|max(a, b') - max(a, b)| <= |b' - b|).  Where S_m (S_v) is zero the output must be exactly zero (its input).
  inactive    all five arrays bit-identical to their inputs.
  dp          dp = p' - p (exact in f64 from the f32 values) = s x_i, with the scalar s = (lr / (1 - b1^t)) sqrt(1 - b2^t) shared by all
              elements.  Elements where the ORACLE has sqrt(vmax') > 1e4 eps and |dp| > 64 ulp(p) enter (asserted: at most 5 % of the active
              elements are left out, by the oracle alone).  r_i = dp_gpu / dp_oracle.
    spread    |r_i / median(r) - 1| <= b_i + (the median's own share, see below), b_i = u (5 S_m / |m'| + 3.5 S_v / vmax' + 5) + ulp(p') / 2 / |dp|:
              the error of m' relative to m' itself, half the relative error of vmax' (square root), five roundings of the element's chain
              (sqrtf, / sqrt(1 - b2^t), + eps, m' / denom, * step size) and the rounding of the final subtraction p - x.
    median    |median(r) - 1| <= P u (b1^t / (1 - b1^t) + 1/2 b2^t / (1 - b2^t)) + 4 u: powf's relative error P u amplified by 1 - b^t, plus
              the subtraction 1 - b1^t, the divide, half the subtraction 1 - b2^t and sqrtf (3.5 u).  P = 2: the ROCm tree this was written
              against carries no HIP math-API accuracy table, so 2 is taken (the published table gives powf 1 ulp).
              The median of N selected elements is s (1 + e) with |e| <= median(b_i) (if a_i <= b_i for all i then median(a) <= median(b)); at
              n = 1 the median IS the element.  For N < 4096 selected elements median(b_i) is therefore added to both bars.  For N >= 4096
              nothing is added to the median's bar, which stands as stated: the elements' roundings are independent, the median's sampling
              error is of the order median(b_i) / sqrt(N), and that is left to the 1/2 u between the 3.5 u counted and the 4 u (the spread's
              bar gets that 1/2 u).
    every     The same counts in absolute form hold every active element, selected or not (on the real step the two conditions leave out
    element   97 .. 99.9 % of the bucket: most gradient elements are below 3e-3): with x = m' / denom, denom = sqrt(vmax') / sqrt(1 - b2^t) + eps,
              |dp - dp64| <= |s| (5 u S_m / denom + |x| (3.5 u S_v / vmax' + 5 u)) + |dp64| (the median's bar) + ulp(p') / 2.
  accumulate  bit for bit dst + src in f32 (one add per element).
  gnorm       (real step) the bucket holds fl(coef g): |g|_2 is recovered as |grad|_2 / coef in f64 with coef recomputed in f32 from the returned
              gnorm: the bar of ``total`` plus the u of the scaling.

Every case appends one JSON line (bars, measured values, share of elements left out, per t the median ratio against the f32-hyper oracle and
against the exact-double-hyper oracle -- the distance from the reference's double-precision bias correction, reported without a bar) to
optim_parity.jsonl beside step_grad_parity.jsonl; profiles/optim_parity.json is the last clean run condensed by
``python -m oracle.optim_oracle <jsonl> <out>``."""
import copy
import ctypes
import functools
import json
import math
import os
import weakref
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import dic_oracle as O
from oracle import optim_oracle as OO
from oracle import step_grads as S
from test_gpu_traj import DEV_LOG

pytestmark = pytest.mark.gpu


def _model(dev):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.Tanh(), torch.nn.Linear(64, 5)).to(dev)


def test_flat_adam_matches_torch_adam_and_roundtrips_state():
    from deep_interpolation_clustering_amd import dist
    from deep_interpolation_clustering_amd.flat_adam import FlatAdam
    dev = torch.device('cuda')
    m1, m2 = _model(dev), _model(dev)
    flat = dist.FlatParams(m1)
    o1 = FlatAdam(m1.parameters(), lr=3e-3, weight_decay=4e-4).bind(flat)
    o2 = torch.optim.Adam(m2.parameters(), lr=3e-3, weight_decay=4e-4, amsgrad=True)
    x = torch.randn(200, 37, device=dev)
    y = torch.randn(200, 5, device=dev)

    def run(m, o, fl, steps, scale):
        for s in range(steps):
            if fl is not None:
                fl.zero_grad()
            else:
                o.zero_grad()
            ((m(x) - y) ** 2).mean().mul(scale * (1 + s)).backward()
            if fl is not None:
                total, coef = fl.clip_coef(0.5)
                o.step(grad_scale=coef)
            else:
                total = torch.nn.utils.clip_grad_norm_(m.parameters(), 0.5)
                o.step()
        return float(total)

    t1, t2 = run(m1, o1, flat, 7, 3.0), run(m2, o2, None, 7, 3.0)       # large loss scale: the clip is active
    assert abs(t1 - t2) <= 1e-5 * abs(t2)
    for p, q in zip(m1.parameters(), m2.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
    # gradients were scaled in place, as clip_grad_norm_ leaves them
    for p, q in zip(m1.parameters(), m2.parameters()):
        np.testing.assert_allclose(p.grad.cpu().numpy(), q.grad.cpu().numpy(), rtol=2e-5, atol=1e-7)

    # state_dict compatibility in both directions, then keep training: trajectories stay together
    sd1, sd2 = copy.deepcopy(o1.state_dict()), copy.deepcopy(o2.state_dict())
    assert set(sd1['state'][0]) == set(sd2['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}
    m3, m4 = copy.deepcopy(m2), copy.deepcopy(m1)
    flat3 = dist.FlatParams(m3)
    o3 = FlatAdam(m3.parameters(), lr=3e-3, weight_decay=4e-4).bind(flat3)
    o3.load_state_dict(sd2)                                              # torch Adam -> FlatAdam
    o4 = torch.optim.Adam(m4.parameters(), lr=3e-3, weight_decay=4e-4, amsgrad=True)
    o4.load_state_dict(sd1)                                              # FlatAdam -> torch Adam
    run(m3, o3, flat3, 3, 0.01), run(m4, o4, None, 3, 0.01)              # small loss scale: clip inactive (coef = 1)
    run(m1, o1, flat, 3, 0.01), run(m2, o2, None, 3, 0.01)
    for name, a, b in (('torch->flat', m3, m2), ('flat->torch', m4, m1), ('flat vs torch', m1, m2)):
        for p, q in zip(a.parameters(), b.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=5e-5, atol=5e-6, err_msg=name)


def test_flat_adam_requires_binding():
    from deep_interpolation_clustering_amd.flat_adam import FlatAdam
    m = _model(torch.device('cuda'))
    with pytest.raises(RuntimeError):
        FlatAdam(m.parameters(), lr=1e-3).step()


def test_captured_step_follows_the_scheduler_and_cache_is_bounded():
    """the fused optimiser reads lr from device memory, so ONE captured hipGraph serves every learning rate (no
    re-capture per scheduler step), the graph cache is bounded, and a graphed trajectory with a changing lr equals the eager one."""
    from types import SimpleNamespace
    from deep_interpolation_clustering_amd import synthetic
    from deep_interpolation_clustering_amd.clustering_interp import Net
    from deep_interpolation_clustering_amd.step import Stepper
    from deep_interpolation_clustering_amd.utils import pytorch_optimizer
    args = SimpleNamespace(num_variables=6, num_timestamps=96, ref_points=24, hours_from_admission=24, dropout=0.0, aux_tasks={},
                           fake_detection=False, triple_margin=0.0, cluster_number=4, loss='ae_mse_kl', grad_clip=15.0,
                           unsup_aux_tasks={'fake_detection': 1., 'triplet': 1., 'kl': 10.})
    dev = torch.device('cuda')
    coh = synthetic.make_cohort(384, seed=8)
    x_np, ob_np, n = synthetic.stacked_batch(coh)
    X, OB, LEN = torch.tensor(x_np, device=dev), torch.tensor(ob_np, device=dev), torch.tensor(n, device=dev)
    traj = {}
    for graphs in (False, True):
        torch.manual_seed(4)
        net = Net(args, dev).to(dev)
        net.train()
        st = Stepper(net, lambda m: pytorch_optimizer(m, 'Adam', 3e-3, 4e-4), args, autocast_dtype=torch.bfloat16, use_graphs=graphs)
        out = []
        for i in range(6):
            st.optimizer.param_groups[0]['lr'] = 3e-3 * (0.5 ** i)             # a scheduler step before every batch
            losses, gnorm, _ = st.step(X[:256], OB[:256], None, LEN[:256])
            out.append([float(losses['loss'].detach()), float(gnorm)])
        if graphs:
            assert len(st._graphs) == 1                                          # lr is not part of the graph key
            for b in (64, 96, 128, 160):                                         # four more shapes: the cache stays bounded
                st.step(X[:b], OB[:b], None, LEN[:b])
            assert len(st._graphs) <= st.MAX_GRAPHS
        traj[graphs] = np.array(out)
    np.testing.assert_allclose(traj[True], traj[False], rtol=2e-3)


# ================================================================================================ kernels against the f64 oracle
LOG = os.path.join(os.path.dirname(DEV_LOG), 'optim_parity.jsonl')          # beside step_grad_parity.jsonl and traj_deviation.jsonl
U = 2.0 ** -24                      # unit roundoff of f32
TINY = 2.0 ** -149                  # twice the absolute error of one rounding into the subnormal range
POWF_P = 2                          # powf's bound in units of u: no accuracy table in the ROCm tree, see the module docstring
K_M, K_V, K_CHAIN = 5, 7, 5         # rounding counts of m', of v' / vmax', of an element's chain after them (module docstring)
MEDIAN_FREE_N = 4096
SIZES = [1, 255, 256, 257, 1023, 1025, 131072, 131073, 524288, 524289, 'bucket', 2 ** 24 + 3]
ADAM_GRID_CAP = 8 * 256 * 256       # elements one pass of the Adam kernel's grid covers; beyond it the grid-stride loop runs
T_STEPS = OO.T_STEPS
LR, B1, B2, EPS, adam_inputs = OO.LR, OO.B1, OO.B2, OO.EPS, OO.adam_inputs          # (shared with tests/test_optim_oracle.py)
DIC_ERR_INVALID_ARG, DIC_ERR_WORKSPACE = -1, -3


def f32(x):
    return float(np.float32(x))


def _append(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, 'a') as f:
            f.write(json.dumps(rec) + '\n')
    except OSError:
        pass


def _worst(outputs, name, got, bar):
    """Keep, per output, the (measured, bar) pair nearest to or furthest over its bar."""
    got, bar = float(got), float(bar)
    over = lambda g, b: (g / b if b > 0 else (0.0 if g == 0 else math.inf))          # noqa: E731
    if name not in outputs or over(got, bar) > over(*outputs[name]):
        outputs[name] = [got, bar]


def _misses(outputs):
    return [(k, g, b) for k, (g, b) in outputs.items() if not g <= b]


CFG_ARGS = dict(C=6, R=24, H=24.0, K=4)


def net_args(shape, T, loss, grad_clip, fake_detection=False):
    return SimpleNamespace(num_variables=shape['C'], num_timestamps=T, ref_points=shape['R'], hours_from_admission=shape['H'], dropout=0.0,
                           aux_tasks={}, fake_detection=fake_detection, triple_margin=0.0, cluster_number=shape['K'], loss=loss,
                           grad_clip=grad_clip, unsup_aux_tasks={'fake_detection': 1., 'triplet': 1., 'kl': 10.}, aux_pos_weights={})


@functools.lru_cache(maxsize=None)
def bucket_size():
    """Elements of the flat bucket of the real Net at the configured shape, K = 4."""
    from deep_interpolation_clustering_amd.clustering_interp import Net
    net = Net(net_args(CFG_ARGS, 96, 'ae_mse_kl', 15.0), torch.device('cuda'))
    n = sum(p.numel() for p in net.parameters() if p.requires_grad)
    assert n > ADAM_GRID_CAP          # production runs the Adam kernel's grid-stride loop and a 512-partial norm
    return n


def size_of(n):
    return bucket_size() if n == 'bucket' else n


def norm_blocks(n):
    """(workgroups, squares per thread's f32 chain) of dic_grad_norm_clip at n elements, from the library's own workspace size."""
    from deep_interpolation_clustering_amd import _native as N
    nblk = N.lib().dic_grad_norm_workspace(n) // 8
    return nblk, -(-n // (256 * nblk))


def coef_f32(total32, max_norm):
    """torch's clip coefficient evaluated in f32: clamp(max_norm / (total + 1e-6), max=1.0) (a NaN stays a NaN)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.float32(max_norm) / (np.float32(total32) + np.float32(1e-6))
    return q if (np.isnan(q) or q < np.float32(1.0)) else np.float32(1.0)


def run_norm(g_dev, max_norm, ws=None, ws_bytes=None):
    from deep_interpolation_clustering_amd import _native as N
    L = N.lib()
    n = g_dev.numel()
    need = L.dic_grad_norm_workspace(n)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=g_dev.device) if ws is None else ws
    out2 = torch.full((2,), -7.0, device=g_dev.device)
    rc = L.dic_grad_norm_clip(N.ptr(g_dev), n, f32(max_norm), N.ptr(out2), N.ptr(ws), need if ws_bytes is None else ws_bytes, N.stream_of(g_dev))
    torch.cuda.synchronize()
    t, c = out2.cpu().numpy()
    return rc, t, c


def norm_gradients(n, rng):
    blocks = np.arange(n) // 256
    gauss = rng.standard_normal(n).astype(np.float32)
    last = np.zeros(n, np.float32)
    last[-1] = 3.7
    return {'gauss': gauss, 'spread1e6': (gauss * 10.0 ** (-3.0 + 6.0 * blocks / max(1, blocks[-1]))).astype(np.float32),
            'zero': np.zeros(n, np.float32), 'last': last}


@pytest.mark.parametrize('n', SIZES, ids=str)
def test_grad_norm_clip_kernel_against_f64(n):
    """``total`` within (L/2 + 1) u of the f64 norm, ``coef`` bit for bit torch's formula in f32 on that total and within 3 u of the oracle's,
    for Gaussian gradients, a 1e6 spread of magnitudes across workgroups, all zeros (total 0, coef 1) and one non-zero element at the last
    index; the clip active, inactive and exactly at its boundary."""
    n = size_of(n)
    dev = torch.device('cuda')
    nblk, L = norm_blocks(n)
    bar_total = (L / 2 + 1) * U
    outputs = {}
    for kind, g in norm_gradients(n, np.random.default_rng(n % 9973)).items():
        g_dev = torch.from_numpy(g).to(dev)
        total64 = OO.grad_norm_clip(g, 1.0)[0]
        if kind == 'zero':
            rc, t, c = run_norm(g_dev, 15.0)
            assert rc == 0 and t == 0.0 and c == 1.0
            continue
        rc, t0, _ = run_norm(g_dev, 15.0)
        assert rc == 0
        edge = np.float32(t0) + np.float32(1e-6)                        # max_norm / (total + 1e-6f) == 1 exactly
        for what, mn in (('active', 0.5 * total64), ('inactive', 2.0 * total64), ('edge', edge), ('below-edge', np.nextafter(edge, np.float32(0)))):
            rc, t, c = run_norm(g_dev, mn)
            assert rc == 0 and t == t0                                  # (fixed order: the same bits on every launch)
            _worst(outputs, 'total', abs(float(t) / total64 - 1), bar_total)
            want = coef_f32(t, f32(mn))
            assert c == want, (kind, what, float(c), float(want))
            _worst(outputs, 'coef', abs(float(c) / OO.grad_norm_clip(g, f32(mn))[1] - 1), 3 * U)
            assert {'active': c < 1, 'inactive': c == 1, 'edge': c == 1, 'below-edge': c < 1}[what], (kind, what, float(c))
    print(f'[optim] grad_norm_clip n={n} nblk={nblk} L={L}: {outputs}')
    _append({'test': 'grad_norm_clip', 'case': f'n={n}', 'nblk': nblk, 'L': L, 'outputs': outputs})
    assert not _misses(outputs), _misses(outputs)


def test_grad_norm_clip_rejects_a_short_workspace():
    from deep_interpolation_clustering_amd import _native as N
    for n in (1, 131073):
        g = torch.ones(n, device='cuda')
        need = N.lib().dic_grad_norm_workspace(n)
        assert need == 8 * norm_blocks(n)[0] and need >= 8
        ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
        rc, t, c = run_norm(g, 1.0, ws=ws, ws_bytes=need - 1)
        assert rc == DIC_ERR_WORKSPACE and t == -7.0 and c == -7.0 and not bool(ws.any())          # nothing was launched
        assert run_norm(g, 1.0, ws=ws, ws_bytes=need)[0] == 0


# ------------------------------------------------------------------------------------------------ Adam
def switching_mask(n):
    """Active bytes that switch at indices which are multiples of neither 256 nor 64."""
    i = np.arange(n)
    on = ((i // 37) % 3 != 1) & ~((i > 1000) & (i < 1531)) & ~((i >= 300007) & (i < 524301))
    assert n < 64 or (on.any() and not on.all())
    return on.astype(np.uint8)


def adam_figures(outputs, pre, g_in, coef, active, t, hyper32, got, hyper_exact, returned_g=True, cap=0.05, min_selected=0, full=None):
    """Every output of one Adam step against the oracle, per the module docstring: fills ``outputs`` (name -> [measured, bar]; where the bar is
    per element the measured value is max(error / bar) against 1) and returns (share of active elements left out, the median of dp_gpu /
    dp_oracle against the f32-hyper oracle, the same against the exact-double-hyper oracle); (0, None, None) without an active element.
    ``pre`` = (p, m, v, vmax) and ``g_in`` as the kernel received them, ``got`` = (p, g, m, v, vmax) as it left them, all f32 arrays.
    ``min_selected``: the least number of elements the dp ratio must be taken over (the real step, where the 5 % cap cannot be asked).
    ``full`` = ``oracle_pair(...)`` of the same step without a mask, when the caller shares it between masks (the mask is then applied here:
    inactive elements keep their inputs)."""
    p, m, v, vm = pre
    lr, b1, b2, eps, wd = (float(x) for x in hyper32)
    on = np.ones(p.size, bool) if active is None else np.asarray(active) != 0
    full = oracle_pair(pre, g_in, coef, t, hyper32, hyper_exact) if full is None else full
    o_p, o_g, o_m, o_v, o_vm = (np.where(on, new, old) for new, old in zip(full[0], (p, g_in, m, v, vm)))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)          # noqa: E731
    for name, new, old in zip(('p', 'g', 'm', 'v', 'vmax'), got, (p, g_in, m, v, vm)):
        assert new.dtype == np.float32 and old.dtype == np.float32
        _worst(outputs, f'inactive {name} bits changed', int((bits(new)[~on] != bits(old)[~on]).sum()), 0)
    if not on.any():
        return 0.0, None, None
    c32 = np.float32(1.0 if coef is None else coef)
    if returned_g:
        _worst(outputs, 'g bits off float32(g) * float32(coef)', int((bits(got[1])[on] != bits(g_in * c32)[on]).sum()), 0)
    p64, gs, wdp = p.astype(np.float64), np.abs(g_in.astype(np.float64) * float(c32)), np.abs(wd * p.astype(np.float64))
    s_m = np.abs(m.astype(np.float64)) + gs + wdp
    s_v = np.abs(v.astype(np.float64)) + (1.0 - b2) * (gs + wdp) ** 2
    for name, new, want, k, s in (('m', got[2], o_m, K_M, s_m), ('v', got[3], o_v, K_V, s_v), ('vmax', got[4], o_vm, K_V, s_v)):
        err = np.abs(new.astype(np.float64) - want)[on] / (k * (U * s[on] + TINY))          # (s = 0: the output must be exactly its input)
        _worst(outputs, f'{name}: max |got - f64| / ({k} u S + {k} 2^-149)', err.max(), 1.0)
    dp_g, dp_o = got[0].astype(np.float64) - p64, o_p - p64
    dead = on & (s_m == 0) & (wd == 0)
    _worst(outputs, 'p bits changed where g = m = v = vmax = 0 and wd = 0', int((bits(got[0])[dead] != bits(p)[dead]).sum()), 0)
    # every active element, no selection: |dp - dp64| <= |s| (K_M u S_m / denom + |x| (K_V/2 u S_v / vmax' + K_CHAIN u)) + |dp64| (median's bar) + ulp(p') / 2
    pw1, pw2 = b1 ** t, b2 ** t
    scalar_bar = POWF_P * U * (pw1 / (1 - pw1) + 0.5 * pw2 / (1 - pw2)) + 4 * U
    s_size, bc2s = OO.bias_corrections(t, lr, b1, b2)
    denom = np.sqrt(o_vm) / bc2s + eps
    with np.errstate(invalid='ignore', divide='ignore'):
        v_rel = np.where(s_v > 0, 0.5 * K_V * U * s_v / o_vm, 0.0)
    bound = (s_size * (K_M * (U * s_m + TINY) / denom + np.abs(o_m) / denom * (v_rel + K_CHAIN * U)) + np.abs(dp_o) * scalar_bar
             + 0.5 * np.spacing(np.abs(got[0])).astype(np.float64))
    _worst(outputs, 'dp on every active element: max |dp - dp64| / bound', (np.abs(dp_g - dp_o)[on] / bound[on]).max(), 1.0)
    sel = on & (np.sqrt(o_vm) > 1e4 * eps) & (np.abs(dp_o) > 64 * np.spacing(np.abs(p)).astype(np.float64))
    left_out = 1.0 - sel.sum() / on.sum()
    _worst(outputs, 'share of active elements left out of the dp ratio', left_out, cap)
    if min_selected:
        _worst(outputs, f'dp ratio taken over too few elements: {min_selected} / selected', min_selected / max(1, int(sel.sum())), 1.0)
    if not sel.any():
        return left_out, None, None
    r = dp_g[sel] / dp_o[sel]
    med = float(np.median(r))
    b = (U * (K_M * s_m[sel] / np.abs(o_m[sel]) + 0.5 * K_V * s_v[sel] / o_vm[sel] + K_CHAIN)
         + 0.5 * np.spacing(np.abs(got[0][sel])).astype(np.float64) / np.abs(dp_o[sel]))
    med_own = float(np.median(b)) if r.size < MEDIAN_FREE_N else 0.0
    _worst(outputs, 'dp spread: max |r_i / median - 1| / b_i', (np.abs(r / med - 1) / (b + (med_own if med_own else 0.5 * U))).max(), 1.0)
    _worst(outputs, 'dp median: |median(r) - 1|', abs(med - 1), scalar_bar + med_own)
    return left_out, med, float(np.median(dp_g[sel] / (full[1] - p64)[sel]))


def oracle_pair(pre, g_in, coef, t, hyper32, hyper_exact):
    """(the five oracle outputs with the f32 hyper-parameters the kernel receives, the oracle's p' with the exact doubles) of one step
    without a mask: the costly part of a case, shared by the masks of the same (t, wd, coef)."""
    p, m, v, vm = pre
    return (OO.adam_amsgrad_step(p, g_in, m, v, vm, t, *(float(x) for x in hyper32), coef=coef),
            OO.adam_amsgrad_step(p, g_in, m, v, vm, t, *hyper_exact, coef=coef)[0])


def run_adam(arrs, t, hyper32, coef, active, hyper_on_device, dev):
    """One launch of dic_adam_amsgrad_step on copies of ``arrs`` = (p, g, m, v, vmax); returns the five arrays as it left them."""
    from deep_interpolation_clustering_amd import _native as N
    d = [torch.from_numpy(a).to(dev) for a in arrs]
    step = torch.full((1,), float(t), device=dev)
    cf = None if coef is None else torch.full((1,), f32(coef), device=dev)
    act = None if active is None else torch.from_numpy(active).to(dev)
    hy = torch.tensor(hyper32, dtype=torch.float32, device=dev) if hyper_on_device else None
    sc = [0.0] * 5 if hyper_on_device else [float(x) for x in hyper32]          # (with `hyper` the scalar arguments must not matter)
    rc = N.lib().dic_adam_amsgrad_step(*[N.ptr(a) for a in d], d[0].numel(), *sc, N.ptr(step), N.ptr(cf), N.ptr(act), N.ptr(hy), N.stream_of(d[0]))
    torch.cuda.synchronize()
    assert rc == 0
    return [a.cpu().numpy() for a in d]


MASK_KINDS = ('none', 'ones', 'switch', 'zeros')


def adam_combos(n):
    """[(t, wd, coef, mask kinds)].  Up to the real bucket's size -- through the grid cap, so the grid-stride loop and the large masks are in --
    the full product t x wd x coef x mask (the oracle is evaluated once per (t, wd, coef) and shared by the four masks).  Only at 2^24 + 3,
    where one oracle evaluation costs seconds, nine rows in which every t, both wd, the three coef and the four masks occur."""
    if n <= bucket_size():
        return [(t, wd, c, MASK_KINDS) for t in T_STEPS for wd in (0.0, 4e-4) for c in (None, 1.0, 0.37)]
    return [(1, 0.0, None, ('none',)), (2, 4e-4, 0.37, ('switch',)), (10, 4e-4, 1.0, ('ones',)), (1000, 0.0, 0.37, ('zeros',)),
            (100000, 4e-4, None, ('switch',)), (1, 4e-4, 0.37, ('none',)), (100000, 0.0, 1.0, ('switch',)), (10, 0.0, 0.37, ('ones',)),
            (1000, 4e-4, 0.37, ('switch',))]


@pytest.mark.parametrize('n', SIZES, ids=str)
def test_adam_amsgrad_kernel_against_f64(n):
    """Every output array of ``dic_adam_amsgrad_step`` against the oracle at the bars of the module docstring, over t, weight decay, the clip
    coefficient (none / 1 / 0.37), the byte mask (none / all ones / switching off the 64- and 256-boundaries / all zeros), with the
    hyper-parameters as scalars and in device memory -- the two must give the same bits."""
    n = size_of(n)
    dev = torch.device('cuda')
    p, g, m, v, vm, _ = adam_inputs(n, np.random.default_rng(1000 + n % 9973))
    masks = {'none': None, 'ones': np.ones(n, np.uint8), 'switch': switching_mask(n) if n >= 64 else np.ones(n, np.uint8), 'zeros': np.zeros(n, np.uint8)}
    outputs, ratios, worst_left = {}, {}, 0.0
    for t, wd, coef, kinds in adam_combos(n):
        hyper32, exact = [f32(x) for x in (LR, B1, B2, EPS, wd)], (LR, B1, B2, EPS, wd)
        c32 = None if coef is None else f32(coef)
        full = oracle_pair((p, m, v, vm), g, c32, t, hyper32, exact)
        for kind in kinds:
            got = run_adam((p, g, m, v, vm), t, hyper32, coef, masks[kind], True, dev)
            plain = run_adam((p, g, m, v, vm), t, hyper32, coef, masks[kind], False, dev)
            _worst(outputs, 'arrays that differ between hyper in device memory and as scalars',
                   sum(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, plain)), 0)
            left, r32, r64 = adam_figures(outputs, (p, m, v, vm), g, c32, masks[kind], t, hyper32, got, exact, full=full)
            worst_left = max(worst_left, left)
            if r32 is not None:
                cur = ratios.setdefault(str(t), [r32, r64])
                ratios[str(t)] = [max(cur[0], r32, key=lambda x: abs(x - 1)), max(cur[1], r64, key=lambda x: abs(x - 1))]
    print(f'[optim] adam n={n}: {outputs}\n[optim] adam n={n}: median dp ratio per t (f32 hyper, exact double hyper): {ratios}')
    _append({'test': 'adam_amsgrad_step', 'case': f'n={n}', 'outputs': outputs, 'left_out': worst_left, 'scalar_ratio': ratios})
    assert not _misses(outputs), _misses(outputs)


# ------------------------------------------------------------------------------------------------ accumulate_many
ACC_LENGTHS = [200000, 1, 255, 131073, 257, 2049, 70001, 16385, 3, 129025, 64, 199999, 1023, 4097, 31, 150000, 2]


def _accumulate(srcs, dsts, ns, count=None, null_table=False):
    from deep_interpolation_clustering_amd import _native as N
    n = (ctypes.c_int * max(1, len(ns)))(*ns)
    rc = N.lib().dic_accumulate_many(None if null_table else N.ptr_array(srcs), None if null_table else N.ptr_array(dsts), n,
                                     len(ns) if count is None else count, N.stream_of(dsts[0]) if dsts else None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('count', [0, 1, 16, 17, 33])
def test_accumulate_many_adds_every_entry_in_f32(count):
    """dst += src for ``count`` entries of 1 .. 200 000 elements (beyond kAccumMax = 16 entries per launch and beyond the 64 x 256-thread column
    cap): bit for bit the f32 sum, destinations non-zero beforehand, and not one element past an entry's length touched."""
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(count)
    ns = [ACC_LENGTHS[j % len(ACC_LENGTHS)] for j in range(count)]
    PAD = 67
    srcs = [torch.randn(k + PAD, generator=gen) for k in ns]
    dsts = [torch.randn(k + PAD, generator=gen) + 3.0 for k in ns]
    s_dev, d_dev = [t.to(dev) for t in srcs], [t.to(dev) for t in dsts]
    assert _accumulate(s_dev, d_dev, ns) == 0
    wrong = 0
    for k, s, d, got in zip(ns, srcs, dsts, d_dev):
        want = d.clone()
        want[:k] += s[:k]
        wrong += int((got.cpu().view(torch.int32) != want.view(torch.int32)).sum())
    _append({'test': 'accumulate_many', 'case': f'count={count}', 'outputs': {'elements off the f32 sum': [wrong, 0]}})
    assert wrong == 0


def test_accumulate_many_rejects_an_empty_entry_and_a_null_table():
    dev = torch.device('cuda')
    s, d = [torch.ones(8, device=dev) for _ in range(18)], [torch.full((8,), 2.0, device=dev) for _ in range(18)]
    assert _accumulate(s, d, [8] * 17 + [0]) == DIC_ERR_INVALID_ARG              # (the empty entry sits in the second batch of 16)
    assert _accumulate(s[:2], d[:2], [8, 0]) == DIC_ERR_INVALID_ARG
    assert all(bool((t == 2.0).all()) for t in d)                                # a rejected call has added nothing, not even its first batch
    assert _accumulate([], d[:1], [8], count=1, null_table=True) == DIC_ERR_INVALID_ARG
    assert _accumulate(s[:1], d[:1], [8], count=-1) == DIC_ERR_INVALID_ARG


# ================================================================================================ the update of the real step
def real_case(B, fake=False, wide=False):
    """Pretrained weights + k-means centres at the configured shape (``wide``: the configs[3] shape) with a synthetic batch: the state the
    step-gradient cases build (tests/test_gpu_step_grads.synthetic_case)."""
    from test_gpu_step_grads import synthetic_case
    return synthetic_case(B, fake=fake, wide=wide)


def make_stepper(case, mode, loss, grad_clip, use_graphs=False, lr=LR, wd=4e-4, load_state=True):
    from deep_interpolation_clustering_amd.clustering_interp import Net
    from deep_interpolation_clustering_amd.step import Stepper
    from deep_interpolation_clustering_amd.utils import pytorch_optimizer
    dev = torch.device('cuda')
    args = net_args(case['shape'], case['x'].shape[-1], loss, grad_clip, fake_detection=case['fake'] is not None)
    net = Net(args, dev).to(dev)
    if load_state:
        net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in case['state'].items()}, strict=True)
    net.train()
    return Stepper(net, lambda m: pytorch_optimizer(m, 'Adam', lr, wd), args, autocast_dtype=torch.bfloat16 if mode == 'bf16' else None,
                   precision=None if mode == 'bf16' else mode, use_graphs=use_graphs)


def batch_call(st, case, rows, **extra):
    """() -> st.step(...) on the encounters ``rows`` of the case (prefix lengths; the fake-detection inputs when the net has that head)."""
    dev, C = torch.device('cuda'), case['shape']['C']
    x = torch.tensor(case['x'][rows], device=dev)
    mask = x[:, C:2 * C].contiguous()
    ob, lengths = torch.tensor(case['ob'][rows], device=dev), mask.sum(-1).to(torch.int32)
    kw = dict(extra)
    if case['fake'] is not None:
        B = x.shape[0]
        kw.update(fake_x=torch.tensor(case['fake']['fake_x'][rows], device=dev), fake_perm_idx=torch.randperm(2 * B, generator=torch.Generator().manual_seed(B)).to(dev))
    return lambda: st.step(x, ob, mask, lengths, **kw)


def oracle_unreached(case, kl_weight):
    """Names of the parameters the backward of ae_mse (+ kl_weight * kl) does not reach, from the f64 OracleNet (``grad is None``) -- the GPU is
    not asked."""
    sh, fake = case['shape'], case['fake']
    net = O.OracleNet(sh['C'], sh['R'], sh['H'], sh['K'], 0.0, fake_detection=fake is not None)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in case['state'].items()}, strict=True)
    net = net.double().train()
    x = torch.as_tensor(case['x'][:8]).double()
    kw = {}
    if fake is not None:
        kw = dict(fake_x=torch.as_tensor(fake['fake_x'][:8]).double(), fake_perm_idx=torch.randperm(16, generator=torch.Generator().manual_seed(8)))
    terms, _, _, _ = O.joint_loss(net, x, torch.as_tensor(case['ob'][:8]).double(), x[:, sh['C']:2 * sh['C']], kl_weight, **kw)
    terms['loss'].backward()
    return [k for k, p in net.named_parameters() if p.grad is None]


def mask_of(st, unreached):
    """Per-element active bytes of the flat bucket for the parameter names ``unreached`` (None when empty)."""
    if not unreached:
        return None
    names = {id(p): k for k, p in st.model.named_parameters()}
    assert set(unreached) <= set(names.values())
    return np.concatenate([np.full(p.numel(), 0 if names[id(p)] in unreached else 1, np.uint8) for p in st.flat.params])


def state_arrays(st):
    o = st.optimizer
    return [a.detach().cpu().numpy().copy() for a in (st.flat.flat, o._m, o._v, o._vmax)]


def forced_step(st, call, outputs, ratios, unreached=()):
    """One teacher-forced step: clone parameters and optimiser state, run ``call`` (a ``Stepper.step``), read the returned gnorm, the bucket's
    gradient (now coef * g) and the state back, and hold (a) gnorm to the f64 norm of grad / coef with coef recomputed in f32 from gnorm,
    (b) every Adam output to the oracle applied to the cloned pre-state and the read-back gradient, at the kernel-level bars.  The share of
    elements the two dp conditions leave out is recorded, not capped: the gradients are the network's, not chosen (a bias that feeds a
    BatchNorm has a gradient of rounding noise; at t = 1 sqrt(vmax') > 1e4 eps asks |g| > 3e-3), and m', v', vmax' and the inactive bits are
    held on every element regardless; the ratio must still be taken over at least 256 elements on every step, so that the spread and the median
    cannot pass empty.  Returns (the step's coef, the state arrays after the step)."""
    opt = st.optimizer
    pre, t0 = state_arrays(st), float(opt._step)
    _, gnorm, _ = call()
    torch.cuda.synchronize()
    t = t0 + 1
    assert float(opt._step) == t
    grp = opt.param_groups[0]
    exact = (grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'], grp['weight_decay'])
    hyper32 = opt._hyper.cpu().numpy()
    assert np.array_equal(hyper32, np.array(exact, np.float32))          # what the kernel read is what the scheduler set
    post, grad = state_arrays(st), st.flat.grad.cpu().numpy().copy()
    gn = np.float32(float(gnorm))
    coef = coef_f32(gn, st.args.grad_clip)
    nblk, L = norm_blocks(grad.size)
    g64 = grad.astype(np.float64)
    _worst(outputs, 'gnorm: |gnorm / (|grad|_2 / coef) - 1|', abs(float(gn) / (math.sqrt(float(g64 @ g64)) / float(coef)) - 1), (L / 2 + 1) * U + U)
    left, r32, r64 = adam_figures(outputs, pre, grad, None, mask_of(st, unreached), t, hyper32, [post[0], grad] + post[1:], exact, returned_g=False, cap=1.0, min_selected=256)
    if r32 is not None:
        ratios.setdefault(str(int(t)), [r32, r64])
    return float(coef), post


def finish(test, case, outputs, ratios, **extra):
    print(f'[optim] {test} {case}: {outputs}\n[optim] {test} {case}: median dp ratio per t (f32 hyper, exact double hyper): {ratios}')
    left = outputs.get('share of active elements left out of the dp ratio', [0.0])[0]
    _append(dict({'test': test, 'case': case, 'outputs': outputs, 'left_out': left, 'scalar_ratio': ratios}, **extra))
    assert not _misses(outputs), _misses(outputs)


@functools.lru_cache(maxsize=None)
def oracle_gnorm(B):
    """f64 gradient norm of the first step of ``real_case(B)`` (oracle/step_grads.py, CPU)."""
    c = real_case(B)
    return S.reference_grads(c['state'], c['x'], c['ob'], arithmetic='f64', **c['shape'])[1]['gnorm']


@pytest.mark.parametrize('clip', ['reference-15', 'half-the-f64-norm'])
@pytest.mark.parametrize('mode', ['exact', 'bf16'])
def test_eager_step_update_is_the_oracles(mode, clip):
    """Six eager steps of the real Net (pretrained state, 64 encounters), teacher-forced: grad_clip = 15 as the reference sets it (inactive here)
    and half the f64 oracle's gradient norm of the first step (certainly active there); the lr halved before every step, weight_decay
    changed once mid-run."""
    B = 64
    case = real_case(B)
    grad_clip = 15.0 if clip == 'reference-15' else 0.5 * oracle_gnorm(B)
    st = make_stepper(case, mode, 'ae_mse_kl', grad_clip)
    outputs, ratios, coefs = {}, {}, []
    for i in range(6):
        st.optimizer.param_groups[0]['lr'] = LR * 0.5 ** i
        if i == 3:
            st.optimizer.param_groups[0]['weight_decay'] = 1e-4
        coefs.append(forced_step(st, batch_call(st, case, slice(0, B)), outputs, ratios)[0])
    assert (coefs[0] < 1.0) == (clip != 'reference-15'), coefs
    finish('eager_step', f'{mode} clip={clip}', outputs, ratios, coefs=coefs, grad_clip=grad_clip)


def test_eager_step_update_is_the_oracles_at_the_wide_shape():
    """The same at the configs[3] shape (C = 12, T = 288, K = 16), three steps in bf16."""
    case = real_case(32, wide=True)
    st = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0)
    outputs, ratios = {}, {}
    for i in range(3):
        st.optimizer.param_groups[0]['lr'] = LR * 0.5 ** i
        forced_step(st, batch_call(st, case, slice(0, 32)), outputs, ratios)
    finish('eager_step', 'wide bf16 clip=reference-15', outputs, ratios)


def test_graphed_first_call_and_replays_update_like_the_oracle():
    """use_graphs=True at B = 256.  The very first call is snapshot, two warm-up steps, restore, capture and first replay: afterwards the step
    count reads exactly 1, the update is the oracle's for t = 1 from the UNTOUCHED initial state (forced_step clones it before the call), and
    the BatchNorm buffers are those of one eager step from the same start, bit for bit (the two runs execute the same kernels on the same
    state; num_batches_tracked is one more than before).  Then five replays, the lr changed before each,
    with a second shape (64 encounters) entering the cache in between -- all teacher-forced."""
    case = real_case(256)
    st = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0, use_graphs=True)
    eager = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0, use_graphs=False)
    outputs, ratios = {}, {}
    tracked = {k: int(b) for k, b in st.model.named_buffers() if k.endswith('num_batches_tracked')}
    forced_step(st, batch_call(st, case, slice(0, 256)), outputs, ratios)
    assert float(st.optimizer._step) == 1.0 and len(st._graphs) == 1
    batch_call(eager, case, slice(0, 256))()
    torch.cuda.synchronize()
    n_buf = 0
    for (k, a), (_, b) in zip(st.model.named_buffers(), eager.model.named_buffers()):
        n_buf += 1
        assert torch.equal(a, b) and (k not in tracked or int(a) == tracked[k] + 1), k          # bit for bit; ONE batch was tracked, not three
    assert n_buf >= 3 and tracked
    for i in range(5):
        st.optimizer.param_groups[0]['lr'] = LR * 0.7 ** (i + 1)
        forced_step(st, batch_call(st, case, slice(0, 256)), outputs, ratios)
        if i == 1:
            forced_step(st, batch_call(st, case, slice(100, 164)), outputs, ratios)
    assert len(st._graphs) == 2 and float(st.optimizer._step) == 7.0
    finish('graphed_step', 'bf16 B=256 first call + 5 replays + second shape', outputs, ratios)


@pytest.mark.parametrize('use_graphs', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('kind', ['centres', 'fake-head'])
def test_unreached_parameters_are_left_alone(kind, use_graphs):
    """loss='ae_mse' on a Net with cluster centres; a Net with the fake-detection head under a loss without it.  Which parameters are unreached
    comes from the f64 OracleNet.  Over four steps with weight_decay > 0 their slices of p, m, v, vmax keep their bits; everything else meets
    the bars.  The one known difference from torch.optim (flat_adam.py's docstring): the step count is shared, so the unreached parameter
    carries the global count where torch would hold no state for it."""
    case = real_case(64, fake=kind == 'fake-head')
    loss, kl = ('ae_mse', 0.0) if kind == 'centres' else ('ae_mse_kl', 10.0)
    unreached = oracle_unreached(case, kl)
    assert unreached == ['cluster_assignment.cluster_centers'] if kind == 'centres' else (unreached and all(k.startswith('fake_det_head.') for k in unreached)), unreached
    st = make_stepper(case, 'bf16', loss, 15.0, use_graphs=use_graphs, wd=4e-4)
    off = mask_of(st, unreached) == 0
    assert 0 < off.sum() < off.size
    first = state_arrays(st)
    outputs, ratios = {}, {}
    for i in range(4):
        _, last = forced_step(st, batch_call(st, case, slice(0, 64)), outputs, ratios, unreached)
    for a, b in zip(first, last):
        assert np.array_equal(a[off].view(np.uint32), b[off].view(np.uint32))
        assert not np.array_equal(a[~off], b[~off]) or not a.any()
    assert not last[1][off].any() and not last[3][off].any() and first[0][off].any()
    p_un = dict(st.model.named_parameters())[unreached[0]]
    assert st.optimizer.state[p_un]['step'] is st.optimizer._step and float(st.optimizer._step) == 4.0          # torch.optim.Adam: no state at all
    assert use_graphs == (len(st._graphs) == 1)
    finish('unreached', f'{kind} {"graphed" if use_graphs else "eager"}', outputs, ratios, unreached=unreached)


def test_a_captured_steps_mask_outlives_a_change_of_reach_pattern():
    """One Stepper: (1) a graphed step under reach pattern A (loss 'ae_mse' on a Net with centres and the fake-detection head: both unreached);
    (2) an eager step under pattern B (loss 'ae_mse_kl': only the head unreached; a dict among the step() arguments makes it eager);
    (3) eight device allocations of the mask's size filled with zeros; (4) a replay of A.  The captured Adam launch carries the device
    pointer of A's mask: it must still hold A's bytes -- the replay meets the bars, A's unreached slices keep their bits, and the tensor
    ``active_mask()`` handed out for A is still alive and unchanged.  (A second partial pattern cannot be formed through a `_sup` loss:
    ``sup_aux_loss`` needs a label for every task, so the loss name is switched on ``args`` instead.)"""
    case = real_case(64, fake=True)
    un_a, un_b = oracle_unreached(case, 0.0), oracle_unreached(case, 10.0)
    assert set(un_b) < set(un_a) and un_b
    st = make_stepper(case, 'bf16', 'ae_mse', 15.0, use_graphs=True)
    outputs, ratios = {}, {}
    call = batch_call(st, case, slice(0, 64))
    forced_step(st, call, outputs, ratios, un_a)                                                         # (1)
    assert len(st._graphs) == 1
    alive = weakref.ref(st.flat.active_mask())
    bytes_a = alive().cpu().numpy().copy()
    assert np.array_equal(bytes_a, mask_of(st, un_a))
    st.args.loss = 'ae_mse_kl'
    forced_step(st, batch_call(st, case, slice(0, 64), aux_label_dict={'unused': torch.zeros(1)}), outputs, ratios, un_b)      # (2)
    assert len(st._graphs) == 1 and np.array_equal(st.flat.active_mask().cpu().numpy(), mask_of(st, un_b))
    junk = [torch.zeros(bytes_a.size, dtype=torch.uint8, device='cuda') for _ in range(8)]              # (3)
    st.args.loss = 'ae_mse'
    forced_step(st, call, outputs, ratios, un_a)                                                         # (4)
    assert len(st._graphs) == 1 and float(st.optimizer._step) == 3.0 and len(junk) == 8
    still = alive() is not None and np.array_equal(alive().cpu().numpy(), bytes_a)
    _worst(outputs, "pattern A's mask freed or changed", int(not still), 0)
    finish('mask_lifetime', 'A graphed, B eager, zeros, A replayed', outputs, ratios)


def test_resumed_graphed_run_is_bit_identical_to_an_uninterrupted_one(tmp_path):
    """Three graphed steps, the trainers' checkpoint writer, a FRESH Net and Stepper that load it the way ``TrainerBase.load_weight`` does,
    three more graphed steps: parameters and all optimiser state bit-identical to six uninterrupted steps."""
    from deep_interpolation_clustering_amd import _host
    case = real_case(384)
    rows = [slice(64 * i, 64 * i + 64) for i in range(6)]

    def run(st, which):
        for r in which:
            batch_call(st, case, r)()
        torch.cuda.synchronize()

    whole = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0, use_graphs=True)
    run(whole, rows)
    first = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0, use_graphs=True)
    run(first, rows[:3])
    path = str(tmp_path / 'model.pth.tar')
    _host.write_checkpoint(3, first.model, first.optimizer, path)
    torch.manual_seed(99)
    second = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0, use_graphs=True, load_state=False)
    ckpt = torch.load(path, map_location=torch.device('cuda'))
    second.model.load_state_dict(ckpt['state_dict'])
    second.optimizer.load_state_dict(ckpt['optimizer'])
    run(second, rows[3:])
    assert float(second.optimizer._step) == float(whole.optimizer._step) == 6.0
    differ = {name: int((a.view(np.uint32) != b.view(np.uint32)).sum()) for name, a, b in zip(('p', 'm', 'v', 'vmax'), state_arrays(whole), state_arrays(second))}
    _append({'test': 'resume', 'case': '3 + checkpoint + 3 against 6', 'outputs': {f'{k} elements that differ': [v, 0] for k, v in differ.items()}})
    assert not any(differ.values()), differ
    for (k, a), (_, b) in zip(whole.model.named_buffers(), second.model.named_buffers()):
        assert torch.equal(a, b), k


def test_nan_gradient_kills_the_step_as_torch_does():
    """One NaN element written into the bucket's gradient, then ``clip_coef`` + ``FlatAdam.step``: what tests/test_optim_oracle.py records for
    torch -- the norm and the coefficient are NaN (clamp(max=1.0) keeps a NaN) and every parameter, with its m and v, is NaN.  One stated
    difference stays: vmax keeps its old value (fmaxf drops the NaN, torch.maximum hands it on) -- recorded, not asserted; the parameters
    are gone either way, and the select that would hand it on changes the bits of every healthy step (csrc/dic_optim.hip)."""
    case = real_case(64)
    st = make_stepper(case, 'bf16', 'ae_mse_kl', 15.0)
    st.flat.zero_grad()
    st.flat.grad.copy_(1e-3 * torch.randn(st.flat.grad.numel(), generator=torch.Generator().manual_seed(0)))
    st.flat.grad[12345] = float('nan')
    total, coef = st.flat.clip_coef(15.0)
    st.optimizer.step(grad_scale=coef)
    torch.cuda.synchronize()
    p, m, v, vm = state_arrays(st)
    got = {'total is NaN': math.isnan(float(total)), 'coef is NaN': math.isnan(float(coef)), 'p all NaN': bool(np.isnan(p).all()),
           'm all NaN': bool(np.isnan(m).all()), 'v all NaN': bool(np.isnan(v).all())}
    print(f'[optim] NaN gradient element: total {float(total)} coef {float(coef)} {got}; finite p {int(np.isfinite(p).sum())} of {p.size}; NaN vmax {int(np.isnan(vm).sum())}')
    _append({'test': 'nan_gradient', 'case': 'one NaN element', 'outputs': {k: [int(not ok), 0] for k, ok in got.items()}, 'coef': repr(float(coef)),
             'reported': {'vmax elements that are NaN (torch: all; not asserted, see csrc/dic_optim.hip)': int(np.isnan(vm).sum())}})
    assert all(got.values()), got
