"""Every parameter gradient of one joint step from the CPU oracle, and how far another set of gradients is from it.

TEST INFRASTRUCTURE ONLY -- see ``oracle/__init__.py``.  ``reference_grads`` runs ``dic_oracle.OracleNet`` / ``joint_loss`` once, forward and
backward, in train mode, in float64 (the reference the GPU step's gradients are held to), in float32 (the floor: how far one plain f32
evaluation is from f64) or under CPU bf16 autocast around an f32 net (the floor of the bf16 mode).  ``compare`` gives the per-tensor and
whole-bucket distances.  tests/test_step_grads_oracle.py pins the f64 gradients to the ones the reference itself wrote into
tests/golden/netstep_*.npz; tests/test_gpu_step_grads.py holds the GPU step to them.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import dic_oracle as O

NULL_SHARE = 1e-6     # a tensor whose true gradient carries less than this share of the total norm is a "null" tensor: its true gradient is zero
ARITHMETICS = ('f64', 'f32', 'bf16', 'x3')


def _t(v, dtype=None):
    v = v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
    return v.to(dtype) if (dtype is not None and v.dtype.is_floating_point) else v


# ---------------------------------------------------------------------------------------------------------------- the x3 emulation
def _split(a):
    """f32 operand -> (hi, lo) as the x3 kernels split it: hi = bf16(a), lo = bf16(a - hi); returned in f64."""
    a32 = a.detach().float()
    hi = a32.bfloat16().float()
    return hi.double(), (a32 - hi).bfloat16().double()


class _X3MatMul(torch.autograd.Function):
    """a @ b as the three-term bf16 split hi.hi + lo.hi + hi.lo of the f32-rounded operands, accumulated in f64 -- forward and both backward
    products (lo.lo dropped, lo rounded to bf16: about 2^-17 per product)."""

    @staticmethod
    def x3(a, b):
        ah, al = _split(a)
        bh, bl = _split(b)
        return ah @ bh + al @ bh + ah @ bl

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _X3MatMul.x3(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _X3MatMul.x3(g, b.t()), _X3MatMul.x3(a.t(), g)


def _x3_linear(lin):
    lin.forward = lambda x: _X3MatMul.apply(x, lin.weight.t()) + lin.bias


def _x3_lstm(lstm):
    """nn.LSTM(bidirectional, one layer, time-major) as a hand-written loop whose input and recurrent products are split products."""
    def forward(x, state=None):
        R, B, _ = x.shape
        H = lstm.hidden_size
        outs, hn, cn = [], [], []
        for d, sfx in enumerate(('', '_reverse')):
            w_ih, w_hh = getattr(lstm, 'weight_ih_l0' + sfx), getattr(lstm, 'weight_hh_l0' + sfx)
            bias = getattr(lstm, 'bias_ih_l0' + sfx) + getattr(lstm, 'bias_hh_l0' + sfx)
            gx = (_X3MatMul.apply(x.reshape(R * B, -1), w_ih.t()) + bias).reshape(R, B, 4 * H)
            h = x.new_zeros(B, H) if state is None else state[0][d]
            c = x.new_zeros(B, H) if state is None else state[1][d]
            hs = [None] * R
            for t in (range(R) if d == 0 else range(R - 1, -1, -1)):
                i, f, g, o = (gx[t] + _X3MatMul.apply(h, w_hh.t())).chunk(4, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                hs[t] = h
            outs.append(torch.stack(hs))
            hn.append(h)
            cn.append(c)
        return torch.cat(outs, dim=2), (torch.stack(hn), torch.stack(cn))
    lstm.forward = forward


def reference_grads(state_dict, x, ob, *, C, R, H, K, fake: Optional[dict] = None, arithmetic: str = 'f64',
                    kl_weight: float = 10.0, chunk: Optional[int] = 512, taps: Optional[dict] = None) -> Tuple[Dict[str, torch.Tensor], Dict[str, float]]:
    """({parameter name: float64 gradient}, {loss term: float, 'gnorm': float}) of ``joint_loss(...)['loss'].backward()`` on an ``OracleNet`` carrying
    ``state_dict`` (upstream key names; tensors or arrays), train mode, dropout 0, padding mask = the mask plane of ``x``.
    ``fake``: None, or {'fake_x', 'fake_perm_idx', 'fake_label'} for the fake-detection objective (weight 1).  ``chunk``: encounters per
    checkpointed piece of the interpolation layers (memory of a large batch; ``dic_oracle._by_encounters``).  ``taps``: see
    ``dic_oracle.tapped_relu`` -- receives the pre-activations of the two ReLUs; ``taps['flip']`` inverts chosen derivative masks."""
    if arithmetic not in ARITHMETICS:
        raise ValueError(arithmetic)
    dtype = torch.float64 if arithmetic in ('f64', 'x3') else torch.float32
    net = O.OracleNet(C, R, H, K, 0.0, fake_detection=fake is not None)
    net.load_state_dict({k: _t(v) for k, v in state_dict.items()}, strict=True)
    net = net.to(dtype)
    net.train()
    net.chunk, net.taps = chunk, taps
    if arithmetic == 'x3':        # the dense products of the GPU's x3 step: both LSTMs, the first layer of CompressFC and of the detection head
        _x3_lstm(net.encoder.lstm)
        _x3_lstm(net.decoder.lstm)
        _x3_linear(net.rbf.compress_fc.module.model[0])
        if fake is not None:
            _x3_linear(net.fake_det_head.model[0])
    x, ob = _t(x, dtype), _t(ob, dtype)
    kw = {}
    if fake is not None:
        kw = dict(fake_x=_t(fake['fake_x'], dtype), fake_perm_idx=_t(fake['fake_perm_idx']).long(), fake_label=_t(fake['fake_label']).long())
    with torch.autocast('cpu', dtype=torch.bfloat16, enabled=arithmetic == 'bf16'):
        terms, _, _, _ = O.joint_loss(net, x, ob, x[:, C:2 * C], kl_weight, **kw)
    terms['loss'].backward()
    grads = {k: p.grad.detach().double() for k, p in net.named_parameters()}
    out = {k: float(v.detach()) for k, v in terms.items()}
    # the total gradient norm the way clip_grad_norm_ forms it, in this arithmetic: per-tensor norms, then the norm of those
    out['gnorm'] = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in net.parameters()])))
    return grads, out


def total_norm(grads) -> float:
    return math.sqrt(sum(float(_t(g, torch.float64).pow(2).sum()) for g in grads.values()))


def compare(got, want, gnorm: Optional[float] = None) -> dict:
    """Distances of the gradients ``got`` from the reference ``want`` (same keys).  Per tensor: rel_l2 = |got - want|_2 / |want|_2,
    max_over_max = max|got - want| / max|want|, share = |want|_2 / gnorm, got_share = |got|_2 / gnorm (what a null tensor, share <
    NULL_SHARE, is judged on), cos.  Over all tensors: total = |got - want|_2 / gnorm.  ``gnorm`` defaults to the reference's total norm."""
    if set(got) != set(want):
        raise KeyError(f'gradient names differ: {sorted(set(got) ^ set(want))}')
    gnorm = total_norm(want) if gnorm is None else float(gnorm)
    out, sq = {}, 0.0
    for k, w in want.items():
        w, g = _t(w, torch.float64).reshape(-1), _t(got[k], torch.float64).reshape(-1)
        if g.shape != w.shape:
            raise ValueError(f'{k}: {tuple(g.shape)} against {tuple(w.shape)}')
        d = g - w
        nw, ng, nd = float(w.norm()), float(g.norm()), float(d.norm())
        sq += nd * nd
        out[k] = {'rel_l2': nd / nw if nw > 0 else math.inf, 'max_over_max': float(d.abs().max()) / float(w.abs().max()) if nw > 0 else math.inf,
                  'share': nw / gnorm, 'got_share': ng / gnorm, 'cos': float(g @ w) / (ng * nw) if ng > 0 and nw > 0 else 0.0,
                  'null': nw / gnorm < NULL_SHARE}
        if not math.isfinite(ng):
            out[k]['rel_l2'] = out[k]['max_over_max'] = out[k]['got_share'] = math.inf
    return {'tensors': out, 'total': math.sqrt(sq) / gnorm if math.isfinite(sq) else math.inf, 'gnorm': gnorm}


# ---------------------------------------------------------------------------------------------------------------- fixture plumbing
def fixture_case(name: str, load) -> dict:
    """State, batch and shape of one ``tests/golden/netstep_<name>.npz`` step as ``reference_grads`` takes them.  ``load(file name)`` returns
    the fixture as a dict of arrays.  cfg_K4 / cfg_K8: the p1 state of traj_cfg1.npz with the fixture's k-means centres; wide_K16 carries its
    own state; plain / fake: netstep_plain's state, fake overlaying its detection head."""
    g = load(f'netstep_{name}.npz')
    fake = None
    if name in ('cfg_K4', 'cfg_K8'):
        t = load('traj_cfg1.npz')
        sd = {k[5:]: v for k, v in t.items() if k.startswith('p1sd/')}
        sd['cluster_assignment.cluster_centers'] = g['centers']
    else:
        sd = {}
        if name in ('plain', 'fake'):
            sd = {k[4:]: v for k, v in load('netstep_plain.npz').items() if k.startswith('sd0/')}
        sd.update({k[4:]: v for k, v in g.items() if k.startswith('sd0/')})
        if name == 'fake':
            fake = {k: g[k] for k in ('fake_x', 'fake_perm_idx', 'fake_label')}
    C = int(g['C']) if 'C' in g else 6
    return {'g': g, 'state': sd, 'x': g['x'], 'ob': g['ob'], 'fake': fake,
            'shape': dict(C=C, R=int(g['R']), H=float(g['H']), K=int(g['K']))}


def fixture_gradient_misses(grads, g, bar: float = 1e-4, bars: Optional[dict] = None, null_bar: float = NULL_SHARE) -> list:
    """The full gradients a netstep fixture stores (``g/<name>``: the reference's own f32 values) against ``grads`` (name -> tensor, e.g. the
    ``.grad`` of ``named_parameters()`` after an unclipped step): every (name, figure, value, bar) with rel_l2 above ``bar`` (or above the
    tensor's own entry in ``bars``).  A tensor whose stored gradient is null (the reference's own rounding noise, below NULL_SHARE of the
    fixture's gnorm) is held to |got|_2 / gnorm <= ``null_bar`` instead."""
    stored = {k[2:]: v for k, v in g.items() if k.startswith('g/')}
    cmp = compare({k: grads[k] for k in stored}, stored, float(g['gnorm']))['tensors']
    bad = []
    for k, v in cmp.items():
        if v['null']:
            if not v['got_share'] <= null_bar:
                bad.append((k, 'null |got|/gnorm', v['got_share'], null_bar))
        else:
            allowed = max(bar, (bars or {}).get(k, 0.0))
            if not v['rel_l2'] <= allowed:
                bad.append((k, 'rel_l2', v['rel_l2'], allowed))
    return bad


def x3_bars(case: dict, g64=None) -> dict:
    """Per live tensor the bars of the x3 mode: (max(1e-4, 4 x d), max(2e-4, 4 x m)) with d / m the rel_l2 / max_over_max of the x3 EMULATION
    (``reference_grads(arithmetic='x3')``: split products accumulated in f64) from the f64 reference -- what the split itself costs, from the
    reference side; the plain bars wherever that is below a quarter of them."""
    ref = dict(fake=case['fake'], **case['shape'])
    if g64 is None:
        g64, _ = reference_grads(case['state'], case['x'], case['ob'], arithmetic='f64', **ref)
    gx, _ = reference_grads(case['state'], case['x'], case['ob'], arithmetic='x3', **ref)
    return {k: {'rel_l2': max(1e-4, 4 * v['rel_l2']), 'max_over_max': max(2e-4, 4 * v['max_over_max']), 'x3_rel_l2': v['rel_l2'], 'x3_max_over_max': v['max_over_max']}
            for k, v in compare(gx, g64)['tensors'].items() if not v['null']}


# ---------------------------------------------------------------------------------------------------------------- ReLU kinks
def kink_radius(pre64, pre32, mode: str) -> float:
    """How close to zero a ReLU input of the f64 forward must lie for an f32-grade implementation to be entitled to the other side of the
    kink (the candidates of ``flip_explained``).  'exact': 4 x the rms distance of the CPU f32 oracle's pre-activations from the f64 ones at this site (one plain f32 evaluation's own
    forward error -- the rms, not the maximum, which sits on the largest activations -- with the factor every floor of these tests carries).
    'x3': at least 2^-17 of the pre-activations' rms -- the relative error of ONE three-term bf16 split product (lo.lo dropped, lo rounded to
    bf16) at the scale of the sum it enters."""
    r = 4.0 * float((pre32.double() - pre64).pow(2).mean().sqrt())
    if mode == 'x3':
        r = max(r, 2.0 ** -17 * float(pre64.pow(2).mean().sqrt()))
    return r


def flip_explained(case: dict, mode: str, got: dict, g64: dict, most: int = 16) -> dict:
    """Is the residual ``got - g64`` the signature of ReLU derivatives taken on the other side of zero?  The candidates are the (at most ``most``)
    ReLU inputs of the f64 forward nearest zero inside ``kink_radius``; for each, one more f64 backward with that ONE derivative mask inverted
    gives its flip gradient c_e over all parameters.  The residual is fitted, over the whole bucket at once, as sum_e s_e c_e with every s_e in
    [0, 1] (bounded least squares).  Returns {'elements': [(site, index, |a|, s_e)], 'got': got - sum_e s_e c_e}: the caller holds the remainder
    to the plain bars, so whatever is not exactly a flipped mask of a named near-zero element still has to be inside them."""
    from scipy.optimize import lsq_linear
    ref = dict(fake=case['fake'], **case['shape'])
    taps64, taps32 = {}, {}
    reference_grads(case['state'], case['x'], case['ob'], arithmetic='f64', taps=taps64, **ref)
    reference_grads(case['state'], case['x'], case['ob'], arithmetic='f32', taps=taps32, **ref)
    cand = []
    for site, a in taps64['pre'].items():
        r = kink_radius(a, taps32['pre'][site], mode)
        flat = a.abs().reshape(-1)
        for i in torch.nonzero(flat <= r).reshape(-1).tolist():
            cand.append((float(flat[i]) / r, site, i, float(flat[i])))
    cand = sorted(cand)[:most]
    names = [k for k in g64 if float(g64[k].norm()) > NULL_SHARE * total_norm(g64)]
    vec = lambda g: torch.cat([_t(g[k], torch.float64).reshape(-1) for k in names])          # noqa: E731
    base, cols = vec(g64), []
    for _, site, i, _ in cand:
        flip = torch.zeros(taps64['pre'][site].numel(), dtype=torch.bool)
        flip[i] = True
        ge, _ = reference_grads(case['state'], case['x'], case['ob'], arithmetic='f64', taps={'flip': {site: flip.reshape(taps64['pre'][site].shape)}}, **ref)
        cols.append(vec(ge) - base)
    out = {k: _t(v, torch.float64).clone() for k, v in got.items()}
    coef = []
    if cols:
        A = torch.stack(cols, dim=1).numpy()
        scale = float(np.abs(A).max()) or 1.0          # (gradients are O(1e-4): the solver's tolerances are absolute)
        coef = lsq_linear(A / scale, (vec(got) - base).numpy() / scale, bounds=(0.0, 1.0), method='bvls', tol=1e-13).x.tolist()
        fit, o = torch.as_tensor(A @ np.asarray(coef)), 0
        for k in names:
            n = out[k].numel()
            out[k] = out[k] - fit[o:o + n].reshape(out[k].shape)
            o += n
    return {'elements': [(site, i, a, s) for (_, site, i, a), s in zip(cand, coef)], 'got': out}


# ---------------------------------------------------------------------------------------------------------------- the committed record
def condense(jsonl_path: str, out_path: str) -> None:
    """profiles/step_grad_parity.json from the JSON lines one run of tests/test_gpu_step_grads.py appends: per (case, mode) the whole-bucket
    distance, the oracle-side floors, the worst live tensor by each figure and by figure / bar, the null tensors over their bar, the ReLU
    flips taken out (if any); the tail-sensitivity lines as they are.  ``python -m oracle.step_grads <jsonl> <out>``."""
    import json
    sig = lambda x: float('%.3g' % x)          # noqa: E731
    recs = []
    for r in (json.loads(line) for line in open(jsonl_path)):
        if 'tensors' not in r:
            recs.append({k: ({n: sig(x) for n, x in v.items()} if isinstance(v, dict) else v) for k, v in r.items()})
            continue
        live = {n: v for n, v in r['tensors'].items() if 'null' not in v['bar']}
        over = lambda v: max(v['rel_l2'] / v['bar']['rel_l2'], v['max_over_max'] / v['bar']['max_over_max'] if v['bar']['max_over_max'] else 0.0)   # noqa: E731
        worst = max(live, key=lambda n: over(live[n]))
        q = {'case': r['case'], 'mode': r['mode'], 'variant': r['variant'], 'total': sig(r['total']), 'floor_total': [sig(r['floor_total'][k]) for k in ('f32', 'bf16')],
             'worst_rel_l2': sig(max(v['rel_l2'] for v in live.values())), 'worst_max_over_max': sig(max(v['max_over_max'] for v in live.values())),
             'worst_over_bar': [worst, sig(over(live[worst]))],
             'null_over_bar': sig(max(v['got_share'] / v['bar']['null'] for v in r['tensors'].values() if 'null' in v['bar'])),
             'above_plain_bars': [n for n, v in live.items() if r['mode'] != 'bf16' and (v['rel_l2'] > 1e-4 or v['max_over_max'] > 2e-4)],
             'relu_flips_taken_out': r.get('relu_flips_taken_out')}
        recs.append({k: v for k, v in q.items() if v not in (None, [])})
    note = ('tests/test_gpu_step_grads.py on one MI355X, one run, condensed by oracle.step_grads.condense. Per (case, mode): total = |got - f64|_2 / gnorm over the whole '
            'bucket; floor_total = the same for the CPU f32 and the CPU bf16-autocast oracle; the worst live tensor by rel_l2, by max_over_max and by figure / bar; '
            "null_over_bar = the null tensors' |got|/gnorm over their bar; above_plain_bars = tensors above 1e-4 / 2e-4 (x3: held to 4 x the x3 emulation); "
            'relu_flips_taken_out = (site, index, |a|, fitted share) where a residual was explained by flipped ReLU derivatives.')
    with open(out_path, 'w') as f:
        f.write('{\n "_note": %s,\n "records": [\n' % json.dumps(note) + ',\n'.join('  ' + json.dumps(q) for q in recs) + '\n ]\n}\n')


if __name__ == '__main__':
    import sys
    condense(sys.argv[1], sys.argv[2])
