"""The tail of the training step -- clip_grad_norm_ followed by Adam(amsgrad=True, weight_decay = L2) -- restated in NumPy float64.

TEST INFRASTRUCTURE ONLY -- see ``oracle/__init__.py``.  Written from the formulas (torch/nn/utils/clip_grad.py, torch/optim/adam.py's
single-tensor path, as the header of csrc/dic_optim.hip states them), over ONE flat vector as the kernels see it:

    total = |g|_2 ;  coef = min(1, max_norm / (total + 1e-6))            (NaN total -> NaN coef, as torch.clamp(max=1.0) gives)
    g <- coef * g  (written back) ;  g' = g + wd * p
    m = m + (g' - m)(1 - b1) ;  v = b2 v + (1 - b2) g' g' ;  vmax = max(vmax, v)
    p = p - lr / (1 - b1^t) * (m / (sqrt(vmax) / sqrt(1 - b2^t) + eps))

Every hyper-parameter is taken AS GIVEN and widened to float64: handed the f32-rounded values a kernel receives, the oracle measures that
kernel's own roundings; handed the exact Python doubles, it is what the reference's optimiser computes (tests/test_optim_oracle.py pins it
to ``torch.optim.Adam`` + ``clip_grad_norm_`` in float64 at 1e-12).  Elements whose ``active`` byte is zero are unchanged in all five arrays
(``torch.optim`` skips a parameter whose ``grad is None``: no decay, no state).
"""
from __future__ import annotations

import json

import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def grad_norm_clip(g, max_norm):
    """(total, coef) of clip_grad_norm_ over the flat gradient ``g``, in float64."""
    g = _f64(g).reshape(-1)
    total = np.sqrt(np.sum(g * g))
    with np.errstate(invalid='ignore'):
        coef = np.minimum(np.float64(1.0), np.float64(max_norm) / (total + np.float64(1e-6)))          # np.minimum propagates NaN, as clamp does
    return float(total), float(coef)


def bias_corrections(t, lr, b1, b2):
    """(step_size = lr / (1 - b1^t), sqrt(1 - b2^t)) in float64 from the values as given."""
    t, lr, b1, b2 = (np.float64(x) for x in (t, lr, b1, b2))
    return float(lr / (1.0 - np.power(b1, t))), float(np.sqrt(1.0 - np.power(b2, t)))


def adam_amsgrad_step(p, g, m, v, vmax, t, lr, b1, b2, eps, wd, coef=None, active=None):
    """New (p, g, m, v, vmax) as float64 arrays.  ``t``: the step count already incremented (1 on the first step).  ``coef``: the clip
    coefficient multiplied into ``g`` first (None: 1).  ``active``: None or a per-element mask; inactive elements keep all five inputs."""
    p, g, m, v, vmax = (_f64(a).copy() for a in (p, g, m, v, vmax))
    lr, b1, b2, eps, wd = (np.float64(x) for x in (lr, b1, b2, eps, wd))
    step_size, bc2_sqrt = bias_corrections(t, lr, b1, b2)
    with np.errstate(invalid='ignore', over='ignore'):
        gs = g * (np.float64(1.0) if coef is None else np.float64(coef))
        gd = gs + wd * p
        m1 = m + (gd - m) * (1.0 - b1)
        v1 = b2 * v + (1.0 - b2) * gd * gd
        vm1 = np.maximum(vmax, v1)                                    # (propagates NaN, as torch.maximum does)
        p1 = p - step_size * (m1 / (np.sqrt(vm1) / bc2_sqrt + eps))
    if active is None:
        return p1, gs, m1, v1, vm1
    on = np.asarray(active).reshape(-1) != 0
    return tuple(np.where(on, new, old) for new, old in ((p1, p), (gs, g), (m1, m), (v1, v), (vm1, vmax)))


# ---------------------------------------------------------------------------------------------------------------- inputs of the kernel tests
LR, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8          # utils.py:83 / p1:86
T_STEPS = [1, 2, 10, 1000, 100000]


def adam_inputs(n, rng):
    """(p, g, m, v, vmax, dead) in f32 for the kernel-level Adam cases: the state is what two oracle steps leave (consistent, vmax >= v), with
    vmax > v on every seventh row (a large gradient followed by a small one) and g = m = v = vmax = 0 on every 53rd row (from index 17 on;
    ``dead`` marks them)."""
    i = np.arange(n)
    p = (0.05 * rng.standard_normal(n)).astype(np.float32)
    ga, gb, g = (rng.standard_normal(n) for _ in range(3))
    big = i % 7 == 3
    ga[big] *= 10.0
    gb[big] = 0.02 * ga[big]
    dead = i % 53 == 17
    for a in (ga, gb, g):
        a[dead] = 0.0
    z = np.zeros(n)
    hy = [float(np.float32(x)) for x in (LR, B1, B2, EPS)]
    _, _, m, v, vm = adam_amsgrad_step(p, ga, z, z, z, 1, *hy, 0.0)
    _, _, m, v, vm = adam_amsgrad_step(p, gb, m, v, vm, 2, *hy, 0.0)
    m, v, vm = (a.astype(np.float32) for a in (m, v, vm))
    assert (vm >= v).all() and (n < 64 or (vm[big] > v[big]).any()) and not (m[dead].any() or vm[dead].any())
    return p, g.astype(np.float32), m, v, vm, dead


# ---------------------------------------------------------------------------------------------------------------- the committed record
def condense(jsonl_path: str, out_path: str) -> None:
    """profiles/optim_parity.json from the JSON lines one run of tests/test_gpu_optim.py appends: per test the worst measured / bar of every
    output over its cases (with the case it occurred in), the largest share of elements left out, and per step count t the scalar ratios of
    the parameter update against the f32-hyper and the exact-double-hyper oracle.  ``python -m oracle.optim_oracle <jsonl> <out>``."""
    sig = lambda x: float('%.4g' % x)          # noqa: E731
    tests, ratios = {}, {}
    for r in (json.loads(line) for line in open(jsonl_path)):
        q = tests.setdefault(r['test'], {'cases': 0, 'outputs': {}, 'left_out_max': 0.0})
        q['cases'] += 1
        q['left_out_max'] = max(q['left_out_max'], sig(r.get('left_out', 0.0)))
        if r.get('reported'):
            q.setdefault('reported', {}).update(r['reported'])
        for name, (got, bar) in r.get('outputs', {}).items():
            o = q['outputs'].get(name)
            over = got / bar if bar else (0.0 if got == 0 else float('inf'))
            if o is None or over > o['_over']:
                q['outputs'][name] = {'measured': sig(got), 'bar': sig(bar), 'case': r.get('case'), '_over': over}
        # (the kernel-level case of ONE element is kept apart: its "median" is that element, with the element's own roundings in it)
        group = r['test'] + (' (n = 1)' if r.get('case') == 'n=1' else '')
        for t, pair in r.get('scalar_ratio', {}).items():
            e = ratios.setdefault(group, {}).setdefault(str(t), {'f32_hyper_minus_1': 0.0, 'double_hyper_minus_1': 0.0})
            for key, val in zip(('f32_hyper_minus_1', 'double_hyper_minus_1'), pair):
                if abs(val - 1.0) > abs(e[key]):
                    e[key] = sig(val - 1.0)
    for q in tests.values():
        for o in q['outputs'].values():
            del o['_over']
    note = ('tests/test_gpu_optim.py on one MI355X, one run, condensed by oracle.optim_oracle.condense.  Per test: the number of recorded cases and, per output, '
            'the measured value nearest to (or furthest over) its bar with that bar and the case; left_out_max = the largest share of elements the update-ratio '
            'conditions left out (capped at 0.05 in the kernel-level cases; on the real step recorded, with a floor of 256 selected elements instead); '
            'reported = figures stated without an assertion.  scalar_ratio: per test and step count t the median of dp_gpu / dp_oracle minus 1 that lies furthest from 0, against '
            'the oracle with the f32-rounded hyper-parameters the kernel receives (barred) and against the oracle with the exact Python doubles (the distance '
            "from the reference optimiser's double-precision bias correction: reported, no bar).")
    with open(out_path, 'w') as f:
        json.dump({'_note': note, 'tests': tests, 'scalar_ratio': ratios}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    import sys
    condense(sys.argv[1], sys.argv[2])
