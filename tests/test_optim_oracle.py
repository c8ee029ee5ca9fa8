"""oracle/optim_oracle.py against the optimiser of the reference's training step: ``torch.optim.Adam(amsgrad=True, weight_decay=...)`` after
``torch.nn.utils.clip_grad_norm_`` (pretrain_trainer.py:228-229, utils.py:83), both run in float64 on CPU tensors.

Teacher-forced: before every step the oracle is handed torch's own parameters, optimiser state and unclipped gradients as ONE flat vector (with
an ``active`` mask over the parameter that never receives a gradient); after it, every output must agree with torch's to 1e-12 relative -- two
float64 evaluations of the same formula.  The last step carries a NaN gradient element and records what torch does with it."""
import math

import numpy as np
import torch

from oracle import optim_oracle as OO

SHAPES = [(37, 5), (5,), (3, 4, 2), (1,), (11,)]
IDLE = 3                   # index of the parameter whose .grad stays None throughout
STEPS = 20
MAX_NORM = 2.0


def _flat(ts):
    return np.concatenate([np.asarray(t.detach().numpy(), dtype=np.float64).reshape(-1) for t in ts])


def _state_flat(opt, params, key):
    return np.concatenate([(opt.state[p][key].detach().numpy().reshape(-1) if p in opt.state and key in opt.state[p]
                            else np.zeros(p.numel())) for p in params])


def _assert_rel(got, want, what, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert (err <= tol * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))


def test_oracle_is_torch_adam_amsgrad_after_clip_grad_norm_in_f64():
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in SHAPES]
    idle0 = params[IDLE].detach().clone()
    wd, betas, eps = 4e-4, (0.9, 0.999), 1e-8
    opt = torch.optim.Adam(params, lr=3e-3, betas=betas, eps=eps, weight_decay=wd, amsgrad=True)
    active = np.concatenate([np.full(p.numel(), 0 if i == IDLE else 1, np.uint8) for i, p in enumerate(params)])
    clipped = []
    for s in range(STEPS + 1):
        nan_step = s == STEPS
        lr = 3e-3 * (0.8 ** s)                                            # a scheduler step before every batch
        opt.param_groups[0]['lr'] = lr
        scale = 10.0 if s % 3 == 0 else 0.01                              # |g| ~ 60 (clipped to 2) on every third step, ~ 0.06 (coef = 1) otherwise
        for i, p in enumerate(params):
            p.grad = None if i == IDLE else scale * torch.randn(p.shape, generator=gen, dtype=torch.float64)
        if nan_step:
            params[2].grad.view(-1)[5] = float('nan')
        g0 = np.concatenate([np.zeros(p.numel()) if p.grad is None else p.grad.numpy().reshape(-1) for p in params])
        pre = [_flat(params)] + [_state_flat(opt, params, k) for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')]
        total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        coef_torch = float(params[0].grad.view(-1)[0]) / g0[0]            # what clip_grad_norm_ multiplied the gradients by
        opt.step()
        o_total, o_coef = OO.grad_norm_clip(g0, MAX_NORM)
        p1, g1, m1, v1, vm1 = OO.adam_amsgrad_step(pre[0], g0, pre[1], pre[2], pre[3], s + 1, lr, betas[0], betas[1], eps, wd, coef=o_coef, active=active)
        assert IDLE not in [i for i, p in enumerate(params) if p in opt.state and opt.state[p]]          # no state for the parameter without a gradient
        assert torch.equal(params[IDLE].detach(), idle0)
        if nan_step:
            # what torch does with one NaN gradient element: the norm is NaN, clamp(max=1.0) keeps the NaN, every gradient is multiplied by it,
            # and every parameter that has a gradient -- with its whole state -- is NaN after the step.  The oracle says the same.
            assert math.isnan(float(total)) and math.isnan(coef_torch) and math.isnan(o_total) and math.isnan(o_coef)
            on = active != 0
            for got, want in ((p1, _flat(params)), (m1, _state_flat(opt, params, 'exp_avg')), (v1, _state_flat(opt, params, 'exp_avg_sq')),
                              (vm1, _state_flat(opt, params, 'max_exp_avg_sq'))):
                assert np.isnan(want[on]).all() and np.isnan(got[on]).all()
            assert np.array_equal(p1[~on], idle0.numpy().reshape(-1)) and not vm1[~on].any()
            break
        clipped.append(o_coef < 1.0)
        above = bool((vm1 > v1).any())
        _assert_rel(o_total, float(total), 'total')
        _assert_rel(o_coef, coef_torch if o_coef < 1.0 else 1.0, 'coef')
        assert (coef_torch == 1.0) == (o_coef == 1.0)
        assert all(float(opt.state[p]['step']) == s + 1 for i, p in enumerate(params) if i != IDLE)
        grads1 = np.concatenate([np.zeros(p.numel()) if p.grad is None else p.grad.numpy().reshape(-1) for p in params])
        for got, want, what in ((p1, _flat(params), 'p'), (g1, grads1, 'g'), (m1, _state_flat(opt, params, 'exp_avg'), 'm'),
                                (v1, _state_flat(opt, params, 'exp_avg_sq'), 'v'), (vm1, _state_flat(opt, params, 'max_exp_avg_sq'), 'vmax')):
            _assert_rel(got, want, f'{what} at step {s + 1}')
        # inactive elements: all five arrays exactly as they went in
        off = active == 0
        for got, was in zip((p1, g1, m1, v1, vm1), (pre[0], g0, pre[1], pre[2], pre[3])):
            assert np.array_equal(got[off], was[off])
    assert any(clipped) and not all(clipped)
    assert above                       # amsgrad did something: once the large-gradient steps decay, vmax stays above v


def test_oracle_takes_hyper_parameters_as_given():
    """f32-rounded hyper-parameters widened to f64 are NOT the Python doubles: the oracle keeps them apart (at t = 1, 1 - b2 differs by 2e-5
    relative between b2 = 0.999 and float32(0.999)), and a zero coefficient / an all-zero mask behave as the formulas say."""
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal(64), rng.standard_normal(64)
    z = np.zeros(64)
    exact = OO.adam_amsgrad_step(p, g, z, z, z, 1, 3e-3, 0.9, 0.999, 1e-8, 0.0)
    f32 = OO.adam_amsgrad_step(p, g, z, z, z, 1, *(float(np.float32(x)) for x in (3e-3, 0.9, 0.999, 1e-8, 0.0)))
    rel = np.abs((f32[0] - p) / (exact[0] - p) - 1)
    assert 1e-9 < rel.max() < 1e-4
    # t = 1 from zero state: the update is lr * sign(g) up to eps
    np.testing.assert_allclose(exact[0] - p, -3e-3 * np.sign(g), rtol=1e-6)
    same = OO.adam_amsgrad_step(p, g, z, z, z, 1, 3e-3, 0.9, 0.999, 1e-8, 4e-4, coef=0.37, active=np.zeros(64, np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip(same, (p, g, z, z, z)))
    assert OO.grad_norm_clip(z, 1.0) == (0.0, 1.0)
    assert OO.grad_norm_clip([3.0, 4.0], 5.0 + 1e-6)[1] == 1.0 and OO.grad_norm_clip([3.0, 4.0], 2.5)[1] < 0.5


def test_update_ratio_selection_keeps_95_percent_by_the_oracle_alone():
    """The two conditions under which tests/test_gpu_optim.py compares the parameter update element by element (sqrt(vmax') > 1e4 eps and
    |dp| > 64 ulp(p)), evaluated on the oracle's own step, leave out at most 5 % of the inputs those tests build -- at every t they use and
    at both ends of the clip coefficient.  No GPU arithmetic enters: the cap is met by the choice of inputs."""
    p, g, m, v, vm, dead = OO.adam_inputs(131073, np.random.default_rng(5))
    assert 0.015 < dead.mean() < 0.02
    hy = [float(np.float32(x)) for x in (OO.LR, OO.B1, OO.B2, OO.EPS, 4e-4)]
    for t in OO.T_STEPS:
        for coef in (1.0, 0.37):
            o_p, _, _, _, o_vm = OO.adam_amsgrad_step(p, g, m, v, vm, t, *hy, coef=coef)
            sel = (np.sqrt(o_vm) > 1e4 * hy[3]) & (np.abs(o_p - p) > 64 * np.spacing(np.abs(p)))
            assert 1 - sel.mean() <= 0.05, (t, coef, 1 - sel.mean())
