"""Every parameter gradient of ONE optimisation step on the GPU, tensor by tensor, against the float64 CPU oracle of the whole step
(oracle/step_grads.py: OracleNet + joint_loss, pinned to the reference's own gradients by tests/test_step_grads_oracle.py).

The gradient is read the way the optimiser sees it: ``Stepper.step`` (the real optimiser factory and learning rate, ``_step_eager`` /
``_step_graphed``) with ``grad_clip = 1e9``, so that clipping multiplies by exactly 1, then ``p.grad`` of every ``named_parameters()`` entry --
views into the flat gradient bucket, written by autograd, by the kernels that add past autograd, by the grad-sink session and, with fake
detection, twice.  Cases: the reference's own batches (padded input with a mask and with lengths) and synthetic batches from real state
(pretrained weights + k-means centres: KL = 0.1) at sizes that leave a tail in every tile size and cross every kernel switch -- see CASES.
Each case runs in the three precisions of the step: 'exact' (f32), 'x3' (f32 tensors, products as three-term bf16 splits), 'bf16'.

Bars (none of them comes from what the GPU measured):
  exact       per tensor max|got - want| / max|want| <= 2e-4 (the bar tests/test_gpu_ops.py holds the interpolation kernels' gradients to) and
              rel_l2 <= max(1e-4, 4 x the CPU-f32 oracle's rel_l2 for that tensor) (1e-4: the bar every step test puts on gnorm; the f32 oracle
              is 2e-7 .. 4e-5 from f64, so the bar IS 1e-4 -- except the encoder's bias gradients at fake2800, where the CPU f32 oracle itself is
              7.7e-4 / 3.1e-4 from f64: a sum over 134 400 rows of two branches that cancel).
  x3          the same, and where the three-term split itself costs more, 4 x the distance of the x3 EMULATION from f64 for that tensor, on
              both figures (oracle.step_grads.x3_bars: reference_grads(arithmetic='x3'), hand-written LSTM loops and first FC layers whose
              products are hi.hi + lo.hi + hi.lo of bf16-split f32 operands accumulated in f64).  At the cfg shape the emulation is at most 2.6e-5
              from f64 and the bars stay 1e-4 / 2e-4 (1.04e-4 on the encoder's bias gradients); at the configs[3] shape (C = 12, T = 288) it is 0.7 .. 3.5e-4 (max over max up to
              1.1e-3) and reproduces the GPU's x3 figures tensor by tensor to two digits (wide_K16: decoder.lstm.weight_ih_l0 3.15e-4 both,
              compress_fc.0.weight 3.53e-4 / 1.03e-3 both, encoder.lstm.weight_ih_l0 7.6e-5 against 7.9e-5): the miss of 1e-4 there is the
              split's own, not a kernel's; no DIC_X3_DW / DX_TILE / REC_PROJ / ROW_PROJ setting moves it.
  null        tensors whose true gradient is zero (a Linear bias feeding a training-mode BatchNorm): |got|_2 / gnorm <= 1e-6 in exact and x3.
              Only at plain / fake (B = 16, R = 12, untrained weights) the bar is 50 x the CPU-f32 oracle's value for that tensor: the column
              sum that cancels to zero leaves 5.1e-7 / 3.3e-7 of gnorm in the CPU f32 oracle itself (1e-8 .. 6e-8 everywhere else) and 1.2 ..
              1.6e-6 on the GPU -- rounding in a 192-row sum of O(1) terms; 1e-6 was never available there.
  ReLU kinks  The network has two ReLUs (between the LSTMs; inside CompressFC) and the gradient is discontinuous where a ReLU input crosses zero:
              an implementation whose forward is good to 1e-6 may land on either side of an input of 7e-7, and one such element moves a whole
              row of a small batch's gradients by more than the bars (syn257 exact: max_over_max 2.6e-4 on CompressFC's first weight, all of
              it in channel 1, whose BatchNorm output at row 2458 is 7.1e-7 in f64).  The bars are NOT widened for that.  When a case misses
              them, oracle.step_grads.flip_explained names the (at most 16) ReLU inputs of the f64 forward nearest zero inside kink_radius,
              computes each one's flip gradient by one more f64 backward with that single derivative mask inverted, fits the residual over
              the whole bucket as a combination of those with coefficients in [0, 1], and the REMAINDER is held to the same plain bars.
  bf16        per tensor rel_l2 <= 4 x the CPU bf16-autocast oracle's rel_l2 for the same tensor and case (two independent bf16 implementations
              sit up to the sum of their distances apart: 2 x; the GPU step also rounds saved gates, gate gradients and packed encoder rows to
              bf16, which CPU autocast does not: another 2 x), cosine >= 0.99, total <= 4 x the oracle's total, null tensors <= 4 x the bf16
              oracle's |got|_2 / gnorm.  That is 1 .. 12 %: loose against one dropped row, tight against anything misplaced, mis-signed or
              mis-scaled (rel_l2 ~ 1.4).

Every (case, mode) appends one JSON line with the GPU's per-tensor numbers and the oracle-side floors to step_grad_parity.jsonl beside the
trajectory tests' traj_deviation.jsonl
(last clean run, condensed by `python -m oracle.step_grads <jsonl> <out>`: profiles/step_grad_parity.json).  The float64 references are computed once per case and shared by the modes.
"""
import json
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import dic_oracle as O
from oracle import step_grads as S
from test_gpu_traj import DEV_LOG

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
LOG = os.path.join(os.path.dirname(DEV_LOG), 'step_grad_parity.jsonl')          # beside the trajectory tests' record (test_gpu_traj.log_deviation)
MODES = ['exact', 'x3', 'bf16']
TAIL_TENSORS = ('encoder.lstm.weight_ih_l0', 'decoder.lstm.weight_hh_l0_reverse', 'rbf.compress_fc.module.model.4.weight')

# name: (builder, its arguments, how the batch is handed to the step).  Why each is here:
CASES = {
    # the reference's own batches (B = 64; plain / fake: B = 16, R = 12, fake: the second encoder pass adds into the sci / cci / encoder gradients)
    'cfg_K4/mask': ('fixture', 'cfg_K4', 'mask'), 'cfg_K4/lengths': ('fixture', 'cfg_K4', 'lengths'),
    'cfg_K8/mask': ('fixture', 'cfg_K8', 'mask'), 'cfg_K8/lengths': ('fixture', 'cfg_K8', 'lengths'),
    'wide_K16/mask': ('fixture', 'wide_K16', 'mask'), 'wide_K16/lengths': ('fixture', 'wide_K16', 'lengths'),     # C = 12: packed width 64
    'plain/mask': ('fixture', 'plain', 'mask'), 'plain/lengths': ('fixture', 'plain', 'lengths'),
    'fake/mask': ('fixture', 'fake', 'mask'), 'fake/lengths': ('fixture', 'fake', 'lengths'),
    # tile tails of the 32-row (16-row) kernels; DX_TILE_MIN_ROWS and FC_BWD_MIN_ROWS crossed
    'syn31': ('synthetic', dict(B=31), 'lengths'), 'syn257': ('synthetic', dict(B=257), 'lengths'), 'syn1000': ('synthetic', dict(B=1000), 'lengths'),
    # the 64-row kernels with a one-row and a 37-row tail, resident-weight projections, fused CompressFC; ragged store input
    'store4097': ('synthetic', dict(B=4097, heavy_last=True), 'store'), 'store8229': ('synthetic', dict(B=8192 + 37, heavy_last=True), 'store'),
    # fake detection; 2800 x 24 rows > SEPARATE_ENCODER_ROWS: the fake branch gets its own encoder call
    'fake384': ('synthetic', dict(B=384, fake=True), 'lengths'), 'fake2800': ('synthetic', dict(B=2800, fake=True), 'lengths'),
    # C = 12, T = 288 on the 64-row kernels: what test_joint_step_wide_shape_bf16_tracks_f32[4160] checks on losses only
    'wide4160': ('synthetic', dict(B=4160, wide=True), 'lengths'),
}
TAIL_CASES = ('syn31', 'syn257', 'store4097', 'store8229')
NULL_50X = ('plain/', 'fake/')          # the cases whose null tensors cannot meet 1e-6 of gnorm in f32 (see the module docstring)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


# ---------------------------------------------------------------------------------------------------------------- cases (CPU side)
def heavy_encounter(C, T, H, scale=5.0):
    """One encounter that weighs as much as an encounter of the cohort can: every slot of every channel observed, at evenly spread times,
    every value at the upper end of the cohort's range (+scale/2: far from every phenotype mean, so a large reconstruction residual)."""
    val = np.full(T, scale / 2, np.float32)
    tim = ((np.arange(T) + 0.5) * (H / T)).astype(np.float32)
    one = np.ones(T, np.float32)
    return np.concatenate([np.tile(p, (C, 1)) for p in (val, one, tim, one)], axis=0)


def synthetic_case(B, fake=False, wide=False, heavy_last=False):
    from deep_interpolation_clustering_amd import synthetic
    if wide:
        g = load('netstep_wide_K16.npz')
        state = {k[4:]: v for k, v in g.items() if k.startswith('sd0/')}
        shape = dict(C=12, R=24, H=24.0, K=16)
        coh = synthetic.make_cohort(B, C=12, T=288, H=24.0, lam=200.0, G=16, seed=45)
    else:
        state = {k[5:]: v for k, v in load('traj_cfg1.npz').items() if k.startswith('p1sd/')}
        state['cluster_assignment.cluster_centers'] = load('netstep_cfg_K4.npz')['centers']
        shape = dict(C=6, R=24, H=24.0, K=4)
        coh = synthetic.make_cohort(B, G=4, seed=35)
    x = synthetic.stacked_batch(coh)[0]
    if heavy_last:
        x[-1] = heavy_encounter(shape['C'], x.shape[-1], shape['H'])
    fk = None
    if fake:
        # the pretrained state holds no detection head: one initialised under a fixed seed in the oracle, loaded into the GPU net with the rest
        torch.manual_seed(20)
        ref = O.OracleNet(shape['C'], shape['R'], shape['H'], shape['K'], 0.0, fake_detection=True)
        missing = ref.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=False)
        assert all(k.startswith('fake_det_head.') for k in missing.missing_keys) and not missing.unexpected_keys
        state = {k: v.detach().numpy().copy() for k, v in ref.state_dict().items()}
        C = shape['C']
        fx = x.copy()                    # corrupted samples: the observed values of another encounter at this one's times
        fx[:, :C] = np.where(x[:, C:2 * C] > 0, x[::-1, :C], x[:, :C])
        perm = np.random.default_rng(B).permutation(2 * B)
        fk = {'fake_x': fx, 'fake_perm_idx': perm.astype(np.int64), 'fake_label': np.concatenate([np.ones(B), np.zeros(B)]).astype(np.int64)[perm]}
    return {'state': state, 'x': x, 'ob': np.ascontiguousarray(x[:, :shape['C']]), 'fake': fk, 'shape': shape}


def build_case(name):
    kind, arg, inp = CASES[name]
    c = S.fixture_case(arg, load) if kind == 'fixture' else synthetic_case(**arg)
    c.pop('g', None)
    c['input'] = inp
    return c


def oracle_bundle(name, case):
    """Everything the oracle says about one case, all on the CPU: the f64 gradients and loss terms (the reference); 'floors', compare() of the CPU
    f32 and the CPU bf16-autocast oracle against f64; 'x3', the bars the x3 emulation gives (step_grads.x3_bars); 'tail', for the cases with a
    tile tail, the rel_l2 of the f64 gradients without the last encounter against the reference."""
    ref = dict(fake=case['fake'], **case['shape'])
    t0 = time.time()
    g64, t64 = S.reference_grads(case['state'], case['x'], case['ob'], arithmetic='f64', **ref)
    seconds = time.time() - t0
    g32, _ = S.reference_grads(case['state'], case['x'], case['ob'], arithmetic='f32', **ref)
    gbf, _ = S.reference_grads(case['state'], case['x'], case['ob'], arithmetic='bf16', **ref)
    gn = S.total_norm(g64)
    out = {'g64': g64, 't64': t64, 'f64_seconds': seconds, 'gnorm': gn, 'floors': {'f32': S.compare(g32, g64, gn), 'bf16': S.compare(gbf, g64, gn)},
           'x3': S.x3_bars(case, g64), 'null_50x': name.startswith(NULL_50X)}
    del g32, gbf
    if name in TAIL_CASES:
        cut, _ = S.reference_grads(case['state'], case['x'][:-1], case['ob'][:-1], arithmetic='f64', **ref)
        out['tail'] = {n: v['rel_l2'] for n, v in S.compare(cut, g64, gn)['tensors'].items()}
    out['seconds'] = time.time() - t0
    return out


_BUNDLES = {}


def oracle_for(name):
    """name -> (case, oracle_bundle): computed once per case, shared by the modes."""
    if name not in _BUNDLES:
        case = build_case(name)
        bundle = oracle_bundle(name, case)
        print(f'[step-grads] {name}: oracle side {bundle["seconds"]:.1f} s (f64 forward + backward {bundle["f64_seconds"]:.1f} s)')
        _BUNDLES[name] = (case, bundle)
    return _BUNDLES[name]


@pytest.fixture(scope='module')
def oracle_side():
    return oracle_for


# ---------------------------------------------------------------------------------------------------------------- the GPU side
def gpu_grads(case, mode, use_graphs=False, lr=3e-3, wd=4e-4, steps=1):
    """The gradients ``Stepper.step`` leaves in the flat bucket (name -> float64 CPU tensor), the loss terms, the step's own gradient norm."""
    from deep_interpolation_clustering_amd.clustering_interp import Net
    from deep_interpolation_clustering_amd.ragged import RaggedBatch, RaggedStore
    from deep_interpolation_clustering_amd.step import Stepper
    from deep_interpolation_clustering_amd.utils import pytorch_optimizer
    sh, fake = case['shape'], case['fake']
    C = sh['C']
    args = SimpleNamespace(num_variables=C, num_timestamps=case['x'].shape[-1], ref_points=sh['R'], hours_from_admission=sh['H'], dropout=0.0,
                           aux_tasks={}, fake_detection=fake is not None, triple_margin=0.0, cluster_number=sh['K'],
                           loss='ae_mse_fake_detect_kl' if fake is not None else 'ae_mse_kl', grad_clip=1e9,
                           unsup_aux_tasks={'fake_detection': 1., 'triplet': 1., 'kl': 10.}, aux_pos_weights={})
    dev = torch.device('cuda')
    net = Net(args, dev).to(dev)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in case['state'].items()}, strict=True)
    net.train()
    st = Stepper(net, lambda m: pytorch_optimizer(m, 'Adam', lr, wd), args, autocast_dtype=torch.bfloat16 if mode == 'bf16' else None,
                 precision=None if mode == 'bf16' else mode, use_graphs=use_graphs)
    x = torch.tensor(case['x'], device=dev)
    kw = {}
    if fake is not None:
        kw = dict(fake_x=torch.tensor(fake['fake_x'], device=dev), fake_perm_idx=torch.tensor(fake['fake_perm_idx'], device=dev),
                  fake_det_label=torch.tensor(fake['fake_label'], device=dev))
    store = RaggedStore(case['x'], C, dev) if case['input'] == 'store' else None
    for _ in range(steps):
        if store is not None:
            rb = RaggedBatch(store, torch.arange(x.shape[0], device=dev))
            losses, gnorm, _ = st.step(rb, None, None, **kw)
        else:
            mask = x[:, C:2 * C].contiguous()
            ob = torch.tensor(case['ob'], device=dev)
            losses, gnorm, _ = st.step(x, ob, mask, mask.sum(-1).to(torch.int32) if case['input'] == 'lengths' else None, **kw)
    torch.cuda.synchronize()
    if use_graphs:
        assert len(st._graphs) == 1
    grads = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}
    assert all(p.grad.data_ptr() >= st.flat.grad.data_ptr() and p.grad.data_ptr() < st.flat.grad.data_ptr() + 4 * st.flat.grad.numel()
               for p in net.parameters())                       # what was read IS the bucket the optimiser consumed
    return grads, {k: float(v.detach()) for k, v in losses.items()}, float(gnorm)


def bars(mode, k, bundle):
    """(rel_l2 bar, max_over_max bar) of a live tensor and (|got|/gnorm bar) of a null tensor, per the module docstring."""
    f32, bf = bundle['floors']['f32']['tensors'][k], bundle['floors']['bf16']['tensors'][k]
    if mode == 'bf16':
        return 4 * bf['rel_l2'], None, 4 * bf['got_share']
    rel, mx = max(1e-4, 4 * f32['rel_l2']), 2e-4
    if mode == 'x3' and k in bundle['x3']:
        rel, mx = max(rel, bundle['x3'][k]['rel_l2']), max(mx, bundle['x3'][k]['max_over_max'])
    return rel, mx, (50 * f32['got_share'] if bundle['null_50x'] else 1e-6)


def record(name, mode, cmp, bundle, variant=None, **extra):
    """One JSON line per (case, mode), and one printed line per tensor: the GPU's distance from f64 beside the oracle-side floors and the bars."""
    floors = bundle['floors']
    rec = {'case': name, 'mode': mode, 'variant': variant, 'total': cmp['total'], 'gnorm_f64': cmp['gnorm'],
           'floor_total': {k: floors[k]['total'] for k in ('f32', 'bf16')}, 'f64_seconds': bundle['f64_seconds'], 'oracle_seconds': bundle['seconds'], 'tensors': {}}
    rec.update(extra)
    tag = f'{name} {mode}{"/" + variant if variant else ""}'
    print(f'[step-grads] {tag}: total {cmp["total"]:.2e} (CPU f32 oracle {floors["f32"]["total"]:.2e}, CPU bf16 oracle {floors["bf16"]["total"]:.2e})')
    for k, v in cmp['tensors'].items():
        rel_bar, max_bar, null_bar = bars(mode, k, bundle)
        f32, bf, x3 = floors['f32']['tensors'][k], floors['bf16']['tensors'][k], bundle['x3'].get(k)
        rec['tensors'][k] = {'rel_l2': v['rel_l2'], 'max_over_max': v['max_over_max'], 'share': v['share'], 'got_share': v['got_share'], 'cos': v['cos'],
                             'f32_rel_l2': f32['rel_l2'], 'f32_got_share': f32['got_share'], 'bf16_rel_l2': bf['rel_l2'], 'bf16_got_share': bf['got_share'],
                             'x3_rel_l2': x3['x3_rel_l2'] if x3 else None, 'x3_max_over_max': x3['x3_max_over_max'] if x3 else None,
                             'bar': {'null': null_bar} if v['null'] else {'rel_l2': rel_bar, 'max_over_max': max_bar}}
        if v['null']:
            print(f'[step-grads]   {k:<44s} null: |got|/gnorm {v["got_share"]:.1e} (bar {null_bar:.1e}; CPU f32 {f32["got_share"]:.1e}, CPU bf16 {bf["got_share"]:.1e})')
        else:
            print(f'[step-grads]   {k:<44s} rel_l2 {v["rel_l2"]:.2e} max/max {v["max_over_max"]:.2e} (bars {rel_bar:.1e} / {max_bar or 0:.1e}; CPU f32 {f32["rel_l2"]:.1e}, '
                  f'x3 emulation {x3["x3_rel_l2"] if x3 else 0:.1e}, CPU bf16 {bf["rel_l2"]:.1e})')
    _append(rec)


def _append(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, 'a') as f:
            f.write(json.dumps(rec) + '\n')
    except OSError:
        pass


def misses(mode, cmp, bundle):
    """Every (tensor, figure, value, bar) outside the bars of the module docstring."""
    bad = []
    for k, v in cmp['tensors'].items():
        rel_bar, max_bar, null_bar = bars(mode, k, bundle)
        if v['null']:
            if not v['got_share'] <= null_bar:
                bad.append((k, 'null |got|/gnorm', v['got_share'], null_bar))
            continue
        if not v['rel_l2'] <= rel_bar:
            bad.append((k, 'rel_l2', v['rel_l2'], rel_bar))
        if max_bar is not None and not v['max_over_max'] <= max_bar:
            bad.append((k, 'max_over_max', v['max_over_max'], max_bar))
        if mode == 'bf16' and not v['cos'] >= 0.99:
            bad.append((k, 'cos', v['cos'], 0.99))
    if mode == 'bf16' and not cmp['total'] <= 4 * bundle['floors']['bf16']['total']:
        bad.append(('(all)', 'total', cmp['total'], 4 * bundle['floors']['bf16']['total']))
    return bad


def check(name, mode, oracle_side, variant=None, **kw):
    case, bundle = oracle_side(name)
    g64, t64 = bundle['g64'], bundle['t64']
    got, losses, gnorm = gpu_grads(case, mode, **kw)
    assert set(got) == set(g64) and len(got) >= 26
    cmp = S.compare(got, g64, bundle['gnorm'])
    bad, flips = misses(mode, cmp, bundle), None
    if bad and mode != 'bf16':
        # outside the bars: only a residual that IS the flip gradient of named near-zero ReLU inputs is taken out; the remainder meets the same bars
        fe = S.flip_explained(case, mode, got, g64)
        flips = [(site, i, a, s) for site, i, a, s in fe['elements'] if s > 1e-3]
        print(f'[step-grads] {name} {mode}: outside the bars on {sorted({b[0] for b in bad})}; ReLU inputs near zero (site, index, |a|, fitted share of a flip): {fe["elements"]}')
        bad = misses(mode, S.compare(fe['got'], g64, bundle['gnorm']), bundle) if flips else bad
    record(name, mode, cmp, bundle, variant, gpu_gnorm=gnorm, losses=losses, losses_f64=t64, relu_flips_taken_out=flips)
    assert t64['kl'] > (1e-4 if name.startswith(('plain', 'fake/')) else 0.02)            # real state: no gradient sits near zero
    nulls = {k for k, v in cmp['tensors'].items() if v['null']}
    assert 'rbf.compress_fc.module.model.0.bias' in nulls and nulls <= {'rbf.compress_fc.module.model.0.bias', 'fake_det_head.model.0.bias'}
    assert not bad, '\n'.join(f'{name} {mode}: {k}: {what} {v:.3e} > bar {bar:.3e}' if what != 'cos' else f'{name} {mode}: {k}: cos {v:.5f} < {bar}'
                              for k, what, v, bar in bad)
    np.testing.assert_allclose(gnorm, cmp['gnorm'], rtol=1e-4 if mode != 'bf16' else 4 * bundle['floors']['bf16']['total'] + 1e-3)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_step_gradients_match_f64_oracle(name, mode, oracle_side):
    check(name, mode, oracle_side)


def test_replayed_graph_step_gradients_match_f64_oracle(oracle_side):
    """bf16 with use_graphs=True at B = 257: the second call is a replay of the captured step (lr = 0, so the parameters stay put between the
    two); its gradients meet the eager bf16 bars."""
    check('syn257', 'bf16', oracle_side, variant='graph-replay', use_graphs=True, lr=0.0, wd=0.0, steps=2)


def test_side_stream_step_gradients_match_f64_oracle(oracle_side, monkeypatch):
    """bf16 at B = 8229 with the decoder's weight-gradient kernel on a side stream (the branch must be taken: the side stream is asked for)."""
    from deep_interpolation_clustering_amd import lstm as L
    asked, inner = [], L._side_stream
    monkeypatch.setattr(L, 'DW_SIDE_STREAM', True)
    monkeypatch.setattr(L, '_side_stream', lambda dev: (asked.append(dev), inner(dev))[1])
    check('store8229', 'bf16', oracle_side, variant='dw-side-stream')
    assert len(asked) == 1, asked


@pytest.mark.parametrize('name', TAIL_CASES)
def test_reference_gradient_feels_the_tail_encounter(name, oracle_side):
    """A condition on the REFERENCE alone, which makes "a dropped tail row fails" true rather than hoped for: the f64 gradients of the batch
    without its last encounter (the one in the partial tile) differ from the full batch's by rel_l2 >= 5 x the bar the f32-grade modes are held
    to (>= 5e-4; the larger of the exact and the x3 bar) in the encoder's input weights, the decoder's reverse recurrent
    weights and the reconstruction head's last layer.  Measured (f64, CPU): B = 31: 1.2e-1 / 1.3e-1 / 2.1e-1; 257: 1.3e-2 / 2.9e-2 / 3.7e-2 (the
    cohort's own last encounters); 4097: 4.1e-3 / 3.9e-2 / 1.8e-2 and 8229: 2.1e-3 / 2.0e-2 / 1.0e-2, where the last encounter is
    heavy_encounter() -- the cohort's own last one gives 5.4e-4 / 1.6e-3 / 1.8e-3 at 4097, too close to 5e-4, and half of that at 8229.
    The bf16 mode is held to 4 x the CPU bf16 oracle's distance (1 .. 12 %): 5 x that is more than one encounter moves these gradients at any of
    the four sizes (the ratio felt / bar is 1.7 .. 9 at B = 31, 0.2 .. 1.1 at 257, below 0.3 at the large ones), so in bf16 a dropped tail row is
    caught at B = 31 only -- the ratio is reported (ratio_bf16 in the record), not asserted."""
    _, bundle = oracle_side(name)
    felt = {k: bundle['tail'][k] for k in TAIL_TENSORS}
    need = {k: 5 * max(bars(mode, k, bundle)[0] for mode in ('exact', 'x3')) for k in TAIL_TENSORS}
    ratio_bf16 = {k: felt[k] / bars('bf16', k, bundle)[0] for k in TAIL_TENSORS}
    print(f'[step-grads] {name} tail sensitivity (f64, rel_l2): {felt}; needed {need}; against the bf16 bar: {ratio_bf16}')
    _append({'case': name, 'mode': 'reference', 'variant': 'last-encounter-removed', 'rel_l2': felt, 'needed': need, 'ratio_bf16': ratio_bf16})
    for k in TAIL_TENSORS:
        assert need[k] >= 5e-4 and felt[k] >= need[k], (k, felt[k], need[k])
