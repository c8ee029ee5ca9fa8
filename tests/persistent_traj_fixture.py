"""Writes tests/golden/persistent_traj.json: what ONE joint bf16 step at B = 16 454, R = 24 leaves behind (loss, gradient norm, f64 sum of all parameters after
the update).  Run it on the GPU from the root of a checkout of the commit whose numbers are to be pinned, with that checkout's library built:
    python tests/persistent_traj_fixture.py [out.json]
tests/test_gpu_lstm_persistent.py calls one_step() on the current tree and compares exactly."""
import json
import os
import sys
from types import SimpleNamespace

import torch

B = 2 * 128 * 64 + 70       # 16 454: five or four 32-row tiles per workgroup on 256 CUs, a ragged last tile


def one_step():
    from deep_interpolation_clustering_amd import synthetic
    from deep_interpolation_clustering_amd.clustering_interp import Net
    from deep_interpolation_clustering_amd.step import Stepper
    from deep_interpolation_clustering_amd.utils import pytorch_optimizer
    dev = torch.device('cuda', 0)
    coh = synthetic.make_cohort(B, C=6, T=96, H=24.0, lam=50.0, G=4, seed=11)
    x_np, ob_np, n = synthetic.stacked_batch(coh)
    args = SimpleNamespace(num_variables=6, num_timestamps=96, ref_points=24, hours_from_admission=24, dropout=0.0, aux_tasks={}, fake_detection=False,
                           triple_margin=0.0, cluster_number=4, loss='ae_mse_kl', grad_clip=15.0, unsup_aux_tasks={'fake_detection': 1., 'triplet': 1., 'kl': 10.},
                           aux_pos_weights={})
    torch.manual_seed(1234)
    net = Net(args, dev).to(dev)
    net.train()
    st = Stepper(net, lambda m: pytorch_optimizer(m, 'Adam', 3e-3, 4e-4), args, autocast_dtype=torch.bfloat16, use_graphs=False)
    losses, gnorm, _ = st.step(torch.tensor(x_np).to(dev), torch.tensor(ob_np).to(dev), None, torch.tensor(n, device=dev))
    torch.cuda.synchronize()
    psum = sum(float(p.detach().double().sum()) for p in net.parameters())
    return {'loss': float(losses['loss'].detach()), 'gnorm': float(gnorm), 'param_sum': psum}


if __name__ == '__main__':
    sys.path.insert(0, os.getcwd())
    res = one_step()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join('tests', 'golden', 'persistent_traj.json')
    with open(out, 'w') as f:
        json.dump(res, f)
        f.write('\n')
    print(res)
