"""fp64 reference of the chain MotionTrajJointModel.inference_grad exposes: the port's infiller -> body pose -> forward kinematics -> trajectory
predictor -> local-to-global -> SMPL joints, L = sum(W * joints), differentiated with respect to both latents by torch autograd in the dtype
of the priors and of the body model (cast the way tests/attach_common.py casts them).  One sequence at a time: the port's inference has no
padding, a batch of the device test is its sequences side by side.

Tolerance = 16 x the deviation of the fp32 run of the SAME port from its fp64 run, per latent, relative to the sequence's largest reference
entry (tests/test_global_vjp_ref.py measures the floors again within [1/2, 2] x the constants).  The input seeds are chosen on the CPU so that
no ReLU pre-activation of either prior lies within KINK of zero in the fp64 forward: the VJP jumps at a kink, and an fp32 forward that lands
on its other side has another VJP.

The fp64 gradients are kept in tests/golden/global_vjp_chain.npz, written by `python -m tests.global_vjp_chain` (numbers only); the CPU suite
runs the port again and holds the file to it."""
import copy
import os

import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build
from tests.nets_vjp_common import RELU_INPUTS

FLOOR_FACTOR = 16
KINK = 1e-6
# name: ((seed of mg.net_inputs, frames), ...).  70 frames = two infiller windows (the autoregression is live).  The seeds were searched on the CPU
# (0 ... 79 per length, in order): the first whose fp64 forward keeps every ReLU pre-activation of both priors at least 2 x KINK from zero
# (margins 2.04e-6, 2.63e-6 and 2.06e-6); tests/test_global_vjp_ref.py checks the margins again.
CHAIN = {'one': ((23, 70),),
         'two': ((74, 70), (13, 45))}
FIXTURE = 'global_vjp_chain'


def sequences(name):
    """[(seed, frames)] of the case."""
    return list(CHAIN[name])


def betas(name, b):
    return (0.5 * np.random.default_rng(600 + 7 * len(name) + b).normal(size=10)).astype(np.float32)


def weights(name, b, n, J):
    return np.random.default_rng(700 + 7 * len(name) + b).normal(size=(n, J, 3)).astype(np.float32)


_MODELS = {}


def models(asset_root, dtype):
    """(body model, joint model of the two priors) of the port in `dtype`."""
    if dtype not in _MODELS:
        smpl = build.load_smpl(asset_root).to(dtype)
        mt = build.load_joint_model(asset_root, copy.deepcopy(smpl))
        mt.mfiller.to(dtype), mt.traj_predictor.to(dtype)
        _MODELS[dtype] = (smpl, mt)
    return _MODELS[dtype]


def vjp(asset_root, name, b, seed, dtype=torch.float64, margins=None):
    """(d L / d in_motion_latent (windows, 128), d L / d in_traj_latent (128,)) of sequence b of the case with input seed `seed`, fp64 numbers.
    `margins` (a list) receives the smallest |ReLU pre-activation| of every ReLU call of both priors."""
    n = CHAIN[name][b][1]
    smpl, mt = models(asset_root, dtype)
    x = mg.net_inputs(n, seed)
    hooks = [] if margins is None else [m.register_forward_hook(lambda mod, i, o: margins.append(float(o.detach().abs().min())))
                                        for net in (mt.mfiller, mt.traj_predictor) for k, m in net.named_modules()
                                        if isinstance(m, torch.nn.Linear) and any(r in k for r in RELU_INPUTS)]
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(dtype)
        me = torch.tensor(x['in_motion_latent'], dtype=dtype).requires_grad_(True)
        te = torch.tensor(x['in_traj_latent'], dtype=dtype).requires_grad_(True)
        d = mt.inference({'in_body_pose': torch.tensor(x['in_body_pose'], dtype=dtype), 'frame_mask': torch.tensor(x['frame_mask']),
                          'in_motion_latent': me, 'in_traj_latent': te}, sample_num=1)
        j = smpl(global_orient=d['infer_out_orient'][0, 0], body_pose=d['infer_out_body_pose'][0, 0], betas=torch.tensor(betas(name, b), dtype=dtype)[None].expand(n, -1),
                 root_trans=d['infer_out_trans'][0, 0]).joints
        loss = (j * torch.tensor(weights(name, b, n, j.shape[1]), dtype=dtype)).sum()
        g_m, g_t = torch.autograd.grad(loss, (me, te))
        return g_m.double().numpy(), g_t.double().numpy().reshape(-1)
    finally:
        torch.set_default_dtype(old)
        for h in hooks:
            h.remove()


_REF, _MARGIN = {}, {}


def relu_margin(asset_root, name, b, seed):
    """Smallest |ReLU pre-activation| of both priors in the fp64 forward of the sequence (kept from the reference run when that is the seed's)."""
    if (name, b, seed) not in _MARGIN:
        m = []
        vjp(asset_root, name, b, seed, margins=m)
        _MARGIN[(name, b, seed)] = min(m)
    return _MARGIN[(name, b, seed)]


def reference(asset_root, name):
    """{'<name>_s<b>_g_motion' / '_g_traj': fp64 array} of the case's kept sequences.  Cached."""
    if name not in _REF:
        out = {}
        for b, (seed, n) in enumerate(sequences(name)):
            m = []
            out['%s_s%d_g_motion' % (name, b)], out['%s_s%d_g_traj' % (name, b)] = vjp(asset_root, name, b, seed, margins=m)
            _MARGIN[(name, b, seed)] = min(m)
        _REF[name] = out
    return _REF[name]


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


def measure_floor(asset_root, name):
    """The fp32 run of the port against its fp64 run (one thread), worst over the case's sequences."""
    from tests.traj_ref_common import single_thread
    ref = reference(asset_root, name)
    acc = {'g_motion': 0.0, 'g_traj': 0.0}
    with single_thread():
        for b, (seed, n) in enumerate(sequences(name)):
            g_m, g_t = vjp(asset_root, name, b, seed, torch.float32)
            acc['g_motion'] = max(acc['g_motion'], rel_err(g_m, ref['%s_s%d_g_motion' % (name, b)]))
            acc['g_traj'] = max(acc['g_traj'], rel_err(g_t, ref['%s_s%d_g_traj' % (name, b)]))
    return acc


# fp32 port against fp64 port (one thread), rounded up to two digits; tests/test_global_vjp_ref.py measures them again
FLOOR = {'one': {'g_motion': 7.8e-7, 'g_traj': 1.9e-7},        # 7.425e-7, 1.771e-7
         'two': {'g_motion': 5.0e-7, 'g_traj': 3.1e-7}}        # 4.732e-7, 2.908e-7


def tol(name):
    return {k: FLOOR_FACTOR * v for k, v in FLOOR[name].items()}


def fixture_arrays(asset_root):
    out = {}
    for name in CHAIN:
        out.update(reference(asset_root, name))
    return out


if __name__ == '__main__':
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    for name in CHAIN:
        for b, (seed, n) in enumerate(sequences(name)):
            print('%s sequence %d (seed %d, %d frames): smallest |ReLU pre-activation| %.2e' % (name, b, seed, n, relu_margin(root, name, b, seed)))
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', FIXTURE + '.npz'), **fixture_arrays(root))
    for name in CHAIN:
        print("    '%s': {%s}," % (name, ', '.join("'%s': %.3e" % kv for kv in measure_floor(root, name).items())))
