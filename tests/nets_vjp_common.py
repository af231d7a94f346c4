"""fp64 reference of the infiller's vector-Jacobian product, the product glamr_nets_infill_backward computes for the latent-optimisation
mode: d sum(G * infer_out_body_pose) / d in_motion_latent through oracle.port.nets.MotionInfillerVAE.inference(multi_step=True), one
sequence at a time, in torch autograd.  The VJP is linear in G, so a scaled upstream gradient is answered by scaling the cached result."""
import os
import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build
from oracle.port.nets import MotionInfillerVAE

PAST, CUR = 10, 30


def n_windows(T):
    return int(np.ceil((T - PAST) / CUR))


def infiller(asset_root, dtype=torch.float64):
    """The CPU port of the motion infiller with the synthetic checkpoint's weights, converted to `dtype`."""
    sd = torch.load(build._ckpt(asset_root, os.path.join('motion_filler', 'motion_infiller_demo')), map_location='cpu', weights_only=False)['state_dict']
    net = MotionInfillerVAE()
    net.load_state_dict({k: v for k, v in sd.items() if not k.startswith('smpl.')}, strict=True)
    return net.to(dtype).eval()


# Sequences (seed, length) of the route sweep of tests/test_nets_vjp_gpu.py; every batch there is a prefix of this list.  Lengths 11 ... 150;
# seeds whose fp64 forward pass has a ReLU input within KINK of zero are left out (tests/test_nets_vjp_ref.py checks): the VJP jumps at a
# ReLU's kink, and an fp32 forward that lands on the other side of one moves the VJP of the whole sequence (seed 49 at length 73 has a ReLU
# input of 1.5e-7 that the batch-69 forward put on the other side; flipping that ReLU alone moves its VJP by 1.9e-3 of its largest entry).
KINK = 1e-6
ROUTE_SEEDS = [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 23, 24, 25, 26, 30, 31, 32, 33, 34, 35, 36, 38, 39, 40, 41,
               42, 43, 49, 50, 52, 53, 54, 55, 60, 65, 66, 68, 69, 73, 75, 76, 78, 80, 81, 82, 83, 84, 86, 87, 89, 90, 91, 94, 95, 97, 98, 99, 100,
               102]
ROUTE_SEQS = [(seed, 150 - (i * 53) % 140) for i, seed in enumerate(ROUTE_SEEDS)]

# the linear layers whose outputs go through a ReLU (feed-forward blocks of the transformer layers, the decoder's output MLP)
RELU_INPUTS = ('.linear1', '.affine_layers.')


def vjp(net, inp, G, margins=None):
    """(pose (T,69), dL/d latent (n_win,128)) of one sequence for L = sum(G * infer_out_body_pose), in the dtype of `net`.
    `inp`: mg.net_inputs(T, seed); G: (T,69).  `margins` (a list) receives the smallest |input| of every ReLU call: the VJP jumps where one
    crosses zero, so a sequence with an input within rounding reach of the kink has no fp32-stable VJP to compare with."""
    hooks = [] if margins is None else [m.register_forward_hook(lambda mod, i, o: margins.append(float(o.detach().abs().min())))
                                        for n, m in net.named_modules() if isinstance(m, torch.nn.Linear) and any(k in n for k in RELU_INPUTS)]
    try:
        return _vjp(net, inp, G)
    finally:
        for h in hooks:
            h.remove()


def _vjp(net, inp, G):
    dt = next(net.parameters()).dtype
    lat = torch.tensor(inp['in_motion_latent'], dtype=dt).requires_grad_(True)
    d = net.inference({'in_body_pose': torch.tensor(inp['in_body_pose'], dtype=dt), 'frame_mask': torch.tensor(inp['frame_mask']),
                       'in_motion_latent': lat}, sample_num=1, multi_step=True)
    pose = d['infer_out_body_pose'][0, 0]
    (pose * torch.as_tensor(np.asarray(G), dtype=dt)).sum().backward()
    return pose.detach().numpy(), lat.grad.numpy()


class Reference:
    """Cached fp64 VJPs keyed by (seed, length, name of the upstream-gradient pattern), and the ReLU margin of each sequence."""

    def __init__(self, asset_root):
        self.net = infiller(asset_root)
        self.cache = {}
        self.margins = {}

    def __call__(self, seed, T, key, G):
        k = (seed, T, key)
        if k not in self.cache:
            m = []
            self.cache[k] = vjp(self.net, mg.net_inputs(T, seed), G, m)
            self.margins[(seed, T)] = min(m)
        return self.cache[k]

    def margin(self, seed, T):
        """Smallest |ReLU input| of the sequence's forward pass (zero padding and masked frames included)."""
        if (seed, T) not in self.margins:
            self(seed, T, 'W', mg.latent_loss_weights(T, seed))
        return self.margins[(seed, T)]


def rel_err(got, ref):
    """max |got - ref| / max |ref| (ref all zero: max |got|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))
