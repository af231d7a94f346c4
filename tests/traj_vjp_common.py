"""fp64 reference of the trajectory predictor's vector-Jacobian product, the product glamr_nets_traj_backward computes:
d sum(G * infer_out_local_traj) / d (latent draw, joint rows) through the inference pass of oracle.port.nets.TrajPredVAE on the conditioned
checkpoint of tests/traj_ref_common.py, one sequence at a time, in torch autograd.  `forward` restates the pass with autograd on
(traj_ref_common.predict runs under no_grad), reusing traj_ref_common._run for the cells; a mutation breaks the BACKWARD in one place and
leaves the forward values alone.  The VJP is linear in G, so a scaled upstream gradient is answered by scaling the cached result."""
import numpy as np
import torch

from tests import traj_ref_common as tc
from oracle.port.nets import Gaussian

NZ = 128
PINNED = (0, 1, 9, 10)            # columns of row 0 that are constants (DataDecoder :319-327)

# ---- the sequences ------------------------------------------------------------------------------------------------------------------------
# Candidates (seed, length).  SMALL: the batches of the one-sequence-per-workgroup route (B = 1, 7, 33: prefixes; 7 x 100 rows stay below
# SMALL_ROWS, 33 x 100 are above it with max_len >= 64: the split GEMMs and the fused row kernels); MFMA: the 16-sequence tiles of the
# large-batch route (B = 512, 523: the kept ones repeated cyclically, so every tile mixes lengths 2 ... 33); LONG: 300 steps of recurrence.
# The seeds were chosen on the CPU, by the fp64 reference alone: per length, the first seeds from 300 / 400 / 500 on whose forward keeps every
# ReLU input at least 2e-6 from zero (at 300 frames two sequences in three have one closer than that).
SMALL = [(309, 100), (300, 2), (301, 11), (302, 12), (304, 31), (305, 33), (307, 47), (308, 63), (310, 64), (311, 65), (322, 100), (303, 2),
         (312, 11), (306, 12), (313, 31), (314, 33), (317, 47), (315, 63), (319, 64), (316, 65), (327, 100), (318, 2), (320, 11), (321, 12),
         (323, 31), (325, 33), (326, 47), (330, 63), (336, 64), (331, 65), (332, 100), (328, 2), (324, 11)]
MFMA = [(400, 2), (401, 3), (402, 4), (403, 5), (404, 6), (405, 7), (406, 8), (408, 9), (407, 10), (409, 11), (411, 12), (412, 13), (410, 14),
        (414, 15), (413, 16), (415, 17), (416, 18), (418, 19), (419, 20), (417, 21), (420, 22), (423, 23), (421, 24), (422, 25), (425, 26),
        (426, 27), (430, 28), (431, 29), (428, 30), (427, 31), (429, 32), (432, 33)]
LONG = [(644, 300), (701, 300)]
CANDIDATES = SMALL + MFMA + LONG
# A sequence whose fp64 forward has a ReLU input within KINK of zero has no fp32-stable VJP (the VJP jumps at the kink) and is left out of
# the sweep: tests/test_traj_vjp_ref.py checks that this list is what the margins say and that it is at most a quarter of the candidates.
KINK = 1e-6
KINKED = []
MAX_LEFT_OUT = len(CANDIDATES) // 4


def kept(seqs):
    return [s for s in seqs if s not in KINKED]


def batch(route, B):
    """The (seed, length) of every slot: 'small' | 'mfma' | 'long', kept sequences repeated cyclically."""
    seqs = kept({'small': SMALL, 'mfma': MFMA, 'long': LONG}[route])
    return [seqs[i % len(seqs)] for i in range(B)]


# ---- upstream gradients -------------------------------------------------------------------------------------------------------------------
PATTERNS = ('dense', 'last', 'pinned')


def upstream(seed, T, pattern):
    """G (T,11) fp32.  dense: random; last: one column (the height, 2) of the LAST frame only -- the gradient reaches frame 0 through the
    backward direction and the last frame through the forward one; pinned: only the four constant entries of row 0 (every gradient is zero)."""
    G = np.zeros((T, 11), np.float32)
    if pattern == 'dense':
        G[:] = np.random.default_rng(7000 + 13 * seed + T).normal(size=(T, 11))
    elif pattern == 'last':
        G[T - 1, 2] = 1.0
    else:
        G[0, list(PINNED)] = (1.0, -2.0, 3.0, 0.5)
    return G


# ---- the forward with autograd on, with room for a mutation of the backward -----------------------------------------------------------------
MUTATIONS = ('a', 'b', 'c', 'd', 'e')
MUTATION_NAMES = {'a': 'dc_prev = dc f dropped', 'b': 'backward of layer 2 with the two directions\' weights swapped', 'c': 'no path through the prior',
                  'd': 'mean backward divided by max_len', 'e': 'no ReLU mask in in_mlp'}


def _graft(value, grad_of):
    """`value`'s numbers with `grad_of`'s gradient."""
    return value.detach() + (grad_of - grad_of.detach())


def _run_no_dc(cell, x, reverse):
    """traj_ref_common._run with the cell state's own path cut in the backward (mutation 'a')."""
    h = torch.zeros((x.size(1), cell.hidden_size), dtype=x.dtype)
    c = torch.zeros_like(h)
    out = [None] * x.size(0)
    for t in (range(x.size(0) - 1, -1, -1) if reverse else range(x.size(0))):
        g = x[t] @ cell.weight_ih.T + cell.bias_ih + cell.bias_hh + h @ cell.weight_hh.T
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c.detach() + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out, 0)


def forward(net, joints, eps, mut=None, max_len=None, margins=None):
    """local_traj (T,B,11) of inference mode for joints (T,B,69) and eps (B,128), tensors of the net's dtype (either may require grad).
    `margins` (a list) receives the smallest |input| of every ReLU."""
    T = joints.shape[0]

    def mlp(m, x, mask=True):
        for lin in m.affine_layers:
            a = lin(x)
            if margins is not None:
                margins.append(float(a.detach().abs().min()))
            x = torch.relu(a) if mask else _graft(torch.relu(a), a)
        return x
    ce, dd = net.context_encoder, net.data_decoder
    run = (lambda cell, x, rev: _run_no_dc(cell, x, rev)) if mut == 'a' else (lambda cell, x, rev: tc._run(cell, x, rev, None))
    h = mlp(ce.in_mlp, joints, mask=mut != 'e')
    for l, bl in enumerate(ce.temporal_net):
        out = torch.cat([run(bl.rnn_f, h, False), run(bl.rnn_b, h, True)], dim=2)
        if mut == 'b' and l == 1:
            out = _graft(out, torch.cat([run(bl.rnn_b, h, False), run(bl.rnn_f, h, True)], dim=2))
        h = out
    ctx = mlp(ce.out_mlp, h)
    cm = ctx.mean(dim=0)
    if mut == 'd':
        cm = _graft(cm, ctx.sum(dim=0) / max_len)
    params = dd.p_z_net(mlp(dd.prior_mlp, cm))
    prior = Gaussian(params=params.detach() if mut == 'c' else params)
    z = prior.sample(eps)
    raw = dd.out_fc(mlp(dd.out_mlp, torch.cat([z.repeat((T, 1, 1)), ctx], dim=-1)))
    loc = raw.clone()
    loc[0, :, :2] = 0.0
    loc[0, :, -2:] = torch.tensor([0., 1.], dtype=raw.dtype)
    return loc


def vjp(net, joints32, eps32, Gs, mut=None, max_len=None, margins=None):
    """One sequence: joints32 (T,69) / eps32 (128,) fp32 arrays, Gs a list of (T,11) upstream gradients.  Returns local_traj (T,11) and, per G,
    (g_eps (128,), g_joint_pos (T,69)) for L = sum(G * local_traj), numpy fp64, computed in the dtype of `net`."""
    dt = next(net.parameters()).dtype
    j = torch.tensor(np.asarray(joints32), dtype=dt)[:, None].requires_grad_(True)
    e = torch.tensor(np.asarray(eps32), dtype=dt)[None].requires_grad_(True)
    loc = forward(net, j, e, mut, max_len, margins)
    out = []
    for G in Gs:
        ge, gj = torch.autograd.grad((loc[:, 0] * torch.tensor(np.asarray(G), dtype=dt)).sum(), (e, j), retain_graph=True)
        out.append((ge[0].double().numpy(), gj[:, 0].double().numpy()))
    return loc[:, 0].detach().double().numpy(), out


class Reference:
    """Cached VJPs of the port in `dtype`, one entry per (seed, length, mutation, max_len): local_traj and the products for the dense and
    the last-frame upstream gradients (the pinned pattern's are exactly zero: checked in tests/test_traj_vjp_ref.py)."""

    def __init__(self, asset_root, dtype=torch.float64, base=None):
        self.net = tc.predictor(asset_root, dtype)
        self.base = base or self               # the fp64 reference whose forward kinematics feeds every dtype the same fp32 joint rows
        self.cache, self.margins, self._joints = {}, {}, {}

    def inputs(self, seed, T):
        """(joint rows (T,69), latent draw (128,)) fp32: what the device is given."""
        if self.base is not self:
            return self.base.inputs(seed, T)
        if (seed, T) not in self._joints:
            pose, eps = tc.seq_inputs(seed, T)
            self._joints[(seed, T)] = (tc.joints_of(self.net, pose).numpy().astype(np.float32), np.asarray(eps, np.float32))
        return self._joints[(seed, T)]

    def __call__(self, seed, T, mut=None, max_len=None):
        """dict: local_traj (T,11), and per pattern 'dense' / 'last' the pair (g_eps, g_joint_pos)."""
        k = (seed, T, mut, max_len if mut == 'd' else None)
        if k not in self.cache:
            j, e = self.inputs(seed, T)
            m = []
            loc, g = vjp(self.net, j, e, [upstream(seed, T, p) for p in ('dense', 'last')], mut, max_len, m)
            self.cache[k] = {'local_traj': loc, 'dense': g[0], 'last': g[1]}
            if mut is None:
                self.margins[(seed, T)] = min(m)
        return self.cache[k]

    def margin(self, seed, T):
        self(seed, T)
        return self.margins[(seed, T)]


def rel_err(got, ref):
    """max |got - ref| / max |ref| (ref all zero: max |got|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------
# The project's rule (traj_ref_common.FLOOR_FACTOR = 16): the device bound per output is 16 x the largest error of the same autograd in fp32
# on one thread against fp64, over every kept candidate and the dense and last-frame upstream gradients, each error relative to the
# sequence's largest reference entry.  Measured floors, rounded up to two digits, the measured figure beside each;
# tests/test_traj_vjp_ref.py derives them again and fails if they have drifted by more than 2 x.
FLOOR = {'g_eps': 5.9e-7,          # 5.810e-7
         'g_joint_pos': 5.5e-4}    # 5.455e-4 (the recurrences of the conditioned checkpoint amplify the fp32 forward's rounding of their states)
TOL = {k: tc.FLOOR_FACTOR * v for k, v in FLOOR.items()}


def floors(r32, r64, seqs=None):
    acc = {'g_eps': 0.0, 'g_joint_pos': 0.0}
    with tc.single_thread():
        for seed, T in (kept(CANDIDATES) if seqs is None else seqs):
            a, b = r32(seed, T), r64(seed, T)
            for p in ('dense', 'last'):
                acc['g_eps'] = max(acc['g_eps'], rel_err(a[p][0], b[p][0]))
                acc['g_joint_pos'] = max(acc['g_joint_pos'], rel_err(a[p][1], b[p][1]))
    return acc


if __name__ == '__main__':          # the margins and the floors on this machine's CPU build of torch
    import os
    import tempfile
    from oracle.port import build
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    r64 = Reference(root)
    r32 = Reference(root, torch.float32, base=r64)
    m = {s: r64.margin(*s) for s in CANDIDATES}
    print('kinked (margin < %.0e): %s' % (KINK, [s for s in CANDIDATES if m[s] < KINK]))
    print('smallest kept margin %.2e' % min(v for v in m.values() if v >= KINK))
    print('floors: %s' % ', '.join('%s=%.3e' % kv for kv in sorted(floors(r32, r64, [s for s in CANDIDATES if m[s] >= KINK]).items())))
