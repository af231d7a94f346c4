"""fp64 reference of the trajectory predictor (oracle.port.nets.TrajPredVAE in .double(), no default-dtype switch) on a checkpoint that makes
its output depend on its input, the sweep of distinct sequences the device tests run, the mutations that show those tests can fail, and the
tolerances, each derived from the rounding of the fp32 CPU port against the fp64 one.

Why a second checkpoint: glamr_amd/utils/synth.py draws every weight as U(+-1/sqrt(fan_in)), every layer has gain below one and by the output
the pose-dependent part of the signal is ~2e-5 -- under the 1e-4 the fixture tests hold the predictor to.  conditioned_state_dict() scales the
layers UPSTREAM of the recurrences (free for the range analysis of glamr_nets_create: LSTM states are bounded by 1) until the layer-2 states
saturate; the same mutation then moves the output three to four orders of magnitude further while the fp32 rounding floor stays where it was.

`predict` restates the forward of the three sub-modules so that a mutation can be placed inside it; tests/test_traj_ref.py pins the
unmutated restatement to the port's own inference() / forward() bit for bit."""
import os
import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build
from oracle.port import transforms as tf
from oracle.port.nets import TrajPredVAE, Gaussian

NZ = 128

# ---- the conditioned checkpoint ---------------------------------------------------------------------------------------------------------
# gain per parameter-name prefix (weights and biases alike).  Context encoder: 6 on both in_mlp layers and on the four LSTM cells (weight_ih,
# weight_hh, biases): |h| of layer 2 ~ 1.  Posterior encoder: the same on its LSTM cells; its in_mlp sees heading-frame translations the range
# analysis takes up to 200 m, so its in_mlp has less room: 6 on its first layer alone already puts the bound at 3.2e4 > 3e4 and would tip the
# handle into fp32-only mode; 4 gives 2.1e4.  Downstream (out_mlp, prior, fusion, decoder) untouched: t_dctx -> t_d2 is at 1.6e4, half the
# limit, with the default weights.  (More is not better: 10 on the cells makes the recurrence chaotic -- the fp32 port then differs from the
# fp64 port by 2e-2 and there is nothing left to compare with.)
GAINS = (('context_encoder.in_mlp.', 6.0), ('context_encoder.temporal_net.', 6.0),
         ('data_encoder.in_mlp.affine_layers.0.', 4.0), ('data_encoder.temporal_net.', 6.0))
FP16_LIMIT = 3.0e4


def conditioned_state_dict(sd):
    """The synthetic trajectory-predictor state dict with the per-layer gains of GAINS (a copy; smpl.* keys dropped)."""
    out = {}
    for k, v in sd.items():
        if k.startswith('smpl.'):
            continue
        g = 1.0
        for prefix, gain in GAINS:
            if k.startswith(prefix):
                g = gain
        out[k] = v.detach().clone() * g
    return out


def range_bound(sd):
    """The trajectory-predictor part of glamr_nets_create's range analysis, restated: (worst converted activation, largest weight).  Both must
    stay below FP16_LIMIT for the handle to keep the fp16-split kernels.  It mirrors the trajectory-predictor lines of the bound that
    glamr_nets_create computes in glamr_amd/csrc/nets.hip (described at glamr_nets_precision in include/glamr_hip.h: joints <= 4 m,
    translations <= 200 m, |z| <= 100, LSTM states <= 1) and has to follow them; it exists so that a change of GAINS is judged without a device, the device fixture
    asserts glamr_nets_precision == 0 on the real analysis."""
    W = lambda k: sd[k + '.weight'].double().abs()
    rowabs = lambda k, c0=None, c1=None: float(W(k)[:, c0:c1].sum(1).max())
    babs = lambda k: float(sd[k + '.bias'].double().abs().max())
    worst = [0.0]

    def see(b):
        worst[0] = max(worst[0], b)
        return b

    def mlp(name, x):
        hd = see(rowabs(name + '.affine_layers.0') * see(x) + babs(name + '.affine_layers.0'))
        return see(rowabs(name + '.affine_layers.1') * hd + babs(name + '.affine_layers.1'))
    JOINTS, TRANS, ZMAX = 4.0, 200.0, 100.0
    mlp('context_encoder.in_mlp', JOINTS)
    tctx = mlp('context_encoder.out_mlp', 1.0)
    mlp('data_decoder.prior_mlp', tctx)
    d0 = 'data_decoder.out_mlp.affine_layers.0'
    dh = see(rowabs(d0, NZ, None) * tctx + rowabs(d0, 0, NZ) * ZMAX + babs(d0))
    see(rowabs('data_decoder.out_mlp.affine_layers.1') * dh + babs('data_decoder.out_mlp.affine_layers.1'))
    mlp('data_encoder.in_mlp', TRANS)
    te = mlp('data_encoder.out_mlp', 1.0)
    mlp('data_encoder.fusion_mlp', max(te, tctx))
    wmax = max(float(v.abs().max()) for k, v in sd.items() if k.endswith('weight') or k.endswith('weight_ih') or k.endswith('weight_hh'))
    return worst[0], wmax


def load_state_dict(asset_root, conditioned=True):
    sd = torch.load(build._ckpt(asset_root, os.path.join('traj_pred', 'traj_pred_demo')), map_location='cpu', weights_only=False)['state_dict']
    sd = {k: v for k, v in sd.items() if not k.startswith('smpl.')}
    return conditioned_state_dict(sd) if conditioned else sd


def predictor(asset_root, dtype=torch.float64, conditioned=True):
    """The CPU port of the trajectory predictor (with its SMPL) in `dtype`."""
    net = TrajPredVAE(smpl=build.load_smpl(asset_root).to(dtype))
    net.load_state_dict(load_state_dict(asset_root, conditioned), strict=True)
    return net.to(dtype).eval()


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
# 48 distinct (seed, length) pairs of mg.net_inputs.  Three blocks of 16; every block holds the shortest and the longest lengths, so every
# group of 16 consecutive slots of a cyclic tiling (the 16 sequences one lstm_mfma_kernel workgroup steps together) is as ragged as can be.
_LENS = [11, 300, 31, 255, 64, 100, 12, 299, 33, 257, 63, 150, 47, 200, 65, 128,
         12, 299, 32, 256, 65, 101, 11, 300, 20, 270, 63, 127, 80, 220, 97, 180,
         13, 298, 33, 257, 64, 129, 15, 300, 31, 240, 48, 160, 90, 210, 16, 289]
SWEEP = [(200 + i, n) for i, n in enumerate(_LENS)]


def tiling(B, max_len=None):
    """B slots: the sweep (only its sequences of at most max_len frames, if given) repeated cyclically."""
    seqs = [s for s in SWEEP if max_len is None or s[1] <= max_len]
    return [seqs[i % len(seqs)] for i in range(B)]


# the batches of glamr_nets_infer(traj only) the device tests run, as (B, longest length allowed or None), and the outputs that call returns --
# the only ones a fault confined to a large-batch route can be seen in (p_z, z and the raw rows come from glamr_nets_traj_clip, whose
# sequences all have the length of the batch)
ROUTE_BATCHES = [(1, None), (7, None), (40, 63), (33, 64), (511, None), (512, None), (523, None)]
ROUTE_KEYS = ('local_traj', 'trans', 'rot')
MFMA_BATCH, MFMA_GROUP = 512, 16          # lstm_mfma_kernel from 512 sequences on, 16 sequences per workgroup


def route_seqs(B, max_len=None):
    return tiling(B, max_len) if B > 1 else [SWEEP[1]]          # alone: a 300-frame sequence (300 rows, the small-batch kernels)


def _t(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt)


def seq_inputs(seed, T):
    """(body pose (T,69) fp32, latent draw (128,) fp32) of one sweep sequence."""
    inp = mg.net_inputs(T, seed)
    return inp['in_body_pose'][0], inp['in_traj_latent'][0]


def clip_inputs(i, T):
    """Sequence i of the traj_clip batches: body pose (T,69), latent draw (128,), ground-truth root translation and orientation (T,3) each
    (fp32).  A walk with its own speed, a root near the z-up convention that turns at its own rate (up to 1.5 rad/s either way: the heading
    passes +-pi within 300 frames)."""
    pose, eps = seq_inputs(1000 + i, T)
    rng = np.random.default_rng(31337 + i)
    t = np.arange(T)[:, None] / 30.0
    orient = 0.3 * np.sin(2 * np.pi * rng.uniform(0.2, 0.8, size=(1, 3)) * t + rng.uniform(0, 6.28, size=(1, 3)))
    orient[:, 0] += np.pi / 2
    orient[:, 2] += rng.uniform(-1.5, 1.5) * t[:, 0]
    v = rng.uniform(0.3, 1.4)
    trans = np.concatenate([0.8 * np.sin(0.7 * t + rng.uniform(0, 3)), v * t + 0.1 * np.cos(1.3 * t), 0.9 + 0.03 * np.sin(5 * t + rng.uniform(0, 3))], axis=1)
    return pose, eps, trans.astype(np.float32), orient.astype(np.float32)


# ---- the forward, with room for a mutation ----------------------------------------------------------------------------------------------
MUTATIONS = ('a', 'b', 'c', 'd', 'e')
MUTATION_NAMES = {'a': 'weight_hh x 1.01', 'b': 'forward and backward cells of layer 2 swapped', 'c': 'no recurrent term at the last step of the backward direction',
                  'd': "the neighbour's joint rows for one frame", 'e': 'context mean over max_len instead of the own length'}


def _cell(cell, x, h, c, whh_scale, skip_rec):
    if whh_scale == 1.0 and not skip_rec:
        return cell(x, (h, c))
    g = x @ cell.weight_ih.T + cell.bias_ih + cell.bias_hh
    if not skip_rec:
        g = g + h @ (cell.weight_hh * whh_scale).T
    i, f, gg, o = g.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _run(cell, x, reverse, mut):
    h = torch.zeros((x.size(1), cell.hidden_size), dtype=x.dtype)
    c = torch.zeros_like(h)
    out = [None] * x.size(0)
    order = list(range(x.size(0) - 1, -1, -1) if reverse else range(x.size(0)))
    for t in order:
        h, c = _cell(cell, x[t], h, c, 1.01 if mut == 'a' else 1.0, mut == 'c' and reverse and t == order[-1])
        out[t] = h
    return torch.stack(out, 0)


def joints_of(net, pose):
    """Root-relative joint rows (..., 69) of body poses (..., 69) by the port's forward kinematics, in the net's dtype."""
    dt = next(net.parameters()).dtype
    with torch.no_grad():
        return net.get_joint_pos(_t(pose, dt))


def predict(net, joints, eps=None, mode='infer', trans=None, orient=None, mut=None, max_len=None, neighbour=None):
    """One forward of the predictor in the dtype of `net`.  joints (T,B,69) tensor; eps (B,128) for infer / train; trans / orient (T,B,3) for
    train / recon (optional for infer: they pin the first row, as in the port).  `mut`: one of MUTATIONS, applied to the context encoder
    ('a'-'c'), to its input ('d': frame T // 2 replaced by `neighbour`'s (T',69) row of the same index, its last if it is shorter) or to the
    prior's temporal mean ('e': divided by `max_len`).  Returns numpy fp64 arrays, batch-major: raw, local_traj (B,T,11), trans (B,T,3),
    orient (axis-angle), quat (B,T,4), p_z (B,256), z (B,128) [, q_z (B,256), g2l (B,T,11)]."""
    dt = next(net.parameters()).dtype
    T, B = joints.shape[:2]
    with torch.no_grad():
        x = joints.to(dt)
        if mut == 'd':
            x = x.clone()
            x[T // 2, 0] = neighbour[min(T // 2, neighbour.shape[0] - 1)].to(dt)
        data = {'in_joint_pos_tp': x, 'batch_size': B, 'seq_len': T}
        ce = net.context_encoder
        h = ce.in_mlp(x)
        for l, bl in enumerate(ce.temporal_net):
            f, b = (bl.rnn_b, bl.rnn_f) if (mut == 'b' and l == 1) else (bl.rnn_f, bl.rnn_b)
            h = torch.cat([_run(f, h, False, mut), _run(b, h, True, mut)], dim=2)
        ctx = data['context'] = ce.out_mlp(h)
        out = {}
        if trans is not None:
            data['trans_tp'] = _t(trans, dt)
            data['orient_q_tp'] = tf.aa_to_quat(_t(orient, dt))
            data['local_traj_tp'] = tf.global_to_local_traj(data['trans_tp'], data['orient_q_tp'])
            out['g2l'] = data['local_traj_tp']
        if mode != 'infer':
            net.data_encoder(data)                      # (its own sample is not used: z is formed from `eps` below)
            q = data['q_z_dist']
            out['q_z'] = torch.cat([q.mu, q.logvar], dim=-1)
        dd = net.data_decoder
        cm = ctx.mean(dim=0) if mut != 'e' else ctx.sum(dim=0) / max_len
        prior = Gaussian(params=dd.p_z_net(dd.prior_mlp(cm)))
        out['p_z'] = torch.cat([prior.mu, prior.logvar], dim=-1)
        if mode == 'train':
            z = q.sample(_t(eps, dt))
        elif mode == 'recon':
            z = q.mode()
        else:
            z = prior.sample(_t(eps, dt))
        out['z'] = z
        raw = dd.out_fc(dd.out_mlp(torch.cat([z.repeat((T, 1, 1)), ctx], dim=-1)))
        loc = raw.clone()
        if 'local_traj_tp' in data:
            loc[0, :, :2], loc[0, :, -2:] = data['local_traj_tp'][0, :, :2], data['local_traj_tp'][0, :, -2:]
        else:
            loc[0, :, :2] = 0.0
            loc[0, :, -2:] = torch.tensor([0., 1.], dtype=dt)
        tr, qq = tf.local_to_global_traj(loc)
        out.update(raw=raw, local_traj=loc, trans=tr, quat=qq, orient=tf.quat_to_aa(qq))
    return {k: (v.transpose(0, 1) if v.dim() == 3 else v).double().numpy() for k, v in out.items()}


def local_to_global(local, dtype=torch.float64):
    """tf.local_to_global_traj on (B,T,11) rows in `dtype`: dict trans, quat, orient (numpy fp64, batch-major)."""
    tr, qq = tf.local_to_global_traj(_t(local, dtype).transpose(0, 1))
    return {k: v.transpose(0, 1).double().numpy() for k, v in (('trans', tr), ('quat', qq), ('orient', tf.quat_to_aa(qq)))}


def l2g_inputs(T, B=5, seed=0):
    """Local rows (B,T,11) fp32 for the local_to_global tests: heading increments of up to +-0.5 rad per frame (the accumulated heading
    passes +-pi every few frames); sequence 1: 6D rows of rotations by ~pi about varying axes (quaternion w ~ 0: every branch of
    rotmat_to_quat); sequence 2: 6D rows far from orthonormal (scaled and sheared columns)."""
    rng = np.random.default_rng(5150 + 17 * T + seed)
    loc = mg._local_traj(rng, B * T).reshape(B, T, 11)
    dh = rng.uniform(-0.5, 0.5, size=(B, T))
    if B > 3:
        dh[3] = 0.45                                                        # a steady turn: 14 frames per revolution
    scale = rng.uniform(0.5, 2.0, size=(B, T))                              # the heading vector is not a unit vector either
    loc[..., 9], loc[..., 10] = np.cos(dh) * scale, np.sin(dh) * scale
    if B > 1:
        ax = rng.normal(size=(T, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        ang = np.pi - rng.uniform(0.0, 0.02, size=T) * rng.integers(0, 2, size=T)     # exactly pi on about half the frames
        R = aa_to_rotmat(ax * ang[:, None])
        loc[1, :, 3:6], loc[1, :, 6:9] = R[:, :, 0], R[:, :, 1]
    if B > 2:
        loc[2, :, 3:6] = loc[2, :, 3:6] * rng.uniform(0.2, 5.0, size=(T, 1)) + 0.0
        loc[2, :, 6:9] = loc[2, :, 6:9] * rng.uniform(0.2, 5.0, size=(T, 1)) + 0.7 * loc[2, :, 3:6]
    return loc.astype(np.float32)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def aa_to_rotmat(aa):
    """Rodrigues in fp64 numpy: (...,3) -> (...,3,3)."""
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -aa[..., 2], aa[..., 1], aa[..., 2], -aa[..., 0], -aa[..., 1], aa[..., 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(ths) / ths)
    b = np.where(small, 0.5, (1.0 - np.cos(ths)) / (ths * ths))
    return np.eye(3) + a * K + b * (K @ K)


def quat_to_rotmat(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def errors(got, ref, n=None):
    """Largest absolute difference per compared output over the first n frames: every key both hold, `orient` (axis-angle) as the difference
    of the rotation MATRICES ('rot': acos of a quaternion dot product is ill-conditioned at 1e-3 in fp32) and `quat` up to its sign."""
    out = {}
    for k in ref:
        if k not in got:
            continue
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if n is not None and k not in ('p_z', 'q_z', 'z'):
            g, r = g[..., :n, :], r[..., :n, :]
        if k == 'orient':
            out['rot'] = float(np.abs(aa_to_rotmat(g) - aa_to_rotmat(r)).max())
        elif k == 'quat':
            out['quat'] = float(np.minimum(np.abs(g - r), np.abs(g + r)).max())
        else:
            out[k] = float(np.abs(g - r).max())
    return out


class Reference:
    """Cached results of the port in `dtype`, one per (seed, length, mutation) of the sweep and one per traj_clip batch."""

    def __init__(self, asset_root, dtype=torch.float64, conditioned=True):
        self.net = predictor(asset_root, dtype, conditioned)
        self.cache = {}

    def joints(self, seed, T):
        k = ('joints', seed, T)
        if k not in self.cache:
            self.cache[k] = joints_of(self.net, seq_inputs(seed, T)[0])
        return self.cache[k]

    def __call__(self, seed, T, mut=None, max_len=300, neighbour=None):
        """The inference-mode result of sweep sequence (seed, T), each array with its leading batch axis removed.  `neighbour`: the (seed,
        length) whose joint row mutation 'd' plants."""
        k = (seed, T, mut, max_len if mut == 'e' else None, neighbour if mut == 'd' else None)
        if k not in self.cache:
            nb = self.joints(*neighbour) if mut == 'd' else None
            r = predict(self.net, self.joints(seed, T)[:, None], seq_inputs(seed, T)[1][None], mut=mut, max_len=max_len, neighbour=nb)
            self.cache[k] = {kk: v[0] for kk, v in r.items()}
        return self.cache[k]

    def clip(self, B, T, mode, valid_len=0):
        """traj_clip batch of the sequences clip_inputs(0 .. B-1, T) in `mode` ('infer' | 'train' | 'recon'); valid_len > 0: the joint rows
        of frames >= valid_len are zero (the chunk padding of the multi-step inference), everything still runs over T frames."""
        k = ('clip', B, T, mode, valid_len)
        if k not in self.cache:
            ins = [clip_inputs(i, T) for i in range(B)]
            j = joints_of(self.net, np.stack([x[0] for x in ins], axis=1))
            if 0 < valid_len < T:
                j[valid_len:] = 0.0
            self.cache[k] = predict(self.net, j, np.stack([x[1] for x in ins]), mode=mode, trans=np.stack([x[2] for x in ins], axis=1),
                                    orient=np.stack([x[3] for x in ins], axis=1))
        return self.cache[k]


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------
# Each is 16 x the largest error of the fp32 CPU port against the fp64 port (the reference's own rounding) over what the device tests run:
# 4 x for the split-fp16 products' 2^-22 per product against fp32's 2^-24, times 4 x for the summation order and the 1e-7 of the v_exp / v_rcp
# gates.  tests/test_traj_ref.py measures the floors again and asserts floor x 16 <= the constant, so they cannot drift from their basis.
FLOOR_FACTOR = 16


def _tol(**floors):
    return {k: FLOOR_FACTOR * v for k, v in floors.items()}


# measured floors (one thread), rounded up to two digits; the measured figure beside each.  They belong to the CPU build of torch that measured
# them: where another BLAS or vector path rounds differently and tests/test_traj_ref.py reports a floor above its constant,
# `python -m tests.traj_ref_common` prints the floors to write here (round up, keep the factor).  L2G_TOL[1]['trans'] is exactly 0: with one
# frame the translation is the row's own x, y, z, copied.
TOL = _tol(                # glamr_nets_infer routes and traj_clip on the sweep: floor over the 48 sequences of SWEEP, inference mode
    p_z=1.4e-7,            # 1.331e-7
    z=3.1e-7,              # 3.029e-7
    raw=3.4e-7,            # 3.302e-7
    local_traj=3.4e-7,     # 3.302e-7
    trans=1.3e-5,          # 1.206e-5 (a sum over up to 300 frames of steps rotated by an accumulated heading)
    quat=8.4e-7,           # 8.316e-7
    rot=2.0e-6)            # 1.914e-6 (rotation matrix of the axis-angle output)
CLIP_TOL = _tol(           # traj_clip batches: floor over CLIP_CASES x (infer, train, recon)
    g2l=1.7e-6,            # 1.620e-6 (global -> local rows of the ground-truth trajectory)
    q_z=2.6e-6,            # 2.543e-6
    p_z=1.1e-6,            # 1.066e-6
    z=2.7e-6,              # 2.674e-6
    raw=4.9e-6,            # 4.865e-6
    local_traj=4.9e-6,     # 4.865e-6
    trans=2.4e-5,          # 2.362e-5
    quat=4.6e-6,           # 4.561e-6
    rot=9.9e-6)            # 9.837e-6
L2G_TOL = {                # glamr_traj_local_to_global on l2g_inputs(T): floor per T
    1: _tol(trans=0.0, quat=1.9e-7, rot=3.2e-7),              # 0 (row 0 is copied), 1.838e-7, 3.191e-7
    2: _tol(trans=1.7e-8, quat=1.4e-7, rot=2.4e-7),           # 1.610e-8, 1.327e-7, 2.381e-7
    255: _tol(trans=4.9e-6, quat=1.2e-6, rot=3.3e-6),         # 4.821e-6, 1.199e-6, 3.240e-6
    256: _tol(trans=3.4e-6, quat=1.4e-6, rot=3.4e-6),         # 3.326e-6, 1.331e-6, 3.391e-6
    257: _tol(trans=6.2e-6, quat=1.6e-6, rot=4.2e-6),         # 6.161e-6, 1.574e-6, 4.189e-6
    600: _tol(trans=7.6e-6, quat=4.6e-6, rot=1.3e-5)}         # 7.585e-6, 4.589e-6, 1.245e-5
CLIP_CASES = [(2, 100, 0), (32, 100, 0), (523, 100, 0), (8, 300, 0), (2, 100, 70), (8, 300, 230)]      # (B, T, valid_len) of the traj_clip tests
L2G_LENS = [1, 2, 255, 256, 257, 600]


def _worse(acc, e):
    for k, v in e.items():
        acc[k] = max(acc.get(k, 0.0), v)
    return acc


class single_thread:
    """The fp32 port on one thread: its rounding then does not depend on how many cores the machine has."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def sweep_floor(r32, r64):
    """Largest error of the fp32 port against the fp64 port per output, over the whole sweep (inference mode)."""
    acc = {}
    with single_thread():
        for seed, T in SWEEP:
            _worse(acc, errors(r32(seed, T), r64(seed, T)))
    return acc


def clip_floor(r32, r64, most=None):
    """The same over every traj_clip batch of CLIP_CASES in the three modes.  `most`: at most that many sequences of a batch (sequence i is
    the same clip in every batch, so this is a subset: the constants were measured over all 523, the CPU suite checks them on the first 96)."""
    acc = {}
    with single_thread():
        for B, T, valid in sorted(set((min(B, most or B), T, valid) for B, T, valid in CLIP_CASES)):
            for mode in ('infer', 'train', 'recon'):
                _worse(acc, errors(r32.clip(B, T, mode, valid), r64.clip(B, T, mode, valid)))
    return acc


def l2g_floor(T):
    loc = l2g_inputs(T)
    with single_thread():
        return errors(local_to_global(loc, torch.float32), local_to_global(loc))


if __name__ == '__main__':          # the floors behind TOL, CLIP_TOL and L2G_TOL on this machine's CPU build of torch
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    r32, r64 = Reference(root, torch.float32), Reference(root)
    for name, floor in [('TOL', sweep_floor(r32, r64)), ('CLIP_TOL', clip_floor(r32, r64))] + [('L2G_TOL[%d]' % T, l2g_floor(T)) for T in L2G_LENS]:
        print('%s: %s' % (name, ', '.join('%s=%.3e' % kv for kv in sorted(floor.items()))))
