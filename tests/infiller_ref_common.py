"""fp64 reference of the motion infiller's forward (the weights of oracle.port.nets.MotionInfillerVAE in .double()), the two checkpoints it runs
on, the sweep of distinct sequences the device tests run, the mutations that show those tests can fail, and the tolerances, each derived from
the rounding of the fp32 CPU port against the fp64 one.

`window` / `infer` restate the forward of the port's three sub-modules (post-norm transformer layers written out) so that a mutation, or the
rounding of every product operand to two fp16 planes, can be placed inside it; tests/test_infiller_ref.py pins the unmutated restatement to
the port's own inference(multi_step=True) / forward().

One difference from the port, on purpose: the port builds its sinusoid table in the default dtype (torch.arange * exp(...) in fp32) whatever
the module's dtype is, so `.double()` still adds a table that is 3e-6 off (pos * mul rounded before the sine); through it the context moves
by 1.8e-6 and the pose by 1.5e-8.  The reference here evaluates sin / cos of pos * exp(-2 i ln(1e4) / 256) in fp64, as glamr_nets_create
does on the host, and the fp32 run takes that table rounded to fp32: floor (a) is the rounding of fp32 arithmetic on the same function,
not the distance between two tables.  (port_table=True gives the port's table back, for the pin against the port.)

Why a second checkpoint: glamr_amd/utils/synth.py draws every weight as U(+-1/sqrt(fan_in)); attention is then close to uniform and a wrong
row or a wrong softmax scale moves the pose by 2e-5 to 4e-6.  conditioned_state_dict() scales the input projections and every attention
in_proj until the attention weights depend on the data."""
import math
import os
import numpy as np
import torch

from oracle.port import build
from oracle.port.nets import MotionInfillerVAE
from tests import traj_ref_common as tc

D, FF, NZ, HEADS, HD = 256, 512, 128, 8, 32
PAST, CUR, FUT, WIN = 10, 30, 10, 50
FLOOR_FACTOR = tc.FLOOR_FACTOR
single_thread = tc.single_thread
FP16_LIMIT = 3.0e4
SMALL_ROWS = 2048                  # nn_kernels.hpp: the fused / split / co-schedulable kernels start at this many rows

# ---- the two checkpoints ----------------------------------------------------------------------------------------------------------------
# gain per parameter-name fragment (weights and biases alike).  x4 on the two input projections and x6 on every attention in_proj: the
# softmax logits grow by 36 (Q and K both scale), attention stops being uniform.  LayerNorm follows every block, so nothing downstream grows:
# the infiller lines of the range analysis go from 3288 to 19727, below the 3e4 at which a handle drops to fp32-only (range_bound()).
GAINS = (('context_encoder.in_fc.', 4.0), ('data_encoder.in_fc.', 4.0), ('_attn.in_proj_', 6.0))
CHECKPOINTS = ('shipped', 'conditioned')


def conditioned_state_dict(sd):
    out = {}
    for k, v in sd.items():
        g = 1.0
        for frag, gain in GAINS:
            if frag in k:
                g = gain
        out[k] = v.detach().clone() * g
    return out


def load_state_dict(asset_root, conditioned=False):
    sd = torch.load(build._ckpt(asset_root, os.path.join('motion_filler', 'motion_infiller_demo')), map_location='cpu', weights_only=False)['state_dict']
    sd = {k: v for k, v in sd.items() if not k.startswith('smpl.')}
    return conditioned_state_dict(sd) if conditioned else sd


def port(asset_root, dtype=torch.float64, conditioned=False):
    """The CPU port with the checkpoint's weights in `dtype`."""
    net = MotionInfillerVAE()
    net.load_state_dict(load_state_dict(asset_root, conditioned), strict=True)
    return net.to(dtype).eval()


def pos_table(n, offset, dtype, port=False):
    """Interleaved (sin, cos) rows for positions offset .. offset + n - 1, evaluated in fp64 and rounded to `dtype`; port=True: in the
    port's own fp32 arithmetic (ConcatPosEnc.table under the default dtype)."""
    if port:
        pos = (torch.arange(n) + offset).unsqueeze(-1)
        mul = torch.exp(torch.arange(0, D, 2) * (-np.log(10000.0) / D))
    else:
        pos = (torch.arange(n, dtype=torch.float64) + offset).unsqueeze(-1)
        mul = torch.exp(torch.arange(0, D, 2, dtype=torch.float64) * (-math.log(10000.0) / D))
    return torch.stack([torch.sin(pos * mul), torch.cos(pos * mul)], dim=-1).view(-1, D).to(dtype)


def range_bound(sd):
    """The infiller lines of glamr_nets_create's range analysis (glamr_amd/csrc/nets.hip: enc_layer, dec_layer_b, the prior, dec_z and qe_in
    lines; |pose| <= 10, |z| <= 100; a LayerNorm's output is bounded by |gamma| sqrt(255) + |beta|), restated: (worst converted activation,
    largest weight).  Both must stay below FP16_LIMIT for the handle to keep the fp16-split kernels.  It has to follow those lines; it exists
    so that a change of GAINS is judged without a device.  The device fixture asserts glamr_nets_precision == 0 on the real analysis (whose
    figure also covers the trajectory predictor)."""
    P = {k: v.double() for k, v in sd.items()}
    worst, wmax = [0.0], [0.0]

    def see(b):
        worst[0] = max(worst[0], float(b))
        return float(b)

    def out_of(W, b, x):
        wmax[0] = max(wmax[0], float(W.abs().max()))
        return float(W.abs().sum(1).max()) * x + (float(b.abs().max()) if b is not None else 0.0)

    def lnb(pre):
        return float((P[pre + '.weight'].abs() * math.sqrt(255.0) + P[pre + '.bias'].abs()).max())

    def lin(pre, x):
        return out_of(P[pre + '.weight'], P[pre + '.bias'], x)

    def folded(pre, n, offset, tokens=None):
        """in_fc folded into pos_enc.fc: (W_x W_in, table[pos] = W_p code(pos) + b_pe + W_x b_in, or + W_x token for the token rows)"""
        Wpe, bpe = P[pre + '.pos_enc.fc.weight'], P[pre + '.pos_enc.fc.bias']
        Wx, Wp = Wpe[:, :D], Wpe[:, D:]
        table = pos_table(n, offset, torch.float64) @ Wp.T + bpe
        fold = Wx @ P[pre + '.in_fc.bias']
        rows = [Wx @ t for t in (tokens or [])] + [fold] * (n - len(tokens or []))
        return Wx @ P[pre + '.in_fc.weight'], float((table + torch.stack(rows)).abs().max())

    def enc_layer(pre, x):
        see(x)
        see(out_of(P[pre + '.self_attn.in_proj_weight'], P[pre + '.self_attn.in_proj_bias'], x))
        see(lin(pre + '.linear1', lnb(pre + '.norm1')))
        see(lnb(pre + '.norm1'))
        wmax[0] = max(wmax[0], float(P[pre + '.self_attn.out_proj.weight'].abs().max()), float(P[pre + '.linear2.weight'].abs().max()))
        return lnb(pre + '.norm2')

    def dec_layer(pre, x, ctx):
        see(x), see(ctx)
        see(out_of(P[pre + '.self_attn.in_proj_weight'], P[pre + '.self_attn.in_proj_bias'], x))
        cw, cb = P[pre + '.multihead_attn.in_proj_weight'], P[pre + '.multihead_attn.in_proj_bias']
        n1, n2 = lnb(pre + '.norm1'), lnb(pre + '.norm2')
        see(n1), see(out_of(cw[:D], cb[:D], n1)), see(out_of(cw[D:], cb[D:], ctx))
        see(n2), see(lin(pre + '.linear1', n2))
        for k in ('.self_attn.out_proj', '.multihead_attn.out_proj', '.linear2'):
            wmax[0] = max(wmax[0], float(P[pre + k + '.weight'].abs().max()))
        return lnb(pre + '.norm3')

    POSE, ZMAX = 10.0, 100.0
    W, tab = folded('context_encoder', WIN, 0)
    h0 = see(out_of(W, None, see(POSE)) + tab)
    ctx = enc_layer('context_encoder.temporal_net.layers.1', enc_layer('context_encoder.temporal_net.layers.0', h0))
    pr = 'data_decoder.prior_temporal_net.layers.0'
    cw, cb = P[pr + '.multihead_attn.in_proj_weight'], P[pr + '.multihead_attn.in_proj_bias']
    see(out_of(cw[D:], cb[D:], ctx)), see(lnb(pr + '.norm2')), see(lin(pr + '.linear1', lnb(pr + '.norm2'))), see(lnb(pr + '.norm3'))
    Wz, bz = P['data_decoder.pos_enc.fc.weight'], P['data_decoder.pos_enc.fc.bias']
    q = see(out_of(Wz[:, :NZ], None, see(ZMAX)) + float((pos_table(CUR, PAST, torch.float64) @ Wz[:, NZ:].T + bz).abs().max()))
    q = dec_layer('data_decoder.temporal_net.layers.1', dec_layer('data_decoder.temporal_net.layers.0', q, ctx), ctx)
    o1 = see(lin('data_decoder.out_mlp.affine_layers.0', q))
    see(lin('data_decoder.out_mlp.affine_layers.1', o1))
    W, tab = folded('data_encoder', 32, 0, [P['data_encoder.mu_token'], P['data_encoder.logvar_token']])
    qe = see(out_of(W, None, POSE) + tab)
    see(dec_layer('data_encoder.temporal_net.layers.1', dec_layer('data_encoder.temporal_net.layers.0', qe, ctx), ctx))
    for k in (pr + '.multihead_attn.out_proj', pr + '.linear2', 'data_decoder.p_z_mu_net', 'data_decoder.p_z_logvar_net', 'data_decoder.out_fc',
              'data_encoder.q_z_mu_net', 'data_encoder.q_z_logvar_net'):
        wmax[0] = max(wmax[0], float(P[k + '.weight'].abs().max()))
    return worst[0], wmax[0]


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
# A sequence is (seed, length, mask kind).  The pose and the latent draws are mg.net_inputs' (same generator, same stream); kinds:
#   'gap'       mg.net_inputs' own: frames [T // 3, T // 3 + T // 5) invisible
#   'straddle'  frames [35, 45) invisible: the gap holds the last 5 generated frames of window 0 and the first 5 of window 1
#   'blind'     frames [10, 50) invisible: window 0 sees its 10 past frames and nothing else
#   'none'      every frame visible (keys are masked only past the sequence's end)
KINDS = ('gap', 'straddle', 'blind', 'none')
_LENS = [11, 40, 41, 70, 71, 100, 12, 39, 42, 69, 72, 99, 50, 51, 25, 64, 33, 80, 81, 47, 18, 90, 60]       # 23: coprime with the 4 kinds
ROUTE_SEQS = [(500 + i, _LENS[i % len(_LENS)], KINDS[i % 4]) for i in range(69)]       # every device batch is a prefix: distinct data per slot
LONG_SEQS = [(0, 120, 'gap'), (1, 300, 'gap'), (5, 150, 'gap'), (7, 200, 'straddle'), (8, 130, 'blind'), (9, 257, 'none')]
ALL_SEQS = ROUTE_SEQS + LONG_SEQS                # what the floors are taken over
SWEEP = ROUTE_SEQS[:24] + LONG_SEQS              # what the mutations are judged on (30 sequences; none left out)
ROUTE_BATCHES = [1, 40, 41, 68, 69]              # glamr_nets_infer: 2000 rows | 2050 encoder rows fused, 1230 decoder rows not | 2040 / 2070 decoder rows
WINDOW_BATCHES = [1, 41, 63, 64, 69]             # glamr_nets_infiller_window: the posterior's B * 32 rows cross 2048 at 64


def route_seqs(B):
    return [LONG_SEQS[1]] if B == 1 else ROUTE_SEQS[:B]          # alone: the 300-frame sequence, ten windows


def n_windows(T):
    return int(np.ceil((T - PAST) / CUR))


def seq_inputs(seed, T, kind='gap'):
    """dict: full (T,69) fp32 the pose with nothing hidden, pose (T,69) fp32 with the invisible frames zeroed, vis (T,) fp32 1 = visible,
    eps (n_win,128) fp32."""
    rng = np.random.default_rng(4242 + seed)
    t = np.arange(T)[:, None] / 30.0
    full = (0.3 * np.sin(2 * np.pi * rng.uniform(0.2, 0.8, size=(1, 69)) * t + rng.uniform(0, 6.28, size=(1, 69)))).astype(np.float32)
    vis = np.ones(T, np.float32)
    if kind == 'gap':
        vis[T // 3:T // 3 + T // 5] = 0
    elif kind == 'straddle':
        vis[35:45] = 0
    elif kind == 'blind':
        vis[10:50] = 0
    else:
        assert kind == 'none', kind
    pose = full.copy()
    pose[vis == 0] = 0
    return dict(full=full, pose=pose, vis=vis, eps=rng.normal(size=(n_windows(T), 128)).astype(np.float32))


def window_inputs(seq):
    """Window 0 of a sequence as glamr_nets_infiller_window takes it: in_body_pose (50,69), frame_mask (50,) 1 = visible (the 10 past frames
    always, nothing past the end), eps (128,), body_pose (50,69) the full pose for the posterior encoder."""
    inp = seq_inputs(*seq)
    n = min(WIN, seq[1])
    x, gx, m = np.zeros((WIN, 69), np.float32), np.zeros((WIN, 69), np.float32), np.zeros(WIN, np.float32)
    x[:n], gx[:n], m[:n] = inp['pose'][:n], inp['full'][:n], inp['vis'][:n]
    m[:PAST] = 1
    return dict(in_body_pose=x, frame_mask=m, eps=inp['eps'][0], body_pose=gx)


# ---- the forward, with room for a mutation ----------------------------------------------------------------------------------------------
MUTATION_NAMES = {
    'enc_lo': "low fp16 plane of the second encoder layer's self_attn.out_proj.weight lost",
    'out_lo': 'low fp16 plane of out_fc.weight lost',
    'row': "a neighbour's row for frame 5 of every window",
    'q_enc': 'Q x 1.01 in the first encoder layer',
    'q_dec': "Q x 1.01 in the last decoder layer's cross-attention",
    'ln_eps': "eps 1e-3 in the second encoder layer's norm2",
    'ln_div': "variance over 255 in the last decoder layer's norm3",
    'mask': 'the first masked key of a window let through in the first encoder layer',
    'pos': "the decoder's position offset 11 instead of 10",
    'resid': "the first encoder layer's feed-forward residual taken before norm1 instead of after",
    'tokens': "the prior's mu read from the logvar token's row and the other way round",
    'past': 'the past frames of window i + 1 taken from the input instead of from the output of window i',
}
MUTATIONS = tuple(MUTATION_NAMES)
LN_EPS_AT = 'context_encoder.temporal_net.layers.1.norm2'
LN_DIV_AT = 'data_decoder.temporal_net.layers.1.norm3'
_LO = {'enc_lo': 'context_encoder.temporal_net.layers.1.self_attn.out_proj.weight', 'out_lo': 'data_decoder.out_fc.weight'}


def split16(x):
    """x rounded to two fp16 planes, hi + lo: what the split kernels multiply (nn_kernels.hpp), 2^-22 relative per operand."""
    hi = x.to(torch.float16).to(x.dtype)
    return hi + (x - hi).to(torch.float16).to(x.dtype)


def _ident(x):
    return x


class _Fwd:
    """One forward in the dtype of the parameters P (name -> tensor); R rounds every product operand; mut: one of MUTATIONS or None."""

    def __init__(self, P, R=_ident, mut=None, port_table=False):
        self.P, self.R, self.mut = P, R, mut
        self.dt = P['data_decoder.out_fc.weight'].dtype
        self.port_table = port_table
        if mut in _LO:
            self.P = dict(P)
            self.P[_LO[mut]] = P[_LO[mut]].to(torch.float16).to(self.dt)

    def mm(self, x, W, b):
        return self.R(x) @ self.R(W).T + b

    def lin(self, pre, x):
        return self.mm(x, self.P[pre + '.weight'], self.P[pre + '.bias'])

    def ln(self, pre, x):
        eps = 1e-3 if (self.mut == 'ln_eps' and pre == LN_EPS_AT) else 1e-5
        div = D - 1 if (self.mut == 'ln_div' and pre == LN_DIV_AT) else D
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / div
        return (x - mean) / torch.sqrt(var + eps) * self.P[pre + '.weight'] + self.P[pre + '.bias']

    def mha(self, pre, xq, xkv, mask, qscale=1.0, leak=False):
        W, b = self.P[pre + '.in_proj_weight'], self.P[pre + '.in_proj_bias']
        heads = lambda t: t.view(t.shape[0], t.shape[1], HEADS, HD).transpose(1, 2)
        q = heads(self.mm(xq, W[:D], b[:D])) * qscale
        k, v = heads(self.mm(xkv, W[D:2 * D], b[D:2 * D])), heads(self.mm(xkv, W[2 * D:], b[2 * D:]))
        s = self.R(q) @ self.R(k).transpose(-1, -2) / math.sqrt(HD)
        if mask is not None:
            m = mask
            if leak:
                m = mask.clone()
                for bi in range(m.shape[0]):
                    idx = torch.nonzero(m[bi])
                    if len(idx):
                        m[bi, idx[0, 0]] = False
            s = s.masked_fill(m[:, None, None, :], float('-inf'))
        o = (self.R(torch.softmax(s, dim=-1)) @ self.R(v)).transpose(1, 2).reshape(xq.shape[0], xq.shape[1], D)
        return self.lin(pre + '.out_proj', o)

    def ffn(self, pre, x):
        return self.lin(pre + '.linear2', torch.relu(self.lin(pre + '.linear1', x)))

    def enc_layer(self, l, x, mask):
        pre, m = 'context_encoder.temporal_net.layers.%d' % l, self.mut
        t = x + self.mha(pre + '.self_attn', x, x, mask, 1.01 if (m == 'q_enc' and l == 0) else 1.0, m == 'mask' and l == 0)
        x1 = self.ln(pre + '.norm1', t)
        return self.ln(pre + '.norm2', (t if (m == 'resid' and l == 0) else x1) + self.ffn(pre, x1))

    def dec_layer(self, pre, x, mem, mask, last=False):
        m = self.mut
        x = self.ln(pre + '.norm1', x + self.mha(pre + '.self_attn', x, x, None))
        x = self.ln(pre + '.norm2', x + self.mha(pre + '.multihead_attn', x, mem, mask, 1.01 if (m == 'q_dec' and last) else 1.0))
        return self.ln(pre + '.norm3', x + self.ffn(pre, x))

    def pos_enc(self, pre, x, offset=0):
        pe = pos_table(x.shape[1], offset, self.dt, self.port_table).expand(x.shape[0], -1, -1)
        return self.lin(pre + '.fc', torch.cat([x, pe], dim=-1))

    def window(self, x, mask, eps, mode='infer', gx=None):
        """x (B,50,69), mask (B,50) bool True = key ignored, eps (B,128) or None, gx (B,50,69) for train / recon.  Returns tensors context
        (B,50,256), p_z (B,2,128), z (B,128), out (B,30,69) [, q_z (B,2,128)]."""
        P, B = self.P, x.shape[0]
        h = self.pos_enc('context_encoder.pos_enc', self.lin('context_encoder.in_fc', x))
        ctx = self.enc_layer(1, self.enc_layer(0, h, mask), mask)
        out = {'context': ctx}
        if mode != 'infer':
            tok = torch.stack([P['data_encoder.mu_token'], P['data_encoder.logvar_token']]).expand(B, -1, -1)
            q = self.pos_enc('data_encoder.pos_enc', torch.cat([tok, self.lin('data_encoder.in_fc', gx[:, PAST:PAST + CUR])], dim=1))
            q = self.dec_layer('data_encoder.temporal_net.layers.0', q, ctx, mask)
            q = self.dec_layer('data_encoder.temporal_net.layers.1', q, ctx, mask)
            q_mu, q_lv = self.lin('data_encoder.q_z_mu_net', q[:, 0]), self.lin('data_encoder.q_z_logvar_net', q[:, 1])
            out['q_z'] = torch.stack([q_mu, q_lv], dim=1)
        tok = torch.stack([P['data_decoder.mu_token'], P['data_decoder.logvar_token']]).expand(B, -1, -1)
        p = self.dec_layer('data_decoder.prior_temporal_net.layers.0', self.pos_enc('data_decoder.prior_pos_enc', tok), ctx, mask)
        r_mu, r_lv = (1, 0) if self.mut == 'tokens' else (0, 1)
        p_mu, p_lv = self.lin('data_decoder.p_z_mu_net', p[:, r_mu]), self.lin('data_decoder.p_z_logvar_net', p[:, r_lv])
        out['p_z'] = torch.stack([p_mu, p_lv], dim=1)
        if mode == 'train':
            z = q_mu + eps * torch.exp(0.5 * q_lv)
        elif mode == 'recon':
            z = q_mu
        else:
            z = p_mu + eps * torch.exp(0.5 * p_lv)
        out['z'] = z
        q = self.pos_enc('data_decoder.pos_enc', z[:, None, :].expand(-1, CUR, -1), offset=PAST + (1 if self.mut == 'pos' else 0))
        q = self.dec_layer('data_decoder.temporal_net.layers.0', q, ctx, mask)
        q = self.dec_layer('data_decoder.temporal_net.layers.1', q, ctx, mask, last=True)
        q = torch.relu(self.lin('data_decoder.out_mlp.affine_layers.1', torch.relu(self.lin('data_decoder.out_mlp.affine_layers.0', q))))
        out['out'] = self.lin('data_decoder.out_fc', q)
        return out

    def infer(self, pose, vis, eps, neighbour=None):
        """inference(multi_step=True) of one sequence: pose (T,69), vis (T,), eps (n_win,128) tensors.  Returns pose (T,69) and, per window,
        context (n_win,50,256), p_z (n_win,2,128), z (n_win,128)."""
        T = pose.shape[0]
        cur, rec = pose.clone(), {'context': [], 'p_z': [], 'z': []}
        for i in range(n_windows(T)):
            s = i * CUR
            eb = min(s + WIN, T)
            x, m = torch.zeros((WIN, 69), dtype=self.dt), torch.ones(WIN, dtype=torch.bool)
            x[:eb - s], m[:eb - s] = cur[s:eb], vis[s:eb] == 0
            m[:PAST] = False
            if self.mut == 'past' and i > 0:
                x[:PAST] = pose[s:s + PAST]
            if self.mut == 'row':
                x[5] = neighbour[min(s + 5, neighbour.shape[0] - 1)]
            o = self.window(x[None], m[None], eps[i][None])
            nf = min(s + PAST + CUR, T) - s
            cur[s + PAST:s + nf] = o['out'][0, :nf - PAST]
            for k in rec:
                rec[k].append(o[k][0])
        return dict(pose=cur, **{k: torch.stack(v) for k, v in rec.items()})


KEYS = ('pose', 'context', 'p_z', 'q_z', 'z')


def errors(got, ref):
    """Largest absolute difference per output both hold."""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) for k in KEYS if k in got and k in ref}


def _worse(acc, e):
    for k, v in e.items():
        acc[k] = max(acc.get(k, 0.0), v)
    return acc


class Reference:
    """Cached results of the restated forward, per (sequence, mutation) for the sliding-window inference and per (sequence, mode) for one
    window.  split: every product operand rounded to two fp16 planes (floor (b))."""

    def __init__(self, asset_root, dtype=torch.float64, conditioned=False, split=False, port_table=False):
        self.dt, self.R, self.port_table = dtype, split16 if split else _ident, port_table
        self.P = {k: v.to(dtype) for k, v in load_state_dict(asset_root, conditioned).items()}
        self.cache = {}

    def _t(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dt)

    def infer(self, seq, mut=None, neighbour=None):
        """dict of numpy fp64 arrays: pose (T,69), context (n_win,50,256), p_z (n_win,2,128), z (n_win,128)."""
        k = ('infer', seq, mut, neighbour if mut == 'row' else None)
        if k not in self.cache:
            inp = seq_inputs(*seq)
            nb = self._t(seq_inputs(*neighbour)['pose']) if mut == 'row' else None
            with torch.no_grad():
                r = _Fwd(self.P, self.R, mut, self.port_table).infer(self._t(inp['pose']), self._t(inp['vis']), self._t(inp['eps']), nb)
            self.cache[k] = {kk: v.double().numpy() for kk, v in r.items()}
        return self.cache[k]

    def windows(self, seqs, mode):
        """Window 0 of every sequence (window_inputs) in `mode`, one batched forward for those not cached yet: list of dicts context (50,256),
        p_z (2,128), z (128,), pose (30,69) [, q_z (2,128)]."""
        todo = [s for s in dict.fromkeys(seqs) if ('window', s, mode) not in self.cache]
        if todo:
            w = [window_inputs(s) for s in todo]
            st = lambda k: self._t(np.stack([x[k] for x in w]))
            with torch.no_grad():
                r = _Fwd(self.P, self.R, None, self.port_table).window(st('in_body_pose'), torch.as_tensor(np.stack([x['frame_mask'] for x in w]) != 1),
                                                                        st('eps'), mode, st('body_pose'))
            r['pose'] = r.pop('out')
            for i, s in enumerate(todo):
                self.cache[('window', s, mode)] = {kk: v[i].double().numpy() for kk, v in r.items()}
        return [self.cache[('window', s, mode)] for s in seqs]

    def window(self, seq, mode):
        return self.windows([seq], mode)[0]


def window0(r):
    """Of an infer() result what the window tests of the device compare as well: the pose over the whole sequence, the rest for window 0."""
    return {k: (v if k == 'pose' else v[0]) for k, v in r.items()}


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------
# Floor (a): the largest error of the fp32 CPU port (restated, one thread, the port's fp32 position table) against the fp64 reference, per
# output, over ALL_SEQS through the sliding-window inference (every window's context, p_z and z) and over ROUTE_SEQS through one window in the
# three modes.  Floor (b): the same for the fp64 forward with every product operand rounded to two fp16 planes -- the number format of the
# split kernels, 2^-22 per operand.  The tolerance is FLOOR_FACTOR x floor (a) on every route; (b) is recorded to show where it lies (below
# a quarter of the tolerance).  tests/test_infiller_ref.py measures both again and holds the tables to [1/2, 2] x;
# `python -m tests.infiller_ref_common` prints them.
FLOOR_A = {                 # measured (one thread), rounded up to two digits; the measured figure beside each
    'shipped': dict(pose=6.2e-8, context=3.4e-6, p_z=1.4e-6, q_z=1.6e-6, z=2.2e-6),            # 6.107e-8, 3.398e-6, 1.307e-6, 1.540e-6, 2.118e-6
    'conditioned': dict(pose=1.2e-7, context=7.1e-6, p_z=2.6e-6, q_z=2.6e-6, z=3.7e-6),       # 1.198e-7, 7.022e-6, 2.522e-6, 2.581e-6, 3.699e-6
}
FLOOR_B = {
    'shipped': dict(pose=2.3e-7, context=3.7e-6, p_z=2.0e-6, q_z=1.6e-6, z=4.0e-6),            # 2.253e-7, 3.613e-6, 1.973e-6, 1.535e-6, 3.979e-6
    'conditioned': dict(pose=2.4e-7, context=1.5e-5, p_z=4.8e-6, q_z=4.1e-6, z=6.6e-6),       # 2.305e-7, 1.439e-5, 4.757e-6, 4.087e-6, 6.532e-6
}
TOL = {c: {k: FLOOR_FACTOR * v for k, v in FLOOR_A[c].items()} for c in CHECKPOINTS}


def floors(other, r64, seqs=None, window_seqs=None):
    """Largest error of `other` (the fp32 or the split reference) against r64 per output."""
    acc = {}
    with single_thread():
        for seq in (ALL_SEQS if seqs is None else seqs):
            _worse(acc, errors(other.infer(seq), r64.infer(seq)))
        for mode in ('infer', 'train', 'recon'):
            ws = ROUTE_SEQS if window_seqs is None else window_seqs
            for a, b in zip(other.windows(ws, mode), r64.windows(ws, mode)):
                _worse(acc, errors(a, b))
    return acc


if __name__ == '__main__':          # the floors behind FLOOR_A and FLOOR_B on this machine's CPU build of torch
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    for c in CHECKPOINTS:
        r64 = Reference(root, conditioned=c == 'conditioned')
        print('%s: range bound %.0f, largest weight %.3f' % ((c,) + range_bound(load_state_dict(root, c == 'conditioned'))))
        for name, other in (('FLOOR_A', Reference(root, torch.float32, c == 'conditioned')), ('FLOOR_B', Reference(root, conditioned=c == 'conditioned', split=True))):
            print('%s[%r]: %s' % (name, c, ', '.join('%s=%.3e' % kv for kv in sorted(floors(other, r64).items()))))
