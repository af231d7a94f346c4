"""fp64 reference of the pose VJP glamr_grecon_pose_backward computes (csrc/grecon_pose_bwd.hpp): torch autograd of
oracle.port.grecon.GlobalReconOptimizer.pred_trajectory_base plus the world_dheading lines of its forward, for
L = sum(G_o * orient_world) + sum(G_t * trans_world), scattered into the layout of the stage kernel's gradient array.  Cases, inputs,
screening, upstream patterns, mutations and tolerances of tests/test_extra_loss_ref.py (CPU: the header on the host runtime) and
tests/test_extra_loss_gpu.py (the kernel).

Inputs: the ASSEMBLED rows (prior + deltas) of a person are a sequence of tests/global_vjp_common.py's generator -- decoder-like rows, large
turns, every rotmat_to_quat branch, world orientations 1e-2 (and, small headings only, 1e-4) from angle pi -- the parameters are randn x 1e-2
(the sizes Adam reaches in the fixtures) and the prior is the row minus the parameters, so the families sit where the generator put them.  The
screening is the generator's (every branch condition 1e-3 away from switching in the fp64 forward), on the assembled rows, and with
world_dheading also on the second quaternion -> axis-angle step.

Tolerances follow the project's rule: FLOOR_FACTOR = 16 x the error of the SAME autograd run in float32 against float64, relative to the
largest reference entry of the variable group within the person; groups xy/dxy, z, rot, heading/dheading, world_dheading; per case the worst
over its persons and upstream patterns.  The floors are constants below (`python -m tests.extra_loss_common` prints them); the CPU test
measures them again and fails outside [1/2, 2] x the constant.  A floor of exactly 0 (local_z is a copy of g_trans's z) asks for the exact result."""
import ctypes

import numpy as np
import torch

from oracle.port import transforms as tf
from oracle.port.grecon import GlobalReconOptimizer
from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import global_vjp_common as gc

FLOOR_FACTOR = 16
GROUPS = ('xy', 'z', 'rot', 'heading', 'world_dheading')
PATTERNS = ('all', 'trans', 'orient', 'onehot')
SCALES = (1e-6, 1e5)      # G x scale: the VJP is plain fp32 and linear in G
PARAM_SCALE = 1e-2
CANDIDATES = 4
MAX_DROPPED_SHARE = 0.25
VB = packing.VAR_BITS
ALL_VARS = VB['local_xy'] | VB['local_heading'] | VB['world_dheading'] | VB['local_dxy'] | VB['local_rot'] | VB['local_z'] | VB['local_dheading']
DEFAULT_FIX = ((0, None),)      # the shipped cam_fix_frames: the mask is all zero and the batch carries none

# scenes: (seq_len, [(fr_start, fr_end) | None = empty slot, ...]); kinds: global_vjp_common.sequence's `kind` per case (bit 0 = large turns)
SPECS = {
    'one24': dict(scenes=[(24, [(0, 24)])], fix=DEFAULT_FIX, kind=0),
    'two': dict(scenes=[(24, [(0, 24), (5, 22)])], fix=((0, 5),), kind=1),
    'T257': dict(scenes=[(257, [(0, 257)])], fix=((0, 5),), kind=1),                      # the first length with two frames on a thread
    'single': dict(scenes=[(8, [(3, 4)])], fix=((0, 5),), kind=0),                        # one existing frame
    'batch': dict(scenes=[(20, [(0, 20), (2, 15), (4, 20)]), (13, [(0, 13), (1, 9), None])], fix=((0, 5),), kind=3),
    'frozen': dict(scenes=[(16, [(0, 16), (3, 16)])], fix=((0, 5),), kind=0, frozen=[0, 1]),
    'norot': dict(scenes=[(24, [(0, 24)])], fix=((0, 5),), kind=3, var_mask=ALL_VARS & ~VB['local_rot']),
}
CASE_NAMES = [n + s for n in SPECS for s in ('', '_wd')]      # _wd: GLAMR_FLAG_HAS_WORLD_DHEADING

MUTATIONS = {'mask': 'dheading_mask ignored', 'wd_disp': 'world_dheading also rotates the displacement', 'row0': 'row 0 reads local_dxy',
             'vec_add': 'the heading delta added to the vector instead of the angle', 'outside': 'frames outside the existing range counted',
             'var_mask': 'var_mask ignored'}


def _graft(value, grad_of):
    """`value`'s numbers with `grad_of`'s gradient."""
    return value.detach() + (grad_of - grad_of.detach())


class PosePort(GlobalReconOptimizer):
    """The port's optimiser cut down to the map world poses <- trajectory variables: its own pred_trajectory_base and the world_dheading
    lines of its forward.  `mut` changes the BACKWARD of a copy of pred_trajectory_base only."""

    def __init__(self, cam_fix_frames, mut=None):      # (nothing of the base class's state is needed)
        self.cam_fix_frames, self.mut, self.device, self.flag_opt_traj = cam_fix_frames, mut, 'cpu', True

    def pred_trajectory_base(self, d):
        if self.mut not in ('mask', 'row0', 'vec_add'):
            return GlobalReconOptimizer.pred_trajectory_base(self, d)
        L = d['traj_local_pred'].detach().clone()
        L[0, :2] += d['traj_local_xy'].detach() if self.mut == 'row0' else d['traj_local_xy']
        L[1:, :2] += d['traj_local_dxy']
        mask = torch.ones_like(L[1:, 0])
        for (s, e) in self.cam_fix_frames:
            mask[s:e] = 0.0
        h0 = tf.vec_to_heading(L[[0], -2:].clone()) + d['traj_local_heading']
        L[0, -2:] = tf.heading_to_vec(h0).squeeze(0)
        delta = d['traj_local_dheading'] * mask
        if self.mut == 'mask':
            delta = _graft(delta, d['traj_local_dheading'])
        prior_vec = L[1:, -2:].clone()
        vec = tf.heading_to_vec(tf.vec_to_heading(prior_vec) + delta)
        if self.mut == 'vec_add':
            vec = _graft(vec, prior_vec + delta[:, None])
        L[1:, -2:] = vec
        L[:, 2] += d['traj_local_z']
        L[:, 3:-2] += d['traj_local_rot']
        d['traj_local'] = L
        trans, q = tf.local_to_global_traj(L)
        ex = d['exist_frames']
        d['smpl_orient_world_base'] = d['smpl_orient_world_base'].detach().clone()
        d['root_trans_world_base'] = d['root_trans_world_base'].detach().clone()
        d['smpl_orient_world_base'][ex] = tf.quat_to_aa(q)
        d['root_trans_world_base'][ex] = trans

    def poses(self, d):
        """(orient_world, trans_world) (Ts, 3) of one person: forward's lines for it (global_recon_model.py:394-426, 459-465)."""
        self.pred_trajectory_base(d)
        orient, trans = d['smpl_orient_world_base'], d['root_trans_world_base']
        if 'world_dheading' in d:
            w = d['world_dheading']
            wq = tf.aa_to_quat(torch.cat((torch.zeros([w.shape[0], 2], dtype=w.dtype), w), dim=-1))
            orient = tf.quat_to_aa(tf.quat_mul(wq, tf.aa_to_quat(d['smpl_orient_world_base'])))
            if self.mut == 'wd_disp':      # the displacement of row e + 1 turned by world_dheading of row e's frame as well
                ex = torch.where(d['exist_frames'])[0]
                xy = trans[ex, :2]
                if len(ex) > 1:
                    step = tf._rot2d(xy[1:] - xy[:-1], w[ex[:-1], 0])
                    xy2 = torch.cumsum(torch.cat([xy[:1], step], dim=0), dim=0)
                    trans = trans.clone()
                    trans[ex, :2] = _graft(xy, xy2)
        return orient, trans


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _person_inputs(n, Ts, fs, seed, kind, fix, rng):
    """Prior rows, parameters (randn x 1e-2), mask and base orientation of one person; the assembled rows are gc.sequence(n, seed, kind)."""
    A, near = gc.sequence(n, seed, kind)
    A = A.astype(np.float64)
    f32 = lambda a: np.asarray(a, np.float32)
    p = dict(xy=f32(rng.normal(size=2) * PARAM_SCALE), heading=f32(rng.normal(size=1) * PARAM_SCALE), dxy=f32(rng.normal(size=(n - 1, 2)) * PARAM_SCALE),
             dheading=f32(rng.normal(size=n - 1) * PARAM_SCALE), z=f32(rng.normal(size=n) * PARAM_SCALE), rot=f32(rng.normal(size=(n, 6)) * PARAM_SCALE),
             world_dheading=f32(rng.normal(size=(Ts, 1)) * PARAM_SCALE))
    mask = np.ones(n - 1, np.float32)
    for (s, e) in fix:
        mask[s:e] = 0.0
    prior = A.copy()
    prior[0, :2] -= p['xy']
    prior[1:, :2] -= p['dxy']
    prior[:, 2] -= p['z']
    prior[:, 3:9] -= p['rot']
    ang = np.arctan2(A[:, 10], A[:, 9]) - np.concatenate([p['heading'], p['dheading'] * mask]).astype(np.float64)
    prior[:, 9:] = np.linalg.norm(A[:, 9:], axis=-1, keepdims=True) * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    base = rng.normal(size=(Ts, 3)) * 0.8      # read outside the existing range only (and only with world_dheading)
    return dict(prior=f32(prior), params=p, mask=mask, base=f32(base), near=near, n=n, fs=fs, Ts=Ts)


def person_dict(pi, dtype, wd):
    """The port's person dictionary of one person's inputs in `dtype`, the variables as leaves."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    n, fs, Ts = pi['n'], pi['fs'], pi['Ts']
    ex = torch.zeros(Ts, dtype=torch.bool)
    ex[fs:fs + n] = True
    d = dict(traj_local_pred=t(pi['prior']), exist_frames=ex, smpl_orient_world_base=t(pi['base']), root_trans_world_base=torch.zeros(Ts, 3, dtype=dtype))
    names = ['xy', 'heading', 'dxy', 'dheading', 'z', 'rot']
    for k in names:
        d['traj_local_' + k] = t(pi['params'][k]).requires_grad_(True)
    if wd:
        d['world_dheading'] = t(pi['params']['world_dheading']).requires_grad_(True)
    return d


def _margin(pi, fix, wd):
    """Smallest distance of a branch condition from switching in the fp64 forward of one person, relative to its bound (>= 1 passes)."""
    d = person_dict(pi, torch.float64, wd)
    port = PosePort(fix)
    with torch.no_grad():
        orient, _ = port.poses(d)
        rel = float(gc.frame_margins(d['traj_local'].numpy(), pi['near']).min())
        if wd:      # the second aa -> quaternion -> aa round trip, on every frame of the scene
            base = d['smpl_orient_world_base']
            th2 = (base ** 2).sum(-1).numpy()
            w = d['world_dheading']
            q = tf.quat_mul(tf.aa_to_quat(torch.cat((torch.zeros([w.shape[0], 2], dtype=w.dtype), w), dim=-1)), tf.aa_to_quat(base)).numpy()
            c, s2 = q[:, 0], (q[:, 1:] ** 2).sum(-1)
            rel = min(rel, float(np.minimum(np.minimum(th2, s2) - 1e-6, np.abs(c)).min() / gc.MARGIN))
    return rel


_CASES = {}


def cases():
    """{name: case} and the screening statistics (generated, dropped).  A case: dict(S, P, T, persons {(si, pi): inputs}, seq_len, n_persons,
    frozen, fix, wd, var_mask, seed).  Built once; the first candidate seed that passes the screening is the case."""
    if not _CASES:
        generated = dropped = 0
        out = {}
        for ci, (base_name, spec) in enumerate(SPECS.items()):
            for wd in (False, True):
                name = base_name + ('_wd' if wd else '')
                for cand in range(CANDIDATES):
                    generated += 1
                    rng = np.random.default_rng(5000 + 100 * cand + 10 * ci)
                    persons, k = {}, 0
                    for si, (Ts, plist) in enumerate(spec['scenes']):
                        for pi, rng_ in enumerate(plist):
                            if rng_ is not None:
                                persons[(si, pi)] = _person_inputs(rng_[1] - rng_[0], Ts, rng_[0], 100 * cand + 10 * ci + k, spec['kind'], spec['fix'], rng)
                                k += 1
                    if all(_margin(p, spec['fix'], wd) >= 1.0 for p in persons.values()):
                        S, P = len(spec['scenes']), max(len(pl) for _, pl in spec['scenes'])
                        frozen = spec.get('frozen')
                        out[name] = dict(S=S, P=P, T=max(Ts for Ts, _ in spec['scenes']), persons=persons, seq_len=[Ts for Ts, _ in spec['scenes']],
                                         n_persons=[sum(r is not None for r in pl) for _, pl in spec['scenes']], frozen=frozen, fix=spec['fix'], wd=wd,
                                         var_mask=spec.get('var_mask', ALL_VARS), seed=cand)
                        break
                    dropped += 1
        _CASES.update(cases=out, generated=generated, dropped=dropped)
    return _CASES


def live(case):
    """The persons that receive a gradient: {(si, pi): inputs} without the frozen slots."""
    fr = case['frozen']
    return {k: v for k, v in case['persons'].items() if not (fr and fr[k[0] * case['P'] + k[1]])}


def layout(case):
    return packing.param_layout_py(case['P'], case['T'])


def block(case, si, pi):
    """Offset of a person's block in the flattened (S, scene_stride) arrays."""
    l = layout(case)
    return si * l['scene_stride'] + l['person0'] + pi * l['person_stride']


def host_arrays(case):
    """The batch's arrays (fp32 / int32 numpy) the VJP may read, with NaN wherever it must not: the camera block, the blocks of empty and frozen
    slots, parameter rows outside a range, prior and mask rows beyond it, base_orient inside it and at or beyond seq_len."""
    S, P, T = case['S'], case['P'], case['T']
    l = layout(case)
    a = dict(n_persons=np.asarray(case['n_persons'], np.int32), seq_len=np.asarray(case['seq_len'], np.int32), fr_start=np.zeros(S * P, np.int32),
             fr_end=np.ones(S * P, np.int32), traj_local_pred=np.full((S * P, T, 11), np.nan, np.float32), base_orient=np.full((S * P, T, 3), np.nan, np.float32),
             params=np.full((S, l['scene_stride']), np.nan, np.float32))
    if case['fix'] != DEFAULT_FIX:
        a['dheading_mask'] = np.full((S * P, T), np.nan, np.float32)
    if case['frozen']:
        a['frozen'] = np.asarray(case['frozen'], np.int32)
    flat = a['params'].reshape(-1)
    for (si, pi), p in case['persons'].items():
        slot, n, fs, Ts = si * P + pi, p['n'], p['fs'], p['Ts']
        a['fr_start'][slot], a['fr_end'][slot] = fs, fs + n
        if (si, pi) not in live(case):
            continue
        a['traj_local_pred'][slot, :n] = p['prior']
        a['base_orient'][slot, :fs] = p['base'][:fs]
        a['base_orient'][slot, fs + n:Ts] = p['base'][fs + n:]
        if 'dheading_mask' in a:
            a['dheading_mask'][slot, 1:n] = p['mask']
        pp, q = flat[block(case, si, pi):block(case, si, pi) + l['person_stride']], p['params']
        pp[l['local_xy']:l['local_xy'] + 2] = q['xy']
        pp[l['local_heading']] = q['heading'][0]
        pp[l['local_dxy']:l['local_dxy'] + 2 * T].reshape(T, 2)[1:n] = q['dxy']
        pp[l['local_dheading']:l['local_dheading'] + T][1:n] = q['dheading']
        pp[l['local_z']:l['local_z'] + T][:n] = q['z']
        pp[l['local_rot']:l['local_rot'] + 6 * T].reshape(T, 6)[:n] = q['rot']
        if case['wd']:
            pp[l['world_dheading']:l['world_dheading'] + T][:Ts] = q['world_dheading'][:, 0]
    return a


def stage_desc(case, flags=None, var_mask=None):
    sd = _lib.StageDesc()
    sd.var_mask = case['var_mask'] if var_mask is None else var_mask
    sd.flags = (packing.FLAG_HAS_WORLD_DHEADING if case['wd'] else 0) if flags is None else flags
    return sd


def scene_batch(case, pointers):
    """glamr_scene_batch of the case; pointers: {array name: address} (host or device)."""
    sb = _lib.SceneBatch()
    sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = case['S'], case['P'], case['T'], packing.NJ
    for k, v in pointers.items():
        setattr(sb, k, ctypes.c_void_p(v))
    return sb


def upstream(case, pattern, nan_pad=True, scale=1.0):
    """(G_o, G_t) fp32 (S * P, T, 3), None for an array the pattern does not give.  nan_pad: NaN in every row the VJP must not read -- frames at
    or beyond seq_len, empty and frozen slots, and outside the existing range everything but G_o under world_dheading."""
    S, P, T = case['S'], case['P'], case['T']
    rng = np.random.default_rng(11 + T + 31 * S * P)
    G_o, G_t = (rng.normal(size=(S * P, T, 3)).astype(np.float32) for _ in range(2))
    if pattern == 'onehot':      # the longest path back to row 0
        G_t[:] = 0.0
        for (si, pi), p in case['persons'].items():
            G_t[si * P + pi, p['fs'] + p['n'] - 1, 0] = 1.0
    out = []
    for g, is_orient in ((G_o, True), (G_t, False)):
        if pattern == ('trans' if is_orient else 'orient') or (is_orient and pattern == 'onehot'):
            out.append(None)
            continue
        g = g * np.float32(scale)
        if nan_pad:
            keep = np.zeros((S * P, T), bool)
            for (si, pi), p in live(case).items():
                if is_orient and case['wd']:
                    keep[si * P + pi, :p['Ts']] = True
                else:
                    keep[si * P + pi, p['fs']:p['fs'] + p['n']] = True
            g[~keep] = np.nan
        out.append(g)
    return tuple(out)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def reference(case, pattern, dtype=torch.float64, mut=None, scale=1.0):
    """dL/d params (S * scene_stride,) as fp64 numbers by autograd in `dtype`, zero wherever the VJP writes nothing."""
    P, T = case['P'], case['T']
    l = layout(case)
    G_o, G_t = upstream(case, pattern, nan_pad=False, scale=scale)
    out = np.zeros(case['S'] * l['scene_stride'], np.float64)
    vm = ALL_VARS if mut == 'var_mask' else case['var_mask']
    port = PosePort(case['fix'], mut)
    for (si, pi), p in live(case).items():
        slot, n, fs, Ts = si * P + pi, p['n'], p['fs'], p['Ts']
        d = person_dict(p, dtype, case['wd'])
        orient, trans = port.poses(d)
        rows = slice(0, Ts) if case['wd'] else slice(fs, fs + n)
        loss = 0.0
        if G_o is not None:
            loss = loss + (torch.tensor(G_o[slot, rows], dtype=dtype) * orient[rows]).sum()
        if G_t is not None:
            loss = loss + (torch.tensor(G_t[slot, fs:fs + n], dtype=dtype) * trans[fs:fs + n]).sum()
            if mut == 'outside':      # the frames after / before the range as if they held the last / first existing pose
                g = torch.tensor(G_t[slot], dtype=dtype)
                loss = loss + (g[fs + n:Ts] * trans[fs + n - 1]).sum() + (g[:fs] * trans[fs]).sum()
        leaves = {k: d['traj_local_' + k] for k in ('xy', 'heading', 'dxy', 'dheading', 'z', 'rot')}
        if case['wd']:
            leaves['world_dheading'] = d['world_dheading']
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        g = {k: (np.zeros(tuple(v.shape)) if gr is None else gr.double().numpy()) for (k, v), gr in zip(leaves.items(), grads)}
        pp = out[block(case, si, pi):block(case, si, pi) + l['person_stride']]
        on = lambda name: bool(vm & VB[name])
        if on('local_xy'):
            pp[l['local_xy']:l['local_xy'] + 2] = g['xy']
        if on('local_heading'):
            pp[l['local_heading']] = g['heading'][0]
        if on('local_dxy'):
            pp[l['local_dxy']:l['local_dxy'] + 2 * T].reshape(T, 2)[1:n] = g['dxy']
        if on('local_dheading'):
            pp[l['local_dheading']:l['local_dheading'] + T][1:n] = g['dheading']
        if on('local_z'):
            pp[l['local_z']:l['local_z'] + T][:n] = g['z']
        if on('local_rot'):
            pp[l['local_rot']:l['local_rot'] + 6 * T].reshape(T, 6)[:n] = g['rot']
        if case['wd'] and on('world_dheading'):
            pp[l['world_dheading']:l['world_dheading'] + T][:Ts] = g['world_dheading'][:, 0]
    return out


def group_slices(case):
    l, T = layout(case), case['T']
    return {'xy': [slice(l['local_xy'], l['local_xy'] + 2), slice(l['local_dxy'], l['local_dxy'] + 2 * T)], 'z': [slice(l['local_z'], l['local_z'] + T)],
            'rot': [slice(l['local_rot'], l['local_rot'] + 6 * T)],
            'heading': [slice(l['local_heading'], l['local_heading'] + 1), slice(l['local_dheading'], l['local_dheading'] + T)],
            'world_dheading': [slice(l['world_dheading'], l['world_dheading'] + T)]}


def person_errors(case, got, ref, key):
    """Error per variable group of one person, relative to the person's largest reference entry of the group."""
    l = layout(case)
    b = block(case, *key)
    g, r = np.asarray(got, np.float64).reshape(-1)[b:b + l['person_stride']], np.asarray(ref, np.float64).reshape(-1)[b:b + l['person_stride']]
    out = {}
    for k, sl in group_slices(case).items():
        gg, rr = np.concatenate([g[s] for s in sl]), np.concatenate([r[s] for s in sl])
        scale = np.abs(rr).max()
        out[k] = float(np.abs(gg - rr).max() / (scale if scale > 0 else 1.0))
    return out


def errors(case, got, ref):
    """Worst error over the persons per variable group."""
    out = {k: 0.0 for k in GROUPS}
    for key in live(case):
        e = person_errors(case, got, ref, key)
        out = {k: max(out[k], e[k]) for k in out}
    return out


def written_mask(case):
    """True for every entry of the flattened gradient array some variable of a live person owns (everything else must come back zero in
    store mode and untouched in add mode)."""
    l, T = layout(case), case['T']
    m = np.zeros(case['S'] * l['scene_stride'], bool)
    vm = case['var_mask']
    for (si, pi), p in live(case).items():
        n, Ts = p['n'], p['Ts']
        pp = m[block(case, si, pi):block(case, si, pi) + l['person_stride']]
        pp[l['local_xy']:l['local_xy'] + 2] = bool(vm & VB['local_xy'])
        pp[l['local_heading']] = bool(vm & VB['local_heading'])
        pp[l['local_dxy'] + 2:l['local_dxy'] + 2 * n] = bool(vm & VB['local_dxy'])
        if case['fix'] != DEFAULT_FIX:
            pp[l['local_dheading'] + 1:l['local_dheading'] + n] = bool(vm & VB['local_dheading'])
        pp[l['local_z']:l['local_z'] + n] = bool(vm & VB['local_z'])
        pp[l['local_rot']:l['local_rot'] + 6 * n] = bool(vm & VB['local_rot'])
        if case['wd']:
            pp[l['world_dheading']:l['world_dheading'] + Ts] = bool(vm & VB['world_dheading'])
    return m


_REF = {}


def ref64(name, pattern):
    """The fp64 reference of a case, computed once and left unchanged."""
    if (name, pattern) not in _REF:
        _REF[(name, pattern)] = reference(cases()['cases'][name], pattern)
    return _REF[(name, pattern)]


def measure_floor(name):
    """fp32 autograd against fp64, worst over the upstream patterns and the scaled runs, per group (one thread: the rounding does not depend on the machine's cores)."""
    from tests.traj_ref_common import single_thread
    case = cases()['cases'][name]
    acc = {k: 0.0 for k in GROUPS}
    with single_thread():
        for pattern in PATTERNS:
            e = errors(case, reference(case, pattern, torch.float32), ref64(name, pattern))
            acc = {k: max(acc[k], e[k]) for k in GROUPS}
        for scale in SCALES:      # the scaled runs are compared within the same tolerances, so they are part of the floor
            e = errors(case, reference(case, 'all', torch.float32, scale=scale), reference(case, 'all', scale=scale))
            acc = {k: max(acc[k], e[k]) for k in GROUPS}
    return acc


# fp32 autograd of the port against fp64 (one thread), rounded up to two digits; tests/test_extra_loss_ref.py measures them again
FLOOR = {
    'one24':     {'xy': 7.1e-08, 'z': 0.0e+00, 'rot': 2.4e-07, 'heading': 1.4e-07, 'world_dheading': 0.0e+00},      # 6.755e-08, 0.000e+00, 2.251e-07, 1.356e-07, 0.000e+00
    'one24_wd':  {'xy': 7.3e-08, 'z': 0.0e+00, 'rot': 2.9e-07, 'heading': 2.9e-07, 'world_dheading': 2.4e-07},      # 6.944e-08, 0.000e+00, 2.741e-07, 2.758e-07, 2.264e-07
    'two':       {'xy': 9.1e-07, 'z': 0.0e+00, 'rot': 3.6e-07, 'heading': 7.5e-07, 'world_dheading': 0.0e+00},      # 8.630e-07, 0.000e+00, 3.431e-07, 7.127e-07, 0.000e+00
    'two_wd':    {'xy': 9.1e-07, 'z': 0.0e+00, 'rot': 4.5e-07, 'heading': 7.5e-07, 'world_dheading': 4.4e-07},      # 8.630e-07, 0.000e+00, 4.258e-07, 7.127e-07, 4.213e-07
    'T257':      {'xy': 1.7e-05, 'z': 0.0e+00, 'rot': 4.6e-06, 'heading': 6.7e-06, 'world_dheading': 0.0e+00},      # 1.606e-05, 0.000e+00, 4.403e-06, 6.373e-06, 0.000e+00
    'T257_wd':   {'xy': 8.7e-06, 'z': 0.0e+00, 'rot': 3.2e-06, 'heading': 3.8e-06, 'world_dheading': 1.7e-06},      # 8.306e-06, 0.000e+00, 3.050e-06, 3.621e-06, 1.588e-06
    'single':    {'xy': 0.0e+00, 'z': 0.0e+00, 'rot': 2.9e-07, 'heading': 2.4e-07, 'world_dheading': 0.0e+00},      # 0.000e+00, 0.000e+00, 2.740e-07, 2.247e-07, 0.000e+00
    'single_wd': {'xy': 0.0e+00, 'z': 0.0e+00, 'rot': 2.9e-07, 'heading': 1.2e-07, 'world_dheading': 2.1e-07},      # 0.000e+00, 0.000e+00, 2.799e-07, 1.108e-07, 1.986e-07
    'batch':     {'xy': 1.4e-06, 'z': 0.0e+00, 'rot': 4.8e-07, 'heading': 1.4e-06, 'world_dheading': 0.0e+00},      # 1.356e-06, 0.000e+00, 4.614e-07, 1.364e-06, 0.000e+00
    'batch_wd':  {'xy': 1.4e-06, 'z': 0.0e+00, 'rot': 4.8e-07, 'heading': 1.4e-06, 'world_dheading': 5.6e-07},      # 1.356e-06, 0.000e+00, 4.574e-07, 1.364e-06, 5.339e-07
    'frozen':    {'xy': 6.6e-08, 'z': 0.0e+00, 'rot': 4.3e-07, 'heading': 3.5e-07, 'world_dheading': 0.0e+00},      # 6.321e-08, 0.000e+00, 4.094e-07, 3.365e-07, 0.000e+00
    'frozen_wd': {'xy': 6.6e-08, 'z': 0.0e+00, 'rot': 3.2e-07, 'heading': 3.7e-07, 'world_dheading': 2.3e-07},      # 6.321e-08, 0.000e+00, 3.038e-07, 3.520e-07, 2.168e-07
    'norot':     {'xy': 1.0e-06, 'z': 0.0e+00, 'rot': 0.0e+00, 'heading': 7.5e-07, 'world_dheading': 0.0e+00},      # 9.721e-07, 0.000e+00, 0.000e+00, 7.156e-07, 0.000e+00
    'norot_wd':  {'xy': 1.0e-06, 'z': 0.0e+00, 'rot': 0.0e+00, 'heading': 7.5e-07, 'world_dheading': 3.9e-07},      # 9.721e-07, 0.000e+00, 0.000e+00, 7.156e-07, 3.739e-07
}


def tol(name):
    return {k: FLOOR_FACTOR * v for k, v in FLOOR[name].items()}


if __name__ == '__main__':
    st = cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    for name in st['cases']:
        f = measure_floor(name)
        up = {k: (0.0 if v == 0 else float('%.1e' % (v * 1.05))) for k, v in f.items()}
        print("    %-12s {%s},      # %s" % ("'%s':" % name, ', '.join("'%s': %.1e" % (k, up[k]) for k in GROUPS), ', '.join('%.3e' % f[k] for k in GROUPS)))
