"""fp64 reference of the camera VJP glamr_grecon_cam_backward computes (csrc/grecon_cam_bwd.hpp): torch autograd of the camera
block of oracle.port.grecon.GlobalReconOptimizer.forward (its lines for global_recon_model.py:473-508, run as they stand with the persons'
world poses given as leaves) for L = sum(G * cam_pose[:, :3, :4]), scattered into the layout of the stage kernel's gradient array and into
pose-gradient arrays shaped like orient_world / trans_world.  Cases, inputs, screening, upstream patterns, mutations and tolerances of
tests/test_extra_loss_cam_ref.py (CPU: the header on the host runtime) and tests/test_extra_loss_cam_gpu.py (the kernel).

Inputs: a camera's 6D is the first two columns of the MEAN of two generic rotations (not orthonormal, as the averaged transform of two persons
is); person orientations are generic axis-angles of angle 0.3 .. 2.8 with every fifth frame 1e-2 from angle pi; person2cam puts every person's camera within 0.3 rad and 0.1 m of the scene's (the averaged transform of
two persons is not orthonormal, but no more degenerate than init_data leaves it);
translations randn, the residuals randn x 1e-2 (the sizes Adam reaches).  Screening (as tests/extra_loss_common.py: every branch condition at
least global_vjp_common.MARGIN from switching in the fp64 forward): the Taylor switch theta^2 > 1e-6 of aa_to_rotmat and the two clamped norms
of the Gram-Schmidt step.

Tolerances follow the project's rule: FLOOR_FACTOR = 16 x the error of the SAME autograd run in float32 against float64, per gradient group,
relative to the group's largest reference entry within the scene (parameter groups) or person (pose groups); per case the worst over the upstream
patterns and the scaled runs.  The floors are constants below (`python -m tests.extra_loss_cam_common` prints them); the CPU test measures them
again and fails outside [1/2, 2] x the constant.  A floor of exactly 0 (cam_trans of the per-frame camera is a copy of G's fourth column) asks
for the exact result."""
import ctypes
import types

import numpy as np
import torch

from oracle.port import transforms as tf
from oracle.port.grecon import GlobalReconOptimizer
from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests.global_vjp_common import MARGIN

FLOOR_FACTOR = 16
PARAM_GROUPS = ('cam_rot6d', 'cam_trans', 'cam_inv_rot_res', 'cam_inv_trans_res')
POSE_GROUPS = ('g_orient_world', 'g_trans_world')
GROUPS = PARAM_GROUPS + POSE_GROUPS
PATTERNS = ('all', 'rot', 'trans', 'onehot')
SCALES = (1e-6, 1e5)      # G x scale: the VJP is plain fp32 and linear in G
CANDIDATES = 4
MAX_DROPPED_SHARE = 0.25
VB = packing.VAR_BITS
PERSON_VARS = VB['local_xy'] | VB['local_heading'] | VB['local_dxy'] | VB['local_rot'] | VB['local_z'] | VB['local_dheading']
MODE_DESC = {'frame': (VB['cam'] | PERSON_VARS, 0), 'fixed': (VB['cam'] | PERSON_VARS, packing.FLAG_FIXED_CAM),
             'derived': (PERSON_VARS, packing.FLAG_CAM_FROM_PERSON), 'constant': (PERSON_VARS, 0)}      # (var_mask, flags)


def _vis(T, spans):
    v = np.zeros(T, bool)
    for s, e in spans:
        v[s:e] = True
    return v


# scenes: (seq_len, [visible spans of a person | None = empty slot, ...]); the optimised modes carry no persons
SPECS = {
    'frame24': dict(mode='frame', scenes=[(24, [])]),
    'frame257': dict(mode='frame', scenes=[(257, [])]),                                    # two frames on thread 0
    'frame1': dict(mode='frame', scenes=[(1, [])]),
    'frame_batch': dict(mode='frame', scenes=[(20, []), (13, [])]),                        # one scene shorter than max_len
    'fixed24': dict(mode='fixed', scenes=[(24, [])]),
    'fixed257': dict(mode='fixed', scenes=[(257, [])]),                                    # the reduction across the thread wrap
    'fixed_short': dict(mode='fixed', scenes=[(16, []), (11, [])]),                        # NaN in the padding rows of g_cam_pose
    # leading person-less frames 0-3, one person 4-9, two 10-14, interior run 15-20, person 1 alone 21-29 (person 0 exists but is not visible
    # there: its poses are NaN), two 30-33, trailing run 34-39
    'derived40': dict(mode='derived', scenes=[(40, [[(4, 15), (30, 34)], [(10, 15), (21, 34)], None])]),
    'derived257': dict(mode='derived', scenes=[(257, [[(2, 250)], [(100, 180)]])]),        # a person-less run across frame 256
    'derived_single': dict(mode='derived', scenes=[(8, [[(5, 6)]])]),                      # one visible frame
    'derived_frozen': dict(mode='derived', scenes=[(20, [[(3, 9), (12, 17)], [(0, 20)]])], frozen=[0, 1]),
}
CASE_NAMES = list(SPECS)

MUTATIONS = {'lead0': 'leading person-less frames sourced from frame 0', 'rot_all': 'the rotation residual applied on every frame',
             'trans_empty': 'the translation residual applied only on person-less frames', 'div_nt': 'division by n[t] instead of n[src]',
             'invis': 'invisible persons counted', 'fixed0': "the fixed camera taking frame 0's gradient only",
             'inv_nocouple': "the inverse's backward without the rotation-translation coupling"}


def _graft(value, grad_of):
    """`value`'s numbers with `grad_of`'s gradient."""
    return value.detach() + (grad_of - grad_of.detach())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _rand_rot(rng, n):
    q = rng.normal(size=(n, 4))
    return tf.quat_to_rotmat(torch.tensor(q / np.linalg.norm(q, axis=-1, keepdims=True))).numpy()


def _orient(rng, n):
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    ang = rng.uniform(0.3, 2.8, size=n)
    ang[::5] = np.pi - 1e-2 * rng.uniform(0.4, 1.0, size=len(ang[::5]))
    return axis * ang[:, None]


def _scene_inputs(Ts, plist, mode, rng):
    f32 = lambda a: np.asarray(a, np.float32)
    sc = dict(Ts=Ts, persons={})
    if mode in ('frame', 'fixed'):
        R = 0.5 * (_rand_rot(rng, Ts) + np.einsum('tij,tjk->tik', _rand_rot(rng, Ts), _rand_rot(rng, Ts)))
        sc['cam_rot6d'] = f32(np.concatenate([R[:, :, 0], R[:, :, 1]], axis=-1))
        sc['cam_trans'] = f32(rng.normal(size=(Ts, 3)))
    else:
        sc['rot_res'] = f32(rng.normal(size=(Ts, 6)) * 1e-2)
        sc['trans_res'] = f32(rng.normal(size=(Ts, 3)) * 1e-2)
        c2w = tf.make_transform(torch.tensor(_rand_rot(rng, Ts)), torch.tensor(rng.normal(size=(Ts, 3))))
        for pi, spans in enumerate(plist):
            if spans is None:
                continue
            # person2cam = person_world^-1 . (the scene's camera-to-world) . (a person's own error: 0.3 rad, 0.1 m), as init_data leaves it
            orient, trans = f32(_orient(rng, Ts)), f32(rng.normal(size=(Ts, 3)))
            axis = rng.normal(size=(Ts, 3))
            err = tf.make_transform(torch.tensor(0.3 * axis / np.linalg.norm(axis, axis=-1, keepdims=True)), torch.tensor(0.1 * rng.normal(size=(Ts, 3))), 'axis_angle')
            world = tf.make_transform(torch.tensor(orient, dtype=torch.float64), torch.tensor(trans, dtype=torch.float64), 'axis_angle')
            p2c = torch.matmul(torch.matmul(torch.linalg.inv(world), c2w), err)[:, :3].numpy()
            sc['persons'][pi] = dict(vis=_vis(Ts, spans), orient=orient, trans=trans, person2cam=f32(p2c))
    return sc


def _margin(case, sc):
    """Smallest distance of a branch condition from switching in the fp64 forward of one scene, relative to MARGIN (>= 1 passes)."""
    rel = np.inf
    for p in sc['persons'].values():
        th2 = (p['orient'].astype(np.float64) ** 2).sum(-1)[p['vis']]
        if th2.size:
            rel = min(rel, float(np.abs(th2 - 1e-6).min() / MARGIN))
    if case['mode'] == 'derived':
        with torch.no_grad():
            r6 = cam_block(case, sc, leaves(case, sc, torch.float64), '')[1]['r6'].numpy()
    else:
        r6 = sc['cam_rot6d'].astype(np.float64)
    a1, a2 = r6[:, :3], r6[:, 3:]
    n1 = np.linalg.norm(a1, axis=-1)
    u = a2 - (a1 * a2).sum(-1, keepdims=True) * a1 / n1[:, None] ** 2
    return min(rel, float(min(n1.min(), np.linalg.norm(u, axis=-1).min()) / MARGIN))


_CASES = {}


def cases():
    """{name: case} and the screening statistics (generated, dropped).  A case: dict(name, mode, S, P, T, scenes [inputs], seq_len, n_persons,
    frozen, seed).  Built once; the first candidate seed that passes the screening is the case."""
    if not _CASES:
        generated = dropped = 0
        out = {}
        for ci, (name, spec) in enumerate(SPECS.items()):
            S, P = len(spec['scenes']), max(1, max(len(pl) for _, pl in spec['scenes']))
            for cand in range(CANDIDATES):
                generated += 1
                rng = np.random.default_rng(7000 + 100 * cand + 10 * ci)
                case = dict(name=name, mode=spec['mode'], S=S, P=P, T=max(Ts for Ts, _ in spec['scenes']), seq_len=[Ts for Ts, _ in spec['scenes']],
                            n_persons=[max(1, sum(r is not None for r in pl)) for _, pl in spec['scenes']], frozen=spec.get('frozen'), seed=cand)
                case['scenes'] = [_scene_inputs(Ts, pl, spec['mode'], rng) for Ts, pl in spec['scenes']]
                if all(_margin(case, sc) >= 1.0 for sc in case['scenes']):
                    out[name] = case
                    break
                dropped += 1
        _CASES.update(cases=out, generated=generated, dropped=dropped)
    return _CASES


def live(case, si):
    """The persons of a scene that take part: {pi: inputs} without the frozen slots."""
    fr = case['frozen']
    return {pi: p for pi, p in case['scenes'][si]['persons'].items() if not (fr and fr[si * case['P'] + pi])}


def layout(case):
    return packing.param_layout_py(case['P'], case['T'])


def n_visible(case, si):
    sc = case['scenes'][si]
    return sum([p['vis'].astype(np.int64) for p in live(case, si).values()], np.zeros(sc['Ts'], np.int64))


def host_arrays(case):
    """The batch's arrays (fp32 / int32 numpy) the VJP may read, with NaN wherever it must not: the parameter blocks of the other camera modes
    and of the persons, rows at or beyond seq_len, the rotation residual where a person is visible; orient_world / trans_world / person2cam of
    empty and frozen slots and at frames where the person is not visible."""
    S, P, T = case['S'], case['P'], case['T']
    l = layout(case)
    a = dict(n_persons=np.asarray(case['n_persons'], np.int32), seq_len=np.asarray(case['seq_len'], np.int32), params=np.full((S, l['scene_stride']), np.nan, np.float32))
    if case['mode'] == 'derived':
        a.update(vis=np.full((S * P, T), np.nan, np.float32), orient_world=np.full((S * P, T, 3), np.nan, np.float32),
                 trans_world=np.full((S * P, T, 3), np.nan, np.float32), person2cam=np.full((S * P, T, 12), np.nan, np.float32))
        if case['frozen']:
            a['frozen'] = np.asarray(case['frozen'], np.int32)
    for si, sc in enumerate(case['scenes']):
        Ts, pp = sc['Ts'], a['params'][si]
        if case['mode'] == 'frame':
            pp[l['cam_rot6d']:l['cam_rot6d'] + 6 * Ts] = sc['cam_rot6d'].reshape(-1)
            pp[l['cam_trans']:l['cam_trans'] + 3 * Ts] = sc['cam_trans'].reshape(-1)
        elif case['mode'] == 'fixed':
            pp[l['cam_rot6d']:l['cam_rot6d'] + 6] = sc['cam_rot6d'][0]
            pp[l['cam_trans']:l['cam_trans'] + 3] = sc['cam_trans'][0]
        else:
            n = n_visible(case, si)
            pp[l['cam_inv_rot_res']:l['cam_inv_rot_res'] + 6 * Ts].reshape(Ts, 6)[n == 0] = sc['rot_res'][n == 0]
            pp[l['cam_inv_trans_res']:l['cam_inv_trans_res'] + 3 * Ts] = sc['trans_res'].reshape(-1)
            for pi, p in live(case, si).items():
                slot, v = si * P + pi, p['vis']
                a['vis'][slot, :Ts] = v
                a['orient_world'][slot, :Ts][v] = p['orient'][v]
                a['trans_world'][slot, :Ts][v] = p['trans'][v]
                a['person2cam'][slot, :Ts][v] = p['person2cam'][v].reshape(-1, 12)
    return a


def stage_desc(case, mode=None):
    sd = _lib.StageDesc()
    sd.var_mask, sd.flags = MODE_DESC[case['mode'] if mode is None else mode]
    return sd


def scene_batch(case, pointers):
    """glamr_scene_batch of the case; pointers: {array name: address} (host or device)."""
    sb = _lib.SceneBatch()
    sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = case['S'], case['P'], case['T'], packing.NJ
    for k, v in pointers.items():
        setattr(sb, k, ctypes.c_void_p(v))
    return sb


def upstream(case, pattern, nan_pad=True, scale=1.0):
    """G fp32 (S, T, 12).  nan_pad: NaN in the rows at or beyond seq_len."""
    S, T = case['S'], case['T']
    G = np.random.default_rng(13 + T + 31 * S).normal(size=(S, T, 3, 4)).astype(np.float32)
    if pattern == 'rot':
        G[..., 3] = 0.0
    elif pattern == 'trans':
        G[..., :3] = 0.0
    elif pattern == 'onehot':      # the last frame's translation: in the derived cases the end of the trailing run
        G[:] = 0.0
        for si, Ts in enumerate(case['seq_len']):
            G[si, Ts - 1, 0, 3] = 1.0
    G = G * np.float32(scale)
    if nan_pad:
        for si, Ts in enumerate(case['seq_len']):
            G[si, Ts:] = np.nan
    return G.reshape(S, T, 12)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
class CamPort(GlobalReconOptimizer):
    """The port's optimiser cut down to its forward with the trajectory step and the body model taken out: what remains is make_transform on
    the given poses and the camera block (oracle/port/grecon.py:433-462), run as it stands."""

    def __init__(self, mode):      # (nothing else of the base class's state is needed)
        self.device, self.flag_opt_traj, self.flag_opt_cam, self.flag_cam_inv_trans_res_all = 'cpu', False, True, True
        self.flag_fixed_cam, self.flag_cam_from_person = mode == 'fixed', mode == 'derived'
        self.smpl = lambda **kw: types.SimpleNamespace(joints=kw['root_trans'][:, None])

    def pred_trajectory_base(self, d):
        pass


def scene_index(case, sc):
    return [s is sc for s in case['scenes']].index(True)


def leaves(case, sc, dtype, mut=None):
    """The leaves of one scene in `dtype`: the camera parameters of the mode, or the residuals and every live person's pose.  mut 'rot_all':
    the rotation residual has a row for EVERY frame (zero where a person is visible, so the numbers stay)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True)
    if case['mode'] == 'frame':
        return dict(cam_rot6d=t(sc['cam_rot6d']), cam_trans=t(sc['cam_trans']))
    if case['mode'] == 'fixed':
        return dict(cam_rot6d=t(sc['cam_rot6d'][:1]), cam_trans=t(sc['cam_trans'][:1]))
    si = scene_index(case, sc)
    n = n_visible(case, si)
    lv = dict(rot_res=t(sc['rot_res'] * (n == 0)[:, None] if mut == 'rot_all' else sc['rot_res'][n == 0]), trans_res=t(sc['trans_res']))
    for pi, p in live(case, si).items():
        lv['orient%d' % pi], lv['trans%d' % pi] = t(p['orient']), t(p['trans'])
    return lv


def cam_block(case, sc, lv, mut=None):
    """(cam_pose (Ts, 4, 4), the port's data dictionary) of one scene from its leaves: the port's forward (mut None), or the restated block
    (mut '' = unchanged) with one mutation."""
    dtype, Ts, mode = lv[next(iter(lv))].dtype, sc['Ts'], case['mode']
    si = scene_index(case, sc)
    cst = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    data = dict(cam_pose=torch.zeros(Ts, 4, 4, dtype=dtype), person_data={})
    if mode == 'frame':
        data.update(cam_rot_6d=lv['cam_rot6d'], cam_trans=lv['cam_trans'])
    elif mode == 'fixed':
        data.update(cam_rot_6d_fix=lv['cam_rot6d'], cam_trans_fix=lv['cam_trans'])
    else:
        vis = {pi: (np.ones(Ts) if mut == 'invis' else p['vis'].astype(np.float64)) for pi, p in live(case, si).items()}
        data.update(fr_num_persons=cst(sum(vis.values())), cam_inv_rot_residual=lv['rot_res'], cam_inv_trans_residual=lv['trans_res'])
        for pi, p in live(case, si).items():
            data['person_data'][pi] = dict(smpl_orient_world=lv['orient%d' % pi], root_trans_world=lv['trans%d' % pi], vis_frames=cst(vis[pi]),
                                           person2cam=cst(np.concatenate([p['person2cam'], np.tile([[[0, 0, 0, 1.0]]], (Ts, 1, 1))], axis=1)),
                                           smpl_pose=None, smpl_beta=None, cam_K=torch.eye(3, dtype=dtype).repeat(Ts, 1, 1))
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(dtype)
        if mut is None:
            CamPort(mode).forward(data, ['cam'] if mode != 'derived' else [], {'stage': 'test'})
        else:
            _restated_block(data, mode, mut, cst(n_visible(case, si)))
    finally:
        torch.set_default_dtype(old)
    return data['cam_pose'], data


def _restated_block(data, mode, mut, n_true):
    """The port's camera block restated (tests/test_extra_loss_cam_ref.py holds it to the port's own with mut = ''), with one
    mutation.  n_true: the unmutated person counts (which residual rows exist)."""
    T = data['cam_pose'].shape[0]
    if mode != 'derived':
        r6, tr = (data['cam_rot_6d'], data['cam_trans']) if mode == 'frame' else (data['cam_rot_6d_fix'].expand(T, -1), data['cam_trans_fix'].expand(T, -1))
        if mut == 'fixed0' and mode == 'fixed':      # only frame 0 sends its gradient to the shared row
            keep = torch.zeros(T, 1, dtype=r6.dtype)
            keep[0] = 1.0
            r6, tr = _graft(r6, r6 * keep), _graft(tr, tr * keep)
        data['cam_pose'] = tf.make_transform(r6, tr, '6d')
        return
    npers = data['fr_num_persons']
    ind = npers > 0
    per = [torch.matmul(tf.make_transform(d['smpl_orient_world'], d['root_trans_world'], 'axis_angle'), d['person2cam']) * d['vis_frames'][:, None, None]
           for d in data['person_data'].values()]
    inv = torch.zeros_like(data['cam_pose'])
    inv[ind] = sum(per)[ind] / npers[ind, None, None]
    first = int(torch.where(ind)[0][0])
    src, last = torch.zeros(T, dtype=torch.long), first
    for i in range(T):
        if npers[i] > 0:
            last = i
        src[i] = last
    inv = inv[src]
    if mut == 'lead0':      # the leading frames' gradient goes to frame 0's (empty) average: lost
        inv = torch.where((torch.arange(T) < first)[:, None, None], inv.detach(), inv)
    if mut == 'div_nt':     # the fold divides by the count of the frame itself (a zero count taken as 1)
        inv = _graft(inv, inv * (npers[src] / npers.clamp(min=1.0))[:, None, None])
    r6 = tf.rotmat_to_6d(inv[:, :3, :3])
    res = data['cam_inv_rot_residual']
    if res.shape[0] != T or mut != 'rot_all':
        full = torch.zeros_like(r6)
        full[n_true == 0] = res
        res = full
    r6 = r6 + res
    data['r6'] = r6.detach()
    tres = data['cam_inv_trans_residual']
    if mut == 'trans_empty':
        tres = _graft(tres, tres * (npers == 0)[:, None].to(tres.dtype))
    out = torch.zeros_like(inv)
    out[:, :3, :3], out[:, :3, 3], out[:, 3, 3] = tf.sixd_to_rotmat(r6), inv[:, :3, 3] + tres, 1.0
    data['cam_pose_inv'] = out
    if mut == 'inv_nocouple':      # the translation of the inverse does not reach the rotation
        o = torch.zeros_like(out)
        o[:, :3, :3] = out[:, :3, :3].transpose(-2, -1)
        o[:, :3, 3] = -torch.matmul(out[:, :3, 3].unsqueeze(-2), out[:, :3, :3].detach()).squeeze(-2)
        o[:, 3, 3] = 1.0
        data['cam_pose'] = o
    else:
        data['cam_pose'] = tf.invert_transform(out)


def touches(mut, case, si):
    """Whether the mutation changes the gradient of this scene at all."""
    Ts = case['scenes'][si]['Ts']
    if case['mode'] != 'derived':
        return mut == 'fixed0' and case['mode'] == 'fixed' and Ts > 1
    n = n_visible(case, si)
    if mut == 'lead0':
        return n[0] == 0
    if mut in ('rot_all', 'trans_empty'):
        return bool((n > 0).any())
    if mut == 'div_nt':
        src = np.maximum.accumulate(np.where(n > 0, np.arange(Ts), -1))
        return bool(((n == 0) & (src >= 0) & (n[np.maximum(src, 0)] > 1)).any())
    if mut == 'invis':
        return any(not p['vis'].all() for p in live(case, si).values())
    return mut == 'inv_nocouple'


def reference(case, pattern, dtype=torch.float64, mut=None, scale=1.0):
    """dict(grads (S * scene_stride,), g_orient_world, g_trans_world (S * P, T, 3)) as fp64 numbers by autograd in `dtype`, zero wherever the
    VJP writes nothing."""
    S, P, T = case['S'], case['P'], case['T']
    l = layout(case)
    G = upstream(case, pattern, nan_pad=False, scale=scale).reshape(S, T, 3, 4)
    out = dict(grads=np.zeros((S, l['scene_stride']), np.float64), g_orient_world=np.zeros((S * P, T, 3), np.float64), g_trans_world=np.zeros((S * P, T, 3), np.float64))
    for si, sc in enumerate(case['scenes']):
        Ts = sc['Ts']
        lv = leaves(case, sc, dtype, mut)
        cam, _ = cam_block(case, sc, lv, mut)
        loss = (torch.tensor(G[si, :Ts], dtype=dtype) * cam[:, :3, :4]).sum()
        grads = torch.autograd.grad(loss, list(lv.values()), allow_unused=True)
        g = {k: (np.zeros(tuple(v.shape)) if gr is None else gr.double().numpy()) for (k, v), gr in zip(lv.items(), grads)}
        pp = out['grads'][si]
        if case['mode'] == 'derived':
            n = n_visible(case, si)
            rr = pp[l['cam_inv_rot_res']:l['cam_inv_rot_res'] + 6 * Ts].reshape(Ts, 6)
            if mut == 'rot_all':
                rr[:] = g['rot_res']
            else:
                rr[n == 0] = g['rot_res']
            pp[l['cam_inv_trans_res']:l['cam_inv_trans_res'] + 3 * Ts] = g['trans_res'].reshape(-1)
            for pi in live(case, si):
                out['g_orient_world'][si * P + pi, :Ts] = g['orient%d' % pi]
                out['g_trans_world'][si * P + pi, :Ts] = g['trans%d' % pi]
        else:
            rows = Ts if case['mode'] == 'frame' else 1
            pp[l['cam_rot6d']:l['cam_rot6d'] + 6 * rows] = g['cam_rot6d'].reshape(-1)
            pp[l['cam_trans']:l['cam_trans'] + 3 * rows] = g['cam_trans'].reshape(-1)
    out['grads'] = out['grads'].reshape(-1)
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------
def group_slices(case):
    l, T = layout(case), case['T']
    return {'cam_rot6d': slice(l['cam_rot6d'], l['cam_rot6d'] + 6 * T), 'cam_trans': slice(l['cam_trans'], l['cam_trans'] + 3 * T),
            'cam_inv_rot_res': slice(l['cam_inv_rot_res'], l['cam_inv_rot_res'] + 6 * T), 'cam_inv_trans_res': slice(l['cam_inv_trans_res'], l['cam_inv_trans_res'] + 3 * T)}


def _rel(g, r):
    scale = np.abs(r).max() if r.size else 0.0
    return float(np.abs(g - r).max() / (scale if scale > 0 else 1.0)) if r.size else 0.0


def scene_errors(case, got, ref, si):
    """Error per group of one scene: parameter groups relative to the scene's largest reference entry of the group, pose groups relative to
    the person's (the worst over its persons)."""
    l, P = layout(case), case['P']
    g, r = (np.asarray(x['grads'], np.float64).reshape(case['S'], l['scene_stride'])[si] for x in (got, ref))
    out = {k: _rel(g[s], r[s]) for k, s in group_slices(case).items()}
    for k in POSE_GROUPS:
        out[k] = max([_rel(np.asarray(got[k], np.float64)[si * P + pi], np.asarray(ref[k], np.float64)[si * P + pi]) for pi in range(P)], default=0.0)
    return out


def errors(case, got, ref):
    """Worst error over the scenes per group."""
    out = {k: 0.0 for k in GROUPS}
    for si in range(case['S']):
        e = scene_errors(case, got, ref, si)
        out = {k: max(out[k], e[k]) for k in out}
    return out


def written_mask(case):
    """True for every entry of the flattened gradient array the VJP owns (everything else must come back zero in store mode and untouched in
    add mode)."""
    l = layout(case)
    m = np.zeros((case['S'], l['scene_stride']), bool)
    for si, sc in enumerate(case['scenes']):
        Ts = sc['Ts']
        if case['mode'] == 'frame':
            m[si, l['cam_rot6d']:l['cam_rot6d'] + 6 * Ts] = True
            m[si, l['cam_trans']:l['cam_trans'] + 3 * Ts] = True
        elif case['mode'] == 'fixed':
            m[si, l['cam_rot6d']:l['cam_rot6d'] + 6] = True
            m[si, l['cam_trans']:l['cam_trans'] + 3] = True
        else:
            n = n_visible(case, si)
            m[si, l['cam_inv_rot_res']:l['cam_inv_rot_res'] + 6 * Ts].reshape(Ts, 6)[n == 0] = True
            m[si, l['cam_inv_trans_res']:l['cam_inv_trans_res'] + 3 * Ts] = True
    return m.reshape(-1)


def pose_written_mask(case):
    """(S * P, T) True where a pose gradient is added: the frames at which a live person is visible."""
    m = np.zeros((case['S'] * case['P'], case['T']), bool)
    if case['mode'] == 'derived':
        for si, sc in enumerate(case['scenes']):
            for pi, p in live(case, si).items():
                m[si * case['P'] + pi, :sc['Ts']] = p['vis']
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


# fp32 autograd of the port against fp64 (one thread), rounded up to two digits; tests/test_extra_loss_cam_ref.py measures them again
FLOOR = {
    'frame24':         {'cam_rot6d': 6.2e-07, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 5.939e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'frame257':        {'cam_rot6d': 4.8e-06, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 4.556e-06, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'frame1':          {'cam_rot6d': 1.3e-07, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 1.192e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'frame_batch':     {'cam_rot6d': 2.0e-07, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 1.883e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'fixed24':         {'cam_rot6d': 3.4e-07, 'cam_trans': 1.2e-07, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 3.226e-07, 1.116e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'fixed257':        {'cam_rot6d': 3.1e-07, 'cam_trans': 1.2e-07, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 2.989e-07, 1.180e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'fixed_short':     {'cam_rot6d': 5.9e-07, 'cam_trans': 7.5e-07, 'cam_inv_rot_res': 0.0e+00, 'cam_inv_trans_res': 0.0e+00, 'g_orient_world': 0.0e+00, 'g_trans_world': 0.0e+00},      # 5.650e-07, 7.172e-07, 0.000e+00, 0.000e+00, 0.000e+00, 0.000e+00
    'derived40':       {'cam_rot6d': 0.0e+00, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 1.8e-07, 'cam_inv_trans_res': 2.0e-07, 'g_orient_world': 2.9e-07, 'g_trans_world': 1.5e-07},      # 0.000e+00, 0.000e+00, 1.684e-07, 1.864e-07, 2.732e-07, 1.469e-07
    'derived257':      {'cam_rot6d': 0.0e+00, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 2.6e-07, 'cam_inv_trans_res': 2.4e-07, 'g_orient_world': 7.9e-07, 'g_trans_world': 2.6e-07},      # 0.000e+00, 0.000e+00, 2.451e-07, 2.244e-07, 7.520e-07, 2.511e-07
    'derived_single':  {'cam_rot6d': 0.0e+00, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 1.4e-06, 'cam_inv_trans_res': 2.3e-07, 'g_orient_world': 2.1e-06, 'g_trans_world': 1.6e-07},      # 0.000e+00, 0.000e+00, 1.326e-06, 2.215e-07, 1.987e-06, 1.534e-07
    'derived_frozen':  {'cam_rot6d': 0.0e+00, 'cam_trans': 0.0e+00, 'cam_inv_rot_res': 3.0e-07, 'cam_inv_trans_res': 1.2e-07, 'g_orient_world': 4.3e-07, 'g_trans_world': 9.4e-08},      # 0.000e+00, 0.000e+00, 2.839e-07, 1.098e-07, 4.070e-07, 8.981e-08
}


def tol(name):
    return {k: FLOOR_FACTOR * v for k, v in FLOOR[name].items()}


if __name__ == '__main__':
    st = cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    for name in st['cases']:
        f = measure_floor(name)
        up = {k: (0.0 if v == 0 else float('%.1e' % (v * 1.05))) for k, v in f.items()}
        print("    %-18s {%s},      # %s" % ("'%s':" % name, ', '.join("'%s': %.1e" % (k, up[k]) for k in GROUPS), ', '.join('%.3e' % f[k] for k in GROUPS)))
