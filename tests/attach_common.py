"""Reference of the ATTACHED trajectory prior (flag_attach_traj_pred): "the reference minus one detach".  `AttachedOptimizer` is
oracle.port.grecon's optimiser whose pred_trajectory_base is the port's with the `.detach()` of global_recon_model.py:396 dropped, so torch
autograd carries the loss to `traj_local_pred` (and, through the priors, to the latents).  Everything runs in the dtype of the data it is
given: `scene_reference(..., dtype=torch.float64)` casts the port's state to fp64 the way tests/smpl_ref_common.py does for the body model.

Tolerances follow the project's rule (tests/traj_ref_common.FLOOR_FACTOR = 16): 16 x the deviation of the fp32 run of the SAME port from
its fp64 run on the same inputs, measured on the CPU (tests/test_attach_ref.py derives them again), never taken from the code under test."""
import copy

import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build, transforms as tf
from oracle.port.grecon import GlobalReconOptimizer
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth

FLOOR_FACTOR = 16

# mutations of the reference's BACKWARD (the forward values stay): each must move the result by more than the tolerance of the comparison
# it targets, or the GPU tests could not fail
MUTATIONS = {'heading': 'heading columns dropped', 'reg': 'regulariser leaked into columns 0-8', 'mask': 'dheading_mask applied to columns 9-10',
             'fk_leaf': 'FK backward without the descendants\' contribution', 'no_fk': 'FK term not added to motion_latent'}


def _graft(value, grad_of):
    """`value`'s numbers with `grad_of`'s gradient."""
    return value.detach() + (grad_of - grad_of.detach())


class AttachedOptimizer(GlobalReconOptimizer):
    mut = None

    def pred_trajectory_base(self, d):
        """oracle.port.grecon.GlobalReconOptimizer.pred_trajectory_base with `traj_local_pred` left attached (the only difference)."""
        P = d['traj_local_pred']
        L = P.clone()
        L[0, :2] += d['traj_local_xy']
        L[1:, :2] += d['traj_local_dxy']
        mask = torch.ones_like(L[1:, 0])
        for (s, e) in self.cam_fix_frames:
            mask[s:e] = 0.0
        hv = L[:, -2:].clone()
        if self.mut == 'heading':
            hv = hv.detach()
        h0 = tf.vec_to_heading(hv[[0]]) + d['traj_local_heading']
        L[0, -2:] = tf.heading_to_vec(h0).squeeze(0)
        hp = tf.vec_to_heading(hv[1:])
        if self.mut == 'mask':
            hp = _graft(hp, hp * mask)
        h = hp + d['traj_local_dheading'] * mask
        L[1:, -2:] = tf.heading_to_vec(h)
        L[:, 2] += d['traj_local_z']
        L[:, 3:-2] += d['traj_local_rot']
        return L

    def forward(self, data, opt_variables, opt_meta):
        for d in data['person_data'].values():
            if self.mut == 'reg':        # the deltas' regularisers pull on the prior rows as well
                ghost = d['traj_local_pred'] - d['traj_local_pred'].detach()
                d['traj_local_dxy'] = d['traj_local_dxy'] + ghost[1:, :2]
                d['traj_local_z'] = d['traj_local_z'] + ghost[:, 2]
                d['traj_local_rot'] = d['traj_local_rot'] + ghost[:, 3:-2]
        super().forward(data, opt_variables, opt_meta)

    # (the base class's forward calls self.pred_trajectory_base(d) and expects it to fill d)
    def _fill(self, d, L):
        d['traj_local'] = L
        trans, q = tf.local_to_global_traj(L)
        ex = d['exist_frames']
        d['smpl_orient_world_base'] = d['smpl_orient_world_base'].detach().clone()
        d['root_trans_world_base'] = d['root_trans_world_base'].detach().clone()
        d['smpl_orient_world_base'][ex] = tf.quat_to_aa(q)
        d['root_trans_world_base'][ex] = trans


def _attached_pred(self, d):
    AttachedOptimizer._fill(self, d, AttachedOptimizer._row(self, d))


AttachedOptimizer._row = AttachedOptimizer.pred_trajectory_base
AttachedOptimizer.pred_trajectory_base = _attached_pred


def _cast(x, dt):
    if torch.is_tensor(x):
        return x.to(dt) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: _cast(v, dt) for k, v in x.items()}
    return x


# ---- the scenes of the g_traj_local comparison -------------------------------------------------------------------------------------------
# (config, frames, persons, seed, trim): trim = (person, first frame, end frame) cut out of the video (ragged existence)
SCENES = {'one': ('glamr_dynamic', 24, 1, 21, None),                 # one person, per-frame camera
          'two': ('glamr_static_multi', 24, 2, 22, (1, 5, 22)),      # shared camera, lengths 24 and 17, one fr_start = 5, rel_transform on
          'nine': ('glamr_dynamic_multi', 12, 9, 23, None)}          # the wide compile


def scene_inputs(name):
    cfg_id, T, P, seed, trim = SCENES[name]
    in_dict = synth.make_in_dict(seed=seed, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model(), gap=(0, 0))
    if trim is not None:
        in_dict = synth.trim_person(in_dict, *trim)
    return cfg_id, in_dict, mg.latents_for(in_dict, seed)


def stage_of(cfg):
    """The stage whose loss the comparison uses: the LAST one (every variable group and every term of the configuration)."""
    name = list(cfg['opt_stage_specs'])[-1]
    return name, cfg['opt_stage_specs'][name]


_INIT = {}


def scene_state(asset_root, name):
    """(cfg, optimiser, fp32 state after init_data) -- computed once per scene and left unchanged (callers deep-copy)."""
    if name not in _INIT:
        cfg_id, in_dict, lat = scene_inputs(name)
        cfg = get_config(cfg_id)
        ora = build.load_optimizer(asset_root, cfg)
        ora.__class__ = AttachedOptimizer
        with torch.no_grad():
            data = ora.init_data(in_dict, latents=lat)
        _INIT[name] = (cfg, ora, data)
    return _INIT[name]


def scene_reference(asset_root, name, dtype=torch.float64, mut=None):
    """dL/d traj_local_pred per person {idx: (n, 11) fp64 array} of the last stage's weighted loss at the state after init_data (deltas zero),
    by torch autograd through the attached port in `dtype`."""
    cfg, ora, data0 = scene_state(asset_root, name)
    stage, spec = stage_of(cfg)
    data = _cast(copy.deepcopy(data0), dtype)
    smpl0 = ora.smpl
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(dtype)
        ora.smpl = copy.deepcopy(smpl0).to(dtype)
        ora.mut = mut
        params = ora.get_parameter(data, spec['opt_variables'])
        for p in params:
            p.requires_grad_(True)
        leaves = {}
        for idx, d in data['person_data'].items():
            d['traj_local_pred'] = d['traj_local_pred'].detach().clone().requires_grad_(True)
            leaves[idx] = d['traj_local_pred']
        ora.forward(data, spec['opt_variables'], {'stage': stage})
        loss, _, _ = ora.compute_loss(data, spec['loss_cfg'])
        loss.backward()
        return {idx: (t.grad if t.grad is not None else torch.zeros_like(t)).double().numpy() for idx, t in leaves.items()}
    finally:
        ora.smpl, ora.mut = smpl0, None
        torch.set_default_dtype(old)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


COLS = {'row': slice(0, 9), 'heading': slice(9, 11)}


def scene_errors(got, ref):
    """Worst relative error over the persons, columns 0-8 and 9-10 apart (each relative to the person's largest reference entry of the group)."""
    return {k: max(rel_err(got[i][:, c], ref[i][:, c]) for i in ref) for k, c in COLS.items()}


# fp32 port vs fp64 port (tests/test_attach_ref.py measures them again and fails if they drifted by more than 2 x in either direction), rounded up to two digits
G_TRAJ_FLOOR = {'one': {'row': 2.2e-5, 'heading': 1.1e-5},        # 2.104e-5, 1.030e-5
                'two': {'row': 1.4e-6, 'heading': 1.3e-6},        # 1.375e-6, 1.235e-6
                'nine': {'row': 2.7e-5, 'heading': 1.4e-5}}       # 2.670e-5, 1.323e-5
G_TRAJ_TOL = {n: {k: FLOOR_FACTOR * v for k, v in f.items()} for n, f in G_TRAJ_FLOOR.items()}


# ---- FK backward ------------------------------------------------------------------------------------------------------------------------
FK_LENS = (1, 9, 10, 11, 23)                      # one ragged batch around FK_FRAMES = 10 frames per workgroup
FK_FAMILIES = ('zero', 'small', 'generic', 'near_pi')


def fk_inputs(family):
    """body pose (B, 23, 69) and upstream gradient (B, 23, 69), fp32; rows at or beyond FK_LENS[b] are zero."""
    rng = np.random.default_rng({'zero': 1, 'small': 2, 'generic': 3, 'near_pi': 4}[family])
    B, T = len(FK_LENS), max(FK_LENS)
    if family == 'zero':
        pose = np.zeros((B, T, 69))
    elif family == 'small':
        pose = rng.normal(size=(B, T, 69)) * 1e-4
    elif family == 'generic':
        pose = rng.normal(size=(B, T, 69)) * 0.4
    else:
        ax = rng.normal(size=(B, T, 23, 3))
        ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
        pose = (ax * (np.pi - rng.uniform(1e-3, 5e-2, size=(B, T, 23, 1)))).reshape(B, T, 69)
    G = rng.normal(size=(B, T, 69))
    for b, n in enumerate(FK_LENS):
        pose[b, n:] = 0.0
        G[b, n:] = 0.0
    return pose.astype(np.float32), G.astype(np.float32)


def fk_reference(asset_root, family, dtype=torch.float64, mut=None):
    """d sum(G * get_joint_pos(pose)) / d pose (B, T, 69) by autograd through the port's TrajPredVAE.get_joint_pos in `dtype`."""
    from tests import traj_ref_common as tc
    net = tc.predictor(asset_root, dtype)
    pose32, G = fk_inputs(family)
    out = np.zeros(pose32.shape, np.float64)
    for b, n in enumerate(FK_LENS):
        p = torch.tensor(pose32[b, :n], dtype=dtype)[:, None].requires_grad_(True)
        j = net.get_joint_pos(p)
        if mut == 'fk_leaf':      # a joint's rotation only moves its own children's offsets: the descendants' contribution is cut
            j = _fk_leaf_only(net, p)
        (g,) = torch.autograd.grad((j[:, 0] * torch.tensor(G[b, :n], dtype=dtype)).sum(), p)
        out[b, :n] = g[:, 0].double().numpy()
    return out


def _fk_leaf_only(net, p):
    """Joint rows with the numbers of get_joint_pos and the gradient of a chain whose parent transforms are constants."""
    from oracle.port.smpl import batch_rodrigues
    full = net.get_joint_pos(p)
    sm = net.smpl
    rest = torch.matmul(sm.J_regressor, sm.v_template).to(p.dtype)
    parents = [int(x) for x in sm.parents]
    T = p.shape[0]
    aa = torch.cat([torch.zeros((T, 1, 3), dtype=p.dtype), p[:, 0].reshape(T, 23, 3)], dim=1)
    R = batch_rodrigues(aa.reshape(-1, 3)).reshape(T, 24, 3, 3)
    G = [R[:, 0]]
    for j in range(1, 24):
        G.append(torch.matmul(G[parents[j]].detach(), R[:, j]))
    pos = [rest[0].expand(T, 3)]
    for j in range(1, 24):
        pa = parents[j]
        pos.append(pos[pa].detach() + torch.matmul(G[pa], rest[j] - rest[pa]))
    approx = torch.stack([pos[j] - pos[0] for j in range(1, 24)], dim=1).reshape(T, 1, 69)
    return _graft(full, approx)


# fp32 autograd of the port against fp64, relative to the batch's largest reference entry (the 1e-4-small poses: the fp32 Rodrigues formula
# divides by an angle whose square is rounded at 1e-8 + 1e-16)
FK_FLOOR = {'zero': 1.2e-7, 'small': 1.1e-4, 'generic': 1.7e-7, 'near_pi': 5.0e-7}      # 1.169e-7, 1.055e-4, 1.640e-7, 4.989e-7
FK_TOL = {k: FLOOR_FACTOR * v for k, v in FK_FLOOR.items()}


# ---- the mode end to end: the port's latent-optimisation loop with the detach dropped ------------------------------------------------------
class AttachedLatentOptimizer(AttachedOptimizer):
    """The reference's latent-optimisation mode (global_recon_model.py:434-437, 619-622) on the port: from `opt_latent_start_iter` on every
    forward re-runs infer_motion_traj with the current latents, which are Adam parameters beside the stage's.  `attached = False` keeps the
    port's own pred_trajectory_base (with the detach): the reference as it is."""
    attached = True
    opt_motion = opt_traj = True

    def pred_trajectory_base(self, d):
        if self.attached:
            return _attached_pred(self, d)
        return GlobalReconOptimizer.pred_trajectory_base(self, d)

    def infer_motion_traj(self, d):
        tp = self.mt_model.traj_predictor
        if self.mut == 'no_fk':      # the predictor sees the infiller's poses as constants: no term through the FK joints
            orig = tp.inference
            tp.inference = lambda tb, **kw: orig(dict(tb, in_body_pose=tb['in_body_pose'].detach()), **kw)
        try:
            super().infer_motion_traj(d)
        finally:
            tp.__dict__.pop('inference', None)

    def forward(self, data, opt_variables, opt_meta):
        if opt_meta['stage'] != 'init' and self.cur_iter >= opt_meta.get('opt_latent_start_iter', 100):
            for d in data['person_data'].values():
                self.infer_motion_traj(d)
        super().forward(data, opt_variables, opt_meta)

    def get_parameter(self, data, opt_variables):
        params = super().get_parameter(data, opt_variables)
        for d in data['person_data'].values():
            params += ([d['in_motion_latent']] if self.opt_motion else []) + ([d['in_traj_latent']] if self.opt_traj else [])
        return params


# (config, frames, persons, trim, candidate seeds): 70 frames = two infiller windows (the autoregression is live); lengths 70 and 45.
# A candidate whose fp64 forward at the initial state puts a ReLU pre-activation of either prior within KINK of zero has no stable VJP and
# is left out (E2E_KINKED, found on the CPU, tests/test_attach_ref.py checks the list and the cap of one quarter); the device tests run the
# first candidate that is kept.
KINK = 1e-6
E2E_K = 5
E2E = {'one': ('glamr_dynamic', 70, 1, None, (37, 49, 57, 62)),
       'two': ('glamr_dynamic_multi', 70, 2, (1, 12, 57), (36, 82))}
E2E_KINKED = {'one': (), 'two': ()}


def e2e_seed(name):
    return [s for s in E2E[name][4] if s not in E2E_KINKED[name]][0]


def e2e_inputs(name, seed=None):
    cfg_id, T, P, trim, _ = E2E[name]
    seed = e2e_seed(name) if seed is None else seed
    in_dict = synth.make_in_dict(seed=seed, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model(), gap=(0, 0))
    if trim is not None:
        in_dict = synth.trim_person(in_dict, *trim)
    return cfg_id, in_dict, mg.latents_for(in_dict, seed), P


_E2E_INIT, _E2E_RUNS = {}, {}


def _e2e_state(asset_root, name, seed):
    if (name, seed) not in _E2E_INIT:
        cfg_id, in_dict, lat, _ = e2e_inputs(name, seed)
        cfg = get_config(cfg_id)
        ora = build.load_optimizer(asset_root, cfg)
        ora.__class__ = AttachedLatentOptimizer
        with torch.no_grad():
            data = ora.init_data(in_dict, latents=lat)
        _E2E_INIT[(name, seed)] = (cfg, ora, data)
    return _E2E_INIT[(name, seed)]


def relu_margin(asset_root, name, seed):
    """Smallest |ReLU pre-activation| of the two priors' fp64 forward at the initial latents of candidate `seed`."""
    from tests.nets_vjp_common import RELU_INPUTS
    cfg, ora, data0 = _e2e_state(asset_root, name, seed)
    mt = copy.deepcopy(ora.mt_model)
    mt.mfiller.double(), mt.traj_predictor.double()
    mt.traj_predictor.__dict__['smpl'] = copy.deepcopy(ora.smpl).double()
    margins = []
    hooks = [m.register_forward_hook(lambda mod, i, o: margins.append(float(o.detach().abs().min())))
             for net in (mt.mfiller, mt.traj_predictor) for n, m in net.named_modules()
             if isinstance(m, torch.nn.Linear) and any(k in n for k in RELU_INPUTS)]
    old, mt0 = torch.get_default_dtype(), ora.mt_model
    try:
        torch.set_default_dtype(torch.float64)
        ora.mt_model = mt
        with torch.no_grad():
            for d in _cast(copy.deepcopy(data0), torch.float64)['person_data'].values():
                AttachedLatentOptimizer.infer_motion_traj(ora, d)
    finally:
        ora.mt_model = mt0
        torch.set_default_dtype(old)
        for h in hooks:
            h.remove()
    return min(margins)


def e2e_reference(asset_root, name, dtype=torch.float64, K=E2E_K, attached=True, mut=None, weight_scale=1.0, seed=None):
    """K iterations per stage of the port's latent-optimisation loop (both latent flags) in `dtype`, priors and body model cast the way
    scene_reference does.  Returns per person idx: g_traj (128,) and g_motion (windows, 128), the latents' gradients of the run's first
    iteration (None where autograd gave none), and traj_latent (1, 128), motion_latent (windows, 128) after the K iterations.  Cached."""
    seed = e2e_seed(name) if seed is None else seed
    key = (name, seed, dtype, K, attached, mut, weight_scale)
    if key in _E2E_RUNS:
        return _E2E_RUNS[key]
    cfg, ora, data0 = _e2e_state(asset_root, name, seed)
    data = _cast(copy.deepcopy(data0), dtype)
    smpl0, mt0, old = ora.smpl, ora.mt_model, torch.get_default_dtype()
    first = {}
    try:
        torch.set_default_dtype(dtype)
        ora.smpl = copy.deepcopy(smpl0).to(dtype)
        ora.mt_model = copy.deepcopy(mt0)
        ora.mt_model.mfiller.to(dtype), ora.mt_model.traj_predictor.to(dtype)
        ora.mt_model.traj_predictor.__dict__['smpl'] = ora.smpl
        ora.mut, ora.attached = mut, attached
        for idx, d in data['person_data'].items():
            for k, key_ in (('g_motion', 'in_motion_latent'), ('g_traj', 'in_traj_latent')):
                d[key_] = d[key_].detach().clone().requires_grad_(True)
                d[key_].register_hook(lambda g, slot=(idx, k): first.setdefault(slot, g.detach().clone()) is None or None)
        for stage, spec in ora.opt_stage_specs.items():
            loss_cfg = {n: dict(c, weight=c['weight'] * weight_scale) for n, c in spec['loss_cfg'].items()}
            ora.optimize_main(data, spec['opt_variables'], spec['opt_lr'], min(K, spec['opt_niters']), loss_cfg,
                              {'stage': stage, 'opt_latent_start_iter': spec.get('opt_latent_start_iter', 0)})
            if spec.get('reinitialize_cam', False):
                data['cam_pose'][:] = data['cam_pose'][[0]]
                data['cam_pose_inv'] = tf.invert_transform(data['cam_pose'])
        out = {}
        for idx, d in data['person_data'].items():
            out[idx] = {k: (first[(idx, k)].double().numpy() if (idx, k) in first else None) for k in ('g_motion', 'g_traj')}
            out[idx]['g_traj'] = None if out[idx]['g_traj'] is None else out[idx]['g_traj'].reshape(-1)
            out[idx].update(traj_latent=d['in_traj_latent'].detach().double().numpy(), motion_latent=d['in_motion_latent'].detach().double().numpy())
    finally:
        ora.smpl, ora.mt_model, ora.mut, ora.attached, ora.cur_iter = smpl0, mt0, None, True, 0
        torch.set_default_dtype(old)
    _E2E_RUNS[key] = out
    return out


E2E_KEYS = ('g_traj', 'g_motion', 'traj_latent')


def e2e_errors(got, ref):
    """Worst error over the persons: the two first gradients relative to the person's largest reference entry, traj_latent after the K
    iterations absolute (the draw is of order one)."""
    return {'g_traj': max(rel_err(got[i]['g_traj'], ref[i]['g_traj']) for i in ref),
            'g_motion': max(rel_err(got[i]['g_motion'], ref[i]['g_motion']) for i in ref),
            'traj_latent': max(float(np.abs(np.asarray(got[i]['traj_latent'], np.float64) - ref[i]['traj_latent']).max()) for i in ref)}


# fp32 run of the port against its fp64 run (one thread), rounded up to two digits; tests/test_attach_ref.py measures them again
E2E_FLOOR = {'one': {'g_traj': 3.0e-7, 'g_motion': 6.4e-7, 'traj_latent': 2.0e-7},        # 2.932e-7, 6.362e-7, 1.990e-7
             'two': {'g_traj': 1.8e-5, 'g_motion': 2.0e-6, 'traj_latent': 1.9e-5}}        # 1.784e-5, 1.961e-6, 1.872e-5
E2E_TOL = {n: {k: FLOOR_FACTOR * v for k, v in f.items()} for n, f in E2E_FLOOR.items()}


# The fp64 run takes the CPU tens of seconds, so the device tests read its results from tests/golden/attach_e2e.npz (written by
# `python -m tests.attach_common`, numbers only); tests/test_attach_ref.py runs the port again and holds the file to it.
FIXTURE = 'attach_e2e'


def fixture_arrays(asset_root):
    out = {}
    for name in E2E:
        for idx, r in e2e_reference(asset_root, name).items():
            for k, v in r.items():
                out['%s_p%d_%s' % (name, idx, k)] = v
    return out


def from_fixture(g, name):
    """The layout of e2e_reference from the loaded fixture `g`."""
    P = E2E[name][2]
    return {idx: {k: g['%s_p%d_%s' % (name, idx, k)] for k in ('g_traj', 'g_motion', 'traj_latent', 'motion_latent')} for idx in range(P)}


if __name__ == '__main__':
    import os
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', FIXTURE + '.npz'), **fixture_arrays(root))
