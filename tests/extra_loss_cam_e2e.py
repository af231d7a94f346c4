"""References of the camera terms of GlobalReconOptimizer.extra_loss, from oracle.port.grecon's optimiser on the CPU.

End to end: the port with the caller's term added to the total inside compute_loss, K iterations per stage from the state after init_data,
in fp64.  The device tests (tests/test_extra_loss_cam_gpu.py) pack the SAME state, run extra_loss_schedule.ExtraLossSchedule with the term as
a torch callback and compare every stage's first gradient, the last stage's variables, and the camera and world poses of its last evaluation.
The three runs, one per camera mode:
  'kp'      glamr_dynamic, one person of 24 frames: kp_2d leaves loss_cfg and comes back as the callback on ctx.project(ctx.joints()) (the
            reference is the port on the unmodified loss_cfg);
  'height'  glamr_static, one person: a camera-height prior, W_HEIGHT x the mean over the frames of (up-coordinate of the camera origin - H)^2,
            on ctx.cam_pose alone;
  'heels'   glamr_3dpw, two persons of 40 frames with a detection gap each (person 0 frames 14-21, person 1 frame 16, which sees nobody): W_HEELS x the mean squared reprojection
            error of the two heel joints against synthetic 2D targets (the projections after init_data plus 3 px of noise; in the fixture).

Agreement with the stage kernel: the same three scenes with kp_2d ALONE in the last stage's loss_cfg.  The device test compares the stage
kernel's gradient with the gradient of the same term written in torch and pushed through glamr_grecon_cam_backward and
glamr_grecon_pose_backward; its bound is the port's on that gradient (AGREE_FLOOR, measured here).

Bounds follow the project's rule: FLOOR_FACTOR = 16 x the deviation of the fp32 run of the SAME port from its fp64 run; gradients and
variables relative to the largest reference entry of the variable, the poses and cameras absolute.  The fp64 results live in
tests/golden/extra_loss_cam_e2e.npz (`python -m tests.extra_loss_cam_e2e` writes it, numbers only); tests/test_extra_loss_cam_ref.py runs the
port again and holds the file and the floors to it."""
import copy
import os

import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build, transforms as tf
from oracle.port.grecon import GlobalReconOptimizer, loss_kp_2d
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth
from tests import attach_common as ac
from tests.extra_loss_e2e import _named

FLOOR_FACTOR = 16
K = 5
HEELS = (13, 14)                      # 'OP LHeel', 'OP RHeel' of the body26fk joint set
W_HEIGHT, H_CAM, W_HEELS = 100.0, 1.5, 0.1
FIXTURE = 'extra_loss_cam_e2e'
# run: (config, frames, persons, seed, detection gap of person 0 or None, the term, the loss_cfg entry the device run drops)
RUNS = {'kp': ('glamr_dynamic', 24, 1, 21, (0, 0), None, 'kp_2d'),
        'height': ('glamr_static', 24, 1, 25, (0, 0), 'height', None),
        'heels': ('glamr_3dpw', 40, 2, 26, (14, 22), 'heels', None)}


def _cut(in_dict, idx, first, last):
    """Person `idx` is not detected in frames [first, last) (synth.trim_person for an interior range).  In place."""
    src = in_dict['est'][idx]
    ex = np.asarray(src['bboxes_dict']['exist']).copy()
    keep_frames = np.flatnonzero(ex)
    keep = (keep_frames < first) | (keep_frames >= last)
    ex[first:last] = 0
    for k in ('smpl_pose_quat_wroot', 'smpl_beta', 'root_trans', 'kp_2d', 'cam_K'):
        src[k] = src[k][keep]
    frames = np.flatnonzero(ex)
    src['frames'] = frames
    src['frame2ind'] = {int(f): i for i, f in enumerate(frames)}
    src['bboxes_dict'] = dict(src['bboxes_dict'], exist=ex, start=int(frames[0]), end=int(frames[-1]), num_frames=float(ex.sum()), exist_frames=frames)


def scene_inputs(run):
    cfg_id, T, P, seed, gap, _, _ = RUNS[run]
    in_dict = synth.make_in_dict(seed=seed, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model(), gap=gap)
    if P > 1:      # the second person's gap inside the first's: frame 16 sees nobody.  ONE frame: in a longer person-less run Adam's first steps
        # (exactly +-lr) cancel exactly in cam_origin_smoothness' gradient of the middle frames, and the sign of the rounding residue -- 3e-7 on
        # the device against a scale of 3e3, 0 in the port -- then decides a full step of the translation residual (the stage kernel's own term,
        # with or without a callback)
        _cut(in_dict, 1, gap[0] + 2, gap[0] + 3)
    return cfg_id, in_dict, mg.latents_for(in_dict, seed)


class CamTermPort(GlobalReconOptimizer):
    term, targets = None, None

    def compute_loss(self, data, loss_cfg):
        total, ld, lud = GlobalReconOptimizer.compute_loss(self, data, loss_cfg)
        if self.term == 'height':
            total = total + W_HEIGHT * (data['cam_pose_inv'][:, 2, 3] - H_CAM).pow(2).mean()
        elif self.term == 'heels':
            tot, n = 0, 0
            for idx, d in data['person_data'].items():
                diff = d['kp_2d_pred'][:, list(HEELS)] - self.targets[idx].to(d['kp_2d_pred'].dtype)
                tot = tot + diff.pow(2).sum()
                n += 2 * diff.shape[0]
            total = total + W_HEELS * tot / n
        return total, ld, lud


_INIT, _RUNS, _AGREE = {}, {}, {}


def state(asset_root, run):
    """(cfg, port optimiser, fp32 state after init_data, heel targets {idx: (T, 2, 2) fp64 tensor}) -- computed once per run and left unchanged
    (callers deep-copy)."""
    if run not in _INIT:
        cfg_id, in_dict, lat = scene_inputs(run)
        cfg = get_config(cfg_id)
        ora = build.load_optimizer(asset_root, cfg)
        ora.__class__ = CamTermPort
        with torch.no_grad():
            data = ora.init_data(in_dict, latents=lat)
        rng = np.random.default_rng(77)
        targets = {idx: d['kp_2d_pred'][:, list(HEELS)].detach().double() + torch.tensor(3.0 * rng.normal(size=(d['kp_2d_pred'].shape[0], 2, 2)))
                   for idx, d in data['person_data'].items()}
        _INIT[run] = (cfg, ora, data, targets)
    return _INIT[run]


def _cast_run(ora, data0, dtype):
    data = ac._cast(copy.deepcopy(data0), dtype)
    smpl = copy.deepcopy(ora.smpl).to(dtype)
    return data, smpl


def reference(asset_root, run, dtype=torch.float64):
    """{'<stage>/grad/<variable>', '<stage>/param/<variable>', '<stage>/cam/pose', '<stage>/orient/p<idx>', '<stage>/trans/p<idx>': fp64 arrays}
    of K iterations per stage of the port with the term, in `dtype`: every stage's first gradient; of the LAST stage the variables after it and
    the camera and world poses of its last evaluation.  Cached."""
    if (run, dtype) in _RUNS:
        return _RUNS[(run, dtype)]
    cfg, ora, data0, targets = state(asset_root, run)
    smpl0, old = ora.smpl, torch.get_default_dtype()
    out = {}
    try:
        torch.set_default_dtype(dtype)
        data, ora.smpl = _cast_run(ora, data0, dtype)
        ora.term, ora.targets = RUNS[run][5], targets
        for stage, spec in ora.opt_stage_specs.items():
            var = spec['opt_variables']
            params = ora.get_parameter(data, var)
            for p in params:
                p.requires_grad_(True)
            opt = torch.optim.Adam(params, lr=spec['opt_lr'], betas=(0.9, 0.999))

            def closure():
                opt.zero_grad()
                ora.forward(data, var, {'stage': stage})
                loss, _, _ = ora.compute_loss(data, spec['loss_cfg'])
                loss.backward()
                return loss
            for it in range(min(K, spec['opt_niters'])):
                ora.cur_iter = it
                if it == 0:
                    closure()
                    out.update({'%s/grad/%s' % (stage, k): v for k, v in _named(data, var, ora.specs, 'grad').items()})
                opt.step(closure)
            for p in params:
                p.requires_grad_(False)
            if stage == list(ora.opt_stage_specs)[-1]:
                out.update({'%s/param/%s' % (stage, k): v for k, v in _named(data, var, ora.specs).items()})
                out['%s/cam/pose' % stage] = data['cam_pose'][:, :3].detach().double().numpy().copy()
                for idx, d in data['person_data'].items():
                    out['%s/orient/p%d' % (stage, idx)] = d['smpl_orient_world'].detach().double().numpy().copy()
                    out['%s/trans/p%d' % (stage, idx)] = d['root_trans_world'].detach().double().numpy().copy()
            data['cam_pose'], data['cam_pose_inv'] = data['cam_pose'].detach(), data['cam_pose_inv'].detach()
            if spec.get('reinitialize_cam', False):
                data['cam_pose'][:] = data['cam_pose'][[0]]
                data['cam_pose_inv'] = tf.invert_transform(data['cam_pose'])
    finally:
        ora.smpl, ora.term, ora.targets, ora.cur_iter = smpl0, None, None, 0
        torch.set_default_dtype(old)
    _RUNS[(run, dtype)] = out
    return out


def agree_reference(asset_root, run, dtype=torch.float64):
    """{'<stage>/grad/<variable>'}: the port's gradient of the LAST stage's variables with kp_2d alone in loss_cfg, at the state after init_data."""
    if (run, dtype) in _AGREE:
        return _AGREE[(run, dtype)]
    cfg, ora, data0, _ = state(asset_root, run)
    smpl0, old = ora.smpl, torch.get_default_dtype()
    try:
        torch.set_default_dtype(dtype)
        data, ora.smpl = _cast_run(ora, data0, dtype)
        stage, spec = ac.stage_of(cfg)
        var = spec['opt_variables']
        params = ora.get_parameter(data, var)
        for p in params:
            p.requires_grad_(True)
        ora.forward(data, var, {'stage': stage})
        (loss_kp_2d(data, spec['loss_cfg']['kp_2d']) * spec['loss_cfg']['kp_2d']['weight']).backward()
        out = {'%s/grad/%s' % (stage, k): v for k, v in _named(data, var, ora.specs, 'grad').items()}
    finally:
        ora.smpl = smpl0
        torch.set_default_dtype(old)
    _AGREE[(run, dtype)] = out
    return out


KINDS = ('grad', 'param', 'cam', 'orient', 'trans')


def errors(got, ref):
    """Worst error per kind over stages and variables: gradients and variables relative to the variable's largest reference entry, poses and
    cameras absolute."""
    out = {k: 0.0 for k in KINDS}
    for name, r in ref.items():
        kind = name.split('/')[1]
        d = float(np.abs(np.asarray(got[name], np.float64) - r).max()) if r.size else 0.0
        if kind in ('grad', 'param'):
            scale = float(np.abs(r).max()) if r.size else 0.0
            d = d / (scale if scale > 0 else 1.0)
        out[kind] = max(out[kind], d)
    return out


def measure_floor(asset_root, run):
    from tests.traj_ref_common import single_thread
    with single_thread():
        e = errors(reference(asset_root, run, torch.float32), reference(asset_root, run))
        a = errors(agree_reference(asset_root, run, torch.float32), agree_reference(asset_root, run))['grad']
    return e, a


# fp32 run of the port against its fp64 run (one thread), rounded up to two digits; tests/test_extra_loss_cam_ref.py measures them again
FLOOR = {
    'kp':     {'grad': 3.8e-05, 'param': 8.4e-05, 'cam': 3.9e-07, 'orient': 7.3e-07, 'trans': 2.2e-08},      # 3.663e-05, 7.984e-05, 3.693e-07, 6.949e-07, 2.064e-08
    'height': {'grad': 1.7e-05, 'param': 1.4e-04, 'cam': 4.1e-08, 'orient': 5.9e-07, 'trans': 3.1e-08},      # 1.624e-05, 1.336e-04, 3.939e-08, 5.628e-07, 2.962e-08
    'heels':  {'grad': 6.1e-05, 'param': 3.8e-01, 'cam': 2.4e-06, 'orient': 2.4e-04, 'trans': 2.2e-07},      # 5.827e-05, 3.617e-01, 2.261e-06, 2.309e-04, 2.117e-07
}
# ... and of the port's gradient of the last stage with kp_2d alone (the bound of the agreement with the stage kernel)
AGREE_FLOOR = {
    'kp':     2.1e-05,      # 1.971e-05
    'height': 8.3e-06,      # 7.880e-06
    'heels':  4.8e-05,      # 4.588e-05
}
TOL = {n: {k: FLOOR_FACTOR * v for k, v in f.items()} for n, f in FLOOR.items()}
AGREE_TOL = {n: FLOOR_FACTOR * v for n, v in AGREE_FLOOR.items()}


def fixture_arrays(asset_root):
    out = {'%s:%s' % (run, k): v for run in RUNS for k, v in reference(asset_root, run).items()}
    out.update({'heels:target/p%d' % idx: t.numpy() for idx, t in state(asset_root, 'heels')[3].items()})
    return out


def from_fixture(g, run):
    return {k[len(run) + 1:]: v for k, v in g.items() if k.startswith(run + ':') and '/' in k and not k.startswith(run + ':target/')}


def targets_from_fixture(g):
    return {int(k.split('/p')[1]): v for k, v in g.items() if k.startswith('heels:target/')}


if __name__ == '__main__':
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', FIXTURE + '.npz'), **fixture_arrays(root))
    agree = {}
    for run in RUNS:
        f, agree[run] = measure_floor(root, run)
        up = {k: (0.0 if v == 0 else float('%.1e' % (v * 1.05))) for k, v in f.items()}
        print("    %-9s {%s},      # %s" % ("'%s':" % run, ', '.join("'%s': %.1e" % (k, up[k]) for k in KINDS), ', '.join('%.3e' % f[k] for k in KINDS)))
    for run, a in agree.items():
        print("    %-9s %.1e,      # %.3e" % ("'%s':" % run, float('%.1e' % (a * 1.05)), a))
