"""Reference of the optimiser's built-in `penetration` term end to end: oracle.port.grecon's optimiser with the term of
tests/penetration_common.py (frame_term: the restated definition) added to the total inside compute_loss the way loss_func.py:274-290 does --
per frame of the scene over the persons visible in it, divided by the scene's length --, K iterations per stage from the state after
init_data, in fp64.  The device tests (tests/test_penetration_gpu.py) pack the SAME state, run the schedule with `penetration` in loss_cfg and
compare every stage's first gradient, the last stage's variables, the world poses and penetration_history.

Scene: glamr_dynamic_multi, two persons, 24 frames; the second person's camera-space translations are moved beside the first's so that the
boxes overlap.  Body: the synthetic SMPL model with its faces replaced by the outward-oriented convex hull of the template (closed; the shipped
synthetic faces are a triangle soup without an inside).  GRID = 16 keeps the fp64 restatement affordable; the kernels at 32 are covered by
tests/test_penetration_gpu.py::test_kernels_match_the_fp64_restatement[g32].

Bounds: FLOOR_FACTOR = 16 x the deviation of the fp32 run of the SAME port from its fp64 run (recorded below by `python -m tests.penetration_e2e`,
which also writes tests/golden/penetration_e2e.npz, numbers only); tests/test_penetration_ref.py holds the first gradient of the file and its
floor to a fresh run of the port."""
import copy
import os

import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build, transforms as tf
from oracle.port.grecon import GlobalReconOptimizer
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth
from tests import attach_common as ac
from tests import penetration_common as pc
from tests.extra_loss_e2e import _named, errors as _errors

FLOOR_FACTOR = 16
K = 5
GRID = 16
WEIGHT = 10.0
CFG_ID, SEED, T, OFFSET = 'glamr_dynamic_multi', 24, 24, (0.22, 0.02, 0.08)
FIXTURE = 'penetration_e2e'
KINDS = ('grad', 'param', 'orient', 'trans', 'history')


def hull_faces():
    """Outward-oriented convex hull of the synthetic template (V = 6890; the vertices inside the hull belong to no face)."""
    from scipy.spatial import ConvexHull
    v = np.asarray(synth.make_smpl_model()['v_template'], np.float64)
    f = ConvexHull(v).simplices.astype(np.int32)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    flip = (n * (v[f].mean(1) - v[np.unique(f)].mean(0))).sum(1) < 0
    f[flip] = f[flip][:, ::-1]
    return np.ascontiguousarray(f)


def scene_inputs():
    in_dict = synth.make_in_dict(seed=SEED, num_frames=T, num_persons=2, smpl_model=synth.make_smpl_model(), gap=(0, 0))
    est = in_dict['est']
    est[1]['root_trans'] = (est[0]['root_trans'][est[1]['frames']] + np.asarray(OFFSET, np.float32)).astype(np.float32)
    return in_dict, mg.latents_for(in_dict, SEED)


def device_cfg(weight=WEIGHT, monitor_only=False, stages=None):
    """The device configuration: flag_use_pen_loss and the term in the loss_cfg of `stages` (default: every stage)."""
    cfg = copy.deepcopy(get_config(CFG_ID))
    cfg['grecon_model_specs']['flag_use_pen_loss'] = True
    for stage, spec in cfg['opt_stage_specs'].items():
        if stages is None or stage in stages:
            spec['loss_cfg']['penetration'] = dict(weight=weight, monitor_only=True) if monitor_only else dict(weight=weight)
    return cfg


class TermPort(GlobalReconOptimizer):
    pen_weight = None              # None: the port as it is
    pen_faces = None
    pen_values = None              # the unweighted value of every compute_loss call

    def penetration(self, data):
        """loss_func.py:274-290 with the restated SDFLoss"""
        pd = data['person_data']
        verts = {i: self.smpl(global_orient=d['smpl_orient_world'], body_pose=d['smpl_pose'], betas=d['smpl_beta'], root_trans=d['root_trans_world'],
                              root_scale=None, return_full_pose=True).vertices for i, d in pd.items()}
        max_fr = int(data['seq_len'])
        total, per_frame = 0, np.zeros(max_fr)
        for fr in range(max_fr):
            x = [verts[i][fr] for i, d in pd.items() if bool(d['vis_frames'][fr])]
            if len(x) < 2:
                continue
            v = pc.frame_term(torch.stack(x), self.pen_faces, GRID, 0.2, 1.0)
            total, per_frame[fr] = total + v, float(v)
        self.pen_frames = per_frame
        return total / max_fr

    def compute_loss(self, data, loss_cfg):
        total, ld, lud = GlobalReconOptimizer.compute_loss(self, data, loss_cfg)
        if self.pen_weight is not None:
            value = self.penetration(data)
            self.pen_values.append(float(value))
            total = total + self.pen_weight * value
        return total, ld, lud


_INIT, _RUNS = {}, {}


def state(asset_root):
    """(cfg of the port (no penetration entry), port optimiser, fp32 state after init_data) -- computed once and left unchanged."""
    if not _INIT:
        in_dict, lat = scene_inputs()
        cfg = get_config(CFG_ID)
        ora = build.load_optimizer(asset_root, cfg)
        ora.__class__ = TermPort
        ora.pen_faces = hull_faces()
        from tests.traj_ref_common import single_thread
        with torch.no_grad(), single_thread():                # (one thread: the fp32 state does not depend on the machine's core count)
            data = ora.init_data(in_dict, latents=lat)
        _INIT['s'] = (cfg, ora, data)
    return _INIT['s']


def reference(asset_root, dtype=torch.float64, weight=WEIGHT, first_only=False):
    """{'<stage>/grad/<variable>', '<stage>/history', '<stage>/param/<variable>', '<stage>/orient/p<idx>', '<stage>/trans/p<idx>', 'frames',
    'grad0_without'}: K iterations per stage of the port with the term, in `dtype`.  `frames`: the per-frame values of the very first
    evaluation; `grad0_without/<variable>`: the first stage's first gradient of the port WITHOUT the term (weight None).  first_only: stop after
    the first stage's first gradient.  Cached."""
    key = (dtype, weight, first_only)
    if key in _RUNS:
        return _RUNS[key]
    cfg, ora, data0 = state(asset_root)
    data = ac._cast(copy.deepcopy(data0), dtype)
    smpl0, old = ora.smpl, torch.get_default_dtype()
    out = {}
    try:
        torch.set_default_dtype(dtype)
        ora.smpl = copy.deepcopy(smpl0).to(dtype)
        for si, (stage, spec) in enumerate(ora.opt_stage_specs.items()):
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
            ora.pen_weight, ora.pen_values = weight, []
            n = min(K, spec['opt_niters'])
            for it in range(n):
                ora.cur_iter = it
                if it == 0:
                    if si == 0:
                        ora.pen_weight = None
                        closure()
                        out.update({'grad0_without/%s' % k: v for k, v in _named(data, var, ora.specs, 'grad').items()})
                        ora.pen_weight = weight
                    closure()
                    ora.pen_values.pop()
                    out.update({'%s/grad/%s' % (stage, k): v for k, v in _named(data, var, ora.specs, 'grad').items()})
                    if si == 0:
                        out['frames'] = ora.pen_frames.copy()
                    if first_only:
                        break
                opt.step(closure)
            for p in params:
                p.requires_grad_(False)
            if first_only:
                break
            out['%s/history' % stage] = np.asarray(ora.pen_values, np.float64)[None]            # (1, K): the value each iteration started from
            if stage == list(ora.opt_stage_specs)[-1]:
                out.update({'%s/param/%s' % (stage, k): v for k, v in _named(data, var, ora.specs).items()})
                for idx, d in data['person_data'].items():
                    out['%s/orient/p%d' % (stage, idx)] = d['smpl_orient_world'].detach().double().numpy().copy()
                    out['%s/trans/p%d' % (stage, idx)] = d['root_trans_world'].detach().double().numpy().copy()
            data['cam_pose'], data['cam_pose_inv'] = data['cam_pose'].detach(), data['cam_pose_inv'].detach()
            if spec.get('reinitialize_cam', False):
                data['cam_pose'][:] = data['cam_pose'][[0]]
                data['cam_pose_inv'] = tf.invert_transform(data['cam_pose'])
    finally:
        ora.smpl, ora.pen_weight, ora.cur_iter = smpl0, None, 0
        torch.set_default_dtype(old)
    _RUNS[key] = out
    return out


def errors(got, ref):
    """Worst error per kind (tests/extra_loss_e2e.errors: gradients and variables relative to the variable's largest reference entry, poses
    absolute) and `history`: absolute, over stages and iterations."""
    keys = [k for k in ref if '/' in k and k.split('/')[1] in ('grad', 'param', 'orient', 'trans') and not k.startswith('grad0_without')]
    out = _errors({k: got[k] for k in keys}, {k: ref[k] for k in keys})
    hk = [k for k in ref if k.endswith('/history')]
    out['history'] = max([float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) for k in hk] or [0.0])
    return out


def term_share(ref):
    """|first gradient with the term - without| / |first gradient with the term| over the first stage's variables (2-norms)."""
    first = next(k.split('/')[0] for k in ref if '/grad/' in k)
    names = [k.split('/', 2)[2] for k in ref if k.startswith(first + '/grad/')]
    num = np.sqrt(sum(((ref['%s/grad/%s' % (first, n)] - ref['grad0_without/%s' % n]) ** 2).sum() for n in names))
    den = np.sqrt(sum((ref['%s/grad/%s' % (first, n)] ** 2).sum() for n in names))
    return float(num / den)


# fp32 run of the port against its fp64 run (one thread), rounded up to two digits
FLOOR = {'grad': 2.1e-04, 'param': 6.4e-04, 'orient': 7.5e-07, 'trans': 4.1e-07, 'history': 1.3e-06}      # 2.025e-04, 6.096e-04, 7.109e-07, 3.951e-07, 1.252e-06
FLOOR_FIRST_GRAD = 2.025e-04          # the first stage's first gradient alone (what tests/test_penetration_ref.py measures again)
TOL = {k: FLOOR_FACTOR * v for k, v in FLOOR.items()}


def measure_floor(asset_root, first_only=False):
    from tests.traj_ref_common import single_thread
    with single_thread():
        return errors(reference(asset_root, torch.float32, first_only=first_only), reference(asset_root, first_only=first_only))


if __name__ == '__main__':
    import tempfile
    import time
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    t0 = time.time()
    ref = reference(root)
    print('fp64 run: %.0f s; frames with a non-zero term: %d; share of the first gradient: %.3f' % (time.time() - t0, int((ref['frames'] > 0).sum()), term_share(ref)))
    print({k: v for k, v in ref.items() if k.endswith('/history')})
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', FIXTURE + '.npz'), **ref)
    f = measure_floor(root)
    up = {k: (0.0 if v == 0 else float('%.1e' % (v * 1.05))) for k, v in f.items()}
    _RUNS.clear()
    print('FLOOR_FIRST_GRAD = %.3e' % measure_floor(root, first_only=True)['grad'])
    print("FLOOR = {%s}      # %s" % (', '.join("'%s': %.1e" % (k, up[k]) for k in KINDS), ', '.join('%.3e' % f[k] for k in KINDS)))
