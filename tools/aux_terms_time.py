"""DEVELOPMENT AID (GPU): what the six loss_cfg terms of packing.AUX_LOSS_IDS cost, device events as tools/penetration_time.py
takes them (an event pair around the work, median of ROUNDS rounds after a warm-up).
  1. glamr_grecon_aux_terms alone on the scene's batch: all six terms, add mode, REPS calls per round.
  2. One iteration of extra_loss_schedule.ExtraLossSchedule on ONE 2-person scene of `frames` frames (default 100, glamr_dynamic_multi), three
     ways: with the terms in loss_cfg (the four that run everywhere in both stages, the two on the camera variables where `cam` is optimised);
     with skip_term (the parent's path: gradient launch + Adam step); and with the same terms written in torch as a caller's extra_loss -- the
     three on trans_world / cam_pose through autograd and the VJP kernels, the three on variables evaluated from params for their values only (a
     callback cannot reach the variables, so those give no gradient there).
usage: python tools/aux_terms_time.py [frames]"""
import copy, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from glamr_amd import _lib
from glamr_amd.global_recon import extra_loss_schedule as xs, packing
from glamr_amd.global_recon.configs import get_config
from glamr_amd.global_recon.models import model_dict
from glamr_amd.utils import synth

T = int(sys.argv[1]) if len(sys.argv) > 1 else 100
ROUNDS, ITERS, REPS = 7, 20, 20
dev = torch.device('cuda:0')
L = _lib.lib()
EVERYWHERE = {'cam_depth_smoothness': dict(weight=1.0e3), 'traj_trans_smoothness': dict(weight=1.0e2), 'cam_traj_trans': dict(weight=1.0e4, first_frame_weight=10.0),
              'local_traj_dheading_reg': dict(weight=1.0e3)}
ON_CAM = {'cam_rot_smoothness': dict(weight=1.0e3), 'cam_trans_smoothness': dict(weight=1.0e3)}


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def config(with_terms):
    cfg = copy.deepcopy(get_config('glamr_dynamic_multi'))
    if with_terms:
        for spec in cfg['opt_stage_specs'].values():
            spec['loss_cfg'].update(copy.deepcopy(EVERYWHERE))
            if 'cam' in spec['opt_variables']:
                spec['loss_cfg'].update(copy.deepcopy(ON_CAM))
    return cfg


assets = bench.ensure_assets()
base = bench.build_model(assets, dev)
make = lambda cfg: model_dict['global_recon_model'](cfg, dev, None, smpl=base.smpl, mt_model=base.mt_model)      # noqa: E731
in_dict = synth.make_in_dict(seed=0, num_frames=T, num_persons=2, smpl_model=synth.make_smpl_model())
model, plain = make(config(True)), make(config(False))


def torch_terms(packed):
    """The six definitions in torch on what a callback is given (module docstring)."""
    S, P, T_ = packed.S, packed.P, packed.T
    rtc, l = packed.person_arrays['trans_cam'].view(S, P, T_, 3), packed.layout

    def fn(ctx):
        cam, x, vis = ctx.cam_pose, ctx.trans_world, ctx.vis.float()
        R, c = cam[..., :3], cam[..., 3]
        o = -torch.matmul(R.transpose(-1, -2), c.unsqueeze(-1)).squeeze(-1)
        depth = (30 * ((o[:, :-1] - o[:, 1:]) * R[:, 1:, 2, :]).sum(-1)).pow(2).sum(1)
        traj = ((x[:, :, 1:] - x[:, :, :-1]) * 30).pow(2).sum((1, 2, 3)) / (P * (T_ - 1))
        diff = torch.matmul(R[:, None], x.unsqueeze(-1)).squeeze(-1) + c[:, None] - rtc
        first = (vis.cumsum(-1) == 1) & (vis > 0)
        w = torch.where(first, torch.full_like(vis, 10.0), torch.ones_like(vis)) * vis
        cam_traj = (diff * w.unsqueeze(-1)).pow(2).sum((1, 2, 3)) / vis.sum((1, 2))
        prm = packed.t['params']
        total = 1.0e3 * depth + 1.0e2 * traj + 1.0e4 * cam_traj
        if 'cam' in model.opt_stage_specs[ctx.stage]['opt_variables']:
            r6, tr = prm[:, l['cam_rot6d']:l['cam_rot6d'] + 6 * T_].view(S, T_, 6), prm[:, l['cam_trans']:l['cam_trans'] + 3 * T_].view(S, T_, 3)
            total = total + 0.0 * (((r6[:, :-1] - r6[:, 1:]) * 30).pow(2).sum((1, 2)) + ((tr[:, :-1] - tr[:, 1:]) * 30).pow(2).sum((1, 2))) / (T_ - 1)
        dh = torch.stack([prm[:, l['person0'] + p * l['person_stride'] + l['local_dheading']:][:, 1:T_] for p in range(P)], 1)
        return total + 0.0 * (dh * 30).pow(2).sum((1, 2)) / (P * (T_ - 1))
    return fn


def iteration_ms(which):
    m = model if which == 'terms' else plain
    datas, packed = m.init_data_batch([in_dict], init_forward=False)
    m.extra_loss = torch_terms(packed) if which == 'callback' else (lambda ctx: 0.0 * ctx.trans_world.sum((1, 2, 3))) if which == 'skipped' else None
    sched = xs.ExtraLossSchedule(m, packed, skip_term=which == 'skipped')
    sched.run(max_iters=2)                                     # warm-up
    torch.cuda.synchronize()
    t = ms(lambda: sched.run(max_iters=ITERS)) / (ITERS * len(m.opt_stage_specs))
    m.extra_loss = None
    return t, packed


res = {k: [] for k in ('terms', 'skipped', 'callback')}
for _ in range(ROUNDS):
    for k in res:
        t, packed = iteration_ms(k)
        res[k].append(t)
for k, what in (('terms', 'the six terms (loss_cfg)'), ('skipped', 'terms skipped (parent path)'), ('callback', 'the terms as a torch callback')):
    print('schedule iteration, %-30s %9.3f ms (device events around %d iterations per stage, median of %d rounds; min %.3f, max %.3f)  [2 persons, %d frames]'
          % (what + ':', float(np.median(res[k])), ITERS, ROUNDS, min(res[k]), max(res[k]), T))

# ---- the kernel alone, on the last batch -----------------------------------------------------------------------------------------------------
S, P = packed.S, packed.P
sd = packing.stage_desc(list(model.opt_stage_specs.values())[-1], model.specs, niters=1)
ad = packing.aux_desc(list(model._aux_cfg.values())[-1])
values, g_t, g_c = torch.empty((S, 6), device=dev), torch.zeros((S * P, T, 3), device=dev), torch.zeros((S, T, 12), device=dev)
grads = torch.zeros_like(packed.t['params'])
ws = torch.empty(max(L.glamr_grecon_aux_terms_workspace_bytes(S, P, T), 4), dtype=torch.uint8, device=dev)
sb = packed.struct()


def call():
    _lib.check(L.glamr_grecon_aux_terms(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), _lib.ptr(packed.person_arrays['trans_cam']), _lib.ptr(values), _lib.ptr(g_t),
                                        _lib.ptr(g_c), _lib.ptr(grads), 1, _lib.ptr(ws), _lib.current_stream()))


call()
torch.cuda.synchronize()
v = [ms(lambda: [call() for _ in range(REPS)]) / REPS for _ in range(ROUNDS)]
print('glamr_grecon_aux_terms, %d scene(s) x %d persons x %d frames, all terms of the last stage, add mode: %.4f ms per call (median of %d rounds of %d calls; min %.4f, max %.4f)'
      % (S, P, T, float(np.median(v)), ROUNDS, REPS, min(v), max(v)))
