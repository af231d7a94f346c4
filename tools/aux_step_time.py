"""DEVELOPMENT AID (GPU): what an Adam iteration with the six loss_cfg terms of packing.AUX_LOSS_IDS costs on the device-only path (DESIGN.md
20), on the scene and settings of tools/aux_terms_time.py (ONE 2-person scene of `frames` frames, default 100, glamr_dynamic_multi with the four
terms that run everywhere in both stages and the two on the camera variables where `cam` is optimised), device events as that tool takes them
(an event pair around the work, median of ROUNDS rounds after a warm-up).
  1. One schedule iteration three ways: extra_loss_schedule.ExtraLossSchedule (the flag off: the parent's path), aux_step_schedule.AuxStepSchedule
     with plain launches, and the same schedule captured once into a HIP graph and replayed.
  2. glamr_grecon_aux_step alone on the scene's batch, REPS calls per round.
usage: python tools/aux_step_time.py [frames]"""
import copy, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from glamr_amd import _lib
from glamr_amd.global_recon import aux_step_schedule, extra_loss_schedule as xs, packing, stepwise
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


def config(on_device):
    cfg = copy.deepcopy(get_config('glamr_dynamic_multi'))
    cfg['grecon_model_specs']['flag_aux_on_device'] = on_device
    for spec in cfg['opt_stage_specs'].values():
        spec['loss_cfg'].update(copy.deepcopy(EVERYWHERE))
        if 'cam' in spec['opt_variables']:
            spec['loss_cfg'].update(copy.deepcopy(ON_CAM))
    return cfg


assets = bench.ensure_assets()
base = bench.build_model(assets, dev)
make = lambda cfg: model_dict['global_recon_model'](cfg, dev, None, smpl=base.smpl, mt_model=base.mt_model)      # noqa: E731
in_dict = synth.make_in_dict(seed=0, num_frames=T, num_persons=2, smpl_model=synth.make_smpl_model())
fused, parent = make(config(True)), make(config(False))
side = torch.cuda.Stream(device=dev)


def iteration_ms(which):
    m = parent if which == 'parent' else fused
    datas, packed = m.init_data_batch([in_dict], init_forward=False)
    sched = xs.ExtraLossSchedule(m, packed) if which == 'parent' else aux_step_schedule.AuxStepSchedule(m, packed)
    sched.run(max_iters=2)                                     # warm-up
    torch.cuda.synchronize()
    if which == 'captured':
        graph = stepwise.capture_iteration(lambda: sched.run(max_iters=ITERS), dev, side)
        graph.replay()
        torch.cuda.synchronize()
        run = graph.replay
    else:
        run = lambda: sched.run(max_iters=ITERS)               # noqa: E731
    return ms(run) / (ITERS * len(m.opt_stage_specs)), packed


res = {k: [] for k in ('parent', 'plain', 'captured')}
for _ in range(ROUNDS):
    for k in res:
        t, packed = iteration_ms(k)
        res[k].append(t)
for k, what in (('parent', 'ExtraLossSchedule (parent path)'), ('plain', 'AuxStepSchedule, plain launches'), ('captured', 'AuxStepSchedule, captured step')):
    print('schedule iteration, %-34s %9.3f ms (device events around %d iterations per stage, median of %d rounds; min %.3f, max %.3f)  [2 persons, %d frames]'
          % (what + ':', float(np.median(res[k])), ITERS, ROUNDS, min(res[k]), max(res[k]), T))

# ---- the kernel alone, on the last batch -----------------------------------------------------------------------------------------------------
S, P = packed.S, packed.P
sd = packing.stage_desc(list(fused.opt_stage_specs.values())[-1], fused.specs, niters=1)
ad = packing.aux_desc(list(fused._aux_cfg.values())[-1])
values = torch.empty((S, 6), device=dev)
grads, m_, v_ = (torch.zeros_like(packed.t['params']) for _ in range(3))
ws = torch.empty(max(L.glamr_grecon_aux_step_workspace_bytes(S, P, T), 4), dtype=torch.uint8, device=dev)
sb = packed.struct()


def call():
    _lib.check(L.glamr_grecon_aux_step(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), _lib.ptr(packed.person_arrays['trans_cam']), _lib.ptr(values), 6, 0,
                                       _lib.ptr(grads), _lib.ptr(m_), _lib.ptr(v_), 1e-4, 1, _lib.ptr(ws), _lib.current_stream()))


call()
torch.cuda.synchronize()
v = [ms(lambda: [call() for _ in range(REPS)]) / REPS for _ in range(ROUNDS)]
print('glamr_grecon_aux_step, %d scene(s) x %d persons x %d frames, all terms of the last stage: %.4f ms per call (median of %d rounds of %d calls; min %.4f, max %.4f)'
      % (S, P, T, float(np.median(v)), ROUNDS, REPS, min(v), max(v)))
