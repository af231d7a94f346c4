"""DEVELOPMENT AID (GPU): what a caller-defined loss term costs.
  1. glamr_grecon_pose_backward at n_slots x frames (default 1024 x 300, one person per scene, both upstream arrays, every variable, world_dheading on):
     ms per call, device events around REPS calls, median of ROUNDS rounds after a warm-up.
  2. One iteration of extra_loss_schedule.ExtraLossSchedule on ONE sequence of `frames` frames: with the zero-term callback
     (0 * trans_world.sum) and with the term skipped (the gradient launch and the Adam step alone), us per iteration, host clock around ITERS
     iterations that end in a device synchronise.
usage: python tools/extra_loss_time.py [n_slots] [frames]"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from glamr_amd import _lib
from glamr_amd.global_recon import extra_loss_schedule as xs, packing
from glamr_amd.utils import synth

B, T = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024), (int(sys.argv[2]) if len(sys.argv) > 2 else 300)
REPS, ROUNDS, ITERS = 20, 7, 50
dev = torch.device('cuda:0')
g = torch.Generator(device='cpu').manual_seed(0)

# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
l = packing.param_layout_py(1, T)
prior = torch.zeros((B, T, 11))
prior[..., :2] = 0.03 * torch.randn((B, T, 2), generator=g)
prior[..., 2] = 0.9
prior[..., 3:9] = torch.tensor([1.0, 0, 0, 0, 1.0, 0]) + 0.2 * torch.randn((B, T, 6), generator=g)
prior[..., 9] = 1.0 + 0.1 * torch.randn((B, T), generator=g)
prior[..., 10] = 0.05 * torch.randn((B, T), generator=g)
t = dict(n_persons=torch.ones(B, dtype=torch.int32), seq_len=torch.full((B,), T, dtype=torch.int32), fr_start=torch.zeros(B, dtype=torch.int32),
         fr_end=torch.full((B,), T, dtype=torch.int32), traj_local_pred=prior, base_orient=torch.zeros((B, T, 3)), dheading_mask=torch.ones((B, T)),
         params=1e-2 * torch.randn((B, l['scene_stride']), generator=g))
t = {k: v.to(dev) for k, v in t.items()}
sb = _lib.SceneBatch()
sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = B, 1, T, packing.NJ
for k, v in t.items():
    setattr(sb, k, ctypes.c_void_p(v.data_ptr()))
sd = _lib.StageDesc()
sd.var_mask = sum(v for k, v in packing.VAR_BITS.items() if k != 'cam')
sd.flags = packing.FLAG_HAS_WORLD_DHEADING
G = [torch.randn((B, T, 3), generator=g).to(dev) for _ in range(2)]
grads = torch.zeros((B, l['scene_stride']), device=dev)
L = _lib.lib()
ws = torch.empty(L.glamr_grecon_pose_backward_workspace_bytes(B, 1, T), dtype=torch.uint8, device=dev)


def pose_backward():
    _lib.check(L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(G[0]), _lib.ptr(G[1]), _lib.ptr(grads), 0, _lib.ptr(ws), _lib.current_stream()))


def ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


pose_backward()
torch.cuda.synchronize()
v = [ms(pose_backward, REPS) for _ in range(ROUNDS)]
print('pose_backward   %9.3f ms per call (median of %d rounds of %d calls; min %.3f, max %.3f)  [%d x %d frames]' % (float(np.median(v)), ROUNDS, REPS, min(v), max(v), B, T))

# ---- 2. one iteration of the schedule ----------------------------------------------------------------------------------------------------------
model = bench.build_model(bench.ensure_assets(), dev)
in_dict = synth.make_in_dict(seed=0, num_frames=T, num_persons=1, smpl_model=synth.make_smpl_model())
model.extra_loss = lambda ctx: 0 * ctx.trans_world.sum((1, 2, 3))


def iteration_us(skip):
    datas, packed = model.init_data_batch([in_dict], init_forward=False)
    sched = xs.ExtraLossSchedule(model, packed, skip_term=skip)
    sched.run(max_iters=3)                                      # warm-up: allocations, the body model's handle
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sched.run(max_iters=ITERS)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (ITERS * len(model.opt_stage_specs))


res = {False: [], True: []}
for _ in range(ROUNDS):
    for skip in (True, False):
        res[skip].append(iteration_us(skip))
for skip, name in ((True, 'term skipped'), (False, 'zero-term callback')):
    print('schedule iteration, %-18s %8.1f us (median of %d rounds of %d iterations; min %.1f, max %.1f)  [one sequence of %d frames]'
          % (name + ':', float(np.median(res[skip])), ROUNDS, ITERS, min(res[skip]), max(res[skip]), T))
