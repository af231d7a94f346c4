"""DEVELOPMENT AID (GPU): what a caller-defined loss term on the camera costs.
  1. glamr_grecon_cam_backward at n_scenes x frames (default 1024 x 300) in each camera mode -- per frame, fixed, derived from the persons (two
     persons per scene, frames 100-159 see nobody, 160-199 one person) -- store mode: ms per call, device events around REPS calls, median of
     ROUNDS rounds after a warm-up.
  2. One iteration of extra_loss_schedule.ExtraLossSchedule on ONE sequence of `frames` frames (the benchmark's model: per-frame camera): with
     a zero-term callback on the camera (0 * cam_pose.sum: the camera VJP runs, the pose VJP does not), on the poses (0 * trans_world.sum:
     DESIGN.md 15's figure) and with the term skipped, us per iteration, host clock around ITERS iterations that end in a device synchronise.
usage: python tools/extra_loss_cam_time.py [n_scenes] [frames]"""
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
L = _lib.lib()


def ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
for mode, P in (('per frame', 1), ('fixed', 1), ('derived', 2)):
    l = packing.param_layout_py(P, T)
    vis = torch.ones((B * P, T))
    if mode == 'derived' and T > 200:
        vis[:, 100:160] = 0.0
        vis[1::2, 160:200] = 0.0
    params = 1e-2 * torch.randn((B, l['scene_stride']), generator=g)
    params[:, :6 * T] += torch.tensor([1.0, 0, 0, 0, 1.0, 0]).repeat(T)
    p2c = torch.zeros((B * P, T, 3, 4))
    p2c[..., :3, :3] = torch.eye(3)
    p2c[..., 3] = torch.randn((B * P, T, 3), generator=g)
    t = dict(n_persons=torch.full((B,), P, dtype=torch.int32), seq_len=torch.full((B,), T, dtype=torch.int32), vis=vis, params=params,
             orient_world=0.3 * torch.randn((B * P, T, 3), generator=g), trans_world=torch.randn((B * P, T, 3), generator=g), person2cam=p2c)
    t = {k: v.contiguous().to(dev) for k, v in t.items()}
    sb = _lib.SceneBatch()
    sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = B, P, T, packing.NJ
    for k, v in t.items():
        setattr(sb, k, ctypes.c_void_p(v.data_ptr()))
    sd = _lib.StageDesc()
    sd.var_mask = 0 if mode == 'derived' else packing.VAR_BITS['cam']
    sd.flags = {'per frame': 0, 'fixed': packing.FLAG_FIXED_CAM, 'derived': packing.FLAG_CAM_FROM_PERSON}[mode]
    G = torch.randn((B, T, 12), generator=g).to(dev)
    grads = torch.zeros((B, l['scene_stride']), device=dev)
    pose = [torch.zeros((B * P, T, 3), device=dev) for _ in range(2)]
    ws = torch.empty(L.glamr_grecon_cam_backward_workspace_bytes(B, P, T), dtype=torch.uint8, device=dev)

    def cam_backward():
        _lib.check(L.glamr_grecon_cam_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(G), _lib.ptr(grads), 0, _lib.ptr(pose[0]), _lib.ptr(pose[1]), _lib.ptr(ws),
                                               _lib.current_stream()))

    cam_backward()
    torch.cuda.synchronize()
    v = [ms(cam_backward, REPS) for _ in range(ROUNDS)]
    print('cam_backward, %-10s %9.3f ms per call (median of %d rounds of %d calls; min %.3f, max %.3f)  [%d scenes x %d frames, %d person(s)]'
          % (mode + ':', float(np.median(v)), ROUNDS, REPS, min(v), max(v), B, T, P))

# ---- 2. one iteration of the schedule ----------------------------------------------------------------------------------------------------------
model = bench.build_model(bench.ensure_assets(), dev)
in_dict = synth.make_in_dict(seed=0, num_frames=T, num_persons=1, smpl_model=synth.make_smpl_model())
TERMS = {'camera': lambda ctx: 0 * ctx.cam_pose.sum((1, 2, 3)), 'poses': lambda ctx: 0 * ctx.trans_world.sum((1, 2, 3)), 'skipped': None}


def iteration_us(name):
    model.extra_loss = TERMS[name] or TERMS['poses']
    datas, packed = model.init_data_batch([in_dict], init_forward=False)
    sched = xs.ExtraLossSchedule(model, packed, skip_term=TERMS[name] is None)
    sched.run(max_iters=3)                                      # warm-up: allocations, the body model's handle
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sched.run(max_iters=ITERS)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (ITERS * len(model.opt_stage_specs))


res = {k: [] for k in TERMS}
for _ in range(ROUNDS):
    for name in TERMS:
        res[name].append(iteration_us(name))
for name, what in (('skipped', 'term skipped'), ('poses', 'zero term on the poses'), ('camera', 'zero term on the camera')):
    print('schedule iteration, %-24s %8.1f us (median of %d rounds of %d iterations; min %.1f, max %.1f)  [one sequence of %d frames]'
          % (what + ':', float(np.median(res[name])), ROUNDS, ITERS, min(res[name]), max(res[name]), T))
