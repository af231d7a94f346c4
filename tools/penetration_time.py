"""DEVELOPMENT AID (GPU): what the multi-person penetration term costs.
  1. glamr_sdf_penetration at the workload's shape -- SMPL's 6890 vertices, 13 776 faces (random index triples: the kernels' time
     depends on the counts, not on the surface), grid 32, `meshes` meshes (default 64 = 32 frames x 2 persons, every pair
     overlapping): device events around the call (boxes + grid + sample + finish), and around the same call with the persons shifted apart
     (boxes, early exits, zero stores), median of ROUNDS rounds after a warm-up; the two launches the difference holds are told apart by a
     kernel trace (`frames` = 0 runs this part alone).  The difference as sdf_grid_kernel's: (voxel, face) pairs per second and, at FLOP_PER_PAIR counted from csrc/sdf.hpp, the fraction of the fp32 vector
     peak of the MI355X (157.3 TFLOP/s with packed fp32, which this library's build switches off: half of it is the reachable rate).
  2. One iteration of extra_loss_schedule.ExtraLossSchedule with the built-in term on ONE 2-person scene of `frames` frames (default 100) in
     which the persons' boxes overlap on 20 frames, against the same iteration with the term skipped (skip_term): us per iteration, host clock
     around ITERS iterations that end in a device synchronise.
usage: python tools/penetration_time.py [meshes] [frames]"""
import copy, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from glamr_amd import _lib
from glamr_amd.global_recon import extra_loss_schedule as xs
from glamr_amd.global_recon.configs import get_config
from glamr_amd.global_recon.models import model_dict
from glamr_amd.utils import synth

M, T = (int(sys.argv[1]) if len(sys.argv) > 1 else 64), (int(sys.argv[2]) if len(sys.argv) > 2 else 100)
V, NF, G = 6890, 13776, 32
ROUNDS, ITERS = 7, 20
PEAK_TFLOPS = 157.3
# one (voxel, face) evaluation of sdf.hpp point_face, multiply-adds as 2: corners 9, three segments 3 x 20, plane and interior test 22,
# lengths and dots 36 (sqrt as 1), denominator 7, atan2 21 (division as 1), minima and sum 3
FLOP_PER_PAIR = 158
dev = torch.device('cuda:0')
L = _lib.lib()


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(0)
F_, P = M // 2, 2
unit = rng.standard_normal((V, 3))
unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True) * (0.3 + 0.05 * rng.random((V, 1)))).astype(np.float32)
faces = torch.tensor(rng.integers(0, V, size=(NF, 3)).astype(np.int32), device=dev)      # (timing only: counts, not a closed surface)
verts = np.stack([np.stack([unit, unit + np.float32([0.25, 0.05, 0.0])])] * F_)
apart = verts.copy()
apart[:, 1] += 10.0
active = torch.ones((F_, P), dtype=torch.uint8, device=dev)
loss, g = torch.empty(F_, device=dev), torch.empty((F_, P, V, 3), device=dev)
ws = torch.empty(L.glamr_sdf_workspace_bytes(F_, P, V, NF, G), dtype=torch.uint8, device=dev)


def call(x):
    _lib.check(L.glamr_sdf_penetration(_lib.ptr(x), _lib.ptr(active), _lib.ptr(faces), F_, P, V, NF, G, 0.2, 1.0, _lib.ptr(loss), _lib.ptr(g), None, None, None,
                                       _lib.ptr(ws), _lib.current_stream()))


x_on, x_off = torch.tensor(verts, device=dev), torch.tensor(apart, device=dev)
call(x_on), call(x_off)
torch.cuda.synchronize()
full = [ms(lambda: call(x_on)) for _ in range(ROUNDS)]
idle = [ms(lambda: call(x_off)) for _ in range(ROUNDS)]
grid_ms = float(np.median(full)) - float(np.median(idle))
pairs = float(M) * G ** 3 * NF
print('glamr_sdf_penetration, %d meshes of %d vertices / %d faces, grid %d: %.3f ms per call (median of %d; min %.3f, max %.3f); the same call with '
      'nobody overlapping (boxes, early exits, zero stores): %.3f ms (min %.3f, max %.3f)' % (M, V, NF, G, float(np.median(full)), ROUNDS, min(full), max(full),
                                                                                             float(np.median(idle)), min(idle), max(idle)))
print('sdf_grid_kernel + sdf_sample_kernel (difference): %.3f ms = %.3e (voxel, face) pairs/s = %.1f TFLOP/s at %d FLOP per pair = %.1f %% of the %.1f TFLOP/s fp32 '
      'vector peak (packed fp32, switched off in this build: %.1f %% of the unpacked rate)'
      % (grid_ms, pairs / (grid_ms * 1e-3), pairs * FLOP_PER_PAIR / (grid_ms * 1e-3) / 1e12, FLOP_PER_PAIR, 100 * pairs * FLOP_PER_PAIR / (grid_ms * 1e-3) / 1e12 / PEAK_TFLOPS,
         PEAK_TFLOPS, 200 * pairs * FLOP_PER_PAIR / (grid_ms * 1e-3) / 1e12 / PEAK_TFLOPS))
print('per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/penetration_time.py %d 0   (frames 0: part 1 only)' % M)
if T == 0:
    sys.exit(0)

# ---- 2. one iteration of the schedule ----------------------------------------------------------------------------------------------------------
assets = bench.ensure_assets()
base = bench.build_model(assets, dev)
cfg = copy.deepcopy(get_config('glamr_dynamic_multi'))
cfg['grecon_model_specs']['flag_use_pen_loss'] = True
for spec in cfg['opt_stage_specs'].values():
    spec['loss_cfg']['penetration'] = dict(weight=1.0)
model = model_dict['global_recon_model'](cfg, dev, None, smpl=base.smpl, mt_model=base.mt_model)
in_dict = synth.make_in_dict(seed=0, num_frames=T, num_persons=2, smpl_model=synth.make_smpl_model(), gap=(0, 0))
est = in_dict['est']
near = est[0]['root_trans'][est[1]['frames']] + np.float32([0.25, 0.0, 0.05])
sel = est[1]['frames'] < 20                                   # the first 20 frames: person 1 stands beside person 0
est[1]['root_trans'] = np.where(sel[:, None], near, est[1]['root_trans'] + np.float32([3.0, 0.0, 0.0])).astype(np.float32)


def iteration_us(skip):
    datas, packed = model.init_data_batch([in_dict], init_forward=False)
    sched = xs.ExtraLossSchedule(model, packed, skip_term=skip)
    sched.run(max_iters=2)                                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sched.run(max_iters=ITERS)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (ITERS * len(model.opt_stage_specs))


res = {True: [], False: []}
for _ in range(ROUNDS):
    for skip in (True, False):
        res[skip].append(iteration_us(skip))
print('overlapping frames at the last iteration (penetration_history non-zero): value %s' % {k: float(v[0, -1]) for k, v in model.penetration_history.items()})
for skip, what in ((True, 'term skipped'), (False, 'penetration term')):
    print('schedule iteration, %-18s %9.1f us (median of %d rounds of %d iterations; min %.1f, max %.1f)  [2 persons, %d frames, 20 beside each other]'
          % (what + ':', float(np.median(res[skip])), ROUNDS, ITERS, min(res[skip]), max(res[skip]), T))
