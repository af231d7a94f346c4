"""DEVELOPMENT AID (GPU): the local-to-global step's VJP next to its forward, and inference_grad next to inference.
  1. glamr_traj_local_to_global_backward at n_seq x frames (default 1024 x 300, every upstream gradient given) beside glamr_traj_local_to_global
     of the same build on the same box: ms per call, device events around REPS calls, the two alternated over ROUNDS rounds after a warm-up.
     (The forward call copies its lengths and ends with a stream synchronise; the backward only launches.)
  2. forward + backward of MotionTrajJointModel.inference_grad (L = sum of the translation and the orientation, both latents' gradients) for ONE
     sequence of `frames` frames beside inference(sample_num=1): ms per call, host clock around calls that end in a device synchronise.
The median round is reported with the spread.  usage: python tools/global_vjp_time.py [n_seq] [frames]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from glamr_amd.models import priors as pr

B, T = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024), (int(sys.argv[2]) if len(sys.argv) > 2 else 300)
REPS, ROUNDS = 20, 7
dev = torch.device('cuda:0')
g = torch.Generator(device='cpu').manual_seed(0)
L = torch.zeros((B, T, 11))
L[..., :2] = 0.03 * torch.randn((B, T, 2), generator=g)
L[..., 2] = 0.9
L[..., 3:9] = torch.tensor([1.0, 0, 0, 0, 1.0, 0]) + 0.2 * torch.randn((B, T, 6), generator=g)
L[..., 9] = 1.0 + 0.1 * torch.randn((B, T), generator=g)
L[..., 10] = 0.05 * torch.randn((B, T), generator=g)
L = L.to(dev)
G = [torch.randn((B, T, w), generator=g).to(dev) for w in (3, 3, 4)]
lens = torch.full((B,), T, dtype=torch.int32, device=dev)


def forward():
    pr.local_to_global(L)


def backward():
    pr.local_to_global_backward(L, lens, *G)


def ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def report(fns, timer, reps, what):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    res = {fn.__name__: [] for fn in fns}
    for _ in range(ROUNDS):
        for fn in fns:
            res[fn.__name__].append(timer(fn, reps))
    for k, v in res.items():
        print('%-15s %9.3f ms per call (median of %d rounds of %d calls; min %.3f, max %.3f)  [%s]' % (k, float(np.median(v)), ROUNDS, reps, min(v), max(v), what))
    return {k: float(np.median(v)) for k, v in res.items()}


r = report((forward, backward), ms, REPS, '%d x %d frames' % (B, T))
print('backward / forward = %.2f' % (r['backward'] / r['forward']))

model = bench.build_model(bench.ensure_assets(), dev)
mt = model.mt_model
nw = pr.num_windows(T)
batch = dict(in_body_pose=(0.3 * torch.randn((1, T, 69), generator=g)).to(dev), frame_mask=torch.ones((1, T), device=dev),
             in_motion_latent=torch.randn((nw, 128), generator=g).to(dev), in_traj_latent=torch.randn((1, 128), generator=g).to(dev))


def inference():
    with torch.no_grad():
        mt.inference(batch, sample_num=1)


def inference_grad():
    me, te = batch['in_motion_latent'].clone().requires_grad_(True), batch['in_traj_latent'].clone().requires_grad_(True)
    out = mt.inference_grad(dict(batch, in_motion_latent=me, in_traj_latent=te))
    (out['infer_out_trans'].sum() + out['infer_out_orient'].sum()).backward()


r = report((inference, inference_grad), wall_ms, 5, 'one sequence of %d frames' % T)
print('inference_grad (forward + backward) / inference = %.2f' % (r['inference_grad'] / r['inference']))
