"""DEVELOPMENT AID (GPU): the trajectory predictor's taped forward, its backward and the untaped forward of the same build, ms per call for
1024 sequences x 300 frames (device events around REPS calls each, the three alternated over ROUNDS rounds after a warm-up of every shape;
the median round is reported with the spread).  The recurrence kernel's share: run this script under a kernel trace with statistics;
lstm_bwd_mfma_kernel is launched twice per backward, `frames` steps each.  usage: python tools/traj_vjp_time.py [n_seq] [frames]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench

B, T = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024), (int(sys.argv[2]) if len(sys.argv) > 2 else 300)
REPS, ROUNDS = 5, 5
dev = torch.device('cuda:0')
model = bench.build_model(bench.ensure_assets(), dev)
h = model.mt_model.handle
g = torch.Generator(device='cpu').manual_seed(0)
pose = (0.3 * torch.randn((B, T, 69), generator=g)).to(dev)
eps = torch.randn((B, 128), generator=g).to(dev)
G = torch.randn((B, T, 11), generator=g).to(dev)
lens = [T] * B
state = {}


def taped():
    state['out'], state['tape'] = h.traj_taped(lens, eps, in_body_pose=pose)


def backward():
    h.traj_backward(state['tape'], G)


def untaped():
    h.traj_clip(0, in_body_pose=pose, eps=eps, want=())


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


for fn in (taped, backward, untaped):
    fn()
torch.cuda.synchronize()
res = {fn.__name__: [] for fn in (taped, backward, untaped)}
for _ in range(ROUNDS):
    for fn in (taped, backward, untaped):
        res[fn.__name__].append(ms(fn))
for k, v in res.items():
    print('%-9s %8.2f ms per call (median of %d rounds of %d calls; min %.2f, max %.2f)  [%d x %d frames]' % (k, float(np.median(v)), ROUNDS, REPS, min(v), max(v), B, T))
print('backward / taped forward = %.2f, taped / untaped forward = %.2f' % (np.median(res['backward']) / np.median(res['taped']), np.median(res['taped']) / np.median(res['untaped'])))
