"""Development aid: bit-level fingerprints of the motion priors, for A/B runs of two builds of the library on one box (GLAMR_LIB_PATH selects
the build).  Prints one sha1 per case over every output array of every glamr_nets_* entry point -- a change of the host-side launch code
must keep every fingerprint.  glamr_nets_infer runs three times per case on the same buffers: plain launches, capture, replay.
usage: python tools/nets_bits.py                      (under `rocprofv3 --kernel-trace` for the launches themselves)
       python tools/nets_bits.py --kernel-list <kernel_trace.csv>    the trace as ordered (kernel, grid, workgroup) lines, to diff two builds"""
import csv, ctypes, glob, hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_list(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: (int(r['Start_Timestamp']), int(r.get('Dispatch_Id', 0))))
    for r in rows:
        print('%s grid=(%s,%s,%s) wg=(%s,%s,%s)' % (r['Kernel_Name'], r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z'],
                                                    r['Workgroup_Size_X'], r['Workgroup_Size_Y'], r['Workgroup_Size_Z']))


if len(sys.argv) > 2 and sys.argv[1] == '--kernel-list':
    kernel_list(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch
import bench
from glamr_amd import _lib
from glamr_amd.models import priors as P
from glamr_amd.utils import synth

dev = torch.device('cuda:0')
T = 120
NW = P.num_windows(T)


def sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()[:16]


def make_handle(root):
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    return P.MotionPriorsHandle(sd['inf'], sd['trj'], rest, synth.SMPL_PARENTS, dev)


def inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [T] + [int(x) for x in torch.randint(P.PAST + 1, T + 1, (B - 1,), generator=g)]      # ragged; the first one full length
    pose = (0.3 * torch.randn(B, T, 69, generator=g)).to(dev)
    vis = (torch.rand(B, T, generator=g) < 0.6).float().to(dev)
    vis[:, :P.PAST] = 1.0
    meps = torch.randn(B, NW, P.NZ, generator=g).to(dev)
    teps = torch.randn(B, P.NZ, generator=g).to(dev)
    return lens, pose, vis, meps, teps


def infer_case(h, B, flags, stream=None):
    """Three calls on the same buffers; returns the fingerprints of the three."""
    L = _lib.lib()
    lens, pose, vis, meps, teps = inputs(B, B)
    lens_np = np.ascontiguousarray(lens, dtype=np.int32)
    out = [torch.zeros(B, T, 69, device=dev), torch.zeros(B, T, 11, device=dev), torch.zeros(B, T, 3, device=dev), torch.zeros(B, T, 3, device=dev)]
    ws = torch.zeros(L.glamr_nets_workspace_bytes(h.h, B, T), dtype=torch.uint8, device=dev)
    res = []

    def call():
        infill, traj = flags & P.NETS_INFILL, flags & P.NETS_TRAJ
        _lib.check(L.glamr_nets_infer(h.h, B, T, _lib.ptr(lens_np), _lib.ptr(pose), _lib.ptr(vis) if infill else None, _lib.ptr(meps) if infill else None, NW,
                                      _lib.ptr(teps) if traj else None, _lib.ptr(out[0]) if infill else None, _lib.ptr(out[1]) if traj else None,
                                      _lib.ptr(out[2]) if traj else None, _lib.ptr(out[3]) if traj else None, flags, _lib.ptr(ws), _lib.current_stream()))
    if stream is None:
        for _ in range(3):
            for o in out:
                o.zero_()
            call()
            torch.cuda.synchronize()
            res.append(sha(*out))
    else:       # the call recorded into the caller's own graph, replayed twice
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
            call()
        for _ in range(2):
            for o in out:
                o.zero_()
            graph.replay()
            torch.cuda.synchronize()
            res.append(sha(*out))
    return ' '.join(res)


def taped_case(h, B):
    L = _lib.lib()
    lens, pose, vis, meps, _ = inputs(B, 1000 + B)
    lens_np = np.ascontiguousarray(lens, dtype=np.int32)
    out_pose = torch.zeros(B, T, 69, device=dev)
    tape = torch.zeros(L.glamr_nets_tape_bytes(h.h, B, T), dtype=torch.uint8, device=dev)
    _lib.check(L.glamr_nets_infill_taped(h.h, B, T, _lib.ptr(lens_np), _lib.ptr(pose), _lib.ptr(vis), _lib.ptr(meps), NW, _lib.ptr(out_pose), _lib.ptr(tape),
                                         _lib.current_stream()))
    torch.cuda.synchronize()
    fwd = sha(out_pose, tape)            # the pose and every kept activation (the gradient half of the arena is still zero)
    g_out = torch.randn(B, T, 69, generator=torch.Generator().manual_seed(B)).to(dev)
    g_eps = torch.zeros_like(meps)
    _lib.check(L.glamr_nets_infill_backward(h.h, B, T, _lib.ptr(lens_np), _lib.ptr(meps), NW, _lib.ptr(g_out), _lib.ptr(g_eps), _lib.ptr(tape),
                                            _lib.current_stream()))
    torch.cuda.synchronize()
    # the same inputs through glamr_nets_infer: is the taped pose the plain call's pose, bit for bit?
    plain = h.infer(pose, vis, lens, motion_eps=meps, traj=False)['pose']
    return '%s %s  taped pose == glamr_nets_infer pose: %s' % (fwd, sha(g_eps, tape), bool(torch.equal(plain, out_pose)))


def window_cases(h, B):
    g = torch.Generator().manual_seed(2000 + B)
    in_pose = (0.3 * torch.randn(B, 50, 69, generator=g)).to(dev)
    full = (0.3 * torch.randn(B, 50, 69, generator=g)).to(dev)
    mask = (torch.rand(B, 50, generator=g) < 0.6).float().to(dev)
    mask[:, :P.PAST] = 1.0
    eps = torch.randn(B, P.NZ, generator=g).to(dev)
    for mode in (P.VAE_INFER, P.VAE_TRAIN, P.VAE_RECON):
        out = h.infiller_window(mode, in_pose, mask, eps=eps, body_pose=None if mode == P.VAE_INFER else full)
        torch.cuda.synchronize()
        print('bits window B=%d mode=%d  %s' % (B, mode, sha(*[out[k] for k in sorted(out)])), flush=True)


def clip_cases(h, B):
    g = torch.Generator().manual_seed(3000 + B)
    pose = (0.3 * torch.randn(B, T, 69, generator=g)).to(dev)
    trans = torch.cumsum(0.02 * torch.randn(B, T, 3, generator=g), 1).to(dev)
    orient = (0.3 * torch.randn(B, T, 3, generator=g)).to(dev)
    eps = torch.randn(B, P.NZ, generator=g).to(dev)
    for mode in (P.VAE_INFER, P.VAE_TRAIN, P.VAE_RECON):
        out = h.traj_clip(mode, in_body_pose=pose, trans=trans, orient=orient, eps=eps)
        torch.cuda.synchronize()
        print('bits clip B=%d mode=%d  %s' % (B, mode, sha(*[out[k] for k in sorted(out)])), flush=True)


def main():
    root = bench.ensure_assets()
    h = make_handle(root)
    for B in (1, 8, 40, 41, 64, 512, 1024):      # 40 / 41 straddle SMALL_ROWS / WIN, 512 is the LSTM switch
        for flags in (P.NETS_INFILL, P.NETS_TRAJ, P.NETS_INFILL | P.NETS_TRAJ):
            for co in (0, P.NETS_COSCHEDULE):
                print('bits infer B=%d flags=%d  %s' % (B, flags | co, infer_case(h, B, flags | co)), flush=True)
    side = torch.cuda.Stream()
    print('bits infer under the caller\'s capture B=64 flags=11  %s' % infer_case(h, 64, P.NETS_INFILL | P.NETS_TRAJ | P.NETS_COSCHEDULE, stream=side), flush=True)
    for B in (3, 64):
        window_cases(h, B)
    for B in (3, 32):
        clip_cases(h, B)
    lt = torch.randn(5, T, 11, generator=torch.Generator().manual_seed(7)).to(dev)
    print('bits local_to_global  %s' % sha(*P.local_to_global(lt)), flush=True)
    for B in (1, 3, 41):
        print('bits taped B=%d  %s' % (B, taped_case(h, B)), flush=True)
    os.environ['GLAMR_NETS_FORCE_FP32'] = '1'
    h32 = make_handle(root)
    del os.environ['GLAMR_NETS_FORCE_FP32']
    assert h32.fp32_only
    for B in (8, 64):
        print('bits fp32 infer B=%d flags=11  %s' % (B, infer_case(h32, B, P.NETS_INFILL | P.NETS_TRAJ | P.NETS_COSCHEDULE)), flush=True)
    window_cases(h32, 64)
    print('bits fp32 taped B=41  %s' % taped_case(h32, 41), flush=True)


if __name__ == '__main__':
    main()
