"""Development aid: bit-level fingerprint + time of the optimiser stage kernel, for A/B runs of two builds of the library on one box
(GLAMR_LIB_PATH selects the build).  Prints one sha1 per case over every output array of the stage (parameters, cameras, poses,
projections, losses) -- a change that only moves loads or barriers must keep every fingerprint -- and the launch time of 1 / 1024 scenes.
usage: python tools/stage_bits.py [--time] [--cases a,b,..]"""
import ctypes, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from glamr_amd import _lib
from glamr_amd.global_recon import packing
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth
from oracle.port import build
from oracle import make_golden as mg
from tests.grecon_common import j_local_from_oracle

CASES = {   # name: (cfg, frames, persons, seeds, gap[, options])
    'dyn300': ('glamr_dynamic', 300, 1, (0, 1, 4, 6), True),
    'dyn300_nogap': ('glamr_dynamic', 300, 1, (0, 2), False),
    'dyn120': ('glamr_dynamic', 120, 1, (0, 3), True),
    'static300': ('glamr_static', 300, 1, (0,), True),
    '3dpw120': ('glamr_3dpw', 120, 1, (0,), False),
    'static_multi300': ('glamr_static_multi', 300, 4, (0,), True),
    'dyn_multi90': ('glamr_dynamic_multi', 90, 2, (0,), True),
    # small cases for the instances the seven above never reach (csrc/grecon_launch.hpp); options: iters = iterations per stage, copies = the
    # scenes repeated that often, env = development knobs for the launches, history / traj_grad = the launch records the per-iteration loss
    # history / writes dL/d traj_local_pred and the gradient record (both hashed)
    'wide9': ('glamr_dynamic_multi', 48, 9, (0,), True, dict(iters=5)),                                   # 32-person build, lite arena
    'share257': ('glamr_dynamic', 64, 1, (0,), True, dict(iters=5, copies=257)),                          # per-CU share of the LDS: arena mode 3
    'lite2': ('glamr_dynamic_multi', 120, 2, (0,), True, dict(iters=5, env={'GLAMR_GRECON_LDS_KB_RT': '26'})),      # (26 KB: lite from 100 frames on)
    'history': ('glamr_dynamic', 64, 1, (0, 1), True, dict(iters=5, history=True)),                       # workspace instance
    'traj_grad': ('glamr_dynamic_multi', 64, 2, (0,), True, dict(iters=1, traj_grad=True)),               # grecon_stage_traj_grad_kernel
}


def run_case(L, dev, root, md, name, iters=None):
    cfg_id, T, P, seeds, gap = CASES[name][:5]
    opts = CASES[name][5] if len(CASES[name]) > 5 else {}
    iters = opts.get('iters', iters)
    cfg = get_config(cfg_id)
    ora = build.load_optimizer(root, cfg)
    datas, jls = [], []
    for s in seeds:
        in_dict = synth.make_in_dict(seed=s, num_frames=T, num_persons=P, smpl_model=md, gap=None if gap else (0, 0))
        d = ora.init_data(in_dict, latents=mg.latents_for(in_dict, s))
        datas.append(d); jls.append(j_local_from_oracle(ora.smpl, d))
    packed = packing.PackedScenes(datas * opts.get('copies', 1), jls * opts.get('copies', 1), dev)
    ws = torch.empty(L.glamr_grecon_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=dev)
    h = hashlib.sha1()
    seen_wd = False
    saved = {k: os.environ.get(k) for k in opts.get('env', {})}
    os.environ.update(opts.get('env', {}))
    try:
        for stage, spec in cfg['opt_stage_specs'].items():
            sd = packing.stage_desc(spec, cfg['grecon_model_specs'], seen_wd, niters=iters)
            seen_wd = seen_wd or ('world_dheading' in spec['opt_variables'])
            extra = {}
            if opts.get('history'):
                extra['loss_history'] = torch.zeros((packed.S, int(sd.niters), len(packing.LOSS_IDS)), dtype=torch.float32, device=dev)
            if opts.get('traj_grad'):
                extra['g_traj_local'] = torch.zeros((packed.S * packed.P, packed.T, 11), dtype=torch.float32, device=dev)
            packed.t.update(extra)
            grads = torch.zeros_like(packed.t['params']) if opts.get('traj_grad') else None
            sb = packed.struct()
            _lib.check(L.glamr_grecon_run_stage(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(grads), _lib.ptr(ws), _lib.current_stream()))
            torch.cuda.synchronize()
            for k, v in sorted(packed.fetch().items()) + sorted((k, packed.t.pop(k).cpu().numpy()) for k in extra) + ([('grads', grads.cpu().numpy())] if grads is not None else []):
                h.update(np.ascontiguousarray(np.asarray(v)).tobytes())
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return h.hexdigest()[:16]


def main():
    dev = torch.device('cuda:0')
    root = build.ensure_synthetic_assets('/tmp/glamr_bench_assets')
    md = synth.make_smpl_model()
    L = _lib.lib()
    names = list(CASES)
    for a in sys.argv[1:]:
        if a.startswith('--cases='):
            names = a.split('=', 1)[1].split(',')
    for n in names:
        print('bits %-16s %s' % (n, run_case(L, dev, root, md, n)), flush=True)
    if '--time' in sys.argv:
        cfg = get_config('glamr_dynamic')
        ora = build.load_optimizer(root, cfg)
        in_dict = synth.make_in_dict(seed=0, num_frames=300, num_persons=1, smpl_model=md)
        d = ora.init_data(in_dict, latents=mg.latents_for(in_dict, 0))
        jl = j_local_from_oracle(ora.smpl, d)
        spec = cfg['opt_stage_specs']['init_opt']
        for S in (1, 1024):
            packed = packing.PackedScenes([d] * S, [jl] * S, dev)
            sd = packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=200)
            sb = packed.struct()
            ws = torch.empty(L.glamr_grecon_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=dev)
            best = 1e9
            for rep in range(4):
                torch.cuda.synchronize(); t0 = time.time()
                _lib.check(L.glamr_grecon_run_stage(ctypes.byref(sb), ctypes.byref(sd), None, _lib.ptr(ws), _lib.current_stream()))
                torch.cuda.synchronize(); best = min(best, time.time() - t0)
            print('time scenes=%4d  %.3f ms  %.2f us/iter' % (S, best * 1e3, best * 1e6 / 200), flush=True)


if __name__ == '__main__':
    main()
