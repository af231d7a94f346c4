"""Time of one stage launch on case a's shape (glamr_dynamic, 120 frames, 1 person, 50 iterations; tests/heading_vec_common.py) from the kernel's
own clock (glamr_grecon_last_launch_ns), smallest of three launches after a first: plain (ext == NULL) / an extension with nothing in it /
vector headings / vector headings + world_dxy + world_res + both of their terms.  MI355X.  `python tools/heading_vec_time.py [scenes]`.
Figures are recorded in DESIGN.md 23, not asserted."""
import ctypes
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from glamr_amd import _lib                                   # noqa: E402
from glamr_amd.global_recon import packing, stepwise         # noqa: E402
from glamr_amd.global_recon.configs import get_config        # noqa: E402
from oracle.port import build                                # noqa: E402
from tests import heading_vec_common as hv                   # noqa: E402

K = 50
WORLD_ALL = dict(variables=['world_dxy', 'world_res'], terms={'traj_rot_res': dict(weight=1.0e2, monitor_only=False), 'traj_trans_res': dict(weight=1.0e2, monitor_only=False)})


def launch_ms(ws):
    ns = ctypes.c_double()
    _lib.check(_lib.lib().glamr_grecon_last_launch_ns(_lib.ptr(ws), ctypes.byref(ns)))
    return ns.value * 1e-6


def main(scenes):
    root = build.ensure_synthetic_assets(os.path.join(tempfile.gettempdir(), 'glamr_smoke_assets'))
    dev = torch.device('cuda:0')
    state = {twin: hv.prepared(root, 'a', twin) for twin in (True, False)}
    for name, vec, world in (('plain', False, None), ('empty ext', False, {}), ('vec', True, None), ('vec + world residuals', True, WORLD_ALL)):
        cfg, specs, data, jl = state[not vec]
        full = get_config('glamr_dynamic')['opt_stage_specs']['init_opt']      # (the shipped stage, camera included: what section 22 timed)
        spec, heading = packing.split_heading_vec(full) if vec else (full, None)
        if world:
            spec = dict(spec, opt_variables=[v for v in spec['opt_variables'] if v != 'world_dheading'])      # (beside it the orientation residual is inert)
        best = None
        for it in range(4):
            packed = packing.PackedScenes([data] * scenes, [jl] * scenes, dev, [tuple(x) for x in specs['cam_fix_frames']], heading_vec=vec)
            sd = packing.stage_desc(spec, specs, False, niters=K)
            ext = None
            if vec or world is not None:
                ext, keep = packing.world_ext(world, packed, niters=K, heading=heading)
            stepwise.run_stage(packed, sd, False, ext=ext)
            ms = launch_ms(packed.last_ws)
            if it > 0:
                best = ms if best is None else min(best, ms)
        print('%-24s %d scene(s): %.3f ms, %.1f us per iteration of the launch' % (name, scenes, best, best * 1e3 / K))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
