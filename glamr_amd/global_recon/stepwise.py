"""What the launch-by-launch schedules share (latent_schedule.LatentSchedule, extra_loss_schedule.ExtraLossSchedule,
parallel.PersonShardedSchedule; stage_iters / end_stage / run_stage also GlobalReconOptimizer.run_schedule): a stage's iteration count and
epilogue, the gradient launch's descriptor, the stage launch itself (run_stage), torch.optim.Adam's step with its step number from the host
(adam_step) or on the device (IndexedAdam), and the capture of one iteration as a HIP graph."""
import ctypes

import numpy as np
import torch

from .. import _lib
from . import packing


def stage_iters(spec, max_iters):
    """Iterations of a stage: `max_iters` caps the configured count (tests); None = the configured schedule."""
    return spec['opt_niters'] if max_iters is None else min(max_iters, spec['opt_niters'])


def end_stage(packed, spec, has_wd):
    """After a stage's last iteration: reinitialize_cam (the first frame's camera for every frame); returns `has_wd` for the stages that
    follow -- the world heading offset is applied whenever the variable exists (:459-465), from the first stage that optimises it on."""
    if spec.get('reinitialize_cam', False):
        packed.t['cam_pose'][:] = packed.t['cam_pose'][:, :1]
    return has_wd or 'world_dheading' in spec['opt_variables']


def grad_launch_desc(spec, model_specs, has_wd, first, extra_flags=0):
    """The stage descriptor of a GRADIENT launch: one iteration with lr 0 (the caller makes the update from grads_out).  Only a stage's
    `first` launch sets the camera parameters from cam_pose; every later one keeps what the optimiser made of them."""
    sd = packing.stage_desc(spec, model_specs, has_wd, niters=1)
    sd.lr = 0.0
    sd.flags |= (0 if first else packing.FLAG_KEEP_CAM_PARAMS) | extra_flags
    return sd


def world_stage(packed, world):
    """What a stage's launch takes of the world-frame residuals: `world` (packing.split_world's second result for the stage, or None) when the
    stage lists one of their names, {} when it only carries an existing world_dxy along (:467-468 adds it in every later stage), None when the
    plain launch serves the stage."""
    return world if world is not None else ({} if packed.has_world_dxy else None)


def end_world_stage(packed, world, keep):
    """After a stage that ran with the extension: `world_dxy` exists from the first stage that lists it on (get_parameter :628-631), the residual
    tensors are reported once a stage listed world_res or one of the terms, and the two terms' last values stay with the batch."""
    if world:
        packed.has_world_dxy = packed.has_world_dxy or 'world_dxy' in world['variables']
        packed.world_res_listed = packed.world_res_listed or 'world_res' in world['variables'] or bool(world['terms'])
    packed.world_losses = keep['losses']


def run_stage(packed, sd, want_grads, ws=None, ext=None):
    """glamr_grecon_run_stage on the packed batch (current stream); returns the gradient record (n_scenes, scene_stride) or None.  `ws`: a
    workspace the caller keeps across launches (GLAMR_FLAG_KEEP_TABLES needs the previous launch's); a fresh one otherwise (packed.last_ws).
    `ext`: a glamr_stage_ext (packing.world_ext) -- the launch then is glamr_grecon_run_stage_ext's."""
    L = _lib.lib()
    sb = packed.struct()
    grads = torch.zeros_like(packed.t['params']) if want_grads else None
    if ws is None:
        ws = torch.empty(L.glamr_grecon_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=packed.device)
    if ext is None:
        _lib.check(L.glamr_grecon_run_stage(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(grads), _lib.ptr(ws), _lib.current_stream()))
    else:
        _lib.check(L.glamr_grecon_run_stage_ext(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ext), _lib.ptr(grads), _lib.ptr(ws), _lib.current_stream()))
    packed.last_ws = ws
    return grads


def adam_step(p, m, v, g, lr, step):
    """glamr_adam_step: p, m, v <- one Adam step with gradient g, the 1-based step number given by the host (current stream)."""
    _lib.check(_lib.lib().glamr_adam_step(p.numel(), _lib.ptr(p), _lib.ptr(m), _lib.ptr(v), _lib.ptr(g), float(lr), int(step), _lib.current_stream()))


class IndexedAdam:
    """torch.optim.Adam's arithmetic for the `n` iterations of a stage with the step NUMBER on the device, so that a captured iteration steps
    on at every replay: the host-made coefficient table (glamr_adam_coef_table) and one int32 counter per `slot` -- the 0-based row of the
    table a parameter group is at (a group's count advances only when it is stepped, as a parameter's whose grad is None does not)."""

    def __init__(self, lr, n, device, slots=1):
        n = max(int(n), 1)
        tab = np.empty((n, 2), np.float32)
        _lib.check(_lib.lib().glamr_adam_coef_table(float(lr), n, _lib.ptr(tab)))
        self.coef = torch.from_numpy(tab).to(device)
        self.counters = torch.empty(slots, dtype=torch.int32, device=device)
        self.reset()

    def reset(self):
        self.counters.zero_()

    def step(self, x, m, v, g, slot=0):
        """x, m, v <- one Adam step with gradient g at the slot's row of the table; the slot's counter + 1 (current stream)."""
        L, idx, st = _lib.lib(), _lib.ptr(self.counters[slot:]), _lib.current_stream()
        _lib.check(L.glamr_adam_step_indexed(x.numel(), _lib.ptr(x), _lib.ptr(m), _lib.ptr(v), _lib.ptr(g), _lib.ptr(self.coef), idx, st))
        _lib.check(L.glamr_counter_add(idx, 1, st))


def capture_iteration(fn, device, side_stream, capture_error_mode=None):
    """The launches of fn() as a HIP graph: captured on `side_stream`, which joins the current stream before and is joined by it after.
    Nothing runs; the caller replays the graph.  Whatever the capture raises is the caller's to handle."""
    graph = torch.cuda.CUDAGraph()
    cur = torch.cuda.current_stream(device)
    side_stream.wait_stream(cur)
    with torch.cuda.graph(graph, stream=side_stream, **({} if capture_error_mode is None else {'capture_error_mode': capture_error_mode})):
        fn()
    cur.wait_stream(side_stream)
    return graph
