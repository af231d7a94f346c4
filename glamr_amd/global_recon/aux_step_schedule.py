"""The six terms of packing.AUX_LOSS_IDS without host Python in the iteration (grecon_model_specs.flag_aux_on_device): per Adam
iteration the gradient launch (glamr_grecon_run_stage, one iteration with lr 0 and grads_out) and ONE launch of glamr_grecon_aux_step, which
evaluates the stage's terms, takes their adjoints on trans_world / cam_pose back to the variables and makes torch.optim.Adam's step.  The
same arithmetic as extra_loss_schedule.ExtraLossSchedule with AuxTerms alone, function by function; nothing is read back and nothing is
allocated outside torch's pool, so the schedule runs under a stream capture (capture_resident) and in optimize_stream's pipeline.  The values
stay on the device with the batch (packed.aux_values[stage]: (S, n, 6)); GlobalReconOptimizer.collect publishes aux_loss_history from them.
A caller's extra_loss and the penetration term need torch autograd on the host: with either, the optimiser ignores the flag."""
import ctypes

import torch

from .. import _lib
from . import extra_loss_schedule, packing, stepwise


def publish(aux_cfg, aux_values):
    """packed.aux_values -> aux_loss_history in ExtraLossSchedule's shape: {stage: {name: (S, n) unweighted values}} (numpy; waits for the device)."""
    out = {}
    for stage, values in aux_values.items():
        h = values.cpu().numpy()
        out[stage] = {name: h[:, :, i] for name, i in packing.AUX_LOSS_IDS.items() if name in aux_cfg[stage]}
    return out


class AuxStepSchedule:
    """run_schedule with the stages' terms of packing.AUX_LOSS_IDS added to their totals, two launches per iteration (and the zero fill of the
    gradient array: the stage kernel stores only the entries of the stage's variables)."""

    def __init__(self, opt, packed):
        self.opt, self.packed = opt, packed

    def run(self, max_iters=None, has_wd=False):
        opt, packed, L = self.opt, self.packed, _lib.lib()
        cfg = opt._aux_cfg
        if not cfg:
            raise ValueError('AuxStepSchedule needs a term of packing.AUX_LOSS_IDS in loss_cfg')
        extra_loss_schedule.check_not_sharded(packed, extra_loss_schedule.aux_what({n for c in cfg.values() for n in c}))
        S, P, T, params = packed.S, packed.P, packed.T, packed.t['params']
        pa = packed.person_arrays      # (root_trans_cam as AuxTerms finds it)
        root_trans_cam = pa['trans_cam'] if pa is not None and pa.get('trans_cam') is not None else packed.root_trans_cam
        if root_trans_cam is None and any('cam_traj_trans' in c for c in cfg.values()):
            raise RuntimeError('cam_traj_trans needs root_trans_cam of every person (person_data[...][\'root_trans_cam\'])')
        ws = torch.empty(max(L.glamr_grecon_aux_step_workspace_bytes(S, P, T), 4), dtype=torch.uint8, device=packed.device)
        stage_ws = torch.empty(L.glamr_grecon_workspace_bytes(S, P, T), dtype=torch.uint8, device=packed.device)
        packed.aux_values = {}
        for stage, spec in opt.opt_stage_specs.items():
            n = stepwise.stage_iters(spec, max_iters)
            ad = packing.aux_desc(cfg.get(stage, {}))      # (a stage that lists none of the names: the step alone)
            m, v = torch.zeros_like(params), torch.zeros_like(params)
            values = torch.zeros((S, max(n, 1), _lib.AUX_NUM_TERMS), dtype=torch.float32, device=packed.device)
            for it in range(n):
                sd = stepwise.grad_launch_desc(spec, opt.specs, has_wd, first=(it == 0))
                grads = stepwise.run_stage(packed, sd, True, ws=stage_ws)
                # the stage kernel applies the world heading offset as soon as the stage optimises it (the variable exists from then on, :459-465)
                if 'world_dheading' in spec['opt_variables']:
                    sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
                sb = packed.struct()
                _lib.check(L.glamr_grecon_aux_step(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), _lib.ptr(root_trans_cam), _lib.ptr(values),
                                                   values.shape[1] * _lib.AUX_NUM_TERMS, it, _lib.ptr(grads), _lib.ptr(m), _lib.ptr(v), float(spec['opt_lr']), it + 1,
                                                   _lib.ptr(ws), _lib.current_stream()))
            if stage in cfg:
                packed.aux_values[stage] = values[:, :n]
            has_wd = stepwise.end_stage(packed, spec, has_wd)
        packed.has_world_dheading = has_wd
        packed.stage_ws = []
        return packed
