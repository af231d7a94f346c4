"""The staged optimisation in LATENT-OPTIMISATION mode (flag_opt_motion_latent / flag_opt_traj_latent; global_recon_model.py:155-158,434-437,
619-622 of the reference).  Every iteration from `opt_latent_start_iter` on re-runs infer_motion_traj with the current latents (:352-392): the
infiller's output becomes `smpl_pose`, the trajectory predictor's local trajectory the new `traj_local_pred`, and SMPL gives new joints; the
loss reaches `motion_latent` through the reprojection term -> joints -> SMPL (body pose) -> infiller (all windows, autoregressively).
Detached (the default), `traj_latent` is in the parameter list but never receives a data gradient: get_pred_trajectory_base detaches
traj_local_pred (:396), and torch.optim.Adam skips a parameter whose grad is None -- its value stays, exactly as in the reference; with
flag_attach_traj_pred it gets one through the taped predictor, and a latent regulariser is a gradient of its own.
The first two iterations of a stage are plain launches; the third is CAPTURED as a HIP graph and the rest of the stage replays it
(GLAMR_LATENT_GRAPH=0: plain launches throughout; model.latent_graph_replays counts)."""
import collections
import os
import sys

import numpy as np
import torch

from .. import _lib
from ..models.priors import num_windows
from . import packing, stepwise

# The latent gradients of ONE iteration (None = the latent has none): the data gradients that came back through the priors, and -- in a stage
# with a latent regulariser -- what each latent was stepped by (data gradient + regulariser, or the regulariser alone).
LatentGrads = collections.namedtuple('LatentGrads', 'g_motion g_traj g_motion_total g_traj_total', defaults=(None, None))
# What is fixed for the iterations of a stage: the spec its launches get, whether the scenes carry a world heading offset, the latent regularisers
# [(weight, mode)] * 2 or None, their history (n_scenes, n_iterations, 2) or None, the optimiser (slots: 0 scene parameters, 1 motion latents, 2 trajectory latents).
_Stage = collections.namedtuple('_Stage', 'spec has_wd regs hist adam')


def frame_row_index(lens, fr_start, occupied, T):
    """Frame rows of the priors' outputs (row e of slot k = video frame fr_start[k] + e) <-> the per-slot video-frame arrays of T frames: ONE
    gather / scatter index pair (src, dst; int64) for the whole batch.  Person slots a scene with fewer persons leaves empty have no rows."""
    n = np.where(np.asarray(occupied).reshape(-1), np.asarray(lens).reshape(-1), 0).astype(np.int64)
    first = np.cumsum(n) - n                                             # index of every slot's row 0 in the result
    src = np.repeat(np.arange(len(n)) * T - first, n) + np.arange(n.sum())
    return src, src + np.repeat(np.asarray(fr_start, np.int64).reshape(-1), n)


class LatentSchedule:
    """One run of the schedule on an initialised batch.  The attributes set in __init__ are ALL that lives longer than an iteration: the
    launches of an iteration read and write them at fixed addresses (which is what lets one captured iteration be replayed)."""

    def __init__(self, model, rin, packed):
        L = _lib.lib()
        self.model, self.packed, dev = model, packed, model.device
        T = self.T = packed.T
        n_slots = self.n_slots = packed.S * packed.P
        self.meps, self.teps = (x.clone() for x in packed.latents)
        self.pa = packed.person_arrays
        h = self.nets = model.mt_model.handle
        self.attach = model.flag_attach_traj_pred
        tape_gb = (L.glamr_nets_tape_bytes(h.h, n_slots, T) + (L.glamr_nets_traj_tape_bytes(h.h, n_slots, T) if self.attach else 0)) / 2.0 ** 30
        if tape_gb > 96:
            raise ValueError('latent-optimisation mode keeps every activation of the infiller (and of the attached trajectory predictor) for its backward: %.0f GB for %d person slots of %d frames; '
                             'run it on smaller batches (the reference runs it on one sequence at a time)' % (tape_gb, n_slots, T))
        lens = self.lens = np.ascontiguousarray(rin.lens, dtype=np.int32)
        # (the predictor takes lengths >= 1: an empty slot runs as one frame whose gradient rows are zero)
        self.lens_t = np.maximum(lens, 1).astype(np.int32)
        occupied = rin.seq_len_slot.cpu().numpy() > 0                    # (person slots a scene with fewer persons leaves empty are skipped)
        self.src, self.dst = (torch.as_tensor(x, device=dev) for x in frame_row_index(lens, packed.t['fr_start'].cpu().numpy(), occupied, T))
        self.smpl_h = model.smpl._handle(dev)
        self.zeros3 = torch.zeros((n_slots * T, 3), device=dev)
        self.g_j_local = packed.t['g_j_local'] = torch.zeros((n_slots, T, packing.NJ, 3), device=dev)
        # dL/d traj_local_pred of the gradient launch, rows in the priors' own order (traj_local_pred is stored by existing-frame row)
        self.g_traj_local = torch.zeros((n_slots, T, 11), device=dev) if self.attach else None
        # init_opt creates a fresh optimiser per stage (:635-644): the moments of the three parameter groups are zeroed at every stage's start
        self.params = packed.t['params']
        self.m_motion, self.v_motion = torch.zeros_like(self.meps), torch.zeros_like(self.meps)
        self.m_traj, self.v_traj = torch.zeros_like(self.teps), torch.zeros_like(self.teps)      # (stepped in attached mode or by a regulariser)
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        # the latent regularisers (glamr_latent_reg): per-slot window counts (0 = an empty slot) on the host for the argument checks
        # and on the device for the kernel, the gradient arrays of a latent that has no data gradient in an iteration, the values of the last launch
        self.n_win_host = np.ascontiguousarray([num_windows(int(lens[k])) if occupied[k] else 0 for k in range(n_slots)], dtype=np.int32)
        self.n_win_dev = torch.as_tensor(self.n_win_host, device=dev)
        self.g_reg_m, self.g_reg_t = torch.zeros_like(self.meps), torch.zeros_like(self.teps)
        self.reg_values = torch.zeros((packed.S, 2), device=dev)

    def iteration(self, st, with_priors, first):
        """One Adam iteration (:547-570 in latent mode), launches only -- nothing here reads a value back or depends on the iteration number
        except through the optimiser's counters on the device, so the same launch sequence is captured ONCE per stage and replayed."""
        pose_out, tape, ttape = self._forward_priors() if with_priors else (None, None, None)
        grads = self._gradient_launch(st, first, with_traj_grad=ttape is not None)
        g = self._backward_to_latents(st, pose_out, tape, ttape)
        if st.regs is not None:
            g = self._regularise_and_step(st, g)
        st.adam.step(self.params, self.m, self.v, grads)
        return g

    def _forward_priors(self):
        """infer_motion_traj with the current latents (:352-392): taped infiller, trajectory predictor, their rows into `smpl_pose` and
        `traj_local_pred`, joints-only skinning into `j_local`.  Returns (the infiller's pose, its tape, the predictor's tape or None)."""
        h, pa, t, n_slots, T = self.nets, self.pa, self.packed.t, self.n_slots, self.T
        ttape = None
        pose_out, tape = h.infill_taped(pa['nets_pose'], pa['nets_vis'], self.lens, self.meps)
        if self.attach:      # the same predictor with its activations kept (the rows are bit-identical)
            local_traj, ttape = h.traj_taped(self.lens_t, self.teps, in_body_pose=pose_out)
        else:
            local_traj = h.infer(pose_out, None, self.lens, traj_eps=self.teps, infill=False, traj=True)['local_traj']
        pa['smpl_pose'].view(-1, 69).index_copy_(0, self.dst, pose_out.view(-1, 69).index_select(0, self.src))
        t['traj_local_pred'].view(-1, 11).index_copy_(0, self.src, local_traj.view(-1, 11).index_select(0, self.src))
        with torch.no_grad():
            jl = self.model.smpl(global_orient=self.zeros3, body_pose=pa['smpl_pose'].view(-1, 69), betas=pa['smpl_beta'].view(-1, 10), root_trans=self.zeros3,
                                 return_verts=False).joints
        if t['j_local'].shape == (n_slots, T, packing.NJ, 3):
            t['j_local'].copy_(jl.view(n_slots, T, packing.NJ, 3))          # (a fixed address: the gradient launch is captured with it)
        else:
            t['j_local'] = jl.view(n_slots, T, packing.NJ, 3).clone()
        return pose_out, tape, ttape

    def _gradient_launch(self, st, first, with_traj_grad):
        """The stage kernel's gradient launch: dL/d scene parameters (returned), dL/d j_local and -- only when the launch has a reader for it,
        the taped predictor (before opt_latent_start_iter the usual instance runs) -- dL/d traj_local_pred."""
        self.packed.t['g_traj_local'] = self.g_traj_local if with_traj_grad else None
        return stepwise.run_stage(self.packed, stepwise.grad_launch_desc(st.spec, self.model.specs, st.has_wd, first), True)

    def _backward_to_latents(self, st, pose_out, tape, ttape):
        """The gradient launch's adjoints back through the priors that ran; in a stage without a latent regulariser each latent is stepped as
        soon as its gradient exists.  Returns LatentGrads (data gradients only)."""
        L, h, pa, model, n_rows = _lib.lib(), self.nets, self.pa, self.model, self.n_slots * self.T
        g_motion = g_traj = g_bp = None
        if ttape is not None:
            # dL/d traj_local_pred -> trajectory latent, and -> joint rows -> body pose (the FK step in reverse) for the motion latent
            g_traj, g_joints = h.traj_backward(ttape, self.g_traj_local, want_joints=model.flag_opt_motion_latent)
            if g_joints is not None:
                g_bp = h.fk_backward(pose_out, self.lens_t, g_joints)
            if model.flag_opt_traj_latent and st.regs is None:
                st.adam.step(self.teps, self.m_traj, self.v_traj, g_traj, slot=2)
        if tape is not None and model.flag_opt_motion_latent:
            # dL/d j_local -> body pose (skinning, blend shapes, chain, re-anchoring in reverse) -> latents (all windows)
            pose72 = torch.cat([self.zeros3, pa['smpl_pose'].view(-1, 69)], dim=1).contiguous()
            g_pose = torch.empty((n_rows, 72), device=model.device)
            ws = torch.empty(L.glamr_smpl_backward_workspace_bytes(self.smpl_h, n_rows, 0), dtype=torch.uint8, device=model.device)
            _lib.check(L.glamr_smpl_backward(self.smpl_h, n_rows, _lib.ptr(pose72), _lib.ptr(pa['smpl_beta'].view(-1, 10)), _lib.ptr(self.zeros3), None, None, None,
                                             None, _lib.ptr(self.g_j_local), _lib.ptr(g_pose), None, None, None, 0, _lib.ptr(ws), _lib.current_stream()))
            g_out = torch.zeros((n_rows, 69), device=model.device)
            g_out.index_copy_(0, self.src, g_pose[:, 3:].index_select(0, self.dst))
            if g_bp is not None:
                g_out += g_bp.view(-1, 69)
            g_motion = h.infill_backward(tape, g_out.view(self.n_slots, self.T, 69))
            if st.regs is None:
                st.adam.step(self.meps, self.m_motion, self.v_motion, g_motion, slot=1)
        return LatentGrads(g_motion, g_traj)

    def _regularise_and_step(self, st, g):
        """A stage with a latent regulariser (compute_loss :533-545 evaluates it in EVERY iteration, also before opt_latent_start_iter): one launch
        for both latents, at the latents this iteration started from.  A latent that has a data gradient gets the regulariser's ADDED to it, one
        that has none gets it STORED -- and is stepped by it alone (traj_latent in detached mode; both latents before opt_latent_start_iter, when
        the priors are not re-run).  One Adam step per latent that has any gradient; returns LatentGrads with what each was stepped by."""
        (w_m, mode_m), (w_t, mode_t) = st.regs
        g_t_data = g.g_traj if self.model.flag_opt_traj_latent else None
        g_m = g.g_motion if g.g_motion is not None else self.g_reg_m
        g_t = g_t_data if g_t_data is not None else self.g_reg_t
        _lib.check(_lib.lib().glamr_latent_reg(self.packed.S, self.packed.P, self.meps.shape[1], _lib.ptr(self.meps), _lib.ptr(self.teps), _lib.ptr(self.n_win_dev),
                                               _lib.ptr(self.n_win_host), w_m, w_t, mode_m, mode_t, int(g.g_motion is not None), int(g_t_data is not None), _lib.ptr(g_m),
                                               _lib.ptr(g_t), _lib.ptr(self.reg_values), _lib.ptr(st.hist), st.hist.shape[1], _lib.ptr(st.adam.counters),
                                               _lib.current_stream()))
        step_t = g_t_data is not None or mode_t == _lib.LATENT_REG_ACTIVE
        step_m = g.g_motion is not None or mode_m == _lib.LATENT_REG_ACTIVE
        if step_t:
            st.adam.step(self.teps, self.m_traj, self.v_traj, g_t, slot=2)
        if step_m:
            st.adam.step(self.meps, self.m_motion, self.v_motion, g_m, slot=1)
        return g._replace(g_motion_total=g_m if step_m else None, g_traj_total=g_t if step_t else None)

    def _record_trace(self, st, g, with_priors):
        """model.latent_trace (a dict the parity tests set): the two values of the run's first regularised iteration, and the state and the
        latent gradients of the first iteration of the run in which a gradient came back through the priors."""
        trace, t = self.model.latent_trace, self.packed.t
        if trace is None:
            return
        host = lambda x: x.detach().cpu().numpy()
        if st.regs is not None and 'latent_reg' not in trace:
            trace['latent_reg'] = host(self.reg_values)
        if (g.g_motion is not None or (with_priors and (self.attach or st.regs is not None))) and 'losses' not in trace:
            trace.update(losses=host(t['losses']), smpl_pose=host(self.pa['smpl_pose']), traj_local_pred=host(t['traj_local_pred']))
            if g.g_motion is not None:
                trace['g_motion_latent'] = host(g.g_motion)
            if self.attach:
                trace.update(g_traj_latent=host(g.g_traj), g_traj_local=host(self.g_traj_local))
            elif g.g_traj_total is not None:                              # detached mode: the regulariser is traj_latent's whole gradient
                trace['g_traj_latent'] = host(g.g_traj_total)

    def run(self, max_iters=None):
        """The stage loop: fresh moments and a fresh optimiser per stage; plain iterations until the launch sequence repeats (the second
        iteration with priors at the earliest), then replays of that iteration captured once."""
        model, packed, dev = self.model, self.packed, self.model.device
        model.latent_loss_history = {}
        model.latent_graph_replays = 0
        use_graph = os.environ.get('GLAMR_LATENT_GRAPH', '1') != '0'
        has_wd = False
        for stage, spec in model.opt_stage_specs.items():
            n = stepwise.stage_iters(spec, max_iters)
            start = spec.get('opt_latent_start_iter', 0)                 # optimize() :581
            for x in (self.m, self.v, self.m_motion, self.v_motion, self.m_traj, self.v_traj):
                x.zero_()
            # the latent regularisers are this loop's, not the stage kernel's: the launch gets the loss_cfg without them
            rest_cfg, regs = packing.split_latent_regs(spec['loss_cfg'])
            hist = None
            if any(mode != _lib.LATENT_REG_ABSENT for _, mode in regs):
                spec = dict(spec, loss_cfg=rest_cfg)
                hist = torch.zeros((packed.S, max(n, 1), 2), device=dev)
            else:
                regs = None                                              # (no regulariser: no launch of it, the latents are stepped as their gradients arrive)
            st = _Stage(spec, has_wd, regs, hist, stepwise.IndexedAdam(spec['opt_lr'], n, dev, slots=3))
            graph = None
            for it in range(n):
                if graph is not None:
                    graph.replay()
                    model.latent_graph_replays += 1
                    continue
                with_priors = it >= start
                self._record_trace(st, self.iteration(st, with_priors, it == 0), with_priors)
                # from here on every iteration of the stage is the same launch sequence: capture it once, replay it n - it - 2 times
                if use_graph and with_priors and it >= 1 and n - it - 1 >= 2 and not torch.cuda.is_current_stream_capturing():
                    try:
                        if model._latent_capture_stream is None:
                            model._latent_capture_stream = torch.cuda.Stream(device=dev)
                        graph = stepwise.capture_iteration(lambda: self.iteration(st, True, False), dev, model._latent_capture_stream)
                    except Exception as e:      # noqa: BLE001 -- the plain launches are always available
                        sys.stderr.write('latent-optimisation mode: iteration graph not used (%s); plain launches\n' % e)
                        torch.cuda.synchronize(dev)
                        graph, use_graph = None, False
            has_wd = stepwise.end_stage(packed, spec, has_wd)
            del graph
            if hist is not None:
                self._report_latent_stage(stage, st, hist[:, :n])
        packed.has_world_dheading = has_wd
        packed.stage_ws = []
        packed.latents = (self.meps, self.teps)
        packed.t['g_j_local'] = None
        packed.t['g_traj_local'] = None
        return packed

    def _report_latent_stage(self, stage, st, hist):
        """latent_loss_history[stage] and, with a `log`, write_logs' line (:646-659) per iteration for the stage's latent regularisers under the
        reference's names (the unweighted values, loss_uw_dict :564).  The latent-optimisation schedule records no other term per iteration."""
        model, packed = self.model, self.packed
        h = hist.cpu().numpy()                                          # (waits for the stage)
        model.latent_loss_history[stage] = h
        if model.log is None:
            return
        names = [(t, n) for t, n in enumerate(packing.LATENT_REG_TERMS) if st.regs[t][1] != _lib.LATENT_REG_ABSENT]
        for si in range(packed.S):
            for it in range(h.shape[1]):
                loss_str = ' | '.join('%s: %7.3f' % (n, h[si, it, t]) for t, n in names)
                model.log.info('%s - %s - %s | %4d/%d | LR: %.0e | %s' % (model.cfg_id, packed.seq_names[si], stage, it, h.shape[1], st.spec['opt_lr'], loss_str))
