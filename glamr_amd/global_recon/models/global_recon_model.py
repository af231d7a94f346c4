"""GlobalReconOptimizer on MI355X -- drop-in for global_recon/models/global_recon_model.py:23-659.

    model = GlobalReconOptimizer(cfg, device, log)        # cfg: reference-style Config object or the dict of configs.get_config()
    out = model.optimize(in_dict)                         # same input/output dictionaries as the reference (:572-589)
    outs = model.optimize_batch([in_dict, ...])           # extension: many independent sequences in one pass

Division of labour:
  * host (this file, numpy): the HybrIK wire format -> per-person arrays with the reference's frame/visibility bookkeeping
    (:88-148, bit-exact indices), scipy interpolation over gaps, `filter_pose` (a sequential data-dependent loop, :250-271), and
    the one-off camera / heading initialisation (:166-183, :273-317).
  * device (HIP kernels behind libglamr_hip.so): motion infilling + trajectory prediction for ALL persons of ALL sequences in one
    batched call, SMPL skinning for the cached root-relative joints, and every optimisation stage as ONE kernel launch that runs all
    Adam iterations of all scenes (glamr_grecon_run_stage).
There is no CPU path for the device part: a missing library or a non-HIP device raises.
"""
import contextlib
import ctypes
import os
import time

import numpy as np
import torch

from ... import _lib
from ...lib.models.sdf import SDFLoss
from ...lib.models.smpl import SMPL, SMPL_MODEL_DIR
from ...lib.utils import np_transform as nt
from ...models import latent_rng
from ...models.prior_models import MotionTrajJointModel
from ...models.priors import num_windows, NZ
from .. import aux_step_schedule, extra_loss_schedule, packing, stepwise
from ..configs import get_config

# (body26fk index, smpl index) pairs with identical joint names (lib/utils/joints.py:48-73,619-641 through :82-85): the 14
# keypoints of HybrIK's 24 SMPL joints that GLAMR trusts; the other 12 body26fk joints keep score 0.
SMPL_TO_BODY26FK = np.array([[8, 8], [5, 5], [2, 2], [21, 17], [23, 19], [25, 21], [7, 7], [4, 4], [1, 1],
                             [20, 16], [22, 18], [24, 20], [6, 12], [0, 0]])


def _cfg_parts(cfg):
    if isinstance(cfg, str):
        cfg = get_config(cfg)
    if isinstance(cfg, dict):
        return cfg['grecon_model_specs'], cfg['opt_stage_specs'], cfg.get('id', 'glamr')
    return cfg.grecon_model_specs, cfg.opt_stage_specs, getattr(cfg, 'id', 'glamr')


_PERSON_KEYS = ('smpl_pose', 'smpl_beta', 'smpl_orient_cam', 'root_trans_cam', 'cam_K', 'traj_local_pred', 'smpl_orient_world_base',
                'root_trans_world_base', 'smpl_orient_world', 'root_trans_world', 'kp_2d_pred', 'smpl_orient_cam_in_world', 'traj_local_xy',
                'traj_local_heading', 'traj_local_dxy', 'traj_local_dheading', 'traj_local_z', 'traj_local_rot', 'visible', 'visible_orig',
                'exist_frames', 'frames', 'vis_frames', 'invis_frames', 'frame2ind', 'kp_2d', 'kp_2d_aligned', 'kp_2d_score', 'person2cam')


class ResidentInputs:
    """A batch of sequences in HBM as stage_inputs() leaves it.
    Geometry: S scenes x P person slots x T frames (the batch maxima); Ts, ids [per scene]: its length and its person ids; lens (S * P,): the length
    of every slot's existing range (11 for an empty slot); exists {(scene, person id): `exist` array}.  Device arrays: g {'exist', 'rot', 'betas',
    'trans', 'kp', 'K'}, the HybrIK arrays by (slot, frame); n_persons, seq_len (S,) and seq_len_slot (S * P,; 0 = an empty slot) int32.
    meps (S * P, windows, NZ), teps (S * P, NZ): the caller's latents or None (init_resident draws).  meta [per scene]: seq_name, seq_len, gt,
    gt_meta; explicit_seq_ids [per scene]: in_dict['seq_id'] or None.  latent_seq_ids, latent_person_ids, latent_seed_word: what the 'philox'
    draw reads (_latent_table), None until a draw under 'philox' needs them.  validate: the value checks are still to run (value_checks clears
    it); verdict (2, S * P) int32 on the device with its event verdict_ready, None before the checks and again after check_inputs; verdict_host
    (pinned copy, event): set by _fetch_async, consumed by check_inputs.  upload_done: the event after the batch's host->device copies."""

    def __init__(self, S, P, T, Ts, ids, lens, exists, g, n_persons, seq_len, seq_len_slot, meta, explicit_seq_ids, validate, meps=None, teps=None):
        self.S, self.P, self.T, self.Ts, self.ids, self.lens, self.exists = S, P, T, Ts, ids, lens, exists
        self.g, self.n_persons, self.seq_len, self.seq_len_slot, self.meps, self.teps = g, n_persons, seq_len, seq_len_slot, meps, teps
        self.meta, self.explicit_seq_ids = meta, explicit_seq_ids
        self.latent_seq_ids = self.latent_person_ids = self.latent_seed_word = None
        self.validate, self.verdict, self.verdict_ready, self.verdict_host = bool(validate), None, None, None
        self.upload_done = None               # (stage_inputs records it once everything above is on its way)

    def raw_batch(self):
        """glamr_raw_batch over the staged arrays."""
        raw, g = _lib.RawBatch(), self.g
        raw.n_slots, raw.max_len = self.S * self.P, self.T
        for name, ten in (('seq_len', self.seq_len_slot), ('exist', g['exist']), ('rotmats', g['rot']), ('betas', g['betas']), ('root_trans', g['trans']), ('kp_2d', g['kp'])):
            setattr(raw, name, ctypes.c_void_p(ten.data_ptr()))
        return raw


class LazyDict(dict):
    """A dictionary some of whose values are produced on first access (and then kept).  optimize_batch returns the reference's per-person
    dictionaries (~40 arrays each); most consumers read a handful of them, so the slices of the batch arrays -- and
    the ones that need a conversion (float64 copies of the masks and keypoints, 4 x 4 expansions, frame tables) -- are cut when somebody
    asks.  Pending values come from per-key thunks (`lazy`) or from one `factory(key)` shared by the keys in `factory_keys`.  Behaves as
    a plain dict otherwise: `in`, iteration, len, items(), pickling and equality see every key."""

    def __init__(self, eager, lazy=(), factory=None, factory_keys=()):
        super().__init__(eager)
        self._lazy = dict(lazy)
        self._factory, self._fkeys, self._gone = factory, factory_keys, None

    def _pending(self, key):
        return key in self._lazy or (key in self._fkeys and not dict.__contains__(self, key) and not (self._gone and key in self._gone))

    def __missing__(self, key):
        if key in self._lazy:
            value = self._lazy.pop(key)()
        elif self._pending(key):
            value = self._factory(key)
        else:
            raise KeyError(key)
        dict.__setitem__(self, key, value)
        return value

    def _force(self):
        for k in list(self._lazy):
            self[k]
        for k in self._fkeys:
            if self._pending(k):
                self[k]
        return self

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __contains__(self, key):
        return dict.__contains__(self, key) or self._pending(key)

    def __iter__(self):
        return iter(self._force().keys())

    def __len__(self):
        return dict.__len__(self) + len(self._lazy) + sum(1 for k in self._fkeys if self._pending(k) and k not in self._lazy)

    def keys(self):
        return dict.keys(self._force())

    def values(self):
        return dict.values(self._force())

    def items(self):
        return dict.items(self._force())

    def __eq__(self, other):
        return dict.__eq__(self._force(), other)

    def __ne__(self, other):
        return not self.__eq__(other)

    def __setitem__(self, key, value):
        self._lazy.pop(key, None)
        dict.__setitem__(self, key, value)

    def __delitem__(self, key):
        self.pop(key)

    def pop(self, key, *default):
        if self._pending(key):
            self[key]
        if key in self._fkeys:
            self._gone = (self._gone or set()) | {key}
        return dict.pop(self, key, *default)

    def copy(self):
        return dict(self._force())

    def __reduce__(self):
        return (dict, (dict(self._force()),))


def coschedule_enabled():
    """GLAMR_COSCHEDULE=0 switches the staggered two-stream pipeline (PipelineGate + GLAMR_NETS_COSCHEDULE kernels) off."""
    return os.environ.get('GLAMR_COSCHEDULE', '1') != '0'


class PipelineGate:
    """Staggers batches that alternate between TWO streams so that a batch's motion infiller runs while the previous batch's optimiser stage
    is resident (GlobalReconOptimizer.pipeline_gate).  A stage workgroup leaves three of a CU's four SIMDs half empty and its matrix pipes
    idle, and the infiller's co-schedulable kernels (GLAMR_NETS_COSCHEDULE, csrc/nn_free.hpp) fit into exactly that space -- but two streams
    left to themselves fall into step (both in their priors, then both stages one after the other) and nothing overlaps.  The rule: a batch
    starts its device work when the PREVIOUS batch's priors have finished, a few milliseconds before that batch's stage starts.  (Measured and
    dropped: opening the gate only when the stage is launched -- the infiller then loses its head start on an almost empty GPU, does not
    finish within the stage's 35 ms, and the step goes from 43.4 to 49.0 ms.)  Measured on
    1024 x 300 frames (tools/pipeline_probe.py): 42.6 ms per batch against 47.1 for the LDS kernels free-running."""

    def __init__(self):
        self.last = None

    def before(self, stream):
        if self.last is not None:
            stream.wait_event(self.last)

    def after(self, stream):
        # (an event created with hipEventReleaseToDevice instead of torch's system-scope one: measured, no difference -- profiles/r05_pipeline_experiments.log)
        ev = torch.cuda.Event()
        ev.record(stream)
        self.last = ev


class ResidentGraph:
    """A captured optimize_resident step (GlobalReconOptimizer.capture_resident): one HIP graph, or -- under a PipelineGate -- two, split
    where the gate's event is recorded (an event shared with another stream's graph cannot live inside a captured graph).  A step captured under
    latent_source 'philox' holds the latent draw but not its seed: every replay() first writes the model's `latent_seed` AS IT IS AT REPLAY TIME
    to the batch's seed word on this stream (`before_replay`), so the seed may change between replays without re-capture."""

    def __init__(self, graph, datas, packed, stream, tail=None, gate=None, head=None):
        self.graph, self.datas, self.packed, self.stream, self.tail, self.gate, self.head = graph, datas, packed, stream, tail, gate, head
        self.before_replay = None                 # set by capture_resident under latent_source 'philox' (see the class docstring)

    def replay(self):
        with torch.cuda.stream(self.stream):
            if self.before_replay is not None:
                self.before_replay()
            if self.head is not None:
                self.head.replay()                                    # what precedes the priors does not wait for the gate (GLAMR_GATE_PREP=early)
            if self.gate is not None:
                self.gate.before(self.stream)
            self.graph.replay()
            if self.tail is not None:
                if self.gate is not None:
                    self.gate.after(self.stream)
                self.tail.replay()
        return self.packed


class GlobalReconOptimizer:
    # optimize_stream's two compute streams, made at its first call.  On the class, not in __init__: bench.py hands over its own two with
    # `model.__dict__.setdefault('_compute_streams', ...)`, which an instance attribute set to None would turn into a no-op.
    _compute_streams = None

    def __init__(self, cfg, device=torch.device('cuda'), log=None, smpl=None, mt_model=None, results_root='results'):
        self.cfg = cfg
        self.specs, self.opt_stage_specs, self.cfg_id = _cfg_parts(cfg)
        self.device = torch.device(device)
        self.log = log
        if self.device.type != 'cuda':
            raise RuntimeError('glamr_amd.GlobalReconOptimizer runs on an MI355X (device %r given); there is no CPU fallback' % (device,))
        _lib.lib()                                                     # fail early and loudly if the HIP library is missing
        self.pipeline_gate = None                                      # a PipelineGate when the caller alternates batches between two streams
        # Where the priors' Gaussian latents come from when the caller gives none.  'torch': torch.randn on the global generator, the reference's
        # source -- a person's draw then depends on its slot in the batch.  'philox': the library's counter-based streams (csrc/rng.hip,
        # DESIGN.md 10): a function of (latent_seed, sequence id, person id, prior, element) alone, whatever batch, shard or padding.
        self._latent_source = 'torch'
        self.latent_seed = 0
        self._capture_split = None
        self._capture_head_split = None
        # kept between calls, made at first use: the pinned staging sets (_staging), optimize_stream's copy stream, run_latent_schedule's capture stream
        self._pinned = {'sets': [None, None], 'turn': 0}
        self._download_stream = self._latent_capture_stream = None
        self.kernel_ms = None                 # a list: collect() appends the duration of every stage launch of the batches it collects
        self.last_losses = None               # (scenes, GLAMR_NUM_LOSSES): the loss values of the last batch collected
        self.latent_graph_replays = 0         # run_latent_schedule: iterations of its last run that were graph replays
        self.latent_trace = None              # a dict: run_latent_schedule records its first iteration with priors there (the parity tests)
        # Per-iteration loss log (:564,646-659).  The reference calls write_logs after EVERY optimizer.step -- with `log` None it prints.  Here
        # the iterations of a stage are one kernel launch: with a `log` (or keep_loss_history = True) the launch records the unweighted value of
        # every term at every iteration (glamr_scene_batch.loss_history; the plain instance with the reporting evaluation, about 2x the time),
        # run_schedule hands them to `log.info` in the reference's line format once the stage is done, and `loss_history[stage]` keeps the
        # (scenes, iterations, GLAMR_NUM_LOSSES) array.  Without a log nothing is recorded and nothing is printed: a batch of 1024 sequences
        # would be half a million lines.
        self.keep_loss_history = False
        self.loss_history = {}
        # extra_loss: a caller-defined term on the world poses, `extra_loss(ctx) -> (S,) tensor`, added to every stage's total.
        # None (the default): nothing changes.  Set: optimize / optimize_batch run extra_loss_schedule.ExtraLossSchedule in place of
        # run_schedule; extra_loss_history[stage] keeps the term's (scenes, iterations) values.
        self._extra_loss = None
        self.extra_loss_grad_hook = None      # hook(stage, iteration, grads): sees every iteration's complete gradient array before the Adam step
        self.extra_loss_history = {}
        g = self.specs.get
        if g('est_type', 'hybrik') != 'hybrik' or not g('flag_infer_motion_traj', False) or not g('flag_pred_traj', True) \
                or not g('flag_opt_traj', True) or not g('flag_infill_motion', True):
            raise NotImplementedError('only est_type=hybrik with motion infilling + trajectory prediction + trajectory optimisation '
                                      '(every shipped config) is supported')
        # flag_opt_vis_local_rot (:45,416-419): the per-frame rotation residual `traj_local_rot` is only applied at the frames a person is SEEN in.
        # A residual that is never applied gets no gradient (its regulariser's is 2 w r = 0 at r = 0) and Adam leaves it at its initial zero: the
        # flag amounts to "no update of traj_local_rot at invisible frames" -- run_schedule then goes launch by launch with that gradient mask
        self.flag_opt_vis_local_rot = bool(g('flag_opt_vis_local_rot', False))
        if self.flag_opt_vis_local_rot and (g('flag_opt_motion_latent', False) or g('flag_opt_traj_latent', False)):
            # (run_latent_schedule makes its own iterations and does not apply the gradient mask: refused rather than silently ignored)
            raise NotImplementedError('flag_opt_vis_local_rot together with the latent-optimisation mode')
        # flag_traj_from_cam (:55,237,325-351): the world trajectory is first read off the initial camera (orientation interpolated between the
        # frames a person is seen in, heading separately).  With a trajectory predictor -- the only mode this path runs -- init_traj_heading_from_cam
        # then overwrites every EXISTING frame (:283-289), so what the flag changes is the base pose of the frames outside a person's existence
        # range.  Round 5: on the device as well (glamr_init_scenes_ex, GLAMR_INIT_TRAJ_FROM_CAM); init_data_batch_host keeps its numpy twin.
        self.flag_traj_from_cam = bool(g('flag_traj_from_cam', False))
        if self.flag_traj_from_cam and g('traj_interp_method', 'linear_interp') != 'linear_interp':
            raise NotImplementedError("flag_traj_from_cam with traj_interp_method other than 'linear_interp'")
        # absolute_heading (:59,283,421): the heading entries of the local trajectory are absolute -- packing.stage_desc passes
        # GLAMR_FLAG_ABSOLUTE_HEADING, and every launch of the stage kernel (the 'init' forward passes included) then runs on the instances of
        # csrc/grecon_wide.hip.  (In latent mode the reference also converts the PREDICTED headings before opt_latent_start_iter, :441-444: refused.)
        if g('absolute_heading', False) and (g('flag_opt_motion_latent', False) or g('flag_opt_traj_latent', False)):
            raise NotImplementedError('absolute_heading together with the latent-optimisation mode')
        for flag in ('flag_opt_person2cam_rot',
                     'flag_opt_person2cam_trans'):
            if g(flag, False):
                raise NotImplementedError('%s is not supported by the MI355X path' % flag)
        if not g('flag_cam_inv_trans_res_all', True):
            raise NotImplementedError('flag_cam_inv_trans_res_all = False in grecon_model_specs is not supported')
        if not g('flag_opt_cam', True):
            raise NotImplementedError('flag_opt_cam = False in grecon_model_specs is not supported')
        # heading_type 'vec' (:191-193, 403-405): traj_local_heading (2,) and traj_local_dheading (len - 1, 2) are added to the (cos, sin)
        # slots of the prior rows before vec_to_heading.  They live in PackedScenes.t['heading_vec'], every stage launch (the 'init' forward passes
        # included) carries a glamr_stage_ext that points at it, and the variable's two regularisers are taken off every stage's loss_cfg here and
        # run in that extension.  heading_vec_loss_history[stage]: (scenes, iterations, 2) UNWEIGHTED values, with a log / keep_loss_history.
        self.heading_vec = packing.is_heading_vec(self.specs)
        self._heading_cfg = {}
        self.heading_vec_loss_history = {}
        if self.heading_vec:
            self.opt_stage_specs, self._heading_cfg = packing.split_heading_vec_specs(self.opt_stage_specs)
        # latent-optimisation mode (:43-44,155-158,434-437,619-622): the priors run INSIDE the Adam loop and the latent draws are parameters
        self.flag_opt_motion_latent = bool(g('flag_opt_motion_latent', False))
        self.flag_opt_traj_latent = bool(g('flag_opt_traj_latent', False))
        # flag_attach_traj_pred (NOT a reference key): the latent-optimisation mode with the trajectory prior ATTACHED -- what the reference would
        # compute with the .detach() of :396 removed.  `traj_latent` then receives a gradient (and moves, with flag_opt_traj_latent), and
        # `motion_latent` also the term infiller -> body pose -> FK joints -> predictor -> trajectory.  Off: the reference's behaviour, to the bit.
        self.flag_attach_traj_pred = bool(g('flag_attach_traj_pred', False))
        if self.flag_attach_traj_pred and not (self.flag_opt_motion_latent or self.flag_opt_traj_latent):
            raise ValueError('flag_attach_traj_pred needs the latent-optimisation mode (flag_opt_motion_latent and / or flag_opt_traj_latent)')
        # motion_latent_reg / traj_latent_reg (loss_func.py:293-310): run_latent_schedule takes them (glamr_latent_reg), the stage
        # kernel never sees them.  A term whose latent is not a parameter is refused here.  latent_loss_history[stage]: (scenes, iterations, 2)
        # UNWEIGHTED values, motion_latent_reg then traj_latent_reg, at the latents each iteration started from (a term the stage does not list: 0).
        packing.check_latent_regs(self.opt_stage_specs, self.specs)
        self.latent_loss_history = {}
        # penetration (loss_func.py:274-290): the multi-person term on the skinned vertices.  Not a term of the stage kernel: its entry
        # is taken off every stage's loss_cfg here (what every schedule and stage_desc see is the rest) and optimize / optimize_batch then run
        # extra_loss_schedule.ExtraLossSchedule with the built-in term (PenetrationTerm), beside a caller's extra_loss if one is set.  penetration_history[stage]:
        # (scenes, iterations) UNWEIGHTED values.  Without an entry in any stage nothing changes.
        self.flag_use_pen_loss = bool(g('flag_use_pen_loss', False))
        self.penetration_history = {}
        # the six terms of packing.AUX_LOSS_IDS (cam_rot_smoothness ... local_traj_dheading_reg): taken off every stage's loss_cfg
        # like the penetration term and run by the same schedule (extra_loss_schedule.AuxTerms, one launch of glamr_grecon_aux_terms per
        # iteration).  aux_loss_history[stage][name]: (scenes, iterations) UNWEIGHTED values.  Without one of the names in any stage nothing changes.
        self.aux_loss_history = {}
        # flag_aux_on_device (NOT a reference key): a run whose only terms outside the stage kernel are those six goes through
        # aux_step_schedule.AuxStepSchedule -- two launches per iteration, no host Python, values kept on the device until collect() -- on every
        # entry point, optimize_resident / capture_resident / optimize_stream included.  Off (the default), or with a caller's extra_loss or
        # the penetration term present: ExtraLossSchedule and its refusals, as before.
        self.flag_aux_on_device = bool(g('flag_aux_on_device', False))
        packing.check_penetration(self.opt_stage_specs, self.specs)
        packing.check_aux(self.opt_stage_specs, self.specs)
        self.opt_stage_specs, self._pen_cfg, self._aux_cfg = packing.split_off_kernel(self.opt_stage_specs)
        # world-frame residuals: `world_dxy` / `world_res` in opt_variables, traj_rot_res / traj_trans_res in loss_cfg.  Their names are
        # taken off every stage here (what every schedule and stage_desc see is the rest) and run_schedule launches those stages with a
        # glamr_stage_ext beside the descriptor (glamr_grecon_run_stage_ext: the instances of csrc/grecon_wide.hip).  world_loss_history[stage]:
        # (scenes, iterations, 2) UNWEIGHTED values, with a log / keep_loss_history.  Without one of the names in any stage nothing changes.
        self.opt_stage_specs, self._world_cfg = packing.split_world_specs(self.opt_stage_specs)
        self.world_loss_history = {}
        if self._world_cfg:
            what = 'world_dxy / world_res / traj_rot_res / traj_trans_res (the world-frame residuals)'
            # (the two VJP kernels and glamr_grecon_aux_step do not know the residuals; the other schedules make their own iterations without them)
            for on, other in ((bool(self._pen_cfg), 'the penetration term (loss_cfg)'), (bool(self._aux_cfg), self._aux_what() if self._aux_cfg else ''),
                              (bool(g('flag_aux_on_device', False)), 'flag_aux_on_device'),
                              (bool(g('flag_opt_motion_latent', False) or g('flag_opt_traj_latent', False)), 'the latent-optimisation mode'),
                              (self.flag_opt_vis_local_rot, 'flag_opt_vis_local_rot'), (bool(g('absolute_heading', False)), 'absolute_heading')):
                if on:
                    raise NotImplementedError('%s together with %s is not supported' % (what, other))
        if self.heading_vec:
            # (the VJP kernels, glamr_grecon_aux_step and the launch-by-launch schedules read the scalar heading entries, which are dead here)
            for on, other in ((bool(g('flag_attach_traj_pred', False)), 'flag_attach_traj_pred'),
                              (bool(g('flag_opt_motion_latent', False) or g('flag_opt_traj_latent', False)), 'the latent-optimisation mode'),
                              (bool(self._pen_cfg), 'the penetration term (loss_cfg)'), (bool(self._aux_cfg), self._aux_what() if self._aux_cfg else ''),
                              (bool(g('flag_aux_on_device', False)), 'flag_aux_on_device'),
                              (self.flag_opt_vis_local_rot, 'flag_opt_vis_local_rot'), (bool(g('absolute_heading', False)), 'absolute_heading')):
                if on:
                    raise NotImplementedError("heading_type = 'vec' together with %s is not supported" % other)
        if self._off_kernel_term() is not None:
            extra_loss_schedule.check_supported(self.specs, what=self._off_kernel_term())
        elif self._aux_on_device():
            extra_loss_schedule.check_supported(self.specs, what=self._aux_what())
        self.flag_filter_pose = g('flag_filter_pose', True)
        # keypoint-count filter inside filter_pose (:50-52,264-268); with HybrIK's binary scores (14 scored joints per detected frame) it is all or
        # nothing: the reference's default minimum of 15 removes every frame, 14 or less none
        self.flag_make_invis_with_keypoint = bool(g('flag_make_invis_with_keypoint', False))
        self.make_invis_keypoint_min_score = float(g('make_invis_keypoint_min_score', 0.6))
        self.make_invis_keypoint_min_num = int(g('make_invis_keypoint_min_num', 15))
        self.flag_init_cam_all_frames = g('flag_init_cam_all_frames', False)
        self.cam_fix_frames = [tuple(x) for x in g('cam_fix_frames', [[0, None]])]
        self.smpl = smpl if smpl is not None else SMPL(SMPL_MODEL_DIR, pose_type='body26fk', create_transl=False).to(self.device)
        self.mt_model = mt_model if mt_model is not None else MotionTrajJointModel(None, self.device, log, smpl=self.smpl, results_root=results_root)
        if self.flag_use_pen_loss:
            self.sdf_loss = SDFLoss(self.smpl.faces, robustifier=True)      # (:64-65)
        self.timings = {}

    @property
    def extra_loss(self):
        return self._extra_loss

    @extra_loss.setter
    def extra_loss(self, fn):
        if fn is not None:
            if not callable(fn):
                raise TypeError('extra_loss must be callable: extra_loss(ctx) -> tensor (S,)')
            if getattr(self, '_world_cfg', None):
                raise NotImplementedError('extra_loss together with world_dxy / world_res / traj_rot_res / traj_trans_res (the world-frame residuals) is not '
                                          'supported: glamr_grecon_pose_backward does not know the residuals')
            if getattr(self, 'heading_vec', False):
                raise NotImplementedError("extra_loss together with heading_type = 'vec' is not supported: glamr_grecon_pose_backward reads the scalar "
                                          'heading entries')
            extra_loss_schedule.check_supported(self.specs)
        self._extra_loss = fn

    flag_aux_on_device = False      # (the default of grecon_model_specs.flag_aux_on_device, also for an optimiser that never ran __init__)
    heading_vec, _heading_cfg = False, {}      # (heading_type 'scalar', likewise)

    def _aux_what(self):
        return extra_loss_schedule.aux_what({n for c in self._aux_cfg.values() for n in c})

    def _aux_on_device(self):
        """flag_aux_on_device takes effect: the run lists terms of packing.AUX_LOSS_IDS and neither a caller's extra_loss nor a penetration term."""
        return self.flag_aux_on_device and bool(self._aux_cfg) and self._extra_loss is None and not self._pen_cfg

    def _off_kernel_term(self):
        """None when the run has no term the stage kernel does not hold -- run_schedule serves it -- or flag_aux_on_device takes effect --
        AuxStepSchedule does --, else the name a refusal gives what needs the launch-by-launch schedule: the caller's term before the
        penetration term before the terms of packing.AUX_LOSS_IDS."""
        if self._aux_on_device():
            return None
        return 'extra_loss' if self._extra_loss is not None else 'the penetration term (loss_cfg)' if self._pen_cfg else \
            self._aux_what() if self._aux_cfg else None

    _WHY_OPTIMIZE_ONLY = {'extra_loss': 'while extra_loss is set: the term runs user Python in every iteration',
                          'the penetration term (loss_cfg)': 'with the penetration term in loss_cfg: the term runs launch by launch on the skinned vertices'}

    def _refuse_extra_loss(self, what):
        term = self._off_kernel_term()
        if term is not None:
            why = self._WHY_OPTIMIZE_ONLY.get(term, 'with %s: these terms run launch by launch on a kernel of their own' % term)
            raise NotImplementedError('%s %s (optimize / optimize_batch only)' % (what, why))

    def _run_schedule_or_extra(self, packed, max_iters, has_wd=False):
        if packed.has_world_dxy and (self._aux_on_device() or self._off_kernel_term() is not None):
            # (a continued optimisation of a result that carries world_dxy: the reference adds it on every frame of every later stage, :467-468,
            # and the launch-by-launch schedules do not know it)
            raise NotImplementedError('an existing world_dxy (the world-frame residuals) together with %s is not supported'
                                      % ('the loss_cfg terms of glamr_grecon_aux_step' if self._aux_on_device() else self._off_kernel_term()))
        if self._aux_on_device():
            return aux_step_schedule.AuxStepSchedule(self, packed).run(max_iters, has_wd=has_wd)
        if self._off_kernel_term() is None:
            return self.run_schedule(packed, max_iters, has_wd=has_wd)
        return extra_loss_schedule.ExtraLossSchedule(self, packed).run(max_iters, has_wd=has_wd)

    @property
    def latent_source(self):
        return self._latent_source

    @latent_source.setter
    def latent_source(self, value):
        self._latent_source = latent_rng.check_source(value)

    def _latent_table(self, rin):
        """latent_source 'philox': the per-slot (sequence id, person id) table of a staged batch and the seed word its draw kernel reads, on the
        device (person id -1 = an empty slot of a scene with fewer persons than the batch maximum: its draws are zeros)."""
        seq_ids, person_ids = [], []
        for si, m in enumerate(rin.meta):
            # (an explicit in_dict['seq_id'] was noted by stage_inputs whatever the source was then: a batch staged under 'torch' draws the same)
            sid = latent_rng.seq_id_for(dict(seq_name=m['seq_name'], seq_id=rin.explicit_seq_ids[si]))
            for pi in range(rin.P):
                seq_ids.append(sid)
                person_ids.append(latent_rng.person_id_of(rin.ids[si][pi]) if pi < len(rin.ids[si]) else -1)
        rin.latent_seq_ids, rin.latent_person_ids = latent_rng.slot_table(seq_ids, person_ids, self.device)
        rin.latent_seed_word = latent_rng.new_seed_word(self.device)

    def _draw_latents(self, rin, meps, teps):
        """glamr_latents_draw into (meps, teps) on the current stream.  Outside a capture the seed word is written first; a captured step holds
        the draw only and ResidentGraph.replay() writes the seed (so the seed can change between replays without re-capture)."""
        if rin.latent_seq_ids is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("this batch was staged under latent_source 'torch': stage_inputs() it again under 'philox' before capturing")
            self._latent_table(rin)
        if not torch.cuda.is_current_stream_capturing():
            latent_rng.set_seed(rin.latent_seed_word, self.latent_seed)
        latent_rng.draw_into(rin.latent_seed_word, rin.latent_seq_ids, rin.latent_person_ids, meps.shape[1], meps, teps)

    # ------------------------------------------------------------------------------------------------------------------------
    # host preprocessing of one person (global_recon_model.py:88-148)
    # ------------------------------------------------------------------------------------------------------------------------
    def _person_arrays(self, src):
        d = {}
        d['visible'] = visible = src['bboxes_dict']['exist'].copy()                      # float64, compared with == 1 / == 0
        d['visible_orig'] = visible.copy()
        nz = np.where(visible)[0]
        d['fr_start'], d['fr_end'] = start, end = nz[0], nz[-1] + 1
        d['exist_frames'] = visible == 1
        d['exist_frames'][start:end] = True
        d['exist_len'] = end - start
        d['max_len'] = max_len = visible.shape[0]
        d['frames'] = np.arange(max_len)
        vis_frames = visible == 1
        d['frame2ind'] = {f: i for i, f in enumerate(d['frames'])}
        d['scale'] = None
        rm = src['smpl_pose_quat_wroot']
        nvis = rm.shape[0]
        aa = nt.rotmat_to_rotvec_nearest(rm.reshape((-1, 3, 3))).reshape((nvis, -1, 3)).astype(np.float32)     # = scipy Rotation.from_matrix(..).as_rotvec() (:105-108)
        d['smpl_pose'] = aa[:, 1:].reshape(-1, 69)
        d['smpl_beta'] = src['smpl_beta']
        d['smpl_orient_cam'] = aa[:, 0]
        d['root_trans_cam'] = src['root_trans']
        kp = np.concatenate((src['kp_2d'][:, :24], np.ones_like(src['kp_2d'][:, :24, [0]])), axis=-1)
        kps = np.zeros((int(vis_frames.sum()), 26, 3))
        kps[:, SMPL_TO_BODY26FK[:, 0]] = kp[:, SMPL_TO_BODY26FK[:, 1]]
        d['kp_2d'], d['kp_2d_score'] = kps[:, :, :2], kps[:, :, 2]
        d['kp_2d_aligned'] = d['kp_2d'].copy()
        d['cam_K'] = src['cam_K'].astype(np.float32)
        if not np.all(visible):
            for key in ('kp_2d', 'kp_2d_score', 'kp_2d_aligned', 'cam_K'):
                full = np.zeros((max_len,) + d[key].shape[1:], dtype=d[key].dtype)
                full[vis_frames] = d[key]
                d[key] = full
            vis_ind = np.where(visible)[0]
            for key in ('smpl_pose', 'smpl_beta', 'root_trans_cam', 'smpl_orient_cam'):
                d[key] = nt.lerp_extrapolate(vis_ind, d[key], max_len)
        for key in ('smpl_pose', 'smpl_beta', 'root_trans_cam', 'smpl_orient_cam'):
            d[key] = np.ascontiguousarray(d[key], dtype=np.float32)
        if self.flag_filter_pose:
            self._filter_pose(d)
            if self.flag_make_invis_with_keypoint:                                        # :264-268
                vis_ind = np.where(d['visible'] == 1.0)[0]
                num_valid = (d['kp_2d_score'][vis_ind] > self.make_invis_keypoint_min_score).sum(axis=1)
                d['visible'][vis_ind[num_valid < self.make_invis_keypoint_min_num]] = 0.0
        d['vis_frames'] = d['visible'] == 1
        d['invis_frames'] = d['visible'] == 0
        # identity initial camera: world := camera frame (:141-144)
        d['root_trans_world_base'] = d['root_trans_cam'].copy()
        d['smpl_orient_world_base'] = nt.quat_to_aa(nt.rotmat_to_quat(nt.aa_to_rotmat(d['smpl_orient_cam'])))
        d['smpl_pose_nofill'] = d['smpl_pose'].copy()
        d['smpl_pose_nofill'][~d['exist_frames']] = 0.0
        return d

    @staticmethod
    def _filter_pose(d):
        """:250-262, the numpy twin of the loop in csrc/init.hip prep_person_kernel (sequential and data dependent: one thread there)."""
        visible = d['visible']
        quat = nt.aa_to_quat(d['smpl_orient_cam'])
        jump = nt.quat_angle_between(quat[1:], quat[:-1])
        ind = np.where((jump > np.pi / 3) & (visible[1:] != 0))[0] + 1
        ind_set = set(int(i) for i in ind)
        for i in ind:
            if visible[i - 1]:
                if i + 1 < quat.shape[0] and visible[i + 1] and (i + 1) not in ind_set:
                    visible[i - 1] = 0
                else:
                    visible[i] = 0

    # ------------------------------------------------------------------------------------------------------------------------
    # scene initialisation after the priors have run (:166-246)
    # ------------------------------------------------------------------------------------------------------------------------
    def _init_scene(self, in_dict, persons):
        first = next(iter(persons.values()))
        num_fr = first['max_len']
        for d in persons.values():
            d['person_transform_cam'] = nt.make_transform(d['smpl_orient_cam'], d['root_trans_cam'])
            d['person2cam'] = nt.invert_transform(d['person_transform_cam'])
            d['person_transform_world'] = nt.make_transform(d['smpl_orient_world'], d['root_trans_world'])
            n = int(d['exist_len'])
            d['traj_local_xy'] = np.zeros(2, np.float32)
            d['traj_local_dxy'] = np.zeros((n - 1, 2), np.float32)
            d['traj_local_heading'] = np.zeros(2 if self.heading_vec else 1, np.float32)      # (:191-193)
            d['traj_local_dheading'] = np.zeros((n - 1, 2) if self.heading_vec else n - 1, np.float32)
            d['traj_local_z'] = np.zeros(n, np.float32)
            d['traj_local_rot'] = np.zeros((n, 6), np.float32)
        ids = list(persons.keys())
        rel = {}
        for i in range(len(ids)):
            for j in range(len(ids)):
                if i != j:
                    rel[(i, j)] = np.matmul(nt.invert_transform(persons[ids[i]]['person_transform_cam']), persons[ids[j]]['person_transform_cam'])
        fr_num_persons = sum(d['vis_frames'].astype(np.int64) for d in persons.values())
        n_empty = int((fr_num_persons == 0).sum())
        data = {
            'seq_name': in_dict['seq_name'], 'person_data': persons, 'seq_len': num_fr, 'fr_num_persons': fr_num_persons,
            'cam_pose': np.tile(np.eye(4, dtype=np.float32), (num_fr, 1, 1)), 'cam_pose_inv': np.tile(np.eye(4, dtype=np.float32), (num_fr, 1, 1)),
            'cam_inv_rot_residual': np.zeros((n_empty, 6), np.float32), 'cam_inv_trans_residual': np.zeros((num_fr, 3), np.float32),
            'rel_transform_cam': rel, 'gt': in_dict.get('gt', {}), 'gt_meta': in_dict.get('gt_meta', {}),
            'meta': {'algo': 'global_recon', 'num_fr': num_fr},
        }
        self._init_cam_pose(data, all_frames=False)
        if self.flag_traj_from_cam:                                  # get_traj_from_cam (:325-351), traj_interp_method 'linear_interp'
            for d in persons.values():
                w = np.matmul(data['cam_pose_inv'], d['person_transform_cam'])
                d['person_transform_world'] = w
                q = nt.rotmat_to_quat(np.ascontiguousarray(w[:, :3, :3]))
                qi = nt.interp_orient_sep_heading(q[d['vis_frames']], d['vis_frames'])
                d['root_trans_world'] = d['root_trans_world_base'] = np.ascontiguousarray(w[:, :3, 3]).astype(np.float32)
                d['smpl_orient_world'] = d['smpl_orient_world_base'] = nt.quat_to_aa(qi).astype(np.float32)
        # heading initialisation from the camera (:273-292); the resulting world trajectory is produced by the device forward pass
        for d in persons.values():
            w = np.matmul(data['cam_pose_inv'], d['person_transform_cam'])
            q = nt.rotmat_to_quat(np.ascontiguousarray(w[:, :3, :3]))
            qi = nt.interp_orient_sep_heading(q[d['vis_frames']], d['vis_frames'])
            local = nt.global_to_local_traj(w[:, :3, 3], qi)[d['exist_frames']]
            for (s, e) in self.cam_fix_frames:
                d['traj_local_pred'][s:e, -2:] = local[s:e, -2:]
        return data

    def _init_cam_pose(self, data, all_frames):
        """:294-317 -- camera-to-world from the FIRST person only; with all_frames the frames the first person is not seen in are
        left as zero matrices (the reference's forward fill writes into a discarded tensor)."""
        first = next(iter(data['person_data'].values()))
        cand = np.matmul(first['person_transform_world'], first['person2cam']) * first['vis_frames'][:, None, None].astype(np.float32)
        ind = data['fr_num_persons'] > 0
        start = np.where(ind)[0][0]
        inf = np.zeros_like(data['cam_pose'])
        inf[ind] = cand[ind]
        if not all_frames:
            inf[...] = inf[[start]].copy()
        inf[:, :3, :3] = nt.sixd_to_rotmat(nt.rotmat_to_6d(inf[:, :3, :3]))
        data['pose_infer_cam_pose_inv'] = inf
        data['cam_pose_inv'] = inf
        data['cam_pose'] = nt.invert_transform(inf)

    # ------------------------------------------------------------------------------------------------------------------------
    # batched pipeline
    # ------------------------------------------------------------------------------------------------------------------------
    def init_data_batch_host(self, in_dicts, latents=None, init_forward=True):
        """Host-side variant of init_data_batch (numpy; kept for cam_fix_frames other than the default and as a cross-check):
        host preprocessing + ONE batched prior inference + scene initialisation.  latents: optional list (per sequence) of
        {person idx: {'motion': (n_windows,128), 'traj': (1,128)}} replacing the Gaussian draws."""
        t0 = time.time()
        dev = self.device
        scenes = [{idx: self._person_arrays(src) for idx, src in in_dict['est'].items()} for in_dict in in_dicts]
        flat = [(si, idx, d) for si, persons in enumerate(scenes) for idx, d in persons.items()]
        lens = [int(d['exist_len']) for _, _, d in flat]
        Tm = max(lens)
        nw = num_windows(Tm)
        pose = np.zeros((len(flat), Tm, 69), np.float32)
        vis = np.zeros((len(flat), Tm), np.float32)
        for k, (si, idx, d) in enumerate(flat):
            ex = d['exist_frames']
            pose[k, :lens[k]] = d['smpl_pose_nofill'][ex]
            vis[k, :lens[k]] = d['visible'][ex]
        if latents is not None:
            meps, teps = packing.pack_latents(latents, [(si, idx) for si, idx, _ in flat], nw, NZ, dev)
        elif self.latent_source == 'philox':
            sids = [latent_rng.seq_id_for(d) for d in in_dicts]
            meps, teps = latent_rng.draw(self.latent_seed, [sids[si] for si, _, _ in flat], [latent_rng.person_id_of(idx) for _, idx, _ in flat], nw, dev)
        else:
            meps, teps = torch.randn((len(flat), nw, NZ), device=dev), torch.randn((len(flat), NZ), device=dev)
        t1 = time.time()
        out = self.mt_model.infer_padded(torch.from_numpy(pose).to(dev), torch.from_numpy(vis).to(dev), lens, meps, teps)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        t2 = time.time()
        for k, (si, idx, d) in enumerate(flat):                                              # infer_motion_traj :370-392
            ex, n = d['exist_frames'], lens[k]
            d['infilled'] = d['traj_predicted'] = True
            d['smpl_pose'] = d['smpl_pose'].copy()
            d['smpl_pose'][ex] = out['pose'][k, :n]
            d['traj_local_pred'] = out['local_traj'][k, :n].copy()
            d['smpl_orient_world_base'][ex] = out['orient'][k, :n]
            d['root_trans_world_base'][ex] = out['trans'][k, :n]
            d['smpl_orient_world'], d['root_trans_world'] = d['smpl_orient_world_base'], d['root_trans_world_base']
        datas = [self._init_scene(in_dict, persons) for in_dict, persons in zip(in_dicts, scenes)]
        t3 = time.time()
        # root-relative joints, cached for the whole optimisation: one batched skinning call
        poses = np.concatenate([d['smpl_pose'] for _, _, d in flat])
        betas = np.concatenate([d['smpl_beta'] for _, _, d in flat])
        zeros = torch.zeros((poses.shape[0], 3), device=dev)
        with torch.no_grad():
            jl = self.smpl(global_orient=zeros, body_pose=torch.from_numpy(poses).to(dev), betas=torch.from_numpy(betas).to(dev),
                           root_trans=zeros, return_verts=False).joints
        j_locals, off = [dict() for _ in scenes], 0
        for si, idx, d in flat:
            j_locals[si][idx] = jl[off:off + d['max_len']]
            off += d['max_len']
        # first world trajectory + (optionally) the all-frames camera, then the 'init' forward pass (:241-246)
        packed = packing.PackedScenes(datas, j_locals, dev, self.cam_fix_frames, heading_vec=self.heading_vec)
        self._run(packed, self._forward_only_desc())
        if self.flag_init_cam_all_frames:
            h = packed.fetch(('orient_world', 'trans_world'))
            for si, dn in enumerate(datas):
                for pi, idx in enumerate(packed.person_ids[si]):
                    T = dn['seq_len']
                    dn['person_data'][idx]['person_transform_world'] = nt.make_transform(h['orient_world'][si * packed.P + pi, :T],
                                                                                           h['trans_world'][si * packed.P + pi, :T])
                self._init_cam_pose(dn, all_frames=True)
            packed.set_cam_pose([dn['cam_pose'] for dn in datas])
            self._run(packed, self._forward_only_desc())
        packed.unpack_into(datas, None, self.specs, as_torch=False)      # world trajectory / projections of the 'init' forward pass
        self.timings.update(host_pre=t1 - t0, priors=t2 - t1, host_init=t3 - t2, lbs_pack_init=time.time() - t3)
        return datas, packed


    # ------------------------------------------------------------------------------------------------------------------------
    # device pipeline: the host only scatters the HybrIK arrays to their frame rows (pose_est/hybrik_demo/demo.py:317-354 layout)
    # ------------------------------------------------------------------------------------------------------------------------
    def _staging(self, n_slots, T):
        """Pinned host staging buffers for the HybrIK arrays, two sets used alternately (a set is rewritten only after the upload that
        last used it has finished).  Rows of frames without a detection keep whatever an earlier batch left there: the device
        preparation reads detection rows only (init.hip prep_person_kernel); `exist` and `K` are cleared because their other rows count."""
        pool = self._pinned
        i = pool['turn']
        pool['turn'] = 1 - i
        cur = pool['sets'][i]
        widths = dict(exist=0, rot=216, betas=10, trans=3, kp=48, K=9)
        if cur is None or cur['shape'] != (n_slots, T):
            mk = lambda w: torch.empty((n_slots, T, w) if w else (n_slots, T), dtype=torch.float32, pin_memory=True).zero_()
            cur = {'shape': (n_slots, T), 't': {k: mk(w) for k, w in widths.items()}, 'event': None}
            cur['np'] = {k: v.numpy() for k, v in cur['t'].items()}
            pool['sets'][i] = cur
        else:
            if cur['event'] is not None:
                cur['event'].synchronize()
            cur['np']['exist'].fill(0.0)
            cur['np']['K'].fill(0.0)
        return cur

    def _scatter_inputs(self, in_dicts, ids, P, h):
        """Per-detection HybrIK arrays -> their frame rows in the staging arrays `h` (numpy views): glamr_host_scatter, a few host threads
        doing block copies without the GIL (numpy on one thread took 60-130 ms per 1024 sequences depending on the box, a Python thread
        pool was slower still).  This loop only collects the ten numbers per person the library needs.  Returns (seq_len per slot,
        length of the existing range per slot, {(sequence, person id): exist array})."""
        n_slots = len(in_dicts) * P
        T = h['exist'].shape[1]
        seq_len_slot = np.zeros(n_slots, np.int32)
        lens = np.full(n_slots, 11, np.int32)
        exists = {}
        table = np.zeros((n_slots, 10), np.int64)
        keep = []                                                  # converted copies must outlive the call
        f32, f64 = np.dtype(np.float32), np.dtype(np.float64)

        def addr(a, width):
            if type(a) is not np.ndarray or a.dtype != f32 or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=np.float32)
                keep.append(a)
            if a.size != nv * width:
                raise ValueError('a per-detection array has %d values, expected %d x %d' % (a.size, nv, width))
            return a.__array_interface__['data'][0]
        for si, d in enumerate(in_dicts):
            est = d['est']
            for pi, idx in enumerate(ids[si]):
                src = est[idx]
                ex = np.asarray(src['bboxes_dict']['exist'])
                exists[(si, idx)] = ex
                exa = ex
                if exa.dtype != f64 and exa.dtype != f32 or not exa.flags.c_contiguous:
                    exa = np.ascontiguousarray(exa, dtype=np.float64)
                    keep.append(exa)
                nv = len(src['smpl_beta'])
                kpw = 2 * int(np.shape(src['kp_2d'])[1])               # floats per detection row: HybrIK writes 29 keypoints, the wire format asks for >= 24
                table[si * P + pi] = (exa.__array_interface__['data'][0], exa.dtype == f64, exa.shape[0], nv, addr(src['smpl_pose_quat_wroot'], 216),
                                      addr(src['smpl_beta'], 10), addr(src['root_trans'], 3), addr(src['cam_K'], 9), addr(src['kp_2d'], kpw), kpw)
        # (rows left at zero = the empty person slots of scenes with fewer persons than the batch maximum: seq_len 0, nothing copied)
        stg = _lib.HostStaging(*[ctypes.c_void_p(h[k].ctypes.data) for k in ('exist', 'rot', 'betas', 'trans', 'K', 'kp')])
        _lib.check(_lib.lib().glamr_host_scatter(n_slots, ctypes.c_void_p(table.ctypes.data), T, ctypes.byref(stg), ctypes.c_void_p(seq_len_slot.ctypes.data),
                                                 ctypes.c_void_p(lens.ctypes.data), self._copy_threads()))
        return seq_len_slot, lens, exists

    def stage_inputs(self, in_dicts, latents=None, validate=True):
        """Host dictionaries -> HBM: checks them against the wire format (glamr_amd/utils/wire.py: keys and shapes on the host, values --
        finite numbers, orthonormal rotation matrices -- on the uploaded arrays, reported by check_inputs() / collect()), scatters the
        per-detection HybrIK arrays to their frame rows in pinned staging buffers and uploads them asynchronously (the ONLY host->device
        traffic of a batch).  Returns a ResidentInputs; everything after this runs on device arrays."""
        t0 = time.time()
        dev = self.device
        if validate:
            from glamr_amd.utils import wire
            for d in in_dicts:
                wire.check_layout(d['est'])
        S = len(in_dicts)
        ids = [list(d['est'].keys()) for d in in_dicts]
        P = max(len(x) for x in ids)
        Ts = [len(d['est'][i[0]]['bboxes_dict']['exist']) for d, i in zip(in_dicts, ids)]
        T = max(Ts)
        if P > 32:
            raise NotImplementedError('at most 32 persons per scene (csrc/grecon_wide.hip)')
        n_slots = S * P
        stg = self._staging(n_slots, T)
        h = stg['np']
        seq_len_slot, lens, exists = self._scatter_inputs(in_dicts, ids, P, h)
        up = lambda x: x.to(dev, non_blocking=True)
        rin = ResidentInputs(S, P, T, Ts, ids, lens, exists, g={k: up(v) for k, v in stg['t'].items()},
                             n_persons=up(torch.tensor([len(x) for x in ids], dtype=torch.int32)), seq_len=up(torch.tensor(Ts, dtype=torch.int32)),
                             seq_len_slot=up(torch.from_numpy(seq_len_slot)), validate=validate, explicit_seq_ids=[d.get('seq_id') for d in in_dicts],
                             meta=[{'seq_name': d['seq_name'], 'seq_len': Ts[si], 'gt': d.get('gt', {}), 'gt_meta': d.get('gt_meta', {})} for si, d in enumerate(in_dicts)])
        if latents is not None:
            slots = [(si, ids[si][pi]) if pi < len(ids[si]) else None for si in range(S) for pi in range(P)]
            rin.meps, rin.teps = packing.pack_latents(latents, slots, num_windows(int(lens.max())), NZ, dev)
        if self.latent_source == 'philox' and latents is None:
            self._latent_table(rin)                          # (uploaded with the rest of the batch: before `upload_done`)
        # one event for "uploaded", on the stream this call ran on: the staging set is rewritten only after it and a pipelined caller's compute
        # stream waits for it.  The VALUE checks of the wire format run on the device later, on the stream that consumes the batch
        # (value_checks(), called by init_resident): as kernels of the upload stream they gated `upload_done` while competing for CUs with
        # the previous batch's optimiser stage -- a pipelined caller's next batch started 15 ms late.
        stg['event'] = torch.cuda.Event()
        stg['event'].record()
        rin.upload_done = stg['event']
        self.timings['host_pre'] = time.time() - t0
        return rin

    @staticmethod
    def value_checks(rin):
        """Every number of a detection row finite, the 24 matrices of `smpl_pose_quat_wroot` orthonormal to 1e-2 (the field is named after
        quaternions, demo.py:320): glamr_check_inputs, ONE pass over the uploaded arrays on the current stream (the torch expressions it
        replaces were 5 ms of reductions per 1024 sequences), once per ResidentInputs; the verdict (2, n_slots) stays on the device until
        check_inputs() / collect() reads it."""
        if not rin.validate or rin.verdict is not None:
            return
        raw, g = rin.raw_batch(), rin.g
        verdict = torch.empty((2, raw.n_slots), dtype=torch.int32, device=g['exist'].device)
        _lib.check(_lib.lib().glamr_check_inputs(ctypes.byref(raw), _lib.ptr(g['K']), _lib.ptr(verdict), _lib.current_stream()))
        rin.verdict = verdict                                                                    # (2, n_slots) on the device
        rin.verdict_ready = torch.cuda.Event()
        rin.verdict_ready.record()
        rin.validate = False

    @staticmethod
    def _copy_threads():
        return max(1, min(8, (os.cpu_count() or 4) // 2))

    def check_inputs(self, rin):
        """Raises WireFormatError for the first person whose uploaded arrays failed the value checks (one small device->host copy)."""
        if rin.verdict is None:
            if rin.validate and not torch.cuda.is_current_stream_capturing():
                self.value_checks(rin)                                  # a batch nobody has checked yet (its only uses so far were graph replays)
            if rin.verdict is None:
                return
        from glamr_amd.utils import wire
        hv = rin.verdict_host
        if hv is not None:                                             # (copied with the batch's results: _fetch_async)
            hv[1].synchronize()
            v = hv[0].numpy()
            rin.verdict_host = None
        else:
            rin.verdict_ready.synchronize()                             # computed on the stream that consumed the batch
            v = rin.verdict.cpu().numpy()
        rin.verdict = None
        for kind, msg in ((0, 'smpl_pose_quat_wroot does not hold rotation matrices (|R R^T - I| > 1e-2); the field is named after quaternions but '
                              'carries 24 x 3 x 3 matrices regrouped by 4 (demo.py:320)'), (1, 'an input array contains non-finite values')):
            bad = np.flatnonzero(v[kind])
            if bad.size:
                si, pi = divmod(int(bad[0]), rin.P)
                raise wire.WireFormatError('sequence %d (%s), person %r: %s' % (si, rin.meta[si]['seq_name'], rin.ids[si][pi] if pi < len(rin.ids[si]) else pi, msg))

    def _init_prepare(self, rin, packed, pa_t):
        """glamr_init_prepare on the staged batch: visibility bookkeeping, rotation matrices -> axis-angle, interpolation over detection gaps,
        filter_pose (:88-148,250-271).  Returns the structures the following launches share."""
        L, n_slots, T, raw = _lib.lib(), rin.S * rin.P, rin.T, rin.raw_batch()
        pa = _lib.PersonArrays()
        for name, ten in pa_t.items():
            setattr(pa, name, ctypes.c_void_p(ten.data_ptr()))
        sb = packed.struct()
        ws = torch.empty(L.glamr_init_workspace_bytes(n_slots, T), dtype=torch.uint8, device=self.device)
        st = _lib.current_stream()
        fo = _lib.FilterOpts(int(bool(self.flag_filter_pose)), int(self.flag_make_invis_with_keypoint), self.make_invis_keypoint_min_score, self.make_invis_keypoint_min_num)
        _lib.check(L.glamr_init_prepare(ctypes.byref(raw), ctypes.byref(sb), ctypes.byref(pa), ctypes.byref(fo), _lib.ptr(ws), st))
        return pa, sb, ws, st

    def prepare_only(self, in_dicts):
        """The per-person preparation alone (no priors, no scene): `visible` after filter_pose, (person slots, frames) float32 on the host.
        For inspecting what the filters of :250-271 do to a batch (a batch they leave without a visible frame cannot be reconstructed)."""
        rin = self.stage_inputs(in_dicts)
        n_slots, T, dev = rin.S * rin.P, rin.T, self.device
        packed = packing.PackedScenes.empty(rin.S, rin.P, T, dev)
        packed.t['cam_K'], packed.t['n_persons'], packed.t['seq_len'] = rin.g['K'], rin.n_persons, rin.seq_len
        packed.t['j_local'] = torch.zeros(1, dtype=torch.float32, device=dev)
        pa_t = packing.carve_zeros([('visible_orig', torch.float32, (n_slots, T)), ('smpl_pose', torch.float32, (n_slots, T, 69)), ('smpl_beta', torch.float32, (n_slots, T, 10)),
                                    ('trans_cam', torch.float32, (n_slots, T, 3)), ('nets_pose', torch.float32, (n_slots, T, 69)), ('nets_vis', torch.float32, (n_slots, T))], dev)
        self._init_prepare(rin, packed, pa_t)
        torch.cuda.synchronize(dev)
        return packed.t['vis'].view(n_slots, T).cpu().numpy()

    def init_resident(self, rin, init_forward=True):
        """init_data (:76-248) on device-resident inputs: per-person preparation, motion priors, scene assembly, cached joints and
        the 'init' forward pass -- kernel launches only, nothing crosses PCIe.  Returns (datas, packed): `datas` are light
        per-sequence dictionaries that collect() completes from the device arrays."""
        t1 = time.time()
        dev, L = self.device, _lib.lib()
        S, P, T, g = rin.S, rin.P, rin.T, rin.g
        n_slots = S * P
        gate = self.pipeline_gate
        # The gate is waited for where the PRIORS start, not where the batch starts: the arrays' zero fills and the per-person preparation (1.6 ms on
        # the chain preparation -> infiller -> predictor) read the inputs only and run beside the previous batch's priors; capture_resident cuts the
        # step into three graphs for it (preparation | priors + skinning | rest): 34.7 against 38.5 ms per 1024-sequence step.  Round 5 kept this
        # behind a knob because its replays sometimes differed from the plain step; round 6 found the cause (packed-fp32 VALU instructions beside the
        # other stream's MFMA kernels: glamr_amd/build.py) and removed it.  GLAMR_GATE_PREP=late selects the two-graph cut.
        prep_early = gate is not None and os.environ.get('GLAMR_GATE_PREP', 'early') != 'late'
        if not torch.cuda.is_current_stream_capturing():
            self.value_checks(rin)                                       # (first use of this batch only)
            if gate is not None and not prep_early:
                gate.before(torch.cuda.current_stream(dev))
        packed = packing.PackedScenes.empty(S, P, T, dev, seq_names=[str(m['seq_name']) for m in rin.meta])
        packed.heading_vec = self.heading_vec      # (heading_type 'vec': zeros of their own, made with the first launch's extension)
        packed.person_ids = rin.ids
        packed.t['cam_K'] = g['K']
        packed.t['n_persons'] = rin.n_persons
        packed.t['seq_len'] = rin.seq_len
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        # inputs / outputs / workspace of the priors live at fixed addresses (two sets per stream): the library replays the call as a HIP graph
        nw = num_windows(int(rin.lens.max()))
        rs = self.mt_model.handle.resident_set(n_slots, T, nw) if hasattr(self.mt_model, 'handle') else None
        pa_t = packing.carve_zeros([('visible_orig', torch.float32, (n_slots, T)), ('smpl_pose', torch.float32, (n_slots, T, 69)),
                                    ('smpl_beta', torch.float32, (n_slots, T, 10)), ('trans_cam', torch.float32, (n_slots, T, 3))], dev)
        pa_t['nets_pose'] = rs['nets_pose'] if rs else f32(n_slots, T, 69)
        pa_t['nets_vis'] = rs['nets_vis'] if rs else f32(n_slots, T)
        # the cached joints are produced in place by the skinning kernel: keep a placeholder until then
        packed.t['j_local'] = f32(1)
        pa, sb, ws, st = self._init_prepare(rin, packed, pa_t)
        if prep_early:
            if self._capture_head_split is not None:
                self._capture_head_split()                             # capture_resident under a gate: the first cut (replay() waits for the gate there)
            elif not torch.cuda.is_current_stream_capturing():
                gate.before(torch.cuda.current_stream(dev))
        # the latent draws of the motion priors.  Where they live: the priors' fixed arrays when there is a resident set, else the caller's own
        # tensors or fresh ones.  What fills them: the caller's latents, the library's Philox streams, or torch.randn (motion, then trajectory).
        given = rin.meps is not None
        meps, teps = (rs['meps'], rs['teps']) if rs else (rin.meps, rin.teps) if given else \
            (torch.empty((n_slots, nw, NZ), device=dev), torch.empty((n_slots, NZ), device=dev))
        if given:
            if rs:
                meps.copy_(rin.meps)
                teps.copy_(rin.teps)
        elif self.latent_source == 'philox':
            self._draw_latents(rin, meps, teps)
        else:
            torch.randn(meps.shape, out=meps)
            torch.randn(teps.shape, out=teps)
        # motion priors on every person of every sequence in one call
        def open_gate():
            if self._capture_split is not None:
                self._capture_split()                                   # capture_resident under a gate: the graph is cut here
            elif gate is not None and not torch.cuda.is_current_stream_capturing():
                gate.after(torch.cuda.current_stream(dev))
        # the next batch may start when this batch's priors are done (opening the gate later lets the rest of this batch's preparation run
        # without the next batch's first kernels beside it, but that batch starts later: profiles/r05_pipeline_experiments.log)
        # Under a gate the SKINNING runs between the infiller and the trajectory predictor, i.e. before the gate opens: everything it needs (the
        # infilled poses in video-frame rows, glamr_init_scatter_pose) is known by then, and it runs alone (1.5 ms) instead of beside the next batch's
        # first kernels (2.4 ms): 34.7 against 35.4 ms per step (profiles/r06_pipeline_corruption.log).  (Round 5 moved it there to dodge the
        # corruption of its results beside the other stream's attention kernels; with that fixed at its root the order is kept for its speed.)
        skin_early = gate is not None and hasattr(self.mt_model, 'handle')

        def skin():
            # root-relative joints of every frame, cached for the whole optimisation
            packed.t['j_local'] = self.smpl.root_relative_joints(pa_t['smpl_pose'].view(-1, 69), pa_t['smpl_beta'].view(-1, 10)).view(n_slots, T, 26, 3)

        def skin_after_infiller(out_inf):
            _lib.check(L.glamr_init_scatter_pose(ctypes.byref(sb), ctypes.byref(pa), _lib.ptr(out_inf['pose']), st))
            skin()
        out = self.mt_model.infer_padded(pa_t['nets_pose'], pa_t['nets_vis'], rin.lens, meps, teps, buffers=rs, coschedule=gate is not None,
                                         between=skin_after_infiller if skin_early else None)
        open_gate()
        packed.latents = (meps, teps)                                  # the draws this batch was initialised with (parameters in latent-optimisation mode)
        # (flag_traj_from_cam :237,325-351: the base pose of the frames outside a person's existence range read off the initial camera)
        _lib.check(L.glamr_init_scenes_ex(ctypes.byref(sb), ctypes.byref(pa), _lib.ptr(out['pose']), _lib.ptr(out['local_traj']), _lib.ptr(out['trans']),
                                          _lib.ptr(out['orient']), (1 if self.flag_traj_from_cam else 0) | (2 if skin_early else 0), _lib.ptr(ws), st))
        if not skin_early:
            skin()
        # with flag_init_cam_all_frames this pass is only there for the world poses the cameras are initialised from; whoever needs the 'init'
        # outputs gets them from the second pass (init_forward), or from the first stage's last evaluation
        self._run(packed, self._forward_only_desc(poses_only=self.flag_init_cam_all_frames or not init_forward))
        if self.flag_init_cam_all_frames:
            sb = packed.struct()
            _lib.check(L.glamr_init_cam_all_frames(ctypes.byref(sb), st))
            # the 'init' forward pass with the new cameras (:246) only produces outputs (projections, camera-relative orientation, loss
            # values); a caller that runs the schedule right away overwrites every one of them with the first stage's last evaluation
            if init_forward:
                self._run(packed, self._forward_only_desc())
        packed.person_arrays = pa_t
        packed.exists = rin.exists
        packed.keepalive = (rin, ws, out)
        datas = [dict(m, meta={'algo': 'global_recon', 'num_fr': m['seq_len']}, _pending=True) for m in rin.meta]
        self.timings.update(priors=0.0, host_init=0.0, lbs_pack_init=time.time() - t1)
        return datas, packed

    def init_data_batch(self, in_dicts, latents=None, init_forward=True):
        """init_data (:76-248) for a batch of host dictionaries: stage_inputs + init_resident."""
        if self.cam_fix_frames != [(0, None)]:
            return self.init_data_batch_host(in_dicts, latents)
        return self.init_resident(self.stage_inputs(in_dicts, latents), init_forward=init_forward)

    _FETCH = ('fr_start', 'fr_end', 'vis', 'kp_2d', 'kp_score', 'cam_K', 'traj_local_pred', 'orient_cam', 'base_orient', 'base_trans', 'person2cam',
              'cam_pose', 'params', 'orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'losses')

    def _fetch_async(self, packed, stream=None):
        """Device -> pinned host copies of everything the output dictionaries are cut from, enqueued on `stream` (default: the current
        one).  Returns (host arrays, event); the arrays are valid once the event has completed."""
        src = {k: packed.t[k] for k in self._FETCH}
        src.update({'pa_' + k: v for k, v in packed.person_arrays.items() if k not in ('nets_pose', 'nets_vis')})
        if 'rel_transform_cam' in packed.t:
            src['rel'] = packed.t['rel_transform_cam']
        if 'world_res' in packed.t and (packed.has_world_dxy or packed.world_res_listed):      # (a 'vec' run has the array for its extension's launches: not reported, not copied)
            src['world_res'] = packed.t['world_res']
        if packed.heading_vec:
            src['heading_vec'] = packed.heading_vec_arrays()
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        host = {}
        rin = packed.keepalive[0] if packed.keepalive else None
        with ctx:
            for k, v in src.items():
                hbuf = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)      # (one pinned slab per batch was measured slower: 3 ms per allocation)
                hbuf.copy_(v, non_blocking=True)
                host[k] = hbuf
            hv = None
            if rin is not None and rin.verdict is not None:
                # the wire-format verdict rides along (a blocking .cpu() of its own was 7 ms of host stall per batch: tools/host_profile.py)
                torch.cuda.current_stream(self.device).wait_event(rin.verdict_ready)
                hv = torch.empty(rin.verdict.shape, dtype=rin.verdict.dtype, pin_memory=True)
                hv.copy_(rin.verdict, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            if hv is not None:
                rin.verdict_host = (hv, ev)
        return host, ev

    def _materialise(self, datas, packed, stage_vars, fetched=None):
        """Builds the reference-style output dictionaries (numpy) from the device arrays: ONE device->host copy per array; per person, plain
        slices of the batch arrays right away and the converted ones (float64 masks / keypoints, 4 x 4 matrices, frame tables) on access."""
        P, l = packed.P, packed.layout
        if fetched is None:
            fetched = self._fetch_async(packed)
        host, ev = fetched
        ev.synchronize()
        h = {k: v.numpy() for k, v in host.items()}
        self.last_losses = h['losses']
        rel = h.get('rel')
        eye_row = np.array([0, 0, 0, 1], np.float32)

        def to44(m12):
            out = np.zeros(m12.shape[:-1] + (4, 4), np.float32)
            out[..., :3, :] = m12.reshape(m12.shape[:-1] + (3, 4))
            out[..., 3, :] = eye_row
            return out
        fr_start, fr_end = h['fr_start'].tolist(), h['fr_end'].tolist()
        wd = 'world_dheading' in stage_vars
        # the world-frame residuals: world_dxy once created, the residual tensors once a stage listed world_res or one of their terms
        world_keys = tuple(k for k in packing.WORLD_KEYS if 'world_res' in h and (packed.has_world_dxy if k == 'world_dxy' else packed.world_res_listed))
        person_keys = _PERSON_KEYS + (('world_dheading',) if wd else ()) + world_keys

        def person_factory(k, pi, si, Ts):
            fs, fe = fr_start[k], fr_end[k]
            n = fe - fs
            frame = lambda name: (lambda: h[name][k, :Ts])
            var = lambda name: (lambda: packing.person_view(h['params'][si], l, pi, name)[packing.var_rows(name, n, Ts)])
            cut = {name: var(name) for name in packing.PERSON_VARS}
            cut.update({key: (lambda key=key: h['world_res'][k, :Ts, packing.WORLD_KEYS[key]]) for key in world_keys})
            if 'heading_vec' in h:      # heading_type 'vec': (2,) and (len - 1, 2)
                cut.update({'traj_local_heading': lambda: h['heading_vec'][k, 0], 'traj_local_dheading': lambda: h['heading_vec'][k, 1:n]})
            cut.update({
                'smpl_pose': frame('pa_smpl_pose'), 'smpl_beta': frame('pa_smpl_beta'), 'smpl_orient_cam': frame('orient_cam'), 'root_trans_cam': frame('pa_trans_cam'),
                'cam_K': lambda: h['cam_K'][k, :Ts].reshape(Ts, 3, 3), 'traj_local_pred': lambda: h['traj_local_pred'][k, :n],
                'smpl_orient_world_base': frame('base_orient'), 'root_trans_world_base': frame('base_trans'), 'smpl_orient_world': frame('orient_world'),
                'root_trans_world': frame('trans_world'), 'kp_2d_pred': frame('kp_2d_pred'), 'smpl_orient_cam_in_world': frame('orient_cam_in_world'),
                'visible': lambda: h['vis'][k, :Ts].astype(np.float64), 'visible_orig': lambda: h['pa_visible_orig'][k, :Ts].astype(np.float64),
                'frames': lambda: np.arange(Ts), 'vis_frames': lambda: h['vis'][k, :Ts] == 1, 'invis_frames': lambda: h['vis'][k, :Ts] == 0,
                'frame2ind': lambda: {f: f for f in range(Ts)},
                'kp_2d': lambda: h['kp_2d'][k, :Ts].astype(np.float64), 'kp_2d_aligned': lambda: h['kp_2d'][k, :Ts].astype(np.float64),
                'kp_2d_score': lambda: h['kp_score'][k, :Ts].astype(np.float64), 'person2cam': lambda: to44(h['person2cam'][k, :Ts]),
            })

            def exist_frames():
                e = np.zeros(Ts, bool)
                e[fs:fe] = True
                return e
            cut['exist_frames'] = exist_frames
            return lambda key: cut[key]()
        fixed_cam = bool(self.specs.get('flag_fixed_cam', False))
        has_cam = 'cam' in stage_vars
        scene_keys = ('cam_pose', 'cam_pose_inv', 'fr_num_persons', 'cam_inv_rot_residual', 'rel_transform_cam', 'cam_inv_trans_residual') + \
            ((('cam_rot_6d_fix', 'cam_trans_fix') if fixed_cam else ('cam_rot_6d', 'cam_trans')) if has_cam else ())
        h_vis, h_params, h_cam = h['vis'], h['params'], h['cam_pose']
        person_ids = packed.person_ids

        def scene_factory(si, Ts):
            """Everything of a scene that is cut from the batch arrays, built when the first such key is read."""
            prm = h_params[si]
            cam12 = h_cam[si, :Ts]
            n_p = len(person_ids[si])

            def num_persons():
                return sum((h_vis[si * P + pi, :Ts] == 1).astype(np.int64) for pi in range(n_p))

            def rel_dict():
                if rel is None:
                    return {}
                return {(i, j): to44(rel[si, i, j, :Ts]) for i in range(n_p) for j in range(n_p) if i != j}
            # (`empty` is only worked out for the variable whose rows it is)
            var = lambda name: (lambda: packing.scene_view(prm, l, name)[packing.var_rows(
                name, Ts=Ts, empty=np.where(num_persons() == 0)[0] if name == 'cam_inv_rot_residual' else None)])
            cut = {name: var(name) for name in packing.SCENE_VARS}
            cut.update({'cam_pose': lambda: to44(cam12), 'cam_pose_inv': lambda: nt.invert_transform(to44(cam12)), 'fr_num_persons': num_persons,
                        'rel_transform_cam': rel_dict})
            return lambda key: cut[key]()
        for si, d in enumerate(datas):
            Ts = d['seq_len']
            persons = {}
            for pi, idx in enumerate(person_ids[si]):
                k = si * P + pi
                fs, fe = fr_start[k], fr_end[k]
                eager = {'fr_start': fs, 'fr_end': fe, 'exist_len': fe - fs, 'max_len': Ts, 'scale': None, 'infilled': True, 'traj_predicted': True}

                def factory(key, args=(k, pi, si, Ts), cache=[None]):
                    if cache[0] is None:
                        cache[0] = person_factory(*args)
                    return cache[0](key)
                persons[idx] = LazyDict(eager, factory=factory, factory_keys=person_keys)

            def sfactory(key, args=(si, Ts), cache=[None]):
                if cache[0] is None:
                    cache[0] = scene_factory(*args)
                return cache[0](key)
            d.pop('_pending', None)
            d['person_data'] = persons
            datas[si] = LazyDict(d, factory=sfactory, factory_keys=scene_keys)
        return datas

    def _schedule_overwrites_init(self):
        """True when the configured schedule has at least one stage: its last evaluation rewrites all outputs of the 'init' forward pass."""
        return len(self.opt_stage_specs) > 0

    def _forward_only_desc(self, poses_only=False):
        first = next(iter(self.opt_stage_specs.values()))
        if self.latent_mode:      # (the latent regularisers are run_latent_schedule's, never the stage kernel's; the 'init' forward evaluates no loss)
            first = dict(first, loss_cfg=packing.split_latent_regs(first['loss_cfg'])[0])
        sd = packing.stage_desc(first, self.specs, has_world_dheading=False, niters=0)
        sd.var_mask = 0
        sd.flags &= ~packing.FLAG_CAM_FROM_PERSON           # stage 'init' keeps the initial camera (:473)
        if poses_only:
            sd.flags |= packing.FLAG_POSES_ONLY             # only orient_world / trans_world are wanted (the pass before init_cam_pose(all_frames))
        return sd

    def _run(self, packed, sd):
        ext = None
        if packed.heading_vec:      # (a forward pass of a heading_type 'vec' batch: the extension's instances, without a term)
            ext, _ = packing.world_ext(stepwise.world_stage(packed, None), packed, niters=int(sd.niters), heading={})
        stepwise.run_stage(packed, sd, False, ext=ext)
        return packed.last_ws

    @staticmethod
    def launch_ms(ws):
        """Duration of the stage launch that used workspace `ws`, from the kernel's own clock (blocks until it has finished)."""
        ns = ctypes.c_double()
        _lib.check(_lib.lib().glamr_grecon_last_launch_ns(_lib.ptr(ws), ctypes.byref(ns)))
        return ns.value * 1e-6

    def run_schedule(self, packed, max_iters=None, has_wd=False):
        """The staged optimisation (:250-262) of an initialised batch: one kernel launch per stage, asynchronous on the current
        stream.  `max_iters` caps the iterations of every stage (tests); None = the configured schedule.  `has_wd`: the scenes already
        carry a world heading offset (a continued optimisation, :459-465 applies it whenever the variable exists)."""
        if self.flag_opt_vis_local_rot:
            return self._run_schedule_masked(packed, max_iters, has_wd)
        events = []
        want_hist = (self.log is not None or self.keep_loss_history) and not torch.cuda.is_current_stream_capturing()
        for stage, spec in self.opt_stage_specs.items():
            sd = packing.stage_desc(spec, self.specs, has_world_dheading=has_wd, niters=stepwise.stage_iters(spec, max_iters))
            if want_hist and sd.niters > 0:
                packed.t['loss_history'] = torch.zeros((packed.S, int(sd.niters), len(packing.LOSS_IDS)), dtype=torch.float32, device=self.device)
            world = stepwise.world_stage(packed, self._world_cfg.get(stage))
            if packed.heading_vec != self.heading_vec:
                raise ValueError("the batch was packed with heading_type = %r, the optimiser has %r" % tuple('vec' if v else 'scalar' for v in (packed.heading_vec, self.heading_vec)))
            heading = self._heading_cfg[stage] if self.heading_vec else None
            if world is None and heading is None:
                events.append(self._run(packed, sd))               # the launch's workspace: its header carries the kernel's own clock stamps
                whist = hhist = None
            else:
                if packed.t.get('frozen') is not None:
                    raise NotImplementedError("world_dxy / world_res / traj_rot_res / traj_trans_res (the world-frame residuals) or heading_type = 'vec' on a person-sharded batch")
                ext, keep = packing.world_ext(world, packed, niters=int(sd.niters), want_hist='loss_history' in packed.t, heading=heading)
                stepwise.run_stage(packed, sd, False, ext=ext)
                events.append(packed.last_ws)
                if world is not None:
                    stepwise.end_world_stage(packed, world, keep)
                packed.heading_vec_losses = keep.get('hv_losses')
                whist, hhist = keep.get('loss_history') if world is not None else None, keep.get('hv_loss_history')
            if 'loss_history' in packed.t:
                self._report_stage(packed, stage, spec, packed.t.pop('loss_history'), events[-1], whist, (heading or world or {}).get('loss_order'), hhist)
            has_wd = stepwise.end_stage(packed, spec, has_wd)
        packed.has_world_dheading = has_wd
        packed.stage_ws = events
        return packed

    def _report_stage(self, packed, stage, spec, hist, ws, world_hist=None, loss_order=None, heading_hist=None):
        """write_logs (:646-659) for every iteration of a finished stage launch: `cfg id - sequence - stage | it/niters | TE: .. ETA: .. | LR: .. |
        term: value | ...` with the UNWEIGHTED values (loss_uw_dict, :564) of the stage's terms in the order of its loss_cfg.  The time per
        iteration is the launch's duration divided by its iterations."""
        import datetime
        h = hist.cpu().numpy()                                          # (waits for the launch)
        self.loss_history[stage] = h
        wh = world_hist.cpu().numpy() if world_hist is not None else None
        if wh is not None:
            self.world_loss_history[stage] = wh
        hh = heading_hist.cpu().numpy() if heading_hist is not None else None
        if hh is not None:
            self.heading_vec_loss_history[stage] = hh
        if self.log is None:
            return
        n_it = h.shape[1]
        it_secs = self.launch_ms(ws) * 1e-3 / max(1, n_it)
        hms = lambda secs: str(datetime.timedelta(seconds=round(secs)))
        hv_terms = packing.HEADING_VEC_TERMS if hh is not None else {}      # (a 'vec' run: both of the variable's terms are the extension's)
        names = [n for n in (loss_order or spec['loss_cfg']) if n in hv_terms or n in packing.LOSS_IDS or (wh is not None and n in packing.WORLD_TERMS)]
        value = lambda si, it, n: hh[si, it, hv_terms[n]] if n in hv_terms else h[si, it, packing.LOSS_IDS[n]] if n in packing.LOSS_IDS else wh[si, it, packing.WORLD_TERMS[n]]
        for si in range(packed.S):
            head = '%s - %s - %s' % (self.cfg_id, packed.seq_names[si], stage)
            for it in range(n_it):
                loss_str = ' | '.join('%s: %7.3f' % (n, value(si, it, n)) for n in names)
                self.log.info('%s | %4d/%d | TE: %s ETA: %s | LR: %.0e | %s' % (head, it, n_it, hms(it_secs), hms(it_secs * (n_it - it - 1)), spec['opt_lr'], loss_str))

    def _run_schedule_masked(self, packed, max_iters, has_wd):
        """flag_opt_vis_local_rot: the schedule launch by launch (parallel.PersonShardedSchedule on ONE rank without collectives: a gradient launch
        and glamr_adam_step per iteration, ~0.4 ms each) with the gradient of `traj_local_rot` zeroed at the frames a person is not seen in.  No
        shipped config sets the flag; the one-launch-per-stage kernel is untouched by it."""
        from glamr_amd import parallel
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError('flag_opt_vis_local_rot runs launch by launch and cannot be captured into a step graph')
        if any(self.specs.get('flag_opt_cam_from_person_pose', False) and 'cam' not in spec['opt_variables'] for spec in self.opt_stage_specs.values()):
            raise NotImplementedError('flag_opt_vis_local_rot with a camera derived from the persons')
        S, P, T, l = packed.S, packed.P, packed.T, packed.layout
        vis = packed.t['vis'].view(S, P, T) > 0
        fr_start = packed.t['fr_start'].view(S, P).long()
        keep = torch.ones_like(packed.t['params'])
        t_idx = torch.arange(T, device=packed.device)
        s_idx = torch.arange(S, device=packed.device)[:, None].expand(S, T)
        for pi in range(P):
            # the residual of video frame t sits at row t - fr_start of the person's block (rows of frames before fr_start do not exist)
            e = t_idx[None, :] - fr_start[:, pi:pi + 1]                                        # (S, T)
            ok = (~vis[:, pi]) & (e >= 0)
            packing.person_view(keep, l, pi, 'traj_local_rot')[s_idx[ok], e[ok]] = 0.0         # (S, T, 6): all six numbers of the row

        def hook(packed_, stage, spec, grads):
            grads.mul_(keep)
        sched = parallel.PersonShardedSchedule(rank=0, world=1, grad_hook=hook, use_dist=False)
        sched.run(packed, self.opt_stage_specs, self.specs, max_iters=max_iters, has_wd=has_wd)
        packed.stage_ws = []
        return packed

    def optimize_resident(self, rin, max_iters=None):
        """HBM in, HBM out: init_data + the full schedule on a ResidentInputs batch.  Returns (datas, packed) with every result
        (optimised variables, world trajectories, projections, camera) in packed.t on the device; collect() brings them to the host."""
        self._refuse_extra_loss('optimize_resident')
        datas, packed = self.init_resident(rin, init_forward=self.latent_mode or not self._schedule_overwrites_init())
        if self.latent_mode:
            self.run_latent_schedule(rin, packed, max_iters)
        elif self._aux_on_device():
            aux_step_schedule.AuxStepSchedule(self, packed).run(max_iters)
        else:
            self.run_schedule(packed, max_iters)
        return datas, packed

    def capture_resident(self, rin, max_iters=None, stream=None, check=True):
        """optimize_resident(rin) as ONE replayable HIP graph: returns a ResidentGraph whose replay() enqueues the whole step (per-person
        preparation, priors, skinning, scene assembly, every optimisation stage: ~25 launches of this library, the priors' ~450 included) with a
        single launch on the host.  For callers that run the same batch geometry again and again on resident inputs whose CONTENT changes
        (a service loop; bench.py): a host whose driver calls are slow then no longer paces the GPU.  The step must have run once on this stream
        before (allocations, one-time attribute calls).  check=True replays once against a plain step with the same seed and requires the
        projections to agree bit for bit (RuntimeError otherwise).  Results live in graph.packed (collect() them after a replay)."""
        self._refuse_extra_loss('capture_resident')
        if self.latent_mode:
            raise NotImplementedError('the latent-optimisation schedule captures its own graph per iteration (run_latent_schedule); the whole step is not capturable')
        # the value checks of the wire format run once per batch, outside a capture (init_resident skips them while capturing): a batch whose
        # FIRST use is this capture is checked here -- the verdict surfaces in collect() / check_inputs() as usual
        self.value_checks(rin)
        if self.latent_source == 'philox' and rin.meps is None and rin.latent_seq_ids is None:
            self._latent_table(rin)                                   # (a batch staged under 'torch': its table is uploaded here, outside the capture)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if st == torch.cuda.default_stream(self.device):
            st = torch.cuda.Stream(device=self.device)               # the legacy default stream cannot be captured
            st.wait_stream(torch.cuda.default_stream(self.device))
        graph = torch.cuda.CUDAGraph()
        # (thread-local capture mode: a watchdog thread of a process group may query events while this thread captures)
        if self.pipeline_gate is None:
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                datas, packed = self.optimize_resident(rin, max_iters)
            rg = ResidentGraph(graph, datas, packed, st)
        else:
            # two graphs sharing one memory pool: everything up to and including the priors, and the rest; replay() records the gate's event between them
            tail = torch.cuda.CUDAGraph()
            prep_early = os.environ.get('GLAMR_GATE_PREP', 'early') != 'late'
            head = torch.cuda.CUDAGraph() if prep_early else None     # (three graphs then: preparation | priors | the rest)
            torch.cuda.synchronize(self.device)
            with torch.cuda.stream(st):
                first = head if head is not None else graph
                first.capture_begin(capture_error_mode='thread_local')

                def head_split():
                    head.capture_end()
                    graph.capture_begin(pool=head.pool(), capture_error_mode='thread_local')

                def split():
                    graph.capture_end()
                    tail.capture_begin(pool=first.pool(), capture_error_mode='thread_local')
                self._capture_split = split
                self._capture_head_split = head_split if head is not None else None
                try:
                    datas, packed = self.optimize_resident(rin, max_iters)
                except BaseException:
                    # leave the stream out of capture mode whatever happened: whichever of the graphs is capturing is ended and dropped
                    # (a stream stuck in a broken capture fails every later launch -- bench.py's fall-back to plain launches included)
                    for gph in (tail, graph, head):
                        try:
                            if gph is not None:
                                gph.capture_end()
                        except Exception:      # noqa: BLE001 -- not capturing / already invalidated
                            pass
                    raise
                finally:
                    self._capture_split = None
                    self._capture_head_split = None
                tail.capture_end()
            rg = ResidentGraph(graph, datas, packed, st, tail=tail, gate=self.pipeline_gate, head=head)
        philox = rin.latent_seed_word is not None and rin.meps is None and self.latent_source == 'philox'
        if philox:
            # the captured draw reads its seed from the batch's seed word: every replay first writes the model's CURRENT latent_seed there
            rg.before_replay = lambda: latent_rng.set_seed(rin.latent_seed_word, self.latent_seed)
        if check:
            torch.cuda.synchronize(self.device)
            with torch.random.fork_rng(devices=[self.device]):          # the caller's generators are left as they were
                seed = 20260926
                if not philox:                                          # ('philox': both sides write self.latent_seed to the seed word instead)
                    torch.manual_seed(seed)
                with torch.cuda.stream(st):
                    _, ref = self.optimize_resident(rin, max_iters)
                torch.cuda.synchronize(self.device)
                want = ref.t['kp_2d_pred'].clone()
                if not philox:
                    torch.manual_seed(seed)
                rg.replay()
                torch.cuda.synchronize(self.device)
            got = packed.t['kp_2d_pred']
            if not (bool(torch.isfinite(got).all()) and torch.equal(got, want)):
                raise RuntimeError('the replayed step does not reproduce the plain one (max |diff| %.3g)' % float((got - want).abs().max()))
        return rg

    @property
    def latent_mode(self):
        return self.flag_opt_motion_latent or self.flag_opt_traj_latent

    def run_latent_schedule(self, rin, packed, max_iters=None):
        """The staged optimisation in LATENT-OPTIMISATION mode (flag_opt_motion_latent / flag_opt_traj_latent): the priors run inside the Adam loop
        and the latent draws are parameters -- launch by launch, from the third iteration of a stage on as replays of one captured HIP graph
        (latent_schedule.LatentSchedule; GLAMR_LATENT_GRAPH=0: plain launches throughout; self.latent_graph_replays counts)."""
        from ..latent_schedule import LatentSchedule
        return LatentSchedule(self, rin, packed).run(max_iters)

    def collect(self, datas, packed, fetched=None):
        """Device arrays -> the reference's output dictionaries (numpy): one device->host copy per array.  Waits for this batch only."""
        rin = packed.keepalive[0] if packed.keepalive else None
        if datas and datas[0].get('_pending'):
            if fetched is None:
                fetched = self._fetch_async(packed)
            if rin is not None:
                self.check_inputs(rin)
            t0 = time.time()
            self._materialise(datas, packed, self._all_vars(), fetched)
        else:
            torch.cuda.synchronize(self.device)
            t0 = time.time()
            packed.unpack_into(datas, {'opt_variables': self._all_vars()} if self.opt_stage_specs else None, self.specs, as_torch=False)
            self.last_losses = packed.t['losses'].cpu().numpy()
        if self.latent_mode and packed.latents is not None and rin is not None:
            # the optimised draws, per person as the reference keeps them in pose_dict (:155-158)
            meps, teps = (x.detach().cpu().numpy() for x in packed.latents)
            for si, d in enumerate(datas):
                for pi, idx in enumerate(packed.person_ids[si]):
                    k = si * packed.P + pi
                    d['person_data'][idx]['motion_latent'] = meps[k, :num_windows(int(rin.lens[k]))].copy()
                    d['person_data'][idx]['traj_latent'] = teps[k][None].copy()
        if packed.aux_values:      # (AuxStepSchedule's values: read back here, never inside the schedule)
            self.aux_loss_history = aux_step_schedule.publish(self._aux_cfg, packed.aux_values)
        if self.kernel_ms is not None and packed.stage_ws:
            self.kernel_ms.extend(self.launch_ms(ws) for ws in packed.stage_ws)
        self.timings['unpack'] = time.time() - t0
        return datas

    def _all_vars(self):
        return sorted(set(v for s in self.opt_stage_specs.values() for v in s['opt_variables']))

    def optimize_stream(self, batches, latents=None, max_iters=None):
        """Host dictionaries in, host dictionaries out for a STREAM of batches (an iterable of lists of in_dicts): yields one list of
        result dictionaries per batch, in order.  Software pipeline on the host thread: while the device runs batch i (asynchronous
        launches on a compute stream), the host scatters and uploads batch i + 1 (copy stream, pinned staging) and cuts the output
        dictionaries of batch i - 1 from its device->host copies (copy stream, after that batch's own event -- never a device-wide wait)."""
        self._refuse_extra_loss('optimize_stream')
        return self._optimize_stream(batches, latents, max_iters)

    def _optimize_stream(self, batches, latents, max_iters):
        dev = self.device
        # consecutive batches alternate over two compute streams (the launch seams and tails of one batch are covered by the next, as in bench.py)
        if self._compute_streams is None:
            self._compute_streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        computes = self._compute_streams
        # Uploads and downloads share ONE third stream.  Not more: the runtime multiplexes HIP streams onto 4 hardware queues, and with a
        # separate upload stream (5 streams with the default one) two of them shared a queue -- a batch then started only when the previous one
        # had finished (tools/stream_timeline.py; raising GPU_MAX_HW_QUEUES to 8, three compute streams and the default stream as the uploader
        # were all measured slower, round 4).  Rounds 2-3 put a batch's upload on ITS OWN compute stream: there it queues behind the batch
        # before last, so every batch began with 7 ms of PCIe and nothing else (50.5 ms from batch to batch against 43.4 resident).  On the
        # copy stream the order of the enqueues is what matters: a download waits for its batch's event, and an upload enqueued behind it
        # waits too -- _stream_loop enqueues a batch's download only when the upload of the batch two later is already in the queue.
        if self._download_stream is None:
            self._download_stream = torch.cuda.Stream(device=dev)
        down = self._download_stream
        it = iter(batches)
        lat = iter(latents) if latents is not None else None
        turn = [0]
        # batches alternate between two streams: stagger them so that a batch's infiller runs beside the previous batch's stage (PipelineGate)
        own_gate = self.pipeline_gate is None and not self.latent_mode and coschedule_enabled()
        if own_gate:
            self.pipeline_gate = PipelineGate()
        # The interpreter's cyclic collector: a full collection walks every container object alive -- with torch imported, 30-45 ms -- and the
        # ~10 000 containers a batch of output dictionaries is made of trigger one every 5-6 batches (measured: every fifth yield 85-110 ms late,
        # tools/stream_yield_probe.py).  While the stream runs, everything alive at its start sits in the permanent generation (gc.freeze):
        # collections still run, over the objects created since.
        import gc
        # (a caller that keeps a frozen set of its own -- gc.get_freeze_count() > 0 -- manages the collector itself: gc.unfreeze() would release ITS set too)
        frozen = gc.isenabled() and gc.get_freeze_count() == 0
        if frozen:
            # (no gc.collect() first: a full collection at this point walks every object alive -- 67 ms with torch imported, tools/stream_profile.py,
            # at the head of every stream, before its first batch is even staged; whatever garbage is frozen along is collected after gc.unfreeze())
            gc.freeze()
        try:
            yield from self._stream_loop(it, lat, turn, computes, down, max_iters)
        finally:
            if frozen:
                gc.unfreeze()
            if own_gate:
                self.pipeline_gate = None

    def _stream_loop(self, it, lat, turn, computes, down, max_iters):
        """Host iteration k: enqueue batch k's device work -> scatter + upload batch k + 1 -> enqueue the download of batch k - 2 -> cut batch
        k - 2's dictionaries (the only wait: until that download has landed).  Three batches are in flight, so a batch's launches are queued
        BEFORE its compute stream comes free (the batch before last still runs there) and its inputs were uploaded a batch time earlier."""
        def stage(batch):
            with torch.cuda.stream(down):
                return self.stage_inputs(batch, next(lat) if lat is not None else None)

        def fetch(entry):
            datas, packed, done = entry
            down.wait_event(done)
            return datas, packed, self._fetch_async(packed, down)
        nxt = next(it, None)
        if nxt is None:
            return
        rin = stage(nxt)
        flight = []                                                     # batches whose download has not been enqueued yet, oldest first
        while rin is not None:
            compute = computes[turn[0] % len(computes)]
            turn[0] += 1
            compute.wait_event(rin.upload_done)
            with torch.cuda.stream(compute):
                datas, packed = self.optimize_resident(rin, max_iters)      # (optimize_stream has refused what it refuses)
                done = torch.cuda.Event()
                done.record()
            flight.append((datas, packed, done))
            nxt = next(it, None)
            rin = stage(nxt) if nxt is not None else None              # host work under the device's; the copy stream is idle now
            if len(flight) > 2:
                yield self.collect(*fetch(flight.pop(0)))              # (enqueued only now: a download waiting for its batch must not sit in front of that upload)
        while flight:
            yield self.collect(*fetch(flight.pop(0)))

    def optimize_batch(self, in_dicts, latents=None, max_iters=None):
        """Host dictionaries in, host dictionaries out (optimize() of the reference for a batch of independent sequences)."""
        if self.latent_mode:
            if self.cam_fix_frames != [(0, None)]:
                raise NotImplementedError('latent-optimisation mode with non-default cam_fix_frames')
            rin = self.stage_inputs(in_dicts, latents)
            datas, packed = self.optimize_resident(rin, max_iters)
            return self.collect(datas, packed)
        datas, packed = self.init_data_batch(in_dicts, latents, init_forward=not self._schedule_overwrites_init())
        t0 = time.time()
        self._run_schedule_or_extra(packed, max_iters)
        torch.cuda.synchronize(self.device)
        self.timings['optimise'] = time.time() - t0
        return self.collect(datas, packed)

    # -- reference entry points ---------------------------------------------------------------------------------------------------
    def init_data(self, in_dict, latents=None):
        datas, packed = self.init_data_batch([in_dict], None if latents is None else [latents])
        if datas[0].get('_pending'):
            self._materialise(datas, packed, [])
        return datas[0]

    def optimize(self, in_dict, continue_opt=False, latents=None, max_iters=None):
        if continue_opt:
            return self.continue_batch([in_dict], max_iters)[0]
        return self.optimize_batch([in_dict], None if latents is None else [latents], max_iters)[0]

    def continue_batch(self, datas, max_iters=None):
        """optimize(in_dict, continue_opt=True) (:572-573): `in_dict` is the dictionary a previous optimize() returned; the schedule
        runs again from its variables.  The inputs are not modified."""
        datas = [dict(d, person_data={i: dict(pd) for i, pd in d['person_data'].items()}) for d in datas]
        j_locals = []
        for d in datas:
            jl = {}
            for idx, pd in d['person_data'].items():
                pose = torch.as_tensor(np.asarray(pd['smpl_pose']), dtype=torch.float32, device=self.device)
                beta = torch.as_tensor(np.asarray(pd['smpl_beta']), dtype=torch.float32, device=self.device)
                z = torch.zeros(pose.shape[0], 3, device=self.device)
                with torch.no_grad():
                    jl[idx] = self.smpl(global_orient=z, body_pose=pose, betas=beta, root_trans=z, return_verts=False).joints.cpu()
            j_locals.append(jl)
        packed = packing.PackedScenes(datas, j_locals, self.device, self.cam_fix_frames, heading_vec=self.heading_vec)
        has_wd = any('world_dheading' in pd for d in datas for pd in d['person_data'].values())
        self._run_schedule_or_extra(packed, max_iters, has_wd=has_wd)
        return self.collect(datas, packed)
