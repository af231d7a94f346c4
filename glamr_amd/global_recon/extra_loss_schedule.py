"""Loss terms the stage kernel does not hold, launch by launch on the stepwise core: the term a caller writes in torch
on the world poses and the camera (GlobalReconOptimizer.extra_loss), the built-in `penetration` term of loss_cfg and the six terms of
packing.AUX_LOSS_IDS (AuxTerms, one kernel launch), each added to a stage's total the way a non-monitor term of loss_cfg is
(global_recon_model.py:533-545).  A TERM has `history` (the optimiser's attribute its values are published under), `value_shape` (of one scene's
record per iteration: () = a number), active(stage), evaluate(ctx) -> ((S,) + value_shape values to record, scalar contribution to the total or
None: nothing for autograd to differentiate) and publish(stage, hist) -> what is stored under history[stage].  A term that computes its own
adjoints (AuxTerms) adds those on variables straight into ctx.grads, the launch's gradient array, and hands the ones on trans_world / cam_pose
to ctx.add_adjoint: they join the autograd gradients before step 4.

Per iteration of a stage, one path whatever the terms: (1) the gradient launch (glamr_grecon_run_stage, one iteration with lr 0 and grads_out)
gives the stage kernel's gradient and reports the world poses and the camera at the parameters it was taken at; (2) the stage's active terms are
evaluated under torch autograd on one ExtraLossContext holding copies of those; (3) ONE backward() of the contributions' sum; (4)
glamr_grecon_cam_backward adds the gradient with respect to ctx.cam_pose to the camera variables of the launch's gradient array -- or, when the
camera is derived from the persons, to the residuals and to the pose gradients -- and glamr_grecon_pose_backward then takes the pose gradients
back to the trajectory variables; (5) one Adam step (torch.optim.Adam's arithmetic, fresh moments per stage).  Without an active term, or with
skip_term, (1) and (5) alone.  Plain launches throughout: a term is host Python, so nothing here is captured into a graph."""
import collections
import ctypes

import torch

from .. import _lib
from . import packing, stepwise


def check_supported(model_specs, what='extra_loss'):
    """The model flags `extra_loss` -- or the built-in penetration term, which runs on the same schedule -- cannot be combined with; raises
    ValueError naming the combination."""
    g = model_specs.get
    if g('flag_opt_motion_latent', False) or g('flag_opt_traj_latent', False):
        raise ValueError('%s together with the latent-optimisation mode (flag_opt_motion_latent / flag_opt_traj_latent) is not supported: '
                         'that mode runs a schedule of its own' % what)
    if g('flag_opt_vis_local_rot', False):
        raise ValueError('%s together with flag_opt_vis_local_rot is not supported: the gradient mask of that flag is not applied to the term' % what)
    if g('absolute_heading', False):
        raise ValueError('%s together with absolute_heading is not supported: glamr_grecon_pose_backward differentiates heading increments' % what)


def check_not_sharded(packed, what='extra_loss'):
    """A person-sharded run (frozen person slots, or a process group of several ranks) does not exchange the term's gradient: refused."""
    import torch.distributed as dist
    if packed.t.get('frozen') is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        raise ValueError('%s together with a person-sharded run is not supported: the term would only see this rank\'s persons' % what)


def aux_what(names):
    """How a refusal names the terms of packing.AUX_LOSS_IDS a schedule was asked for."""
    return 'the loss_cfg term%s %s' % ('' if len(names) == 1 else 's', ', '.join(sorted(names, key=packing.AUX_LOSS_IDS.get)))


class _Term:
    value_shape = ()

    def publish(self, stage, hist):
        return hist


class CallerTerm(_Term):
    """opt.extra_loss(ctx) -> (S,) tensor, one already weighted value per scene: recorded as it is, added to every stage's total."""
    history = 'extra_loss_history'

    def __init__(self, fn):
        self.fn = fn

    def active(self, stage):
        return True

    def evaluate(self, ctx):
        S, loss = ctx.exist.shape[0], self.fn(ctx)
        if not torch.is_tensor(loss) or tuple(loss.shape) != (S,):
            raise ValueError('extra_loss must return a tensor of shape (%d,): one value per scene' % S)
        if not loss.requires_grad:
            raise ValueError('extra_loss returned a value that does not depend on ctx.orient_world / ctx.trans_world / ctx.cam_pose (no gradient): '
                             'a term without a gradient would be a silent zero')
        return loss, loss.sum()


class PenetrationTerm(_Term):
    """The built-in `penetration` term (loss_func.py:274-290) of the stages opt._pen_cfg lists ({stage: weight, monitor_only}).
    `vis` is constant over a run: the (scene, frame) rows with at least two visible persons are found once, and every evaluation skins only the
    visible persons of those rows (SMPL with vertices, differentiable through glamr_smpl_backward_root), hands them to SDFLoss.frames and divides
    by the scene's length.  prepare=False: for a run that never evaluates the term (skip_term) -- no body pose is asked for."""
    history = 'penetration_history'

    def __init__(self, opt, packed, vis, pose, beta, prepare=True):
        self.cfg = opt._pen_cfg
        if not prepare:
            return
        if pose is None:
            raise RuntimeError('the penetration term needs the body pose of a batch initialised on the device (default cam_fix_frames, not a continued optimisation)')
        S, P, T = vis.shape
        self.smpl, self.sdf_loss, self.S = opt.smpl, opt.sdf_loss, S
        rows = vis.sum(1) >= 2                                                            # (S, T)
        self.s_idx, self.t_idx = rows.nonzero(as_tuple=True)                              # R rows, scene-major
        self.seen = vis[self.s_idx, :, self.t_idx].to(torch.uint8).contiguous()           # (R, P)
        self.r_of, self.p_of = self.seen.nonzero(as_tuple=True)                           # the N visible (row, person) pairs
        s, t = self.s_idx[self.r_of], self.t_idx[self.r_of]
        self.spt = (s, self.p_of, t)
        self.body_pose, self.betas = pose[s, self.p_of, t].contiguous(), beta[s, self.p_of, t].contiguous()
        self.inv_len = 1.0 / packed.t['seq_len'].view(S).to(torch.float32)                # loss_all /= max_fr (:278,289)

    def active(self, stage):
        return stage in self.cfg

    def __call__(self, ctx):
        """-> (S,) unweighted values, differentiable with respect to ctx.orient_world and ctx.trans_world."""
        orient, trans = ctx.orient_world, ctx.trans_world
        R, P = self.seen.shape
        if R == 0:
            return torch.zeros(self.S, dtype=torch.float32, device=orient.device)
        out = self.smpl(global_orient=orient[self.spt], body_pose=self.body_pose, betas=self.betas, root_trans=trans[self.spt], return_verts=True)
        verts = out.vertices.new_zeros((R, P) + tuple(out.vertices.shape[1:])).index_put((self.r_of, self.p_of), out.vertices)
        per_row = self.sdf_loss.frames(verts, self.seen)
        return torch.zeros(self.S, dtype=torch.float32, device=orient.device).index_add(0, self.s_idx, per_row) * self.inv_len

    def evaluate(self, ctx):
        cfg = self.cfg[ctx.stage]
        with torch.set_grad_enabled(not cfg['monitor_only']):
            value = self(ctx)
            return value, (cfg['weight'] * value.sum() if value.requires_grad else None)      # (None: monitor_only, or no row to look at)


class AuxTerms(_Term):
    """The terms of packing.AUX_LOSS_IDS of the stages opt._aux_cfg lists ({stage: {name: weight, monitor_only[,
    first_frame_weight]}}): ONE launch of glamr_grecon_aux_terms per iteration gives the six unweighted values and the weighted adjoints, at
    the params, trans_world and cam_pose the gradient launch left in the batch.  Nothing goes through autograd: the adjoints of the terms that
    live on variables (cam_rot_smoothness, cam_trans_smoothness, local_traj_dheading_reg) are added to ctx.grads by the kernel, those on
    trans_world / cam_pose go to ctx.add_adjoint.
    The cam_rot6d / cam_trans rows of params ARE the stage's variables when the kernel reads them: a stage's first gradient launch
    (grad_launch_desc(first=True)) sets them from cam_pose (grecon_algo.hpp: the `var_cam && !GLAMR_FLAG_KEEP_CAM_PARAMS` block) and writes them to
    the batch array, every later one keeps what Adam made of them; packing.check_aux has refused the two terms on these rows in a stage that
    does not optimise `cam`.
    root_trans_cam: person_arrays['trans_cam'] of a batch initialised on the device, the packed pd['root_trans_cam'] of host dictionaries.
    prepare=False: for a run that never evaluates the terms (skip_term)."""
    history = 'aux_loss_history'
    value_shape = (_lib.AUX_NUM_TERMS,)
    _ON_TRANS = (1 << packing.AUX_LOSS_IDS['traj_trans_smoothness']) | (1 << packing.AUX_LOSS_IDS['cam_traj_trans'])
    _ON_CAM = (1 << packing.AUX_LOSS_IDS['cam_depth_smoothness']) | (1 << packing.AUX_LOSS_IDS['cam_traj_trans'])

    def __init__(self, opt, packed, prepare=True):
        self.cfg, self.packed = opt._aux_cfg, packed
        if not prepare:
            return
        self.desc = {stage: packing.aux_desc(c) for stage, c in self.cfg.items()}
        pa = packed.person_arrays
        self.root_trans_cam = pa['trans_cam'] if pa is not None and pa.get('trans_cam') is not None else packed.root_trans_cam
        if self.root_trans_cam is None and any('cam_traj_trans' in c for c in self.cfg.values()):
            raise RuntimeError('cam_traj_trans needs root_trans_cam of every person (person_data[...][\'root_trans_cam\'])')
        self._ws = torch.empty(max(_lib.lib().glamr_grecon_aux_terms_workspace_bytes(packed.S, packed.P, packed.T), 4), dtype=torch.uint8, device=packed.device)

    def active(self, stage):
        return stage in self.cfg

    def evaluate(self, ctx):
        packed, ad, sd = self.packed, self.desc[ctx.stage], ctx.stage_desc
        S, P, T = packed.S, packed.P, packed.T
        live = ad.loss_mask & ~ad.monitor_mask
        cam_constant = not (sd.var_mask & packing.VAR_BITS['cam']) and not (sd.flags & packing.FLAG_CAM_FROM_PERSON)
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=packed.device)
        g_trans = zeros(S * P, T, 3) if live & self._ON_TRANS else None
        g_cam = zeros(S, T, 12) if live & self._ON_CAM and not cam_constant else None
        values = torch.empty((S, _lib.AUX_NUM_TERMS), dtype=torch.float32, device=packed.device)
        sb = packed.struct()
        _lib.check(_lib.lib().glamr_grecon_aux_terms(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), _lib.ptr(self.root_trans_cam), _lib.ptr(values),
                                                     _lib.ptr(g_trans), _lib.ptr(g_cam), _lib.ptr(ctx.grads), 1, _lib.ptr(self._ws), _lib.current_stream()))
        ctx.add_adjoint(trans_world=g_trans, cam_pose=g_cam)
        return values, None

    def publish(self, stage, hist):
        return {name: hist[:, :, i] for name, i in packing.AUX_LOSS_IDS.items() if name in self.cfg[stage]}


class ExtraLossContext:
    """What the callback is given.  orient_world / trans_world (S, P, T, 3): leaf tensors that require grad, copies of the poses the gradient
    launch reported (axis-angle / metres, by video frame; zero on frames and slots that do not exist).  exist / vis (S, P, T) bool.
    smpl_pose (S, P, T, 69), smpl_beta (S, P, T, 10): the body pose and shape of every frame (constants), or None when the batch was not
    initialised on the device.  joints() (S, P, T, 26, 3) and vertices() (S, P, T, V, 3): the body model at the world poses, differentiable
    with respect to them (glamr_smpl_backward_root), computed when called.
    cam_pose (S, T, 3, 4): world-to-camera, a copy of what the gradient launch reported; a leaf that requires grad when the stage optimises the
    camera or derives it from the persons (with a fixed camera every frame holds row 0's), a plain tensor when the camera is a constant of the
    stage.  cam_K (S, P, T, 3, 3), kp_2d (S, P, T, 26, 2), kp_score (S, P, T, 26): constants.  project(points): (S, P, T, N, 3) world points
    -> (S, P, T, N, 2) pixels, the reference's perspective_projection(transform_trans(cam_pose, x), cam_K), differentiable with respect to the
    points and cam_pose: project(joints()) is the reference's kp_2d_pred.
    For a term that computes its own adjoints: stage_desc (the gradient launch's descriptor), grads ((S, scene_stride), the launch's gradient
    array: adjoints on variables are added in place) and add_adjoint(trans_world=, cam_pose=): adjoints shaped like trans_world / cam_pose (any
    view of the same elements) that join the autograd gradients of the iteration."""

    def __init__(self, smpl, stage, iteration, seq_names, orient_world, trans_world, exist, vis, smpl_pose, smpl_beta, cam_pose=None, cam_K=None,
                 kp_2d=None, kp_score=None, stage_desc=None, grads=None):
        self._smpl = smpl
        self.stage_desc, self.grads, self.adjoints = stage_desc, grads, {}
        self.stage, self.iteration, self.seq_names = stage, iteration, seq_names
        self.orient_world, self.trans_world, self.exist, self.vis = orient_world, trans_world, exist, vis
        self.smpl_pose, self.smpl_beta = smpl_pose, smpl_beta
        self._cam, self._cam_live = cam_pose, False      # (copied at the first access: a term on the poses alone does not pay for it)
        self.cam_K, self.kp_2d, self.kp_score = cam_K, kp_2d, kp_score

    @property
    def cam_pose(self):
        if not self._cam_live and self._cam is not None:
            src, grad = self._cam if isinstance(self._cam, tuple) else (self._cam, None)
            self._cam = src if grad is None else src.clone().requires_grad_(grad)
            self._cam_live = True
        return self._cam

    def add_adjoint(self, **adjoints):
        for k, v in adjoints.items():
            if v is not None:
                self.adjoints[k] = v if k not in self.adjoints else self.adjoints[k] + v.view_as(self.adjoints[k])

    def cam_grad(self):
        """The gradient the callback left on cam_pose, or None (never looked at, a constant, or unused)."""
        return self._cam.grad if self._cam_live and self._cam is not None else None

    def project(self, points):
        cam = self.cam_pose[:, None, :, None]                                              # (S, 1, T, 1, 3, 4)
        x = torch.matmul(cam[..., :3], points.unsqueeze(-1)).squeeze(-1) + cam[..., 3]     # transform_trans (torch_transform.py:257-262)
        h = torch.matmul(self.cam_K.unsqueeze(3), x.unsqueeze(-1)).squeeze(-1)             # perspective_projection (geometry.py:23-25)
        return h[..., :2] / (h[..., 2:] + 1e-8)

    def _body(self, verts):
        if self.smpl_pose is None:
            raise RuntimeError('extra_loss: joints() / vertices() need the body pose of a batch initialised on the device (default cam_fix_frames, not a continued optimisation)')
        S, P, T = self.exist.shape
        out = self._smpl(global_orient=self.orient_world.reshape(-1, 3), body_pose=self.smpl_pose.reshape(-1, 69), betas=self.smpl_beta.reshape(-1, 10),
                         root_trans=self.trans_world.reshape(-1, 3), return_verts=verts)
        return (out.vertices if verts else out.joints).view(S, P, T, -1, 3)

    def joints(self):
        return self._body(False)

    def vertices(self):
        return self._body(True)


# What is fixed for the iterations of a stage: its name and the spec its launches get, whether the scenes carry a world heading offset, the stage's
# active terms each with its history (n_scenes, n_iterations) [(term, hist)], the moments and the optimiser (fresh per stage).
_Stage = collections.namedtuple('_Stage', 'name spec has_wd terms m v adam')


class ExtraLossSchedule:
    """run_schedule with the run's terms added to the totals of the stages they are active in: opt.extra_loss (every stage) and / or the built-in
    penetration term (the stages whose loss_cfg listed it).  The attributes set in __init__ are all that lives longer than an iteration; `opt`
    None: pose_backward / cam_backward alone."""

    def __init__(self, opt, packed, skip_term=False):
        # skip_term: the same launches and Adam steps without steps 2-4 (what a zero term must reproduce; the timing tool's baseline)
        self.opt, self.packed, self.skip_term = opt, packed, skip_term
        S, P, T, t, L = packed.S, packed.P, packed.T, packed.t, _lib.lib()
        self._ws = torch.empty(L.glamr_grecon_pose_backward_workspace_bytes(S, P, T), dtype=torch.uint8, device=packed.device)
        self._cam_ws = torch.empty(L.glamr_grecon_cam_backward_workspace_bytes(S, P, T), dtype=torch.uint8, device=packed.device)
        if opt is None:
            return
        t_idx = torch.arange(T, device=packed.device)
        fs, fe = t['fr_start'].view(S, P, 1), t['fr_end'].view(S, P, 1)
        slot_ok = torch.arange(P, device=packed.device).view(1, P, 1) < t['n_persons'].view(S, 1, 1)
        pa = packed.person_arrays
        # what every iteration's ExtraLossContext holds unchanged (its constructor's keywords)
        self.const = dict(seq_names=packed.seq_names, exist=(t_idx >= fs) & (t_idx < fe) & (t_idx < t['seq_len'].view(S, 1, 1)) & slot_ok,
                          vis=(t['vis'].view(S, P, T) > 0) & slot_ok, smpl_pose=pa['smpl_pose'].view(S, P, T, 69) if pa is not None else None,
                          smpl_beta=pa['smpl_beta'].view(S, P, T, 10) if pa is not None else None, cam_K=t['cam_K'].view(S, P, T, 3, 3),
                          kp_2d=t['kp_2d'].view(S, P, T, -1, 2), kp_score=t['kp_score'].view(S, P, T, -1))
        self.params = t['params']

    def pose_backward(self, sd, g_orient, g_trans, grads, accumulate=1):
        """glamr_grecon_pose_backward on the packed batch (current stream)."""
        sb = self.packed.struct()
        _lib.check(_lib.lib().glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(g_orient), _lib.ptr(g_trans), _lib.ptr(grads), int(accumulate),
                                                         _lib.ptr(self._ws), _lib.current_stream()))

    def cam_backward(self, sd, g_cam, grads, g_orient, g_trans, accumulate=1):
        """glamr_grecon_cam_backward on the packed batch (current stream); g_orient / g_trans are added into (camera derived from the persons)."""
        sb = self.packed.struct()
        _lib.check(_lib.lib().glamr_grecon_cam_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(g_cam), _lib.ptr(grads), int(accumulate), _lib.ptr(g_orient),
                                                        _lib.ptr(g_trans), _lib.ptr(self._cam_ws), _lib.current_stream()))

    def iteration(self, st, it):
        """One Adam iteration of stage `st`: the stage kernel's gradient, the active terms' added to it, the step, the terms' values recorded."""
        opt, packed = self.opt, self.packed
        sd = stepwise.grad_launch_desc(st.spec, opt.specs, st.has_wd, first=(it == 0))
        grads = stepwise.run_stage(packed, sd, True)                                                  # 1.
        values = []
        if st.terms and not self.skip_term:
            values = self._add_terms(st, it, sd, grads)                                               # 2. - 4.
            if opt.extra_loss_grad_hook is not None:
                opt.extra_loss_grad_hook(st.name, it, grads)        # (the complete gradient of the iteration, before the update)
        st.adam.step(self.params, st.m, st.v, grads)                                                  # 5.
        for (_, hist), value in zip(st.terms, values):
            hist[:, it] = value

    def _add_terms(self, st, it, sd, grads):
        """Steps 2-4: the stage's terms on copies of what the launch reported, their total's gradient into `grads`; returns the terms' values."""
        packed, opt_vars = self.packed, st.spec['opt_variables']
        S, P, T = packed.S, packed.P, packed.T
        orient = packed.t['orient_world'].view(S, P, T, 3).clone().requires_grad_(True)
        trans = packed.t['trans_world'].view(S, P, T, 3).clone().requires_grad_(True)
        cam_derived = 'cam' not in opt_vars and bool(sd.flags & packing.FLAG_CAM_FROM_PERSON)
        # (source, requires grad): a leaf in the three live modes, a plain tensor when the camera is a constant of the stage
        cam = (packed.t['cam_pose'].view(S, T, 3, 4), 'cam' in opt_vars or cam_derived)
        ctx = ExtraLossContext(self.opt.smpl, st.name, it, orient_world=orient, trans_world=trans, cam_pose=cam, stage_desc=sd, grads=grads, **self.const)
        values, total = [], None
        with torch.enable_grad():
            for term, _ in st.terms:                                                                  # 2.
                value, part = term.evaluate(ctx)
                values.append(value.detach())
                if part is not None:
                    total = part if total is None else total + part
            if total is None and not ctx.adjoints:              # (monitor-only terms alone, or no row for the built-in term to see)
                return values
            if total is not None:
                total.backward()                                                                      # 3.
        g_cam = ctx.cam_grad()
        if total is not None and orient.grad is None and trans.grad is None and g_cam is None:
            raise ValueError('extra_loss returned a value that does not depend on ctx.orient_world / ctx.trans_world / ctx.cam_pose (grad is None)')
        # the stage kernel applies the world heading offset as soon as the stage optimises it (the variable exists from then on, :459-465)
        if 'world_dheading' in opt_vars:
            sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
        g_o = None if orient.grad is None else orient.grad.contiguous()
        g_t = None if trans.grad is None else trans.grad.contiguous()
        if 'trans_world' in ctx.adjoints:                       # (a term's own adjoints: added to autograd's)
            a = ctx.adjoints['trans_world'].view(S, P, T, 3)
            g_t = a if g_t is None else g_t + a
        if 'cam_pose' in ctx.adjoints:
            a = ctx.adjoints['cam_pose'].view(S, T, 3, 4)
            g_cam = a if g_cam is None else g_cam + a
        if g_cam is not None:                                                                         # 4. the camera first: it may add to the pose gradients
            if cam_derived:
                g_o = torch.zeros_like(orient) if g_o is None else g_o
                g_t = torch.zeros_like(trans) if g_t is None else g_t
            self.cam_backward(sd, g_cam.contiguous(), grads, g_o if cam_derived else None, g_t if cam_derived else None, accumulate=1)
        if g_o is not None or g_t is not None:
            self.pose_backward(sd, g_o, g_t, grads, accumulate=1)
        return values

    def run(self, max_iters=None, has_wd=False):
        opt, packed, c = self.opt, self.packed, self.const
        what = opt._off_kernel_term()      # (its combination with the model's flags was checked where the term was set: the optimiser's __init__ / extra_loss)
        if what is None:
            raise ValueError('ExtraLossSchedule needs GlobalReconOptimizer.extra_loss, a penetration term or a term of packing.AUX_LOSS_IDS in loss_cfg')
        check_not_sharded(packed, what)
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError('%s runs launch by launch with host Python in every iteration and cannot be captured into a graph' % what)
        # the run's terms, the caller's first: the order their contributions are summed in
        terms = [CallerTerm(opt.extra_loss)] if opt.extra_loss is not None else []
        if opt._pen_cfg:
            terms.append(PenetrationTerm(opt, packed, c['vis'], c['smpl_pose'], c['smpl_beta'], prepare=not self.skip_term))
        if opt._aux_cfg:
            terms.append(AuxTerms(opt, packed, prepare=not self.skip_term))
        opt.extra_loss_history = {}
        for term in terms:
            setattr(opt, term.history, {})
        for stage, spec in opt.opt_stage_specs.items():
            n = stepwise.stage_iters(spec, max_iters)
            st = _Stage(stage, spec, has_wd, [(term, torch.zeros((packed.S, n) + term.value_shape, dtype=torch.float32, device=packed.device)) for term in terms if term.active(stage)],
                        torch.zeros_like(self.params), torch.zeros_like(self.params), stepwise.IndexedAdam(spec['opt_lr'], n, packed.device))
            for it in range(n):
                self.iteration(st, it)
            for term, hist in st.terms:
                getattr(opt, term.history)[stage] = term.publish(stage, hist.cpu().numpy())
            has_wd = stepwise.end_stage(packed, spec, has_wd)
        packed.has_world_dheading = has_wd
        packed.stage_ws = []
        return packed
