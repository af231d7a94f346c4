"""Caller-defined loss terms on the world poses and the camera (GlobalReconOptimizer.extra_loss): the staged optimisation launch by launch
on the stepwise core, with a term the caller writes in torch added to every stage's total the way a non-monitor term of loss_cfg is
(global_recon_model.py:533-545) -- what three lines in the reference's loss_func_dict do.

Per iteration of a stage: (1) the gradient launch (glamr_grecon_run_stage, one iteration with lr 0 and grads_out) gives the built-in terms'
gradient and reports the world poses at the parameters it was taken at; (2) the callback runs under torch autograd on copies of those poses;
(3) loss.sum().backward(); (4) glamr_grecon_cam_backward adds the gradient with respect to ctx.cam_pose to the camera variables of the launch's
gradient array -- or, when the camera is derived from the persons, to the residuals and to the pose gradients -- and glamr_grecon_pose_backward
then takes the pose gradients back to the trajectory variables; (5) one Adam step (torch.optim.Adam's arithmetic, fresh moments per stage).  Plain launches throughout: the
callback is user Python, so nothing here is captured into a graph."""
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


class PenetrationTerm:
    """The built-in `penetration` term (loss_func.py:274-290) on the launch-by-launch schedule.  `vis` is constant over a run: the
    (scene, frame) rows with at least two visible persons are found once, and every iteration skins only the visible persons of those rows
    (SMPL with vertices, differentiable through glamr_smpl_backward_root), hands them to SDFLoss.frames and divides by the scene's length."""

    def __init__(self, opt, packed, vis, pose, beta):
        if pose is None:
            raise RuntimeError('the penetration term needs the body pose of a batch initialised on the device (default cam_fix_frames, not a continued optimisation)')
        S, P, T = vis.shape
        self.smpl, self.sdf_loss, self.S = opt.smpl, opt.sdf_loss, S
        rows = vis.sum(1) >= 2                                                            # (S, T)
        self.s_idx, self.t_idx = rows.nonzero(as_tuple=True)                              # R rows, scene-major
        self.active = vis[self.s_idx, :, self.t_idx].to(torch.uint8).contiguous()         # (R, P)
        self.r_of, self.p_of = self.active.nonzero(as_tuple=True)                         # the N visible (row, person) pairs
        s, t = self.s_idx[self.r_of], self.t_idx[self.r_of]
        self.spt = (s, self.p_of, t)
        self.body_pose, self.betas = pose[s, self.p_of, t].contiguous(), beta[s, self.p_of, t].contiguous()
        self.inv_len = 1.0 / packed.t['seq_len'].view(S).to(torch.float32)                # loss_all /= max_fr (:278,289)

    def __call__(self, orient, trans):
        """orient / trans (S, P, T, 3) -> (S,) unweighted values, differentiable with respect to both."""
        R, P = self.active.shape
        if R == 0:
            return torch.zeros(self.S, dtype=torch.float32, device=orient.device)
        out = self.smpl(global_orient=orient[self.spt], body_pose=self.body_pose, betas=self.betas, root_trans=trans[self.spt], return_verts=True)
        verts = out.vertices.new_zeros((R, P) + tuple(out.vertices.shape[1:])).index_put((self.r_of, self.p_of), out.vertices)
        per_row = self.sdf_loss.frames(verts, self.active)
        return torch.zeros(self.S, dtype=torch.float32, device=orient.device).index_add(0, self.s_idx, per_row) * self.inv_len


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
    points and cam_pose: project(joints()) is the reference's kp_2d_pred."""

    def __init__(self, smpl, stage, iteration, seq_names, orient_world, trans_world, exist, vis, smpl_pose, smpl_beta, cam_pose=None, cam_K=None,
                 kp_2d=None, kp_score=None):
        self._smpl = smpl
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


class ExtraLossSchedule:
    """run_schedule with opt.extra_loss(ctx) -> (S,) tensor, one already weighted value per scene, added to every stage's total -- and / or the
    built-in penetration term of the stages whose loss_cfg listed it (opt._pen_cfg: weight, monitor_only)."""

    def __init__(self, opt, packed, skip_term=False):
        # skip_term: the same launches and Adam steps without steps 2-4 (what a zero term must reproduce; the timing tool's baseline)
        self.opt, self.packed, self.skip_term = opt, packed, skip_term

    def pose_backward(self, sd, g_orient, g_trans, grads, accumulate=1):
        """glamr_grecon_pose_backward on the packed batch (current stream)."""
        packed, L = self.packed, _lib.lib()
        if getattr(self, '_ws', None) is None:
            self._ws = torch.empty(L.glamr_grecon_pose_backward_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=packed.device)
        sb = packed.struct()
        _lib.check(L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(g_orient), _lib.ptr(g_trans), _lib.ptr(grads), int(accumulate),
                                                _lib.ptr(self._ws), _lib.current_stream()))

    def cam_backward(self, sd, g_cam, grads, g_orient, g_trans, accumulate=1):
        """glamr_grecon_cam_backward on the packed batch (current stream); g_orient / g_trans are added into (camera derived from the persons)."""
        packed, L = self.packed, _lib.lib()
        if getattr(self, '_cam_ws', None) is None:
            self._cam_ws = torch.empty(L.glamr_grecon_cam_backward_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=packed.device)
        sb = packed.struct()
        _lib.check(L.glamr_grecon_cam_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(g_cam), _lib.ptr(grads), int(accumulate), _lib.ptr(g_orient),
                                               _lib.ptr(g_trans), _lib.ptr(self._cam_ws), _lib.current_stream()))

    def _penetration_only(self, sd, spec, pen, pen_term, pen_hist, it, grads, S, P, T):
        """Steps 2-4 for the built-in term alone: its value on copies of the reported poses, and unless it is monitor_only the weighted gradient
        through glamr_grecon_pose_backward into `grads`.  The term does not see the camera."""
        packed = self.packed
        orient = packed.t['orient_world'].view(S, P, T, 3).clone().requires_grad_(not pen['monitor_only'])
        trans = packed.t['trans_world'].view(S, P, T, 3).clone().requires_grad_(not pen['monitor_only'])
        with torch.set_grad_enabled(not pen['monitor_only']):
            value = pen_term(orient, trans)
        pen_hist[:, it] = value.detach()
        if pen['monitor_only'] or not value.requires_grad:
            return
        (pen['weight'] * value.sum()).backward()
        if 'world_dheading' in spec['opt_variables']:
            sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
        self.pose_backward(sd, orient.grad.contiguous(), trans.grad.contiguous(), grads, accumulate=1)

    def run(self, max_iters=None, has_wd=False):
        from .. import parallel
        opt, packed = self.opt, self.packed
        pen_cfg = getattr(opt, '_pen_cfg', None) or {}
        if opt.extra_loss is None and not pen_cfg:
            raise ValueError('ExtraLossSchedule needs GlobalReconOptimizer.extra_loss or a penetration term in loss_cfg')
        what = 'extra_loss' if opt.extra_loss is not None else 'the penetration term (loss_cfg)'
        check_supported(opt.specs, what)
        check_not_sharded(packed, what)
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError('%s runs launch by launch with host Python in every iteration and cannot be captured into a graph' % what)
        S, P, T = packed.S, packed.P, packed.T
        params = packed.t['params']
        t_idx = torch.arange(T, device=packed.device)
        fs, fe = packed.t['fr_start'].view(S, P, 1), packed.t['fr_end'].view(S, P, 1)
        slot_ok = torch.arange(P, device=packed.device).view(1, P, 1) < packed.t['n_persons'].view(S, 1, 1)
        exist = (t_idx >= fs) & (t_idx < fe) & (t_idx < packed.t['seq_len'].view(S, 1, 1)) & slot_ok
        vis = (packed.t['vis'].view(S, P, T) > 0) & slot_ok
        pa = getattr(packed, 'person_arrays', None)
        pose = pa['smpl_pose'].view(S, P, T, 69) if pa is not None else None
        beta = pa['smpl_beta'].view(S, P, T, 10) if pa is not None else None
        seq_names = getattr(packed, 'seq_names', None) or ['seq%d' % si for si in range(S)]
        cam_K, kp_2d, kp_score = packed.t['cam_K'].view(S, P, T, 3, 3), packed.t['kp_2d'].view(S, P, T, -1, 2), packed.t['kp_score'].view(S, P, T, -1)
        opt.extra_loss_history = {}
        pen_term = PenetrationTerm(opt, packed, vis, pose, beta) if pen_cfg and not self.skip_term else None
        if pen_cfg:
            opt.penetration_history = {}
        for stage, spec in opt.opt_stage_specs.items():
            n = stepwise.stage_iters(spec, max_iters)
            m, v = torch.zeros_like(params), torch.zeros_like(params)
            adam = stepwise.IndexedAdam(spec['opt_lr'], n, packed.device)
            hist = torch.zeros((S, n), dtype=torch.float32, device=packed.device)
            pen = pen_cfg.get(stage)
            pen_hist = torch.zeros((S, n), dtype=torch.float32, device=packed.device) if pen is not None else None
            for it in range(n):
                sd = stepwise.grad_launch_desc(spec, opt.specs, has_wd, first=(it == 0))
                grads = parallel._device_run_stage(packed, sd, True)                                  # 1.
                if self.skip_term or (opt.extra_loss is None and pen is None):      # (a stage that lists no term: the skip path)
                    adam.step(params, m, v, grads)
                    continue
                if opt.extra_loss is None:
                    self._penetration_only(sd, spec, pen, pen_term, pen_hist, it, grads, S, P, T)
                    if opt.extra_loss_grad_hook is not None:
                        opt.extra_loss_grad_hook(stage, it, grads)
                    adam.step(params, m, v, grads)
                    continue
                orient = packed.t['orient_world'].view(S, P, T, 3).clone().requires_grad_(True)
                trans = packed.t['trans_world'].view(S, P, T, 3).clone().requires_grad_(True)
                cam_derived = 'cam' not in spec['opt_variables'] and bool(sd.flags & packing.FLAG_CAM_FROM_PERSON)
                # (source, requires grad): a leaf in the three live modes, a plain tensor when the camera is a constant of the stage
                cam = (packed.t['cam_pose'].view(S, T, 3, 4), 'cam' in spec['opt_variables'] or cam_derived)
                ctx = ExtraLossContext(opt.smpl, stage, it, seq_names, orient, trans, exist, vis, pose, beta, cam, cam_K, kp_2d, kp_score)
                with torch.enable_grad():
                    loss = opt.extra_loss(ctx)                                                        # 2.
                    if not torch.is_tensor(loss) or tuple(loss.shape) != (S,):
                        raise ValueError('extra_loss must return a tensor of shape (%d,): one value per scene' % S)
                    if not loss.requires_grad:
                        raise ValueError('extra_loss returned a value that does not depend on ctx.orient_world / ctx.trans_world / ctx.cam_pose (no gradient): '
                                         'a term without a gradient would be a silent zero')
                    total = loss.sum()
                    if pen is not None:                                                               # the built-in term beside the caller's
                        with torch.set_grad_enabled(not pen['monitor_only']):
                            value = pen_term(orient, trans)
                        pen_hist[:, it] = value.detach()
                        if not pen['monitor_only']:
                            total = total + pen['weight'] * value.sum()
                    total.backward()                                                                  # 3.
                g_cam = ctx.cam_grad()
                if orient.grad is None and trans.grad is None and g_cam is None:
                    raise ValueError('extra_loss returned a value that does not depend on ctx.orient_world / ctx.trans_world / ctx.cam_pose (grad is None)')
                # the stage kernel applies the world heading offset as soon as the stage optimises it (the variable exists from then on, :459-465)
                if 'world_dheading' in spec['opt_variables']:
                    sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
                g_o = None if orient.grad is None else orient.grad.contiguous()
                g_t = None if trans.grad is None else trans.grad.contiguous()
                if g_cam is not None:                                                                 # 4. the camera first: it may add to the pose gradients
                    if cam_derived:
                        g_o = torch.zeros_like(orient) if g_o is None else g_o
                        g_t = torch.zeros_like(trans) if g_t is None else g_t
                    self.cam_backward(sd, g_cam.contiguous(), grads, g_o if cam_derived else None, g_t if cam_derived else None, accumulate=1)
                if g_o is not None or g_t is not None:
                    self.pose_backward(sd, g_o, g_t, grads, accumulate=1)
                if opt.extra_loss_grad_hook is not None:
                    opt.extra_loss_grad_hook(stage, it, grads)      # (the complete gradient of the iteration, before the update)
                adam.step(params, m, v, grads)                                                        # 5.
                hist[:, it] = loss.detach()
            if opt.extra_loss is not None:
                opt.extra_loss_history[stage] = hist.cpu().numpy()
            if pen is not None:
                opt.penetration_history[stage] = pen_hist.cpu().numpy()
            has_wd = stepwise.end_stage(packed, spec, has_wd)
        packed.has_world_dheading = has_wd
        packed.stage_ws = []
        return packed
