"""MI355X: glamr_grecon_cam_backward through the C ABI against the fp64 autograd reference of tests/extra_loss_cam_common.py, its agreement
with the stage kernel's own camera chain, and camera terms of GlobalReconOptimizer.extra_loss end to end against the fp64 port
(tests/extra_loss_cam_e2e.py, read from tests/golden)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import extra_loss_cam_common as cc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


class Launch:
    """One glamr_grecon_cam_backward call over the C ABI on buffers made beforehand (so it can be recorded into a graph)."""

    def __init__(self, case, G, accumulate=0, before=None, pose_before=None, mode=None, null_pose=False):
        self.arrays = {k: _dev(v) for k, v in cc.host_arrays(case).items()}
        self.sb = cc.scene_batch(case, {k: v.data_ptr() for k, v in self.arrays.items()})
        self.sd = cc.stage_desc(case, mode)
        self.G = _dev(G)
        S, P, T = case['S'], case['P'], case['T']
        n = S * cc.layout(case)['scene_stride']
        self.out = torch.full((n,), 7.0, device=DEV) if before is None else _dev(before)      # (store mode: every entry must be overwritten)
        self.pose = [None, None] if null_pose else [torch.zeros((S * P, T, 3), device=DEV) if pose_before is None else _dev(pose_before[i]) for i in range(2)]
        self.accumulate = accumulate
        self.ws = torch.full((max(1, _lib.lib().glamr_grecon_cam_backward_workspace_bytes(S, P, T)),), 0xff, dtype=torch.uint8, device=DEV)      # NaN

    def __call__(self):
        _lib.check(_lib.lib().glamr_grecon_cam_backward(ctypes.byref(self.sb), ctypes.byref(self.sd), _lib.ptr(self.G), _lib.ptr(self.out), self.accumulate,
                                                        _lib.ptr(self.pose[0]), _lib.ptr(self.pose[1]), _lib.ptr(self.ws), _lib.current_stream()))
        return self

    def result(self):
        torch.cuda.synchronize()
        S, P, T = self.sb.n_scenes, self.sb.max_persons, self.sb.max_len
        z = np.zeros((S * P, T, 3), np.float32)
        return dict(grads=self.out.cpu().numpy(), g_orient_world=z if self.pose[0] is None else self.pose[0].cpu().numpy(),
                    g_trans_world=z if self.pose[1] is None else self.pose[1].cpu().numpy())


def _run(case, G, **kw):
    return Launch(case, G, **kw)().result()


@pytest.mark.parametrize('name', cc.CASE_NAMES)
def test_kernel_matches_fp64_autograd(name):
    """Every upstream pattern of the case (NaN wherever the kernel must not read: padding rows of g_cam_pose, the other modes' and the persons'
    parameter blocks, poses and person2cam of empty, frozen and invisible persons, the workspace) within 16 x the fp32 autograd floor per group
    and scene / person; exact zeros wherever the call owns nothing; a second call gives the same bits."""
    case = cc.cases()['cases'][name]
    tol = cc.tol(name)
    w, pw = cc.written_mask(case), cc.pose_written_mask(case)
    worst = {k: 0.0 for k in cc.GROUPS}
    for pattern in cc.PATTERNS:
        G = cc.upstream(case, pattern)
        got, again = _run(case, G), _run(case, G)
        assert all(np.array_equal(got[k], again[k]) for k in got)
        assert np.isfinite(got['grads']).all() and (got['grads'][~w] == 0).all()
        for k in cc.POSE_GROUPS:
            assert np.isfinite(got[k]).all() and (got[k][~pw] == 0).all()
        e = cc.errors(case, got, cc.ref64(name, pattern))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('camera VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, worst[k], tol[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


@pytest.mark.parametrize('scale', cc.SCALES)
def test_scaled_upstream_gradients_stay_within_the_tolerances(scale):
    """Plain fp32 and linear in G: with G x 1e-6 and G x 1e5 the results keep the tolerances (the reference is given the same scaled arrays)."""
    for name in cc.CASE_NAMES:
        case = cc.cases()['cases'][name]
        got = _run(case, cc.upstream(case, 'all', scale=scale))
        e = cc.errors(case, got, cc.reference(case, 'all', scale=scale))
        print('G x %g, %s: %s' % (scale, name, ', '.join('%s %.2e' % kv for kv in e.items())))
        for k, v in e.items():
            assert v <= cc.tol(name)[k], (name, k, v)


@pytest.mark.parametrize('name', ['frame_batch', 'fixed_short', 'derived40', 'derived_frozen'])
def test_add_mode_is_store_mode_plus_the_previous_contents(name):
    """Add mode is one fp32 addition per entry the call owns and leaves every other entry's bits alone (NaN there); the pose buffers are added
    into in both settings, only where a live person is visible."""
    case = cc.cases()['cases'][name]
    G = cc.upstream(case, 'all')
    S, P, T = case['S'], case['P'], case['T']
    zero = _run(case, G)
    pw, w = cc.pose_written_mask(case), cc.written_mask(case)
    rng = np.random.default_rng(3)
    pose_before = [(rng.integers(-64, 65, size=(S * P, T, 3)) / 64.0).astype(np.float32) for _ in range(2)]
    for pb in pose_before:
        pb[~pw] = np.nan
    before = (rng.integers(-64, 65, size=zero['grads'].shape) / 64.0).astype(np.float32)
    before[~w] = np.nan
    stored = _run(case, G, pose_before=pose_before)
    added = _run(case, G, accumulate=1, before=before, pose_before=pose_before)
    assert np.array_equal(stored['grads'], zero['grads'])
    assert np.array_equal(added['grads'][w], before[w] + zero['grads'][w]) and np.isnan(added['grads'][~w]).all()
    for i, k in enumerate(cc.POSE_GROUPS):
        for r in (stored, added):
            assert np.array_equal(r[k][pw], pose_before[i][pw] + zero[k][pw]) and np.isnan(r[k][~pw]).all()


def test_mode_selection_constant_camera_and_argument_checks():
    case = cc.cases()['cases']['derived40']
    G = cc.upstream(case, 'all')
    # (the case's descriptor is var_mask without cam + FLAG_CAM_FROM_PERSON: the derived mode, checked against its reference above)
    assert cc.stage_desc(case).var_mask & packing.VAR_BITS['cam'] == 0 and cc.stage_desc(case).flags == packing.FLAG_CAM_FROM_PERSON
    launch = Launch(case, G, mode='constant')
    with pytest.raises(RuntimeError, match='constant'):
        launch()
    got = launch.result()
    assert (got['grads'] == 7.0).all() and all((got[k] == 0).all() for k in cc.POSE_GROUPS)
    with pytest.raises(RuntimeError, match='g_orient_world'):
        Launch(case, G, null_pose=True)()
    with pytest.raises(RuntimeError, match='g_cam_pose'):
        Launch(case, None)()
    frame = cc.cases()['cases']['frame24']
    ref = _run(frame, cc.upstream(frame, 'all'))
    assert np.array_equal(_run(frame, cc.upstream(frame, 'all'), null_pose=True)['grads'], ref['grads'])      # ignored in the optimised modes


@pytest.mark.parametrize('name', ['frame_batch', 'fixed257', 'derived40'])
def test_graph_replay_with_new_upstream_gradients(name):
    """The call recorded into a torch.cuda.graph and replayed twice, each time with another g_cam_pose written into the recorded buffer: the
    plain launch's bits."""
    case = cc.cases()['cases'][name]
    launch = Launch(case, cc.upstream(case, 'all'))
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for scale in (0.5, -3.0):
        G = cc.upstream(case, 'all', scale=scale)
        plain = _run(case, G)
        launch.G.copy_(_dev(G))
        launch.out.fill_(3.0)
        for p in launch.pose:
            p.zero_()
        graph.replay()
        got = launch.result()
        assert all(np.array_equal(got[k], plain[k]) for k in got)


# ---- the schedule and the public interface --------------------------------------------------------------------------------------------------
from glamr_amd.global_recon import extra_loss_schedule as xs  # noqa: E402
from tests import attach_common as ac                         # noqa: E402
from tests import extra_loss_cam_e2e as ce                    # noqa: E402
from tests.grecon_common import grads_by_name, j_local_from_oracle      # noqa: E402


@pytest.fixture(scope='module')
def priors(asset_root):
    import os
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    return smpl, MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def _model(priors, cfg):
    from glamr_amd.global_recon.models import model_dict
    return model_dict['global_recon_model'](copy.deepcopy(cfg), DEV, None, smpl=priors[0], mt_model=priors[1])


def _packed(asset_root, run):
    """The port's state after init_data packed for the device, the device configuration (the run's loss_cfg entry dropped) and the state."""
    cfg, ora, data, _ = ce.state(asset_root, run)
    cfg = copy.deepcopy(cfg)
    drop = ce.RUNS[run][6]
    for spec in cfg['opt_stage_specs'].values():
        if drop is not None:
            spec['loss_cfg'].pop(drop)
    packed = packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], DEV)
    S, P, T = packed.S, packed.P, packed.T
    pose, beta = torch.zeros((S * P, T, 69)), torch.zeros((S * P, T, 10))
    for pi, idx in enumerate(packed.person_ids[0]):
        pose[pi], beta[pi] = data['person_data'][idx]['smpl_pose'], data['person_data'][idx]['smpl_beta']
    packed.person_arrays = dict(smpl_pose=pose.to(DEV), smpl_beta=beta.to(DEV))
    return cfg, data, packed


# the callbacks: every slot of the test scenes holds a person and max_len is the scene's length, so the sums run over whole arrays
def term_kp(ctx):
    """kp_2d (loss_func.py:15-36) with the shipped weight 1, min_conf 0.3 and sigma 100, summed in double as the reference does"""
    diff = ctx.project(ctx.joints()).double() - ctx.kp_2d.double()
    score = torch.where(ctx.kp_score < 0.3, torch.zeros_like(ctx.kp_score), ctx.kp_score).double()
    x2 = diff ** 2
    loss = ((1.e4 * x2) / (1.e4 + x2)).sum(-1) * score ** 2 * ctx.vis[..., None]
    return (loss.sum((1, 2, 3)) / ctx.vis.sum((1, 2))).float()


def term_height(ctx):
    origin_up = -(ctx.cam_pose[..., :3, 2] * ctx.cam_pose[..., :3, 3]).sum(-1)      # third coordinate of -R^T t
    return ce.W_HEIGHT * (origin_up - ce.H_CAM).pow(2).mean(1)


def make_term_heels(targets):
    tgt = torch.stack([torch.tensor(targets[idx], dtype=torch.float32) for idx in sorted(targets)])[None].to(DEV)      # (1, P, T, 2, 2)

    def term_heels(ctx):
        S, P, T = ctx.exist.shape
        return ce.W_HEELS * (ctx.project(ctx.joints()[:, :, :, list(ce.HEELS)]) - tgt).pow(2).sum((1, 2, 3, 4)) / (2 * P * T)
    return term_heels


def _terms(golden):
    return {'kp': term_kp, 'height': term_height, 'heels': make_term_heels(ce.targets_from_fixture(golden(ce.FIXTURE)))}


@pytest.mark.parametrize('run', list(ce.RUNS))
def test_new_kernel_and_stage_kernel_describe_one_chain(asset_root, priors, run):
    """kp_2d alone in the last stage's loss_cfg.  First path: the stage kernel's gradient launch gives the gradient of every variable.  Second
    path: the stage kernel with an EMPTY loss set reports the poses and the camera, the same term is written in torch on
    ctx.project(ctx.joints()) and pushed through glamr_grecon_cam_backward, then glamr_grecon_pose_backward.  The two agree within the fp64
    port's bound on that gradient -- per camera mode: per frame ('kp'), fixed ('height'), derived from two persons with a gap ('heels')."""
    from glamr_amd import parallel
    from glamr_amd.global_recon import stepwise
    cfg, data, packed = _packed(asset_root, run)
    stage, spec = ac.stage_of(cfg)
    specs = cfg['grecon_model_specs']
    only = dict(spec, loss_cfg={'kp_2d': spec['loss_cfg'].get('kp_2d', dict(weight=1.0, min_conf=0.3))})
    none = dict(spec, loss_cfg={})
    params0 = packed.t['params'].clone()
    first = parallel._device_run_stage(packed, stepwise.grad_launch_desc(only, specs, False, first=True), True).clone()
    packed.t['params'].copy_(params0)
    sd = stepwise.grad_launch_desc(none, specs, False, first=True)
    second = parallel._device_run_stage(packed, sd, True)
    assert float(second.abs().max()) == 0.0
    S, P, T = packed.S, packed.P, packed.T
    orient = packed.t['orient_world'].view(S, P, T, 3).clone().requires_grad_(True)
    trans = packed.t['trans_world'].view(S, P, T, 3).clone().requires_grad_(True)
    cam = packed.t['cam_pose'].view(S, T, 3, 4).clone().requires_grad_(True)
    pa = packed.person_arrays
    ctx = xs.ExtraLossContext(priors[0], stage, 0, None, orient, trans, None, packed.t['vis'].view(S, P, T) > 0, pa['smpl_pose'].view(S, P, T, 69),
                              pa['smpl_beta'].view(S, P, T, 10), cam, packed.t['cam_K'].view(S, P, T, 3, 3), packed.t['kp_2d'].view(S, P, T, -1, 2),
                              packed.t['kp_score'].view(S, P, T, -1))
    ctx.exist = ctx.vis
    term_kp(ctx).sum().backward()
    sched = xs.ExtraLossSchedule(None, packed)
    if 'world_dheading' in spec['opt_variables']:
        sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
    g_o, g_t = orient.grad.contiguous(), trans.grad.contiguous()
    derived = 'cam' not in spec['opt_variables']
    sched.cam_backward(sd, cam.grad.contiguous(), second, g_o if derived else None, g_t if derived else None)
    sched.pose_backward(sd, g_o, g_t, second)
    torch.cuda.synchronize()
    a, b = (grads_by_name(packed, g.cpu(), data, specs, spec['opt_variables']) for g in (first, second))
    worst = 0.0
    for k, v in a.items():
        scale = float(v.abs().max()) if v.numel() else 0.0
        e = float((b[k] - v).abs().max()) / (scale if scale > 0 else 1.0) if v.numel() else 0.0
        print('%s %-28s stage kernel against torch term + camera VJP + pose VJP: %.2e (largest entry %.2e)' % (run, k, e, scale))
        worst = max(worst, e)
    print('%s: %.2e (bound %.2e)' % (run, worst, ce.AGREE_TOL[run]))
    assert worst <= ce.AGREE_TOL[run], (run, worst, ce.AGREE_TOL[run])


@pytest.mark.parametrize('run', list(ce.RUNS))
def test_end_to_end_against_the_fp64_port(asset_root, golden, priors, run):
    """K = 5 iterations per stage from the port's state after init_data: every stage's first gradient, the last stage's variables and the
    camera and world poses of its last evaluation within 16 x the fp32 port's deviation from its fp64 run."""
    cfg, data, packed = _packed(asset_root, run)
    model = _model(priors, cfg)
    model.extra_loss = _terms(golden)[run]
    first = {}
    model.extra_loss_grad_hook = lambda stage, it, g: first.setdefault(stage, g.clone()) if it == 0 else None
    xs.ExtraLossSchedule(model, packed).run(max_iters=ce.K)
    torch.cuda.synchronize()
    specs, got = cfg['grecon_model_specs'], {}
    for stage, spec in cfg['opt_stage_specs'].items():
        got.update({'%s/grad/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, first[stage].cpu(), data, specs, spec['opt_variables']).items()})
        assert model.extra_loss_history[stage].shape == (1, ce.K) and np.isfinite(model.extra_loss_history[stage]).all()
    got.update({'%s/param/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, packed.t['params'].cpu(), data, specs, spec['opt_variables']).items()})
    Ts = int(data['seq_len'])
    got['%s/cam/pose' % stage] = packed.t['cam_pose'].view(packed.T, 3, 4)[:Ts].cpu().numpy()
    for pi, idx in enumerate(packed.person_ids[0]):
        got['%s/orient/p%d' % (stage, idx)] = packed.t['orient_world'][pi, :Ts].cpu().numpy()
        got['%s/trans/p%d' % (stage, idx)] = packed.t['trans_world'][pi, :Ts].cpu().numpy()
    ref = ce.from_fixture(golden(ce.FIXTURE), run)
    e = ce.errors(got, ref)
    print('extra_loss %s: %s' % (run, ', '.join('%s %.2e (bound %.2e)' % (k, e[k], ce.TOL[run][k]) for k in ce.KINDS)))
    for k in ce.KINDS:
        assert e[k] <= ce.TOL[run][k], (k, e[k], ce.TOL[run][k])


@pytest.mark.parametrize('run', ['height', 'heels'])
def test_zero_camera_term_equals_the_schedule_with_the_term_skipped(asset_root, priors, run):
    out = {}
    for skip in (True, False):
        cfg, data, packed = _packed(asset_root, run)
        model = _model(priors, cfg)
        model.extra_loss = lambda ctx: 0 * ctx.cam_pose.sum((1, 2, 3))
        xs.ExtraLossSchedule(model, packed, skip_term=skip).run(max_iters=3)
        torch.cuda.synchronize()
        out[skip] = packed.t['params'].cpu().numpy()
    assert np.abs(out[True]).max() > 0 and np.array_equal(out[True], out[False])


def test_context_fields_and_the_constant_camera(asset_root, priors):
    """ctx.cam_pose is a leaf that requires grad where the stage has a camera to move (with a fixed camera every frame holds row 0's) and a
    plain tensor in the first stage of a *_multi configuration, where a term on it alone is refused as one without a gradient."""
    from glamr_amd.global_recon.configs import get_config
    cfg_id, in_dict, lat = ac.scene_inputs('two')      # glamr_static_multi: init_opt optimises local_xy / local_heading only
    model = _model(priors, get_config(cfg_id))
    seen = []

    def term(ctx):
        S, P, T = ctx.exist.shape
        seen.append((ctx.stage, ctx.cam_pose.requires_grad, ctx.cam_pose.is_leaf, bool((ctx.cam_pose == ctx.cam_pose[:, :1]).all())))
        assert ctx.cam_pose.shape == (S, T, 3, 4) and ctx.cam_K.shape == (S, P, T, 3, 3) and ctx.kp_2d.shape == (S, P, T, 26, 2) and ctx.kp_score.shape == (S, P, T, 26)
        assert ctx.project(ctx.joints()).shape == (S, P, T, 26, 2)
        return ctx.trans_world.pow(2).sum((1, 2, 3)) + ctx.cam_pose.pow(2).sum((1, 2, 3))
    model.extra_loss = term
    model.optimize(in_dict, latents=lat, max_iters=1)
    assert seen == [('init_opt', False, True, True), ('main_opt', True, True, True)]
    model.extra_loss = lambda ctx: ctx.cam_pose.pow(2).sum((1, 2, 3))
    with pytest.raises(ValueError, match='does not depend'):
        model.optimize(in_dict, latents=lat, max_iters=1)
