"""MI355X: glamr_grecon_pose_backward through the C ABI against the fp64 autograd reference of tests/extra_loss_common.py, its agreement with
the stage kernel's own chain, and GlobalReconOptimizer.extra_loss end to end against the fp64 port (tests/extra_loss_e2e.py, read from
tests/golden)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import extra_loss_common as xc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


class Launch:
    """One glamr_grecon_pose_backward call over the C ABI on buffers made beforehand (so it can be recorded into a graph)."""

    def __init__(self, case, G, accumulate=0, before=None, flags=None, var_mask=None):
        self.arrays = {k: _dev(v) for k, v in xc.host_arrays(case).items()}
        self.sb = xc.scene_batch(case, {k: v.data_ptr() for k, v in self.arrays.items()})
        self.sd = xc.stage_desc(case, flags, var_mask)
        self.G = [_dev(g) for g in G]
        n = case['S'] * xc.layout(case)['scene_stride']
        self.out = torch.full((n,), 7.0, device=DEV) if before is None else _dev(before)      # (store mode: every entry must be overwritten)
        self.accumulate = accumulate
        self.ws = torch.full((_lib.lib().glamr_grecon_pose_backward_workspace_bytes(case['S'], case['P'], case['T']),), 0xff, dtype=torch.uint8, device=DEV)

    def __call__(self):
        _lib.check(_lib.lib().glamr_grecon_pose_backward(ctypes.byref(self.sb), ctypes.byref(self.sd), _lib.ptr(self.G[0]), _lib.ptr(self.G[1]), _lib.ptr(self.out),
                                                         self.accumulate, _lib.ptr(self.ws), _lib.current_stream()))
        return self.out


def _run(case, G, **kw):
    out = Launch(case, G, **kw)().clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', xc.CASE_NAMES)
def test_kernel_matches_fp64_autograd(name):
    """Every upstream pattern of the case (NaN wherever the kernel must not read) within 16 x the fp32 autograd floor per variable group and
    person; exact zeros wherever no variable of the mask lives; a second call gives the same bits."""
    case = xc.cases()['cases'][name]
    tol = xc.tol(name)
    worst = {k: 0.0 for k in xc.GROUPS}
    for pattern in xc.PATTERNS:
        G = xc.upstream(case, pattern)
        a, b = _run(case, G), _run(case, G)
        assert torch.equal(a, b)
        got = a.cpu().numpy()
        assert np.isfinite(got).all()
        assert (got[~xc.written_mask(case)] == 0).all()
        e = xc.errors(case, got, xc.ref64(name, pattern))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('pose VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, worst[k], tol[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


@pytest.mark.parametrize('scale', xc.SCALES)
def test_scaled_upstream_gradients_stay_within_the_tolerances(scale):
    """Plain fp32 and linear in G: with G x 1e-6 and G x 1e5 the results keep the tolerances (the reference is given the same scaled arrays)."""
    for name in xc.CASE_NAMES:
        case = xc.cases()['cases'][name]
        got = _run(case, xc.upstream(case, 'all', scale=scale)).cpu().numpy()
        e = xc.errors(case, got, xc.reference(case, 'all', scale=scale))
        print('G x %g, %s: %s' % (scale, name, ', '.join('%s %.2e' % kv for kv in e.items())))
        for k, v in e.items():
            assert v <= xc.tol(name)[k], (name, k, v)


@pytest.mark.parametrize('name', ['batch_wd', 'norot', 'frozen_wd'])
def test_add_mode_is_store_mode_plus_the_previous_contents(name):
    """Previous contents and upstream gradients on a power-of-two grid; add mode is one fp32 addition per entry a variable of the mask owns and
    leaves every other entry's bits alone (NaN there)."""
    case = xc.cases()['cases'][name]
    G = tuple(np.round(g * 64) / 64 for g in xc.upstream(case, 'all'))
    stored = _run(case, G).cpu().numpy()
    before = (np.random.default_rng(3).integers(-64, 65, size=stored.shape) / 64.0).astype(np.float32)
    w = xc.written_mask(case)
    before[~w] = np.nan
    added = _run(case, G, accumulate=1, before=before).cpu().numpy()
    assert np.array_equal(added[w], before[w] + stored[w])
    assert np.isnan(added[~w]).all()


def test_var_mask_without_local_rot_leaves_its_block_zero_or_untouched():
    case = xc.cases()['cases']['norot_wd']
    l, b = xc.layout(case), xc.block(case, 0, 0)
    rot = slice(b + l['local_rot'], b + l['local_rot'] + 6 * case['T'])
    G = xc.upstream(case, 'all')
    assert (_run(case, G).cpu().numpy()[rot] == 0).all()
    before = np.full(case['S'] * l['scene_stride'], 5.0, np.float32)
    assert (_run(case, G, accumulate=1, before=before).cpu().numpy()[rot] == 5.0).all()
    assert np.abs(_run(case, G, var_mask=xc.ALL_VARS).cpu().numpy()[rot]).max() > 0


def test_graph_replay_with_new_upstream_gradients():
    """The call recorded into a torch.cuda.graph (one chain) and replayed twice, each time with other upstream gradients written into the
    recorded buffers: the plain launch's bits."""
    case = xc.cases()['cases']['batch_wd']
    launch = Launch(case, xc.upstream(case, 'all'))
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for scale in (0.5, -3.0):
        G = xc.upstream(case, 'all', scale=scale)
        plain = _run(case, G)
        for buf, g in zip(launch.G, G):
            buf.copy_(_dev(g))
        launch.out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(launch.out, plain)


def test_argument_checks():
    case = xc.cases()['cases']['one24']
    with pytest.raises(RuntimeError, match='at least one'):
        Launch(case, (None, None))()
    with pytest.raises(RuntimeError, match='ABSOLUTE_HEADING'):
        Launch(case, xc.upstream(case, 'all'), flags=packing.FLAG_ABSOLUTE_HEADING)()


# ---- the schedule and the public interface --------------------------------------------------------------------------------------------------
from oracle.port import transforms as tf                      # noqa: E402
from glamr_amd.global_recon import extra_loss_schedule as xs  # noqa: E402
from tests import attach_common as ac                         # noqa: E402
from tests import extra_loss_e2e as xe                        # noqa: E402
from tests.grecon_common import grads_by_name, j_local_from_oracle      # noqa: E402


@pytest.fixture(scope='module')
def priors(asset_root):
    import os
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    return smpl, MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def _model(priors, cfg, **flags):
    from glamr_amd.global_recon.models import model_dict
    cfg = copy.deepcopy(cfg)
    cfg['grecon_model_specs'].update(flags)
    return model_dict['global_recon_model'](cfg, DEV, None, smpl=priors[0], mt_model=priors[1])


# the callbacks: every slot of the test scenes holds a person and max_len is the scene's length, so the sums run over whole arrays
def term_rot(ctx):
    """traj_rot_smoothness (loss_func.py:117-132, rot_type 6d) with its normaliser and the shipped weight"""
    S, P, T = ctx.exist.shape
    d6 = tf.aa_to_6d(ctx.orient_world)
    return 1.e+3 * ((d6[:, :, 1:] - d6[:, :, :-1]) * 30).pow(2).sum((1, 2, 3)) / (P * (T - 1))


def term_trans(ctx):
    """traj_trans_smoothness (loss_func.py:135-144)"""
    S, P, T = ctx.exist.shape
    return xe.W_TRANS * ((ctx.trans_world[:, :, 1:] - ctx.trans_world[:, :, :-1]) * 30).pow(2).sum((1, 2, 3)) / (P * (T - 1))


def term_heels(ctx):
    S, P, T = ctx.exist.shape
    return xe.W_HEELS * ctx.joints()[:, :, :, list(xe.HEELS), 2].pow(2).sum((1, 2, 3)) / (2 * P * T)


TERMS = {'rot': term_rot, 'trans': term_trans, 'heels': term_heels}


def _packed(asset_root, run):
    """The port's state after init_data packed for the device, the device configuration (the run's loss_cfg entry dropped) and the state."""
    cfg, ora, data = xe.state(asset_root, run)
    cfg = copy.deepcopy(cfg)
    drop = xe.RUNS[run][3]
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


def test_new_kernel_and_stage_kernel_describe_one_chain(asset_root, golden):
    """A stage of glamr_dynamic WITHOUT traj_rot_smoothness: its gradient launch, plus that term's torch gradient with respect to orient_world
    pushed through glamr_grecon_pose_backward, is the fp64 port's gradient of the unmodified loss_cfg."""
    from glamr_amd import parallel
    from glamr_amd.global_recon import stepwise
    cfg, data, packed = _packed(asset_root, 'rot')
    (stage, spec), = cfg['opt_stage_specs'].items()
    sd = stepwise.grad_launch_desc(spec, cfg['grecon_model_specs'], False, first=True)
    grads = parallel._device_run_stage(packed, sd, True)
    S, P, T = packed.S, packed.P, packed.T
    orient = packed.t['orient_world'].view(S, P, T, 3).clone().requires_grad_(True)
    ctx = xs.ExtraLossContext(None, stage, 0, None, orient, None, packed.t['vis'].view(S, P, T) > 0, None, None, None)
    term_rot(ctx).sum().backward()
    sd.flags |= packing.FLAG_HAS_WORLD_DHEADING                       # (the stage optimises world_dheading: the kernel applies it)
    ws = torch.empty(_lib.lib().glamr_grecon_pose_backward_workspace_bytes(S, P, T), dtype=torch.uint8, device=DEV)
    sb = packed.struct()
    _lib.check(_lib.lib().glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(orient.grad.contiguous()), None, _lib.ptr(grads), 1,
                                                     _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    got = {'%s/grad/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, grads.cpu(), data, cfg['grecon_model_specs'], spec['opt_variables']).items()}
    ref = {k: v for k, v in xe.from_fixture(golden(xe.FIXTURE), 'rot').items() if '/grad/' in k}
    e = xe.errors(got, ref)
    print('stage kernel + pose VJP against the fp64 port: grad %.2e (bound %.2e)' % (e['grad'], xe.TOL['rot']['grad']))
    assert e['grad'] <= xe.TOL['rot']['grad']


@pytest.mark.parametrize('run', list(xe.RUNS))
def test_end_to_end_against_the_fp64_port(asset_root, golden, priors, run):
    """K = 5 iterations per stage from the port's state after init_data: every stage's first gradient, the last stage's variables and the
    world poses of its last evaluation within 16 x the fp32 port's deviation from its fp64 run."""
    cfg, data, packed = _packed(asset_root, run)
    model = _model(priors, cfg)
    model.extra_loss = TERMS[run]
    first = {}
    model.extra_loss_grad_hook = lambda stage, it, g: first.setdefault(stage, g.clone()) if it == 0 else None
    xs.ExtraLossSchedule(model, packed).run(max_iters=xe.K)
    torch.cuda.synchronize()
    specs, got = cfg['grecon_model_specs'], {}
    for stage, spec in cfg['opt_stage_specs'].items():
        got.update({'%s/grad/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, first[stage].cpu(), data, specs, spec['opt_variables']).items()})
        assert model.extra_loss_history[stage].shape == (1, xe.K) and np.isfinite(model.extra_loss_history[stage]).all()
    got.update({'%s/param/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, packed.t['params'].cpu(), data, specs, spec['opt_variables']).items()})
    Ts = int(data['seq_len'])
    for pi, idx in enumerate(packed.person_ids[0]):
        got['%s/orient/p%d' % (stage, idx)] = packed.t['orient_world'][pi, :Ts].cpu().numpy()
        got['%s/trans/p%d' % (stage, idx)] = packed.t['trans_world'][pi, :Ts].cpu().numpy()
    ref = xe.from_fixture(golden(xe.FIXTURE), run)
    e = xe.errors(got, ref)
    print('extra_loss %s: %s' % (run, ', '.join('%s %.2e (bound %.2e)' % (k, e[k], xe.TOL[run][k]) for k in xe.KINDS)))
    for k in xe.KINDS:
        assert e[k] <= xe.TOL[run][k], (k, e[k], xe.TOL[run][k])


def _inputs():
    return ac.scene_inputs('one')


def test_zero_term_equals_the_schedule_with_the_term_skipped(priors):
    cfg_id, in_dict, lat = _inputs()
    from glamr_amd.global_recon.configs import get_config
    model = _model(priors, get_config(cfg_id))
    model.extra_loss = lambda ctx: 0 * ctx.trans_world.sum((1, 2, 3))
    out = {}
    for skip in (True, False):
        datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
        xs.ExtraLossSchedule(model, packed, skip_term=skip).run(max_iters=3)
        torch.cuda.synchronize()
        out[skip] = packed.t['params'].cpu().numpy()
    assert np.abs(out[True]).max() > 0 and np.array_equal(out[True], out[False])
    # ... and optimize() with the callback set runs that schedule
    res = model.optimize(in_dict, latents=lat, max_iters=3)
    assert set(model.extra_loss_history) == set(model.opt_stage_specs) and (model.extra_loss_history['init_opt'] == 0).all()
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    xs.ExtraLossSchedule(model, packed).run(max_iters=3)
    ref = model.collect(datas, packed)[0]
    for k in ('smpl_orient_world', 'root_trans_world', 'traj_local_rot'):
        assert np.array_equal(np.asarray(res['person_data'][0][k]), np.asarray(ref['person_data'][0][k])), k


def test_without_extra_loss_optimize_is_the_fused_schedule(priors, monkeypatch):
    """extra_loss None: optimize() gives run_schedule's results bit for bit and never enters the launch-by-launch schedule."""
    cfg_id, in_dict, lat = _inputs()
    from glamr_amd.global_recon.configs import get_config
    model = _model(priors, get_config(cfg_id))
    assert model.extra_loss is None

    def boom(*a, **k):
        raise AssertionError('the launch-by-launch schedule ran without extra_loss')
    monkeypatch.setattr(xs.ExtraLossSchedule, 'run', boom)
    res = model.optimize(in_dict, latents=lat, max_iters=3)
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    model.run_schedule(packed, 3)
    ref = model.collect(datas, packed)[0]
    for k in ('smpl_orient_world', 'root_trans_world', 'kp_2d_pred', 'traj_local_rot', 'traj_local_xy', 'world_dheading'):
        assert np.array_equal(np.asarray(res['person_data'][0][k]), np.asarray(ref['person_data'][0][k])), k
    assert np.array_equal(np.asarray(res['cam_pose']), np.asarray(ref['cam_pose']))


def test_refused_combinations_and_entry_points(priors):
    cfg_id, in_dict, lat = _inputs()
    from glamr_amd.global_recon.configs import get_config
    term = lambda ctx: ctx.trans_world.pow(2).sum((1, 2, 3))
    for flags, word in ((dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'), (dict(absolute_heading=True), 'absolute_heading'),
                        (dict(flag_opt_traj_latent=True), 'latent')):
        with pytest.raises(ValueError, match=word):
            _model(priors, get_config(cfg_id), **flags).extra_loss = term
    model = _model(priors, get_config(cfg_id))
    model.extra_loss = term
    rin = model.stage_inputs([in_dict], [lat])
    with pytest.raises(NotImplementedError, match='optimize_resident'):
        model.optimize_resident(rin, 1)
    with pytest.raises(NotImplementedError, match='optimize_stream'):
        model.optimize_stream([[in_dict]])
    with pytest.raises(NotImplementedError, match='capture_resident'):
        model.capture_resident(rin, 1)
    model.extra_loss = lambda ctx: torch.zeros(1, device=DEV)                # does not depend on the poses
    with pytest.raises(ValueError, match='does not depend'):
        model.optimize(in_dict, latents=lat, max_iters=1)
    model.extra_loss = term
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='person-sharded'):
        xs.ExtraLossSchedule(model, packed).run(max_iters=1)
