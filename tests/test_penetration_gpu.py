"""MI355X: glamr_sdf_penetration through the C ABI against the fp64 restatement of tests/penetration_common.py -- every launch's output on its
own (boxes, flags, grids, loss, vertex gradients) --, the SDFLoss module over it, and the optimiser's built-in `penetration` term end to end
against the fp64 port (tests/penetration_e2e.py, read from tests/golden)."""
import numpy as np
import pytest
import torch

from glamr_amd import _lib
from tests import penetration_common as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


class Launch:
    """One glamr_sdf_penetration call on buffers made beforehand (so it can be recorded into a graph).  Outputs are poisoned before the call
    and the workspace is NaN."""

    def __init__(self, case, want_grad=True, want_mid=True, verts=None):
        v = case['verts'] if verts is None else verts
        self.F, self.P, self.V = v.shape[:3]
        self.G, self.case = case['G'], case
        self.verts = torch.tensor(v, device=DEV)
        self.active = torch.tensor(case['active'], device=DEV)
        self.faces = torch.tensor(case['faces'], device=DEV)
        nan = float('nan')
        self.loss = torch.full((self.F,), nan, device=DEV)
        self.g = torch.full(v.shape, nan, device=DEV) if want_grad else None
        self.phi = torch.full((self.F, self.P, self.G, self.G, self.G), nan, device=DEV) if want_mid else None
        self.boxes = torch.full((self.F, self.P, 2, 3), nan, device=DEV) if want_mid else None
        self.overlap = torch.full((self.F, self.P), -7, dtype=torch.int32, device=DEV) if want_mid else None
        n = _lib.lib().glamr_sdf_workspace_bytes(self.F, self.P, self.V, len(case['faces']), self.G)
        assert n > 0
        self.ws = torch.full((n,), 0xff, dtype=torch.uint8, device=DEV)      # NaN

    def __call__(self):
        c = self.case
        _lib.check(_lib.lib().glamr_sdf_penetration(_lib.ptr(self.verts), _lib.ptr(self.active), _lib.ptr(self.faces), self.F, self.P, self.V, len(c['faces']),
                                                    self.G, c['scale_factor'], c['rho'], _lib.ptr(self.loss), _lib.ptr(self.g), _lib.ptr(self.phi),
                                                    _lib.ptr(self.boxes), _lib.ptr(self.overlap), _lib.ptr(self.ws), _lib.current_stream()))
        return self

    def result(self):
        torch.cuda.synchronize()
        return {k: None if t is None else t.cpu().numpy() for k, t in (('loss', self.loss), ('g_verts', self.g), ('phi', self.phi), ('boxes', self.boxes),
                                                                       ('overlap', self.overlap))}


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_kernels_match_the_fp64_restatement(name):
    """phi over the whole grid, boxes, flags, loss and vertex gradients, each within 16 x the fp32 floor (boxes and flags exactly), with NaN in
    the inactive persons' vertices and the workspace and every output poisoned; exact zeros for inactive and isolated persons; a second call
    gives the same bits; without g_verts and without the intermediate outputs the loss keeps its bits."""
    case = pc.cases()[name]
    got, again = Launch(case)().result(), Launch(case)().result()
    assert all(np.array_equal(got[k], again[k]) for k in got)
    assert all(np.isfinite(got[k]).all() for k in pc.OUTPUTS)
    e, tol = pc.errors(name, got), pc.tol(name)
    print('sdf %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, e[k], tol[k]) for k in pc.OUTPUTS)))
    for k in pc.OUTPUTS:
        assert e[k] <= tol[k], (name, k, e[k], tol[k])
    idle = got['overlap'] == 0
    assert (got['g_verts'][idle] == 0).all() and (got['phi'][idle] == 0).all() and (got['boxes'][case['active'] == 0] == 0).all()
    fwd = Launch(case, want_grad=False)().result()
    lean = Launch(case, want_mid=False)().result()
    assert np.array_equal(fwd['loss'], got['loss']) and np.array_equal(fwd['phi'], got['phi'])
    assert np.array_equal(lean['loss'], got['loss']) and np.array_equal(lean['g_verts'], got['g_verts'])


def test_graph_replay_with_new_vertices_equals_plain_launches():
    case = pc.cases()['third_isolated']
    other = case['verts'][::-1].copy()                                                   # (the frames swapped: other boxes, flags and grids)
    plain = [Launch(case)().result(), Launch(case, verts=other)().result()]
    assert not np.array_equal(plain[0]['loss'], plain[1]['loss'])
    launch = Launch(case)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        launch()                                                                         # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for verts, want in ((other, plain[1]), (case['verts'], plain[0])):
        launch.verts.copy_(torch.tensor(verts, device=DEV))
        for t in (launch.loss, launch.g, launch.phi):
            t.fill_(float('nan'))
        graph.replay()
        got = launch.result()
        assert all(np.array_equal(got[k], want[k]) for k in got)


def test_sdf_loss_module_forward_frames_and_autograd():
    from glamr_amd.lib.models.sdf import SDFLoss
    name = 'third_isolated'
    case, ref = pc.cases()[name], pc.ref64(name)
    tol = pc.tol(name)
    keep = pc.screen(name)[0]
    mod = SDFLoss(case['faces'], grid_size=case['G'], robustifier=True)
    x = torch.tensor(case['verts'], device=DEV, requires_grad=True)
    per_frame = mod.frames(x, torch.tensor(case['active'], device=DEV), scale_factor=case['scale_factor'])
    w = torch.tensor([0.5, -2.0], device=DEV)
    (per_frame * w).sum().backward()
    assert np.abs(per_frame.detach().cpu().numpy() - ref['loss']).max() <= tol['loss']
    want = ref['g_verts'] * w.cpu().numpy().astype(np.float64)[:, None, None, None]
    assert np.abs(x.grad.cpu().numpy() - want)[keep].max() <= 2.0 * tol['g_verts']      # (|w| <= 2)
    # the package's call: one frame, everybody active
    y = torch.tensor(case['verts'][1], device=DEV, requires_grad=True)
    one = mod(y)
    one.backward()
    assert abs(one.item() - ref['loss'][1]) <= tol['loss'] and np.abs(y.grad.cpu().numpy() - ref['g_verts'][1])[keep[1]].max() <= tol['g_verts']
    shifted = mod(torch.tensor(case['verts'][1], device=DEV) - 1.5, translation=torch.full((3, 3), 1.5, device=DEV))
    # (x - 1.5 + 1.5 moves every coordinate by up to an ulp of 2, 2^-22 with both roundings: first order in the reference's gradient)
    assert abs(shifted.item() - ref['loss'][1]) <= tol['loss'] + 2.0 ** -22 * np.abs(ref['g_verts'][1]).sum()
    with torch.no_grad():
        assert torch.equal(mod.frames(x, torch.tensor(case['active'], device=DEV)), per_frame.detach())


# ---- the optimiser's built-in term end to end ------------------------------------------------------------------------------------------------
import copy                                                   # noqa: E402

from glamr_amd.global_recon import extra_loss_schedule as xs, packing      # noqa: E402
from tests import penetration_e2e as pe                       # noqa: E402
from tests.grecon_common import grads_by_name, j_local_from_oracle      # noqa: E402


@pytest.fixture(scope='module')
def priors(asset_root):
    """The body model with the closed hull faces of tests/penetration_e2e.py (the shipped synthetic faces have no inside) and the priors."""
    import os
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    smpl.faces = pe.hull_faces().astype(np.int64)
    return smpl, MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def _model(priors, cfg, **flags):
    from glamr_amd.global_recon.models import model_dict
    from glamr_amd.lib.models.sdf import SDFLoss
    cfg = copy.deepcopy(cfg)
    cfg['grecon_model_specs'].update(flags)
    model = model_dict['global_recon_model'](cfg, DEV, None, smpl=priors[0], mt_model=priors[1])
    if getattr(model, 'sdf_loss', None) is not None:
        assert model.sdf_loss.grid_size == 32 and model.sdf_loss.rho == 1.0 and np.array_equal(model.sdf_loss.faces.numpy(), pe.hull_faces())
        model.sdf_loss = SDFLoss(priors[0].faces, grid_size=pe.GRID, robustifier=True)      # (the grid of the fp64 reference)
    return model


def _packed(asset_root):
    """The port's state after init_data packed for the device."""
    _, ora, data = pe.state(asset_root)
    packed = packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], DEV)
    S, P, T = packed.S, packed.P, packed.T
    pose, beta = torch.zeros((S * P, T, 69)), torch.zeros((S * P, T, 10))
    for pi, idx in enumerate(packed.person_ids[0]):
        pose[pi], beta[pi] = data['person_data'][idx]['smpl_pose'], data['person_data'][idx]['smpl_beta']
    packed.person_arrays = dict(smpl_pose=pose.to(DEV), smpl_beta=beta.to(DEV))
    return data, packed


def _run(asset_root, priors, cfg, extra=None, skip=False, iters=pe.K, make_extra=None):
    data, packed = _packed(asset_root)
    model = _model(priors, cfg)
    model.extra_loss = make_extra(model, packed) if make_extra is not None else extra
    first = {}
    model.extra_loss_grad_hook = lambda stage, it, g: first.setdefault(stage, g.clone()) if it == 0 else None
    xs.ExtraLossSchedule(model, packed, skip_term=skip).run(max_iters=iters)
    torch.cuda.synchronize()
    return model, data, packed, first


def test_end_to_end_against_the_fp64_port(asset_root, golden, priors):
    """K = 5 iterations per stage from the port's state after init_data with `penetration` in every stage's loss_cfg: every stage's first
    gradient, the last stage's variables, the world poses of its last evaluation and penetration_history within 16 x the fp32 port's deviation
    from its fp64 run."""
    cfg = pe.device_cfg()
    model, data, packed, first = _run(asset_root, priors, cfg)
    specs, got = cfg['grecon_model_specs'], {}
    for stage, spec in model.opt_stage_specs.items():
        assert 'penetration' not in spec['loss_cfg']
        got.update({'%s/grad/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, first[stage].cpu(), data, specs, spec['opt_variables']).items()})
        got['%s/history' % stage] = model.penetration_history[stage]
        assert model.penetration_history[stage].shape == (1, pe.K)
    got.update({'%s/param/%s' % (stage, k): v.numpy() for k, v in grads_by_name(packed, packed.t['params'].cpu(), data, specs, spec['opt_variables']).items()})
    Ts = int(data['seq_len'])
    for pi, idx in enumerate(packed.person_ids[0]):
        got['%s/orient/p%d' % (stage, idx)] = packed.t['orient_world'][pi, :Ts].cpu().numpy()
        got['%s/trans/p%d' % (stage, idx)] = packed.t['trans_world'][pi, :Ts].cpu().numpy()
    ref = dict(golden(pe.FIXTURE))
    e = pe.errors(got, ref)
    print('penetration end to end: %s' % ', '.join('%s %.2e (bound %.2e)' % (k, e[k], pe.TOL[k]) for k in pe.KINDS))
    for k in pe.KINDS:
        assert e[k] <= pe.TOL[k], (k, e[k], pe.TOL[k])
    assert model.extra_loss_history == {}


def test_monitor_only_and_a_stage_without_the_term_leave_the_parameters_alone(asset_root, priors):
    """monitor_only computes the value and adds nothing: the parameters are those of the same schedule with the term skipped, bit for bit, and
    the history is that of the active term's first iteration; a stage that does not list the term keeps no history."""
    mon, _, p_mon, _ = _run(asset_root, priors, pe.device_cfg(monitor_only=True), iters=2)
    skipped, _, p_skip, _ = _run(asset_root, priors, pe.device_cfg(), skip=True, iters=2)
    assert np.abs(p_skip.t['params'].cpu().numpy()).max() > 0 and np.array_equal(p_mon.t['params'].cpu().numpy(), p_skip.t['params'].cpu().numpy())
    act, _, p_act, _ = _run(asset_root, priors, pe.device_cfg(), iters=2)
    assert not np.array_equal(p_act.t['params'].cpu().numpy(), p_skip.t['params'].cpu().numpy())
    stages = list(act.opt_stage_specs)
    assert mon.penetration_history[stages[0]][0, 0] == act.penetration_history[stages[0]][0, 0] > 0
    only_last, _, _, _ = _run(asset_root, priors, pe.device_cfg(stages=stages[-1:]), iters=2)
    assert list(only_last.penetration_history) == stages[-1:]


def test_the_term_beside_a_callers_extra_loss_adds_both_gradients(asset_root, priors):
    """First gradient with both = gradient with the built-in term + gradient with the caller's term - gradient with neither.  The VJPs are
    linear, so the four runs differ by fp32 rounding alone: the pose gradients are added before the VJP in one run and after it in the
    others, through prefix sums over 24 frames -- held to 64 ulp of the largest entry.  (The caller's term pulls the persons towards x = 0: a
    term on translation differences has no gradient with respect to the first stage's variables, the initial position and heading.)"""
    user = lambda ctx: 30.0 * ctx.trans_world[..., 0].pow(2).sum((1, 2))      # noqa: E731
    plain = copy.deepcopy(pe.device_cfg())
    for spec in plain['opt_stage_specs'].values():
        spec['loss_cfg'].pop('penetration')
    stage = list(plain['opt_stage_specs'])[0]
    g_both = _run(asset_root, priors, pe.device_cfg(), extra=user, iters=1)[3][stage]
    g_pen = _run(asset_root, priors, pe.device_cfg(), iters=1)[3][stage]
    g_user = _run(asset_root, priors, plain, extra=user, iters=1)[3][stage]
    g_none = _run(asset_root, priors, plain, extra=lambda ctx: 0 * ctx.trans_world.sum((1, 2, 3)), iters=1)[3][stage]
    want = g_pen.double() + g_user.double() - g_none.double()
    scale = max(float(g.abs().max()) for g in (g_pen, g_user, g_none))
    assert float((g_pen - g_none).abs().max()) > 0 and float((g_user - g_none).abs().max()) > 0
    err = float((g_both.double() - want).abs().max())
    print('term + extra_loss: |both - (pen + user - none)| %.2e (bound %.2e; term %.2e, the caller term %.2e)'
          % (err, 64 * 2.0 ** -23 * scale, float((g_pen - g_none).abs().max()), float((g_user - g_none).abs().max())))
    assert err <= 64 * 2.0 ** -23 * scale


def _without_the_term(cfg):
    cfg = copy.deepcopy(cfg)
    for spec in cfg['opt_stage_specs'].values():
        spec['loss_cfg'].pop('penetration')
    return cfg


def _params(packed):
    return packed.t['params'].cpu().numpy()


def test_the_built_in_term_is_just_a_term(asset_root, priors):
    """`penetration` in loss_cfg against the same PenetrationTerm handed in as a caller's extra_loss, times the configured weight: by the chain
    rule both upstream gradients are exactly the weight, so every stage's first gradient and the parameters after two iterations agree bit for
    bit, and extra_loss_history is the weight times penetration_history to the bit (one scene: the sum over scenes adds nothing)."""
    w = pe.WEIGHT

    def as_a_callers(model, packed):
        S, P, T, pa = packed.S, packed.P, packed.T, packed.person_arrays
        term = xs.PenetrationTerm(model, packed, packed.t['vis'].view(S, P, T) > 0, pa['smpl_pose'].view(S, P, T, 69), pa['smpl_beta'].view(S, P, T, 10))
        return lambda ctx: w * term(ctx)
    built_in, _, p_a, first_a = _run(asset_root, priors, pe.device_cfg(weight=w), iters=2)
    callers, _, p_b, first_b = _run(asset_root, priors, _without_the_term(pe.device_cfg()), iters=2, make_extra=as_a_callers)
    assert callers._pen_cfg == {} and callers.penetration_history == {} and built_in.extra_loss_history == {}
    assert list(first_a) == list(first_b) == list(built_in.opt_stage_specs)
    for stage in built_in.opt_stage_specs:
        assert float(first_a[stage].abs().max()) > 0 and torch.equal(first_a[stage], first_b[stage]), stage
        assert np.array_equal(callers.extra_loss_history[stage], np.float32(w) * built_in.penetration_history[stage]), stage
    assert built_in.penetration_history[next(iter(first_a))][0, 0] > 0 and np.array_equal(_params(p_a), _params(p_b))


def test_a_monitor_only_term_beside_a_callers_term_adds_nothing(asset_root, priors):
    """monitor_only beside a caller's extra_loss: first gradients and parameters are those of the caller's term alone, bit for bit, and the
    recorded value is the active term's."""
    user = lambda ctx: 30.0 * ctx.trans_world[..., 0].pow(2).sum((1, 2))      # noqa: E731
    mon, _, p_mon, first_mon = _run(asset_root, priors, pe.device_cfg(monitor_only=True), extra=user, iters=2)
    alone, _, p_alone, first_alone = _run(asset_root, priors, _without_the_term(pe.device_cfg()), extra=user, iters=2)
    act, _, _, _ = _run(asset_root, priors, pe.device_cfg(), iters=2)
    assert list(first_mon) == list(first_alone) == list(mon.opt_stage_specs)
    for stage in mon.opt_stage_specs:
        assert torch.equal(first_mon[stage], first_alone[stage]), stage
    assert np.abs(_params(p_mon)).max() > 0 and np.array_equal(_params(p_mon), _params(p_alone))
    stage = list(mon.opt_stage_specs)[0]
    assert mon.penetration_history[stage][0, 0] == act.penetration_history[stage][0, 0] > 0


def test_refused_combinations_and_entry_points(asset_root, priors):
    from glamr_amd.global_recon.configs import get_config
    in_dict, lat = pe.scene_inputs()
    no_flag = pe.device_cfg()
    no_flag['grecon_model_specs'].pop('flag_use_pen_loss')
    with pytest.raises(ValueError, match='flag_use_pen_loss'):
        _model(priors, no_flag)
    for flags, word in ((dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'), (dict(absolute_heading=True), 'absolute_heading'),
                        (dict(flag_opt_traj_latent=True), 'latent')):
        with pytest.raises(ValueError, match='penetration.*' + word):
            _model(priors, pe.device_cfg(), **flags)
    model = _model(priors, pe.device_cfg())
    rin = model.stage_inputs([in_dict], [lat])
    for name, call in (('optimize_resident', lambda: model.optimize_resident(rin, 1)), ('optimize_stream', lambda: model.optimize_stream([[in_dict]])),
                       ('capture_resident', lambda: model.capture_resident(rin, 1))):
        with pytest.raises(NotImplementedError, match=name + '.*penetration'):
            call()
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='penetration.*person-sharded'):
        xs.ExtraLossSchedule(model, packed).run(max_iters=1)
    # the flag alone (no stage lists the term): the fused schedule, and the loss object the reference builds (:64-65)
    flag_only = copy.deepcopy(get_config(pe.CFG_ID))
    flag_only['grecon_model_specs']['flag_use_pen_loss'] = True
    m = _model(priors, flag_only)
    assert m._pen_cfg == {} and m.sdf_loss is not None
    # optimize() with the term in loss_cfg runs the launch-by-launch schedule from the device's own init_data
    res = model.optimize(in_dict, latents=lat, max_iters=2)
    assert set(model.penetration_history) == set(model.opt_stage_specs) and all(np.isfinite(h).all() and h.shape == (1, 2) for h in model.penetration_history.values())
    assert np.isfinite(np.asarray(res['person_data'][0]['root_trans_world'])).all()
