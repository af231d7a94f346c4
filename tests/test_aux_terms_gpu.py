"""glamr_grecon_aux_terms on the MI355X: the kernel-level cases of tests/aux_terms_common.py against the fp64 restatement
within 16 x the fp32 floor -- NaN wherever the kernel must not read, every output poisoned --, store and add mode, two calls bit-equal, a
captured launch replayed on new inputs."""
import numpy as np
import pytest
import torch

from glamr_amd import _lib
from tests import aux_terms_common as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _entry(*a):
    return _lib.lib().glamr_grecon_aux_terms(*a, _lib.current_stream())


def _run(case, **kw):
    out = C.run(case, _entry, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV), lambda t: t.cpu().numpy(), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_kernel_matches_fp64(name):
    case = C.cases()[name]
    rc, got = _run(case)
    assert rc == 0
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)      # (a NaN read anywhere, or a poisoned entry left in place)
    err, tol = C.errors(case, got, C.ref64(name)), C.tol(name)
    print('%s MI355X: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, err[k], tol[k]) for k in C.GROUPS)))
    for k in C.GROUPS:
        assert err[k] <= tol[k], (name, k, err[k], tol[k])
    assert C.outside_groups_zero(case, got)
    # two calls give the same bits
    again = _run(case)[1]
    for k in got:
        assert np.array_equal(got[k], again[k]), (name, k)


@pytest.mark.parametrize('name', ['frame257', 'slots3', 'monitor', 'monitor_all'])
def test_kernel_add_mode(name):
    """accumulate != 0 adds what store mode stores -- one addition per entry -- and touches nothing else.  The device contracts the entry's last
    product into that addition (fma(c, d, old) against fl(fl(c d) + old) on the host runtime, which the CPU test holds to equality): the two
    differ by the product's rounding, 2^-24 |stored|, and one rounding of the sum, 2^-24 |sum|; the bound is twice that.  An entry store mode
    leaves at zero keeps its bits."""
    case = C.cases()[name]
    pre = C.prefill(case)
    store = _run(case)[1]
    rc, add = _run(case, accumulate=1, prefill=pre)
    assert rc == 0
    for k in ('g_trans_world', 'g_cam_pose', 'grads'):
        want = pre[k] + store[k]
        assert np.array_equal(add[k][store[k] == 0], pre[k][store[k] == 0]), (name, k)
        assert (np.abs(add[k].astype(np.float64) - want) <= 2.0 ** -23 * (np.abs(store[k]) + np.abs(want))).all(), (name, k)
    assert np.array_equal(add['values'], store['values'])


def test_captured_launch_replays_on_new_inputs():
    """The call recorded into a torch.cuda.graph and replayed after the inputs changed in place equals a plain launch on those inputs."""
    import ctypes
    case = C.cases()['slots3']
    host = C.host_arrays(case)
    a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in host.items()}
    o = {k: torch.full(s, float('nan'), dtype=torch.float32, device=DEV) for k, s in C.output_shapes(case).items()}
    ws = torch.zeros(case['S'] * case['P'], dtype=torch.int32, device=DEV)
    sb, sd, ad = C.scene_batch(case, {k: v.data_ptr() for k, v in a.items()}), C.stage_desc(case), C.aux_desc(case)

    def launch():
        _lib.check(_lib.lib().glamr_grecon_aux_terms(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), _lib.ptr(a['root_trans_cam']), _lib.ptr(o['values']),
                                                     _lib.ptr(o['g_trans_world']), _lib.ptr(o['g_cam_pose']), _lib.ptr(o['grads']), 0, _lib.ptr(ws), _lib.current_stream()))

    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    # new inputs in the same buffers: the trajectories shifted and scaled, another camera translation
    a['trans_world'].mul_(1.25).add_(0.5)
    a['cam_pose'].view(case['S'], case['T'], 3, 4)[..., 3].add_(0.25)
    changed = {k: v.cpu().numpy() for k, v in a.items()}
    for v in o.values():
        v.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu().numpy() for k, v in o.items()}
    plain = _run(case, arrays=changed)[1]
    for k in plain:
        assert np.array_equal(replayed[k], plain[k]), k
    assert not np.array_equal(replayed['values'], _run(case)[1]['values'])


# ---- end to end: the three fixtures of the unmodified reference (tools/aux_terms_golden.py) and their twins ---------------------------------
import copy      # noqa: E402
import os        # noqa: E402

from oracle import make_golden as mg                                                          # noqa: E402
from glamr_amd.global_recon import extra_loss_schedule as xs, packing                         # noqa: E402
from tests import aux_terms_e2e as ae                                                         # noqa: E402
from tests.grecon_common import kp_err, _rot_err, grads_by_name, j_local_from_oracle          # noqa: E402

# the bounds tests/test_e2e_gpu.py:110 uses per quantity: projected keypoints px, root_trans_world m, smpl_orient_world as a rotation
E2E_FLOOR = (0.01, 1e-5, 1.2e-2)
# aux_loss_history against the values the reference's closure computed at every iteration: the formula tests/grecon_common.py:148 applies to the fused
# terms' first values, 2e-4 of max(1, value), on every entry (achieved on the MI355X: 1.8e-5 at worst, cam_depth_smoothness of glamr_3dpw)
HISTORY_RTOL = 2e-4
TWIN_FACTOR = 4
SUM_ULPS = 64      # a gradient that is a sum of two runs' gradients: ulps of the largest entry (tests/test_penetration_gpu.py)


@pytest.fixture(scope='module')
def priors(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    return smpl, MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def _model(priors, cfg):
    from glamr_amd.global_recon.models import model_dict
    return model_dict['global_recon_model'](copy.deepcopy(cfg), DEV, None, smpl=priors[0], mt_model=priors[1])


_STATE = {}


def _port_state(asset_root, case):
    """The port's state after init_data on the case's scene (computed once, callers pack a deep copy) and its optimiser."""
    from oracle.port import build
    if case not in _STATE:
        ora = build.load_optimizer(asset_root, ae.config_of(case, twin=True))
        in_dict = ae.in_dict_of(case)
        with torch.no_grad():
            _STATE[case] = (ora, ora.init_data(in_dict, latents=mg.latents_for(in_dict, ae.CASES[case]['seed'])))
    return _STATE[case]


def _packed(asset_root, case):
    ora, data = _port_state(asset_root, case)
    data = copy.deepcopy(data)
    return data, packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], DEV)


def _run_schedule(asset_root, priors, case, cfg, extra_loss=None, skip_term=False, first=None):
    """K iterations per stage of ExtraLossSchedule from the port's state; first: {stage: the complete gradient of iteration 0} is filled."""
    data, packed = _packed(asset_root, case)
    model = _model(priors, cfg)
    model.extra_loss = extra_loss
    if first is not None:
        model.extra_loss_grad_hook = lambda stage, it, g: first.setdefault(stage, g.clone()) if it == 0 else None
    xs.ExtraLossSchedule(model, packed, skip_term=skip_term).run(max_iters=ae.CASES[case]['K'])
    torch.cuda.synchronize()
    return model, data, packed


@pytest.mark.parametrize('case', list(ae.CASES))
def test_first_iteration_and_history_match_the_reference(asset_root, golden, priors, case):
    """From the port's state after init_data: the first stage's complete first gradient (stage kernel + the six terms) against the reference's
    autograd with the formula of tests/grecon_common.py:140, the terms' first values with the one of :148, and aux_loss_history of every stage
    against the values the reference's closure computed at every iteration, with the same formula (HISTORY_RTOL)."""
    g, cfg, first = golden(ae.fixture_name(case)), ae.config_of(case), {}
    model, data, packed = _run_schedule(asset_root, priors, case, cfg, first=first)
    stage, spec = next(iter(cfg['opt_stage_specs'].items()))
    named = grads_by_name(packed, first[stage].cpu(), data, cfg['grecon_model_specs'], spec['opt_variables'])
    gmax = max([float(np.abs(g['%s_grad_%s' % (stage, n)]).max()) for n in named if g['%s_grad_%s' % (stage, n)].size] + [0.0])
    for name, val in named.items():
        ref = g['%s_grad_%s' % (stage, name)]
        assert tuple(val.shape) == ref.shape, name
        if ref.size == 0:
            continue
        tol = 3e-4 * max(1.0, float(np.abs(ref).max())) + 2e-5 * gmax
        err = np.abs(val.numpy() - ref).max()
        print('%s %s first gradient %s: abs err %.2e (bound %.2e, largest entry %.3g)' % (case, stage, name, err, tol, np.abs(ref).max()))
        assert err < tol, 'gradient %s: abs err %.2e > %.2e' % (name, err, tol)
    for st, terms in ae.CASES[case]['terms'].items():
        assert sorted(model.aux_loss_history[st]) == sorted(terms)
        for name in terms:
            hist, ref = model.aux_loss_history[st][name], g['%s_hist_%s' % (st, name)]
            assert hist.shape == (1, len(ref))
            if st == stage:
                r0 = float(g['%s_loss_%s' % (st, name)])
                assert abs(hist[0, 0] - r0) <= 2e-4 * max(1.0, abs(r0)), 'loss %s: %g vs %g' % (name, hist[0, 0], r0)
            err = np.abs(hist[0] - ref) / np.maximum(1.0, np.abs(ref))
            print('%s %s history %s: worst %.2e of max(1, value) (bound %.1e)' % (case, st, name, err.max(), HISTORY_RTOL))
            assert (err <= HISTORY_RTOL).all(), (case, st, name, hist[0], ref)
            if name in ae.STRUCTURALLY_ZERO[case]:
                assert not hist.any() and not ref.any()


def _state_errors(case, persons, g):
    P = ae.CASES[case]['P']
    worst = [0.0, 0.0, 0.0]
    for pi in range(P):
        pd = persons[pi]
        vis = g['init_p%d_vis_frames' % pi] & g['init_p0_vis_frames']
        worst[0] = max(worst[0], kp_err(np.asarray(pd['kp_2d_pred']), g['opt_p%d_kp_2d_pred' % pi], vis))
        worst[1] = max(worst[1], float(np.abs(np.asarray(pd['root_trans_world']) - g['opt_p%d_root_trans_world' % pi]).max()))
        worst[2] = max(worst[2], _rot_err(np.asarray(pd['smpl_orient_world']), g['opt_p%d_smpl_orient_world' % pi]))
    return worst


@pytest.mark.parametrize('case', list(ae.CASES))
def test_optimize_matches_the_reference_after_k_steps(asset_root, golden, priors, case):
    """GlobalReconOptimizer.optimize on a reference loss_cfg that lists the six names (device init_data, root_trans_cam from person_arrays): the
    state after K iterations per stage against the unmodified reference, per quantity.  Bound = TWIN_FACTOR x the distance of the SAME entry point
    without the names (the parent's path) from the twin fixture, not below the bound of tests/test_e2e_gpu.py:110; glamr_3dpw: keypoints only
    (the world pose is a gauge there, grecon_common.py:164)."""
    in_dict, c = ae.in_dict_of(case), ae.CASES[case]
    lat = mg.latents_for(in_dict, c['seed'])
    err = {}
    for twin in (True, False):
        out = _model(priors, ae.config_of(case, twin)).optimize(copy.deepcopy(in_dict), latents=lat, max_iters=c['K'])
        err[twin] = _state_errors(case, out['person_data'], golden(ae.fixture_name(case, twin)))
    # measured on the MI355X (kp px / root_trans_world m / orientation), with the terms | twin | bound:
    #   glamr_dynamic       0.0095 / 1.8e-7 / 9.5e-4 | 0.0095 / 1.5e-7 / 9.5e-4 | 0.038 / 1e-5 / 1.2e-2
    #   glamr_static_multi  0.0005 / 6.0e-7 / 7.9e-7 | 0.0004 / 8.2e-7 / 9.5e-7 | 0.01  / 1e-5 / 1.2e-2
    #   glamr_3dpw          0.0018                   | 0.084                    | 0.34   (keypoints only)
    bound = [max(TWIN_FACTOR * t, f) for t, f in zip(err[True], E2E_FLOOR)]
    print('%s K=%d: with the terms kp %.4f px, root_trans_world %.2e m, smpl_orient_world %.2e | twin (parent path) %.4f px, %.2e m, %.2e | bounds %.4f px, %.2e m, %.2e'
          % (case, c['K'], *err[False], *err[True], *bound))
    for q in range(1 if c['cfg_id'] == 'glamr_3dpw' else 3):
        assert err[False][q] <= bound[q], (case, q, err[False][q], bound[q])


@pytest.mark.parametrize('case', ['glamr_dynamic', 'glamr_3dpw'])
def test_all_terms_monitor_only_equal_the_schedule_with_the_terms_skipped(asset_root, priors, case):
    def monitor(name, entry):
        if name in packing.AUX_LOSS_IDS:
            entry['monitor_only'] = True
    cfg, out = ae.config_of(case, edit=monitor), {}
    for skip in (True, False):
        model, _, packed = _run_schedule(asset_root, priors, case, cfg, skip_term=skip)
        out[skip] = packed.t['params'].cpu().numpy()
    assert np.abs(out[True]).max() > 0 and np.array_equal(out[True], out[False])
    assert all(h.any() for st in model.aux_loss_history.values() for n, h in st.items() if n not in ae.STRUCTURALLY_ZERO[case])      # (the values are still recorded)


def test_terms_beside_a_callers_extra_loss_give_the_sum_of_the_gradients(asset_root, priors):
    """glamr_3dpw (camera derived from the persons: both VJP kernels run): the complete first gradient with the six names AND a caller's term on
    the poses and the camera equals the sum of the two runs' minus the stage kernel's own.  The VJP kernels are linear in the adjoints they
    are given, so the runs differ by fp32 rounding alone: the adjoints are added before the VJPs in one run and after them in the others,
    through prefix sums over the frames -- held to 64 ulp of the largest entry, as tests/test_penetration_gpu.py holds the same property."""
    case = 'glamr_3dpw'

    def term(ctx):
        return 50.0 * (ctx.trans_world[..., 2] ** 2).sum((1, 2)) + 20.0 * (ctx.cam_pose[..., 3] ** 2).sum((1, 2))
    zero = lambda ctx: 0.0 * ctx.trans_world.sum((1, 2, 3))
    runs = {}
    for key, (twin, fn) in dict(both=(False, term), aux=(False, None), caller=(True, term), kernel=(True, zero)).items():
        first = {}
        _run_schedule(asset_root, priors, case, ae.config_of(case, twin), extra_loss=fn, first=first)
        runs[key] = {st: v.double().cpu().numpy() for st, v in first.items()}
    stage = next(iter(runs['both']))
    want = runs['aux'][stage] + runs['caller'][stage] - runs['kernel'][stage]
    scale = np.max([np.abs(runs[k][stage]).max() for k in runs])
    err = np.abs(runs['both'][stage] - want).max()
    print('sum of the gradients, %s %s: abs err %.2e, largest entry %.3g, bound %.2e' % (case, stage, err, scale, SUM_ULPS * 2.0 ** -23 * scale))
    assert np.abs(runs['aux'][stage] - runs['kernel'][stage]).max() > 1e-3 * scale and np.abs(runs['caller'][stage] - runs['kernel'][stage]).max() > 1e-3 * scale
    assert err <= SUM_ULPS * 2.0 ** -23 * scale


def test_terms_beside_the_penetration_term_give_the_sum_of_the_gradients(asset_root, priors):
    """The scene of tests/penetration_e2e.py (two persons walking through each other) with `penetration` and two of the six names in every
    stage's loss_cfg: one iteration path, one backward(), and the complete first gradient is the sum of the two runs' minus the stage kernel's."""
    from tests import penetration_e2e as pe
    names = {'traj_trans_smoothness': dict(weight=5.0e2), 'cam_traj_trans': dict(weight=1.0e4, first_frame_weight=10.0)}

    def cfg_of(pen, aux):
        cfg = copy.deepcopy(pe.device_cfg())
        for spec in cfg['opt_stage_specs'].values():
            if not pen:
                spec['loss_cfg'].pop('penetration')
            if aux:
                spec['loss_cfg'].update(copy.deepcopy(names))
        return cfg

    def first_gradient(cfg, extra_loss=None):
        _, ora, data = pe.state(asset_root)
        data = copy.deepcopy(data)
        packed = packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], DEV)
        S, P, T = packed.S, packed.P, packed.T
        pose, beta = torch.zeros((S * P, T, 69)), torch.zeros((S * P, T, 10))
        for pi, idx in enumerate(packed.person_ids[0]):
            pose[pi], beta[pi] = data['person_data'][idx]['smpl_pose'], data['person_data'][idx]['smpl_beta']
        packed.person_arrays = dict(smpl_pose=pose.to(DEV), smpl_beta=beta.to(DEV))      # (no trans_cam: root_trans_cam comes from the host dictionaries)
        model, first = _model(priors, cfg), {}
        model.extra_loss = extra_loss
        model.extra_loss_grad_hook = lambda stage, it, g: first.setdefault(stage, g.clone()) if it == 0 else None
        xs.ExtraLossSchedule(model, packed).run(max_iters=1)
        torch.cuda.synchronize()
        stage = next(iter(first))
        return first[stage].double().cpu().numpy(), model

    g_both, model = first_gradient(cfg_of(True, True))
    assert list(model.penetration_history) == list(model.aux_loss_history) and sorted(next(iter(model.aux_loss_history.values()))) == sorted(names)
    g_pen, g_aux = first_gradient(cfg_of(True, False))[0], first_gradient(cfg_of(False, True))[0]
    g_none = first_gradient(cfg_of(False, False), extra_loss=lambda ctx: 0.0 * ctx.trans_world.sum((1, 2, 3)))[0]
    scale = max(np.abs(g).max() for g in (g_pen, g_aux, g_none))
    err = np.abs(g_both - (g_pen + g_aux - g_none)).max()
    print('penetration + the terms: |both - (pen + aux - none)| %.2e (bound %.2e; penetration %.2e, the terms %.2e)'
          % (err, SUM_ULPS * 2.0 ** -23 * scale, np.abs(g_pen - g_none).max(), np.abs(g_aux - g_none).max()))
    assert np.abs(g_pen - g_none).max() > 0 and np.abs(g_aux - g_none).max() > 0
    assert err <= SUM_ULPS * 2.0 ** -23 * scale


def test_refused_combinations_and_entry_points(asset_root, priors):
    """What extra_loss and the penetration term refuse is refused for the six names too, each message naming the terms; a loss_cfg without any of
    them keeps the fused schedule."""
    case = 'glamr_dynamic'
    in_dict = ae.in_dict_of(case)
    lat = mg.latents_for(in_dict, ae.CASES[case]['seed'])

    def with_flags(**flags):
        cfg = ae.config_of(case)
        cfg['grecon_model_specs'].update(flags)
        return cfg
    for flags, word in ((dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'), (dict(absolute_heading=True), 'absolute_heading'),
                        (dict(flag_opt_traj_latent=True), 'latent')):
        with pytest.raises(ValueError, match='cam_rot_smoothness.*local_traj_dheading_reg.*' + word):
            _model(priors, with_flags(**flags))
    with pytest.raises(ValueError, match="cam_rot_smoothness.*needs 'cam'"):      # glamr_3dpw optimises no camera variables
        cfg = ae.config_of('glamr_3dpw')
        cfg['opt_stage_specs']['main_opt']['loss_cfg']['cam_rot_smoothness'] = dict(weight=1.0)
        _model(priors, cfg)
    model = _model(priors, ae.config_of(case))
    assert all(n not in spec['loss_cfg'] for spec in model.opt_stage_specs.values() for n in packing.AUX_LOSS_IDS)
    rin = model.stage_inputs([in_dict], [lat])
    for name, call in (('optimize_resident', lambda: model.optimize_resident(rin, 1)), ('optimize_stream', lambda: model.optimize_stream([[in_dict]])),
                       ('capture_resident', lambda: model.capture_resident(rin, 1))):
        with pytest.raises(NotImplementedError, match=name + '.*cam_rot_smoothness'):
            call()
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='cam_rot_smoothness.*person-sharded'):
        xs.ExtraLossSchedule(model, packed).run(max_iters=1)
    assert _model(priors, ae.config_of(case, twin=True))._aux_cfg == {}
