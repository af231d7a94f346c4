"""World-frame residuals (`world_dxy` / `world_res` in opt_variables, traj_rot_res / traj_trans_res in loss_cfg) on the MI355X:
glamr_grecon_run_stage_ext against the fixtures of the unmodified reference and against its host twin, the two instances against each other,
padding and determinism, and the optimiser's entry points."""
import copy

import numpy as np
import pytest
import torch

from glamr_amd.global_recon import packing, stepwise
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth
from oracle import make_golden as mg
from tests import grecon_common as gc
from tests import world_res_e2e as we
from tests.test_aux_terms_gpu import _model, priors      # noqa: F401 (priors: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT = ('params', 'orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'cam_pose', 'losses', 'world_res')


@pytest.mark.parametrize('case', list(we.CASES))
def test_case_matches_the_reference(asset_root, golden, case):
    """The four cases through the ABI: first-iteration losses and gradients and the K-step state (tests/world_res_e2e.check_case)."""
    failures = we.check_case(we.device_runner(), asset_root, golden, case)
    assert not failures, failures


_STATE = {}


def _port_state(asset_root, cfg_id, T, P, trim=None, gap=None):
    """The port's state after init_data (computed once per scene; callers pack a deep copy).  `gap`: synth.make_in_dict's (None: its own)."""
    from oracle.port import build
    key = (cfg_id, T, P, trim, gap)
    if key not in _STATE:
        cfg = get_config(cfg_id)
        in_dict = synth.make_in_dict(seed=we.SEED, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model(), gap=gap)
        if trim:
            synth.trim_person(in_dict, *trim)
        ora = build.load_optimizer(asset_root, cfg)
        with torch.no_grad():
            data = ora.init_data(in_dict, latents=mg.latents_for(in_dict, we.SEED))
        _STATE[key] = (cfg, data, gc.j_local_from_oracle(ora.smpl, data))
    cfg, data, jl = _STATE[key]
    return cfg, copy.deepcopy(data), jl


WORLD_ALL = dict(variables=['world_dxy', 'world_res'], terms={'traj_rot_res': dict(weight=1.0e2, monitor_only=False), 'traj_trans_res': dict(weight=1.0e2, monitor_only=False)})


def _launch(asset_root, cfg_id, T, P, K, world, dev, run, stage=None, trim=None, prepare=None, drop=('world_dheading',), gap=None):
    """One stage of K iterations with the extension `world` (None: the plain launch) from the port's state; -> {name: numpy array} of OUT."""
    cfg, data, jl = _port_state(asset_root, cfg_id, T, P, trim, gap)
    packed = packing.PackedScenes([data], [jl], dev)
    spec = copy.deepcopy(cfg['opt_stage_specs'][stage or list(cfg['opt_stage_specs'])[-1]])
    spec['opt_variables'] = [v for v in spec['opt_variables'] if v not in drop]      # (beside world_dheading the orientation residual is inert)
    if world is not None:
        packed.world_arrays()
    if prepare is not None:
        prepare(packed)
    run(packed, packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=K), False, world)
    return {k: packed.t[k].detach().cpu().numpy().copy() for k in OUT if k in packed.t}


def _dist(a, b, keys=('params', 'trans_world', 'orient_world', 'world_res')):
    return {k: float(np.abs(a[k].astype(np.float64) - b[k]).max()) for k in keys if k in a and k in b}


@pytest.mark.parametrize('cfg_id,T,P,K', [('glamr_dynamic', 513, 1, 2), ('glamr_dynamic_multi', 48, 9, 2)], ids=['T513-P1', 'T48-P9'])
def test_device_against_the_host_twin(asset_root, cfg_id, T, P, K):
    """T = 513 (one more than the workgroup: frames take two passes) and 9 persons (two scan calls): device against the host twin, bound = 4 x the
    distance the same launch WITHOUT the extension shows between device and host runtime (floored at 1e-6: two launches may agree exactly).

    The scenes have no detection gap (synth's own gives T = 513 one of 60 frames; T = 48 has none), as cases b and d (tests/world_res_e2e.py).
    Adam's first step is -lr . sign(g).  In an unseen frame the orientation residual's only gradient is traj_rot_smoothness's on an interpolated
    trajectory: on the host runtime 35 of its entries in frames 100-159 are below 1e-6 of the largest (9e-6 beside 333), the size of fp32
    rounding there, so two correct runtimes take opposite signs and end 2 . lr = 2e-3 apart whatever the kernel does.  Without the gap the
    smallest entry is 1e-2 (3e-5 of the largest), a thousand times the rounding."""
    (hrun, hdev), (drun, ddev) = we.hostsim_runner(), we.device_runner()
    gap = (0, 0) if T >= 80 else None      # (below 80 frames synth makes no gap of its own)
    plain = _dist(_launch(asset_root, cfg_id, T, P, K, None, ddev, drun, gap=gap), _launch(asset_root, cfg_id, T, P, K, None, hdev, hrun, gap=gap))
    dev_out, host_out = _launch(asset_root, cfg_id, T, P, K, WORLD_ALL, ddev, drun, gap=gap), _launch(asset_root, cfg_id, T, P, K, WORLD_ALL, hdev, hrun, gap=gap)
    ext = _dist(dev_out, host_out)
    print('%s T=%d P=%d K=%d device - host: plain %s | with the residuals %s' % (cfg_id, T, P, K, plain, ext))
    assert np.abs(host_out['world_res']).max() > 1e-4 and np.isfinite(dev_out['world_res']).all()
    for k in ('params', 'trans_world', 'orient_world'):
        assert ext[k] <= max(4 * plain[k], 1e-6), (k, ext[k], plain[k])
    assert ext['world_res'] <= max(4 * max(plain['trans_world'], plain['orient_world']), 1e-6), (ext, plain)


def test_workspace_and_lite_arena_instances_agree(asset_root):
    """A launch that records the loss history runs the workspace instance, one without the lite-arena instance: equal parameters and residuals
    to 1e-5 of an Adam movement of 4e-4, and the history's last row is the reported value.  Achieved on the MI355X: parameters 1.3e-7,
    residuals 2.5e-8, 0.00018 px."""
    drun, ddev = we.device_runner()
    hist = {}

    def with_history(packed):
        packed.t['loss_history'] = torch.zeros((1, 4, len(packing.LOSS_IDS)), dtype=torch.float32, device=DEV)
        hist['packed'] = packed

    def run(packed, sd, want_grads, world):
        out = drun(packed, sd, want_grads, world)
        hist.setdefault('keep', []).append(out[1])
        return out
    a = _launch(asset_root, 'glamr_static_multi', 120, 2, 4, WORLD_ALL, ddev, run, gap=(0, 0))
    b = _launch(asset_root, 'glamr_static_multi', 120, 2, 4, WORLD_ALL, ddev, run, prepare=with_history, gap=(0, 0))
    # Two instances of one algorithm are two compilations of it, not the same bits -- without the extension either (tests/test_loss_log_gpu.py).
    # The stage's opt_lr is 1e-4: four Adam steps move no entry by more than 4e-4, and a wrong moment offset or a swapped residual column
    # shows at that size.  Bound 1e-5, a fortieth of it: what rounding can make of it is the last bit of a parameter of size 1 to 8 per step
    # (4 x 4.8e-7 = 2e-6) plus lr times the relative rounding of a gradient summed over 120 frames (1e-4 x 1e-5); 1e-3 px is eight last bits of
    # a pixel coordinate near 1920.  The scene has no detection gap (test_device_against_the_host_twin), so no entry's first step hangs on the
    # sign of rounding noise.
    d = _dist(a, b, ('params', 'world_res', 'kp_2d_pred', 'trans_world', 'orient_world'))
    print('workspace instance - lite-arena instance, 4 iterations: %s' % d)
    assert d['kp_2d_pred'] < 1e-3 and d['params'] < 1e-5 and d['world_res'] < 1e-5, d
    assert np.abs(a['world_res']).max() > 1e-5
    lite, ws = hist['keep']
    h = ws['loss_history'].cpu().numpy()
    assert h.shape == (1, 4, 2) and h[0, 0].max() == 0 and (h[0, 1:] > 0).all()      # (the residuals start at zero)
    assert np.array_equal(h[0, -1], ws['losses'].cpu().numpy()[0])
    assert np.allclose(ws['losses'].cpu().numpy(), lite['losses'].cpu().numpy(), rtol=2e-4, atol=0)      # (check_case's bound on a loss value)


def test_padding_is_never_read_or_written(asset_root):
    """NaN in the residual arrays beyond seq_len and in the scene's empty slot, every output poisoned: same results, padding untouched."""
    drun, ddev = we.device_runner()
    cfg, data, jl = _port_state(asset_root, 'glamr_static_multi', 120, 2)
    outs = []
    for poison in (False, True):
        packed = packing.PackedScenes([data, _port_state(asset_root, 'glamr_static', 90, 1)[1]], [jl, _port_state(asset_root, 'glamr_static', 90, 1)[2]], ddev)
        res = packed.world_arrays()
        res[:, :, :] = 0.01
        if poison:
            res[2:4, 90:] = float('nan')      # scene 1: 90 of 120 frames
            res[3] = float('nan')             # ... and one of two slots
            for k in ('orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'losses'):
                packed.t[k].fill_(float('nan'))
        spec = copy.deepcopy(cfg['opt_stage_specs']['main_opt'])
        spec['opt_variables'].remove('world_dheading')
        packed.has_world_dxy = True
        _, keep = drun(packed, packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=3), False, WORLD_ALL)
        outs.append(({k: packed.t[k].cpu().numpy().copy() for k in OUT}, keep['losses'].cpu().numpy()))
    (a, la), (b, lb) = outs
    assert np.array_equal(la, lb) and np.isfinite(lb).all()
    assert np.array_equal(a['params'], b['params'])
    live = np.ones(a['world_res'].shape[:2], bool)
    live[2:4, 90:] = False
    live[3] = False
    assert np.array_equal(a['world_res'][live], b['world_res'][live]) and np.isnan(b['world_res'][~live]).all() and (a['world_res'][~live] == np.float32(0.01)).all()
    for k in ('trans_world', 'orient_world'):
        assert np.array_equal(a[k][live], b[k][live]), k


def test_two_launches_are_bit_equal_and_an_empty_extension_changes_nothing(asset_root):
    """Two launches agree to the bit; and with world_dxy existing, all zero and not optimised every output equals the launch of the same
    kernels with an extension that holds nothing (neither variable exists, no term)."""
    drun, ddev = we.device_runner()
    a = _launch(asset_root, 'glamr_dynamic', 120, 1, 5, WORLD_ALL, ddev, drun)
    b = _launch(asset_root, 'glamr_dynamic', 120, 1, 5, WORLD_ALL, ddev, drun)
    for k in OUT:
        assert np.array_equal(a[k], b[k]), k
    none = _launch(asset_root, 'glamr_dynamic', 120, 1, 5, {}, ddev, drun, drop=())
    zero = _launch(asset_root, 'glamr_dynamic', 120, 1, 5, {}, ddev, drun, drop=(), prepare=lambda packed: setattr(packed, 'has_world_dxy', True))
    for k in OUT:
        assert np.array_equal(none[k], zero[k]), k
    assert not zero['world_res'].any()


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------------
def _inputs(case):
    in_dict = we.in_dict_of(case)
    return in_dict, mg.latents_for(in_dict, we.SEED)


KEYS = ('params', 'kp_2d_pred', 'trans_world', 'orient_world', 'cam_pose', 'world_res')


def test_entry_points_agree_and_report_the_residuals(priors):
    """optimize, optimize_batch, optimize_resident, capture_resident and optimize_stream on case c (world_dxy from the first stage, carried
    through the second): the same params and residuals; the output dictionaries carry the new keys; a run without the names carries none."""
    case, K = 'c', 3
    in_dict, lat = _inputs(case)
    model = _model(priors, we.config_of(case))
    res = model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=K)
    for pd in res['person_data'].values():
        assert np.asarray(pd['world_dxy']).shape == (120, 2) and np.abs(np.asarray(pd['world_dxy'])).max() > 1e-3
        assert np.asarray(pd['smpl_orient_world_res']).shape == (120, 3) and not np.any(pd['smpl_orient_world_res']) and not np.any(pd['root_trans_world_res'])
    batch = model.optimize_batch([copy.deepcopy(in_dict)], [lat], max_iters=K)[0]
    rin = model.stage_inputs([copy.deepcopy(in_dict)], [lat])
    datas, packed = model.optimize_resident(rin, K)
    torch.cuda.synchronize()
    want = {k: packed.t[k].clone() for k in KEYS}
    resident = model.collect(datas, packed)[0]
    streamed = list(model.optimize_stream([[copy.deepcopy(in_dict)]], latents=[[lat]], max_iters=K))[0][0]
    for other in (batch, resident, streamed):
        for pi, pd in res['person_data'].items():
            for key in ('world_dxy', 'smpl_orient_world_res', 'root_trans_world_res', 'root_trans_world', 'smpl_orient_world', 'traj_local_rot'):
                assert np.array_equal(np.asarray(pd[key]), np.asarray(other['person_data'][pi][key])), key
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        model.optimize_resident(rin, K)
    torch.cuda.synchronize()
    rg = model.capture_resident(rin, max_iters=K, stream=st, check=True)
    for k in KEYS:
        rg.packed.t[k].fill_(float('nan'))
    torch.cuda.synchronize()
    rg.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(rg.packed.t[k], want[k]), k
    plain = _model(priors, we.config_of(case, twin=True)).optimize(copy.deepcopy(in_dict), latents=lat, max_iters=1)
    assert not any(k in pd for pd in plain['person_data'].values() for k in packing.WORLD_KEYS)


def test_continue_opt_resumes_from_the_residuals(priors):
    """optimize(continue_opt=True) packs world_dxy and the residual tensors of the dictionary it is given: zero further iterations return them
    unchanged, and more iterations move them on."""
    case = 'b'
    in_dict, lat = _inputs(case)
    model = _model(priors, we.config_of(case))
    res = model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=4)
    pd = res['person_data'][0]
    assert 'world_dxy' not in pd and np.abs(np.asarray(pd['smpl_orient_world_res'])).max() > 1e-3
    same = model.optimize(res, continue_opt=True, max_iters=0)['person_data'][0]
    more = model.optimize(res, continue_opt=True, max_iters=2)['person_data'][0]
    for key in ('smpl_orient_world_res', 'root_trans_world_res'):
        assert np.array_equal(np.asarray(same[key]), np.asarray(pd[key])) and not np.array_equal(np.asarray(more[key]), np.asarray(pd[key])), key
    # ... and they are applied: the same dictionary without the residual keys packs zeros, and the forward pass of the same variables
    # (trans = base + res, :452-454) then lacks exactly the translation residual.  (A forward-only launch on a stage's final variables does not
    # return the poses that stage reported, with or without the residuals -- DESIGN.md 22 --, so `same` is not held against `pd`.)
    bare = copy.deepcopy(res)
    for key in ('smpl_orient_world_res', 'root_trans_world_res'):
        del bare['person_data'][0][key]
    bare = model.optimize(bare, continue_opt=True, max_iters=0)['person_data'][0]
    moved = np.asarray(same['root_trans_world']) - np.asarray(bare['root_trans_world'])
    assert np.abs(np.asarray(pd['root_trans_world_res'])).max() > 1e-3 and np.abs(moved - np.asarray(pd['root_trans_world_res'])).max() < 1e-5
    # the orientation is reported as the angle-axis sum itself (orient = angle-axis(R_w) + res)
    turned = np.asarray(same['smpl_orient_world']) - np.asarray(bare['smpl_orient_world'])
    assert np.abs(turned - np.asarray(pd['smpl_orient_world_res'])).max() < 1e-5


def test_loss_log_lists_the_terms_in_loss_cfg_order(priors):
    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)
    case = 'b'
    in_dict, lat = _inputs(case)
    cfg = we.config_of(case)
    model = _model(priors, cfg)
    model.log = Log()
    model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=3)
    names = [seg.split(':')[0].strip() for seg in Log.lines[-1].split(' | ')[4:]]
    assert names == list(cfg['opt_stage_specs']['init_opt']['loss_cfg']) and names[-2:] == ['traj_rot_res', 'traj_trans_res']
    h = model.world_loss_history['init_opt']
    assert h.shape == (1, 3, 2) and (h[0, 0] == 0).all() and (h[0, 1:] > 0).all()


def test_refusals(priors):
    """Where the optimiser is made: the penetration term, the six aux terms, flag_aux_on_device, the latent-optimisation mode,
    flag_opt_vis_local_rot, absolute_heading; extra_loss where it is set; a person-sharded batch where the schedule starts."""
    base = we.config_of('a')
    word = 'world-frame residuals'

    def cfg_with(flags=None, loss=None):
        cfg = copy.deepcopy(base)
        cfg['grecon_model_specs'].update(flags or {})
        cfg['opt_stage_specs']['init_opt']['loss_cfg'].update(loss or {})
        return cfg
    for cfg, other in ((cfg_with(dict(flag_use_pen_loss=True), {'penetration': dict(weight=1.0)}), 'penetration'),
                       (cfg_with(loss={'traj_trans_smoothness': dict(weight=1.0)}), 'traj_trans_smoothness'),
                       (cfg_with(dict(flag_aux_on_device=True)), 'flag_aux_on_device'),
                       (cfg_with(dict(flag_opt_traj_latent=True)), 'latent-optimisation'), (cfg_with(dict(flag_opt_motion_latent=True)), 'latent-optimisation'),
                       (cfg_with(dict(flag_opt_vis_local_rot=True)), 'flag_opt_vis_local_rot'), (cfg_with(dict(absolute_heading=True)), 'absolute_heading')):
        with pytest.raises(NotImplementedError, match='%s.*%s' % (word, other)):
            _model(priors, cfg)
    model = _model(priors, base)
    with pytest.raises(NotImplementedError, match='extra_loss.*' + word):
        model.extra_loss = lambda ctx: (ctx.trans_world ** 2).sum((1, 2, 3))
    in_dict, lat = _inputs('a')
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match=word + '.*person-sharded'):
        model.run_schedule(packed, 1)
    # ... and the entry point itself
    packed.world_arrays()
    ext, keep = packing.world_ext(dict(variables=['world_dxy'], terms={}), packed)
    with pytest.raises(RuntimeError, match='person-sharded'):
        stepwise.run_stage(packed, packing.stage_desc(model.opt_stage_specs['init_opt'], model.specs, niters=1), False, ext=ext)
    # a model without the names that is given a result carrying world_dxy to continue: the launch-by-launch schedules do not know it
    res = _model(priors, base).optimize(copy.deepcopy(in_dict), latents=lat, max_iters=1)
    assert 'world_dxy' in res['person_data'][0]
    plain = _model(priors, we.config_of('a', twin=True))
    plain.extra_loss = lambda ctx: (ctx.trans_world ** 2).sum((1, 2, 3))
    with pytest.raises(NotImplementedError, match='existing world_dxy.*extra_loss'):
        plain.optimize(res, continue_opt=True, max_iters=1)
