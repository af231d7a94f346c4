"""MI355X: the attached trajectory prior (flag_attach_traj_pred) -- the stage kernel's dL/d traj_local_pred (glamr_scene_batch.g_traj_local) and
the FK backward (glamr_nets_fk_backward) against fp64 autograd of the port (tests/attach_common.py), and the mode end to end.

End to end the first gradients of both latents and the K-iteration `traj_latent` are held to the port's latent-optimisation loop with the
detach dropped and fp64 priors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from glamr_amd import _lib
from glamr_amd.global_recon import packing
from glamr_amd.utils import synth
from tests import attach_common as ac
from tests.grecon_common import j_local_from_oracle

pytestmark = pytest.mark.gpu


# ---- g_traj_local ---------------------------------------------------------------------------------------------------------------------------
def _stage_launch(asset_root, name, cam_only=False):
    cfg, ora, data = ac.scene_state(asset_root, name)
    stage, spec = ac.stage_of(cfg)
    dev = torch.device('cuda:0')
    L = _lib.lib()
    packed = packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], dev)
    packed.t['g_traj_local'] = torch.full((packed.S * packed.P, packed.T, 11), 7.0, device=dev)      # (the launch must overwrite every entry)
    sd = packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=1)
    if cam_only:
        assert sd.var_mask & packing.VAR_BITS['cam']
        sd.var_mask = packing.VAR_BITS['cam']
    sb = packed.struct()
    grads = torch.zeros_like(packed.t['params'])
    ws = torch.empty(L.glamr_grecon_workspace_bytes(packed.S, packed.P, packed.T), dtype=torch.uint8, device=dev)
    _lib.check(L.glamr_grecon_run_stage(ctypes.byref(sb), ctypes.byref(sd), _lib.ptr(grads), _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    return packed, packed.t['g_traj_local'].cpu().numpy()


@pytest.mark.parametrize('name', list(ac.SCENES))
def test_g_traj_local_matches_autograd_of_the_attached_port(asset_root, name):
    ref = ac.scene_reference(asset_root, name)
    packed, g = _stage_launch(asset_root, name)
    assert packed.P == ac.SCENES[name][2]
    got = {idx: g[pi, :ref[idx].shape[0]] for pi, idx in enumerate(packed.person_ids[0])}
    err = ac.scene_errors(got, ref)
    print('g_traj_local %s: columns 0-8 %.2e (bound %.2e), columns 9-10 %.2e (bound %.2e)'
          % (name, err['row'], ac.G_TRAJ_TOL[name]['row'], err['heading'], ac.G_TRAJ_TOL[name]['heading']))
    for pi, idx in enumerate(packed.person_ids[0]):
        assert (g[pi, ref[idx].shape[0]:] == 0).all()                       # rows beyond a person's frames
    assert err['row'] < ac.G_TRAJ_TOL[name]['row'] and err['heading'] < ac.G_TRAJ_TOL[name]['heading']
    if name == 'two':      # a camera-only stage hands out the same, complete gradient
        _, g_cam = _stage_launch(asset_root, name, cam_only=True)
        assert np.array_equal(g, g_cam)


# ---- FK backward ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def priors(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    dev = torch.device('cuda:0')
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(dev)
    return smpl, MotionTrajJointModel(None, dev, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


@pytest.mark.parametrize('family', ac.FK_FAMILIES)
def test_fk_backward_matches_fp64_autograd(asset_root, priors, family):
    _, mt = priors
    dev = torch.device('cuda:0')
    pose, G = ac.fk_inputs(family)
    ref = ac.fk_reference(asset_root, family)
    p, g = torch.tensor(pose, device=dev), torch.tensor(G, device=dev)
    a = mt.handle.fk_backward(p, list(ac.FK_LENS), g)
    b = mt.handle.fk_backward(p, list(ac.FK_LENS), g)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                                # fixed summation order
    got = a.cpu().numpy()
    for bi, n in enumerate(ac.FK_LENS):
        assert (got[bi, n:] == 0).all()
    err = ac.rel_err(got, ref)
    print('FK backward, %s poses: %.2e (bound %.2e)' % (family, err, ac.FK_TOL[family]))
    assert err < ac.FK_TOL[family]


def test_joint_pos_backpropagates_to_the_pose(asset_root, priors):
    """TrajPredVAE.joint_pos under torch autograd: the gradient of sum(G * joint_pos(pose)) is the FK backward's."""
    _, mt = priors
    dev = torch.device('cuda:0')
    pose, G = ac.fk_inputs('generic')
    p = torch.tensor(pose, device=dev, requires_grad=True)
    j = mt.traj_predictor.joint_pos(p, lens=list(ac.FK_LENS))
    (j * torch.tensor(G, device=dev)).sum().backward()
    assert ac.rel_err(p.grad.cpu().numpy(), ac.fk_reference(asset_root, 'generic')) < ac.FK_TOL['generic']


# ---- the mode, end to end -------------------------------------------------------------------------------------------------------------------
def _model(priors, cfg_id, weight_scale=1.0, **flags):
    from glamr_amd.global_recon.models import model_dict
    from glamr_amd.global_recon.configs import get_config
    smpl, mt = priors
    cfg = get_config(cfg_id)
    cfg['grecon_model_specs'].update(flags)
    for spec in cfg['opt_stage_specs'].values():
        if 'opt_latent_start_iter' in spec:
            spec['opt_latent_start_iter'] = min(spec['opt_latent_start_iter'], 1)
        for c in spec['loss_cfg'].values():
            c['weight'] = c['weight'] * weight_scale
    return model_dict['global_recon_model'](cfg, torch.device('cuda:0'), None, smpl=smpl, mt_model=mt)


ON = dict(flag_opt_motion_latent=True, flag_opt_traj_latent=True, flag_attach_traj_pred=True)


def _first_gradients(model, ref):
    tr = model.latent_trace
    return {i: {'g_traj': tr['g_traj_latent'][i], 'g_motion': tr['g_motion_latent'][i, :ref[i]['g_motion'].shape[0]]} for i in ref}


@pytest.mark.parametrize('name', list(ac.E2E))
def test_attached_mode_matches_the_no_detach_port(priors, golden, name, monkeypatch):
    """Against the port's latent-optimisation loop with the detach dropped and fp64 priors (tests/attach_common.e2e_reference, read from
    tests/golden): the first iteration's d loss / d traj_latent and d loss / d motion_latent, and traj_latent after K iterations per stage,
    each within 16 x the fp32 port's own deviation from that run."""
    cfg_id, in_dict, lat, P = ac.e2e_inputs(name)
    ref, tol, K = ac.from_fixture(golden(ac.FIXTURE), name), ac.E2E_TOL[name], ac.E2E_K
    on = _model(priors, cfg_id, **ON)
    on.latent_trace = {}
    out_on = on.optimize(in_dict, latents=lat, max_iters=K)
    assert on.latent_graph_replays > 0
    off = _model(priors, cfg_id, flag_opt_motion_latent=True, flag_opt_traj_latent=True)
    off.latent_trace = {}
    out_off = off.optimize(in_dict, latents=lat, max_iters=K)
    got = _first_gradients(on, ref)
    for pi in range(P):
        got[pi]['traj_latent'] = out_on['person_data'][pi]['traj_latent']
    err = ac.e2e_errors(got, ref)
    moved = max(float(np.abs(out_on['person_data'][pi]['traj_latent'] - lat[pi]['traj']).max()) for pi in range(P))
    g_off = off.latent_trace['g_motion_latent']
    differs = max(ac.rel_err(g_off[i, :ref[i]['g_motion'].shape[0]], ref[i]['g_motion']) for i in ref)
    print('attached mode %s: first d loss / d traj_latent %.2e (bound %.2e), d loss / d motion_latent %.2e (bound %.2e); traj_latent after %d iterations per stage %.2e '
          '(bound %.2e), moved %.2e; the detached mode\'s d loss / d motion_latent is %.2e from the reference'
          % (name, err['g_traj'], tol['g_traj'], err['g_motion'], tol['g_motion'], K, err['traj_latent'], tol['traj_latent'], moved, differs))
    for pi in range(P):
        assert np.array_equal(out_off['person_data'][pi]['traj_latent'], lat[pi]['traj'])          # flag off: bit-equal to its draw
        assert np.isfinite(out_on['person_data'][pi]['kp_2d_pred']).all()
    assert moved > 1e-4
    assert differs > tol['g_motion']                                         # the FK term is there: the detached gradient is not the reference's
    # upstream loss weights scaled: the first gradients scale with them
    scaled = {}
    for sc in (1e-6, 1e5):
        m = _model(priors, cfg_id, weight_scale=sc, **ON)
        m.latent_trace = {}
        m.optimize(in_dict, latents=lat, max_iters=1)
        g = _first_gradients(m, ref)
        scaled[sc] = {k: max(ac.rel_err(g[i][k] / sc, ref[i][k]) for i in ref) for k in ('g_traj', 'g_motion')}
    print('loss weights x 1e-6 / x 1e5, gradients divided by the factor: %s' % scaled)
    # graph replay equals plain launches, bit for bit
    monkeypatch.setenv('GLAMR_LATENT_GRAPH', '0')
    plain = _model(priors, cfg_id, **ON)
    out_p = plain.optimize(in_dict, latents=lat, max_iters=K)
    assert plain.latent_graph_replays == 0
    for pi in range(P):
        for key in ('traj_latent', 'motion_latent', 'smpl_pose', 'kp_2d_pred', 'root_trans_world', 'traj_local_pred'):
            assert np.array_equal(out_on['person_data'][pi][key], out_p['person_data'][pi][key]), (pi, key)
    assert err['g_traj'] < tol['g_traj'] and err['g_motion'] < tol['g_motion']
    assert err['traj_latent'] < tol['traj_latent']
    for sc, e in scaled.items():
        assert e['g_traj'] < tol['g_traj'] and e['g_motion'] < tol['g_motion'], (sc, e)


def test_the_flag_needs_latent_mode(priors):
    with pytest.raises(ValueError):
        _model(priors, 'glamr_dynamic', flag_attach_traj_pred=True)
