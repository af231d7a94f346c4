"""Vector headings (grecon_model_specs heading_type = 'vec') on the MI355X: glamr_grecon_run_stage_ext with the heading-vector
fields against the fixtures of the unmodified reference and the fp64 restatement, what the call must not read, determinism, and the
optimiser's entry points."""
import copy

import numpy as np
import pytest
import torch

from glamr_amd.global_recon import packing, stepwise
from glamr_amd.global_recon.configs import get_config
from oracle import make_golden as mg
from tests import heading_vec_common as hv
from tests.test_aux_terms_gpu import _model, priors      # noqa: F401 (priors: a fixture)
from tests.test_heading_vec_ref import check_edges

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT = ('params', 'orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'cam_pose', 'losses', 'heading_vec')
HEADING = dict(terms={'local_traj_dheading_reg': dict(weight=2.0, monitor_only=False), 'local_traj_dheading_reg_new': dict(weight=3.0e3, monitor_only=False)})


@pytest.fixture(scope='module')
def edge(asset_root):
    return hv.EdgeBatch(asset_root)


@pytest.mark.parametrize('case', list(hv.CASES))
def test_case_matches_the_reference(asset_root, golden, case):
    """Cases a-e through the ABI: first-iteration losses and gradients (the dead scalar entries' exactly zero) and the K-step state."""
    failures = hv.check_case(hv.device_runner(), asset_root, golden, case)
    assert not failures, failures


def test_edges_match_the_restatement_and_the_scalar_modes_own_gradient(edge):
    """The edge batch (tests/heading_vec_common.EdgeBatch): every row's vec gradient equals m_e * atan2s_bwd applied to the scalar mode's own
    local_heading / local_dheading gradient at the same heading angles, within 16 x the fp32 restatement's error; poses and projections equal
    the scalar twin's to the bit; the scalar entries' gradients are exactly zero; rows nobody owns are not written."""
    check_edges(edge, hv.device_runner(), torch.device(DEV))


def _edge_launch(edge, K=3, heading=HEADING, prepare=None, vec=True, world=None):
    run, dev = hv.device_runner()
    packed, specs = edge.vec(dev) if vec else edge.scalar_twin(dev)
    spec = packing.split_heading_vec(edge.spec)[0] if vec else edge.spec
    sd = packing.stage_desc(spec, specs, False, niters=K)
    if prepare is not None:
        prepare(packed)
    if vec or world is not None:
        ext, keep = packing.world_ext(world, packed, niters=K, want_grads=True, heading=heading if vec else None)
    else:
        ext, keep = None, {}
    if prepare is not None:
        prepare(packed, ext, keep)
    grads = stepwise.run_stage(packed, sd, True, ext=ext)
    torch.cuda.synchronize()
    out = {k: packed.t[k].cpu().numpy().copy() for k in OUT if k in packed.t}
    out.update(grads=grads.cpu().numpy(), **{k: v.cpu().numpy().copy() for k, v in keep.items() if k in ('hv_grads', 'hv_losses')})
    return out


def test_nan_where_the_call_must_not_read(edge):
    """NaN in the scalar entries of `params`, in the heading array's rows beyond a person's existing ones and in the empty slot, in the moments,
    the gradient record and every output: all results unchanged, the padding untouched."""
    dead = {}

    def poison(packed, ext=None, keep=None):
        if ext is None:
            keep_entries = torch.ones_like(packed.t['params'], dtype=torch.bool)
            for si in range(packed.S):
                for pi in range(packed.P):
                    for k in hv.VEC_KEYS:
                        packing.person_view(packed.t['params'][si], packed.layout, pi, k)[...] = float('nan')
                        packing.person_view(keep_entries[si], packed.layout, pi, k)[...] = False
            dead['live'] = keep_entries.cpu().numpy()
            h = packed.heading_vec_arrays()
            h[0, 72:], h[1, 1:], h[2, 40:], h[3] = float('nan'), float('nan'), float('nan'), float('nan')
            for k in ('orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'losses'):
                packed.t[k].fill_(float('nan'))
        else:
            for k in ('hv_ws', 'hv_losses', 'ws', 'losses'):
                keep[k].fill_(float('nan'))
            g = keep['hv_grads']
            g[0, 72:], g[1, 1:], g[2, 40:], g[3] = float('nan'), float('nan'), float('nan'), float('nan')
    a, b = _edge_launch(edge), _edge_launch(edge, prepare=poison)
    live = dead['live']
    pad = np.zeros(a['heading_vec'].shape[:2], bool)
    pad[0, 72:], pad[1, 1:], pad[2, 40:], pad[3] = True, True, True, True
    assert np.array_equal(a['params'][live], b['params'][live]) and np.isnan(b['params'][~live]).all()
    assert np.array_equal(a['grads'], b['grads']) and np.isfinite(b['grads']).all()
    for k in ('heading_vec', 'hv_grads'):
        assert np.array_equal(a[k][~pad], b[k][~pad]) and np.isnan(b[k][pad]).all(), k
    frames = np.zeros(a['orient_world'].shape[:2], bool)      # the frames t < seq_len of the slots p < n_persons: what a launch writes
    frames[0], frames[1], frames[2, :40] = True, True, True
    for k in ('orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world'):
        assert np.array_equal(a[k][frames], b[k][frames]) and np.isfinite(b[k][frames]).all() and np.isnan(b[k][~frames]).all(), k
    for k in ('losses', 'hv_losses', 'cam_pose'):
        assert np.array_equal(a[k], b[k]) and np.isfinite(b[k]).all(), k
    assert np.abs(a['heading_vec'][0, :72] - edge.inputs[0]['r']).max() > 1e-5      # (the stage moved the variable)


def test_two_calls_are_bit_equal(edge):
    a, b = _edge_launch(edge), _edge_launch(edge)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_flag_off_the_new_fields_are_not_read(edge):
    """Scalar headings through the extension's kernels: with heading_vec NULL, garbage in every other new field changes no bit."""
    def garbage(packed, ext=None, keep=None):
        if ext is not None:
            bad = torch.full((64,), float('nan'), device=DEV)
            keep['bad'] = bad
            ext.heading_vec_grads = ext.heading_vec_workspace = ext.hv_losses = ext.hv_loss_history = bad.data_ptr()
            ext.hv_loss_mask, ext.hv_monitor_mask = 3, 1
            ext.hv_loss_weight[0] = ext.hv_loss_weight[1] = float('nan')
    a = _edge_launch(edge, vec=False, world={})
    b = _edge_launch(edge, vec=False, world={}, prepare=garbage)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_refusals_at_the_abi(edge):
    run, dev = hv.device_runner()
    packed, specs = edge.vec(dev)
    ext, keep = packing.world_ext(None, packed, niters=1, heading={})
    with pytest.raises(RuntimeError, match='ABSOLUTE_HEADING'):
        stepwise.run_stage(packed, packing.stage_desc(packing.split_heading_vec(edge.spec)[0], dict(specs, absolute_heading=True), False, niters=1), False, ext=ext)
    with pytest.raises(RuntimeError, match='LOCAL_DHEADING_REG_NEW'):
        stepwise.run_stage(packed, packing.stage_desc(edge.spec, specs, False, niters=1), False, ext=ext)


def test_together_with_world_dxy(edge):
    """The world-frame residuals of the same extension in the same launch: world_dxy moves, the heading vectors move, and the heading
    gradient of the first evaluation is the one without world_dxy (zero residuals do not change the poses)."""
    world = dict(variables=['world_dxy'], terms={})
    a = _edge_launch(edge, K=1)
    b = _edge_launch(edge, K=1, world=world)
    assert np.array_equal(a['hv_grads'], b['hv_grads'])
    run, dev = hv.device_runner()
    packed, specs = edge.vec(dev)
    ext, keep = packing.world_ext(world, packed, niters=3, heading=HEADING)
    stepwise.run_stage(packed, packing.stage_desc(packing.split_heading_vec(edge.spec)[0], specs, False, niters=3), False, ext=ext)
    torch.cuda.synchronize()
    assert packed.t['world_res'][0, :72, :2].abs().max() > 1e-5 and not packed.t['world_res'][..., 2:].any()
    assert (packed.heading_vec_arrays()[0, :72].cpu() - torch.from_numpy(edge.inputs[0]['r'])).abs().max() > 1e-5


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------------
def _vec_config(cfg_id='glamr_dynamic_multi', **flags):
    cfg = get_config(cfg_id)
    cfg['grecon_model_specs'].update(dict(heading_type='vec', **flags))
    return cfg


def _inputs(case='c'):
    in_dict = hv.in_dict_of(case)
    return in_dict, mg.latents_for(in_dict, hv.SEED)


KEYS = ('params', 'kp_2d_pred', 'trans_world', 'orient_world', 'cam_pose', 'heading_vec')


def test_entry_points_agree_and_report_the_vectors(priors):
    """optimize, optimize_batch, optimize_resident, capture_resident and optimize_stream on case c's scene with the shipped two-stage schedule:
    the same bits; the output dictionaries carry traj_local_heading (2,) and traj_local_dheading (len - 1, 2)."""
    K = 3
    in_dict, lat = _inputs()
    model = _model(priors, _vec_config())
    res = model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=K)
    for pd in res['person_data'].values():
        n = int(pd['fr_end']) - int(pd['fr_start'])
        assert np.asarray(pd['traj_local_heading']).shape == (2,) and np.asarray(pd['traj_local_dheading']).shape == (n - 1, 2)
        assert np.abs(np.asarray(pd['traj_local_heading'])).max() > 1e-4
    batch = model.optimize_batch([copy.deepcopy(in_dict)], [lat], max_iters=K)[0]
    rin = model.stage_inputs([copy.deepcopy(in_dict)], [lat])
    datas, packed = model.optimize_resident(rin, K)
    torch.cuda.synchronize()
    want = {k: packed.t[k].clone() for k in KEYS}
    resident = model.collect(datas, packed)[0]
    streamed = list(model.optimize_stream([[copy.deepcopy(in_dict)]], latents=[[lat]], max_iters=K))[0][0]
    for other in (batch, resident, streamed):
        for pi, pd in res['person_data'].items():
            for key in hv.VEC_KEYS + ('root_trans_world', 'smpl_orient_world', 'traj_local_rot', 'kp_2d_pred'):
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


def test_continue_opt_and_loss_log(priors):
    """Case b through optimize(): the loss line lists both of the variable's terms under the reference's names in loss_cfg's order;
    optimize(continue_opt=True) resumes from the vectors (zero iterations return them unchanged, more move them on); a result of one
    heading_type cannot be continued under the other."""
    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)
    in_dict, lat = _inputs('b')
    cfg = hv.config_of('b')
    model = _model(priors, cfg)
    model.log = Log()
    res = model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=4)
    names = [seg.split(':')[0].strip() for seg in Log.lines[-1].split(' | ')[4:]]
    assert names == list(cfg['opt_stage_specs']['init_opt']['loss_cfg']) and 'local_traj_dheading_reg' in names and 'local_traj_dheading_reg_new' in names
    h = model.heading_vec_loss_history['init_opt']
    assert h.shape == (1, 4, 2) and (h[0, 0] == 0).all() and (h[0, 1:] > 0).all()      # (the vectors start at zero)
    model.log = None
    pd = res['person_data'][0]
    assert np.abs(np.asarray(pd['traj_local_dheading'])).max() > 1e-4
    same = model.optimize(res, continue_opt=True, max_iters=0)['person_data'][0]
    more = model.optimize(res, continue_opt=True, max_iters=2)['person_data'][0]
    for key in hv.VEC_KEYS:
        assert np.array_equal(np.asarray(same[key]), np.asarray(pd[key])) and not np.array_equal(np.asarray(more[key]), np.asarray(pd[key])), key
    with pytest.raises(ValueError, match='heading_type'):
        _model(priors, hv.config_of('b', twin=True)).optimize(res, continue_opt=True, max_iters=1)
    scalar = _model(priors, hv.config_of('c', twin=True)).optimize(copy.deepcopy(_inputs('c')[0]), latents=_inputs('c')[1], max_iters=1)
    with pytest.raises(ValueError, match='heading_type'):
        _model(priors, hv.config_of('c')).optimize(scalar, continue_opt=True, max_iters=1)


def test_person_sharded_batch_is_refused(priors):
    in_dict, lat = _inputs()
    model = _model(priors, _vec_config())
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match="heading_type = 'vec' on a person-sharded"):
        model.run_schedule(packed, 1)
