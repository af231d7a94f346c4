"""MI355X: the latent regularisers (motion_latent_reg / traj_latent_reg; glamr_latent_reg) -- the kernel through the C ABI on a
synthetic padded batch, and the latent-optimisation mode with the terms against the fp64 port (tests/latent_reg_common.py, read from
tests/golden/latent_reg_e2e.npz), against torch.optim.Adam to the bit in detached mode, graph replay against plain launches and the path
without a regulariser against itself."""
import os

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from tests import latent_reg_common as lc

pytestmark = pytest.mark.gpu

ABSENT, MONITOR, ACTIVE = _lib.LATENT_REG_ABSENT, _lib.LATENT_REG_MONITOR, _lib.LATENT_REG_ACTIVE
WEIGHTS = (0.3, 7.0)
SENTINEL = 123.25


# ---- the kernel through the ABI ------------------------------------------------------------------------------------------------------------
def _launch(meps, teps, nw, modes, add, g_m, g_t, n_rows=0, row=None):
    dev = torch.device('cuda:0')
    L = _lib.lib()
    S, P = lc.KERNEL_WINDOWS.shape
    values = torch.full((S, 2), SENTINEL, device=dev)
    hist = torch.full((S, n_rows, 2), SENTINEL, device=dev) if n_rows else None
    row_t = None if row is None else torch.tensor([row], dtype=torch.int32, device=dev)
    nw_dev = torch.as_tensor(nw, device=dev)
    _lib.check(L.glamr_latent_reg(S, P, meps.shape[1], _lib.ptr(meps), _lib.ptr(teps), _lib.ptr(nw_dev), _lib.ptr(nw), WEIGHTS[0], WEIGHTS[1], modes[0], modes[1],
                                  add[0], add[1], _lib.ptr(g_m), _lib.ptr(g_t), _lib.ptr(values), _lib.ptr(hist), n_rows, _lib.ptr(row_t), _lib.current_stream()))
    torch.cuda.synchronize()
    return values.cpu().numpy(), None if hist is None else hist.cpu().numpy()


@pytest.fixture(scope='module')
def kin():
    dev = torch.device('cuda:0')
    meps, teps, nw = lc.kernel_inputs()
    return torch.tensor(meps, device=dev), torch.tensor(teps, device=dev), nw, lc.kernel_reference(meps, teps, nw, WEIGHTS)


def test_kernel_store_mode_values_and_gradient(kin):
    meps, teps, nw, (values, rows, g32, g64, real_m, real_t) = kin
    g_m, g_t = torch.full_like(meps, SENTINEL), torch.full_like(teps, SENTINEL)
    got, _ = _launch(meps, teps, nw, (ACTIVE, ACTIVE), (0, 0), g_m, g_t)
    err = np.abs(got - values) / values
    print('values: fp32 kernel vs fp64 %.2e (bound %.2e)' % (err.max(), lc.KERNEL_VALUE_TOL))
    assert np.isfinite(got).all() and err.max() < lc.KERNEL_VALUE_TOL
    for g, ref32, ref64, real in ((g_m.cpu().numpy(), g32[0], g64[0], real_m), (g_t.cpu().numpy(), g32[1], g64[1], real_t)):
        assert np.isfinite(g).all()
        assert np.array_equal(g.view(np.uint32), ref32.view(np.uint32))            # fl(fl(w / n) * 2 z), padded rows and empty slots +0
        assert (g[~real] == 0).all()
        rel = np.abs(g[real].astype(np.float64) - ref64[real]) / np.abs(ref64[real])
        print('gradient vs fp64: %.2e relative per entry (bound 2^-22 = %.2e)' % (rel.max(), 2.0 ** -22))
        assert rel.max() <= 2.0 ** -22
    # a second launch on the same inputs: identical bits
    g_m2, g_t2 = torch.full_like(meps, SENTINEL), torch.full_like(teps, SENTINEL)
    got2, _ = _launch(meps, teps, nw, (ACTIVE, ACTIVE), (0, 0), g_m2, g_t2)
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and torch.equal(g_m, g_m2) and torch.equal(g_t, g_t2)


def test_kernel_add_mode_leaves_padded_rows_alone(kin):
    meps, teps, nw, (values, rows, g32, g64, real_m, real_t) = kin
    rng = np.random.default_rng(11)
    base_m, base_t = rng.normal(size=tuple(meps.shape)).astype(np.float32), rng.normal(size=tuple(teps.shape)).astype(np.float32)
    base_m[~real_m], base_t[~real_t] = SENTINEL, SENTINEL
    g_m, g_t = torch.tensor(base_m, device=meps.device), torch.tensor(base_t, device=meps.device)
    got, _ = _launch(meps, teps, nw, (ACTIVE, ACTIVE), (1, 1), g_m, g_t)
    assert np.isfinite(got).all()
    for g, base, ref32, real in ((g_m.cpu().numpy(), base_m, g32[0], real_m), (g_t.cpu().numpy(), base_t, g32[1], real_t)):
        assert np.isfinite(g).all()
        assert (g[~real] == SENTINEL).all()                                          # untouched
        assert np.array_equal(g[real].view(np.uint32), (base[real] + ref32[real]).astype(np.float32).view(np.uint32))
    # one latent added, the other stored
    g_m, g_t = torch.tensor(base_m, device=meps.device), torch.tensor(base_t, device=meps.device)
    _launch(meps, teps, nw, (ACTIVE, ACTIVE), (0, 1), g_m, g_t)
    assert np.array_equal(g_m.cpu().numpy().view(np.uint32), g32[0].view(np.uint32))
    assert (g_t.cpu().numpy()[~real_t] == SENTINEL).all()


def test_kernel_monitor_and_absent_modes(kin):
    meps, teps, nw, (values, rows, g32, g64, real_m, real_t) = kin
    g_m, g_t = torch.full_like(meps, SENTINEL), torch.full_like(teps, SENTINEL)
    got, _ = _launch(meps, teps, nw, (MONITOR, ABSENT), (0, 0), g_m, g_t)
    assert (np.abs(got[:, 0] - values[:, 0]) / values[:, 0]).max() < lc.KERNEL_VALUE_TOL          # monitor_only: the value ...
    assert (got[:, 1] == SENTINEL).all()                                                          # absent: neither value ...
    assert (g_m == SENTINEL).all() and (g_t == SENTINEL).all()                                    # ... nor any gradient
    got, _ = _launch(meps, teps, nw, (ABSENT, ACTIVE), (0, 0), g_m, g_t)
    assert (got[:, 0] == SENTINEL).all() and (g_m == SENTINEL).all()
    assert np.array_equal(g_t.cpu().numpy().view(np.uint32), g32[1].view(np.uint32))


@pytest.mark.parametrize('row', [0, 3])
def test_kernel_history_row_comes_from_the_device_index(kin, row):
    meps, teps, nw, (values, rows, g32, g64, real_m, real_t) = kin
    g_m, g_t = torch.zeros_like(meps), torch.zeros_like(teps)
    got, hist = _launch(meps, teps, nw, (ACTIVE, MONITOR), (0, 0), g_m, g_t, n_rows=4, row=row)
    assert np.array_equal(hist[:, row].view(np.uint32), got.view(np.uint32))
    others = [r for r in range(4) if r != row]
    assert (hist[:, others] == SENTINEL).all()


def test_kernel_argument_checks(kin):
    meps, teps, nw, _ = kin
    L = _lib.lib()
    g_m, g_t = torch.zeros_like(meps), torch.zeros_like(teps)
    values = torch.zeros((3, 2), device=meps.device)
    nw_dev = torch.as_tensor(nw, device=meps.device)

    def call(nw_host, n_win_max=3, g_m_=g_m):
        return L.glamr_latent_reg(3, 3, n_win_max, _lib.ptr(meps), _lib.ptr(teps), _lib.ptr(nw_dev), _lib.ptr(nw_host), 1.0, 1.0, ACTIVE, ACTIVE, 0, 0, _lib.ptr(g_m_),
                                  _lib.ptr(g_t), _lib.ptr(values), None, 0, None, _lib.current_stream())
    assert call(nw, n_win_max=2) == -1 and b'n_win_max' in L.glamr_last_error()      # a slot with more windows than the padding holds
    empty = nw.copy()
    empty[6:] = 0
    assert call(empty) == -1 and b'no person' in L.glamr_last_error()
    assert call(nw, g_m_=None) == -1 and b'g_meps' in L.glamr_last_error()
    torch.cuda.synchronize()


# ---- the mode ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def priors(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    dev = torch.device('cuda:0')
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(dev)
    return smpl, MotionTrajJointModel(None, dev, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def _model(priors, cfg, log=None, **flags):
    from glamr_amd.global_recon.models import model_dict
    smpl, mt = priors
    cfg['grecon_model_specs'].update(flags)
    return model_dict['global_recon_model'](cfg, torch.device('cuda:0'), log, smpl=smpl, mt_model=mt)


BOTH = dict(flag_opt_motion_latent=True, flag_opt_traj_latent=True)


def _run(priors, name, attached, **kw):
    cfg_id, in_dict, lat, P = lc.case_inputs(name)
    m = _model(priors, lc.case_config(name, **kw), flag_attach_traj_pred=attached, **BOTH)
    m.latent_trace = {}
    out = m.optimize(in_dict, latents=lat, max_iters=lc.K)
    return m, out, lat, P


def test_detached_traj_latent_follows_torch_adam_to_the_bit(priors):
    """Detached mode (the unmodified reference), traj_latent_reg only, case (a): the regulariser is traj_latent's whole gradient, so K iterations
    are torch.optim.Adam on the CPU in fp32 fed fl(fl(w / n) * 2 z) -- bit for bit (our Adam is torch's, tests/test_adam_exact.py).  Without
    the term traj_latent stays bit-equal to its draw."""
    cfg_id, in_dict, lat, P = lc.case_inputs('a')
    w = lc.CASES['a'][6]['traj_latent_reg']
    cfg = lc.case_config('a', terms=('traj_latent_reg',))
    m = _model(priors, cfg, flag_opt_traj_latent=True)
    out = m.optimize(in_dict, latents=lat, max_iters=lc.K)
    z = torch.tensor(np.asarray(lat[0]['traj'], np.float32).reshape(1, 128), requires_grad=True)
    c = (np.float32(w) / np.float32(1.0)).astype(np.float32)
    for stage, spec in cfg['opt_stage_specs'].items():
        opt = torch.optim.Adam([z], lr=spec['opt_lr'], betas=(0.9, 0.999))
        for _ in range(min(lc.K, spec['opt_niters'])):
            z.grad = torch.tensor(c * (np.float32(2) * z.detach().numpy()))
            opt.step()
    got = out['person_data'][0]['traj_latent']
    assert not np.array_equal(got, lat[0]['traj'])
    assert np.array_equal(got.view(np.uint32), z.detach().numpy().view(np.uint32))
    h = m.latent_loss_history['init_opt']
    assert h.shape == (1, lc.K, 2) and (h[:, :, 0] == 0).all() and (np.diff(h[0, :, 1]) < 0).all()


@pytest.mark.parametrize('attached', [True, False], ids=['attached', 'detached'])
@pytest.mark.parametrize('name', list(lc.CASES))
def test_mode_with_regularisers_matches_the_fp64_port(priors, golden, name, attached, monkeypatch):
    ref, tol = lc.from_fixture(golden(lc.FIXTURE), name, attached), lc.TOL[(name, attached)]
    m, out, lat, P = _run(priors, name, attached)
    assert m.latent_graph_replays > 0
    tr = m.latent_trace
    got = {'values': {s: h[0] for s, h in m.latent_loss_history.items()}}
    for i in range(P):
        nwin = ref[i]['motion_latent'].shape[0]
        got[i] = {'g_traj': tr['g_traj_latent'][i], 'g_motion': tr['g_motion_latent'][i, :nwin],
                  'traj_latent': out['person_data'][i]['traj_latent'], 'motion_latent': out['person_data'][i]['motion_latent']}
        assert (tr['g_motion_latent'][i, nwin:] == 0).all()                          # padded window rows: no gradient
    err = lc.errors(got, ref)
    print('latent regularisers, case %s, %s: %s' % (name, 'attached' if attached else 'detached',
                                                   ', '.join('%s %.2e (bound %.2e)' % (k, err[k], tol[k]) for k in lc.KEYS)))
    first_stage = list(ref['values'])[0]
    assert np.allclose(tr['latent_reg'][0], ref['values'][first_stage][0], rtol=tol['values'], atol=0)          # latent_trace: the first iteration's two values
    # graph replay equals plain launches, bit for bit
    monkeypatch.setenv('GLAMR_LATENT_GRAPH', '0')
    p, out_p, _, _ = _run(priors, name, attached)
    assert p.latent_graph_replays == 0
    for pi in range(P):
        for key in ('traj_latent', 'motion_latent', 'smpl_pose', 'kp_2d_pred', 'root_trans_world', 'traj_local_pred'):
            assert np.array_equal(out['person_data'][pi][key], out_p['person_data'][pi][key]), (pi, key)
    for s in m.latent_loss_history:
        assert np.array_equal(m.latent_loss_history[s], p.latent_loss_history[s])
    for k in lc.KEYS:
        assert err[k] < tol[k], (k, err[k], tol[k])


def test_monitor_only_terms_change_nothing(priors):
    """Both terms at monitor_only: the values are reported, and latents and parameters are bit-equal to a run without the terms."""
    cfg_id, in_dict, lat, P = lc.case_inputs('b')
    mon, out_m, _, _ = _run(priors, 'b', True, monitor=lc.TERMS)
    off, out_o, _, _ = _run(priors, 'b', True, terms=())
    assert off.latent_loss_history == {} and 'latent_reg' not in off.latent_trace
    for s, h in mon.latent_loss_history.items():
        assert h.shape == (1, lc.K, 2) and (h > 0).all()
    for pi in range(P):
        for key in ('traj_latent', 'motion_latent', 'smpl_pose', 'kp_2d_pred', 'root_trans_world', 'traj_local_pred', 'smpl_orient_world'):
            assert np.array_equal(out_m['person_data'][pi][key], out_o['person_data'][pi][key]), (pi, key)
    for key in ('cam_pose', 'cam_pose_inv'):
        if key in out_o:
            assert np.array_equal(out_m[key], out_o[key]), key


def test_log_lines_carry_the_terms(priors):
    class Log:
        lines = []

        def info(self, s):
            self.lines.append(s)
    cfg_id, in_dict, lat, P = lc.case_inputs('a')
    m = _model(priors, lc.case_config('a'), log=Log(), **BOTH)
    m.optimize(in_dict, latents=lat, max_iters=2)
    lines = [ln for ln in Log.lines if 'motion_latent_reg' in ln]
    assert len(lines) == 2 and all('traj_latent_reg' in ln and 'init_opt' in ln for ln in lines)
