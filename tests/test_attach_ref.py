"""CPU: the reference of the attached trajectory prior (tests/attach_common.py) -- its fp32-vs-fp64 rounding levels (the source of every
device bound), mutations that the bounds must catch, and the stage ALGORITHM's dL/d traj_local_pred (grecon_algo.hpp on the single-threaded
host runtime of tests/hostsim) against it, so the column rule is checked without a GPU as well."""
import ctypes

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import attach_common as ac, traj_ref_common as tc
from tests.grecon_common import j_local_from_oracle


@pytest.fixture(scope='module')
def refs(asset_root):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ac.scene_reference(asset_root, name)
        return cache[name]
    return get


@pytest.mark.parametrize('name', list(ac.SCENES))
def test_rounding_level_of_the_port_gradient(asset_root, refs, name):
    with tc.single_thread():
        r32 = ac.scene_reference(asset_root, name, torch.float32)
    floor = ac.scene_errors(r32, refs(name))
    print('dL/d traj_local_pred %s: fp32 port vs fp64 port %s (constants %s)' % (name, floor, ac.G_TRAJ_FLOOR[name]))
    for k, v in floor.items():
        assert ac.G_TRAJ_FLOOR[name][k] / 2 < v <= ac.G_TRAJ_FLOOR[name][k] * 2, (k, v)
    for idx, g in refs(name).items():
        assert np.abs(g[:, :9]).max() > 0 and np.abs(g[:, 9:]).max() > 0          # the attached port does carry a gradient to every column group


@pytest.mark.parametrize('name', ['one', 'two'])
@pytest.mark.parametrize('mut,group', [('heading', 'heading'), ('reg', 'row'), ('mask', 'heading')])
def test_mutations_exceed_the_bounds(asset_root, refs, name, mut, group):
    err = ac.scene_errors(ac.scene_reference(asset_root, name, mut=mut), refs(name))
    print('%s, %s: %s' % (name, ac.MUTATIONS[mut], err))
    assert err[group] > 10 * ac.G_TRAJ_TOL[name][group]


def _host_launch(asset_root, name, cam_only=False):
    from tests import hostsim
    fn = hostsim.build('grecon_traj_grad_host').hostsim_grecon_run_stage_traj_grad
    fn.argtypes = [ctypes.POINTER(_lib.SceneBatch), ctypes.POINTER(_lib.StageDesc), ctypes.c_void_p]
    cfg, ora, data = ac.scene_state(asset_root, name)
    stage, spec = ac.stage_of(cfg)
    packed = packing.PackedScenes([data], [j_local_from_oracle(ora.smpl, data)], torch.device('cpu'))
    packed.t['g_traj_local'] = torch.full((packed.S * packed.P, packed.T, 11), 7.0)
    sd = packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=1)
    if cam_only:
        assert sd.var_mask & packing.VAR_BITS['cam']
        sd.var_mask = packing.VAR_BITS['cam']
    sb = packed.struct()
    grads = torch.zeros_like(packed.t['params'])
    assert fn(ctypes.byref(sb), ctypes.byref(sd), ctypes.c_void_p(grads.data_ptr())) == 0
    return packed, packed.t['g_traj_local'].numpy().copy()


@pytest.mark.parametrize('name', ['one', 'two'])
def test_stage_algorithm_on_the_host_runtime(asset_root, refs, name):
    ref = refs(name)
    packed, g = _host_launch(asset_root, name)
    got = {idx: g[pi, :ref[idx].shape[0]] for pi, idx in enumerate(packed.person_ids[0])}
    err = ac.scene_errors(got, ref)
    print('g_traj_local on the host runtime, %s: %s (bounds %s)' % (name, err, ac.G_TRAJ_TOL[name]))
    for pi, idx in enumerate(packed.person_ids[0]):
        assert (g[pi, ref[idx].shape[0]:] == 0).all()
    assert err['row'] < ac.G_TRAJ_TOL[name]['row'] and err['heading'] < ac.G_TRAJ_TOL[name]['heading']
    _, g_cam = _host_launch(asset_root, name, cam_only=True)
    assert np.array_equal(g, g_cam)                                           # independent of the stage's variable set


@pytest.mark.parametrize('family', ac.FK_FAMILIES)
def test_fk_backward_reference(asset_root, family):
    r64 = ac.fk_reference(asset_root, family)
    with tc.single_thread():
        r32 = ac.fk_reference(asset_root, family, torch.float32)
    floor = ac.rel_err(r32, r64)
    mut = ac.rel_err(ac.fk_reference(asset_root, family, mut='fk_leaf'), r64)
    print('FK backward %s: fp32 port vs fp64 port %.3e (constant %.1e); %s: %.2e' % (family, floor, ac.FK_FLOOR[family], ac.MUTATIONS['fk_leaf'], mut))
    assert ac.FK_FLOOR[family] / 2 < floor <= 2 * ac.FK_FLOOR[family]
    assert mut > 10 * ac.FK_TOL[family]
    for b, n in enumerate(ac.FK_LENS):
        assert (r64[b, n:] == 0).all() and np.abs(r64[b, :n]).max() > 0


def test_abi_has_the_two_additions():
    assert 'glamr_nets_fk_backward' in _lib.exported_symbols()
    assert 'g_traj_local' in [n for n, _ in _lib.SceneBatch._fields_]


# ---- the mode end to end ------------------------------------------------------------------------------------------------------------------
def test_kink_list_and_cap(asset_root):
    """Candidates whose fp64 forward puts a ReLU pre-activation within KINK of zero are the ones listed, at most a quarter of them."""
    for name, (_, _, _, _, seeds) in ac.E2E.items():
        kinked = tuple(s for s in seeds if ac.relu_margin(asset_root, name, s) < ac.KINK)
        print('%s: candidates %s, left out %s' % (name, seeds, kinked))
        assert kinked == tuple(ac.E2E_KINKED[name])
        assert 4 * len(kinked) <= len(seeds)


@pytest.mark.parametrize('name', list(ac.E2E))
def test_end_to_end_reference(asset_root, golden, name):
    """The no-detach port run with fp64 priors: its fp32 rounding levels (the source of the device bounds), the committed results the device
    tests read, the detach's effect (`traj_latent.grad is None` with it, non-zero without it) and the mutation 'FK term not added'."""
    r64 = ac.e2e_reference(asset_root, name)
    with tc.single_thread():
        r32 = ac.e2e_reference(asset_root, name, torch.float32)
    floor = ac.e2e_errors(r32, r64)
    print('end to end %s: fp32 port vs fp64 port %s (constants %s)' % (name, floor, ac.E2E_FLOOR[name]))
    for k, v in floor.items():
        assert ac.E2E_FLOOR[name][k] / 2 < v <= 2 * ac.E2E_FLOOR[name][k], (k, v)
    fix = ac.e2e_errors(ac.from_fixture(golden(ac.FIXTURE), name), r64)
    assert all(fix[k] <= ac.E2E_FLOOR[name][k] / 16 for k in fix), fix          # the file holds this run
    lat = ac.e2e_inputs(name)[2]
    det = ac.e2e_reference(asset_root, name, K=1, attached=False)
    mut = ac.e2e_reference(asset_root, name, K=1, mut='no_fk')
    for idx, r in r64.items():
        assert det[idx]['g_traj'] is None and np.array_equal(det[idx]['traj_latent'], np.asarray(lat[idx]['traj'], np.float64))
        assert np.abs(r['g_traj']).max() > 0 and np.abs(r['traj_latent'] - lat[idx]['traj']).max() > 1e-4
    e_det = max(ac.rel_err(det[i]['g_motion'], r64[i]['g_motion']) for i in r64)
    e_mut = max(ac.rel_err(mut[i]['g_motion'], r64[i]['g_motion']) for i in r64)
    print('%s: d loss / d motion_latent, detached port %.2e, %s %.2e (bound %.2e)' % (name, e_det, ac.MUTATIONS['no_fk'], e_mut, ac.E2E_TOL[name]['g_motion']))
    assert e_det > 10 * ac.E2E_TOL[name]['g_motion'] and e_mut > 10 * ac.E2E_TOL[name]['g_motion']
