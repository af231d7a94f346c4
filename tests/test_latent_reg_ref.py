"""CPU: the reference of the latent regularisers (tests/latent_reg_common.py) -- its fp32-vs-fp64 rounding levels (the source of every device
bound), the committed expectations, the candidate seeds, the weights' share of the gradient, mutations the bounds must catch, the two
functions against the unmodified reference where it is available, and the misconfigurations GlobalReconOptimizer refuses."""
import numpy as np
import pytest
import torch

from glamr_amd.global_recon import packing
from glamr_amd.global_recon.configs import get_config
from tests import latent_reg_common as lc, traj_ref_common as tc


def test_candidate_seeds_and_cap(asset_root):
    for name, case in lc.CASES.items():
        seeds = case[5]
        kinked = tuple(s for s in seeds if lc.relu_margin(asset_root, name, s) < lc.KINK)
        print('%s: candidates %s, left out %s' % (name, seeds, kinked))
        assert kinked == tuple(lc.KINKED[name]) == ()                     # the lists hold no seed at a ReLU kink
        assert 4 * len(kinked) <= len(seeds)


@pytest.mark.parametrize('name,attached', lc.RUNS)
def test_rounding_floors_and_fixture(asset_root, golden, name, attached):
    r64 = lc.reference(asset_root, name, attached=attached)
    with tc.single_thread():
        r32 = lc.reference(asset_root, name, torch.float32, attached=attached)
    floor, const = lc.errors(r32, r64), lc.FLOOR[(name, attached)]
    print('case %s, %s: fp32 port vs fp64 port %s (constants %s)' % (name, 'attached' if attached else 'detached', floor, const))
    for k, v in floor.items():
        assert const[k] / 2 < v <= 2 * const[k], (k, v)
    fix = lc.errors(lc.from_fixture(golden(lc.FIXTURE), name, attached), r64)
    assert all(fix[k] <= const[k] / 16 for k in fix), fix                # the file holds this run
    K = lc.K
    for stage, v in r64['values'].items():
        assert v.shape == (K, 2) and (v > 0).all()


@pytest.mark.parametrize('name', list(lc.CASES))
def test_weights_leave_both_parts_of_the_gradient_visible(asset_root, name):
    """At the first iteration with priors (attached run) the regulariser is between 10 % and 90 % of each latent's gradient norm:
    share = |g_reg| / (|g_reg| + |g - g_reg|), with g_reg = 2 w z / n at the latents that iteration started from."""
    w = lc.CASES[name][6]
    full = lc.reference(asset_root, name, attached=True)
    data_only = lc.reference(asset_root, name, attached=True, mut='skip_all')
    for i in (i for i in full if i != 'values'):
        for k in ('g_motion', 'g_traj'):
            g_reg = full[i][k] - data_only[i][k]
            share = np.linalg.norm(g_reg) / (np.linalg.norm(g_reg) + np.linalg.norm(data_only[i][k]))
            print('case %s person %d %s: regulariser share %.2f (weights %s)' % (name, i, k, share, w))
            assert 0.1 < share < 0.9


# (mutation, case, attached, reference keyword arguments of BOTH runs, quantities it touches)
MUTATION_RUNS = [('slots', 'a', True, {}, ('g_motion', 'motion_latent', 'values')),
                 ('padded', 'b', True, {}, ('g_motion', 'motion_latent', 'values')),
                 ('skip', 'a', False, {}, ('traj_latent', 'motion_latent')),
                 ('no_weight', 'a', True, {}, ('g_traj', 'g_motion')),
                 ('monitor', 'a', False, {'monitor': ('traj_latent_reg',)}, ('traj_latent',)),
                 ('no_traj_step', 'a', False, {}, ('traj_latent',))]


@pytest.mark.parametrize('mut,name,attached,kw,touched', MUTATION_RUNS)
def test_mutations_exceed_the_bounds(asset_root, mut, name, attached, kw, touched):
    ref = lc.reference(asset_root, name, attached=attached, **kw)
    bad = lc.reference(asset_root, name, attached=attached, mut=mut, **kw)
    if mut == 'no_traj_step':      # (no gradient is recorded for a latent that is not a parameter)
        for i in (i for i in bad if i != 'values'):
            bad[i] = dict(bad[i], g_traj=ref[i]['g_traj'])
    err, tol = lc.errors(bad, ref), lc.TOL[(name, attached)]
    mult = {k: err[k] / tol[k] for k in touched}
    print('%s (case %s, %s): moved by %s tolerances' % (lc.MUTATIONS[mut], name, 'attached' if attached else 'detached', {k: '%.1f' % v for k, v in mult.items()}))
    assert min(mult.values()) >= 2


@pytest.mark.reference
@pytest.mark.skipif(not __import__('oracle.ref_harness', fromlist=['x']).available(), reason='/root/reference is not present')
def test_functions_equal_the_unmodified_reference():
    import os
    from oracle import ref_harness as rh
    keep_cwd = os.getcwd()
    try:
        os.chdir(rh.setup())                  # the reference globs its configs / assets relative to the cwd
        from global_recon.models import loss_func
    finally:
        os.chdir(keep_cwd)
    assert loss_func.loss_func_dict['motion_latent_reg'] is loss_func.motion_latent_reg_loss
    assert loss_func.loss_func_dict['traj_latent_reg'] is loss_func.traj_latent_reg_loss
    rng = np.random.default_rng(3)
    for persons in ((2,), (2, 1), (3, 1, 4)):
        lat = {i: (torch.tensor(rng.normal(size=(n, 128))), torch.tensor(rng.normal(size=(1, 128)))) for i, n in enumerate(persons)}
        ours = {'person_data': {i: {'in_motion_latent': m, 'in_traj_latent': t} for i, (m, t) in lat.items()}}
        theirs = {'person_data': {i: {'motion_latent': m, 'traj_latent': t} for i, (m, t) in lat.items()}}
        assert float(lc.motion_latent_reg_loss(ours, {})) == float(loss_func.motion_latent_reg_loss(theirs, {}))
        assert float(lc.traj_latent_reg_loss(ours, {})) == float(loss_func.traj_latent_reg_loss(theirs, {}))


# ---- misconfigurations ---------------------------------------------------------------------------------------------------------------------
def _construct(flags, terms):
    from glamr_amd.global_recon.models import model_dict
    cfg = get_config('glamr_dynamic')
    cfg['grecon_model_specs'].update(flags)
    for spec in cfg['opt_stage_specs'].values():
        for t in terms:
            spec['loss_cfg'][t] = dict(weight=1.0)
    # (smpl and mt_model given: the constructor touches no device)
    return model_dict['global_recon_model'](cfg, torch.device('cuda:0'), None, smpl=object(), mt_model=object())


@pytest.mark.parametrize('flags,terms,flag', [({}, ('motion_latent_reg',), 'flag_opt_motion_latent'),
                                              ({}, ('traj_latent_reg',), 'flag_opt_traj_latent'),
                                              ({'flag_opt_motion_latent': True}, ('traj_latent_reg',), 'flag_opt_traj_latent'),
                                              ({'flag_opt_traj_latent': True}, ('motion_latent_reg',), 'flag_opt_motion_latent'),
                                              ({'flag_opt_motion_latent': True}, lc.TERMS, 'flag_opt_traj_latent')])
def test_a_regulariser_whose_latent_is_no_parameter_is_refused(flags, terms, flag):
    with pytest.raises(ValueError) as e:
        _construct(flags, terms)
    assert flag in str(e.value) and any(t in str(e.value) for t in terms)


def test_valid_combinations_construct():
    m = _construct({'flag_opt_motion_latent': True, 'flag_opt_traj_latent': True}, lc.TERMS)
    assert m.latent_mode and m.latent_loss_history == {}
    _construct({'flag_opt_traj_latent': True}, ('traj_latent_reg',))


@pytest.mark.parametrize('term', lc.TERMS)
def test_stage_desc_still_refuses_the_names(term):
    cfg = get_config('glamr_dynamic')
    spec = cfg['opt_stage_specs']['init_opt']
    spec['loss_cfg'][term] = dict(weight=1.0)
    with pytest.raises(NotImplementedError):
        packing.stage_desc(spec, cfg['grecon_model_specs'])
    rest, regs = packing.split_latent_regs(spec['loss_cfg'])
    assert term not in rest and len(rest) == len(spec['loss_cfg']) - 1
    packing.stage_desc(dict(spec, loss_cfg=rest), cfg['grecon_model_specs'])


def test_abi_has_the_entry_point():
    from glamr_amd import _lib
    assert 'glamr_latent_reg' in _lib.exported_symbols()


def test_kernel_value_floor():
    """The fp32 sum of squares of the kernel test's sizes against fp64 (numpy's pairwise fp32 sum and a sequential fp32 loop): the recorded floor."""
    meps, teps, nw = lc.kernel_inputs()
    worst = 0.0
    for s in range(3):
        z = np.concatenate([meps[k, :nw[k]].reshape(-1) for k in range(3 * s, 3 * s + 3)])
        ref = float((z.astype(np.float64) ** 2).sum())
        seq = np.float32(0)
        for x in z:
            seq = np.float32(seq + np.float32(x * x))
        worst = max(worst, abs(float((z * z).sum(dtype=np.float32)) - ref) / ref, abs(float(seq) - ref) / ref)
    print('fp32 sum of squares vs fp64: %.3e (constant %.1e)' % (worst, lc.KERNEL_VALUE_FLOOR))
    assert lc.KERNEL_VALUE_FLOOR / 2 < worst <= 2 * lc.KERNEL_VALUE_FLOOR


def test_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    """glamr_latent_reg's argument checks run before any HIP call (the error convention of tests/test_abi.py)."""
    import ctypes
    from glamr_amd import build, _lib
    build.build_library()
    L = _lib.lib()
    nw = lc.KERNEL_WINDOWS.reshape(-1).copy()
    A = ctypes.c_void_p(16)                                 # any non-null, 16-byte aligned value: the checks come first

    def call(nw_host, n_win_max=3, mode=2, g_m=A, hist=None):
        return L.glamr_latent_reg(3, 3, n_win_max, A, A, A, _lib.ptr(nw_host), 1.0, 1.0, mode, mode, 0, 0, g_m, A, A, hist, 0, None, None)
    assert call(nw, n_win_max=2) == -1 and b'n_win_max' in L.glamr_last_error()
    empty = nw.copy()
    empty[6:] = 0
    assert call(empty) == -1 and b'no person' in L.glamr_last_error()
    assert call(nw, g_m=None) == -1 and b'g_meps' in L.glamr_last_error()
    assert call(nw, mode=3) == -1 and b'mode' in L.glamr_last_error()
    assert call(nw, hist=A) == -1 and b'history' in L.glamr_last_error()
    assert call(nw, mode=0) == 0                            # both terms absent: nothing to do
