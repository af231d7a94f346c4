"""World-frame residuals (`world_dxy` / `world_res` in opt_variables, traj_rot_res / traj_trans_res in loss_cfg) on the host runtime:
the algorithm as csrc/grecon_wide.hip compiles it, with glamr_stage_ext (tests/hostsim/grecon_wide_ext_host.cpp), against fixtures of the
UNMODIFIED reference (tools/world_res_golden.py).  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing, stepwise
from tests import world_res_e2e as we

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def runner():
    return we.hostsim_runner()


@pytest.mark.parametrize('case', list(we.CASES))
def test_case_matches_the_reference(runner, asset_root, golden, case):
    """Every stage's first-iteration losses and gradients (the new variables' included) and the state after K iterations per stage, the new
    tensors included.  Achieved on the host runtime: the table in tests/world_res_e2e.py."""
    failures = we.check_case(runner, asset_root, golden, case)
    assert not failures, failures


@pytest.mark.parametrize('case', [k for k, c in we.CASES.items() if not c.get('first_only')])
def test_case_misses_its_twins_fixture(runner, asset_root, golden, case):
    """The same run held against the fixture of the twin (the schedule without the four names): the comparison can fail.  (Case e compares no
    state after optimisation.)"""
    failures = we.check_case(runner, asset_root, golden, case, against_twin=True)
    assert any('after optimisation' in f for f in failures), failures


def test_ext_null_is_the_plain_call(asset_root):
    """The wide algorithm without a glamr_stage_ext gives what the 8-person build's plain stage gives, bit for bit."""
    from oracle import make_golden as mg
    from oracle.port import build
    from tests import grecon_common as gc
    cfg = we.config_of('c', twin=True)
    in_dict = we.in_dict_of('c')
    ora = build.load_optimizer(asset_root, cfg)
    data = ora.init_data(in_dict, latents=mg.latents_for(in_dict, we.SEED))
    jl = gc.j_local_from_oracle(ora.smpl, data)
    spec = cfg['opt_stage_specs']['main_opt']
    out = []
    for run in (lambda p, sd: gc.hostsim_runner()[0](p, sd, True), lambda p, sd: we.hostsim_runner()[0](p, sd, True, None)[0]):
        packed = packing.PackedScenes([data], [jl], torch.device('cpu'))
        grads = run(packed, packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=3))
        out.append([grads.numpy()] + [packed.t[k].numpy() for k in ('params', 'orient_world', 'trans_world', 'kp_2d_pred', 'losses', 'cam_pose')])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_world_dxy_existing_and_zero_changes_nothing(asset_root):
    """world_dxy exists, is all zero and is not optimised: every output equals the launch without the extension on the same instance."""
    from oracle import make_golden as mg
    from oracle.port import build
    from tests import grecon_common as gc
    cfg = we.config_of('a', twin=True)
    in_dict = we.in_dict_of('a')
    ora = build.load_optimizer(asset_root, cfg)
    data = ora.init_data(in_dict, latents=mg.latents_for(in_dict, we.SEED))
    jl = gc.j_local_from_oracle(ora.smpl, data)
    spec = cfg['opt_stage_specs']['init_opt']
    run = we.hostsim_runner()[0]
    out = []
    for world in (None, {}):
        packed = packing.PackedScenes([data], [jl], torch.device('cpu'))
        packed.has_world_dxy = world is not None
        run(packed, packing.stage_desc(spec, cfg['grecon_model_specs'], False, niters=3), False, world)
        out.append([packed.t[k].numpy() for k in ('params', 'orient_world', 'trans_world', 'kp_2d_pred', 'losses', 'cam_pose')])
        if world is not None:
            assert not packed.t['world_res'].any()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- packing ---------------------------------------------------------------------------------------------------------------------------------
def test_split_world():
    spec = {'opt_variables': ['cam', 'world_res', 'local_xy', 'world_dxy'], 'opt_niters': 1, 'opt_lr': 0.1,
            'loss_cfg': {'kp_2d': {'weight': 1.0}, 'traj_trans_res': {'weight': 3.0, 'monitor_only': True}, 'cam_up_reg': {'weight': 2.0}, 'traj_rot_res': {'weight': 0.5}}}
    rest, world = packing.split_world(spec)
    assert rest['opt_variables'] == ['cam', 'local_xy'] and list(rest['loss_cfg']) == ['kp_2d', 'cam_up_reg'] and rest['loss_cfg']['kp_2d'] is spec['loss_cfg']['kp_2d']
    assert world == dict(variables=['world_res', 'world_dxy'], loss_order=['kp_2d', 'traj_trans_res', 'cam_up_reg', 'traj_rot_res'],
                         terms={'traj_trans_res': dict(weight=3.0, monitor_only=True), 'traj_rot_res': dict(weight=0.5, monitor_only=False)})
    assert spec['opt_variables'] == ['cam', 'world_res', 'local_xy', 'world_dxy'] and len(spec['loss_cfg']) == 4      # (the argument is not modified)
    plain = {'opt_variables': ['cam'], 'opt_niters': 1, 'opt_lr': 0.1, 'loss_cfg': {'kp_2d': {'weight': 1.0}}}
    assert packing.split_world(plain) == (plain, None) and packing.split_world(plain)[0] is plain
    specs = {'s0': plain, 's1': spec}
    rest_specs, cfg = packing.split_world_specs(specs)
    assert rest_specs['s0'] is plain and list(cfg) == ['s1'] and packing.split_world_specs({'s0': plain}) == ({'s0': plain}, {})
    sd = packing.stage_desc(rest, {})
    assert sd.var_mask == packing.VAR_BITS['cam'] | packing.VAR_BITS['local_xy'] and sd.loss_mask == (1 << 0) | (1 << 12)
    # stage_desc itself keeps refusing all four names: they are not part of glamr_stage_desc
    for v in packing.WORLD_VARS:
        with pytest.raises(NotImplementedError, match='optimisation variable .* is not supported by the fused optimiser'):
            packing.stage_desc(dict(plain, opt_variables=[v]), {})
    for n in packing.WORLD_TERMS:
        with pytest.raises(NotImplementedError, match='loss .* is not supported by the fused optimiser'):
            packing.stage_desc(dict(plain, loss_cfg={n: {'weight': 1.0}}), {})


def test_world_ext_and_stage_bookkeeping():
    packed = packing.PackedScenes.empty(2, 3, 7, torch.device('cpu'))
    assert 'world_res' not in packed.t and stepwise.world_stage(packed, None) is None
    world = packing.split_world({'opt_variables': ['world_dxy'], 'loss_cfg': {'traj_rot_res': {'weight': 4.0}}})[1]
    ex, keep = packing.world_ext(world, packed, niters=5, want_grads=True, want_hist=True)
    assert packed.t['world_res'].shape == (6, 7, 8) and not packed.t['world_res'].any()
    assert (ex.var_mask, ex.flags, ex.loss_mask, ex.monitor_mask) == (1, 0, 1, 0) and ex.loss_weight[0] == 4.0 and ex.loss_weight[1] == 0.0
    assert keep['grads'].shape == (6, 7, 8) and keep['loss_history'].shape == (2, 5, 2) and keep['ws'].shape == (6, 7, packing.EXT_WS_FLOATS)
    assert ex.residuals == packed.t['world_res'].data_ptr() and ex.loss_history == keep['loss_history'].data_ptr()
    stepwise.end_world_stage(packed, world, keep)
    assert packed.has_world_dxy and packed.world_res_listed
    # a later stage that lists none of the names still carries the existing world_dxy (:467-468): an extension without variables
    assert stepwise.world_stage(packed, None) == {}
    ex, keep = packing.world_ext({}, packed)
    assert (ex.var_mask, ex.flags, ex.loss_mask) == (0, packing.EXT_HAS_WORLD_DXY, 0) and ex.grads is None and ex.loss_history is None
    ex, _ = packing.world_ext(dict(variables=['world_res'], terms={'traj_trans_res': dict(weight=1.0, monitor_only=True)}), packed)
    assert (ex.var_mask, ex.flags, ex.loss_mask, ex.monitor_mask) == (2, 3, 2, 2)


def test_sharded_schedule_refuses_the_residuals():
    from glamr_amd import parallel
    packed = packing.PackedScenes.empty(1, 2, 6, torch.device('cpu'))
    sched = parallel.PersonShardedSchedule(rank=0, world=1, use_dist=False)
    specs = {'s0': {'opt_variables': ['local_xy', 'world_dxy'], 'opt_niters': 1, 'opt_lr': 0.1, 'loss_cfg': {'kp_2d': {'weight': 1.0}}}}
    with pytest.raises(NotImplementedError, match='world_dxy.*person-sharded'):
        sched.run(packed, specs, {})
    # ... and the specs a model holds, from which the names have been taken off (what a caller passes on as model.opt_stage_specs)
    stripped = packing.split_world_specs(specs)[0]
    assert stripped['s0']['opt_variables'] == ['local_xy'] and packing.has_world(stripped) and not packing.has_world({'s0': dict(specs['s0'], opt_variables=['local_xy'])})
    with pytest.raises(NotImplementedError, match='world_dxy.*person-sharded'):
        sched.run(packed, stripped, {})


def test_the_library_sizes_the_extension_workspace():
    """packing.EXT_WS_FLOATS is what glamr_grecon_ext_workspace_bytes (the kernel's EXT_WS) gives per slot and frame."""
    assert _lib.lib().glamr_grecon_ext_workspace_bytes(2, 3, 7) == 2 * 3 * 7 * packing.EXT_WS_FLOATS * 4


def test_struct_matches_the_header():
    code = '#include <stdio.h>\n#include "glamr_hip.h"\nint main(){printf("%zu %d %d\\n", sizeof(glamr_stage_ext), GLAMR_EXT_FLOATS, GLAMR_EXT_NUM_LOSSES);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'p.c'), 'w') as f:
            f.write(code)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 'p')]).split()]
    assert out == [ctypes.sizeof(_lib.StageExt), packing.EXT_FLOATS, len(packing.WORLD_TERMS)]
