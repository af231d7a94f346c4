"""Vector headings (grecon_model_specs heading_type = 'vec') on the host runtime: the algorithm as csrc/grecon_wide.hip compiles
it, with the heading-vector fields of glamr_stage_ext (tests/hostsim/grecon_wide_headvec_host.cpp), against fixtures of the UNMODIFIED reference
(tools/heading_vec_golden.py) and against the fp64 restatement of tests/heading_vec_common.py.  No GPU."""
import copy
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import heading_vec_common as hv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
OUT = ('params', 'orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'losses', 'cam_pose')


@pytest.fixture(scope='module')
def runner():
    return hv.hostsim_runner()


@pytest.fixture(scope='module')
def edge(asset_root):
    return hv.EdgeBatch(asset_root)


# ---- end to end against the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(hv.CASES))
def test_case_matches_the_reference(runner, asset_root, golden, case):
    """Every stage's first-iteration losses and gradients (the vec variables' included, the dead scalar entries' exactly zero) and the state
    after K iterations per stage with the case's tests/grecon_common.KSTEP_TOL row."""
    failures = hv.check_case(runner, asset_root, golden, case)
    assert not failures, failures


@pytest.mark.parametrize('case', [k for k, c in hv.CASES.items() if not c.get('first_only')])
def test_case_misses_its_scalar_twins_fixture(runner, asset_root, golden, case):
    """The same run held against the fixture of the scalar twin: the comparison can fail, the flag is visible."""
    failures = hv.check_case(runner, asset_root, golden, case, against_twin=True)
    assert any('after optimisation' in f for f in failures), failures


def test_twin_schedule_matches_the_twins_fixture(runner, asset_root, golden):
    """The unchanged path (scalar headings, no heading fields in the extension) on case c's twin: the fixture pair is consistent.  (Case b's
    twin lists local_traj_dheading_reg, which the scalar path runs off the stage kernel.)"""
    failures = hv.check_case(runner, asset_root, golden, 'c', run_twin=True)
    assert not failures, failures


# ---- the edges against the restatement -----------------------------------------------------------------------------------------------------------
def _edge_runs(edge, runner, dev):
    """One gradient evaluation (niters 1, lr 0) of the edge batch with vector headings and of its scalar twin -> per slot (vec gradient (n, 2),
    angle gradient g_h (n,)), the two runs' outputs, the vec run's regulariser values and its scalar-entry gradients."""
    run, _ = runner
    heading = dict(terms={'local_traj_dheading_reg': dict(weight=2.0, monitor_only=False), 'local_traj_dheading_reg_new': dict(weight=3.0e3, monitor_only=False)})
    out = {}
    pv, specs_v = edge.vec(dev)
    spec = packing.split_heading_vec(edge.spec)[0]
    sd = packing.stage_desc(spec, specs_v, False, niters=1)
    sd.lr = 0.0
    gv, keep = run(pv, sd, True, heading)
    ps, specs_s = edge.scalar_twin(dev)
    sds = packing.stage_desc(spec, specs_s, False, niters=1)      # (without the fused regulariser too: the scalar gradient is g(h_e) alone)
    sds.lr = 0.0
    gs, _ = run(ps, sds, True, None)
    l = pv.layout
    for slot, n in edge.rows:
        si, pi = divmod(slot, pv.P)
        g_h = torch.cat([packing.person_view(gs[si], l, pi, 'traj_local_heading'), packing.person_view(gs[si], l, pi, 'traj_local_dheading')[1:n]]).numpy()
        out[slot] = (keep['hv_grads'][slot, :n].cpu().numpy(), g_h)
    scalar_entries = torch.cat([torch.cat([packing.person_view(gv[si], l, pi, k).reshape(-1) for k in hv.VEC_KEYS]) for si in range(pv.S) for pi in range(pv.P)])
    return out, {k: pv.t[k].cpu().numpy() for k in OUT}, {k: ps.t[k].cpu().numpy() for k in OUT}, keep['hv_losses'].cpu().numpy(), scalar_entries.numpy(), pv, keep


def check_edges(edge, runner, dev):
    """The checks both runtimes share (tests/test_heading_vec_gpu.py runs them on the device)."""
    grads, out_v, out_s, losses, scalar_entries, pv, keep = _edge_runs(edge, runner, dev)
    assert not np.any(scalar_entries), 'the dead scalar entries have a gradient'
    # same heading angles -> same poses, projections and data terms, to the bit (the regularisers' values sit elsewhere; params hold other things)
    for k in ('orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world'):
        assert np.array_equal(out_v[k], out_s[k]), k
    n_m1 = {0: float(sum(n - 1 for slot, n in edge.rows if slot < pv.P)), 1: float(sum(n - 1 for slot, n in edge.rows if slot >= pv.P))}
    tot, tot_floor = {si: np.zeros(2) for si in n_m1}, {si: np.zeros(2) for si in n_m1}
    for slot, n in edge.rows:
        inp = edge.inputs[slot]
        si = slot // pv.P
        ref = hv.restate(inp['prior_cs'][:n], inp['r'][:n], inp['mask'][:n], grads[slot][1], 2.0, 3.0e3, n_m1[si])
        f32 = hv.restate(inp['prior_cs'][:n], inp['r'][:n], inp['mask'][:n], grads[slot][1], 2.0, 3.0e3, n_m1[si], dtype=torch.float32)
        tot[si] += (ref['reg'], ref['new'])
        tot_floor[si] += (abs(f32['reg'] - ref['reg']), abs(f32['new'] - ref['new']))      # (a scene's value is the sum of its persons')
        # a row's gradient has the size |g_h| / |v| (+ the regularisers'): rows are compared in units of it, the rows whose vector the residual
        # shrinks to 1e-3 (fp32 forms that sum with 1e-4 relative error) apart from the rest
        m = inp['mask'][:n].astype(np.float64).copy()
        m[0] = 1.0
        v = np.linalg.norm(inp['prior_cs'][:n].astype(np.float64) + m[:, None] * inp['r'][:n], axis=-1)
        scale = np.abs(grads[slot][1]) / v + np.abs(ref['g_r']).max(axis=-1) + 1e-30
        shrunk = v < 0.01
        for rows in (shrunk, ~shrunk):
            if rows.any():
                floor = hv.scaled_err(f32['g_r'][rows], ref['g_r'][rows], scale[rows])
                err = hv.scaled_err(grads[slot][0][rows], ref['g_r'][rows], scale[rows])
                print('slot %d %s rows: gradient %.3g of its size, fp32 restatement %.3g' % (slot, 'shrunk' if rows is shrunk else 'other', err, floor))
                assert err <= 16 * floor, (slot, err, floor)
        masked = m == 0.0
        reg_only = hv.restate(inp['prior_cs'][:n], inp['r'][:n], inp['mask'][:n], 0 * grads[slot][1], 2.0, 3.0e3, n_m1[si])['g_r']
        assert np.allclose(grads[slot][0][masked], reg_only[masked], rtol=1e-5, atol=0), 'a masked row has a data gradient'
    for si in tot:
        for k in range(2):
            floor = tot_floor[si][k]      # the fp32 restatement's own error on this value
            print('scene %d %s: value %.9g, off fp64 by %.3g, fp32 restatement by %.3g' % (si, list(packing.HEADING_VEC_TERMS)[k], losses[si, k], abs(losses[si, k] - tot[si][k]), floor))
            assert abs(losses[si, k] - tot[si][k]) <= 16 * floor, (si, k, losses[si, k], tot[si][k], floor)
    # the empty slot's rows and the rows beyond a person's existing ones are never written
    assert not keep['hv_grads'][3].any() and not keep['hv_grads'][1, 1:].any()
    return grads


def test_edges_match_the_restatement(edge, runner):
    check_edges(edge, runner, CPU)


def test_mutations_of_the_restatement_are_visible(edge, runner):
    """Each mutation moves an output (angles, gradient, one of the two values) of every person it touches by at least two of the bounds the
    kernel is held to (16 x the fp32 restatement's error): a kernel with that mistake fails test_edges_match_the_restatement."""
    grads = _edge_runs(edge, runner, CPU)[0]
    touched = {m: 0 for m in hv.MUTATIONS}
    for slot, n in edge.rows:
        inp = edge.inputs[slot]
        args = (inp['prior_cs'][:n], inp['r'][:n], inp['mask'][:n], grads[slot][1], 2.0, 3.0e3, float(max(n - 1, 1)))
        ref, f32 = hv.restate(*args), hv.restate(*args, dtype=torch.float32)
        bound = {k: 16 * max(float(np.abs(np.asarray(f32[k], np.float64) - np.asarray(ref[k])).max()), 1e-30) for k in ref}
        for mut in hv.MUTATIONS:
            if n == 1 and mut not in ('mask_on_row0', 'swap_gxy', 'normalised', 'reg_row0'):
                continue      # (a single row has no mask and no regularised row)
            got = hv.restate(*args, mutation=mut)
            moved = max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k])).max()) / bound[k] for k in ref)
            assert moved >= 2.0, (slot, mut, moved)
            touched[mut] += 1
    assert all(touched.values()), touched


def test_nan_in_the_scalar_entries_changes_nothing(edge, runner):
    run, _ = runner
    heading = dict(terms={'local_traj_dheading_reg_new': dict(weight=3.0e3, monitor_only=False)})
    outs = []
    for poison in (False, True):
        pv, specs = edge.vec(CPU)
        if poison:
            for si in range(pv.S):
                for pi in range(pv.P):
                    for k in hv.VEC_KEYS:
                        packing.person_view(pv.t['params'][si], pv.layout, pi, k)[...] = float('nan')
        sd = packing.stage_desc(packing.split_heading_vec(edge.spec)[0], specs, False, niters=3)
        g, keep = run(pv, sd, True, heading)
        keep_entries = torch.ones_like(pv.t['params'], dtype=torch.bool)
        for si in range(pv.S):
            for pi in range(pv.P):
                for k in hv.VEC_KEYS:
                    packing.person_view(keep_entries[si], pv.layout, pi, k)[...] = False
        outs.append([pv.t['params'][keep_entries].numpy(), g.numpy(), pv.t['heading_vec'].numpy(), keep['hv_grads'].numpy(), keep['hv_losses'].numpy()] +
                    [pv.t[k].numpy() for k in OUT[1:]])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_flag_off_is_the_extension_without_the_fields(edge, runner):
    """Scalar headings: an extension whose heading fields are all zero computes the bits of the plain wide stage."""
    run, _ = runner
    outs = []
    for world in (None, {}):
        ps, specs = edge.scalar_twin(CPU)
        g, _ = run(ps, packing.stage_desc(edge.spec, specs, False, niters=3), True, None, world)
        outs.append([g.numpy()] + [ps.t[k].numpy() for k in OUT])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_refusals_of_the_launcher(edge):
    fn = hv.hostsim_fn()
    pv, specs = edge.vec(CPU)
    sb = pv.struct()
    spec = packing.split_heading_vec(edge.spec)[0]
    ext, keep = packing.world_ext(None, pv, niters=1, heading={})
    sd = packing.stage_desc(spec, dict(specs, absolute_heading=True), False, niters=1)
    assert fn(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ext), None) == -2
    sd = packing.stage_desc(edge.spec, specs, False, niters=1)      # (the fused regulariser still listed)
    assert (sd.loss_mask >> packing.LOSS_IDS['local_traj_dheading_reg_new']) & 1
    assert fn(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ext), None) == -2
    ext.heading_vec_workspace = None
    assert fn(ctypes.byref(sb), ctypes.byref(packing.stage_desc(spec, specs, False, niters=1)), ctypes.byref(ext), None) == -1


# ---- packing, outputs, refusals of the host ---------------------------------------------------------------------------------------------------------
SPEC = {'opt_variables': ['cam', 'local_heading', 'local_dheading'], 'opt_niters': 4, 'opt_lr': 0.1,
        'loss_cfg': {'kp_2d': {'weight': 1.0}, 'local_traj_dheading_reg': {'weight': 2.0, 'monitor_only': True}, 'cam_up_reg': {'weight': 2.0},
                     'local_traj_dheading_reg_new': {'weight': 3.0e3}}}


def test_split_heading_vec():
    rest, heading = packing.split_heading_vec(SPEC)
    assert list(rest['loss_cfg']) == ['kp_2d', 'cam_up_reg'] and rest['opt_variables'] == SPEC['opt_variables'] and len(SPEC['loss_cfg']) == 4
    assert heading == dict(loss_order=['kp_2d', 'local_traj_dheading_reg', 'cam_up_reg', 'local_traj_dheading_reg_new'],
                           terms={'local_traj_dheading_reg': dict(weight=2.0, monitor_only=True), 'local_traj_dheading_reg_new': dict(weight=3.0e3, monitor_only=False)})
    assert packing.has_heading_vec({'s': rest}) and not packing.has_heading_vec({'s': SPEC})
    assert packing.split_off_kernel({'s': rest})[2] == {}      # (local_traj_dheading_reg no longer goes to the auxiliary kernel)
    sd = packing.stage_desc(rest, {'heading_type': 'vec'})
    assert not (sd.loss_mask >> packing.LOSS_IDS['local_traj_dheading_reg_new']) & 1
    assert packing.is_heading_vec({'heading_type': 'vec'}) and not packing.is_heading_vec({})
    with pytest.raises(NotImplementedError, match='heading_type'):
        packing.is_heading_vec({'heading_type': 'quat'})


def test_world_ext_carries_the_heading_fields():
    packed = packing.PackedScenes.empty(2, 3, 7, CPU)
    ex, keep = packing.world_ext(None, packed)
    assert ex.heading_vec is None and ex.hv_loss_mask == 0 and 'hv_ws' not in keep and 'heading_vec' not in packed.t      # as before
    with pytest.raises(ValueError, match='heading_type'):
        packing.world_ext(None, packed, heading={})
    packed.heading_vec = True
    ex, keep = packing.world_ext(None, packed, niters=4, want_grads=True, want_hist=True, heading=packing.split_heading_vec(SPEC)[1])
    assert packed.t['heading_vec'].shape == (6, 7, 2) and not packed.t['heading_vec'].any() and ex.heading_vec == packed.t['heading_vec'].data_ptr()
    assert (ex.hv_loss_mask, ex.hv_monitor_mask) == (3, 1) and ex.hv_loss_weight[0] == 2.0 and ex.hv_loss_weight[1] == 3.0e3
    assert keep['hv_ws'].shape == (6, 7, packing.HEADING_VEC_WS_FLOATS) and keep['hv_grads'].shape == (6, 7, 2) and keep['hv_loss_history'].shape == (2, 4, 2)
    assert (ex.var_mask, ex.flags, ex.loss_mask) == (0, 0, 0) and packed.t['world_res'].shape == (6, 7, 8)
    assert _lib.lib().glamr_grecon_heading_vec_workspace_bytes(2, 3, 7) == 2 * 3 * 7 * packing.HEADING_VEC_WS_FLOATS * 4


def test_struct_matches_the_header():
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "glamr_hip.h"\nint main(){printf("%zu %zu %zu %d %d\\n", sizeof(glamr_stage_ext), '
            'offsetof(glamr_stage_ext, heading_vec), offsetof(glamr_stage_ext, hv_losses), GLAMR_EXT_HV_NUM_LOSSES, GLAMR_EXT_HV_WS);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'p.c'), 'w') as f:
            f.write(code)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 'p')]).split()]
    assert out == [ctypes.sizeof(_lib.StageExt), _lib.StageExt.heading_vec.offset, _lib.StageExt.hv_losses.offset, len(packing.HEADING_VEC_TERMS),
                   packing.HEADING_VEC_WS_FLOATS]


def test_outputs_shapes_and_round_trip(asset_root):
    """unpack_into gives traj_local_heading (2,) and traj_local_dheading (len - 1, 2); packing that result again restores the array; a result
    of one heading_type under the other raises ValueError."""
    cfg, specs, data, jl = hv.prepared(asset_root, 'c')
    packed = hv.pack(data, jl, specs, CPU)
    rng = np.random.RandomState(0)
    n_of = (packed.t['fr_end'] - packed.t['fr_start']).tolist()
    for slot, n in enumerate(n_of):
        packed.t['heading_vec'][slot, :n] = torch.from_numpy(rng.randn(n, 2).astype(np.float32))
    want = packed.t['heading_vec'].clone()
    packed.unpack_into([data], None, specs)
    for pi, pd in data['person_data'].items():
        assert tuple(pd['traj_local_heading'].shape) == (2,) and tuple(pd['traj_local_dheading'].shape) == (n_of[pi] - 1, 2)
        assert torch.equal(pd['traj_local_dheading'], want[pi, 1:n_of[pi]])
    again = hv.pack(data, jl, specs, CPU)
    assert torch.equal(again.t['heading_vec'], want) and again.heading_vec
    with pytest.raises(ValueError, match='heading_type'):
        hv.pack(data, jl, dict(specs, heading_type='scalar'), CPU)
    scalar = hv.prepared(asset_root, 'c', twin=True)
    with pytest.raises(ValueError, match='heading_type'):
        hv.pack(scalar[2], scalar[3], specs, CPU)


def _optimizer(specs_update=None, stage_update=None):
    """GlobalReconOptimizer.__init__ up to its refusals, without a device: the body model and the priors are stand-ins."""
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    cfg = hv.config_of('b')
    cfg['grecon_model_specs'].update(specs_update or {})
    for s in cfg['opt_stage_specs'].values():
        s['loss_cfg'].update((stage_update or {}).get('loss_cfg', {}))
        s['opt_variables'] += (stage_update or {}).get('opt_variables', [])
    return GlobalReconOptimizer(cfg, torch.device('cuda'), None, smpl=object(), mt_model=object())      # (the device is only named here)


def test_the_optimiser_accepts_vec_and_refuses_what_it_cannot_run():
    opt = _optimizer()
    assert opt.heading_vec and list(opt._heading_cfg) == ['init_opt']
    assert set(opt._heading_cfg['init_opt']['terms']) == {'local_traj_dheading_reg', 'local_traj_dheading_reg_new'}
    assert not any(n in opt.opt_stage_specs['init_opt']['loss_cfg'] for n in packing.HEADING_VEC_TERMS) and not opt._aux_cfg
    for update, what in ((dict(flag_opt_motion_latent=True), 'latent-optimisation mode'), (dict(flag_opt_traj_latent=True, flag_attach_traj_pred=True), 'flag_attach_traj_pred'),
                         (dict(flag_aux_on_device=True), 'flag_aux_on_device'), (dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'),
                         (dict(absolute_heading=True), 'absolute_heading')):
        with pytest.raises(NotImplementedError, match="heading_type = 'vec' together with .*%s" % what):
            _optimizer(update)
    with pytest.raises(NotImplementedError, match="heading_type = 'vec' together with .*penetration"):
        _optimizer(dict(flag_use_pen_loss=True), dict(loss_cfg={'penetration': {'weight': 1.0}}))
    for name in ('cam_depth_smoothness', 'traj_trans_smoothness', 'cam_traj_trans', 'cam_rot_smoothness', 'cam_trans_smoothness'):
        with pytest.raises(NotImplementedError, match="heading_type = 'vec' together with .*%s" % name):
            _optimizer(None, dict(loss_cfg={name: {'weight': 1.0}}))
    with pytest.raises(NotImplementedError, match="extra_loss together with heading_type = 'vec'"):
        opt.extra_loss = lambda ctx: None
    # the other two conditions of the old catch-all keep raising, each under its own name
    with pytest.raises(NotImplementedError, match='flag_cam_inv_trans_res_all'):
        _optimizer(dict(heading_type='scalar', flag_cam_inv_trans_res_all=False))
    with pytest.raises(NotImplementedError, match='flag_opt_cam'):
        _optimizer(dict(heading_type='scalar', flag_opt_cam=False))
    with pytest.raises(NotImplementedError, match='heading_type'):
        _optimizer(dict(heading_type='quat'))


def test_sharded_schedule_refuses_vec():
    from glamr_amd import parallel
    packed = packing.PackedScenes.empty(1, 2, 6, CPU)
    sched = parallel.PersonShardedSchedule(rank=0, world=1, use_dist=False)
    plain = {'s0': {'opt_variables': ['local_xy'], 'opt_niters': 1, 'opt_lr': 0.1, 'loss_cfg': {'kp_2d': {'weight': 1.0}}}}
    with pytest.raises(NotImplementedError, match="heading_type = 'vec'.*person-sharded"):
        sched.run(packed, plain, {'heading_type': 'vec'})
    with pytest.raises(NotImplementedError, match="heading_type = 'vec'.*person-sharded"):
        sched.run(packed, packing.split_heading_vec_specs(plain)[0], {})
