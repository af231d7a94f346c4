"""CPU checks of glamr_grecon_aux_step: csrc/grecon_aux_step.hpp on the host runtime against the composition it replaces -- the
host builds of glamr_grecon_aux_terms, glamr_grecon_cam_backward and glamr_grecon_pose_backward in add mode on zeroed scratch, then
torch.optim.Adam on the CPU -- bit for bit over three consecutive steps (tests/aux_step_common.py), the entry point's argument checks, the
two mutations that show the cases tell the composition's parts apart, and the optimiser's flag."""
import ctypes

import numpy as np
import pytest

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import aux_step_common as A
from tests import aux_terms_common as C

_RUNS = {}


def _entries():
    if 'e' not in _RUNS:
        _RUNS['e'] = A.host_entries()
    return _RUNS['e']


def _run(name, fused, **kw):
    """A run's record, computed once per (case, side, mutation) and left unchanged."""
    key = (name, fused, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = A.Run(name, _entries(), fused, **kw).record
    return _RUNS[key]


@pytest.mark.parametrize('name', A.CASE_NAMES)
def test_fused_host_step_equals_the_composition_bit_for_bit(name):
    fused, comp = _run(name, True), _run(name, False)
    for k in range(A.N_STEPS):
        for g in A.GROUPS:
            assert np.isfinite(fused[k][g]).all(), (name, k, g)      # (a NaN read anywhere)
            assert A.bit_equal(fused[k][g], comp[k][g]), (name, k, g, int((fused[k][g] != comp[k][g]).sum()), float(np.abs(fused[k][g] - comp[k][g]).max()))
    run_cam, derived, run_pose = A.liveness(C.cases()[name])
    print('%s: cam VJP %s, pose VJP %s, %d steps bit-equal' % (name, 'derived' if derived else run_cam, run_pose, A.N_STEPS))


@pytest.mark.parametrize('name', A.CASE_NAMES)
def test_params_follow_torch_adam_fed_the_outgoing_gradient(name):
    _, st = A.arrays(name)
    adam = A.TorchAdam(st['params'], st['exp_avg'], st['exp_avg_sq'])
    for k, rec in enumerate(_run(name, True)):
        p, m, v = adam.step(rec['grads'])
        assert A.bit_equal(rec['params'], p) and A.bit_equal(rec['exp_avg'], m) and A.bit_equal(rec['exp_avg_sq'], v), (name, k)


@pytest.mark.parametrize('name', A.CASE_NAMES)
def test_structural_zeros(name):
    """Entries no phase may write keep the incoming gradient's bits; all terms monitor-only: the whole array does, the values are still written."""
    case, (_, st) = C.cases()[name], A.arrays(name)
    keep = A.untouched(case)
    assert keep.any()
    for k, rec in enumerate(_run(name, True)):
        assert A.bit_equal(rec['grads'][keep], st['grads_in'][k][keep]), (name, k)
        if name == 'monitor_all':
            assert A.bit_equal(rec['grads'], st['grads_in'][k])
            assert np.isfinite(rec['values']).all() and (rec['values'][:, [C.ROT, C.TRANS, C.DEPTH, C.TRAJ, C.CAMTRAJ]] > 0).all()
        else:
            assert not A.bit_equal(rec['grads'][~keep], st['grads_in'][k][~keep])
    # the values are those of the stand-alone call at the same parameters (step 0: the inputs as they are)
    a, _ = A.arrays(name)
    rc, alone = C.run(case, _entries().aux, lambda x: np.ascontiguousarray(x).copy(), lambda x: x, arrays={k: a[k] for k in C.host_arrays(case)})
    assert rc == 0 and A.bit_equal(alone['values'], _run(name, True)[0]['values'])


@pytest.mark.parametrize('mut', ['skip_cam', 'step_shift'])
def test_mutations_of_the_composition_are_caught_on_every_case_they_touch(mut):
    touched = 0
    for name in A.CASE_NAMES:
        run_cam = A.liveness(C.cases()[name])[0]
        if mut == 'skip_cam' and not run_cam:
            continue
        touched += 1
        fused, bad = _run(name, True), _run(name, False, **({'skip_cam': True} if mut == 'skip_cam' else {'step_shift': 1}))
        group = 'grads' if mut == 'skip_cam' else 'params'
        assert not A.bit_equal(fused[0][group], bad[0][group]), (mut, name)
        assert not A.bit_equal(fused[-1]['params'], bad[-1]['params']), (mut, name)
    assert touched >= (3 if mut == 'skip_cam' else len(A.CASE_NAMES))


def test_cases_cover_the_paths():
    live = {n: A.liveness(C.cases()[n]) for n in A.CASE_NAMES}
    assert {C.cases()[n]['mode'] for n in A.CASE_NAMES if live[n][0]} == {'frame', 'fixed', 'derived'}      # the camera VJP in its three modes
    assert any(C.cases()[n]['mode'] == 'constant' and live[n][2] for n in A.CASE_NAMES)
    assert any(live[n][1] for n in A.CASE_NAMES) and not any(live['monitor_all'])
    assert A.REFUSED_CASE not in A.CASE_NAMES and C.cases()[A.REFUSED_CASE]['T'] == 1
    assert any(min(C.cases()[n]['seq_len']) == 2 and C.cases()[n]['T'] > 256 for n in A.CASE_NAMES)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------
def _call(entry, name, edit=None, null=(), aux_edit=None, stage_edit=None, **over):
    case = C.cases()[name]
    a, st = A.arrays(name if name in A.CASE_NAMES else 'monitor')
    if name not in A.CASE_NAMES:      # (the refused geometry: nothing is dereferenced before the refusal)
        a = {k: np.zeros(4, np.float32) for k in a}
    a = {k: np.ascontiguousarray(v).copy() for k, v in a.items()}
    sb, sd, ad = C.scene_batch(case, {k: _lib.ptr(v).value for k, v in a.items()}), A.stage_desc(case), C.aux_desc(case)
    for fn, obj in ((edit, sb), (aux_edit, ad), (stage_edit, sd)):
        if fn:
            fn(obj)
    o = dict(values=np.zeros((case['S'], 6), np.float32), grads=st['grads_in'][0].copy(), exp_avg=st['exp_avg'].copy(), exp_avg_sq=st['exp_avg_sq'].copy(),
             root_trans_cam=a['root_trans_cam'], ws=np.zeros(1 << 18, np.float32))
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in o.items()}
    kw = dict(values_stride=6, iteration=0, lr=A.LR, step=1)
    kw.update(over)
    return entry(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), p['root_trans_cam'], p['values'], kw['values_stride'], kw['iteration'], p['grads'], p['exp_avg'],
                 p['exp_avg_sq'], kw['lr'], kw['step'], p['ws'])


def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """The host build and the library's own entry point (its checks run before any HIP call) share aux_step_check."""
    from glamr_amd import build
    build.build_library()
    L = _lib.lib()
    host, dev = _entries().fused, (lambda *a: L.glamr_grecon_aux_step(*a, None))
    E_INVALID, E_UNSUPPORTED = -1, -4
    for entry in (host, dev):
        msg = (lambda: L.glamr_last_error()) if entry is dev else (lambda: None)
        sd, ad = A.stage_desc(C.cases()['monitor']), C.aux_desc(C.cases()['monitor'])
        assert entry(None, ctypes.byref(sd), ctypes.byref(ad), None, None, 6, 0, None, None, None, A.LR, 1, None) == E_INVALID
        for arg in ('values', 'grads', 'exp_avg', 'exp_avg_sq', 'ws'):
            assert _call(entry, 'monitor', null=(arg,)) == E_INVALID, arg
            assert msg() is None or b'NULL argument' in msg()
        assert _call(entry, A.REFUSED_CASE) == E_INVALID                      # max_len 1: the pose VJP's limit
        assert msg() is None or b'max_len >= 2' in msg()
        assert _call(entry, 'monitor', edit=lambda sb: setattr(sb, 'max_persons', 33)) == E_INVALID
        assert msg() is None or b'bad batch geometry' in msg()
        assert _call(entry, 'monitor', step=0) == E_INVALID and _call(entry, 'monitor', lr=0.0) == E_INVALID
        assert msg() is None or b'1-based' in msg()
        assert _call(entry, 'monitor', iteration=1) == E_INVALID and _call(entry, 'monitor', iteration=-1) == E_INVALID
        assert msg() is None or b'values_stride' in msg()
        assert _call(entry, 'monitor', aux_edit=lambda ad: setattr(ad, 'loss_mask', 1 << 6)) == E_INVALID
        assert msg() is None or b'loss_mask' in msg()
        assert _call(entry, 'monitor', edit=lambda sb: setattr(sb, 'frozen', 16)) == E_UNSUPPORTED
        assert msg() is None or b'person-sharded' in msg()
        assert _call(entry, 'monitor', stage_edit=lambda sd: setattr(sd, 'flags', sd.flags | packing.FLAG_ABSOLUTE_HEADING)) == E_UNSUPPORTED
        assert msg() is None or b'ABSOLUTE_HEADING' in msg()
        # the camera-variable terms in a stage that does not optimise the camera
        assert _call(entry, 'monitor', stage_edit=lambda sd: setattr(sd, 'var_mask', sd.var_mask & ~C.VB['cam'])) == E_UNSUPPORTED
        assert msg() is None or b'does not optimise the camera' in msg()
        for arr in ('seq_len', 'params', 'trans_world', 'cam_pose', 'vis', 'fr_end', 'traj_local_pred'):
            assert _call(entry, 'monitor', edit=lambda sb, arr=arr: setattr(sb, arr, None)) == E_INVALID, arr
            assert msg() is None or b'NULL batch array' in msg() or b'cam_traj_trans needs' in msg()
        for arr in ('person2cam', 'orient_world', 'base_orient'):              # read when the camera is derived from the persons
            assert _call(entry, 'slots3', edit=lambda sb, arr=arr: setattr(sb, arr, None)) == E_INVALID, arr
        assert _call(entry, 'monitor', null=('root_trans_cam',)) == E_INVALID
        assert _call(entry, 'monitor', edit=lambda sb: setattr(sb, 'n_scenes', 0)) == 0      # an empty batch is a no-op whatever the arrays
    assert L.glamr_grecon_aux_step_workspace_bytes(0, 4, 100) == 0
    S, P, T = 3, 4, 100
    parts = 2 * S * P * T * 3 + S * T * 12 + S * 6 + 2 + S * P + S * T * 13 + S * P * T * 27
    assert L.glamr_grecon_aux_step_workspace_bytes(S, P, T) == 4 * parts == _entries().ws['fused'](S, P, T)


# ---- the optimiser's flag --------------------------------------------------------------------------------------------------------------------
def test_flag_routes_aux_only_schedules_and_nothing_else():
    from glamr_amd.global_recon import extra_loss_schedule as xs
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    aux = {'main_opt': {'cam_depth_smoothness': {'weight': 1.0, 'monitor_only': False}, 'cam_traj_trans': {'weight': 2.0, 'monitor_only': False}}}
    pen = {'main_opt': {'weight': 1.0, 'monitor_only': False}}
    what = xs.aux_what(['cam_depth_smoothness', 'cam_traj_trans'])
    opt = GlobalReconOptimizer.__new__(GlobalReconOptimizer)       # host logic only: no device, no library
    opt._extra_loss, opt._pen_cfg, opt._aux_cfg = None, {}, aux
    assert opt.flag_aux_on_device is False and not opt._aux_on_device() and opt._off_kernel_term() == what      # flag off: as today
    for call in ('optimize_resident', 'capture_resident', 'optimize_stream'):
        with pytest.raises(NotImplementedError, match=call + '.*cam_depth_smoothness'):
            opt._refuse_extra_loss(call)
    opt.flag_aux_on_device = True
    assert opt._aux_on_device() and opt._off_kernel_term() is None
    opt._refuse_extra_loss('optimize_resident')                                                                 # nothing to refuse
    opt._extra_loss = lambda ctx: None                                                                          # a caller's term: the flag is ignored
    assert not opt._aux_on_device() and opt._off_kernel_term() == 'extra_loss'
    with pytest.raises(NotImplementedError, match='optimize_stream while extra_loss is set'):
        opt._refuse_extra_loss('optimize_stream')
    opt._extra_loss, opt._pen_cfg = None, pen
    assert not opt._aux_on_device() and opt._off_kernel_term() == 'the penetration term (loss_cfg)'
    with pytest.raises(NotImplementedError, match='capture_resident with the penetration term'):
        opt._refuse_extra_loss('capture_resident')
    opt._pen_cfg, opt._aux_cfg = {}, {}
    assert not opt._aux_on_device() and opt._off_kernel_term() is None                                          # no names: run_schedule, flag or not


def test_publish_cuts_the_history_by_name():
    import torch
    from glamr_amd.global_recon import aux_step_schedule
    cfg = {'s0': {'cam_traj_trans': {}, 'cam_rot_smoothness': {}}}
    h = torch.arange(2 * 3 * 6, dtype=torch.float32).view(2, 3, 6)
    out = aux_step_schedule.publish(cfg, {'s0': h})
    assert sorted(out['s0']) == ['cam_rot_smoothness', 'cam_traj_trans'] and out['s0']['cam_traj_trans'].shape == (2, 3)
    assert np.array_equal(out['s0']['cam_traj_trans'], h.numpy()[:, :, 4]) and np.array_equal(out['s0']['cam_rot_smoothness'], h.numpy()[:, :, 0])
