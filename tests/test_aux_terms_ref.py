"""CPU checks of the six loss_cfg terms of glamr_grecon_aux_terms: csrc/grecon_aux.hpp on the host runtime against the fp64
restatement of tests/aux_terms_common.py, the entry point's argument checks, packing.split_aux / check_aux and every refusal, and the
mutations that show the restatement's cases tell the definitions apart."""
import ctypes
import os

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import aux_terms_common as C
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host():
    lib = hostsim.build('grecon_aux_host')
    lib.hostsim_grecon_aux_terms.restype = ctypes.c_int
    lib.hostsim_grecon_aux_terms.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_void_p]
    return lib.hostsim_grecon_aux_terms


def _run(case, **kw):
    return C.run(case, _host(), lambda a: np.ascontiguousarray(a), lambda a: a, **kw)


def _assert_within(case, got, ref, what):
    err, tol = C.errors(case, got, ref), C.tol(case['name'])
    print('%s %s: %s' % (case['name'], what, ', '.join('%s %.2e (bound %.2e)' % (k, err[k], tol[k]) for k in C.GROUPS)))
    for k in C.GROUPS:
        assert err[k] <= tol[k], (case['name'], what, k, err[k], tol[k])


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_floor_constants_are_what_fp32_autograd_gives(name):
    got = C.measure_floor(name)
    for k in C.GROUPS:
        f = C.FLOOR[name][k]
        assert (got[k] == 0.0) if f == 0.0 else (0.5 * f <= got[k] <= 2.0 * f), (name, k, got[k], f)


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_host_runtime_matches_fp64(name):
    """Store mode on NaN-filled outputs, unread inputs NaN: values and every adjoint within 16 x the fp32 floor, zero everywhere else."""
    case = C.cases()[name]
    rc, got = _run(case)
    assert rc == 0
    for k, v in got.items():
        assert np.isfinite(v).all(), (name, k)
    _assert_within(case, got, C.ref64(name), 'host')
    assert C.outside_groups_zero(case, got)


@pytest.mark.parametrize('name', ['frame257', 'slots3', 'monitor', 'monitor_all'])
def test_host_runtime_add_mode(name):
    """accumulate != 0 adds exactly what store mode stores (one addition per entry) and touches nothing else."""
    case = C.cases()[name]
    pre = C.prefill(case)
    _, store = _run(case)
    rc, add = _run(case, accumulate=1, prefill=pre)
    assert rc == 0
    for k in ('g_trans_world', 'g_cam_pose', 'grads'):
        assert np.array_equal(add[k], pre[k] + store[k]), (name, k)
    assert np.array_equal(add['values'], store['values'])


def test_zero_denominators_give_zero_not_nan():
    one = _run(C.cases()['seq1'])[1]
    assert np.array_equal(one['values'][0, [C.ROT, C.TRANS, C.DEPTH, C.TRAJ, C.DH]], np.zeros(5, np.float32)) and one['values'][0, C.CAMTRAJ] > 0
    assert not one['grads'].any()
    nv = _run(C.cases()['never_visible'])[1]
    assert nv['values'][1, C.CAMTRAJ] == 0 and nv['values'][1, C.DH] == 0 and not nv['g_cam_pose'].any()
    fixed = _run(C.cases()['fixed'])[1]
    assert np.array_equal(fixed['values'][:, :2], np.zeros((1, 2), np.float32))


@pytest.mark.parametrize('mut', list(C.MUTATIONS))
def test_mutations_move_an_output_of_every_case_they_touch(mut):
    touched = 0
    for name, case in C.cases().items():
        if not any(C.touches(mut, case, si) for si in range(case['S'])):
            continue
        touched += 1
        err, tol = C.errors(case, C.reference(case, mut=mut), C.ref64(name)), C.tol(name)
        moved = {k: err[k] / tol[k] for k in C.GROUPS if tol[k] > 0 and err[k] > 0}
        print('%s on %s: %s' % (mut, name, ', '.join('%s %.1f tol' % kv for kv in moved.items())))
        assert max(moved.values(), default=0.0) >= 2.0, (mut, name, err)
    assert touched >= 1, mut


def test_mutation_free_restatement_is_its_own_reference():
    case = C.cases()['slots3']
    err = C.errors(case, C.reference(case, mut=''), C.ref64('slots3'))
    assert max(err.values()) == 0.0


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------
def _call(entry, case, edit=None, null=(), aux_edit=None, mode=None):
    a = {k: np.ascontiguousarray(v) for k, v in C.host_arrays(case).items()}
    o = {k: np.zeros(s, np.float32) for k, s in C.output_shapes(case).items()}
    ws = np.zeros(case['S'] * case['P'], np.int32)
    sb, sd, ad = C.scene_batch(case, {k: _lib.ptr(v).value for k, v in a.items()}), C.stage_desc(case, mode), C.aux_desc(case)
    if edit:
        edit(sb)
    if aux_edit:
        aux_edit(ad)
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in dict(o, root_trans_cam=a['root_trans_cam'], ws=ws).items()}
    args = [ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ad), p['root_trans_cam'], p['values'], p['g_trans_world'], p['g_cam_pose'], p['grads'], 0, p['ws']]
    return entry(*args), (a, o)


@pytest.fixture(scope='module')
def entries():
    """[(entry point, takes a stream)]: the host build, and the library's own (its checks run before any HIP call)."""
    from glamr_amd import build
    build.build_library()
    L = _lib.lib()
    return [_host(), lambda *a: L.glamr_grecon_aux_terms(*a, None)], L


def test_argument_checks(entries):
    (host, dev), L = entries
    case, E_INVALID, E_UNSUPPORTED = C.cases()['monitor'], -1, -4
    for entry in (host, dev):
        msg = (lambda: L.glamr_last_error()) if entry is dev else (lambda: None)
        sd, ad = C.stage_desc(case), C.aux_desc(case)
        assert entry(None, ctypes.byref(sd), ctypes.byref(ad), None, None, None, None, None, 0, None) == E_INVALID
        assert _call(entry, case, null=('values',))[0] == E_INVALID
        assert _call(entry, case, null=('ws',))[0] == E_INVALID
        assert _call(entry, case, edit=lambda sb: setattr(sb, 'max_persons', 33))[0] == E_INVALID
        assert msg() is None or b'bad batch geometry' in msg()
        assert _call(entry, case, edit=lambda sb: setattr(sb, 'max_len', 0))[0] == E_INVALID
        assert _call(entry, case, aux_edit=lambda ad: setattr(ad, 'loss_mask', 1 << 6))[0] == E_INVALID
        assert msg() is None or b'loss_mask' in msg()
        assert _call(entry, case, edit=lambda sb: setattr(sb, 'frozen', 16))[0] == E_UNSUPPORTED
        assert msg() is None or b'person-sharded' in msg()
        # the camera-variable terms in a stage that does not optimise the camera: derived and constant
        for mode in ('derived', 'constant'):
            assert _call(entry, case, mode=mode)[0] == E_UNSUPPORTED
            assert msg() is None or b'does not optimise the camera' in msg()
        for arr in ('seq_len', 'params', 'trans_world', 'cam_pose', 'vis', 'fr_end'):
            assert _call(entry, case, edit=lambda sb, arr=arr: setattr(sb, arr, None))[0] == E_INVALID, arr
            assert msg() is None or b'NULL batch array' in msg() or b'cam_traj_trans needs' in msg()
        assert _call(entry, case, null=('root_trans_cam',))[0] == E_INVALID
        assert _call(entry, case, null=('grads',))[0] == E_INVALID
        assert _call(entry, case, null=('g_trans_world',))[0] == E_INVALID
        assert _call(entry, case, null=('g_cam_pose',))[0] == E_INVALID
        assert msg() is None or b'g_cam_pose is required' in msg()
        # an empty batch is a no-op whatever the arrays
        assert _call(entry, case, edit=lambda sb: setattr(sb, 'n_scenes', 0))[0] == 0
    # outputs nobody writes to may be NULL: all terms monitor-only, and a constant camera's g_cam_pose
    assert _call(host, C.cases()['monitor_all'], null=('grads', 'g_trans_world', 'g_cam_pose'))[0] == 0
    assert _call(host, C.cases()['never_visible'], null=('g_cam_pose',))[0] == 0
    assert L.glamr_grecon_aux_terms_workspace_bytes(3, 4, 100) == 3 * 4 * 4 and L.glamr_grecon_aux_terms_workspace_bytes(0, 4, 100) == 0


def test_descriptor_matches_the_header():
    """ctypes mirror of glamr_aux_desc against a gcc-compiled probe; the ids of packing.AUX_LOSS_IDS against the header's enum."""
    import subprocess
    import tempfile
    names = ', '.join('GLAMR_AUX_%s' % n.upper() for n in C.NAMES)
    code = '#include <stdio.h>\n#include "glamr_hip.h"\nint main(){printf("%%zu %%d", sizeof(glamr_aux_desc), GLAMR_AUX_NUM_TERMS);int ids[]={%s};' \
           'for(int i=0;i<6;++i)printf(" %%d",ids[i]);return 0;}\n' % names
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(code)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 'p')]).split()]
    assert out[0] == ctypes.sizeof(_lib.AuxDesc) and out[1] == _lib.AUX_NUM_TERMS == len(packing.AUX_LOSS_IDS)
    assert out[2:] == [packing.AUX_LOSS_IDS[n] for n in C.NAMES] == list(range(6))


# ---- packing ---------------------------------------------------------------------------------------------------------------------------------
def test_split_aux():
    cfg = {'kp_2d': {'weight': 1.0}, 'cam_traj_trans': {'weight': 3.0, 'first_frame_weight': 10.0}, 'traj_trans_smoothness': {'weight': 0.5, 'monitor_only': True},
           'penetration': {'weight': 2.0}}
    rest, aux = packing.split_aux(cfg)
    assert list(rest) == ['kp_2d', 'penetration'] and rest['kp_2d'] is cfg['kp_2d']
    assert aux == {'cam_traj_trans': dict(weight=3.0, monitor_only=False, first_frame_weight=10.0), 'traj_trans_smoothness': dict(weight=0.5, monitor_only=True)}
    rest, aux = packing.split_aux({'kp_2d': {'weight': 1.0}})
    assert aux is None and list(rest) == ['kp_2d']
    ad = packing.aux_desc(packing.split_aux(cfg)[1])
    assert ad.loss_mask == (1 << 3) | (1 << 4) and ad.monitor_mask == 1 << 3 and ad.first_frame_weight == 10.0
    assert ad.weight[4] == 3.0 and ad.weight[3] == 0.5 and ad.weight[0] == 0.0
    # the fused optimiser still refuses what nobody holds, and no longer refuses the six
    sd = packing.stage_desc({'opt_variables': ['cam'], 'opt_niters': 1, 'opt_lr': 0.1, 'loss_cfg': packing.split_penetration(rest)[0]}, {})
    assert sd.loss_mask == 1
    for name in ('traj_rot_res', 'traj_trans_res', 'person2cam_res_trans_reg'):
        with pytest.raises(NotImplementedError, match='not supported by the fused optimiser'):
            packing.stage_desc({'opt_variables': ['cam'], 'opt_niters': 1, 'opt_lr': 0.1, 'loss_cfg': packing.split_aux({name: {'weight': 1.0}})[0]}, {})
    for opt in ({'rot_type': 'quat'}, {'first_frame_trans_only': True}):
        with pytest.raises(NotImplementedError, match='loss option not supported'):
            packing.split_aux({'cam_traj_trans': dict(weight=1.0, **opt)})


def test_check_aux():
    stages = lambda name, var: {'s0': {'opt_variables': var, 'loss_cfg': {'kp_2d': {'weight': 1.0}, name: {'weight': 1.0}}}}
    for name in ('cam_rot_smoothness', 'cam_trans_smoothness'):
        packing.check_aux(stages(name, ['cam', 'local_xy']), {})
        with pytest.raises(ValueError, match="needs 'cam' in the stage's opt_variables.*KeyError in the reference.*stale"):
            packing.check_aux(stages(name, ['local_xy']), {})
    for name in ('cam_depth_smoothness', 'traj_trans_smoothness', 'cam_traj_trans', 'local_traj_dheading_reg'):
        packing.check_aux(stages(name, ['local_xy']), {})


def test_schedule_refusals():
    """The combinations the launch-by-launch schedule refuses, named (extra_loss_schedule.check_supported)."""
    from glamr_amd.global_recon import extra_loss_schedule as els
    what = els.aux_what(['cam_traj_trans', 'traj_trans_smoothness'])
    assert 'cam_traj_trans' in what and 'loss_cfg' in what
    for flag, word in (('flag_opt_motion_latent', 'latent-optimisation'), ('flag_opt_traj_latent', 'latent-optimisation'), ('flag_opt_vis_local_rot', 'flag_opt_vis_local_rot'),
                       ('absolute_heading', 'absolute_heading')):
        with pytest.raises(ValueError, match='cam_traj_trans.*%s' % word):
            els.check_supported({flag: True}, what)


@pytest.mark.reference
@pytest.mark.skipif(not __import__('oracle.ref_harness', fromlist=['x']).available(), reason='/root/reference is not present')
def test_smallest_fixture_is_what_the_unmodified_reference_gives(golden):
    """Container only: tools/aux_terms_golden.py run again on the smallest case reproduces the committed file (same machine class: to 1e-5 of an
    array's largest entry, index arrays exactly) and its assertions on the terms' shares hold."""
    import importlib.util
    import sys
    from tests import aux_terms_e2e as ae
    spec = importlib.util.spec_from_file_location('aux_terms_golden', os.path.join(ROOT, 'tools', 'aux_terms_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    cwd, path = os.getcwd(), list(sys.path)
    try:
        spec.loader.exec_module(gen)
        case = 'glamr_dynamic'
        out, shares, final = gen.run_case(case)
    finally:
        os.chdir(cwd)
        sys.path[:] = path
    g = golden(ae.fixture_name(case))
    assert sorted(out) == sorted(g)
    for k, ref in g.items():
        got = np.asarray(out[k])
        assert got.shape == ref.shape, k
        if ref.dtype.kind in 'biu':
            assert np.array_equal(got, ref), k
        elif ref.size:
            assert np.abs(got.astype(np.float64) - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max())), k
    for name, s in shares['init_opt'].items():
        assert (s < 1e-4) if name in ae.ZERO_AT_START[case]['init_opt'] else (s >= gen.MIN_SHARE), (name, s)
