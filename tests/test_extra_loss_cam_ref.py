"""CPU: the camera VJP (csrc/grecon_cam_bwd.hpp, what glamr_grecon_cam_backward launches) on the single-threaded host runtime against the
fp64 autograd reference of tests/extra_loss_cam_common.py, the basis of its tolerances (floors, screening, mutations), the entry point's
argument checks, and the context's projection against the port's."""
import ctypes

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from tests import extra_loss_cam_common as cc
from tests import hostsim


def host_vjp(case, G, accumulate=0, before=None, pose_before=None, mode=None, arrays=None, null_pose=False):
    """The header's algorithm on the host runtime -> (rc, dict(grads (S * scene_stride,), g_orient_world, g_trans_world (S * P, T, 3)))."""
    lib = hostsim.build('grecon_cam_bwd_host')
    lib.hostsim_grecon_cam_bwd.restype = ctypes.c_int
    lib.hostsim_grecon_cam_bwd.argtypes = [ctypes.POINTER(_lib.SceneBatch), ctypes.POINTER(_lib.StageDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.hostsim_grecon_cam_bwd_workspace_floats.restype = ctypes.c_size_t
    a = cc.host_arrays(case) if arrays is None else arrays
    sb = cc.scene_batch(case, {k: v.ctypes.data for k, v in a.items()})
    sd = cc.stage_desc(case, mode)
    G = None if G is None else np.ascontiguousarray(G, np.float32)
    S, P, T = case['S'], case['P'], case['T']
    out = np.full(S * cc.layout(case)['scene_stride'], 7.0, np.float32) if before is None else before.copy()
    go, gt = (np.zeros((S * P, T, 3), np.float32) if pose_before is None else pose_before[i].copy() for i in range(2))
    ws = np.full(max(1, lib.hostsim_grecon_cam_bwd_workspace_floats(S, P, T)), np.nan, np.float32)
    rc = lib.hostsim_grecon_cam_bwd(ctypes.byref(sb), ctypes.byref(sd), None if G is None else G.ctypes.data, out.ctypes.data, accumulate,
                                    None if null_pose else go.ctypes.data, None if null_pose else gt.ctypes.data, ws.ctypes.data)
    return rc, dict(grads=out, g_orient_world=go, g_trans_world=gt)


def check_result(case, got):
    """Finite where written, exact zeros in store mode everywhere else, pose gradients only where a live person is visible."""
    w, pw = cc.written_mask(case), cc.pose_written_mask(case)
    assert np.isfinite(got['grads']).all()
    assert (got['grads'][~w] == 0).all()
    for k in cc.POSE_GROUPS:
        assert np.isfinite(got[k]).all() and (got[k][~pw] == 0).all()


@pytest.mark.parametrize('name', cc.CASE_NAMES)
def test_host_algorithm_matches_fp64_autograd(name):
    """Every upstream pattern (NaN wherever the VJP must not read) within 16 x the fp32 autograd floor per group and scene / person."""
    case = cc.cases()['cases'][name]
    tol = cc.tol(name)
    worst = {k: 0.0 for k in cc.GROUPS}
    for pattern in cc.PATTERNS:
        rc, got = host_vjp(case, cc.upstream(case, pattern))
        assert rc == 0
        check_result(case, got)
        e = cc.errors(case, got, cc.ref64(name, pattern))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('host camera VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, worst[k], tol[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


@pytest.mark.parametrize('scale', cc.SCALES)
def test_scaled_upstream_gradients_stay_within_the_tolerances(scale):
    for name in cc.CASE_NAMES:
        case = cc.cases()['cases'][name]
        rc, got = host_vjp(case, cc.upstream(case, 'all', scale=scale))
        e = cc.errors(case, got, cc.reference(case, 'all', scale=scale))
        for k, v in e.items():
            assert rc == 0 and v <= cc.tol(name)[k], (name, k, v)


def pow2_grid(shape, seed):
    """Multiples of 2^-6 in [-1, 1]."""
    return (np.random.default_rng(seed).integers(-64, 65, size=shape) / 64.0).astype(np.float32)


@pytest.mark.parametrize('name', ['frame_batch', 'fixed_short', 'derived40', 'derived_frozen'])
def test_add_mode_is_store_mode_plus_the_previous_contents(name):
    """Add mode performs one fp32 addition per owned entry: fl(before + stored) bit for bit; every other entry of the gradient array keeps its
    bits, NaN included.  The pose buffers are added into in BOTH settings, and only where a live person is visible."""
    case = cc.cases()['cases'][name]
    G = cc.upstream(case, 'all')
    zero = host_vjp(case, G)[1]
    S, P, T = case['S'], case['P'], case['T']
    pw = cc.pose_written_mask(case)
    pose_before = [pow2_grid((S * P, T, 3), 5 + i) for i in range(2)]
    for pb in pose_before:
        pb[~pw] = np.nan
    rc, stored = host_vjp(case, G, pose_before=pose_before)
    assert rc == 0 and np.array_equal(stored['grads'], zero['grads'])
    before = pow2_grid(stored['grads'].shape, 3)
    w = cc.written_mask(case)
    before[~w] = np.nan
    rc, added = host_vjp(case, G, accumulate=1, before=before, pose_before=pose_before)
    assert rc == 0
    assert np.array_equal(added['grads'][w], before[w] + stored['grads'][w])
    assert np.isnan(added['grads'][~w]).all()
    for i, k in enumerate(cc.POSE_GROUPS):
        for r in (stored, added):
            assert np.array_equal(r[k][pw], pose_before[i][pw] + zero[k][pw]) and np.isnan(r[k][~pw]).all()
    rc, again = host_vjp(case, G, accumulate=1, before=before, pose_before=pose_before)
    assert all(np.array_equal(again[k], added[k], equal_nan=True) for k in added)


def test_mode_selection_and_argument_checks():
    case = cc.cases()['cases']['derived40']
    G = cc.upstream(case, 'all')
    # var_mask without cam together with FLAG_CAM_FROM_PERSON is the derived mode (the case's descriptor); the same batch with neither is a
    # constant camera: the error, and nothing written
    rc, got = host_vjp(case, G, mode='constant')
    assert rc == -4 and (got['grads'] == 7.0).all() and all((got[k] == 0).all() for k in cc.POSE_GROUPS)
    assert host_vjp(case, G, null_pose=True)[0] == -1                                    # a NULL pose buffer in the derived mode
    assert host_vjp(case, None)[0] == -1                                                 # a NULL g_cam_pose
    a = cc.host_arrays(case)
    a.pop('person2cam')
    assert host_vjp(case, G, arrays=a)[0] == -1
    frame = cc.cases()['cases']['frame24']
    assert host_vjp(frame, cc.upstream(frame, 'all'), null_pose=True)[0] == 0            # ignored in the optimised modes


def test_library_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    """The checks of the real entry point run before any HIP call."""
    from glamr_amd import build
    from glamr_amd.global_recon import packing
    build.build_library()
    L = _lib.lib()
    assert L.glamr_grecon_cam_backward_workspace_bytes(0, 1, 24) == 0
    assert L.glamr_grecon_cam_backward_workspace_bytes(2, 3, 24) == 2 * 24 * 13 * 4
    sb, sd = _lib.SceneBatch(), _lib.StageDesc()
    bogus = ctypes.c_void_p(16)
    call = lambda g, go, gt: L.glamr_grecon_cam_backward(ctypes.byref(sb), ctypes.byref(sd), g, bogus, 0, go, gt, bogus, None)
    assert L.glamr_grecon_cam_backward(None, ctypes.byref(sd), bogus, bogus, 0, bogus, bogus, bogus, None) == -1
    assert call(bogus, bogus, bogus) == -1 and b'geometry' in L.glamr_last_error()
    sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = 1, 1, 24, 26
    assert call(None, bogus, bogus) == -1 and b'g_cam_pose' in L.glamr_last_error()
    assert call(bogus, bogus, bogus) == -4 and b'constant' in L.glamr_last_error()
    sd.flags = packing.FLAG_CAM_FROM_PERSON
    assert call(bogus, None, bogus) == -1 and b'g_orient_world' in L.glamr_last_error()
    assert call(bogus, bogus, bogus) == -1 and b'NULL batch array' in L.glamr_last_error()
    sd.var_mask, sd.flags = packing.VAR_BITS['cam'], 0
    assert call(bogus, None, None) == -1 and b'NULL batch array' in L.glamr_last_error()


def test_restated_block_is_the_ports():
    """The copy of the port's camera block the mutations are applied to gives the port's numbers bit for bit and its gradients to fp64
    rounding (the port fills the person-less frames in a loop, the copy with one gather: another order of additions in the backward)."""
    for name, case in cc.cases()['cases'].items():
        for sc in case['scenes']:
            out = []
            for mut in (None, ''):
                lv = cc.leaves(case, sc, torch.float64)
                cam, _ = cc.cam_block(case, sc, lv, mut)
                w = torch.tensor(cc.upstream(case, 'all', nan_pad=False).reshape(case['S'], case['T'], 3, 4)[cc.scene_index(case, sc), :sc['Ts']], dtype=torch.float64)
                out.append([cam.detach()] + list(torch.autograd.grad((w * cam[:, :3, :4]).sum(), list(lv.values()), allow_unused=True)))
            assert torch.equal(out[0][0], out[1][0]), name
            for a, b in zip(out[0][1:], out[1][1:]):
                assert (a is None and b is None) or torch.allclose(a, b, rtol=1e-12, atol=1e-13 * float(a.abs().max())), name


def test_floors_and_screening():
    st = cc.cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    assert set(st['cases']) == set(cc.CASE_NAMES)
    assert st['dropped'] <= cc.MAX_DROPPED_SHARE * st['generated']
    for name in st['cases']:
        f = cc.measure_floor(name)
        print('floor %s: %s' % (name, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], cc.FLOOR[name][k]) for k in f)))
        for k, v in f.items():
            c = cc.FLOOR[name][k]
            assert 0.5 * c <= v <= 2.0 * c, (name, k, v, c)


@pytest.mark.parametrize('mut', list(cc.MUTATIONS))
def test_mutations_of_the_reference_are_caught(mut):
    """Each mutation of the reference moves some compared group of every scene it touches by at least 2 tolerances."""
    touched = 0
    for name, case in cc.cases()['cases'].items():
        scenes = [si for si in range(case['S']) if cc.touches(mut, case, si)]
        if not scenes:
            continue
        ref, bad, tol = cc.ref64(name, 'all'), cc.reference(case, 'all', mut=mut), cc.tol(name)
        for si in scenes:
            e = cc.scene_errors(case, bad, ref, si)
            ratio = max(e[k] / tol[k] if tol[k] > 0 else (np.inf if e[k] > 0 else 0.0) for k in e)
            print('mutation %-12s %-14s scene %d: %s -> %.3g tolerances' % (mut, name, si, ', '.join('%s %.2e' % kv for kv in e.items()), ratio))
            assert ratio >= 2.0, (mut, name, si, e, tol)
            touched += 1
    assert touched > 0


def test_context_projection_is_the_ports():
    """ExtraLossContext.project on the CPU: perspective_projection(transform_trans(cam_pose, x), cam_K) as the port states it."""
    from oracle.port import transforms as tf
    from glamr_amd.global_recon import extra_loss_schedule as xs
    rng = np.random.default_rng(0)
    S, P, T, N = 2, 2, 5, 7
    cam = torch.tensor(rng.normal(size=(S, T, 3, 4)))
    K = torch.tensor(rng.normal(size=(S, P, T, 3, 3)))
    x = torch.tensor(rng.normal(size=(S, P, T, N, 3)))
    ctx = xs.ExtraLossContext(None, 'stage', 0, None, None, None, torch.ones(S, P, T, dtype=torch.bool), None, None, None, cam_pose=cam, cam_K=K)
    got = ctx.project(x)
    for si in range(S):
        M = torch.cat([cam[si], torch.tensor([[[0, 0, 0, 1.0]]]).repeat(T, 1, 1)], dim=1)
        for pi in range(P):
            ref = tf.project(tf.apply_transform(M, x[si, pi]), K[si, pi])
            assert torch.allclose(got[si, pi], ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('run', ['kp', 'height', 'heels'])
def test_e2e_reference_fixture_and_floors(asset_root, golden, run):
    """The fp64 port with the term, run again: the fixture the device tests read holds its results (and the heel targets), and the fp32 run's
    deviation -- end to end and of the kp_2d-only gradient the agreement test is bounded by -- is the stored floor within [1/2, 2]."""
    from tests import extra_loss_cam_e2e as ce
    ref = ce.reference(asset_root, run)
    g = ce.from_fixture(golden(ce.FIXTURE), run)
    assert set(g) == set(ref)
    for k, v in ref.items():
        assert g[k].shape == v.shape and (v.size == 0 or np.abs(g[k] - v).max() <= 1e-9 * max(1.0, np.abs(v).max())), k
    if run == 'heels':
        n = ce.state(asset_root, run)[2]['fr_num_persons'].numpy()
        assert (n == 0).any() and (n == 1).any() and (n == 2).any()                 # the gap: frames with nobody, one and two persons
        for idx, t in ce.state(asset_root, run)[3].items():
            assert np.array_equal(ce.targets_from_fixture(golden(ce.FIXTURE))[idx], t.numpy())
    f, a = ce.measure_floor(asset_root, run)
    print('e2e floor %s: %s; kp_2d-only gradient %.3e (constant %.1e)' % (run, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], ce.FLOOR[run][k]) for k in f), a, ce.AGREE_FLOOR[run]))
    for k, v in f.items():
        assert 0.5 * ce.FLOOR[run][k] <= v <= 2.0 * ce.FLOOR[run][k], (run, k, v)
    assert 0.5 * ce.AGREE_FLOOR[run] <= a <= 2.0 * ce.AGREE_FLOOR[run], (run, a)
