"""CPU: the pose VJP (csrc/grecon_pose_bwd.hpp, what glamr_grecon_pose_backward launches) on the single-threaded host runtime against the
fp64 autograd reference of tests/extra_loss_common.py, the basis of its tolerances (floors, screening, mutations), the entry point's argument
checks, and the combinations GlobalReconOptimizer.extra_loss refuses."""
import ctypes

import numpy as np
import pytest

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import extra_loss_common as xc
from tests import hostsim


def _addr(a):
    return None if a is None else a.ctypes.data


def host_vjp(case, G, accumulate=0, before=None, flags=None, var_mask=None, arrays=None):
    """The header's algorithm on the host runtime (the device's order of additions in the scans) -> (rc, the gradient array (S * scene_stride,))."""
    lib = hostsim.build('grecon_pose_bwd_host')
    lib.hostsim_grecon_pose_bwd.restype = ctypes.c_int
    lib.hostsim_grecon_pose_bwd.argtypes = [ctypes.POINTER(_lib.SceneBatch), ctypes.POINTER(_lib.StageDesc)] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    lib.hostsim_grecon_pose_bwd_workspace_floats.restype = ctypes.c_size_t
    a = xc.host_arrays(case) if arrays is None else arrays
    sb = xc.scene_batch(case, {k: v.ctypes.data for k, v in a.items()})
    sd = xc.stage_desc(case, flags, var_mask)
    G = [None if g is None else np.ascontiguousarray(g, np.float32) for g in G]
    out = np.full(case['S'] * xc.layout(case)['scene_stride'], 7.0, np.float32) if before is None else before.copy()
    ws = np.full(lib.hostsim_grecon_pose_bwd_workspace_floats(case['S'], case['P'], case['T']), np.nan, np.float32)
    rc = lib.hostsim_grecon_pose_bwd(ctypes.byref(sb), ctypes.byref(sd), _addr(G[0]), _addr(G[1]), out.ctypes.data, accumulate, ws.ctypes.data)
    return rc, out


@pytest.mark.parametrize('name', xc.CASE_NAMES)
def test_host_algorithm_matches_fp64_autograd(name):
    """Every upstream pattern (NaN wherever the VJP must not read) within 16 x the fp32 autograd floor per variable group and person; store mode
    leaves exact zeros everywhere no variable of the mask lives."""
    case = xc.cases()['cases'][name]
    tol = xc.tol(name)
    worst = {k: 0.0 for k in xc.GROUPS}
    for pattern in xc.PATTERNS:
        rc, got = host_vjp(case, xc.upstream(case, pattern))
        assert rc == 0
        assert np.isfinite(got).all()
        assert (got[~xc.written_mask(case)] == 0).all()
        e = xc.errors(case, got, xc.ref64(name, pattern))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('host pose VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, worst[k], tol[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


@pytest.mark.parametrize('scale', xc.SCALES)
def test_scaled_upstream_gradients_stay_within_the_tolerances(scale):
    for name in xc.CASE_NAMES:
        case = xc.cases()['cases'][name]
        rc, got = host_vjp(case, xc.upstream(case, 'all', scale=scale))
        e = xc.errors(case, got, xc.reference(case, 'all', scale=scale))
        for k, v in e.items():
            assert rc == 0 and v <= xc.tol(name)[k], (name, k, v)


def pow2_grid(shape, seed):
    """Multiples of 2^-6 in [-1, 1]."""
    return (np.random.default_rng(seed).integers(-64, 65, size=shape) / 64.0).astype(np.float32)


@pytest.mark.parametrize('name', ['batch_wd', 'norot', 'frozen_wd'])
def test_add_mode_is_store_mode_plus_the_previous_contents(name):
    """Upstream gradients and previous contents on a power-of-two grid; add mode performs one fp32 addition per entry, so it equals
    fl(before + stored) bit for bit.  Entries no variable of the mask owns (local_rot without its bit, the camera block, empty and frozen
    slots, rows beyond a range) keep their previous bits, NaN included."""
    case = xc.cases()['cases'][name]
    G = tuple(np.round(g * 64) / 64 for g in xc.upstream(case, 'all'))
    rc, stored = host_vjp(case, G)
    assert rc == 0
    before = pow2_grid(stored.shape, 3)
    w = xc.written_mask(case)
    before[~w] = np.nan
    rc, added = host_vjp(case, G, accumulate=1, before=before)
    assert rc == 0
    assert np.array_equal(added[w], before[w] + stored[w])
    assert np.isnan(added[~w]).all()
    rc, again = host_vjp(case, G, accumulate=1, before=before)
    assert np.array_equal(again, added, equal_nan=True)


def test_var_mask_without_local_rot_leaves_its_block_zero_or_untouched():
    case = xc.cases()['cases']['norot_wd']
    l = xc.layout(case)
    b = xc.block(case, 0, 0)
    rot = slice(b + l['local_rot'], b + l['local_rot'] + 6 * case['T'])
    G = xc.upstream(case, 'all')
    _, stored = host_vjp(case, G)
    assert (stored[rot] == 0).all()
    before = np.full(stored.shape, 5.0, np.float32)
    _, added = host_vjp(case, G, accumulate=1, before=before)
    assert (added[rot] == 5.0).all()
    _, full = host_vjp(case, G, var_mask=xc.ALL_VARS)
    assert np.abs(full[rot]).max() > 0
    keep = np.ones(stored.shape, bool)
    keep[rot] = False
    assert np.array_equal(full[keep], stored[keep])


def test_argument_checks():
    case = xc.cases()['cases']['one24']
    G = xc.upstream(case, 'all')
    assert host_vjp(case, (None, None))[0] == -1                                         # no upstream gradient
    rc, _ = host_vjp(case, G, flags=packing.FLAG_ABSOLUTE_HEADING)
    assert rc == -4                                                                      # GLAMR_E_UNSUPPORTED
    a = xc.host_arrays(case)
    a.pop('traj_local_pred')
    assert host_vjp(case, G, arrays=a)[0] == -1
    a = xc.host_arrays(case)
    a.pop('base_orient')
    assert host_vjp(case, G, arrays=a)[0] == 0                                           # not needed without world_dheading ...
    assert host_vjp(case, G, arrays=a, flags=packing.FLAG_HAS_WORLD_DHEADING)[0] == -1   # ... needed with it


def test_library_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    """The checks of the real entry point run before any HIP call."""
    from glamr_amd import build
    build.build_library()
    L = _lib.lib()
    assert L.glamr_grecon_pose_backward_workspace_bytes(0, 1, 24) == 0
    assert L.glamr_grecon_pose_backward_workspace_bytes(2, 3, 24) == 2 * 3 * 24 * 27 * 4
    sb, sd = _lib.SceneBatch(), _lib.StageDesc()
    bogus = ctypes.c_void_p(16)
    assert L.glamr_grecon_pose_backward(None, ctypes.byref(sd), bogus, bogus, bogus, 0, bogus, None) == -1
    assert L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), bogus, bogus, bogus, 0, bogus, None) == -1
    assert b'geometry' in L.glamr_last_error()
    sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = 1, 1, 24, 26
    assert L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), None, None, bogus, 0, bogus, None) == -1
    assert b'at least one' in L.glamr_last_error()
    sd.flags = packing.FLAG_ABSOLUTE_HEADING
    assert L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), bogus, bogus, bogus, 0, bogus, None) == -4
    assert b'ABSOLUTE_HEADING' in L.glamr_last_error()
    sd.flags = 0
    assert L.glamr_grecon_pose_backward(ctypes.byref(sb), ctypes.byref(sd), bogus, bogus, bogus, 0, bogus, None) == -1
    assert b'NULL batch array' in L.glamr_last_error()


def test_floors_and_screening():
    st = xc.cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    assert set(st['cases']) == set(xc.CASE_NAMES)
    assert st['dropped'] <= xc.MAX_DROPPED_SHARE * st['generated']
    for name in st['cases']:
        f = xc.measure_floor(name)
        print('floor %s: %s' % (name, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], xc.FLOOR[name][k]) for k in f)))
        for k, v in f.items():
            c = xc.FLOOR[name][k]
            assert 0.5 * c <= v <= 2.0 * c, (name, k, v, c)


def _touches(mut, case, p):
    """Whether the mutation changes the gradient of this person at all."""
    n, fs, Ts = p['n'], p['fs'], p['Ts']
    if mut == 'mask':
        return n >= 2                                                       # some masked row exists: rows 1 .. min(5, n - 1) (all of them by default)
    if mut == 'wd_disp':
        return case['wd'] and n >= 2
    if mut == 'vec_add':
        return n >= 7 and case['fix'] != xc.DEFAULT_FIX                     # an unmasked row of local_dheading
    if mut == 'outside':
        return n < Ts
    if mut == 'var_mask':
        return case['var_mask'] != xc.ALL_VARS
    return True                                                             # row0


@pytest.mark.parametrize('mut', list(xc.MUTATIONS))
def test_mutations_of_the_reference_are_caught(mut):
    """Each mutation of the reference moves some compared group of every person it touches by at least 2 tolerances."""
    touched = 0
    for name, case in xc.cases()['cases'].items():
        keys = [k for k, p in xc.live(case).items() if _touches(mut, case, p)]
        if not keys:
            continue
        ref, bad, tol = xc.ref64(name, 'all'), xc.reference(case, 'all', mut=mut), xc.tol(name)
        for key in keys:
            e = xc.person_errors(case, bad, ref, key)
            ratio = max(e[k] / tol[k] if tol[k] > 0 else (np.inf if e[k] > 0 else 0.0) for k in e)
            print('mutation %-8s %-10s person %s: %s -> %.3g tolerances' % (mut, name, key, ', '.join('%s %.2e' % kv for kv in e.items()), ratio))
            assert ratio >= 2.0, (mut, name, key, e, tol)
            touched += 1
    assert touched > 0


# ---- the schedule: the end-to-end reference and the refused combinations --------------------------------------------------------------------
@pytest.mark.parametrize('run', ['rot', 'trans', 'heels'])
def test_e2e_reference_fixture_and_floors(asset_root, golden, run):
    """The fp64 port with the term, run again: the fixture the device tests read holds its results, and the fp32 run's deviation is the stored
    floor within [1/2, 2]."""
    from tests import extra_loss_e2e as xe
    ref = xe.reference(asset_root, run)
    g = xe.from_fixture(golden(xe.FIXTURE), run)
    assert set(g) == set(ref)
    for k, v in ref.items():
        assert g[k].shape == v.shape and (v.size == 0 or np.abs(g[k] - v).max() <= 1e-9 * max(1.0, np.abs(v).max())), k
    f = xe.measure_floor(asset_root, run)
    print('e2e floor %s: %s' % (run, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], xe.FLOOR[run][k]) for k in f)))
    for k, v in f.items():
        assert 0.5 * xe.FLOOR[run][k] <= v <= 2.0 * xe.FLOOR[run][k], (run, k, v)


def test_refused_combinations():
    import torch
    from glamr_amd.global_recon import extra_loss_schedule as xs
    from glamr_amd.global_recon.configs import get_config
    for cfg_id in ('glamr_dynamic', 'glamr_static_multi', 'glamr_3dpw'):
        xs.check_supported(get_config(cfg_id)['grecon_model_specs'])
    for flags, word in ((dict(flag_opt_motion_latent=True), 'latent'), (dict(flag_opt_traj_latent=True), 'latent'),
                        (dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'), (dict(absolute_heading=True), 'absolute_heading')):
        with pytest.raises(ValueError, match=word):
            xs.check_supported(dict(get_config('glamr_dynamic')['grecon_model_specs'], **flags))

    class Packed:
        t = {'frozen': torch.zeros(2, dtype=torch.int32)}
    with pytest.raises(ValueError, match='person-sharded'):
        xs.check_not_sharded(Packed())
    Packed.t = {}
    xs.check_not_sharded(Packed())
