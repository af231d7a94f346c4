"""CPU: the basis of the penetration term's tolerances -- the generated meshes, the fp32 floors of the restatement in
tests/penetration_common.py, the screening cap, what each case exercises, the mutations -- and the kernels' arithmetic (csrc/sdf.hpp on the
host, tests/hostsim/sdf_host.cpp) against the fp64 restatement, the entry point's argument checks, and the host-side routing helpers."""
import ctypes

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from tests import hostsim
from tests import penetration_common as pc


def host_penetration(case, want_grad=True, verts=None):
    """csrc/sdf.hpp in the kernels' order of operations on the host -> (rc, outputs), every output poisoned beforehand."""
    lib = hostsim.build('sdf_host')
    lib.hostsim_sdf_penetration.restype = ctypes.c_int
    lib.hostsim_sdf_penetration.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + [ctypes.c_void_p] * 5
    v = np.ascontiguousarray(case['verts'] if verts is None else verts, np.float32)
    F_, P, V, _ = v.shape
    G = case['G']
    out = dict(loss=np.full(F_, np.nan, np.float32), g_verts=np.full(v.shape, np.nan, np.float32), phi=np.full((F_, P, G, G, G), np.nan, np.float32),
               boxes=np.full((F_, P, 2, 3), np.nan, np.float32), overlap=np.full((F_, P), -7, np.int32))
    rc = lib.hostsim_sdf_penetration(v.ctypes.data, case['active'].ctypes.data, case['faces'].ctypes.data, F_, P, V, len(case['faces']), G,
                                     case['scale_factor'], case['rho'], out['loss'].ctypes.data, out['g_verts'].ctypes.data if want_grad else None,
                                     out['phi'].ctypes.data, out['boxes'].ctypes.data, out['overlap'].ctypes.data)
    return rc, out


def test_meshes_are_closed_oriented_outwards_and_off_the_tile_sizes():
    for level, (nv, nf) in ((1, (42, 80)), (2, (162, 320))):
        v, f = pc.icosphere(level)
        assert (len(v), len(f)) == (nv, nf) and pc.is_closed_and_oriented(f)
    assert not pc.is_closed_and_oriented(pc.icosphere(1)[1][:-1])                       # (the check sees a missing face)
    assert not pc.is_closed_and_oriented(np.concatenate([pc.icosphere(1)[1][:-1], pc.icosphere(1)[1][-1:, ::-1]]))      # (and a flipped one)
    for name, case in pc.cases().items():
        F_, P, V, _ = case['verts'].shape
        assert pc.is_closed_and_oriented(case['faces']) and case['faces'].min() == 0 and case['faces'].max() == V - 1
        assert V % 64 and len(case['faces']) % 256 and F_ <= 4 and P in (2, 3)          # (256 faces = the grid kernel's LDS tile)
        for f in range(F_):
            for p in range(P):
                assert pc.signed_volume(case['verts_full'][f, p], case['faces']) > 0, (name, f, p)
                assert np.isnan(case['verts'][f, p]).all() == (case['active'][f, p] == 0)


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_floors_are_what_is_recorded_and_the_screening_stays_under_its_cap(name):
    """The tolerances are 16 x the fp32 restatement's error against fp64: re-measured here, each within [1/2, 2] x its recorded constant (boxes
    and flags exactly 0); the fp64 reference alone decides the screening, at most 2 % of the sampled vertices."""
    floors = pc.measure_floors(name)
    print('floors %s: %s' % (name, ', '.join('%s %.2e (recorded %.2e)' % (k, floors[k], pc.FLOORS[name][k]) for k in pc.OUTPUTS)))
    for k in pc.OUTPUTS:
        rec = pc.FLOORS[name][k]
        assert (floors[k] == 0.0) if rec == 0.0 else (0.5 * rec <= floors[k] <= 2.0 * rec), (name, k, floors[k], rec)
    keep, share = pc.screen(name)
    assert share <= pc.SCREEN_CAP, (name, share)
    assert np.isfinite(pc.ref64(name)['frac']).sum() >= 42                               # (something is sampled in every case)


def test_cases_exercise_what_they_are_for():
    r = {n: pc.ref64(n) for n in pc.CASE_NAMES}
    c = pc.cases()
    for n in pc.CASE_NAMES:                                                              # every case has a frame with a real penetration
        assert r[n]['loss'].max() > 1e-2 and np.abs(r[n]['g_verts']).max() > 1e-2, n
    # a third, isolated body: flag 0, no gradient, and the frame is divided by 2^2, not 3^2
    t = r['third_isolated']
    assert t['overlap'].tolist() == [[1, 1, 0], [1, 1, 1]] and (t['g_verts'][0, 2] == 0).all() and (t['phi'][0, 2] == 0).all()
    assert abs(pc.restate(c['third_isolated'], torch.float64, 'no_nf2')['loss'][0] / t['loss'][0] - 4.0) < 1e-12
    assert np.abs(t['g_verts'][1]).reshape(3, -1).max(1).min() > 0                      # (three bodies, each sampled in the other two)
    # boxes 1e-3 apart, 1e-3 into each other, touching exactly, and well into each other
    b = r['touch']['boxes']
    gap = b[:, 1, 0, 0] - b[:, 0, 1, 0]
    assert r['touch']['overlap'].tolist() == [[0, 0], [1, 1], [1, 1], [1, 1]]
    assert 0.5e-3 < gap[0] < 1.5e-3 and -1.5e-3 < gap[1] < -0.5e-3 and gap[2] == 0.0 and r['touch']['loss'][0] == 0 and (r['touch']['g_verts'][0] == 0).all()
    # one active person, nobody, two of three
    g = r['gates']
    assert g['overlap'].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 1]] and (g['loss'][:2] == 0).all() and (g['g_verts'][:2] == 0).all() and (g['g_verts'][2, 1] == 0).all()
    assert (g['boxes'][0, 0] == 0).all() and (g['boxes'][1] == 0).all() and np.isfinite(g['boxes']).all()
    # sampled points outside [-1, 1] and in the outer half cell, some of the latter with a value (partial zero padding that matters)
    cp, rp = c['padding'], r['padding']
    G = cp['G']
    seen_outside = seen_half = 0
    for f in range(2):
        for p, q in ((0, 1), (1, 0)):
            lo, hi = rp['boxes'][f, p]
            u = (cp['verts'][f, q].astype(np.float64) - (lo + hi) / 2) / (0.5 * (hi - lo).max())
            fx = ((u + 1) * G - 1) / 2
            outside = (np.abs(u) > 1).any(1)
            half = ~outside & ((fx < 0) | (fx > G - 1)).any(1)
            val = torch.nn.functional.grid_sample(torch.tensor(rp['phi'][f, p])[None, None], torch.tensor(u)[None, None, None], align_corners=False)[0, 0, 0, 0].numpy()
            seen_outside += int(outside.sum())
            seen_half += int((half & (val > 1e-3)).sum())
    assert seen_outside >= 10 and seen_half >= 2, (seen_outside, seen_half)
    # two lobes through each other: voxels with winding number 2, which are inside
    cl, rl = c['lobes'], r['lobes']
    lo, hi = rl['boxes'][0, 0]
    xn = torch.tensor((cl['verts'][0, 0].astype(np.float64) - (lo + hi) / 2) / (0.6 * (hi - lo).max()))
    k = -1.0 + (2.0 * torch.arange(8, dtype=torch.float64) + 1.0) / 8
    pts = torch.stack(torch.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3).flip(-1)
    fc = torch.as_tensor(cl['faces'], dtype=torch.long)
    w = pc.winding_number(pts[:, None], xn[fc[:, 0]][None], xn[fc[:, 1]][None], xn[fc[:, 2]][None]).numpy()
    assert (np.abs(w - np.round(w)) < 1e-9).all() and (np.round(w) == 2).sum() >= 3
    assert (rl['phi'][0, 0].reshape(-1)[np.round(w) == 2] > 0).all()
    assert c['g32']['G'] == 32 and all(c[n]['G'] == 8 for n in pc.CASE_NAMES if n != 'g32')
    assert c['two_overlap_linear']['rho'] == 0.0 and c['two_overlap']['rho'] == 1.0


def test_frame_term_is_the_restatement_of_an_all_active_frame():
    for name in ('third_isolated', 'two_overlap_linear'):
        case, ref = pc.cases()[name], pc.ref64(name)
        for f in range(case['verts'].shape[0]):
            x = torch.tensor(case['verts'][f], dtype=torch.float64, requires_grad=True)
            v = pc.frame_term(x, case['faces'], case['G'], case['scale_factor'], case['rho'])
            g, = torch.autograd.grad(v, x)
            assert abs(float(v) - ref['loss'][f]) <= 1e-14 and np.abs(g.numpy() - ref['g_verts'][f]).max() <= 1e-14


@pytest.mark.parametrize('mut', pc.MUTATIONS)
def test_every_mutation_of_the_restatement_moves_an_output_by_two_tolerances(mut):
    """What the bounds can tell apart: each mutation moves some compared output of every case it touches by at least 2 tolerances."""
    for name in pc.touched(mut):
        e = pc.errors(name, pc.restate(pc.cases()[name], torch.float64, mut))
        tol = pc.tol(name)
        moved = {k: e[k] for k in pc.OUTPUTS if e[k] > 0 and e[k] >= 2 * tol[k]}
        print('%s on %s: %s' % (mut, name, ', '.join('%s %.2e (%.0f tol)' % (k, v, v / tol[k] if tol[k] else np.inf) for k, v in moved.items())))
        assert moved, (mut, name, e, tol)


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_host_arithmetic_matches_the_fp64_restatement(name):
    """csrc/sdf.hpp as the kernels run it, NaN in everything that must not be read, every output poisoned before the call."""
    case = pc.cases()[name]
    rc, got = host_penetration(case)
    assert rc == 0 and all(np.isfinite(got[k]).all() for k in pc.OUTPUTS)
    e, tol = pc.errors(name, got), pc.tol(name)
    print('host sdf %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, e[k], tol[k]) for k in pc.OUTPUTS)))
    for k in pc.OUTPUTS:
        assert e[k] <= tol[k], (name, k, e[k], tol[k])
    inactive = case['active'] == 0
    assert (got['g_verts'][inactive] == 0).all() and (got['g_verts'][got['overlap'] == 0] == 0).all() and (got['phi'][got['overlap'] == 0] == 0).all()
    rc, fwd = host_penetration(case, want_grad=False)
    assert rc == 0 and np.array_equal(fwd['loss'], got['loss'])


def test_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    from glamr_amd import build
    build.build_library()
    L = _lib.lib()
    ok = (2, 2, 42, 80, 8)
    assert L.glamr_sdf_workspace_bytes(*ok) >= 2 * 2 * 8 ** 3 * 4
    p = ctypes.c_void_p(256)
    for bad, word in (((2, 0, 42, 80, 8), 'P'), ((2, 33, 42, 80, 8), 'P'), ((2, 2, 42, 80, 1), 'grid'), ((2, 2, 42, 80, 65), 'grid'), ((-1, 2, 42, 80, 8), 'F'),
                      ((2, 2, 0, 80, 8), 'V'), ((2, 2, 42, 0, 8), 'NF')):
        assert L.glamr_sdf_workspace_bytes(*bad) == 0
        F_, P, V, NF, G = bad
        assert L.glamr_sdf_penetration(p, p, p, F_, P, V, NF, G, 0.2, 1.0, p, None, None, None, None, p, None) == -1
        assert b'bad sizes' in L.glamr_last_error()
    assert L.glamr_sdf_penetration(p, p, p, 2, 2, 42, 80, 8, 0.2, -1.0, p, None, None, None, None, p, None) == -1 and b'rho' in L.glamr_last_error()
    assert L.glamr_sdf_penetration(None, p, p, 2, 2, 42, 80, 8, 0.2, 1.0, p, None, None, None, None, p, None) == -1 and b'NULL' in L.glamr_last_error()
    assert L.glamr_sdf_penetration(p, p, p, 2, 2, 42, 80, 8, 0.2, 1.0, p, None, None, None, None, None, None) == -1
    assert L.glamr_sdf_penetration(None, None, None, 0, 2, 42, 80, 8, 0.2, 1.0, None, None, None, None, None, None, None) == 0      # no frames: nothing to do


def test_sdf_loss_has_no_cpu_path():
    from glamr_amd.lib.models.sdf import SDFLoss
    v, f = pc.icosphere(1)
    loss = SDFLoss(f, grid_size=8, robustifier=True)
    assert loss.rho == 1.0 and SDFLoss(f).rho == 0.0 and SDFLoss(f).grid_size == 32
    with pytest.raises(RuntimeError, match='HIP device'):
        loss(torch.zeros(2, 42, 3))
    with pytest.raises(ValueError):
        SDFLoss(f[:, :2])
    with pytest.raises(ValueError):
        SDFLoss(f, grid_size=65)


# ---- host-side routing and the end-to-end reference --------------------------------------------------------------------------------------------
def test_packing_takes_the_term_off_loss_cfg_and_checks_the_flag():
    from glamr_amd.global_recon import packing
    cfg = {'kp_2d': dict(weight=1.0), 'penetration': dict(weight=3.0, monitor_only=True)}
    rest, pen = packing.split_penetration(cfg)
    assert list(rest) == ['kp_2d'] and pen == dict(weight=3.0, monitor_only=True) and 'penetration' in cfg
    assert packing.split_penetration(rest) == (rest, None)
    assert packing.split_penetration({'penetration': dict(weight=2)})[1] == dict(weight=2.0, monitor_only=False)
    with pytest.raises(NotImplementedError, match='penetration'):                         # the stage kernel still has no such term
        packing.stage_desc(dict(opt_variables=['cam'], opt_niters=1, opt_lr=0.1, loss_cfg=cfg), {})
    packing.stage_desc(dict(opt_variables=['cam'], opt_niters=1, opt_lr=0.1, loss_cfg=rest), {})
    stages = {'a': dict(loss_cfg=rest), 'b': dict(loss_cfg=cfg)}
    with pytest.raises(ValueError, match="'penetration' in stage 'b' needs flag_use_pen_loss"):
        packing.check_penetration(stages, {})
    packing.check_penetration(stages, dict(flag_use_pen_loss=True))
    packing.check_penetration({'a': dict(loss_cfg=rest)}, {})


def test_end_to_end_fixture_meets_its_conditions_and_is_the_ports(asset_root, golden):
    """On the fp64 reference: the hull is closed, at least 8 frames carry a non-zero term and the term's share of the first gradient's norm is at
    least 1 %.  The first stage's first gradient of the file is a fresh fp64 run of the port's, and the fp32 port's distance to it stays under
    twice the recorded floor (no lower limit: that floor is one or two of 317 000 sampled vertices changing their cell between fp32 and
    fp64 -- a step, not a rounding level -- so another host's fp32 summation order may well miss the step)."""
    from tests import penetration_e2e as pe
    faces = pe.hull_faces()
    assert pc.is_closed_and_oriented(faces) and faces.max() < 6890
    from glamr_amd.utils import synth
    assert pc.signed_volume(synth.make_smpl_model()['v_template'], faces) > 0
    ref = dict(golden(pe.FIXTURE))
    assert int((ref['frames'] > 0).sum()) >= 8 and pe.term_share(ref) >= 0.01, (ref['frames'], pe.term_share(ref))
    assert all(ref[k].shape == (1, pe.K) and (ref[k] > 0).all() for k in ref if k.endswith('/history'))
    fresh = pe.reference(asset_root, first_only=True)
    for k, v in fresh.items():
        assert ref[k].shape == v.shape and (v.size == 0 or np.abs(v - ref[k]).max() <= 1e-9 * max(1.0, np.abs(ref[k]).max())), k
    first = pe.measure_floor(asset_root, first_only=True)['grad']
    print('end to end, first gradient: fp32 port against fp64 %.3e (recorded %.3e)' % (first, pe.FLOOR_FIRST_GRAD))
    assert first <= 2.0 * pe.FLOOR_FIRST_GRAD
    assert pe.FLOOR_FIRST_GRAD <= pe.FLOOR['grad'] and set(pe.FLOOR) == set(pe.KINDS)
