"""MI355X: the SMPL kernels (smpl_prep_kernel, the smpl_lbs_kernel<NE, F16> instances, both finish kernels, the anchor kernels,
glamr_smpl_backward_root and the three-kernel general backward) against the fp64 reference of tests/smpl_ref_common.py, on the fixture model and
on the conditioned one, over the mixed pose families, at the smallest batch sizes that reach each path.  Every vertex of every frame is
compared; every tolerance is imported from the common module (16 x the fp32 restatement's own rounding, tests/test_smpl_ref.py); each test
prints its worst error beside its tolerance."""
import os
import numpy as np
import pytest
import torch

from tests import smpl_ref_common as sc

pytestmark = pytest.mark.gpu
FWD_BATCHES = [1, 8, 9, 32, 33, 64, 257]      # prep block edge (8 frames), frame tile edge (32), smpl_finish_small_kernel's 8-frame block, and 257:
                                              # 9 frame tiles, the first size at which the 3-tile joints pass is split over gridDim.y
GRAD_BATCHES = [1, 33, 40]


def _device_model(root, **kw):
    from glamr_amd.lib.models.smpl import SMPL
    return SMPL(os.path.join(root, 'data', 'body_models', 'smpl'), pose_type='body26fk', create_transl=False,
                extra_regressor_path=os.path.join(root, 'data', 'J_regressor_extra.npy'), **kw).to(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def ctx(asset_root, tmp_path_factory):
    """Per model: its asset directory, the fp64 reference, the device model, and the fp64 outputs of frames(257), computed once."""
    out = {}
    fr = sc.frames(sc.FWD_B)
    for name in sc.MODELS:
        root = sc.model_root(name, asset_root, tmp_path_factory.mktemp('smpl_' + name))
        m64 = sc.reference(root)
        out[name] = dict(root=root, m64=m64, mine=_device_model(root), ref=sc.forward_outputs(m64, fr))
    out['frames'] = fr
    return out


def _dev(fr, B):
    d = torch.device('cuda:0')
    return {k: torch.from_numpy(np.ascontiguousarray(v[:B])).to(d) for k, v in fr.items() if k != 'label'}


def device_outputs(mine, x, keys=sc.FWD_KEYS):
    """The calls of sc.forward_outputs on the device model."""
    o, bp, be, s, t1, t50 = x['pose'][:, :3], x['pose'][:, 3:], x['betas'], x['scale'], x['trans1'], x['trans50']
    out = {}
    with torch.no_grad():
        for k, kw in (('plain', {}), ('1m', dict(root_trans=t1, root_scale=s)), ('1m_noscale', dict(root_trans=t1)), ('50m', dict(root_trans=t50, root_scale=s))):
            if k in keys:
                r = mine(global_orient=o, body_pose=bp, betas=be, **kw)
                out[k] = {'verts': r.vertices, 'joints': r.joints}
                if k == '1m':      # the joints-only call (the 3-tile pass alone, no vertex pass) is held to the same bound
                    out['1m joints-only'] = {'joints': mine(global_orient=o, body_pose=bp, betas=be, return_verts=False, **kw).joints}
        if 'orig' in keys:
            out['orig'] = {'joints': mine(global_orient=o, body_pose=bp, betas=be, root_trans=t1, orig_joints=True).joints}
        if 'rootrel' in keys:
            out['rootrel'] = {'joints': mine.root_relative_joints(bp.contiguous(), be)}
        if 'fk' in keys:
            out['fk'] = {'joints': mine.get_joints(global_orient=o, body_pose=bp, betas=be)}
        if 'fk_anchored' in keys:
            out['fk_anchored'] = {'joints': mine.get_joints(global_orient=o, body_pose=bp, betas=be, root_trans=t1, root_scale=s)}
    return {k: {n: v.cpu().double().numpy() for n, v in d.items()} for k, d in out.items()}


def _compare(name, got, ref, B, what, ref_key=lambda k: k.split(' ')[0]):
    bad = []
    for k, d in got.items():
        rk = ref_key(k)
        for n, v in d.items():
            assert v.shape == ref[rk][n][:B].shape and np.isfinite(v).all(), (k, n)
            e, tol = float(np.abs(v - ref[rk][n][:B]).max()), sc.fwd_tol(name, rk, n)
            print('%s %s, %-16s %-6s worst %.2e m   tolerance %.2e   (%.1f fp32 floors)' % (what, name, k, n, e, tol, e / sc.FWD_FLOOR[name][rk][n]))
            if not e <= tol:
                bad.append((k, n, e, tol))
    assert not bad, bad


@pytest.mark.parametrize('B', FWD_BATCHES)
@pytest.mark.parametrize('name', sc.MODELS)
def test_forward_against_fp64(ctx, name, B):
    """Full mesh and joints, every call variant, all pose families in one batch, the two translation regimes against their own bounds."""
    c = ctx[name]
    _compare(name, device_outputs(c['mine'], _dev(ctx['frames'], B)), c['ref'], B, 'B=%d' % B)


def _lbs_frame_chunks(n_tiles, n_ftiles, nw, cus=256):
    """lbs_frame_chunks of glamr_amd/csrc/smpl.hip restated: the gridDim.y that minimises rounds x (0.35 + frame tiles per wave)."""
    best, best_cost = 1, float('inf')
    for gy in range(1, max(1, -(-n_ftiles // nw)) + 1):
        cost = -(-n_tiles * gy // cus) * (0.35 + -(-n_ftiles // (nw * gy)))
        if cost < best_cost - 1e-9:
            best, best_cost = gy, cost
    return best


def test_chunked_full_mesh_launch_repeats_the_64_frame_rows(ctx):
    """The full mesh (216 vertex tiles, 8 waves per workgroup) is launched with gridDim.y = 1 up to 104 frame tiles: 216 workgroups are one
    round of the 256 CUs and a second chunk would make two.  At 105 frame tiles (B = 3329) one chunk costs 1 x (0.35 + 14) = 14.35 and seven
    chunks 6 x (0.35 + 2) = 14.1: the first B at which a vertex is written under a chunked launch.  The batch cycles the 64 distinct frames of
    the B = 64 case (held to fp64 above); frame b must repeat row b % 64 of the 64-frame run -- at the first and last frame of every
    gridDim.y chunk, of the wave slots of chunks 0, 3 and 6, and at frames 3327 and 3328.  The bound set for this was 2 ulp of fp32 at the
    value's magnitude; on the MI355X the kernels proved bit-identical (a frame's arithmetic does not depend on its tile's place in the
    launch), so equality is asserted."""
    NW, NT = 8, 216
    assert _lbs_frame_chunks(NT, 104, NW) == 1 and all(_lbs_frame_chunks(NT, n, NW) == 1 for n in range(1, 105))
    B = 3329
    n_ft = -(-B // 32)
    gy = _lbs_frame_chunks(NT, n_ft, NW)
    assert n_ft == 105 and gy == 7
    pick = {3327, 3328}
    for y in range(gy):
        tiles = [ft for ft in range(n_ft) if (ft // NW) % gy == y]
        pick |= {tiles[0] * 32, min(B - 1, tiles[-1] * 32 + 31)}
        if y in (0, 3, 6):
            for w in (0, 7):
                slot = [ft for ft in tiles if ft % NW == w]
                pick |= {slot[0] * 32, min(B - 1, slot[-1] * 32 + 31)}
    pick = sorted(pick)
    worst, differing = 0.0, 0
    for name in sc.MODELS:
        mine = ctx[name]['mine']
        x64 = _dev(ctx['frames'], 64)
        idx = torch.arange(B, device='cuda:0') % 64
        big = {k: v[idx].contiguous() for k, v in x64.items()}
        sel = torch.tensor(pick, device='cuda:0')
        with torch.no_grad():
            a = mine(global_orient=x64['pose'][:, :3], body_pose=x64['pose'][:, 3:], betas=x64['betas'], root_trans=x64['trans1'], root_scale=x64['scale'])
            b = mine(global_orient=big['pose'][:, :3], body_pose=big['pose'][:, 3:], betas=big['betas'], root_trans=big['trans1'], root_scale=big['scale'])
            assert b.vertices.shape == (B, 6890, 3)
            for what, s, l in (('vertices', a.vertices, b.vertices), ('joints', a.joints, b.joints)):
                small, large = s[sel % 64].cpu().numpy(), l[sel].cpu().numpy()
                ulp = np.abs(large.astype(np.float64) - small) / np.spacing(np.maximum(np.abs(small), np.abs(large)))
                worst, differing = max(worst, float(ulp.max())), differing + int((large != small).sum())
                print('chunked launch, %s, %s of %d sampled frames: worst %.1f ulp, %d of %d values differ' % (name, what, len(pick), ulp.max(), (large != small).sum(), small.size))
                assert np.array_equal(large, small), (name, what, float(ulp.max()))


# joint lists that put 0 and 4 extra-regressed joints into the map: smpl_lbs_kernel<0, *> and <4, *> WITH the joints pass switched on (the
# shipped body26fk map uses two: <2, *>).  The Python class takes them as `joint_names`.
NE_NAMES = {0: ['OP MidHip', 'OP LHip', 'OP RHip', 'OP Neck', 'OP Nose', 'OP LBigToe', 'Right Pinky Tip', 'OP RWrist'],
            4: ['Pelvis (MPII)', 'OP LHip', 'Neck (LSP)', 'Spine (H36M)', 'OP Nose', 'Jaw (H36M)', 'Left Thumb Tip', 'OP RWrist', 'OP RHeel']}


@pytest.mark.parametrize('ne', [0, 4])
def test_joint_maps_with_0_and_4_extra_regressed_joints(ctx, ne):
    from glamr_amd.lib.models.smpl import JOINT_MAP
    name, B = 'conditioned', 33
    c = ctx[name]
    jm = [JOINT_MAP[n] for n in NE_NAMES[ne]]
    assert sum(j >= 45 for j in jm) == ne
    fr = {k: v[:B] for k, v in ctx['frames'].items()}
    ref = sc.forward_outputs(c['m64'], fr, joint_map=jm, keys=('plain', '1m', '50m'))
    mine = _device_model(c['root'], joint_names=NE_NAMES[ne])
    got = device_outputs(mine, _dev(fr, B), keys=('plain', '1m', '50m'))
    assert got['1m']['joints'].shape == (B, len(jm), 3)
    _compare(name, got, ref, B, 'NE=%d B=%d' % (ne, B))


@pytest.fixture(scope='module')
def grad_ref(ctx):
    fr = sc.frames(sc.GRAD_B, sc.GRAD_FAMILIES)
    return fr, {name: sc.reference_gradients(ctx[name]['m64'], fr) for name in sc.MODELS}


def _device_call(mine):
    def call(o, bp, be, t, s, orig, want_verts):
        kw = {}
        if t is not None:
            kw['root_trans'] = t
        if s is not None:
            kw['root_scale'] = s
        r = mine(global_orient=o, body_pose=bp, betas=be, orig_joints=orig, return_verts=want_verts, **kw)
        return r.vertices, r.joints
    return call


@pytest.mark.parametrize('B', GRAD_BATCHES)
@pytest.mark.parametrize('route', sc.ROUTES)
@pytest.mark.parametrize('name', sc.MODELS)
def test_backward_against_fp64_autograd(ctx, grad_ref, name, route, B):
    """glamr_smpl_backward_root (only global_orient, root_trans, root_scale require gradients) and glamr_smpl_backward (everything does), six
    losses each (the plain call has no root route), per (frame, joint) for d/d pose and per frame for the others, every small-angle level of
    d/d pose against its own tolerance.  The prefix of B frames is compared with the rows of the 40-frame fp64 gradients: the loss is a sum
    over frames, a frame's gradient does not depend on its neighbours."""
    fr, g64 = grad_ref
    sub = {k: v[:B] for k, v in fr.items()}
    mine, bad, worst = ctx[name]['mine'], [], {}
    for v in sc.variants_of(route):
        got = sc.gradients(_device_call(mine), sub, v, route, torch.float32, 'cuda:0')
        ref = {k: x[:B, :1] if (k == 'pose' and route == 'root') else x[:B] for k, x in g64[name][v].items() if k in got}
        assert set(ref) == set(got) and all(np.isfinite(x).all() for x in got.values()), v
        # the floor of the relative measure comes from the 40-frame reference tensor, as the tolerances' floors did
        full = {k: x[:, :1] if (k == 'pose' and route == 'root') else x for k, x in g64[name][v].items() if k in got}
        padded = {k: np.concatenate([got[k], full[k][B:]]) for k in got}
        for k, (err, _) in sc.grad_errors(padded, full).items():
            for grp, e in sc.worst_by_group(k, err[:B], sub['label']).items():
                tol = sc.grad_tol(name, k, grp)
                key = (k, grp)
                if e / tol > worst.get(key, (0.0,))[0]:
                    worst[key] = (e / tol, e, tol, v)
                if not e <= tol:
                    bad.append((v, k, grp, e, tol))
    for (k, grp), (_, e, tol, v) in sorted(worst.items()):
        print('%s route, %s, B=%d, d/d %-5s %-13s worst %.2e   tolerance %.2e   (%s)' % (route, name, B, k, grp, e, tol, v))
    assert not bad, bad
