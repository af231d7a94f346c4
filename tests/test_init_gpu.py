"""MI355X: the kernels of csrc/init.hip -- prep_person_kernel, init_scene_kernel, pose_scatter_kernel, cam_all_frames_kernel, check_inputs_kernel -- one
entry point per launch, against the float64 restatement of tests/init_ref_common.py on batches built for their data-dependent branches (the cases are
described where they are built, build_case()).  Tolerances: the converted rotation vectors of a slot detected in every frame within one float32 ulp
of pi (2.4e-7), within 1e-3 of angle pi as rotations at 5e-7; every other compared array within 4 d_ref + 1 ulp of its largest value, d_ref the
float32 port's own distance to float64 on the same case (D_REF, kept current by tests/test_init_ref.py); copies, masks and the zero-camera values
exactly.  Each test prints its achieved error beside its tolerance."""
import numpy as np
import pytest

from tests import init_ref_common as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    """Per case: the batch and its float64 references, computed once."""
    out = {}
    for name in ic.CASES:
        case = ic.build_case(name)
        out[name] = (case, ic.references(case))
    return out


def _judge(name, stage, errs, keys=None):
    bad = []
    for k in (keys or errs):
        e, vals = errs[k]
        tol = ic.tolerance(name, stage, k, vals)
        print('%-8s %-6s %-18s worst %.2e   tolerance %.2e' % (name, stage, k, e, tol))
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, bad


@pytest.mark.parametrize('name', ['prep', 'prep300', 'single'])
def test_prepare_against_fp64(ctx, name):
    case, refs = ctx[name]
    geo, ref = case['geo'], refs['prep']
    got = ic.launch_prepare(case)
    for k, v in got.items():
        assert np.isfinite(v).all(), k                                      # (rows without a detection hold NaN: nothing read them)
    for k in ic.PREP_EXACT:
        assert np.array_equal(got[k].astype(np.float64), np.asarray(ref[k], np.float64)), k
    rows = ic.row_mask(geo)
    assert not got['nets_pose'][~_nets_rows(ref)].any()                     # the zero rows of nets_pose
    for k in ('smpl_pose', 'smpl_beta', 'trans_cam', 'orient_cam', 'base_orient', 'base_trans', 'kp_2d', 'kp_score', 'visible', 'visible_orig', 'nets_pose', 'nets_vis'):
        assert not got[k][~rows].any(), k                                   # rows at or beyond seq_len and empty slots: exactly zero
    empty = np.flatnonzero(~rows.any(1))
    assert (got['fr_start'][empty] == 0).all() and (got['fr_end'][empty] == 1).all()
    _judge(name, 'prep', ic.prep_errors(got, ref, geo))


def _nets_rows(ref):
    m = np.zeros(ref['nets_vis'].shape, bool)
    for s, (a, b) in enumerate(zip(ref['fr_start'], ref['fr_end'])):
        m[s, :int(b) - int(a)] = ref['visible_orig'][s].sum() > 0
    return m


@pytest.fixture(scope='module')
def scene_runs(ctx):
    """The 'scene' batch through glamr_init_scenes_ex without flags, with each flag, and through glamr_init_scatter_pose alone."""
    case, refs = ctx['scene']
    geo, inp, pri = case['geo'], refs['scene_inputs'], case['priors']
    return dict(plain=ic.launch_scenes(geo, inp, pri), from_cam=ic.launch_scenes(geo, inp, pri, flags=1), scattered=ic.launch_scenes(geo, inp, pri, flags=2),
                scatter=ic.launch_scatter_pose(geo, inp, pri))


def _scene_checks(name, case, refs, got, flagged=None):
    geo, ref = case['geo'], refs['scene']
    g = dict(got)
    if flagged is not None:
        g.update(flag_base_trans=flagged['base_trans'], flag_base_orient=flagged['base_orient'])
    errs = ic.scene_errors(g, ref, geo, refs['scene_flag'] if flagged is not None else None)
    _judge(name, 'scene', errs)
    assert errs['traj 0-8'][0] == 0.0 and errs['base_trans'][0] == 0.0                  # copies of the prior rows, zeros past n
    assert np.array_equal(got['smpl_pose'].astype(np.float64), ref['smpl_pose'])
    absent = ~ic.row_mask(geo).any(1)
    for k in ('traj_local_pred', 'person2cam', 'base_orient', 'base_trans', 'smpl_pose'):
        assert not got[k][absent].any(), k                                              # slots without a person are not written


def test_scenes_against_fp64(ctx, scene_runs):
    case, refs = ctx['scene']
    _scene_checks('scene', case, refs, scene_runs['plain'], scene_runs['from_cam'])


def test_scenes_zero_camera_is_the_ports(ctx, scene_runs):
    """Scene 2: filter_pose drops person 0's frame 0, in which person 1 is seen -- the initial camera is a zero matrix, re-orthonormalised and inverted.  No
    float64 statement exists for that; the float32 port's values are compared one by one: the camera exactly, signs of the zeros included, the heading
    columns (cos / sin of constants) within two float32 ulps of 1 (two libms)."""
    case, refs = ctx['scene']
    geo, got = case['geo'], scene_runs['plain']
    assert refs['scene']['zero_cam'][2]
    port = ic.run_port(case)['scene']
    n = int(geo['seq_len'][2])
    a, b = got['cam_pose'][2, :n], port['cam_pose'][2, :n]
    assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and not a.any()
    for s in (6, 7, 8):
        m = int(refs['scene']['fr_end'][s] - refs['scene']['fr_start'][s])
        e = np.abs(got['traj_local_pred'][s, :m, 9:].astype(np.float64) - port['traj_local_pred'][s, :m, 9:]).max()
        print('zero camera, slot %d: heading columns %.2e from the port (bound %.2e)' % (s, e, 2 * ic.ULP))
        assert e <= 2 * ic.ULP


def test_scenes_flags(ctx, scene_runs):
    case, refs = ctx['scene']
    ref, inp = refs['scene'], refs['scene_inputs']
    plain, from_cam, scattered = scene_runs['plain'], scene_runs['from_cam'], scene_runs['scattered']
    inside = np.zeros(inp['visible'].shape, bool)
    for s, (a, b) in enumerate(zip(ref['fr_start'], ref['fr_end'])):
        inside[s, int(a):int(b)] = True
    # GLAMR_INIT_TRAJ_FROM_CAM decides the base pose outside the existence range only (against float64 there: test_scenes_against_fp64)
    for k in ('base_orient', 'base_trans'):
        assert np.array_equal(from_cam[k][inside].view(np.int32), plain[k][inside].view(np.int32)), k
        assert not np.array_equal(from_cam[k][~inside], plain[k][~inside]), k
    for k in ('traj_local_pred', 'person2cam', 'rel_transform_cam', 'cam_pose', 'smpl_pose'):
        assert np.array_equal(from_cam[k].view(np.int32), plain[k].view(np.int32)), k
    # GLAMR_INIT_POSE_SCATTERED: smpl_pose is left as it was, everything else as without the flag
    assert np.array_equal(scattered['smpl_pose'].view(np.int32), inp['smpl_pose'].view(np.int32))
    for k in ('traj_local_pred', 'person2cam', 'rel_transform_cam', 'cam_pose', 'base_orient', 'base_trans'):
        assert np.array_equal(scattered[k].view(np.int32), plain[k].view(np.int32)), k
    # glamr_init_scatter_pose alone writes what the unflagged scene kernel writes there
    assert np.array_equal(scene_runs['scatter'].view(np.int32), plain['smpl_pose'].view(np.int32))
    assert not np.array_equal(plain['smpl_pose'], inp['smpl_pose'])


def test_scenes_single_visible_frame(ctx):
    """filter_pose leaves person 1 of the case one visible frame (frame 10 of detections 10 and 11): its heading and local orientation are held constant."""
    case, refs = ctx['single']
    geo, inp, pri = case['geo'], refs['scene_inputs'], case['priors']
    assert inp['visible'][1].sum() == 1
    _scene_checks('single', case, refs, ic.launch_scenes(geo, inp, pri), ic.launch_scenes(geo, inp, pri, flags=1))


def test_cam_all_frames(ctx):
    case, refs = ctx['scene']
    geo, vis = case['geo'], refs['scene_inputs']['visible']
    ow, tw = refs['world']
    sentinel = np.float32(-7.25)
    got = ic.launch_cam_all_frames(geo, vis, refs['person2cam32'], ow, tw, np.full((geo['S'], geo['T'], 12), sentinel, np.float32))
    srows, seen = ic.row_mask(geo, False), refs['cam_all_seen']
    assert (got[~srows] == sentinel).all() and (~srows).any()                            # rows at or beyond seq_len are untouched
    e = float(np.abs(got.astype(np.float64) - refs['cam_all'])[seen].max())
    tol = ic.tolerance('scene', 'cam_all', None, refs['cam_all'][seen])
    print('scene    cam_pose, all frames, first person seen: worst %.2e   tolerance %.2e' % (e, tol))
    assert e <= tol
    # frames nobody is seen in (+0 of zeros_like) and frames only others are seen in (signed zeros of the product with vis_frames): the port's values
    port = ic.port_cam_all_frames(geo, vis, refs['person2cam32'], ow, tw)
    rest = srows & ~seen
    others = rest & np.stack([(vis[si * geo['P']:(si + 1) * geo['P']] == 1).any(0) for si in range(geo['S'])])
    assert others.any() and (rest & ~others).any()
    assert np.array_equal(got[rest], port[rest]) and np.array_equal(np.signbit(got[rest]), np.signbit(port[rest]))


def _inject(raw, arr, slot, t, idx, value):
    r = {k: v.copy() for k, v in raw.items()}
    r[arr][slot, t].reshape(-1)[idx] = value
    return r


def test_check_inputs_lane_map():
    """One bad value at a time at every boundary of the lane map, NaN and +Inf, in the first row of the batch and in its very last one (row 13: the
    second wave of the last block, whose other two waves are past the end): exactly the slot's bit of the non-finite row; a non-finite MATRIX entry is
    not orthonormal to 1e-2 either and sets the slot's bit of the rotation row as well, as the reference of this test states."""
    raw = ic.check_inputs_raw()
    assert not ic.launch_check_inputs(raw).any()
    for arr, idx in ic.CHECK_INJECTIONS:
        for bad in (np.nan, np.inf):
            for slot, t in ((0, 0), (1, 6)):
                r = _inject(raw, arr, slot, t, idx, bad)
                want = ic.ref_check_inputs(r, r['K'])
                assert want[1].tolist() == [int(slot == 0), int(slot == 1)] and want[0].sum() == int(arr == 'rot')
                got = ic.launch_check_inputs(r)
                assert np.array_equal(got, want), (arr, idx, bad, slot, got.tolist())


def test_check_inputs_threshold_and_undetected_rows():
    raw = ic.check_inputs_raw()
    for M, bad in ic.threshold_matrices():
        r = {k: v.copy() for k, v in raw.items()}
        r['rot'][1, 2, 5] = M.reshape(9)
        got = ic.launch_check_inputs(r)
        print('Gram entry %s 1e-2: verdict %s' % ('over' if bad else 'under', got.tolist()))
        assert got.tolist() == [[0, int(bad)], [0, 0]]
    assert raw['exist'][0, 3] == 0
    r = {k: v.copy() for k, v in raw.items()}
    for arr in ('rot', 'betas', 'trans', 'kp', 'K'):                                     # the same garbage on an undetected row changes nothing
        r[arr][0, 3] = np.nan
    r['rot'][0, 3, :9] = 3.0
    assert not ic.launch_check_inputs(r).any()
