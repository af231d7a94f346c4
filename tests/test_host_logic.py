"""CPU tests of the product's host-side logic (no GPU): numpy transform helpers vs the oracle, and the per-person preprocessing
(frame / visibility bookkeeping must be bit-exact) vs fixtures produced by the unmodified reference."""
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from oracle.port import transforms as tf
from glamr_amd.lib.utils import np_transform as nt
from glamr_amd.utils import synth


def _close(a, b, tol=2e-6):
    assert np.abs(np.asarray(a, np.float64) - np.asarray(b.detach().numpy() if hasattr(b, 'detach') else b, np.float64)).max() < tol


def test_numpy_transforms_match_oracle():
    x = mg.seeded_inputs('geom')
    aa, aa2, d6, trans = x['aa'], x['aa2'], x['d6'], x['trans']
    ta, ta2, td6, tt = map(torch.tensor, (aa, aa2, d6, trans))
    R = nt.aa_to_rotmat(aa)
    _close(R, tf.aa_to_rotmat(ta))
    _close(nt.rotmat_to_quat(R), tf.rotmat_to_quat(tf.aa_to_rotmat(ta)))
    q1, q2 = nt.aa_to_quat(aa), nt.aa_to_quat(aa2)
    _close(q1, tf.aa_to_quat(ta))
    _close(nt.quat_to_aa(q1), tf.quat_to_aa(tf.aa_to_quat(ta)))
    _close(nt.quat_mul(q1, q2), tf.quat_mul(tf.aa_to_quat(ta), tf.aa_to_quat(ta2)))
    _close(nt.quat_angle_between(q1, q2), tf.quat_angle_between(tf.aa_to_quat(ta), tf.aa_to_quat(ta2)), 2e-4)
    _close(nt.quat_to_rotmat(q1), tf.quat_to_rotmat(tf.aa_to_quat(ta)))
    _close(nt.sixd_to_rotmat(d6), tf.sixd_to_rotmat(td6))
    M = nt.make_transform(aa, trans)
    _close(M, tf.make_transform(ta, tt, 'axis_angle'))
    _close(nt.invert_transform(M), tf.invert_transform(tf.make_transform(ta, tt, 'axis_angle')))
    tg, qg = tf.local_to_global_traj(torch.tensor(x['local']))
    _close(nt.global_to_local_traj(tg.numpy(), qg.numpy()), tf.global_to_local_traj(tg, qg), 5e-6)
    vis = np.ones(64, bool)
    vis[20:31] = False
    vis[60:] = False
    _close(nt.interp_orient_sep_heading(qg.numpy()[vis], vis), tf.interp_orient_sep_heading(qg[torch.tensor(vis)], torch.tensor(vis)), 5e-6)


@pytest.mark.parametrize('cfg_id,T,P,K', mg.GRECON_CASES[:3])
def test_person_preprocessing_is_bit_exact(golden, cfg_id, T, P, K):
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    g = golden('grecon_%s_T%d_P%d' % (cfg_id, T, P))
    in_dict = synth.make_in_dict(seed=3, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model())
    opt = GlobalReconOptimizer.__new__(GlobalReconOptimizer)       # host logic only: no device, no library
    opt.flag_filter_pose, opt.flag_make_invis_with_keypoint = True, False
    for pi in range(P):
        d = opt._person_arrays(in_dict['est'][pi])
        for key in ('visible', 'visible_orig', 'exist_frames', 'vis_frames', 'invis_frames', 'kp_2d_score', 'kp_2d_aligned', 'cam_K'):
            assert np.array_equal(np.asarray(d[key]), g['init_p%d_%s' % (pi, key)]), key
        assert int(d['fr_start']) == int(g['init_p%d_fr_start' % pi]) and int(d['fr_end']) == int(g['init_p%d_fr_end' % pi])
        assert int(d['exist_len']) == int(g['init_p%d_exist_len' % pi])
        for key in ('smpl_beta', 'smpl_orient_cam', 'root_trans_cam', 'smpl_pose_nofill'):
            assert np.abs(d[key] - g['init_p%d_%s' % (pi, key)]).max() < 1e-6, key


def test_filter_pose_drops_orientation_jumps():
    """filter_pose look-ahead rule (global_recon_model.py:256-262): of two frames around a > 60 degree jump the EARLIER one is
    dropped unless the next frame is itself a jump or invisible."""
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    T = 12
    orient = np.tile(np.array([[0.1, 0.0, 0.0]], np.float32), (T, 1))
    orient[5] = [0.1, 2.0, 0.0]            # isolated flip: jumps at 5 and at 6
    d = {'visible': np.ones(T), 'smpl_orient_cam': orient}
    GlobalReconOptimizer._filter_pose(d)
    ref = {'visible': torch.ones(T, dtype=torch.float64), 'smpl_orient_cam': torch.tensor(orient)}
    from oracle.port.grecon import GlobalReconOptimizer as Ora
    Ora.filter_pose(Ora.__new__(Ora), ref)
    assert np.array_equal(d['visible'], ref['visible'].numpy())
    assert d['visible'].sum() < T


def test_lazy_dict_is_a_dict_to_its_consumers():
    """LazyDict (the per-person / per-sequence output dictionaries): values made on first access, every dict protocol sees all keys."""
    import pickle
    from glamr_amd.global_recon.models.global_recon_model import LazyDict
    calls = []
    d = LazyDict({'a': 1}, {'b': lambda: calls.append('b') or 2, 'c': lambda: calls.append('c') or 3})
    assert 'b' in d and len(d) == 3 and calls == []
    assert d['b'] == 2 and d['b'] == 2 and calls == ['b']                  # computed once
    assert d.get('c') == 3 and d.get('zzz', 7) == 7
    assert sorted(d.keys()) == ['a', 'b', 'c'] and dict(d) == {'a': 1, 'b': 2, 'c': 3} and d == {'a': 1, 'b': 2, 'c': 3}
    e = LazyDict({}, {'x': lambda: 5})
    e['x'] = 6                                                             # assignment wins over the pending value
    assert e['x'] == 6 and len(e) == 1
    f = LazyDict({'k': 0}, {'y': lambda: [1, 2]})
    back = pickle.loads(pickle.dumps(f))
    assert type(back) is dict and back == {'k': 0, 'y': [1, 2]}
    g = LazyDict({'k': 0}, {'y': lambda: 1})
    assert g.pop('y') == 1 and 'y' not in g
    try:
        g['nope']
        assert False
    except KeyError:
        pass


def test_lazy_dict_with_a_shared_factory():
    from glamr_amd.global_recon.models.global_recon_model import LazyDict
    made = []
    d = LazyDict({'n': 3}, factory=lambda k: made.append(k) or k.upper(), factory_keys=('a', 'b'))
    assert len(d) == 3 and 'a' in d and 'zz' not in d and made == []
    assert d['a'] == 'A' and d['a'] == 'A' and made == ['a']
    assert d.pop('b') == 'B' and 'b' not in d and len(d) == 2             # a popped key does not come back
    assert dict(d) == {'n': 3, 'a': 'A'}


def test_host_scatter_matches_numpy_indexing():
    """glamr_host_scatter (the library's multi-threaded scatter of per-detection rows to frame rows, host memory only) against plain
    numpy fancy indexing: one run, two gaps, detections starting late, float32 `exist`, non-contiguous sources, an empty person slot."""
    import ctypes
    from glamr_amd import _lib
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer as G
    rng = np.random.RandomState(0)
    T = 40

    def person(exist, dtype=np.float64, strided=False, n_kp=29):
        nv = int((exist != 0).sum())
        mk = lambda *shape: rng.rand(*shape).astype(np.float32)
        rot = mk(nv, 54, 4)
        if strided:
            rot = np.asfortranarray(rot)
        return {'bboxes_dict': {'exist': exist.astype(dtype)}, 'smpl_pose_quat_wroot': rot, 'smpl_beta': mk(nv, 10), 'root_trans': mk(nv, 3),
                'cam_K': mk(nv, 3, 3), 'kp_2d': mk(nv, n_kp, 2)}
    e0 = np.ones(T)
    e1 = np.ones(T); e1[5:9] = 0; e1[20:31] = 0
    e2 = np.zeros(33); e2[7:30] = 1
    e3 = np.ones(T); e3[0] = 0; e3[-1] = 0
    # (the wire format takes any kp_2d with >= 24 keypoints, glamr_amd/utils/wire.py: 24 and 31 here beside HybrIK's 29)
    in_dicts = [{'est': {0: person(e0), 1: person(e1, n_kp=24)}}, {'est': {4: person(e2, np.float32, strided=True)}}, {'est': {0: person(e3, n_kp=31), 7: person(e0)}}]
    ids = [list(d['est'].keys()) for d in in_dicts]
    P, n = 2, 6
    h = {'exist': np.full((n, T), -7, np.float32), 'rot': np.full((n, T, 216), -7, np.float32), 'betas': np.full((n, T, 10), -7, np.float32),
         'trans': np.full((n, T, 3), -7, np.float32), 'K': np.full((n, T, 9), -7, np.float32), 'kp': np.full((n, T, 48), -7, np.float32)}
    g = G.__new__(G)
    seq_len, lens, exists = g._scatter_inputs(in_dicts, ids, P, h)
    want = {k: np.full_like(v, -7) for k, v in h.items()}
    for si, d in enumerate(in_dicts):
        for pi, idx in enumerate(ids[si]):
            src, k = d['est'][idx], si * P + pi
            ex = src['bboxes_dict']['exist']
            vi = np.flatnonzero(ex)
            assert seq_len[k] == len(ex) and lens[k] == vi[-1] + 1 - vi[0] and exists[(si, idx)] is ex
            want['exist'][k, :len(ex)] = ex
            for dst, key, w in (('rot', 'smpl_pose_quat_wroot', 216), ('betas', 'smpl_beta', 10), ('trans', 'root_trans', 3), ('K', 'cam_K', 9)):
                want[dst][k, vi] = np.asarray(src[key]).reshape(len(vi), w)
            want['kp'][k, vi] = src['kp_2d'][:, :24].reshape(len(vi), 48)
    assert seq_len[3] == 0                       # the empty slot of the one-person scene
    for k in h:
        assert np.array_equal(h[k], want[k]), k
    # a person whose exist array disagrees with its rows is an error, not a silent mis-scatter
    bad = person(e0)
    bad['bboxes_dict']['exist'] = e1
    with pytest.raises(RuntimeError):
        g._scatter_inputs([{'est': {0: bad}}], [[0]], 1, h)


def test_carved_batch_arrays_are_independent_zero_views():
    """PackedScenes.empty carves its arrays from one zero allocation: right shapes / dtypes, 256-byte steps, no overlap (writing one array
    leaves every other array zero), and the C struct the library receives points at them."""
    from glamr_amd.global_recon import packing
    p = packing.PackedScenes.empty(3, 2, 40, torch.device('cpu'))
    t = {k: v for k, v in p.t.items() if v is not None}
    assert t['fr_start'].dtype == torch.int32 and t['kp_2d'].shape == (6, 40, 26, 2) and t['rel_transform_cam'].shape == (3, 2, 2, 40, 12)
    base = min(v.data_ptr() for v in t.values())
    for name, v in t.items():      # (256-byte steps from the allocation's start; device allocations themselves are 256-byte aligned)
        assert v.is_contiguous() and (v.data_ptr() - base) % 256 == 0 and float(v.abs().sum()) == 0.0, name
    for name, v in t.items():
        v.fill_(1)
        for other, w in t.items():
            if other != name:
                assert float(w.abs().sum()) == 0.0, (name, other)
        v.zero_()
    sb = p.struct()
    assert sb.params == t['params'].data_ptr() and sb.cam_pose == t['cam_pose'].data_ptr()


@pytest.mark.parametrize('case', mg.FILTER_CASES, ids=[c[0] for c in mg.FILTER_CASES])
def test_filter_pose_twin_on_injected_jumps(golden, case):
    """The numpy twin of filter_pose (what init_data_batch_host runs) on sequences with injected root-orientation jumps -- isolated, adjacent
    and persistent ones, at the first / last frame, next to a detection gap, within 1e-4 of the pi / 3 threshold -- against the visibility
    bookkeeping the UNMODIFIED reference's init_data leaves (oracle/make_golden.py gen_filter).  The device twin: tests/test_filter_pose_gpu.py."""
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    g = golden('filter_pose')
    name, T, gap, events, attrs = case
    in_dict, seed = mg.filter_inputs(case)
    opt = GlobalReconOptimizer.__new__(GlobalReconOptimizer)
    opt.flag_filter_pose = True
    opt.flag_make_invis_with_keypoint = bool(attrs.get('flag_make_invis_with_keypoint', False))
    opt.make_invis_keypoint_min_score, opt.make_invis_keypoint_min_num = 0.6, attrs.get('make_invis_keypoint_min_num', 15)
    d = opt._person_arrays(in_dict['est'][0])
    for key in ('visible', 'visible_orig', 'exist_frames', 'vis_frames', 'invis_frames'):
        assert np.array_equal(np.asarray(d[key]), g['%s_%s' % (name, key)]), key
    assert int(d['fr_start']) == int(g[name + '_fr_start']) and int(d['fr_end']) == int(g[name + '_fr_end'])
    assert (d['visible'] != d['visible_orig']).sum() == (g[name + '_visible'] != g[name + '_visible_orig']).sum()


def test_keypoint_count_filter_with_the_reference_default_removes_every_frame(golden):
    """flag_make_invis_with_keypoint (:264-268) with the reference's default minimum of 15 confident keypoints: HybrIK scores 14 joints
    per detected frame, so every frame becomes invisible -- as the reference's own filter_pose does on the same arrays."""
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    g = golden('filter_pose')
    in_dict, seed = mg.filter_inputs(mg.FILTER_CASES[0])
    opt = GlobalReconOptimizer.__new__(GlobalReconOptimizer)
    opt.flag_filter_pose, opt.flag_make_invis_with_keypoint = True, True
    opt.make_invis_keypoint_min_score, opt.make_invis_keypoint_min_num = 0.6, 15
    d = opt._person_arrays(in_dict['est'][0])
    assert np.array_equal(d['visible'], g['kp_default_visible']) and np.array_equal(d['vis_frames'], g['kp_default_vis_frames']) and not d['vis_frames'].any()


@pytest.mark.parametrize('lens,fr_start,occupied', [
    ([17, 9, 30, 1], [0, 5, 3, 29], [True, True, True, True]),          # two scenes x two person slots, ragged starts and lengths
    ([17, 0, 30, 12], [0, 0, 3, 20], [True, False, True, True]),        # one empty slot in the middle
    ([0, 0, 0, 0], [0, 0, 0, 0], [False, False, False, False]),         # a batch whose slots are all empty
])
def test_frame_row_index_equals_the_per_slot_loop(lens, fr_start, occupied):
    from glamr_amd.global_recon.latent_schedule import frame_row_index
    T = 32
    src, dst = frame_row_index(np.asarray(lens, np.int32), np.asarray(fr_start, np.int32), np.asarray(occupied), T)
    want_src, want_dst = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for k in range(len(lens)):
        if occupied[k]:
            want_src.append(k * T + np.arange(lens[k]))
            want_dst.append(k * T + fr_start[k] + np.arange(lens[k]))
    assert src.dtype == dst.dtype == np.int64
    assert np.array_equal(src, np.concatenate(want_src)) and np.array_equal(dst, np.concatenate(want_dst))
    assert len(src) == sum(n for n, o in zip(lens, occupied) if o) and (len(dst) == 0 or dst.max() < len(lens) * T)


def test_stage_iters_and_end_stage():
    """What every schedule does around a stage: the max_iters cap; has_wd turns true with the first stage that optimises world_dheading and
    stays; reinitialize_cam gives every frame the camera of frame 0."""
    import types
    from glamr_amd.global_recon import stepwise
    spec = {'opt_niters': 10, 'opt_variables': ['cam', 'local_xy']}
    assert [stepwise.stage_iters(spec, k) for k in (None, 4, 10, 25)] == [10, 4, 10, 10]
    cam = torch.arange(2 * 3 * 16, dtype=torch.float32).view(2, 3, 4, 4)
    packed = types.SimpleNamespace(t={'cam_pose': cam.clone()})
    stages = [spec, dict(spec, opt_variables=['world_dheading', 'cam']), dict(spec, reinitialize_cam=True)]
    has_wd, seen = False, []
    for s in stages:
        kept = packed.t['cam_pose'].clone()
        has_wd = stepwise.end_stage(packed, s, has_wd)
        seen.append(has_wd)
        want = cam[:, :1].expand_as(cam) if s.get('reinitialize_cam', False) else kept
        assert torch.equal(packed.t['cam_pose'], want)
    assert seen == [False, True, True]
    assert stepwise.end_stage(packed, spec, True) is True


# ------------------------------------------------------------------------------------------------------------------------------------
# the params row: packing's description of it (PERSON_VARS / SCENE_VARS, person_view / scene_view) against explicit offsets
# ------------------------------------------------------------------------------------------------------------------------------------
_PERSON_NAMES = ('traj_local_xy', 'traj_local_heading', 'traj_local_dxy', 'traj_local_dheading', 'traj_local_z', 'traj_local_rot', 'world_dheading')


def _packable_scenes():
    """Two scenes of 7 and 5 frames.  Scene 0: persons 0 on [0, 7) and 3 on [2, 6), nobody seen in frame 1 (a row of cam_inv_rot_residual);
    scene 1: one person, so its second slot is padding.  Every packed variable holds distinct non-zero numbers."""
    counter = [0]

    def fill(*shape):
        n = int(np.prod(shape))
        counter[0] += n
        return (np.arange(counter[0] - n, counter[0], dtype=np.float32) + 1.0).reshape(shape)

    def person(Ts, fs, fe, vis):
        n = fe - fs
        eye = np.tile(np.eye(4, dtype=np.float32), (Ts, 1, 1))
        return {'fr_start': fs, 'fr_end': fe, 'vis_frames': vis, 'kp_2d_aligned': np.zeros((Ts, 26, 2)), 'kp_2d_score': np.zeros((Ts, 26)),
                'cam_K': eye[:, :3, :3].copy(), 'traj_local_pred': np.zeros((n, 11), np.float32), 'smpl_orient_cam': np.zeros((Ts, 3), np.float32),
                'smpl_orient_world_base': np.zeros((Ts, 3), np.float32), 'root_trans_world_base': np.zeros((Ts, 3), np.float32), 'person2cam': eye,
                'traj_local_xy': fill(2), 'traj_local_heading': fill(1), 'traj_local_dxy': fill(n - 1, 2), 'traj_local_dheading': fill(n - 1),
                'traj_local_z': fill(n), 'traj_local_rot': fill(n, 6), 'world_dheading': fill(Ts, 1)}

    def scene(name, Ts, persons):
        fr_num = sum(pd['vis_frames'].astype(np.int64) for pd in persons.values())
        return {'seq_name': name, 'seq_len': Ts, 'person_data': persons, 'fr_num_persons': fr_num, 'cam_pose': np.tile(np.eye(4, dtype=np.float32), (Ts, 1, 1)),
                'cam_inv_rot_residual': fill(int((fr_num == 0).sum()), 6), 'cam_inv_trans_residual': fill(Ts, 3)}
    v0 = np.ones(7, bool)
    v0[1] = False
    v3 = np.zeros(7, bool)
    v3[2:6] = True
    v3[1] = False
    datas = [scene('a', 7, {0: person(7, 0, 7, v0), 3: person(7, 2, 6, v3)}), scene('b', 5, {0: person(5, 0, 5, np.ones(5, bool))})]
    j_locals = [{idx: torch.zeros((d['seq_len'], 26, 3)) for idx in d['person_data']} for d in datas]
    return datas, j_locals


def _expected_params(datas, l, P, T):
    """The params array PackedScenes builds from `datas`, by explicit offsets into param_layout_py's dictionary."""
    want = np.zeros((len(datas), l['scene_stride']), np.float32)
    for si, d in enumerate(datas):
        Ts, row = d['seq_len'], want[si]
        for f, r in zip(np.where(d['fr_num_persons'] == 0)[0], d['cam_inv_rot_residual']):
            row[l['cam_inv_rot_res'] + 6 * f:l['cam_inv_rot_res'] + 6 * f + 6] = r
        row[l['cam_inv_trans_res']:l['cam_inv_trans_res'] + 3 * Ts] = d['cam_inv_trans_residual'].reshape(-1)
        for pi, pd in enumerate(d['person_data'].values()):
            b, n = l['person0'] + pi * l['person_stride'], pd['fr_end'] - pd['fr_start']
            row[b + l['local_xy']:b + l['local_xy'] + 2] = pd['traj_local_xy']
            row[b + l['local_heading']] = pd['traj_local_heading'][0]
            row[b + l['local_dxy'] + 2:b + l['local_dxy'] + 2 * n] = pd['traj_local_dxy'].reshape(-1)
            row[b + l['local_dheading'] + 1:b + l['local_dheading'] + n] = pd['traj_local_dheading']
            row[b + l['local_z']:b + l['local_z'] + n] = pd['traj_local_z']
            row[b + l['local_rot']:b + l['local_rot'] + 6 * n] = pd['traj_local_rot'].reshape(-1)
            row[b + l['world_dheading']:b + l['world_dheading'] + Ts] = pd['world_dheading'][:, 0]
    return want


@pytest.mark.parametrize('fixed_cam', [False, True])
def test_pack_unpack_round_trip_and_the_row_by_explicit_offsets(fixed_cam):
    from glamr_amd.global_recon import packing
    datas, j_locals = _packable_scenes()
    assert (datas[0]['fr_num_persons'] == 0).sum() == 1 and datas[0]['cam_inv_rot_residual'].shape == (1, 6)
    packed = packing.PackedScenes(datas, j_locals, 'cpu')
    S, P, T, l = packed.S, packed.P, packed.T, packed.layout
    assert (S, P, T) == (2, 2, 7) and l == packing.param_layout_py(2, 7)
    want = _expected_params(datas, l, P, T)
    assert np.array_equal(packed.t['params'].numpy(), want)
    assert not want[1, l['person0'] + l['person_stride']:].any() and not want[1, :l['person0']][15 * T + 3 * 5:].any()      # the padding slot, the frames past Ts
    # the camera variables are the kernel's to write: distinct numbers in their columns, to be found again in the dictionaries
    cam = packed.t['params'].numpy()[:, :l['cam_inv_rot_res']]
    cam[...] = 1e4 + np.arange(cam.size, dtype=np.float32).reshape(cam.shape)
    copies = [dict(seq_len=d['seq_len'], fr_num_persons=d['fr_num_persons'],
                   person_data={i: dict(fr_start=pd['fr_start'], fr_end=pd['fr_end']) for i, pd in d['person_data'].items()}) for d in datas]
    packed.unpack_into(copies, {'opt_variables': list(packing.VAR_BITS)}, {'flag_fixed_cam': fixed_cam}, as_torch=False)
    for si, (d, c) in enumerate(zip(datas, copies)):
        Ts = d['seq_len']
        for name in ('cam_inv_rot_residual', 'cam_inv_trans_residual'):
            assert c[name].dtype == np.float32 and np.array_equal(c[name], d[name]), name
        r6, tr = cam[si, :6 * T].reshape(T, 6), cam[si, 6 * T:9 * T].reshape(T, 3)
        if fixed_cam:
            assert np.array_equal(c['cam_rot_6d_fix'], r6[:1]) and np.array_equal(c['cam_trans_fix'], tr[:1]) and 'cam_rot_6d' not in c
        else:
            assert np.array_equal(c['cam_rot_6d'], r6[:Ts]) and np.array_equal(c['cam_trans'], tr[:Ts]) and 'cam_rot_6d_fix' not in c
        for idx, pd in d['person_data'].items():
            for name in _PERSON_NAMES:
                got = c['person_data'][idx][name]
                assert got.shape == pd[name].shape and np.array_equal(got, pd[name]), (si, idx, name)


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_params_views_cut_the_last_axis_of_a_whole_batch(kind):
    """person_view / scene_view on the (S, scene_stride) array: views with the leading S; writing the (S, T, 6) traj_local_rot view of person 1
    changes exactly person_params(si, 1)[local_rot : local_rot + 6 T] and nothing else."""
    from glamr_amd.global_recon import packing
    S, P, T = 3, 2, 5
    packed = packing.PackedScenes.empty(S, P, T, torch.device('cpu'))
    l, params = packed.layout, packed.t['params']
    arr = params.numpy() if kind == 'numpy' else params
    rot = packing.person_view(arr, l, 1, 'traj_local_rot')
    assert tuple(rot.shape) == (S, T, 6)
    values = np.arange(1, S * T * 6 + 1, dtype=np.float32).reshape(S, T, 6)
    rot[...] = values if kind == 'numpy' else torch.from_numpy(values)
    want = np.zeros((S, l['scene_stride']), np.float32)
    for si in range(S):
        b = l['person0'] + l['person_stride'] + l['local_rot']
        want[si, b:b + 6 * T] = values[si].reshape(-1)
        assert np.array_equal(packed.person_params(si, 1)[l['local_rot']:l['local_rot'] + 6 * T].numpy(), values[si].reshape(-1))
    assert np.array_equal(params.numpy(), want)
    assert tuple(packing.person_view(arr, l, 0).shape) == (S, l['person_stride']) and tuple(packing.scene_view(arr, l).shape) == (S, l['person0'])
    assert tuple(packing.scene_view(arr, l, 'cam_trans').shape) == (S, T, 3) and tuple(packing.person_view(arr[0], l, 1, 'traj_local_xy').shape) == (2,)
    assert tuple(packing.person_view(arr, l, 0, 'world_dheading').shape) == (S, T, 1) and packing.person_cols(l, 1) == slice(l['person0'] + l['person_stride'], l['scene_stride'])


def test_off_kernel_terms_are_split_once():
    """packing.split_off_kernel: what GlobalReconOptimizer.__init__ takes off the stages' loss_cfg for the launch-by-launch schedule."""
    import copy
    from glamr_amd.global_recon import packing
    from glamr_amd.global_recon.configs import CONFIGS, get_config
    for cfg_id in CONFIGS:
        specs = get_config(cfg_id)['opt_stage_specs']
        rest, pen, aux = packing.split_off_kernel(specs)
        assert rest is specs and pen == {} and aux == {}, cfg_id
    specs = get_config('glamr_dynamic_multi')['opt_stage_specs']
    specs['init_opt']['loss_cfg']['cam_traj_trans'] = {'weight': 2, 'first_frame_weight': 5}
    specs['main_opt']['loss_cfg']['penetration'] = {'weight': 3}
    specs['main_opt']['loss_cfg']['cam_rot_smoothness'] = {'weight': 0.5, 'monitor_only': True}
    specs['main_opt']['loss_cfg']['local_traj_dheading_reg'] = {'weight': 7.0}
    before = copy.deepcopy(specs)
    rest, pen, aux = packing.split_off_kernel(specs)
    assert specs == before and rest is not specs
    assert pen == {'main_opt': {'weight': 3.0, 'monitor_only': False}}
    assert aux == {'init_opt': {'cam_traj_trans': {'weight': 2.0, 'monitor_only': False, 'first_frame_weight': 5.0}},
                   'main_opt': {'cam_rot_smoothness': {'weight': 0.5, 'monitor_only': True}, 'local_traj_dheading_reg': {'weight': 7.0, 'monitor_only': False}}}
    plain = get_config('glamr_dynamic_multi')['opt_stage_specs']
    assert rest == plain and list(rest) == list(plain) and all(list(rest[s]['loss_cfg']) == list(plain[s]['loss_cfg']) for s in plain)
    specs['main_opt']['loss_cfg']['cam_depth_smoothness'] = {'weight': 1.0, 'rot_type': 'quat'}
    with pytest.raises(NotImplementedError, match='cam_depth_smoothness'):
        packing.split_off_kernel(specs)


def test_the_name_a_refusal_gives_an_off_kernel_term():
    """GlobalReconOptimizer._off_kernel_term for the seven combinations of {extra_loss, penetration, terms of AUX_LOSS_IDS}: the caller's term
    before the penetration term before the others (what ExtraLossSchedule.run names), None without any."""
    from glamr_amd.global_recon.models.global_recon_model import GlobalReconOptimizer
    pen = {'main_opt': {'weight': 1.0, 'monitor_only': False}}
    aux = {'init_opt': {'cam_traj_trans': {'weight': 1.0, 'monitor_only': False}},
           'main_opt': {'local_traj_dheading_reg': {'weight': 1.0, 'monitor_only': False}, 'cam_rot_smoothness': {'weight': 1.0, 'monitor_only': True}}}
    aux_name = 'the loss_cfg terms cam_rot_smoothness, cam_traj_trans, local_traj_dheading_reg'
    want = {(True, False, False): 'extra_loss', (True, True, False): 'extra_loss', (True, False, True): 'extra_loss', (True, True, True): 'extra_loss',
            (False, True, False): 'the penetration term (loss_cfg)', (False, True, True): 'the penetration term (loss_cfg)', (False, False, True): aux_name}
    opt = GlobalReconOptimizer.__new__(GlobalReconOptimizer)
    for (has_fn, has_pen, has_aux), name in want.items():
        opt._extra_loss, opt._pen_cfg, opt._aux_cfg = (lambda ctx: None) if has_fn else None, pen if has_pen else {}, aux if has_aux else {}
        assert opt._off_kernel_term() == name, (has_fn, has_pen, has_aux)
    opt._extra_loss, opt._pen_cfg, opt._aux_cfg = None, {}, {'main_opt': {'cam_depth_smoothness': {'weight': 1.0, 'monitor_only': False}}}
    assert opt._off_kernel_term() == 'the loss_cfg term cam_depth_smoothness'
    opt._aux_cfg = {}
    assert opt._off_kernel_term() is None
