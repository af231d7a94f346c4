"""CPU: the basis of tests/test_init_gpu.py.  The float64 restatement of csrc/init.hip's entry points (tests/init_ref_common.py) agrees with the
float32 port of the reference's init_data at float32 rounding level on ordinary scenes, field by field; the table D_REF of the port's own distance to
float64 per test case and compared array -- the basis of every tolerance, 4 d_ref + 1 ulp -- is measured again and must be current; each listed
defect, applied to the restatement, moves a compared output of the case meant to catch it by at least 20 tolerances; and the share of frames a
case leaves out as ill-conditioned stays within its cap.  Prints every figure it asserts."""
import numpy as np
import pytest

from tests import init_ref_common as ic

CAPS = {'prep': 0.0, 'prep300': 0.0, 'single': 0.0, 'scene': 0.05, 'synth': 0.0}      # 'scene' is the case designed around a heading reversal


@pytest.fixture(scope='module')
def cases():
    out = {}
    for name in ic.CASES + ('synth',):
        case = ic.build_case(name)
        out[name] = (case, ic.references(case))
    return out


def test_cases_hold_what_they_are_designed_around(cases):
    case, refs = cases['prep']
    raw, prep = case['raw'], refs['prep']
    aa = np.concatenate([prep['orient_cam'], prep['smpl_pose']], -1).reshape(9, 40, 24, 3)
    for s in (0, 7):                                                                  # the slots detected in every frame: converted values as they are
        ang = np.linalg.norm(aa[s][prep['detected'][s]], axis=-1)
        for d in (1e-2, 1e-4, 1e-6, np.pi - 1e-3 - 1e-5, np.pi - 1e-3 + 1e-5, np.pi - 1e-8):
            assert (np.abs(ang - (np.pi - d)) < 0.02 * min(d, 1e-3)).any(), (s, d)
    sp = ic.special_rotations(np.random.default_rng(11))
    g = np.abs(sp.astype(np.float32).astype(np.float64) @ np.swapaxes(sp.astype(np.float32).astype(np.float64), 1, 2) - np.eye(3)).max((1, 2))
    assert (np.abs(g[len(sp) // 2:] - 9e-3) < 1e-5).all() and (g[:len(sp) // 2] < 1e-6).all()
    X = sp[:18]                                                                       # near pi: every non-trace branch, with both signs of the extracted w
    seen = set()
    for M in X:
        i = int(np.argmax([M[0, 0], M[1, 1], M[2, 2], np.trace(M)]))
        j, k = (i + 1) % 3, (i + 2) % 3
        seen.add((i, bool(M[k, j] - M[j, k] < 0)))
    assert seen == {(i, b) for i in range(3) for b in (False, True)}
    assert prep['fr_start'].tolist() == [0, 5, 0, 4, 0, 0, 3, 0, 0] and prep['fr_end'].tolist() == [40, 34, 1, 35, 40, 40, 30, 33, 1]
    assert np.array_equal(prep['visible'], prep['visible_orig'])                      # (nothing for filter_pose to drop in this case)
    assert np.isnan(raw['rot'][1, 0]).all()                                           # rows without a detection hold NaN
    case, refs = cases['single']
    assert refs['prep']['visible'][1].sum() == 1 and refs['prep']['visible'][1, 10] == 1 and refs['prep']['visible_orig'][1].sum() == 2
    case, refs = cases['scene']
    assert refs['scene']['zero_cam'].tolist() == [False, False, True]
    assert refs['prep']['visible_orig'][6, 0] == 1 and refs['prep']['visible'][6, 0] == 0 and refs['prep']['visible'][7, 0] == 1      # dropped by filter_pose
    assert refs['prep']['visible'][6].sum() == 44 and refs['prep']['fr_start'][6] == 0
    assert (refs['scene']['fr_start'][4], refs['scene']['fr_end'][4]) == (7, 39)
    hv = ic.heading_of(ic.quat_mul(ic.aa_to_quat(refs['scene']['base_orient'][0]), ic.quat_conj(ic.BASE)))
    assert abs(2 * np.pi - abs(hv[31] - hv[14]) - 3.3) < 0.3         # the heading turns by 3.3 rad (+ the walker's own swing), the long way round, across the gap


def test_restated_rotation_vector_is_scipys():
    """The written-out algorithm that carries the two rotation-vector mutations is scipy's, unmutated, on every designed matrix."""
    sp = ic.special_rotations(np.random.default_rng(11)).astype(np.float32)
    e = np.abs(ic.rotvec(sp, 'manual') - ic.rotvec(sp)).max()
    print('written-out from_matrix().as_rotvec() against scipy: %.1e' % e)
    assert e < 1e-9                 # (at 1e-6 from pi the quaternion's w is 5e-7: 1e-16 / 5e-7 of relative error on an angle of pi)


def test_restatement_is_the_ports_on_ordinary_scenes(cases):
    """Every field the kernels write, restatement in float64 against oracle.port's init_data in float32 with the same prior outputs: exact where the
    field is a copy or a mask, within 64 float32 ulps of max(1, largest value) elsewhere (a chain of ~10 float32 operations on values of up to 6 m and
    pi rad, input roundings amplified by extrapolation over up to 17 frames)."""
    case, refs = cases['synth']
    geo = case['geo']
    port = ic.run_port(case, refs['world'])
    assert not port['skipped']
    for k in ic.PREP_EXACT:
        assert np.array_equal(np.asarray(port['prep'][k], np.float64), np.asarray(refs['prep'][k], np.float64)), k
    errs = dict(('prep ' + k, v) for k, v in ic.prep_errors(port['prep'], refs['prep'], geo).items())
    got = dict(port['scene'], flag_base_trans=port['scene']['traj_cam_trans'], flag_base_orient=port['scene']['traj_cam_orient'])
    errs.update(('scene ' + k, v) for k, v in ic.scene_errors(got, refs['scene'], geo, refs['scene_flag']).items())
    errs['cam_pose, all frames'] = (float(np.abs(port['cam_pose_all'] - refs['cam_all'])[refs['cam_all_seen']].max()), refs['cam_all'][refs['cam_all_seen']])
    for k, (e, vals) in errs.items():
        bound = 64 * ic.ULP * max(1.0, float(np.abs(vals).max()) if np.size(vals) else 1.0)
        print('%-28s port against float64 %.2e   bound %.2e' % (k, e, bound))
        assert e <= bound, k
    assert errs['scene traj 0-8'][0] == 0.0


@pytest.mark.parametrize('name', ic.CASES)
def test_d_ref_table_is_current(cases, name):
    case, refs = cases[name]
    d = ic.measure_d_ref(case, refs)
    flat = lambda t: {(a, b): v for a, x in t.items() for b, v in (x.items() if isinstance(x, dict) else [(None, x)])}
    now, stored = flat(d), flat(ic.D_REF[name])
    assert set(now) == set(stored)
    for k in sorted(now, key=str):
        print('%-8s %-30s measured %.3e   stored %.2e' % (name, k, now[k], stored[k]))
        assert 0.5 * stored[k] <= now[k] <= 2.0 * stored[k], k


@pytest.mark.parametrize('name', ic.CASES + ('synth',))
def test_conditioning_caps(cases, name):
    case, refs = cases[name]
    share = ic.skipped_share(refs['scene'], case['geo'])
    print('%s: %.2f %% of the frames are ill-conditioned (cap %.0f %%)' % (name, 100 * share, 100 * CAPS[name]))
    assert share <= CAPS[name]
    if name == 'scene':
        assert refs['scene']['ill'][0, 15:31].any() and not refs['scene']['ill'][1:].any()       # the reversal is one, and nothing else is left out


# mutation -> (case, stage, compared arrays of which at least one has to move by 20 tolerances)
TARGETS = {'extrap_pair': ('prep', 'prep', ('orient_cam', 'smpl_pose', 'smpl_beta', 'trans_cam')), 'quat_branch': ('prep', 'prep', ('pose det', 'pose pi')),
           'no_wflip': ('prep', 'prep', ('pose det',)), 'inv34': ('scene', 'scene', ('person2cam',)), 'base_heading': ('scene', 'scene', ('traj 9-10',)),
           'dh_origin': ('scene', 'scene', ('traj 9-10',)), 'rel_ij': ('scene', 'scene', ('rel_transform_cam',)), 'kp_remap': ('prep', 'prep', ('kp_2d',)),
           'nets_shift': ('prep', 'prep', ('nets_pose',))}


@pytest.mark.parametrize('mut', ic.MUTATIONS)
def test_every_listed_defect_moves_an_output_by_20_tolerances(cases, mut):
    name, stage, keys = TARGETS[mut]
    case, refs = cases[name]
    if stage == 'prep':
        got = ic.ref_prepare(case['raw'], case['filter'], mut=mut)
        errs = ic.prep_errors(got, refs['prep'], case['geo'])
    else:
        got = ic.ref_scenes(case['geo'], refs['scene_inputs'], case['priors'], mut=mut)
        errs = ic.scene_errors(got, refs['scene'], case['geo'])
    if mut == 'kp_remap':            # compared exactly: any change fails the comparison
        moved = np.abs(got['kp_2d'] - refs['prep']['kp_2d']).max()
        print('(%s) kp_2d moves by %.0f px; compared exactly' % (mut, moved))
        assert moved > 1.0
        return
    best = 0.0
    for k in keys:
        tol = ic.tolerance(name, stage, k, errs[k][1])
        print('(%s) %s, %s: moved %.2e = %.0f tolerances of %.2e' % (mut, name, k, errs[k][0], errs[k][0] / tol, tol))
        best = max(best, errs[k][0] / tol)
    assert best >= 20, (mut, best)


def test_check_inputs_reference_sees_every_injection():
    """The expectations of the GPU test, on the reference alone: every single injection sets exactly its slot's bit of exactly its row."""
    raw = ic.check_inputs_raw()
    assert not ic.ref_check_inputs(raw, raw['K']).any()
    for (arr, idx), bad in [(x, b) for x in ic.CHECK_INJECTIONS for b in (np.nan, np.inf)]:
        for slot, t in ((0, 0), (1, 6)):
            r = {k: v.copy() for k, v in raw.items()}
            r[arr][slot, t].reshape(-1)[idx] = bad
            v = ic.ref_check_inputs(r, r['K'])
            want = np.zeros((2, 2), np.int32)
            want[1, slot] = 1
            if arr == 'rot':
                want[0, slot] = 1        # a non-finite matrix entry is not within 1e-2 of orthonormal either
            assert np.array_equal(v, want), (arr, idx, bad, slot)
    for M, bad in ic.threshold_matrices():
        r = {k: v.copy() for k, v in raw.items()}
        r['rot'][1, 2, 5] = M.reshape(9)
        assert ic.ref_check_inputs(r, r['K'])[0].tolist() == [0, int(bad)]
