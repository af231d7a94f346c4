"""The end-to-end cases of the world-frame residuals (`world_dxy` / `world_res` in opt_variables, traj_rot_res / traj_trans_res in
loss_cfg), shared by the fixture generator (tools/world_res_golden.py: the UNMODIFIED reference on a copy of a shipped schedule) and the tests
(tests/test_world_res_ref.py on the host runtime, tests/test_world_res_gpu.py on the device), and the driver that runs a case stage by stage
through glamr_grecon_run_stage_ext or its host twin.

Every case has a TWIN: the same scene, schedule and K without the four names -- what the unchanged path computes.  The shapes are those of
oracle.make_golden.GRECON_CASES (seed 3), so tests/grecon_common.KSTEP_TOL applies."""
import copy
import ctypes

import numpy as np
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing, stepwise
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth

SEED = 3
TERMS = {'traj_rot_res': dict(weight=1.0e2), 'traj_trans_res': dict(weight=1.0e2)}


def _no_cam(s):
    # Cases a and d leave the camera out of the stage's variables.  On these scenes cam_rot_6d carries 98 % or more of a stage's first gradient
    # (2.6e5 beside 1.6e4 for all of a person's variables; 2.2e11 with synth's detection gap, from joints that project from next to the camera
    # plane), at five seeds alike, and world_dxy or the translation residual then stays below the 1 % of the stage's gradient that the
    # generator requires of every new variable (0.4 - 0.9 %).  Without it: 12 % (a), 45 % and 15 % (d).
    s['opt_variables'].remove('cam')


def _edit_a(specs, twin):
    _no_cam(specs['init_opt'])
    if not twin:
        specs['init_opt']['opt_variables'].append('world_dxy')


def _edit_b(specs, twin):
    # world_dheading replaced by world_res (with a world heading offset the reference overwrites the residuals' effect, :459-465); both terms.
    # opt_lr 5e-3: 25 steps of 1e-3 move an orientation by at most 0.025, less than ten times the case's orientation tolerance
    s = specs['init_opt']
    s['opt_lr'] = 5.e-3
    s['opt_variables'].remove('world_dheading')
    if not twin:
        s['opt_variables'].append('world_res')
        s['loss_cfg'].update(copy.deepcopy(TERMS))


def _edit_c(specs, twin):
    # world_dxy in the first stage only: it exists, and is applied but not optimised, in the second; world_res and both terms in the second,
    # where world_dheading makes the residuals inert
    if not twin:
        specs['init_opt']['opt_variables'].append('world_dxy')
        specs['main_opt']['opt_variables'].append('world_res')
        specs['main_opt']['loss_cfg'].update(copy.deepcopy(TERMS))


def _edit_d(specs, twin):
    # world_res with traj_trans_res monitor-only.  As in case b the stage's world_dheading gives way to world_res: beside it the residuals would
    # be inert (case c covers that), and the generator requires their first gradient to carry at least 1 % of the stage's.  opt_lr 3e-3: as in b
    s = specs['init_opt']
    _no_cam(s)
    s['opt_lr'] = 3.e-3
    s['opt_variables'].remove('world_dheading')
    if not twin:
        s['opt_variables'].append('world_res')
        s['loss_cfg']['traj_trans_res'] = dict(weight=1.0e2, monitor_only=True)


# case: config, frames, persons, iterations per stage, detection gap of person 0 (None: synth.make_in_dict's own), (person, first, last) of
# synth.trim_person or None, the edit of the schedule's copy, what the generator holds against the twin ('trans' / 'orient': at least ten
# tolerances apart), stages whose residuals are inert (exactly zero).
# Cases b and d have NO detection gap.  An orientation residual is a free variable per frame; in a frame nobody is seen in, its only gradient is
# traj_rot_smoothness's (1e-2 beside 1e3 in the frames around), Adam reaches that optimum within a few steps and then steps +-opt_lr with the
# sign of rounding noise, and the smoothness term carries the difference into the neighbouring frames' projections.  With synth's gap of 20
# frames the host runtime is 5e-3 (orientation residual), 3e-4 m and 0.45 px from the reference after 25 steps of case d, with frames 41-43 and
# 58-62 the worst, while every first-iteration gradient agrees to 3e-5 of its largest entry; without it 2e-6, 4e-6 m and 0.001 px.  The
# reference's own result in such frames is as arbitrary.  World_dxy (cases a, c) has no such frames: its gradient there is exactly zero.
CASES = {
    'a': dict(cfg_id='glamr_dynamic', T=120, P=1, K=25, gap=None, trim=None, edit=_edit_a, moved=('trans',), inert=()),
    'b': dict(cfg_id='glamr_static', T=90, P=1, K=25, gap=(0, 0), trim=None, edit=_edit_b, moved=('trans', 'orient'), inert=()),
    'c': dict(cfg_id='glamr_static_multi', T=120, P=2, K=15, gap=None, trim=(1, 20, 100), edit=_edit_c, moved=('trans',), inert=('main_opt',)),
    'd': dict(cfg_id='glamr_dynamic', T=120, P=1, K=25, gap=(0, 0), trim=None, edit=_edit_d, moved=('trans', 'orient'), inert=()),
    # case d's schedule on the scene WITH synth's detection gap, first-iteration losses and gradients only: the residuals in frames nobody is seen
    # in against the reference, without Adam's sign of rounding noise in what is compared
    'e': dict(cfg_id='glamr_dynamic', T=120, P=1, K=1, gap=None, trim=None, edit=_edit_d, moved=(), inert=(), first_only=True),
}
NEW_PERSON_KEYS = ['world_dxy', 'smpl_orient_world_res', 'root_trans_world_res']


def fixture_name(case, twin=False):
    return 'grecon_worldres_%s%s' % (case, '_twin' if twin else '')


def in_dict_of(case):
    c = CASES[case]
    d = synth.make_in_dict(seed=SEED, num_frames=c['T'], num_persons=c['P'], smpl_model=synth.make_smpl_model(), gap=c['gap'])
    if c['trim']:
        synth.trim_person(d, *c['trim'])
    return d


def stage_specs_of(opt_stage_specs, case, twin=False):
    """A copy of a schedule ({stage: spec}, the reference's or this package's) with the case's edit."""
    specs = copy.deepcopy(opt_stage_specs)
    CASES[case]['edit'](specs, twin)
    return specs


def config_of(case, twin=False):
    cfg = get_config(CASES[case]['cfg_id'])
    cfg['opt_stage_specs'] = stage_specs_of(cfg['opt_stage_specs'], case, twin)
    return cfg


# ---- runners: run(packed, sd, want_grads, world) -> (grads or None, world_ext's tensors or None); world as stepwise.world_stage gives it ------------
def _ext_of(packed, sd, world, want_grads):
    if world is None:
        return None, None
    return packing.world_ext(world, packed, niters=int(sd.niters), want_grads=want_grads, want_hist=packed.t.get('loss_history') is not None)


def hostsim_runner():
    from tests import hostsim
    fn = hostsim.build('grecon_wide_ext_host').hostsim_grecon_wide_run_stage_ext
    fn.argtypes = [ctypes.POINTER(_lib.SceneBatch), ctypes.POINTER(_lib.StageDesc), ctypes.POINTER(_lib.StageExt), ctypes.c_void_p]

    def run(packed, sd, want_grads, world=None):
        sb = packed.struct()
        grads = torch.zeros_like(packed.t['params']) if want_grads else None
        ext, keep = _ext_of(packed, sd, world, want_grads)
        assert fn(ctypes.byref(sb), ctypes.byref(sd), ctypes.byref(ext) if ext is not None else None, _lib.ptr(grads)) == 0
        return grads, keep
    return run, torch.device('cpu')


def device_runner():
    dev = torch.device('cuda:0')

    def run(packed, sd, want_grads, world=None):
        ext, keep = _ext_of(packed, sd, world, want_grads)
        grads = stepwise.run_stage(packed, sd, want_grads, ext=ext)
        torch.cuda.synchronize()
        return (grads.cpu() if want_grads else None), keep
    return run, dev


def world_grads_by_name(packed, keep, data, world, si=0):
    """The extension's gradient record under the names run_reference's record carries."""
    out = {}
    Ts = int(data['seq_len'])
    g = keep['grads'].cpu()
    for pi, idx in enumerate(packed.person_ids[si]):
        for v in world['variables']:
            for key in (('world_dxy',) if v == 'world_dxy' else ('smpl_orient_world_res', 'root_trans_world_res')):
                out['p%d_%s' % (idx, key)] = g[si * packed.P + pi, :Ts, packing.WORLD_KEYS[key]]
    return out


def check_case(runner, asset_root, golden, case, against_twin=False, report=None, run_twin=False):
    """Runs `case` from the oracle's init_data state stage by stage and holds it against its fixture -- or, against_twin, against the TWIN's
    fixture, which it must miss; run_twin: the twin's schedule (the unchanged path) against the twin's fixture, the yardstick of KSTEP_TOL_C.  Every stage's first-iteration loss values and gradients with
    tests/grecon_common.check_case's formula, the new variables' included; the state after K iterations per stage with the case's KSTEP_TOL
    row (KSTEP_TOL_C for case c), the new tensors with the root-translation / orientation bound.  `report`: a dict that receives the figures."""
    from oracle import make_golden as mg
    from oracle.port import build
    from tests import grecon_common as gc
    run, dev = runner
    c = CASES[case]
    T, P, K = c['T'], c['P'], c['K']
    g = golden(fixture_name(case, against_twin or run_twin))
    cfg = config_of(case, run_twin)
    specs = cfg['grecon_model_specs']
    in_dict = in_dict_of(case)
    ora = build.load_optimizer(asset_root, cfg)
    data = ora.init_data(in_dict, latents=mg.latents_for(in_dict, SEED))
    jl = gc.j_local_from_oracle(ora.smpl, data)
    has_wd = False
    failures = []

    def hold(ok, msg):
        if not ok:
            failures.append(msg)
    for stage, full_spec in cfg['opt_stage_specs'].items():
        spec, world_cfg = packing.split_world(full_spec)
        # first-iteration losses and gradients vs autograd of the reference
        packed1 = packing.PackedScenes([data], [jl], dev)
        world = stepwise.world_stage(packed1, world_cfg)
        grads, keep = run(packed1, packing.stage_desc(spec, specs, has_wd, niters=1), True, world)
        named = gc.grads_by_name(packed1, grads, data, specs, spec['opt_variables'])
        if world:
            named.update(world_grads_by_name(packed1, keep, data, world))
        refs = {n: g.get('%s_grad_%s' % (stage, n)) for n in named}
        gmax = max([float(np.abs(r).max()) for r in refs.values() if r is not None and r.size] + [0.0])
        for name, val in named.items():
            ref = refs[name]
            if ref is None:
                hold(against_twin, '%s: the fixture has no gradient of %s' % (stage, name))
                continue
            assert tuple(val.shape) == ref.shape, name
            if ref.size == 0:
                continue
            tol = 3e-4 * max(1.0, float(np.abs(ref).max())) + 2e-5 * gmax
            err = float(np.abs(val.numpy() - ref).max())
            if report is not None:
                report['%s_grad_%s' % (stage, name)] = (err, tol)
            hold(err < tol, '%s gradient %s: abs err %.2e > %.2e' % (stage, name, err, tol))
            if world_cfg and stage in c['inert'] and name.endswith('_res'):
                hold(not np.any(val.numpy()), '%s gradient %s of an inert residual is not exactly zero' % (stage, name))
        values = {n: float(packed1.t['losses'][0, i].cpu()) for n, i in packing.LOSS_IDS.items()}
        if world is not None:
            values.update({n: float(keep['losses'][0, i].cpu()) for n, i in packing.WORLD_TERMS.items() if n in world.get('terms', ())})
        for lname, got in values.items():
            key = '%s_loss_%s' % (stage, lname)
            if key in g:
                hold(abs(got - float(g[key])) <= 2e-4 * max(1.0, abs(float(g[key]))), '%s loss %s: %g vs %g' % (stage, lname, got, float(g[key])))
        # K iterations of the stage
        packed = packing.PackedScenes([data], [jl], dev)
        world = stepwise.world_stage(packed, world_cfg)
        _, keep = run(packed, packing.stage_desc(spec, specs, has_wd, niters=min(K, spec['opt_niters'])), False, world)
        if world is not None:
            stepwise.end_world_stage(packed, world, keep)
        packed.unpack_into([data], spec, specs)
        has_wd = has_wd or 'world_dheading' in spec['opt_variables']
        if world_cfg and stage in c['inert']:
            for pd in data['person_data'].values():
                for key in ('smpl_orient_world_res', 'root_trans_world_res'):
                    hold(not np.any(np.asarray(pd[key])), '%s: inert residual %s moved' % (stage, key))
            hold(not np.any(keep['losses'].cpu().numpy()), '%s: values of the inert residuals are not 0' % stage)
    if c.get('first_only'):
        return failures
    tol_kp, tol_tr, tol_rot = KSTEP_TOL_C if case == 'c' else gc.KSTEP_TOL[(c['cfg_id'], T, P)]
    worst = dict(kp=0.0, trans=0.0, orient=0.0, world_dxy=0.0, root_trans_world_res=0.0, smpl_orient_world_res=0.0)
    for pi in range(P):
        pd = data['person_data'][pi]
        vis = g['init_p%d_vis_frames' % pi] & g['init_p0_vis_frames']
        worst['kp'] = max(worst['kp'], gc.kp_err(pd['kp_2d_pred'].numpy(), g['opt_p%d_kp_2d_pred' % pi], vis))
        worst['trans'] = max(worst['trans'], float(np.abs(pd['root_trans_world'].numpy() - g['opt_p%d_root_trans_world' % pi]).max()))
        worst['orient'] = max(worst['orient'], gc._rot_err(pd['smpl_orient_world'].numpy(), g['opt_p%d_smpl_orient_world' % pi]))
        for key in NEW_PERSON_KEYS:
            ref = g.get('opt_p%d_%s' % (pi, key))
            if key in pd and ref is not None:
                worst[key] = max(worst[key], float(np.abs(np.asarray(pd[key]) - ref).max()))
            elif key in pd and np.any(np.asarray(pd[key])):
                hold(against_twin, '%s is not in the fixture' % key)
    if report is not None:
        report.update(worst)
    print('world residuals case %s%s K=%d: %s' % (case, ' against its TWIN' if against_twin else '', K, '  '.join('%s %.3g' % kv for kv in worst.items())))
    hold(worst['kp'] < tol_kp, 'kp_2d_pred after optimisation: %g px (bound %g)' % (worst['kp'], tol_kp))
    for key, tol in (('trans', tol_tr), ('world_dxy', tol_tr), ('root_trans_world_res', tol_tr), ('orient', tol_rot), ('smpl_orient_world_res', tol_rot)):
        hold(worst[key] < tol, '%s after optimisation: %g (bound %g)' % (key, worst[key], tol))
    return failures


# Case c's trimmed scene matches no shipped (cfg, T, P): twice the error the UNCHANGED path shows on the twin fixture (the twin's schedule on
# glamr_grecon_run_stage against grecon_worldres_c_twin), floored at the smallest row of tests/grecon_common.KSTEP_TOL, column by column.
#   unchanged path on the twin, host runtime / MI355X:   kp 0.0109 / 0.0104 px   root 7.2e-7 / 4.0e-6 m   orientation 3.8e-4 / 1.7e-4
#   the case itself, host runtime / MI355X:              kp 0.0013 / 0.0015 px   root 1.6e-6 / 4.8e-6 m   orientation 3.5e-4 / 2.6e-4   
KSTEP_TOL_C = (0.0218, 8.1e-6, 7.6e-4)
