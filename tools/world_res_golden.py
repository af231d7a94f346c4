"""Fixtures of the world-frame residuals (`world_dxy` / `world_res`, traj_rot_res / traj_trans_res) from the UNMODIFIED reference
(build container only): `python tools/world_res_golden.py [case ...]` writes tests/golden/grecon_worldres_<case>.npz and its twin
grecon_worldres_<case>_twin.npz for the cases of tests/world_res_e2e.py.

A case is a shipped schedule with the case's edit applied to a COPY of cfg.opt_stage_specs, run by oracle.make_golden.run_reference for K
iterations per stage (nothing under oracle/ is changed; its list of parameter names, which does not know the new variables, is replaced for the
call by one in get_parameter's order, global_recon_model.py:591-633).  Arrays only: init_* (the state after init_data), opt_* (after the run, the
new tensors included), every stage's first-iteration <stage>_loss_* / <stage>_grad_*.  The twin is the same scene, schedule and K without the
four names.

Asserted, and printed: each new variable's first gradient is at least 1 % of the norm of its stage's whole gradient -- exactly zero where the
case declares the residuals inert --, and root_trans_world / smpl_orient_world after the run differ from the twin's by at least ten of the case's
tolerances (tests/world_res_e2e.py `moved`).  The share of the gradient over the persons' variables alone is printed beside it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg          # noqa: E402
from oracle import ref_harness as rh          # noqa: E402
from tests import grecon_common as gc         # noqa: E402
from tests import world_res_e2e as we         # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MIN_SHARE = 0.01
MIN_MOVED = 10.0


def param_names(model, data, opt_variables):
    """Names in the order get_parameter (global_recon_model.py:591-633) appends them, the world-frame residuals included."""
    names = []
    if 'cam' not in opt_variables:
        names += ['cam_inv_rot_residual', 'cam_inv_trans_residual']
    else:
        names += ['cam_rot_6d_fix', 'cam_trans_fix'] if model.flag_fixed_cam else ['cam_rot_6d', 'cam_trans']
    for idx in data['person_data'].keys():
        for key in opt_variables:
            if key == 'world_res':
                names += ['p%d_smpl_orient_world_res' % idx, 'p%d_root_trans_world_res' % idx]
            if 'local' in key:
                names.append('p%d_traj_%s' % (idx, key))
        if 'world_dheading' in opt_variables:
            names.append('p%d_world_dheading' % idx)
        if 'world_dxy' in opt_variables:
            names.append('p%d_world_dxy' % idx)
    return names


def run_case(case, twin=False):
    """-> (arrays of the fixture, {stage: {new variable: (share of the stage's first gradient over the persons' variables, of the whole)}})."""
    c = we.CASES[case]
    model, cfg = rh.reference_optimizer(c['cfg_id'], log=rh.QuietLog())
    specs = we.stage_specs_of(cfg.opt_stage_specs, case, twin)
    in_dict = we.in_dict_of(case)
    grads = {}
    keep = mg._param_names
    mg._param_names = param_names
    try:
        data, init_state = mg.run_reference(model, specs, in_dict, mg.latents_for(in_dict, we.SEED), niters=c['K'], grads_out=grads)
    finally:
        mg._param_names = keep
    out = {'init_' + k: v for k, v in init_state.items()}
    person_keys = mg.PERSON_KEYS_OPT + ([] if twin else we.NEW_PERSON_KEYS)
    out.update({'opt_' + k: v for k, v in mg._flatten_state(data, person_keys, mg.TOP_KEYS).items()})
    shares = {}
    for stage, g in grads.items():
        out.update({'%s_%s' % (stage, k): v for k, v in g.items()})
        norm = lambda keys: float(np.sqrt(sum(float((g[k].astype(np.float64) ** 2).sum()) for k in keys)))
        whole, persons = norm([k for k in g if k.startswith('grad_')]), norm([k for k in g if k.startswith('grad_p')])
        shares[stage] = {k[5:]: (norm([k]) / persons, norm([k]) / whole) for k in g if k.startswith('grad_') and k.split('_', 2)[2] in we.NEW_PERSON_KEYS}
    out['niters'] = np.array(c['K'])
    return out, shares


def main(argv):
    for case in (argv or list(we.CASES)):
        c = we.CASES[case]
        out, shares = run_case(case)
        if c.get('first_only'):      # (first-iteration values only: nothing is held against a twin)
            for stage, sh in shares.items():
                for n, (s, of_whole) in sh.items():
                    print('%s %-9s %-28s share of the first gradient: of the whole %.3e' % (case, stage, n, of_whole))
                    assert of_whole >= MIN_SHARE, (case, stage, n, of_whole)
            np.savez_compressed(os.path.join(GOLD, we.fixture_name(case) + '.npz'), **{k: v for k, v in out.items() if not k.startswith('opt_')})
            continue
        twin = run_case(case, twin=True)[0]
        for stage, sh in shares.items():
            for n, (s, of_whole) in sh.items():
                inert = stage in c['inert'] and n.endswith('_res')
                print('%s %-9s %-28s share of the first gradient: of the persons\' variables %.3e, of the whole %.3e%s' % (case, stage, n, s, of_whole, '   (inert: exactly 0)' if inert else ''))
                assert (of_whole == 0.0) if inert else (of_whole >= MIN_SHARE), (case, stage, n, of_whole)
        assert any(shares.values()), case
        tol = we.KSTEP_TOL_C if case == 'c' else gc.KSTEP_TOL[(c['cfg_id'], c['T'], c['P'])]
        moved = {'trans': 0.0, 'orient': 0.0}
        for pi in range(c['P']):
            moved['trans'] = max(moved['trans'], float(np.abs(out['opt_p%d_root_trans_world' % pi] - twin['opt_p%d_root_trans_world' % pi]).max()) / tol[1])
            moved['orient'] = max(moved['orient'], gc._rot_err(out['opt_p%d_smpl_orient_world' % pi], twin['opt_p%d_smpl_orient_world' % pi]) / tol[2])
        print('%s after the run, against the twin: root_trans_world %.1f tolerances, smpl_orient_world %.1f tolerances' % (case, moved['trans'], moved['orient']))
        for what in c['moved']:
            assert moved[what] >= MIN_MOVED, (case, what, moved[what])
        np.savez_compressed(os.path.join(GOLD, we.fixture_name(case) + '.npz'), **out)
        np.savez_compressed(os.path.join(GOLD, we.fixture_name(case, True) + '.npz'), **twin)
        print('wrote', we.fixture_name(case), os.path.getsize(os.path.join(GOLD, we.fixture_name(case) + '.npz')), 'bytes and its twin',
              os.path.getsize(os.path.join(GOLD, we.fixture_name(case, True) + '.npz')), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1:])
