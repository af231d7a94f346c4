"""Fixtures of the vector headings (grecon_model_specs heading_type = 'vec') from the UNMODIFIED reference (build container only):
`python tools/heading_vec_golden.py [case ...]` writes tests/golden/grecon_headvec_<case>.npz and, for the cases that run K iterations, the scalar
twin grecon_headvec_<case>_twin.npz (no existing fixture has these scenes: a and b have no detection gap, b its own cam_fix_frames, c a trimmed
person), for the cases of tests/heading_vec_common.py.

A case is a shipped config run by oracle.make_golden.run_reference with model.heading_type = 'vec' (and the case's cam_fix_frames) set on the
reference's optimiser; nothing under oracle/ is changed.  Arrays only: init_* (the state after init_data), opt_* (after K iterations per stage),
every stage's first-iteration <stage>_loss_* / <stage>_grad_*.

Asserted, and printed: each vec variable's first gradient is at least 1 % of the norm of its stage's whole gradient in the stages that
optimise it, and root_trans_world / smpl_orient_world after the run differ from the scalar twin's by at least ten of the case's tolerances."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg          # noqa: E402
from oracle import ref_harness as rh          # noqa: E402
from tests import grecon_common as gc         # noqa: E402
from tests import heading_vec_common as hv    # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MIN_SHARE = 0.01
MIN_MOVED = 10.0


def run_case(case, twin=False):
    """-> (arrays of the fixture, {stage: {vec variable: share of the stage's whole first gradient}})."""
    c = hv.CASES[case]
    model, cfg = rh.reference_optimizer(c['cfg_id'], log=rh.QuietLog())
    if not twin:
        model.heading_type = 'vec'
    if c['fix'] is not None:
        model.cam_fix_frames = [list(x) for x in c['fix']]
    specs = hv.stage_specs_of(cfg.opt_stage_specs, case, twin)
    in_dict = hv.in_dict_of(case)
    grads = {}
    data, init_state = mg.run_reference(model, specs, in_dict, mg.latents_for(in_dict, hv.SEED), niters=c['K'], grads_out=grads)
    out = {'init_' + k: v for k, v in init_state.items()}
    out.update({'opt_' + k: v for k, v in mg._flatten_state(data, mg.PERSON_KEYS_OPT, mg.TOP_KEYS).items()})
    shares = {}
    for stage, g in grads.items():
        out.update({'%s_%s' % (stage, k): v for k, v in g.items()})
        norm = lambda keys: float(np.sqrt(sum(float((g[k].astype(np.float64) ** 2).sum()) for k in keys)))
        whole = norm([k for k in g if k.startswith('grad_')])
        shares[stage] = {k[5:]: norm([k]) / whole for k in g if k.startswith('grad_p') and k.split('_', 2)[2] in hv.VEC_KEYS and g[k].size}
    out['niters'] = np.array(c['K'])
    return out, shares


def main(argv):
    for case in (argv or list(hv.CASES)):
        c = hv.CASES[case]
        out, shares = run_case(case)
        for p in range(c['P']):
            assert out['opt_p%d_traj_local_heading' % p].shape == (2,) and out['opt_p%d_traj_local_dheading' % p].ndim == 2, 'the reference did not run vec headings'
        for stage, sh in shares.items():
            for n, s in sh.items():
                print('%s %-9s %-26s share of the whole first gradient %.3e' % (case, stage, n, s))
        for stage, sh in shares.items():      # a variable's share is taken over the scene's persons (case c: person 1 carries 99 % of init_opt's gradient)
            for key in hv.VEC_KEYS:
                parts = [s for n, s in sh.items() if n.split('_', 1)[1] == key]
                if parts:
                    s = float(np.sqrt(sum(x * x for x in parts)))
                    print('%s %-9s %-26s over the persons %.3e' % (case, stage, key, s))
                    assert s >= MIN_SHARE, (case, stage, key, s)
        assert any(shares.values()), case
        if c.get('first_only'):
            np.savez_compressed(os.path.join(GOLD, hv.fixture_name(case) + '.npz'), **{k: v for k, v in out.items() if not k.startswith('opt_')})
            print('wrote', hv.fixture_name(case), os.path.getsize(os.path.join(GOLD, hv.fixture_name(case) + '.npz')), 'bytes')
            continue
        twin = run_case(case, twin=True)[0]
        tol = gc.KSTEP_TOL[(c['cfg_id'], c['T'], c['P'])]
        moved = {'trans': 0.0, 'orient': 0.0}
        for pi in range(c['P']):
            moved['trans'] = max(moved['trans'], float(np.abs(out['opt_p%d_root_trans_world' % pi] - twin['opt_p%d_root_trans_world' % pi]).max()) / tol[1])
            moved['orient'] = max(moved['orient'], gc._rot_err(out['opt_p%d_smpl_orient_world' % pi], twin['opt_p%d_smpl_orient_world' % pi]) / tol[2])
        print('%s after the run, against the scalar twin: root_trans_world %.1f tolerances, smpl_orient_world %.1f tolerances' % (case, moved['trans'], moved['orient']))
        assert max(moved.values()) >= MIN_MOVED, (case, moved)
        np.savez_compressed(os.path.join(GOLD, hv.fixture_name(case) + '.npz'), **out)
        np.savez_compressed(os.path.join(GOLD, hv.fixture_name(case, True) + '.npz'), **twin)
        print('wrote', hv.fixture_name(case), os.path.getsize(os.path.join(GOLD, hv.fixture_name(case) + '.npz')), 'bytes and its twin',
              os.path.getsize(os.path.join(GOLD, hv.fixture_name(case, True) + '.npz')), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1:])
