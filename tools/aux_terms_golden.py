"""Fixtures of the six loss_cfg terms of packing.AUX_LOSS_IDS from the UNMODIFIED reference (build container only):
`python tools/aux_terms_golden.py [case ...]` writes tests/golden/grecon_aux_<case>.npz and its twin grecon_aux_<case>_twin.npz for the cases of
tests/aux_terms_e2e.py.

A case is a shipped schedule with the case's entries added to a COPY of cfg.opt_stage_specs, run by oracle.make_golden.run_reference for K
iterations per stage (nothing under oracle/ is changed).  Arrays only: init_* (the state after init_data), opt_* (after the run), every stage's
first-iteration <stage>_loss_* / <stage>_grad_*, <stage>_hist_<name> (K,): the term's unweighted value at every iteration of the stage (what
compute_loss returned inside the closure), and final_value_<name>: the values after the run, by forward + compute_loss once more.  The twin
is the same scene, schedule and K without the six names.

Asserted, and printed: each term's first-iteration weighted gradient is at least 1 % of the norm of the stage's whole gradient, or -- where
that gradient is zero by construction (tests/aux_terms_e2e.py ZERO_AT_START, with the reasons) -- it is below 1e-4 of it and the recorded value
after the run is > 0, or exactly 0 for a term listed as structurally zero for the case."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg          # noqa: E402
from oracle import ref_harness as rh          # noqa: E402
from glamr_amd.global_recon import packing    # noqa: E402
from tests import aux_terms_e2e as ae         # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MIN_SHARE = 0.01


def _leaves(data):
    out = []
    for d in [data] + list(data['person_data'].values()):
        out += [v for v in d.values() if torch.is_tensor(v) and v.is_leaf and v.requires_grad]
    return out


def run_case(case, twin=False):
    """-> (arrays of the fixture, {stage: {name: share of the stage's first gradient}}, {name: value after the run})."""
    c = ae.CASES[case]
    model, cfg = rh.reference_optimizer(c['cfg_id'], log=rh.QuietLog())
    specs = ae.stage_specs_with_terms(cfg.opt_stage_specs, case, twin)
    in_dict = ae.in_dict_of(case)
    stage_of = {id(spec['loss_cfg']): stage for stage, spec in specs.items()}
    hist, term_grad = {stage: [] for stage in specs}, {}
    plain = model.compute_loss

    def recording(data, loss_cfg):
        total, ld, lud = plain(data, loss_cfg)
        stage = stage_of.get(id(loss_cfg))
        if stage is not None:
            names = [n for n in loss_cfg if n in packing.AUX_LOSS_IDS]
            hist[stage].append({n: float(torch.as_tensor(lud[n]).detach()) for n in names})
            if stage not in term_grad:      # the stage's first evaluation (run_reference's gradient record): every term's own weighted gradient
                leaves = _leaves(data)
                term_grad[stage] = {}
                for n in names:
                    g = torch.autograd.grad(ld[n], leaves, retain_graph=True, allow_unused=True) if torch.is_tensor(ld[n]) and ld[n].requires_grad else []
                    term_grad[stage][n] = float(np.sqrt(sum(float(x.pow(2).sum()) for x in g if x is not None)))
        return total, ld, lud

    model.compute_loss = recording
    grads = {}
    try:
        data, init_state = mg.run_reference(model, specs, in_dict, mg.latents_for(in_dict, c['seed']), niters=c['K'], grads_out=grads)
    finally:
        model.compute_loss = plain
    out = {'init_' + k: v for k, v in init_state.items()}
    out.update({'opt_' + k: v for k, v in mg._flatten_state(data, mg.PERSON_KEYS_OPT, mg.TOP_KEYS).items()})
    shares = {}
    for stage, g in grads.items():
        out.update({'%s_%s' % (stage, k): v for k, v in g.items()})
        whole = float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for k, v in g.items() if k.startswith('grad_'))))
        shares[stage] = {n: v / whole for n, v in term_grad.get(stage, {}).items()}
        rows = hist[stage][1:]      # (the first evaluation is the gradient record's, at the same parameters as iteration 0)
        for n in (rows[0] if rows else {}):
            out['%s_hist_%s' % (stage, n)] = np.asarray([r[n] for r in rows], np.float64)
    final = {}
    if not twin:
        last, spec = list(specs.items())[-1]
        with torch.no_grad():
            model.forward(data, spec['opt_variables'], {'stage': last})
            _, _, lud = plain(data, {n: e for n, e in spec['loss_cfg'].items() if n in packing.AUX_LOSS_IDS})
        final = {n: float(torch.as_tensor(v).detach()) for n, v in lud.items()}
        out.update({'final_value_' + n: np.asarray(v, np.float64) for n, v in final.items()})
    out['niters'] = np.array(c['K'])
    return out, shares, final


def main(argv):
    for case in (argv or list(ae.CASES)):
        out, shares, final = run_case(case)
        for stage, sh in shares.items():
            for n, s in sh.items():
                at_start, zero = n in ae.ZERO_AT_START[case].get(stage, ()), n in ae.STRUCTURALLY_ZERO[case]
                print('%-20s %-9s %-26s share of the first gradient %.3e   value after the run %.6g%s' % (case, stage, n, s, final.get(n, float('nan')),
                      '   (structurally 0)' if zero else '   (first gradient 0 by construction)' if at_start else ''))
                if at_start:
                    assert s < 1e-4 and ((final[n] == 0) if zero else (final[n] > 0)), (case, stage, n, s, final[n])
                else:
                    assert s >= MIN_SHARE and not zero, (case, stage, n, s)
        np.savez_compressed(os.path.join(GOLD, ae.fixture_name(case) + '.npz'), **out)
        twin = run_case(case, twin=True)[0]
        np.savez_compressed(os.path.join(GOLD, ae.fixture_name(case, True) + '.npz'), **twin)
        print('wrote', ae.fixture_name(case), os.path.getsize(os.path.join(GOLD, ae.fixture_name(case) + '.npz')), 'bytes and its twin')


if __name__ == '__main__':
    main(sys.argv[1:])
