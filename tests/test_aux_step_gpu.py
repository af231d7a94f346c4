"""glamr_grecon_aux_step and grecon_model_specs.flag_aux_on_device on the MI355X: the fused kernel against the host runtime, held
to the distance of the composed entry points it replaces (the parent's code, run in the same test); two calls bit-equal, a captured launch
replayed on new inputs; and the schedule end to end -- the three fixtures of the unmodified reference through stage_inputs ->
optimize_resident -> collect, monitor-only terms against ExtraLossSchedule(skip_term=True), capture_resident, optimize_stream, the refusals
that stay."""
import copy

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import aux_step_schedule, extra_loss_schedule as xs, packing
from oracle import make_golden as mg
from tests import aux_step_common as A
from tests import aux_terms_common as C
from tests import aux_terms_e2e as ae
from tests.test_aux_terms_gpu import E2E_FLOOR, HISTORY_RTOL, TWIN_FACTOR, _model, _packed, _run_schedule, _state_errors, priors      # noqa: F401 (priors: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEAM_FACTOR = 4      # multiply-add contraction may differ at the seams between the composed functions


def _entries():
    L = _lib.lib()
    st = _lib.current_stream
    adam = lambda p, m, v, g, lr, step: _lib.check(L.glamr_adam_step(p.numel(), _lib.ptr(p), _lib.ptr(m), _lib.ptr(v), _lib.ptr(g), float(lr), int(step), st()))
    ws = dict(aux=L.glamr_grecon_aux_terms_workspace_bytes, cam=L.glamr_grecon_cam_backward_workspace_bytes, pose=L.glamr_grecon_pose_backward_workspace_bytes,
              fused=L.glamr_grecon_aux_step_workspace_bytes)
    return A.Entries(lambda *a: L.glamr_grecon_aux_terms(*a, st()), lambda *a: L.glamr_grecon_cam_backward(*a, st()), lambda *a: L.glamr_grecon_pose_backward(*a, st()),
                     lambda *a: L.glamr_grecon_aux_step(*a, st()), ws, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV), lambda t: t.detach().cpu().numpy(), adam)


_HOST = {}


def _host(name):
    """The host-runtime result of a case (the fused header; the CPU suite holds it bit-equal to the composition), computed once."""
    if name not in _HOST:
        _HOST[name] = A.Run(name, A.host_entries(composed=False), True).record
    return _HOST[name]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', A.CASE_NAMES)
def test_kernel_against_the_host_runtime(name):
    """Per output group, over three consecutive steps: |fused device - host| <= max(4 x |composed device entry points - host|, 2^-23), both in
    aux_terms_common's relative measure.  Measured on the MI355X: DESIGN.md 20."""
    host, e = _host(name), _entries()
    fused, comp = A.Run(name, e, True).record, A.Run(name, e, False).record
    again = A.Run(name, e, True).record
    worst = {g: (0.0, 0.0) for g in A.GROUPS}
    for k in range(A.N_STEPS):
        df, dc = A.distance(fused[k], host[k]), A.distance(comp[k], host[k])
        for g in A.GROUPS:
            assert np.isfinite(fused[k][g]).all(), (name, k, g)      # (a NaN read anywhere, or a poisoned entry left in place)
            worst[g] = (max(worst[g][0], df[g]), max(worst[g][1], dc[g]))
    print('%s MI355X, fused | composed distance from the host runtime: %s' % (name, ', '.join('%s %.2e | %.2e' % (g, *worst[g]) for g in A.GROUPS)))
    for k in range(A.N_STEPS):
        df, dc = A.distance(fused[k], host[k]), A.distance(comp[k], host[k])
        for g in A.GROUPS:
            assert df[g] <= max(SEAM_FACTOR * dc[g], 2.0 ** -23), (name, k, g, df[g], dc[g])
    # two runs give the same bits
    for k in range(A.N_STEPS):
        for g in A.GROUPS:
            assert A.bit_equal(fused[k][g], again[k][g]), (name, k, g)
    # entries no phase may write keep the incoming gradient's bits
    keep, (_, st) = A.untouched(C.cases()[name]), A.arrays(name)
    for k in range(A.N_STEPS):
        assert A.bit_equal(fused[k]['grads'][keep], st['grads_in'][k][keep]), (name, k)
        if name == 'monitor_all':
            assert A.bit_equal(fused[k]['grads'], st['grads_in'][k])


@pytest.mark.parametrize('name', ['slots3', 'frame257'])
def test_captured_launch_replays_on_new_inputs(name):
    """The call recorded into a torch.cuda.graph and replayed after inputs and state changed in place equals a plain launch on them."""
    _, st = A.arrays(name)
    r = A.Run(name, _entries(), True, n_steps=0)
    grads = torch.from_numpy(st['grads_in'][0]).to(DEV)
    step = A.FIRST_STEP
    state = lambda: {k: v.clone() for k, v in dict(r.state, grads=grads, values=r.values).items()}

    def restore(s):
        for k, v in s.items():
            (grads if k == 'grads' else r.values if k == 'values' else r.state[k]).copy_(v)
    s0 = state()
    r.fused_call(0, grads, step)
    torch.cuda.synchronize()
    first = state()
    restore(s0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.fused_call(0, grads, step)
    # new inputs in the same buffers: the trajectories shifted and scaled, another gradient, moved parameters
    restore(s0)
    r.a['trans_world'].mul_(1.25).add_(0.5)
    grads.copy_(torch.from_numpy(st['grads_in'][1]).to(DEV))
    r.state['params'].mul_(1.0625)
    s1 = state()
    graph.replay()
    torch.cuda.synchronize()
    replayed = state()
    restore(s1)
    r.fused_call(0, grads, step)
    torch.cuda.synchronize()
    plain = state()
    for k in plain:
        assert torch.isfinite(plain[k]).all() and A.bit_equal(replayed[k].cpu().numpy(), plain[k].cpu().numpy()), (name, k)
    assert not torch.equal(plain['values'], first['values']) and not torch.equal(plain['params'], first['params'])


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------
def _cfg(case, twin=False, edit=None, flag=True):
    cfg = ae.config_of(case, twin=twin, edit=edit)
    cfg['grecon_model_specs']['flag_aux_on_device'] = flag
    return cfg


def _inputs(case):
    in_dict = ae.in_dict_of(case)
    return in_dict, mg.latents_for(in_dict, ae.CASES[case]['seed'])


def _resident(model, in_dict, lat, K):
    rin = model.stage_inputs([copy.deepcopy(in_dict)], [lat])
    datas, packed = model.optimize_resident(rin, K)
    return model.collect(datas, packed), packed


@pytest.mark.parametrize('case', list(ae.CASES))
def test_resident_path_matches_the_reference_after_k_steps(golden, priors, case):
    """stage_inputs -> optimize_resident -> collect with the flag on, against the unmodified reference: the bounds of
    tests/test_aux_terms_gpu.py::test_optimize_matches_the_reference_after_k_steps (TWIN_FACTOR x the same entry point's distance without the
    names from the twin fixture, not below E2E_FLOOR; glamr_3dpw: keypoints only) and aux_loss_history against the fixture's histories."""
    (in_dict, lat), c = _inputs(case), ae.CASES[case]
    err = {}
    for twin in (True, False):
        model = _model(priors, _cfg(case, twin))
        out, packed = _resident(model, in_dict, lat, c['K'])
        err[twin] = _state_errors(case, out[0]['person_data'], golden(ae.fixture_name(case, twin)))
    bound = [max(TWIN_FACTOR * t, f) for t, f in zip(err[True], E2E_FLOOR)]
    print('%s K=%d on the resident path: with the terms kp %.4f px, root_trans_world %.2e m, smpl_orient_world %.2e | twin %.4f px, %.2e m, %.2e | bounds %.4f px, %.2e m, %.2e'
          % (case, c['K'], *err[False], *err[True], *bound))
    for q in range(1 if c['cfg_id'] == 'glamr_3dpw' else 3):
        assert err[False][q] <= bound[q], (case, q, err[False][q], bound[q])
    g = golden(ae.fixture_name(case))
    assert sorted(model.aux_loss_history) == sorted(c['terms'])
    for st, terms in c['terms'].items():
        assert sorted(model.aux_loss_history[st]) == sorted(terms)
        for name in terms:
            hist, ref = model.aux_loss_history[st][name], g['%s_hist_%s' % (st, name)]
            assert hist.shape == (1, len(ref))
            e = np.abs(hist[0] - ref) / np.maximum(1.0, np.abs(ref))
            print('%s %s history %s: worst %.2e of max(1, value) (bound %.1e)' % (case, st, name, e.max(), HISTORY_RTOL))
            assert (e <= HISTORY_RTOL).all(), (case, st, name, hist[0], ref)
    # informative: the distance from ExtraLossSchedule (the flag off) on the same input
    off = _model(priors, _cfg(case, flag=False))
    datas, p_off = off.init_data_batch([copy.deepcopy(in_dict)], [lat], init_forward=False)
    xs.ExtraLossSchedule(off, p_off).run(max_iters=c['K'])
    torch.cuda.synchronize()
    a, b = packed.t['params'].double(), p_off.t['params'].double()
    print('%s params, AuxStepSchedule against ExtraLossSchedule: max |diff| %.2e of largest entry %.3g' % (case, float((a - b).abs().max()), float(b.abs().max())))


@pytest.mark.parametrize('case', ['glamr_dynamic', 'glamr_3dpw'])
def test_all_terms_monitor_only_equal_the_schedule_with_the_terms_skipped(asset_root, priors, case):
    def monitor(name, entry):
        if name in packing.AUX_LOSS_IDS:
            entry['monitor_only'] = True
    K = ae.CASES[case]['K']
    _, _, skipped = _run_schedule(asset_root, priors, case, _cfg(case, edit=monitor, flag=False), skip_term=True)
    model = _model(priors, _cfg(case, edit=monitor))
    _, packed = _packed(asset_root, case)
    aux_step_schedule.AuxStepSchedule(model, packed).run(max_iters=K)
    torch.cuda.synchronize()
    want, got = skipped.t['params'].cpu().numpy(), packed.t['params'].cpu().numpy()
    assert np.abs(want).max() > 0 and np.array_equal(want, got)
    hist = aux_step_schedule.publish(model._aux_cfg, packed.aux_values)
    assert all(h.shape == (1, K) and h.any() for st in hist.values() for n, h in st.items() if n not in ae.STRUCTURALLY_ZERO[case])      # (the values are still recorded)


KEYS = ('params', 'kp_2d_pred', 'trans_world', 'orient_world', 'cam_pose')


def test_capture_resident_replays_the_schedule(priors):
    case, K = 'glamr_static_multi', 3
    in_dict, lat = _inputs(case)
    model = _model(priors, _cfg(case))
    st = torch.cuda.Stream()
    rin = model.stage_inputs([in_dict], [lat])
    torch.cuda.synchronize()

    def plain():
        with torch.cuda.stream(st):
            _, ref = model.optimize_resident(rin, max_iters=K)
        torch.cuda.synchronize()
        return {k: ref.t[k].clone() for k in KEYS}, {s: v.clone() for s, v in ref.aux_values.items()}
    want, want_vals = plain()                                                  # (also the first run on this stream: allocations, attribute calls)
    rg = model.capture_resident(rin, max_iters=K, stream=st, check=True)      # passes its own replay check

    def replayed():
        for k in KEYS:
            rg.packed.t[k].fill_(float('nan'))
        for v in rg.packed.aux_values.values():
            v.fill_(float('nan'))
        torch.cuda.synchronize()
        rg.replay()
        torch.cuda.synchronize()
    replayed()
    for k in KEYS:
        assert torch.equal(rg.packed.t[k], want[k]), k
    assert sorted(rg.packed.aux_values) == sorted(want_vals) and all(torch.equal(rg.packed.aux_values[s], want_vals[s]) for s in want_vals)
    assert all(torch.isfinite(v).all() and v.shape[1] == K for v in want_vals.values())
    # other inputs in place: the graph follows them
    rin.g['trans'].add_(0.05)
    rin.g['kp'][..., :2].add_(1.5)
    torch.cuda.synchronize()
    replayed()
    want2, want_vals2 = plain()
    assert not torch.equal(want2['params'], want['params'])
    for k in KEYS:
        assert torch.equal(rg.packed.t[k], want2[k]), k
    assert all(torch.equal(rg.packed.aux_values[s], want_vals2[s]) for s in want_vals2)
    out = model.collect(rg.datas, rg.packed)
    assert sorted(model.aux_loss_history) == sorted(ae.CASES[case]['terms']) and np.isfinite(np.asarray(out[0]['person_data'][0]['root_trans_world'])).all()


def test_optimize_stream_equals_the_resident_path(priors):
    """Three one-scene batches in flight: every yielded array and every batch's aux_loss_history equal optimize_resident + collect of that batch alone."""
    case, K = 'glamr_dynamic', 3
    c = ae.CASES[case]
    batches, lats = [], []
    for i in range(3):
        d = ae.synth.make_in_dict(seed=c['seed'] + 10 * i, num_frames=c['T'], num_persons=c['P'], smpl_model=ae.synth.make_smpl_model(), gap=c['gap'])
        batches.append([d])
        lats.append([mg.latents_for(d, c['seed'] + i)])
    model = _model(priors, _cfg(case))
    alone = []
    for b, l in zip(batches, lats):
        out, _ = _resident(model, b[0], l[0], K)
        alone.append((out, copy.deepcopy(model.aux_loss_history)))
    n = 0
    for i, out in enumerate(model.optimize_stream([copy.deepcopy(b) for b in batches], latents=lats, max_iters=K)):
        want, want_hist = alone[i]
        for key in ('root_trans_world', 'smpl_orient_world', 'kp_2d_pred'):
            assert np.array_equal(np.asarray(out[0]['person_data'][0][key]), np.asarray(want[0]['person_data'][0][key])), (i, key)
        assert np.array_equal(np.asarray(out[0]['cam_pose']), np.asarray(want[0]['cam_pose'])), i
        hist = model.aux_loss_history
        assert sorted(hist) == sorted(want_hist)
        for s in hist:
            for name in hist[s]:
                assert np.array_equal(hist[s][name], want_hist[s][name]), (i, s, name)
        n += 1
    assert n == 3
    assert not np.array_equal(alone[0][1]['init_opt']['cam_depth_smoothness'], alone[1][1]['init_opt']['cam_depth_smoothness'])


def test_refusals_that_stay(priors):
    """The flag on: a caller's extra_loss or a penetration term still takes the three entry points away, as without it; latent mode,
    flag_opt_vis_local_rot and absolute_heading are refused where the optimiser is made; a person-sharded batch where the schedule starts."""
    case = 'glamr_dynamic'
    in_dict, lat = _inputs(case)
    model = _model(priors, _cfg(case))
    assert model._aux_on_device() and model._off_kernel_term() is None
    rin = model.stage_inputs([in_dict], [lat])
    model.extra_loss = lambda ctx: (ctx.trans_world ** 2).sum((1, 2, 3))
    for name, call in (('optimize_resident', lambda: model.optimize_resident(rin, 1)), ('optimize_stream', lambda: model.optimize_stream([[in_dict]])),
                       ('capture_resident', lambda: model.capture_resident(rin, 1))):
        with pytest.raises(NotImplementedError, match=name + ' while extra_loss is set'):
            call()
    model.extra_loss = None
    from tests import penetration_e2e as pe
    pen_cfg = copy.deepcopy(pe.device_cfg())
    pen_cfg['grecon_model_specs']['flag_aux_on_device'] = True
    for spec in pen_cfg['opt_stage_specs'].values():
        spec['loss_cfg']['traj_trans_smoothness'] = dict(weight=5.0e2)
    pen = _model(priors, pen_cfg)
    assert not pen._aux_on_device()
    p_in, p_lat = pe.scene_inputs()
    p_rin = pen.stage_inputs([p_in], [p_lat])
    for name, call in (('optimize_resident', lambda: pen.optimize_resident(p_rin, 1)), ('optimize_stream', lambda: pen.optimize_stream([[p_in]])),
                       ('capture_resident', lambda: pen.capture_resident(p_rin, 1))):
        with pytest.raises(NotImplementedError, match=name + '.*penetration'):
            call()
    for flags, word in ((dict(flag_opt_vis_local_rot=True), 'flag_opt_vis_local_rot'), (dict(absolute_heading=True), 'absolute_heading'),
                        (dict(flag_opt_traj_latent=True), 'latent')):
        cfg = _cfg(case)
        cfg['grecon_model_specs'].update(flags)
        with pytest.raises(ValueError, match='cam_rot_smoothness.*local_traj_dheading_reg.*' + word):
            _model(priors, cfg)
    datas, packed = model.init_data_batch([in_dict], [lat], init_forward=False)
    packed.t['frozen'] = torch.zeros(packed.S * packed.P, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='cam_rot_smoothness.*person-sharded'):
        aux_step_schedule.AuxStepSchedule(model, packed).run(max_iters=1)
    # optimize() and continue_batch() run the same schedule
    res = model.optimize(copy.deepcopy(in_dict), latents=lat, max_iters=2)
    assert all(h.shape == (1, 2) for st in model.aux_loss_history.values() for h in st.values())
    again = model.optimize(res, continue_opt=True, max_iters=1)
    assert np.isfinite(np.asarray(again['person_data'][0]['root_trans_world'])).all() and all(h.shape == (1, 1) for st in model.aux_loss_history.values() for h in st.values())
