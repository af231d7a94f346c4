"""Reference of the latent regularisers (motion_latent_reg / traj_latent_reg, loss_func.py:293-310) in the latent-optimisation mode.
`RegLatentOptimizer` is tests/attach_common.AttachedLatentOptimizer whose compute_loss adds the two terms, written from the reference's
functions on the port's names for the latents (in_motion_latent / in_traj_latent); the loop is attach_common.e2e_reference's with the
per-iteration values and the first gradient WITH PRIORS recorded.  Everything runs in the dtype it is given (fp64 for the expectations,
fp32 for the rounding floors the tolerances are 16 x of).

Semantics that follow from the reference as it is (global_recon_model.py:428-445, 533-570, 591-633): compute_loss evaluates every term of the
stage's loss_cfg in every iteration, also before opt_latent_start_iter; the latents are Adam parameters from the first iteration of a stage, so
before opt_latent_start_iter the regulariser alone steps them; with the detach of :396 nothing but traj_latent_reg reaches traj_latent."""
import copy

import numpy as np
import torch

from oracle import make_golden as mg
from oracle.port import build, transforms as tf
from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth
from tests import attach_common as ac

FLOOR_FACTOR = ac.FLOOR_FACTOR
KINK = ac.KINK
K = 5
TERMS = ('motion_latent_reg', 'traj_latent_reg')          # the order of glamr_latent_reg's terms and of latent_loss_history's last axis


def motion_latent_reg_loss(data, specs):
    """loss_func.py:293-300"""
    loss_all, num_latent = 0, 0
    for d in data['person_data'].values():
        num_latent += d['in_motion_latent'].shape[0]
        loss_all = loss_all + d['in_motion_latent'].pow(2).sum()
    return loss_all / num_latent


def traj_latent_reg_loss(data, specs):
    """loss_func.py:303-310"""
    loss_all, num_latent = 0, 0
    for d in data['person_data'].values():
        num_latent += d['in_traj_latent'].shape[0]
        loss_all = loss_all + d['in_traj_latent'].pow(2).sum()
    return loss_all / num_latent


REG_FUNCS = {'motion_latent_reg': motion_latent_reg_loss, 'traj_latent_reg': traj_latent_reg_loss}

# mutations of the reference: each must move the least-moved quantity it touches by at least 2 tolerances (tests/test_latent_reg_ref.py)
MUTATIONS = {'slots': 'motion_latent_reg divided by the number of persons instead of windows',
             'padded': 'padded window rows counted in the denominator',
             'skip': 'regulariser skipped before opt_latent_start_iter',
             'no_weight': 'weight not applied',
             'monitor': 'monitor_only ignored',
             'no_traj_step': 'traj_latent not stepped in detached mode'}


class RegLatentOptimizer(ac.AttachedLatentOptimizer):
    reg_mut = None
    start_iter = 0

    def compute_loss(self, data, loss_cfg):
        total, ld, lud = super().compute_loss(data, {n: c for n, c in loss_cfg.items() if n not in REG_FUNCS})
        persons = list(data['person_data'].values())
        for name in TERMS:
            if name not in loss_cfg:
                continue
            spec = loss_cfg[name]
            lud[name] = REG_FUNCS[name](data, spec)
            if name == 'motion_latent_reg' and self.reg_mut in ('slots', 'padded'):
                rows = sum(d['in_motion_latent'].shape[0] for d in persons)
                wrong = len(persons) if self.reg_mut == 'slots' else len(persons) * max(d['in_motion_latent'].shape[0] for d in persons)
                lud[name] = lud[name] * rows / wrong
            ld[name] = lud[name] * (1.0 if self.reg_mut == 'no_weight' else spec['weight'])
            if (self.reg_mut == 'skip' and self.cur_iter < self.start_iter) or self.reg_mut == 'skip_all':      # ('skip_all': the data terms alone, for the shares)
                continue
            if not spec.get('monitor_only', False) or self.reg_mut == 'monitor':
                total = total + ld[name]
        return total, ld, lud


# name: (config, frames, persons, trim, {stage: opt_latent_start_iter}, candidate seeds, {term: weight})
# (a) one person, 70 frames = two infiller windows; the only stage starts the priors at iteration 2: iterations 0-1 are regulariser-only.
# (b) two persons of 70 and 38 frames = 2 windows and 1 window: a padded window row, ragged counts, two stages.
# The weights put the regulariser between 10 % and 90 % of each latent's gradient norm at the first iteration with priors (attached run, fp64;
# REG_SHARE holds the measured shares |g_reg| / (|g_reg| + |g_data|), tests/test_latent_reg_ref.py measures them again).
CASES = {'a': ('glamr_dynamic', 70, 1, None, {'init_opt': 2}, (37, 49, 57, 62), {'motion_latent_reg': 20.0, 'traj_latent_reg': 3000.0}),
         'b': ('glamr_dynamic_multi', 70, 2, (1, 12, 50), {}, (36, 82), {'motion_latent_reg': 6.0e-5, 'traj_latent_reg': 15.0})}
KINKED = {'a': (), 'b': ()}
REG_SHARE = {'a': {'motion': 0.5, 'traj': 0.5}, 'b': {'motion': 0.5, 'traj': 0.5}}


def case_seed(name):
    return [s for s in CASES[name][5] if s not in KINKED[name]][0]


def case_inputs(name, seed=None):
    cfg_id, T, P, trim, _, _, _ = CASES[name]
    seed = case_seed(name) if seed is None else seed
    in_dict = synth.make_in_dict(seed=seed, num_frames=T, num_persons=P, smpl_model=synth.make_smpl_model(), gap=(0, 0))
    if trim is not None:
        in_dict = synth.trim_person(in_dict, *trim)
    return cfg_id, in_dict, mg.latents_for(in_dict, seed), P


def case_config(name, weights=None, monitor=(), terms=TERMS):
    """The case's configuration: its opt_latent_start_iter and the regularisers appended to every stage's loss_cfg."""
    cfg = get_config(CASES[name][0])
    weights = CASES[name][6] if weights is None else weights
    for stage, spec in cfg['opt_stage_specs'].items():
        spec['opt_latent_start_iter'] = CASES[name][4].get(stage, 0)
        for t in terms:
            spec['loss_cfg'][t] = dict(weight=weights[t], **({'monitor_only': True} if t in monitor else {}))
    return cfg


_INIT, _RUNS = {}, {}


def _state(asset_root, name, seed):
    if (name, seed) not in _INIT:
        cfg_id, in_dict, lat, _ = case_inputs(name, seed)
        ora = build.load_optimizer(asset_root, get_config(cfg_id))
        ora.__class__ = RegLatentOptimizer
        with torch.no_grad():
            data = ora.init_data(in_dict, latents=lat)
        _INIT[(name, seed)] = (ora, data)
    return _INIT[(name, seed)]


def relu_margin(asset_root, name, seed):
    """attach_common.relu_margin for a case of this file: the smallest |ReLU pre-activation| of the two priors' fp64 forward at the initial latents."""
    from tests.nets_vjp_common import RELU_INPUTS
    ora, data0 = _state(asset_root, name, seed)
    mt = copy.deepcopy(ora.mt_model)
    mt.mfiller.double(), mt.traj_predictor.double()
    mt.traj_predictor.__dict__['smpl'] = copy.deepcopy(ora.smpl).double()
    margins = []
    hooks = [m.register_forward_hook(lambda mod, i, o: margins.append(float(o.detach().abs().min())))
             for net in (mt.mfiller, mt.traj_predictor) for n, m in net.named_modules()
             if isinstance(m, torch.nn.Linear) and any(k in n for k in RELU_INPUTS)]
    old, mt0 = torch.get_default_dtype(), ora.mt_model
    try:
        torch.set_default_dtype(torch.float64)
        ora.mt_model = mt
        with torch.no_grad():
            for d in ac._cast(copy.deepcopy(data0), torch.float64)['person_data'].values():
                ac.AttachedLatentOptimizer.infer_motion_traj(ora, d)
    finally:
        ora.mt_model = mt0
        torch.set_default_dtype(old)
        for h in hooks:
            h.remove()
    return min(margins)


def reference(asset_root, name, dtype=torch.float64, attached=True, mut=None, weights=None, monitor=(), terms=TERMS, opt_motion=True, seed=None):
    """K iterations per stage of the port's latent-optimisation loop with the regularisers, in `dtype`.  Returns
    {'values': {stage: (iterations, 2)}, idx: {g_traj (128,), g_motion (windows, 128): the latents' gradients of the run's first iteration
    with priors (None where autograd gave none), traj_latent (1, 128), motion_latent (windows, 128): after the K iterations}}.  Cached."""
    seed = case_seed(name) if seed is None else seed
    key = (name, seed, dtype, attached, mut, None if weights is None else tuple(sorted(weights.items())), tuple(monitor), tuple(terms), opt_motion)
    if key in _RUNS:
        return _RUNS[key]
    ora, data0 = _state(asset_root, name, seed)
    cfg = case_config(name, weights, monitor, terms)
    data = ac._cast(copy.deepcopy(data0), dtype)
    smpl0, mt0, old = ora.smpl, ora.mt_model, torch.get_default_dtype()
    out = {'values': {}}
    first = {}
    try:
        torch.set_default_dtype(dtype)
        ora.smpl = copy.deepcopy(smpl0).to(dtype)
        ora.mt_model = copy.deepcopy(mt0)
        ora.mt_model.mfiller.to(dtype), ora.mt_model.traj_predictor.to(dtype)
        ora.mt_model.traj_predictor.__dict__['smpl'] = ora.smpl
        ora.mut, ora.attached, ora.reg_mut, ora.opt_motion = None, attached, mut, opt_motion
        ora.opt_traj = not (mut == 'no_traj_step' and not attached)
        for d in data['person_data'].values():
            for key_ in ('in_motion_latent', 'in_traj_latent'):
                d[key_] = d[key_].detach().clone()
        for stage, spec in cfg['opt_stage_specs'].items():
            start = spec['opt_latent_start_iter']
            ora.start_iter = start
            rows = []

            def log_fn(stage_, it, uw, start=start):
                rows.append([uw.get(t, 0.0) for t in TERMS])
                if it >= start and not first:
                    for idx, d in data['person_data'].items():
                        first[idx] = {k: (None if d[key_].grad is None else d[key_].grad.detach().double().numpy().copy())
                                      for k, key_ in (('g_motion', 'in_motion_latent'), ('g_traj', 'in_traj_latent'))}
            ora.log_fn = log_fn
            ora.optimize_main(data, spec['opt_variables'], spec['opt_lr'], min(K, spec['opt_niters']), spec['loss_cfg'],
                              {'stage': stage, 'opt_latent_start_iter': start})
            out['values'][stage] = np.asarray(rows, np.float64)
            if spec.get('reinitialize_cam', False):
                data['cam_pose'][:] = data['cam_pose'][[0]]
                data['cam_pose_inv'] = tf.invert_transform(data['cam_pose'])
        for idx, d in data['person_data'].items():
            out[idx] = dict(first[idx])
            if out[idx]['g_traj'] is not None:
                out[idx]['g_traj'] = out[idx]['g_traj'].reshape(-1)
            out[idx].update(traj_latent=d['in_traj_latent'].detach().double().numpy(), motion_latent=d['in_motion_latent'].detach().double().numpy())
    finally:
        ora.smpl, ora.mt_model, ora.mut, ora.attached, ora.cur_iter, ora.log_fn = smpl0, mt0, None, True, 0, None
        ora.reg_mut, ora.opt_traj, ora.opt_motion = None, True, True
        torch.set_default_dtype(old)
    _RUNS[key] = out
    return out


KEYS = ('g_traj', 'g_motion', 'traj_latent', 'motion_latent', 'values')


def errors(got, ref):
    """Worst error over the persons: the first gradients relative to the person's largest reference entry, the latents after the K iterations
    absolute (the draws are of order one), the per-iteration values relative to the largest reference value of the term."""
    P = [i for i in ref if i != 'values']
    e = {'g_traj': max(ac.rel_err(got[i]['g_traj'], ref[i]['g_traj']) for i in P),
         'g_motion': max(ac.rel_err(got[i]['g_motion'], ref[i]['g_motion']) for i in P),
         'traj_latent': max(float(np.abs(np.asarray(got[i]['traj_latent'], np.float64).reshape(-1) - ref[i]['traj_latent'].reshape(-1)).max()) for i in P),
         'motion_latent': max(float(np.abs(np.asarray(got[i]['motion_latent'], np.float64) - ref[i]['motion_latent']).max()) for i in P)}
    e['values'] = max(ac.rel_err(np.asarray(got['values'][s])[:, t], ref['values'][s][:, t]) for s in ref['values'] for t in range(2))
    return e


# fp32 run of this reference against its fp64 run (one thread), rounded up to two digits; tests/test_latent_reg_ref.py measures them again
# and fails outside [1/2, 2] x the constant
FLOOR = {('a', True): {'g_traj': 3.8e-7, 'g_motion': 6.3e-7, 'traj_latent': 3.9e-7, 'motion_latent': 4.0e-7, 'values': 1.1e-7},       # 3.748e-7, 6.214e-7, 3.871e-7, 3.994e-7, 1.066e-7
         ('a', False): {'g_traj': 8.2e-8, 'g_motion': 5.7e-7, 'traj_latent': 2.3e-7, 'motion_latent': 3.3e-7, 'values': 1.4e-7},      # 8.177e-8, 5.630e-7, 2.229e-7, 3.209e-7, 1.338e-7
         ('b', True): {'g_traj': 8.8e-6, 'g_motion': 3.0e-6, 'traj_latent': 8.1e-6, 'motion_latent': 2.2e-4, 'values': 1.2e-6},       # 8.724e-6, 2.949e-6, 8.096e-6, 2.183e-4, 1.127e-6
         ('b', False): {'g_traj': 2.8e-8, 'g_motion': 4.3e-8, 'traj_latent': 6.6e-7, 'motion_latent': 7.3e-7, 'values': 1.3e-7}}      # 2.728e-8, 4.221e-8, 6.545e-7, 7.219e-7, 1.203e-7
TOL = {c: {k: FLOOR_FACTOR * v for k, v in f.items()} for c, f in FLOOR.items()}

# The kernel test's synthetic batch: 3 scenes x 3 slots, n_win_max = 3
KERNEL_WINDOWS = np.array([[3, 1, 0], [2, 2, 2], [1, 0, 0]], np.int32)
# fp32 sum of squares of N(0, 1) draws in the kernel's order of magnitude against fp64, relative, for at most 6 x 128 terms: 16 x this bounds the values.
# Measured on the CPU for these sizes with numpy's fp32 pairwise sum and with a sequential fp32 loop (the worse of the two), rounded up.
KERNEL_VALUE_FLOOR = 4.8e-7          # 4.744e-7 (the sequential loop)
KERNEL_VALUE_TOL = FLOOR_FACTOR * KERNEL_VALUE_FLOOR


def kernel_inputs(seed=5):
    """meps (9, 3, 128), teps (9, 128) fp32 with NaN in every padded row and empty slot, and the window counts (9,)."""
    rng = np.random.default_rng(seed)
    nw = KERNEL_WINDOWS.reshape(-1)
    meps = rng.normal(size=(9, 3, 128)).astype(np.float32)
    teps = rng.normal(size=(9, 128)).astype(np.float32)
    for k, n in enumerate(nw):
        meps[k, n:] = np.nan
        if n == 0:
            teps[k] = np.nan
    return meps, teps, nw.copy()


def kernel_reference(meps, teps, nw, weights):
    """fp64 values (3, 2), and per term (rows per scene, fp32 gradient fl(fl(w / n) * 2 z) with zeros in padded rows, fp64 gradient)."""
    S, P = KERNEL_WINDOWS.shape
    real_m = np.arange(3)[None, :] < nw[:, None]                       # (9, 3)
    real_t = nw > 0
    zm = np.where(real_m[..., None], meps, 0).astype(np.float64)
    zt = np.where(real_t[:, None], teps, 0).astype(np.float64)
    rows = np.stack([nw.reshape(S, P).sum(1), real_t.reshape(S, P).sum(1)], 1)          # (3, 2)
    values = np.stack([(zm ** 2).reshape(S, -1).sum(1), (zt ** 2).reshape(S, -1).sum(1)], 1) / rows
    g32, g64 = [], []
    for t, z in enumerate((zm, zt)):
        c32 = (np.float32(weights[t]) / rows[:, t].astype(np.float32)).astype(np.float32)          # fl(w / n)
        c = np.repeat(c32, P).reshape((-1,) + (1,) * (z.ndim - 1))
        g32.append((c * (np.float32(2) * z.astype(np.float32))).astype(np.float32))
        g64.append(2.0 * float(weights[t]) / np.repeat(rows[:, t], P).reshape(c.shape).astype(np.float64) * z)
    return values, rows, g32, g64, real_m, real_t


# The fp64 runs take the CPU tens of seconds, so the device tests read them from tests/golden/latent_reg_e2e.npz (written by
# `python -m tests.latent_reg_common`, numbers only); tests/test_latent_reg_ref.py runs the port again and holds the file to it.
FIXTURE = 'latent_reg_e2e'
RUNS = [(n, att) for n in CASES for att in (True, False)]


def _tag(name, attached):
    return '%s_%s' % (name, 'att' if attached else 'det')


def fixture_arrays(asset_root):
    out = {}
    for name, att in RUNS:
        r = reference(asset_root, name, attached=att)
        for stage, v in r['values'].items():
            out['%s_values_%s' % (_tag(name, att), stage)] = v
        for idx in (i for i in r if i != 'values'):
            for k, v in r[idx].items():
                if v is not None:
                    out['%s_p%d_%s' % (_tag(name, att), idx, k)] = v
    return out


def from_fixture(g, name, attached):
    tag = _tag(name, attached)
    out = {'values': {k[len(tag) + 8:]: v for k, v in g.items() if k.startswith(tag + '_values_')}}
    for idx in range(CASES[name][2]):
        out[idx] = {k: g.get('%s_p%d_%s' % (tag, idx, k)) for k in ('g_traj', 'g_motion', 'traj_latent', 'motion_latent')}
    return out


if __name__ == '__main__':
    import os
    import tempfile
    root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', FIXTURE + '.npz'), **fixture_arrays(root))
