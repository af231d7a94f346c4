"""Cases, inputs and the oracle of glamr_grecon_aux_step (csrc/grecon_aux_step.hpp) for tests/test_aux_step_ref.py (CPU: the
header on the host runtime) and tests/test_aux_step_gpu.py.  The oracle is the COMPOSITION the fused step replaces, on identical inputs:
glamr_grecon_aux_terms in add mode on zeroed scratch adjoints, glamr_grecon_cam_backward and glamr_grecon_pose_backward accumulating into the
gradient array on the conditions extra_loss_schedule.ExtraLossSchedule launches them on, then torch.optim.Adam.

Inputs: the cases of tests/aux_terms_common.py (the one with max_len 1 serves the refusal only) plus what the two VJPs read -- traj_local_pred,
base_orient, person2cam, orient_world, dheading_mask and the residual rows of params -- as well-conditioned random values: 6D rotations
[1 0 0 0 1 0] + 0.2 randn, headings within a few hundredths of a radian per frame, axis-angles of ~0.8 rad, residuals 0.05 randn.  NaN
wherever the composed calls are documented not to read: what aux_terms_common.host_arrays poisons, the new arrays outside existing rows /
visible frames / present slots, all of them when their VJP does not run.  params, the incoming gradient and the moments are finite everywhere:
Adam reads every element of a scene's row.  The cases need not come from a real forward pass: both sides see the same numbers."""
import ctypes

import numpy as np
import torch

from glamr_amd import _lib
from glamr_amd.global_recon import packing
from tests import aux_terms_common as C

CASE_NAMES = [n for n in C.CASE_NAMES if max(Ts for Ts, _ in C.SPECS[n]['scenes']) >= 2]
REFUSED_CASE = 'seq1'                  # max_len 1: glamr_grecon_pose_backward's geometry limit
LR, FIRST_STEP, N_STEPS = 1e-2, 3, 3   # steps 3, 4, 5 on non-zero moments: a step number off by one moves every parameter
GROUPS = ('grads', 'values', 'params', 'exp_avg', 'exp_avg_sq')


def liveness(case):
    """(run_cam, derived, run_pose): which VJPs an iteration runs -- ExtraLossSchedule._add_terms' conditions."""
    gm = case['mask'] & ~case['monitor']
    on_trans, on_cam = gm & ((1 << C.TRAJ) | (1 << C.CAMTRAJ)), gm & ((1 << C.DEPTH) | (1 << C.CAMTRAJ))
    run_cam = bool(on_cam) and case['mode'] != 'constant'
    derived = run_cam and case['mode'] == 'derived'
    return run_cam, derived, bool(on_trans) or derived


def stage_desc(case):
    """aux_terms_common's descriptor; a camera derived from the persons also carries the world heading offset as a variable."""
    sd = C.stage_desc(case)
    if case['mode'] == 'derived':
        sd.var_mask |= C.VB['world_dheading']
        sd.flags |= packing.FLAG_HAS_WORLD_DHEADING
    return sd


_ARRAYS = {}


def arrays(name):
    """(batch arrays, state): numpy, built once per case and never modified (callers copy)."""
    if name in _ARRAYS:
        return _ARRAYS[name]
    case = C.cases()[name]
    S, P, T, l = case['S'], case['P'], case['T'], C.layout(case)
    rng = np.random.default_rng(4200 + C.CASE_NAMES.index(name))
    run_cam, derived, run_pose = liveness(case)
    a = C.host_arrays(case)
    nan = lambda *s: np.full(s, np.nan, np.float32)
    a.update(traj_local_pred=nan(S * P, T, 11), base_orient=nan(S * P, T, 3), person2cam=nan(S * P, T, 12), orient_world=nan(S * P, T, 3), dheading_mask=nan(S * P, T))
    params = a['params']
    hole = ~np.isfinite(params)
    params[hole] = (0.05 * rng.normal(size=int(hole.sum()))).astype(np.float32)
    for si, sc in enumerate(case['scenes']):
        Ts = sc['Ts']
        if case['mode'] in ('frame', 'fixed'):      # the camera VJP reads the rotation rows whatever the terms: a rotation, not noise
            rows = Ts if case['mode'] == 'frame' else 1
            params[si, l['cam_rot6d']:l['cam_rot6d'] + 6 * rows] = sc['cam_rot6d'][:rows].reshape(-1)
        for pi, p in enumerate(sc['persons']):
            slot, (fs, fe), v = si * P + pi, p['fr'], p['vis']
            n = fe - fs
            if run_pose:
                pr = np.zeros((n, 11))
                pr[:, 0:2] = 0.03 * rng.normal(size=(n, 2))
                pr[:, 2] = 0.9 + 0.05 * rng.normal(size=n)
                pr[:, 3:9] = np.array([1, 0, 0, 0, 1, 0.0]) + 0.2 * rng.normal(size=(n, 6))
                h = 0.05 * rng.normal(size=n)
                h[0] = rng.uniform(-3, 3)
                pr[:, 9], pr[:, 10] = np.cos(h), np.sin(h)
                a['traj_local_pred'][slot, :n] = pr
                a['dheading_mask'][slot, 1:n] = rng.integers(0, 2, size=max(n - 1, 0))      # (row 0 is never read)
            if derived:
                k = int(v.sum())
                assert np.isfinite(a['trans_world'][slot, :Ts][v]).all()
                a['orient_world'][slot, :Ts][v] = 0.8 * rng.normal(size=(k, 3))
                R, t = C._rot(rng.normal(size=(k, 3))) if k else np.zeros((0, 3, 3)), rng.normal(size=(k, 3, 1))
                a['person2cam'][slot, :Ts][v] = np.concatenate([R, t], axis=-1).reshape(k, 12)
                out = np.ones(Ts, bool)
                out[fs:fe] = False
                a['base_orient'][slot, :Ts][out] = 0.8 * rng.normal(size=(int(out.sum()), 3))
    shape = params.shape
    state = dict(params=params.copy(), exp_avg=(0.01 * rng.normal(size=shape)).astype(np.float32), exp_avg_sq=(1e-4 * rng.random(shape) + 1e-8).astype(np.float32))
    state['grads_in'] = [(0.1 * rng.normal(size=shape)).astype(np.float32) for _ in range(N_STEPS)]      # the "stage kernel's gradient" of each step
    _ARRAYS[name] = (a, state)
    return _ARRAYS[name]


def untouched(case):
    """(S, scene_stride) bool: entries of `grads` no phase may write -- camera blocks of other modes and rows at or beyond seq_len, empty slots,
    rows beyond a person's existing range, variables outside var_mask."""
    S, P, T, l = case['S'], case['P'], case['T'], C.layout(case)
    m = np.zeros((S, l['scene_stride']), bool)
    mode = case['mode']
    for si, sc in enumerate(case['scenes']):
        Ts = sc['Ts']
        for key, w in (('cam_rot6d', 6), ('cam_trans', 3), ('cam_inv_rot_res', 6), ('cam_inv_trans_res', 3)):
            mine = {'frame': key in ('cam_rot6d', 'cam_trans'), 'fixed': key in ('cam_rot6d', 'cam_trans'), 'derived': key.startswith('cam_inv'), 'constant': False}[mode]
            rows = 0 if not mine else (1 if mode == 'fixed' else Ts)
            m[si, l[key] + w * rows:l[key] + w * T] = True
        for pi in range(P):
            b = l['person0'] + pi * l['person_stride']
            if pi >= len(sc['persons']):
                m[si, b:b + l['person_stride']] = True
                continue
            fs, fe = sc['persons'][pi]['fr']
            n = fe - fs
            for key, w in (('local_dxy', 2), ('local_dheading', 1), ('local_z', 1), ('local_rot', 6)):
                m[si, b + l[key] + w * n:b + l[key] + w * T] = True
            if not case['dh_var']:
                m[si, b + l['local_dheading']:b + l['local_dheading'] + T] = True
            m[si, b + l['world_dheading'] + (Ts if mode == 'derived' else 0):b + l['world_dheading'] + T] = True
    return m


class Entries:
    """The entry points of one side (host runtime or device library) behind one calling convention.  aux / cam / pose / fused: the C
    functions (device: the stream argument already bound); adam(p, m, v, g, lr, step) for the composition; ws: {name: bytes(S, P, T)};
    to_device / to_host move a numpy array to where the entry points read it and back."""

    def __init__(self, aux, cam, pose, fused, ws, to_device, to_host, adam):
        self.aux, self.cam, self.pose, self.fused, self.ws, self.to_device, self.to_host, self.adam = aux, cam, pose, fused, ws, to_device, to_host, adam


def host_entries(composed=True):
    """The host builds (tests/hostsim); composed=False: the fused step alone (the three stand-alone builds are not compiled)."""
    from tests import hostsim
    V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double

    def fn(lib, name, args, res=I):
        f = getattr(hostsim.build(lib), name)
        f.argtypes, f.restype = args, res
        return f
    geo, Z = [I, I, I], ctypes.c_size_t
    fused = fn('grecon_aux_step_host', 'hostsim_grecon_aux_step', [V] * 5 + [I, I, V, V, V, D, I, V])
    fused_ws = fn('grecon_aux_step_host', 'hostsim_grecon_aux_step_workspace_floats', geo, Z)
    ws = dict(fused=lambda *g: 4 * fused_ws(*g))
    aux = cam = pose = None
    if composed:
        aux = fn('grecon_aux_host', 'hostsim_grecon_aux_terms', [V] * 8 + [I, V])
        cam = fn('grecon_cam_bwd_host', 'hostsim_grecon_cam_bwd', [V] * 4 + [I, V, V, V])
        pose = fn('grecon_pose_bwd_host', 'hostsim_grecon_pose_bwd', [V] * 5 + [I, V])
        cam_ws, pose_ws = fn('grecon_cam_bwd_host', 'hostsim_grecon_cam_bwd_workspace_floats', geo, Z), fn('grecon_pose_bwd_host', 'hostsim_grecon_pose_bwd_workspace_floats', geo, Z)
        ws.update(aux=lambda S, P, T: 4 * S * P, cam=lambda *g: 4 * cam_ws(*g), pose=lambda *g: 4 * pose_ws(*g))
    return Entries(aux, cam, pose, fused, ws, lambda x: np.ascontiguousarray(x).copy(), lambda x: np.array(x, copy=True), TorchAdam)


class TorchAdam:
    """torch.optim.Adam on the CPU holding `params` with the given moments, `first_step - 1` steps behind it.  fused=True: torch's one-pass CPU
    kernel, the single-tensor path's operation order with the hardware's correctly rounded square root.  The single-tensor path takes
    exp_avg_sq.sqrt() from a vector library whose result is 1 ulp off for 0.7 % of its arguments (tests/test_adam_exact.py), which moves
    about one parameter in a thousand by an ulp per step -- nothing an IEEE implementation can be held to bit for bit."""

    def __init__(self, params, exp_avg, exp_avg_sq, lr=LR, first_step=FIRST_STEP):
        self.p = torch.tensor(np.array(params, np.float32), requires_grad=True)
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=(0.9, 0.999), fused=True)
        self.opt.state[self.p] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=torch.tensor(np.array(exp_avg, np.float32)),
                                      exp_avg_sq=torch.tensor(np.array(exp_avg_sq, np.float32)))

    def step(self, grads):
        self.p.grad = torch.tensor(np.array(grads, np.float32))
        self.opt.step()
        st = self.opt.state[self.p]
        return self.p.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()


def _ptr(x):
    return None if x is None else _lib.ptr(x)


class Run:
    """N_STEPS consecutive iterations of one case on one side.  fused: the fused entry point; else the composition (skip_cam / step_shift:
    the two mutations).  record[k]: dict of the GROUPS after step k (numpy)."""

    def __init__(self, name, e, fused, skip_cam=False, step_shift=0, n_steps=N_STEPS):
        self.case = case = C.cases()[name]
        S, P, T = case['S'], case['P'], case['T']
        a, st = arrays(name)
        self.a = {k: e.to_device(v) for k, v in a.items()}
        self.sb, self.sd, self.ad = C.scene_batch(case, {k: _lib.ptr(v).value for k, v in self.a.items()}), stage_desc(case), C.aux_desc(case)
        self.state = {k: e.to_device(st[k]) for k in ('exp_avg', 'exp_avg_sq')}
        self.state['params'] = self.a['params']
        self.e, self.name, self.n_vals = e, name, max(n_steps, 1)
        self.values = e.to_device(np.full((S, self.n_vals, 6), np.nan, np.float32))
        geo = (S, P, T)
        zeros = lambda nbytes: e.to_device(np.zeros(max(nbytes // 4, 1), np.float32))
        self.record, self.rc = [], 0
        run_cam, derived, run_pose = liveness(case)
        if fused:
            self.ws = e.to_device(np.full(max(e.ws['fused'](*geo) // 4, 1), np.nan, np.float32))      # (contents irrelevant before the call)
        else:
            ws = {k: zeros(e.ws[k](*geo)) for k in ('aux', 'cam', 'pose')}
            adam = e.adam(st['params'], st['exp_avg'], st['exp_avg_sq']) if e.adam is TorchAdam else None
        for k in range(n_steps):
            grads = e.to_device(st['grads_in'][k])
            step = FIRST_STEP + k
            if fused:
                self.fused_call(k, grads, step + step_shift)
            else:
                g_t, g_o, g_c, vals = zeros(4 * S * P * T * 3), zeros(4 * S * P * T * 3), zeros(4 * S * T * 12), e.to_device(np.full((S, 6), np.nan, np.float32))
                rc = e.aux(ctypes.byref(self.sb), ctypes.byref(self.sd), ctypes.byref(self.ad), _ptr(self.a['root_trans_cam']), _ptr(vals), _ptr(g_t), _ptr(g_c),
                           _ptr(grads), 1, _ptr(ws['aux']))
                assert rc == 0, (name, 'aux', rc)
                if run_cam and not skip_cam:
                    rc = e.cam(ctypes.byref(self.sb), ctypes.byref(self.sd), _ptr(g_c), _ptr(grads), 1, _ptr(g_o if derived else None), _ptr(g_t if derived else None), _ptr(ws['cam']))
                    assert rc == 0, (name, 'cam', rc)
                if run_pose:
                    rc = e.pose(ctypes.byref(self.sb), ctypes.byref(self.sd), _ptr(g_o if derived else None), _ptr(g_t), _ptr(grads), 1, _ptr(ws['pose']))
                    assert rc == 0, (name, 'pose', rc)
                if adam is not None:      # torch.optim.Adam on the CPU; the batch's params row follows it (the next step's terms read it)
                    if step_shift and k == 0:
                        adam.opt.state[adam.p]['step'] += step_shift
                    p, m, v = adam.step(e.to_host(grads))
                    self.state['params'][...] = p
                    self.state['exp_avg'], self.state['exp_avg_sq'] = m, v
                else:
                    e.adam(self.state['params'], self.state['exp_avg'], self.state['exp_avg_sq'], grads, LR, step + step_shift)
                self.values[:, k] = vals
            self.record.append(dict(grads=e.to_host(grads), values=e.to_host(self.values)[:, k].copy(), **{g: e.to_host(self.state[g]) for g in ('params', 'exp_avg', 'exp_avg_sq')}))


    def fused_call(self, k, grads, step):
        """One call of the fused entry point on the run's arrays as they are: iteration k of the values, `grads` in and out."""
        e = self.e
        self.rc = e.fused(ctypes.byref(self.sb), ctypes.byref(self.sd), ctypes.byref(self.ad), _ptr(self.a['root_trans_cam']), _ptr(self.values), self.n_vals * 6, k,
                          _ptr(grads), _ptr(self.state['exp_avg']), _ptr(self.state['exp_avg_sq']), LR, step, _ptr(self.ws))
        assert self.rc == 0, (self.name, self.rc)


def bit_equal(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))


def distance(got, ref):
    """aux_terms_common's relative measure per group: the largest difference over the group's largest reference entry."""
    return {g: C._rel(np.asarray(got[g], np.float64), np.asarray(ref[g], np.float64)) for g in GROUPS}
