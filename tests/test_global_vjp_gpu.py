"""MI355X: the local-to-global step's VJP (glamr_traj_local_to_global_backward) against the fp64 autograd reference of
tests/global_vjp_common.py, the autograd layer above it (TrajPredVAE.global_traj, MotionInfillerVAE.infill, TrajPredVAE.local_traj with
in_body_pose) and MotionTrajJointModel.inference_grad: its values against inference, its gradients against the fp64 composite of
tests/global_vjp_chain.py (read from tests/golden)."""
import os

import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from glamr_amd import _lib
from glamr_amd.models import priors as pr
from tests import global_vjp_common as gc
from tests import global_vjp_chain as ch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CASES = [n for n, _, _ in gc._case_specs()]


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


class Launch:
    """One glamr_traj_local_to_global_backward call over the C ABI on buffers made beforehand (so it can be recorded into a graph)."""

    def __init__(self, case, G, lens='table'):
        self.L = _dev(case['L'])
        self.B, self.T = self.L.shape[:2]
        self.G = [_dev(g) for g in G]
        self.lens = _dev(np.asarray(case['lens'], np.int32), torch.int32) if lens == 'table' else None
        self.out = torch.full((self.B, self.T, 11), 7.0, device=DEV)          # (every entry must be overwritten)
        lib = _lib.lib()
        self.ws = torch.full((lib.glamr_traj_local_to_global_backward_workspace_bytes(self.B, self.T),), 0xff, dtype=torch.uint8, device=DEV)

    def __call__(self):
        _lib.check(_lib.lib().glamr_traj_local_to_global_backward(self.B, self.T, _lib.ptr(self.lens), _lib.ptr(self.L), _lib.ptr(self.G[0]), _lib.ptr(self.G[1]),
                                                                  _lib.ptr(self.G[2]), _lib.ptr(self.out), _lib.ptr(self.ws), _lib.current_stream()))
        return self.out


def _run(case, G, lens='table'):
    out = Launch(case, G, lens)().clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', CASES)
def test_kernel_matches_fp64_autograd(name):
    """Every upstream pattern of the case (NaN in the rows at or beyond a length) within 16 x the fp32 autograd floor per column group; the padded
    output rows are exact zeros; a second call gives the same bits."""
    case = gc.cases()['cases'][name]
    tol = gc.tol(name)
    worst = {k: 0.0 for k in gc.GROUPS}
    for pattern in gc.PATTERNS:
        G = gc.upstream(case, pattern)
        a, b = _run(case, G), _run(case, G)
        assert torch.equal(a, b)
        got = a.cpu().numpy()
        assert np.isfinite(got).all()
        for bi, n in enumerate(case['lens']):
            assert (got[bi, n:] == 0).all()
        e = gc.errors(got, gc.ref64(name, pattern), case['lens'])
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e)' % (k, worst[k], tol[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


@pytest.mark.parametrize('scale', [1e-6, 1e5])
def test_scaled_upstream_gradients_stay_within_the_tolerances(scale):
    """The kernel is plain fp32 and linear in G: with G x 1e-6 and G x 1e5 the results, divided by the factor, keep the tolerances (the
    reference is given the same scaled fp32 arrays, so the relative errors are those of the results divided by the factor)."""
    for name in CASES:
        case = gc.cases()['cases'][name]
        got = _run(case, gc.upstream(case, 'all', scale=scale)).cpu().numpy()
        e = gc.errors(got, gc.reference(case, 'all', scale=scale), case['lens'])
        print('G x %g, %s: %s' % (scale, name, ', '.join('%s %.2e' % kv for kv in e.items())))
        for k, v in e.items():
            assert v <= gc.tol(name)[k], (name, k, v)


def test_graph_replay_equals_the_plain_launch():
    """The call recorded into a torch.cuda.graph (one chain, no parallel branches) and replayed twice gives the plain launch's bits."""
    case = gc.cases()['cases']['ragged5']
    G = gc.upstream(case, 'all')
    plain = _run(case, G)
    launch = Launch(case, G)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        launch.out.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(launch.out, plain)


def test_null_lengths_mean_T_frames():
    case = gc.cases()['cases']['ragged3']
    T = case['L'].shape[1]
    full = dict(case, lens=(T,) * len(case['lens']))
    G = gc.upstream(full, 'all')
    assert torch.equal(_run(full, G, lens=None), _run(full, G))


def test_argument_checks():
    case = gc.cases()['cases']['T3']
    launch = Launch(case, (None, None, None))
    with pytest.raises(RuntimeError):
        launch()                                                               # no upstream gradient at all
    with pytest.raises(ValueError):
        pr.local_to_global_backward(launch.L, None)


# ---- the autograd layer ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def priors(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    return smpl, MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))


def test_global_traj_is_local_to_global_with_the_kernels_gradient(priors):
    _, mt = priors
    case = gc.cases()['cases']['ragged3']
    G = gc.upstream(case, 'all')
    L = _dev(case['L']).requires_grad_(True)
    outs = mt.traj_predictor.global_traj(L, lens=case['lens'])
    for a, b in zip(outs, pr.local_to_global(L.detach())):
        assert torch.equal(a, b)
    (g,) = torch.autograd.grad(outs, L, [_dev(x) for x in G])
    assert torch.equal(g, _run(case, G))
    # one output alone: the others reach the library as NULL
    outs = mt.traj_predictor.global_traj(L, lens=case['lens'])
    (g,) = torch.autograd.grad(outs[1], L, _dev(G[1]))
    assert torch.equal(g, _run(case, (None, G[1], None)))


def _batch(name):
    """The batch of a composite case: in_body_pose (B,T,69), frame_mask (B,T), latents (B,windows,128) / (B,128), lens."""
    seqs = ch.sequences(name)
    T = max(n for _, n in seqs)
    nw = pr.num_windows(T)
    pose, vis = torch.zeros(len(seqs), T, 69, device=DEV), torch.zeros(len(seqs), T, device=DEV)
    me, te = torch.zeros(len(seqs), nw, 128, device=DEV), torch.zeros(len(seqs), 128, device=DEV)
    for b, (seed, n) in enumerate(seqs):
        x = mg.net_inputs(n, seed)
        pose[b, :n], vis[b, :n] = torch.tensor(x['in_body_pose'][0]), torch.tensor(x['frame_mask'][0]).float()
        me[b, :x['in_motion_latent'].shape[0]] = torch.tensor(x['in_motion_latent'])
        te[b] = torch.tensor(x['in_traj_latent'][0])
    return dict(in_body_pose=pose, frame_mask=vis, in_motion_latent=me, in_traj_latent=te), [n for _, n in seqs]


KEYS = ('infer_out_body_pose', 'infer_out_local_traj_tp', 'infer_out_trans', 'infer_out_orient', 'infer_out_pose')


@pytest.mark.parametrize('name', list(ch.CHAIN))
def test_inference_grad_equals_inference_bit_for_bit(priors, name):
    """Every returned key of inference_grad against inference(batch, sample_num=1) under the same latents (inference shares ONE latent among the
    rows of a batch, so the rows are given the first sequence's; the shorter sequence is ragged through frame_mask, as inference has it); and,
    with lengths and a latent per row, against the plain batched call glamr_nets_infer on the rows below each length."""
    _, mt = priors
    batch, lens = _batch(name)
    B = len(lens)
    shared = dict(batch, in_motion_latent=batch['in_motion_latent'][0], in_traj_latent=batch['in_traj_latent'][:1])
    with torch.no_grad():
        plain = mt.inference(shared, sample_num=1)
    grad = mt.inference_grad(dict(batch, in_motion_latent=batch['in_motion_latent'][:1].expand(B, -1, -1).contiguous(),
                                  in_traj_latent=batch['in_traj_latent'][:1].expand(B, -1).contiguous()))
    for k in KEYS:
        assert grad[k].shape == plain[k].shape and torch.equal(grad[k], plain[k]), k
    if B == 1:          # (windows, 128) and (1, 128) are accepted for one sequence
        again = mt.inference_grad(shared)
        for k in KEYS:
            assert torch.equal(again[k], plain[k]), k
    out = mt.inference_grad(batch, lens=lens)
    ref = mt.handle.infer(batch['in_body_pose'], batch['frame_mask'], lens, motion_eps=batch['in_motion_latent'], traj_eps=batch['in_traj_latent'])
    for b, n in enumerate(lens):
        assert torch.equal(out['infer_out_body_pose'][b, 0, :n], ref['pose'][b, :n])
        assert torch.equal(out['infer_out_local_traj_tp'][:n, b, 0], ref['local_traj'][b, :n])
        assert torch.equal(out['infer_out_trans'][b, 0, :n], ref['trans'][b, :n])
        assert torch.equal(out['infer_out_orient'][b, 0, :n], ref['orient'][b, :n])


@pytest.mark.parametrize('name', list(ch.CHAIN))
def test_gradients_of_a_joint_loss_reach_both_latents(priors, golden, name):
    """L = sum(W * joints) of the body model on inference_grad's outputs -- infiller -> body pose -> FK -> predictor -> local-to-global -> SMPL --
    against the fp64 composite (tests/golden/global_vjp_chain.npz), each latent's gradient relative to the person's largest reference entry,
    within 16 x the fp32 port's own deviation from the fp64 run."""
    smpl, mt = priors
    batch, lens = _batch(name)
    g = golden(ch.FIXTURE)
    me, te = batch['in_motion_latent'].clone().requires_grad_(True), batch['in_traj_latent'].clone().requires_grad_(True)
    out = mt.inference_grad(dict(batch, in_motion_latent=me, in_traj_latent=te), lens=lens)
    loss = 0.0
    for b, n in enumerate(lens):
        j = smpl(global_orient=out['infer_out_orient'][b, 0, :n], body_pose=out['infer_out_body_pose'][b, 0, :n], betas=_dev(ch.betas(name, b))[None],
                 root_trans=out['infer_out_trans'][b, 0, :n], return_verts=False).joints
        loss = loss + (j * _dev(ch.weights(name, b, n, j.shape[1]))).sum()
    loss.backward()
    tol = ch.tol(name)
    err = {'g_motion': 0.0, 'g_traj': 0.0}
    for b, n in enumerate(lens):
        nw = pr.num_windows(n)
        err['g_motion'] = max(err['g_motion'], gc_rel(me.grad[b, :nw].cpu().numpy(), g['%s_s%d_g_motion' % (name, b)]))
        err['g_traj'] = max(err['g_traj'], gc_rel(te.grad[b].cpu().numpy(), g['%s_s%d_g_traj' % (name, b)]))
        assert (me.grad[b, nw:] == 0).all()
    print('joint loss through inference_grad, %s: d/d motion latent %.2e (bound %.2e), d/d traj latent %.2e (bound %.2e)'
          % (name, err['g_motion'], tol['g_motion'], err['g_traj'], tol['g_traj']))
    assert err['g_motion'] < tol['g_motion'] and err['g_traj'] < tol['g_traj']


def gc_rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


def test_refusals(priors):
    _, mt = priors
    batch, lens = _batch('one')
    with pytest.raises(NotImplementedError):
        mt.mfiller.infill(batch['in_body_pose'].clone().requires_grad_(True), batch['frame_mask'], batch['in_motion_latent'])
    for missing in ('in_motion_latent', 'in_traj_latent'):
        with pytest.raises(ValueError):
            mt.inference_grad({k: v for k, v in batch.items() if k != missing})
    with pytest.raises(ValueError):
        mt.inference_grad(dict(batch, pose=torch.zeros(1, lens[0], 72, device=DEV)))
    with pytest.raises(ValueError):
        mt.inference_grad(dict(batch, init_xy=torch.zeros(1, 2, device=DEV), init_heading=torch.zeros(1, device=DEV)))
    with pytest.raises(ValueError):
        mt.traj_predictor.local_traj(batch['in_body_pose'], batch['in_traj_latent'], in_body_pose=batch['in_body_pose'])
    torch.cuda.synchronize()
