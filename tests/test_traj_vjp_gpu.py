"""MI355X: the trajectory predictor's VJP (glamr_nets_traj_taped / glamr_nets_traj_backward) against the fp64 autograd reference of
tests/traj_vjp_common.py on the conditioned checkpoint: every route of the recurrence (one sequence per workgroup, the matrix-core kernel with
full, partial and ragged 16-sequence tiles, 300 steps), three upstream-gradient patterns, scaled gradients, bit-level repeatability, the
taped forward against glamr_nets_traj_clip bit for bit, and the autograd surface TrajPredVAE.local_traj.  Bounds: vc.TOL, 16 x the fp32 CPU
autograd's own error against fp64, relative to each sequence's largest reference entry."""
import ctypes
import numpy as np
import pytest
import torch

from tests import traj_vjp_common as vc
from tests.test_traj_pred_gpu import _handle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def handles(asset_root):
    hs = {'default': _handle(asset_root, False), 'fp32': _handle(asset_root, True)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope='module')
def ref(asset_root):
    return vc.Reference(asset_root)


def _batch(ref, seqs, pattern, scale=1.0):
    B, T = len(seqs), max(n for _, n in seqs)
    j, e, G = np.zeros((B, T, 69), np.float32), np.zeros((B, 128), np.float32), np.zeros((B, T, 11), np.float32)
    for b, (seed, n) in enumerate(seqs):
        j[b, :n], e[b] = ref.inputs(seed, n)
        G[b, :n] = vc.upstream(seed, n, pattern) * np.float32(scale)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(j), t(e), t(G), [n for _, n in seqs]


def _run(h, ref, seqs, pattern, scale=1.0):
    j, e, G, lens = _batch(ref, seqs, pattern, scale)
    out, tape = h.traj_taped(lens, e, in_joint_pos=j)
    ge, gj = h.traj_backward(tape, G)
    return out.cpu().numpy(), ge.cpu().numpy(), gj.cpu().numpy()


def _compare(got, seqs, ref, pattern, what, scale=1.0):
    """Every slot against its own fp64 product; rows past a sequence's end exactly zero."""
    _, ge, gj = got
    fails, worst = [], {'g_eps': 0.0, 'g_joint_pos': 0.0}
    assert np.isfinite(ge).all() and np.isfinite(gj).all(), '%s: non-finite gradient' % what
    for b, (seed, n) in enumerate(seqs):
        want = ref(seed, n)[pattern]
        for k, g, w in (('g_eps', ge[b], want[0]), ('g_joint_pos', gj[b, :n], want[1])):
            err = vc.rel_err(g / scale, w)
            worst[k] = max(worst[k], err)
            if not err <= vc.TOL[k]:
                fails.append('%s, slot %d (seed %d, length %d): %s off by %.2e of its largest entry (bound %.2e)' % (what, b, seed, n, k, err, vc.TOL[k]))
        if np.count_nonzero(gj[b, n:]):
            fails.append('%s, slot %d (length %d): g_joint_pos rows past the end are not zero' % (what, b, n))
    print('%s, %s: worst error vs fp64 g_eps %.2e (bound %.1e), g_joint_pos %.2e (bound %.1e)'
          % (what, pattern, worst['g_eps'], vc.TOL['g_eps'], worst['g_joint_pos'], vc.TOL['g_joint_pos']))
    assert not fails, fails[:10]


CASES = [('default', 'small', 1), ('default', 'small', 7), ('default', 'small', 33), ('default', 'mfma', 512), ('default', 'mfma', 523),
         ('default', 'long', 2), ('fp32', 'small', 7)]


@pytest.mark.parametrize('kind,route,B', CASES)
def test_vjp_matches_fp64_on_every_route(handles, ref, kind, route, B):
    """small: lstm_bwd_kernel (B = 33: 3300 rows, the split GEMMs and the fused forward rows); mfma: lstm_bwd_mfma_kernel, 512 = full tiles,
    523 = a partial last tile, lengths 2 ... 33 mixed inside every tile; long: 300 steps; fp32: a handle without fp16 planes."""
    seqs = vc.batch(route, B)
    for pattern in ('dense', 'last'):
        got = _run(handles[kind], ref, seqs, pattern)
        _compare(got, seqs, ref, pattern, '%s handle, %s B=%d' % (kind, route, B))
        if pattern == 'last':      # the gradient of the last frame's output reaches the joints of frame 0 (backward direction) and of the last frame
            for b, (seed, n) in enumerate(seqs[:16]):
                want = ref(seed, n)['last'][1]
                assert np.abs(want[0]).max() > 0 and np.abs(want[n - 1]).max() > 0
                assert np.abs(got[2][b, 0]).max() > 0 and np.abs(got[2][b, n - 1]).max() > 0
    _, ge, gj = _run(handles[kind], ref, seqs, 'pinned')
    assert not np.count_nonzero(ge) and not np.count_nonzero(gj), 'the pinned entries of row 0 must not contribute'


@pytest.mark.parametrize('route,B', [('small', 7), ('mfma', 523)])
@pytest.mark.parametrize('scale', [1e-6, 1e5])
def test_a_scaled_upstream_gradient_gives_the_scaled_result(handles, ref, route, B, scale):
    seqs = vc.batch(route, B)
    _compare(_run(handles['default'], ref, seqs, 'dense', scale), seqs, ref, 'dense', '%s B=%d, G x %g' % (route, B, scale), scale)


@pytest.mark.parametrize('route,B', [('small', 7), ('mfma', 523)])
def test_taped_forward_is_traj_clip_and_the_backward_repeats_bit_for_bit(handles, ref, route, B):
    h = handles['default']
    n = 33 if route == 'mfma' else 31
    seqs = [(seed, n) for seed, n_ in vc.batch(route, B)]          # traj_clip runs every sequence over the clip's length
    j = np.stack([ref.inputs(300 + b % 5, n)[0] for b in range(B)])
    e = np.stack([ref.inputs(seed, n_)[1] for seed, n_ in vc.batch(route, B)])
    j, e = torch.from_numpy(j).to(DEV), torch.from_numpy(e).to(DEV)
    clip = h.traj_clip(0, in_joint_pos=j, eps=e, want=())['out_local_traj'].cpu().numpy()
    out, tape = h.traj_taped([n] * B, e, in_joint_pos=j)
    assert np.array_equal(out.cpu().numpy(), clip)
    G = torch.from_numpy(np.random.default_rng(B).normal(size=(B, n, 11)).astype(np.float32)).to(DEV)
    a = [x.cpu().numpy() for x in h.traj_backward(tape, G)]
    b = [x.cpu().numpy() for x in h.traj_backward(tape, G)]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(seqs) == B


def test_local_traj_autograd_fills_both_grads(handles, ref, asset_root):
    from glamr_amd.models.prior_models import TrajPredVAE
    h = handles['default']
    seqs = vc.batch('small', 7)
    j, e, G, lens = _batch(ref, seqs, 'dense')
    m = TrajPredVAE.__new__(TrajPredVAE)
    m._handle = h
    jj, ee = j.clone().requires_grad_(True), e.clone().requires_grad_(True)
    out = m.local_traj(jj, ee, lens)
    (out * G).sum().backward()
    want_out, tape = h.traj_taped(lens, e, in_joint_pos=j)
    ge, gj = h.traj_backward(tape, G)
    assert out.shape == (7, 100, 11) and torch.equal(out.detach(), want_out)
    assert torch.equal(ee.grad, ge) and torch.equal(jj.grad, gj)


def test_body_pose_input_and_misuse_at_the_abi(handles, ref):
    """in_body_pose: joints by the FK kernel, g_joint_pos still the gradient w.r.t. the joint rows; both / neither input and a null tape
    return GLAMR_E_*, not a fault."""
    from glamr_amd import _lib
    from tests import traj_ref_common as tc
    h, L = handles['default'], _lib.lib()
    seqs = vc.batch('small', 7)
    j, e, G, lens = _batch(ref, seqs, 'dense')
    pose = np.zeros((7, 100, 69), np.float32)
    for b, (seed, n) in enumerate(seqs):
        pose[b, :n] = tc.seq_inputs(seed, n)[0]
    out, tape = h.traj_taped(lens, e, in_body_pose=torch.from_numpy(pose).to(DEV))
    got = (out.cpu().numpy(),) + tuple(x.cpu().numpy() for x in h.traj_backward(tape, G))
    _compare(got, seqs, ref, 'dense', 'in_body_pose B=7')
    ge_only, none = h.traj_backward(tape, G, want_joints=False)
    assert none is None and np.array_equal(ge_only.cpu().numpy(), got[1])
    lens_np = np.asarray(lens, np.int32)
    o = torch.empty((7, 100, 11), device=DEV)
    st = _lib.current_stream()
    args = lambda jp, bp, tp: (h.h, 7, 100, _lib.ptr(lens_np), jp, bp, _lib.ptr(e), _lib.ptr(o), tp, st)
    assert L.glamr_nets_traj_taped(*args(_lib.ptr(j), _lib.ptr(j), _lib.ptr(tape['buf']))) != 0
    assert L.glamr_nets_traj_taped(*args(None, None, _lib.ptr(tape['buf']))) != 0
    assert L.glamr_nets_traj_taped(*args(_lib.ptr(j), None, None)) != 0
    assert L.glamr_nets_traj_backward(h.h, 7, 100, _lib.ptr(lens_np), _lib.ptr(e), _lib.ptr(G), _lib.ptr(o), None, None, st) != 0
    assert L.glamr_nets_traj_tape_bytes(h.h, 0, 100) == 0
    torch.cuda.synchronize()
