"""MI355X: the infiller's VJP (glamr_nets_infill_backward, what the latent-optimisation mode differentiates every Adam iteration) against the
fp64 autograd reference of tests/nets_vjp_common.py -- at upstream-gradient scales far from the N(0,1) weights of the fixture tests, under
power-of-two rescaling bit for bit, at the batch sizes where the backward and the taped forward change kernels, at window edges and with
NaN in the padding.  Errors are max |got - ref| / max |ref| per sequence."""
import glob
import os
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from tests import infiller_ref_common as ic
from tests import nets_vjp_common as vc

pytestmark = pytest.mark.gpu

TOL = 5e-5                     # relative VJP error; ~10x what the s = 1 product achieves with the split-fp16 kernels
POSE_TOL = ic.TOL['shipped']['pose']      # taped forward pose, absolute: 16 x the fp32 port's own rounding (9.9e-7, tests/infiller_ref_common.py)
SCALES = [2.0 ** -30, 1e-6, 1e-3, 1.0, 1e3, 1e4, 1e5]
POW2 = [-30, -10, -1, 1, 10, 16]
EDGE_LENS = [11, 40, 41, 70, 71, 300]     # PAST + 1, one full window, one frame into the second, two windows, ..., ten windows


def _handle(asset_root, force_fp32):
    from glamr_amd import _lib
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(asset_root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    old = os.environ.pop('GLAMR_NETS_FORCE_FP32', None)           # read once, by glamr_nets_create
    try:
        if force_fp32:
            os.environ['GLAMR_NETS_FORCE_FP32'] = '1'
        h = MotionPriorsHandle(sd['inf'], sd['trj'], rest, synth.SMPL_PARENTS, torch.device('cuda:0'))
    finally:
        os.environ.pop('GLAMR_NETS_FORCE_FP32', None)
        if old is not None:
            os.environ['GLAMR_NETS_FORCE_FP32'] = old
    assert _lib.lib().glamr_nets_precision(h.h, None) == (1 if force_fp32 else 0)
    return h


@pytest.fixture(scope='module')
def handles(asset_root):
    hs = {'default': _handle(asset_root, False), 'fp32': _handle(asset_root, True)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope='module')
def ref(asset_root):
    return vc.Reference(asset_root)


def _taped(h, seqs):
    """Taped forward of the sequences (seed, length), zero padded to the longest: (pose (B,T,69) numpy, tape)."""
    dev = torch.device('cuda:0')
    B, T = len(seqs), max(n for _, n in seqs)
    pose, vis, eps = torch.zeros(B, T, 69), torch.zeros(B, T), torch.zeros(B, vc.n_windows(T), 128)
    for b, (seed, n) in enumerate(seqs):
        inp = mg.net_inputs(n, seed)
        pose[b, :n] = torch.from_numpy(inp['in_body_pose'][0])
        vis[b, :n] = torch.from_numpy(inp['frame_mask'][0]).float()
        eps[b, :vc.n_windows(n)] = torch.from_numpy(inp['in_motion_latent'])
    out, tape = h.infill_taped(pose.to(dev), vis.to(dev), [n for _, n in seqs], eps.to(dev))
    return out.cpu().numpy(), tape


def _bwd(h, tape, seqs, Gs, pad=0.0):
    """dL/d motion_eps (B, n_win_max, 128) numpy for the upstream gradients Gs[b] (length_b, 69); frames past a sequence's end hold `pad`."""
    G = torch.full((len(seqs), tape['T'], 69), pad)
    for b, ((_, n), g) in enumerate(zip(seqs, Gs)):
        G[b, :n] = torch.as_tensor(np.asarray(g, np.float32))
    return h.infill_backward(tape, G.to(torch.device('cuda:0'))).cpu().numpy()


def _check_seq(got, ref_grad, n, what, fails, tol=TOL):
    """One sequence's rows of a batched result: its own windows within `tol` of the reference (exactly zero where the reference is), the
    rows of windows it does not have exactly zero.  Returns the relative error."""
    nw = vc.n_windows(n)
    if not np.isfinite(got).all():
        fails.append('%s: non-finite VJP' % what)
        return float('nan')
    e = vc.rel_err(got[:nw], ref_grad)
    if not e < tol:
        fails.append('%s: relative error %.2e' % (what, e))
    if np.count_nonzero(got[:nw][ref_grad == 0]):
        fails.append('%s: %d entries non-zero where the reference is exactly zero' % (what, np.count_nonzero(got[:nw][ref_grad == 0])))
    if np.count_nonzero(got[nw:]):
        fails.append('%s: rows of windows past the sequence are not zero' % what)
    return e


@pytest.mark.parametrize('T', [120, 300])
def test_vjp_is_accurate_at_every_gradient_scale(handles, ref, T):
    """G = s W for s from 2^-30 to 1e5: gradients far below fp16's normal range and far above its largest number."""
    h = handles['default']
    W = mg.latent_loss_weights(T)
    _, g = ref(0, T, 'W', W)
    _, tape = _taped(h, [(0, T)])
    errs, fails = [], []
    for s in SCALES:
        got = _bwd(h, tape, [(0, T)], [(W.astype(np.float64) * s).astype(np.float32)])[0]
        errs.append(_check_seq(got, s * g, T, 's=%g' % s, fails))
    print('VJP vs fp64, T=%d, G = s W: %s' % (T, ', '.join('s=%g %.2e' % se for se in zip(SCALES, errs))))
    assert not fails, fails


@pytest.mark.parametrize('kind', ['default', 'fp32'])
def test_vjp_is_homogeneous_under_power_of_two_scaling(handles, kind):
    """grad(2^k G) == 2^k grad(G) bit for bit: exact for fp32 arithmetic and for any power-of-two pre-scaling taken from the operand; a
    product whose rounding depends on the gradient's magnitude fails it."""
    h = handles[kind]
    seqs = [(0, 120), (1, 83)]
    Ws = [mg.latent_loss_weights(n, seed) for seed, n in seqs]
    _, tape = _taped(h, seqs)
    base = _bwd(h, tape, seqs, Ws)
    assert np.isfinite(base).all() and np.abs(base).max() > 0
    bad = [k for k in POW2 if not np.array_equal(_bwd(h, tape, seqs, [np.ldexp(w, k) for w in Ws]), np.ldexp(base, k))]
    print('%s handle: grad(2^k G) == 2^k grad(G) bit for bit for k in %s, not for %s' % (kind, [k for k in POW2 if k not in bad], bad))
    assert not bad


def test_vjp_scales_each_sequence_of_a_batch_on_its_own(handles, ref):
    """Three sequences whose upstream gradients are 2^34 apart in one call: each within TOL of its own reference, relative to its own size."""
    h = handles['default']
    seqs, scales = [(0, 120), (1, 97), (2, 150)], [2.0 ** -20, 1.0, 2.0 ** 14]
    Ws = [mg.latent_loss_weights(n, seed) for seed, n in seqs]
    _, tape = _taped(h, seqs)
    got = _bwd(h, tape, seqs, [np.ldexp(w, int(np.log2(s))) for w, s in zip(Ws, scales)])
    fails = []
    errs = [_check_seq(got[b], s * ref(seed, n, 'W', W)[1], n, 'sequence %d (scale %g)' % (b, s), fails)
            for b, ((seed, n), s, W) in enumerate(zip(seqs, scales, Ws))]
    print('mixed scales in one batch: %s' % ', '.join('%g: %.2e' % se for se in zip(scales, errs)))
    assert not fails, fails


@pytest.mark.parametrize('kind,B', [('default', 1), ('default', 40), ('default', 41), ('default', 68), ('default', 69),
                                    ('fp32', 1), ('fp32', 41), ('fp32', 69)])
def test_vjp_and_taped_forward_on_every_route(handles, ref, kind, B):
    """Window rows 50 B and decoder rows 30 B cross SMALL_ROWS = 2048 at B = 41 and B = 69: there the backward products and the taped forward
    change kernels.  Every sequence (own seed, own length <= 150; vc.ROUTE_SEQS, every batch a prefix of it so that one fp64 product serves
    every batch size) against its own fp64 product."""
    h = handles[kind]
    seqs = vc.ROUTE_SEQS[:B]
    Ws = [mg.latent_loss_weights(n, seed) for seed, n in seqs]
    pose, tape = _taped(h, seqs)
    got = _bwd(h, tape, seqs, Ws)
    fails, ev, ep = [], 0.0, 0.0
    for b, ((seed, n), W) in enumerate(zip(seqs, Ws)):
        p_ref, g_ref = ref(seed, n, 'W', W)
        ev = max(ev, _check_seq(got[b], g_ref, n, 'sequence %d (length %d)' % (b, n), fails))
        e = float(np.abs(pose[b, :n] - p_ref).max())
        ep = max(ep, e)
        if not e < POSE_TOL:
            fails.append('sequence %d (length %d): taped pose %.2e from fp64' % (b, n, e))
    print('%s handle, B=%d: worst VJP relative error %.2e, worst taped pose error %.2e' % (kind, B, ev, ep))
    assert not fails, fails[:10]


def _edge_patterns(seqs):
    """Upstream-gradient patterns of the window-edge test: name -> (one G per sequence, what must be exactly zero)."""
    Ws = [mg.latent_loss_weights(n, seed) for seed, n in seqs]
    out = {}
    for i in (0, 1, 2, 3):
        lim = vc.PAST + vc.CUR * i                  # frames < lim depend on the latents of windows < i only
        out['frames<%d' % lim] = ([np.where(np.arange(n)[:, None] < lim, W, 0.0).astype(np.float32) for (_, n), W in zip(seqs, Ws)], i)
    last = []
    for b, (_, n) in enumerate(seqs):
        g = np.zeros((n, 69), np.float32)
        g[n - 1, (7 * b) % 69] = 1.0
        last.append(g)
    out['last frame'] = (last, None)
    return out


def test_vjp_window_edges_and_structural_zeros(handles, ref):
    """Lengths at every window edge in one ragged batch.  A gradient on the context frames the infiller copies through must give exactly
    zero; one on frames < 10 + 30 i must leave the latents of windows >= i exactly zero; a lone entry at the last frame reaches back."""
    h = handles['default']
    seqs = [(20 + b, n) for b, n in enumerate(EDGE_LENS)]
    _, tape = _taped(h, seqs)
    fails, report = [], []
    for name, (Gs, first_zero) in _edge_patterns(seqs).items():
        got = _bwd(h, tape, seqs, Gs)
        worst = 0.0
        for b, ((seed, n), G) in enumerate(zip(seqs, Gs)):
            g_ref = ref(seed, n, name, G)[1]
            if first_zero is not None:          # the reference's own structure: what this test relies on
                assert not g_ref[first_zero:].any() and (first_zero == 0 or g_ref[:first_zero].any())
            worst = max(worst, _check_seq(got[b], g_ref, n, '%s, length %d' % (name, n), fails))
        report.append('%s %.2e' % (name, worst))
    print('window edges %s: %s' % (EDGE_LENS, ', '.join(report)))
    assert not fails, fails


def test_vjp_padding_never_leaks(handles):
    """NaN in every upstream-gradient entry past a sequence's end: the result equals the zero-padded call bit for bit."""
    h = handles['default']
    seqs = [(20 + b, n) for b, n in enumerate(EDGE_LENS)]
    Ws = [mg.latent_loss_weights(n, seed) for seed, n in seqs]
    _, tape = _taped(h, seqs)
    zero = _bwd(h, tape, seqs, Ws)
    nan = _bwd(h, tape, seqs, Ws, pad=float('nan'))
    print('NaN padding: %d non-finite entries, %d differences from the zero-padded call' % ((~np.isfinite(nan)).sum(), (nan != zero).sum()))
    assert np.isfinite(zero).all() and np.array_equal(nan, zero)
