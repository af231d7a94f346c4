"""MI355X: the motion infiller's forward against the fp64 reference of tests/infiller_ref_common.py, on the shipped synthetic checkpoint and
on the conditioned one (weights under which attention depends on the data, tests/test_infiller_ref.py), with DISTINCT data in every slot and
every slot compared with its own fp64 result: every kernel family glamr_nets_infer reaches through the three row counts B * 50, B * 32 and
B * 30 against SMALL_ROWS = 2048, the three modes of glamr_nets_infiller_window with every output they return, and the taped forward.
Tolerances are 16 x the fp32 CPU port's own rounding per output (ic.TOL); each test prints its worst error beside them."""
import contextlib
import os
import numpy as np
import pytest
import torch

from tests import infiller_ref_common as ic
from tests import traj_ref_common as tc

pytestmark = pytest.mark.gpu

MODES = {'infer': 0, 'train': 1, 'recon': 2}
WINDOW_KEYS = {'context': 'context', 'p_z': 'p_z', 'q_z': 'q_z', 'z': 'z', 'out_body_pose': 'pose'}


@contextlib.contextmanager
def _env(**kv):
    """Environment switches the library reads: GLAMR_NETS_FORCE_FP32 once, in glamr_nets_create; GLAMR_NETS_FREE at every call."""
    old = {k: os.environ.pop(k, None) for k in ('GLAMR_NETS_FORCE_FP32', 'GLAMR_NETS_FORCE_FP16', 'GLAMR_NETS_FREE')}
    try:
        os.environ.update({k: v for k, v in kv.items() if v is not None})
        yield
    finally:
        for k in old:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _handle(asset_root, ckpt, force_fp32):
    from glamr_amd import _lib
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    with _env(GLAMR_NETS_FORCE_FP32='1' if force_fp32 else None):
        h = MotionPriorsHandle(ic.load_state_dict(asset_root, ckpt == 'conditioned'), tc.load_state_dict(asset_root, conditioned=False), rest, synth.SMPL_PARENTS,
                               torch.device('cuda:0'))
    # a checkpoint that tips the range analysis into fp32-only mode would test none of the split kernels
    assert _lib.lib().glamr_nets_precision(h.h, None) == (1 if force_fp32 else 0), (ckpt, h.precision_bound, h.largest_weight)
    return h


@pytest.fixture(scope='module')
def handles(asset_root):
    hs = {(c, k): _handle(asset_root, c, k == 'fp32') for c in ic.CHECKPOINTS for k in ('default', 'fp32')}
    for c in ic.CHECKPOINTS:
        print('%s checkpoint: worst-case converted activation %.0f (infiller lines alone %.0f), largest weight %.3f -> fp16-split kernels'
              % (c, hs[(c, 'default')].precision_bound, ic.range_bound(ic.load_state_dict(asset_root, c == 'conditioned'))[0], hs[(c, 'default')].largest_weight))
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope='module')
def refs(asset_root):
    return {c: ic.Reference(asset_root, conditioned=c == 'conditioned') for c in ic.CHECKPOINTS}


def _batch(seqs, pad=0.0):
    """Device inputs of the sequences: pose (B,T,69) holding `pad` past each sequence's end, visible (B,T), latent draws (B,n_win,128), lengths."""
    B, T = len(seqs), max(s[1] for s in seqs)
    pose, vis, eps = np.full((B, T, 69), pad, np.float32), np.zeros((B, T), np.float32), np.zeros((B, ic.n_windows(T), 128), np.float32)
    for b, seq in enumerate(seqs):
        inp = ic.seq_inputs(*seq)
        pose[b, :seq[1]], vis[b, :seq[1]], eps[b, :ic.n_windows(seq[1])] = inp['pose'], inp['vis'], inp['eps']
    dev = torch.device('cuda:0')
    return torch.from_numpy(pose).to(dev), torch.from_numpy(vis).to(dev), torch.from_numpy(eps).to(dev), [s[1] for s in seqs]


def _infer(h, seqs, coschedule=False, pad=0.0):
    pose, vis, eps, lens = _batch(seqs, pad)
    with _env():
        return h.infer(pose, vis, lens, motion_eps=eps, infill=True, traj=False, coschedule=coschedule)['pose'].cpu().numpy()


def _check_pose(got, seqs, ref, tol, what):
    """Every slot against its own fp64 result; the first 10 frames are the input's bits; rows past the end exactly zero."""
    fails, worst = [], 0.0
    for b, seq in enumerate(seqs):
        n = seq[1]
        if not np.isfinite(got[b]).all():
            fails.append('%s, slot %d %s: non-finite output' % (what, b, seq))
            continue
        e = float(np.abs(got[b, :n] - ref.infer(seq)['pose']).max())
        worst = max(worst, e)
        if not e <= tol:
            fails.append('%s, slot %d %s: pose off by %.2e (tolerance %.2e)' % (what, b, seq, e, tol))
        if not np.array_equal(got[b, :ic.PAST].view(np.uint32), ic.seq_inputs(*seq)['pose'][:ic.PAST].view(np.uint32)):
            fails.append('%s, slot %d %s: the 10 past frames are not the input\'s bits' % (what, b, seq))
        if np.count_nonzero(got[b, n:]):
            fails.append('%s, slot %d %s: rows past the end are not zero' % (what, b, seq))
    return fails, worst


ROUTES = [('default', B, False) for B in ic.ROUTE_BATCHES] + [('default', B, True) for B in ic.ROUTE_BATCHES if B >= 41] + [('fp32', 1, False), ('fp32', 69, False)]


@pytest.mark.parametrize('kind,B,coschedule', ROUTES)
@pytest.mark.parametrize('ckpt', ic.CHECKPOINTS)
def test_every_slot_on_every_route_matches_fp64(handles, refs, ckpt, kind, B, coschedule):
    """glamr_nets_infer, infiller only.  B = 1 (a 300-frame sequence, ten windows) and 40: 2000 window rows, the small-M fp32 GEMMs and
    attention_mfma_kernel.  B = 41: 2050 encoder rows run the fused row-block / QKV-attention kernels, the decoder's 1230 rows do not.
    B = 68 / 69: 2040 / 2070 decoder rows, either side of the decoder's edge.  coschedule: the LDS-free kernels from B * 50 >= 2048 on.
    fp32: the handle of GLAMR_NETS_FORCE_FP32."""
    seqs = ic.route_seqs(B)
    assert len(seqs) == B and (B * ic.WIN >= ic.SMALL_ROWS) == (B >= 41) and (B * ic.CUR >= ic.SMALL_ROWS) == (B >= 69)
    tol = ic.TOL[ckpt]['pose']
    fails, worst = _check_pose(_infer(handles[(ckpt, kind)], seqs, coschedule), seqs, refs[ckpt], tol, 'B=%d' % B)
    print('%s checkpoint, %s handle, B=%d, coschedule=%s: worst pose error vs fp64 %.2e (tolerance %.2e)' % (ckpt, kind, B, coschedule, worst, tol))
    assert not fails, fails[:10]


def _window(h, seqs, mode, free):
    w = [ic.window_inputs(s) for s in seqs]
    dev = torch.device('cuda:0')
    st = lambda k: torch.from_numpy(np.stack([x[k] for x in w])).to(dev)
    with _env(GLAMR_NETS_FREE='1' if free else None):
        out = h.infiller_window(MODES[mode], st('in_body_pose'), st('frame_mask'), eps=None if mode == 'recon' else st('eps'),
                                body_pose=None if mode == 'infer' else st('body_pose'))
    return {WINDOW_KEYS[k]: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('kind,B', [('default', B) for B in ic.WINDOW_BATCHES] + [('fp32', 64)])
@pytest.mark.parametrize('ckpt', ic.CHECKPOINTS)
def test_window_matches_fp64_in_every_mode(handles, refs, ckpt, kind, B):
    """glamr_nets_infiller_window on window 0 of B distinct sequences, INFER, TRAIN and RECON: context, prior, posterior, the latent the
    decoder used and the 30 generated frames, per sequence.  B = 41: the encoder and the context projections are fused; 63 / 64: the
    posterior's B * 32 rows either side of 2048; 69: the decoder's B * 30.  Then the same with GLAMR_NETS_FREE=1: INFER runs the LDS-free
    kernels at any B and is held to the same bounds; TRAIN and RECON ignore the flag -- the same bits.

    The conditioned B = 64 and 69 cases are the ones that caught the fp16 split of Q and K in qkv_attention_kernel."""
    seqs = ic.ROUTE_SEQS[:B]
    tol, fails, report = ic.TOL[ckpt], [], []
    for mode in ('infer', 'train', 'recon'):
        want = refs[ckpt].windows(seqs, mode)
        plain, free = _window(handles[(ckpt, kind)], seqs, mode, False), _window(handles[(ckpt, kind)], seqs, mode, True)
        assert set(plain) == set(want[0]) and ('q_z' in plain) == (mode != 'infer')
        if mode != 'infer' or kind == 'fp32':
            fails += ['%s: GLAMR_NETS_FREE changed %s' % (mode, k) for k in plain if not np.array_equal(plain[k].view(np.uint32), free[k].view(np.uint32))]
        for name, got in (('plain', plain), ('free', free)):
            if name == 'free' and mode != 'infer':
                continue
            worst = {}
            for b in range(B):
                for k, e in ic.errors({k: v[b] for k, v in got.items()}, want[b]).items():
                    worst[k] = max(worst.get(k, 0.0), e)
                    if not e <= tol[k]:
                        fails.append('%s %s, slot %d %s: %s off by %.2e (tolerance %.2e)' % (mode, name, b, seqs[b], k, e, tol[k]))
            report.append('%s %s: %s' % (mode, name, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    print('%s checkpoint, %s handle, window B=%d, worst error vs fp64 (tolerances %s)\n  %s'
          % (ckpt, kind, B, ', '.join('%s %.1e' % kv for kv in sorted(tol.items())), '\n  '.join(report)))
    assert not fails, fails[:10]


@pytest.mark.parametrize('B', [1, 69])
@pytest.mark.parametrize('ckpt', ic.CHECKPOINTS)
def test_taped_forward_matches_fp64(handles, refs, ckpt, B):
    """glamr_nets_infill_taped keeps every activation: the separate kernels at every row count, the pose at the same bound."""
    seqs = ic.route_seqs(B)
    pose, vis, eps, lens = _batch(seqs)
    with _env():
        got = handles[(ckpt, 'default')].infill_taped(pose, vis, lens, eps)[0].cpu().numpy()
    tol = ic.TOL[ckpt]['pose']
    fails, worst = _check_pose(got, seqs, refs[ckpt], tol, 'taped B=%d' % B)
    print('%s checkpoint, taped forward, B=%d: worst pose error vs fp64 %.2e (tolerance %.2e)' % (ckpt, B, worst, tol))
    assert not fails, fails[:10]


@pytest.mark.parametrize('coschedule', [False, True])
def test_a_permuted_batch_gives_every_slot_the_same_bits(handles, coschedule):
    """Within one route a sequence's result does not depend on its slot or on its neighbours."""
    seqs = ic.ROUTE_SEQS
    perm = np.random.default_rng(69).permutation(len(seqs))
    h = handles[('conditioned', 'default')]
    a, p = _infer(h, seqs, coschedule), _infer(h, [seqs[i] for i in perm], coschedule)
    bad = [int(i) for j, i in enumerate(perm) if not np.array_equal(p[j, :seqs[i][1]].view(np.uint32), a[i, :seqs[i][1]].view(np.uint32))]
    assert not bad, bad[:10]


@pytest.mark.parametrize('coschedule', [False, True])
def test_padding_never_leaks(handles, coschedule):
    """NaN in every body-pose entry past a sequence's end: the same bits as the zero-padded call."""
    h = handles[('conditioned', 'default')]
    zero, nan = _infer(h, ic.ROUTE_SEQS, coschedule), _infer(h, ic.ROUTE_SEQS, coschedule, pad=float('nan'))
    assert np.isfinite(zero).all() and np.array_equal(zero.view(np.uint32), nan.view(np.uint32))
