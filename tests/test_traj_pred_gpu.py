"""MI355X: the trajectory predictor against the fp64 port of tests/traj_ref_common.py, on the conditioned checkpoint (weights under which the
output depends on the input: a wrong recurrence, a wrong row or a wrong mean moves it by 20 tolerances or more, tests/test_traj_ref.py) and on
DISTINCT sequences in every slot -- every route of glamr_nets_infer(traj only), the three modes of glamr_nets_traj_clip,
glamr_traj_local_to_global on its own, and the infiller's large-batch kernels on distinct data.  Every sequence of every batch is compared
with its own fp64 result; tolerances are 16 x the fp32 CPU port's own rounding (tc.TOL, tc.CLIP_TOL, tc.L2G_TOL)."""
import glob
import os
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from tests import infiller_ref_common as ic
from tests import nets_vjp_common as vc
from tests import traj_ref_common as tc

pytestmark = pytest.mark.gpu

POSE_TOL = ic.TOL['shipped']['pose']      # infiller pose, absolute: 16 x the fp32 port's own rounding (9.9e-7, tests/infiller_ref_common.py)
MODES = {'infer': 0, 'train': 1, 'recon': 2}
CLIP_KEYS = {'local_traj': 'g2l', 'q_z': 'q_z', 'p_z': 'p_z', 'z': 'z', 'out_orig_local_traj': 'raw', 'out_local_traj': 'local_traj', 'out_trans': 'trans',
             'out_orient': 'orient', 'out_orient_q': 'quat'}


def _handle(asset_root, force_fp32):
    """Shipped infiller + CONDITIONED predictor; the default handle must keep the fp16-split kernels (a checkpoint that tips the range analysis
    into fp32-only mode would test nothing)."""
    from glamr_amd import _lib
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    path = sorted(glob.glob(os.path.join(asset_root, 'results', 'motion_filler/motion_infiller_demo', 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
    inf = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    old = os.environ.pop('GLAMR_NETS_FORCE_FP32', None)           # read once, by glamr_nets_create
    try:
        if force_fp32:
            os.environ['GLAMR_NETS_FORCE_FP32'] = '1'
        h = MotionPriorsHandle(inf, tc.load_state_dict(asset_root, conditioned=True), rest, synth.SMPL_PARENTS, torch.device('cuda:0'))
    finally:
        os.environ.pop('GLAMR_NETS_FORCE_FP32', None)
        if old is not None:
            os.environ['GLAMR_NETS_FORCE_FP32'] = old
    assert _lib.lib().glamr_nets_precision(h.h, None) == (1 if force_fp32 else 0)
    return h


@pytest.fixture(scope='module')
def handles(asset_root):
    hs = {'default': _handle(asset_root, False), 'fp32': _handle(asset_root, True)}
    print('conditioned checkpoint: worst-case converted activation %.0f, largest weight %.3f -> fp16-split kernels'
          % (hs['default'].precision_bound, hs['default'].largest_weight))
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope='module')
def ref(asset_root):
    return tc.Reference(asset_root)


def _inputs(seqs, pad=0.0):
    """Device inputs of the sequences (seed, length): pose (B,T,69) holding `pad` past each sequence's end, latent draws (B,128), lengths."""
    B, T = len(seqs), max(n for _, n in seqs)
    pose, eps = np.full((B, T, 69), pad, np.float32), np.zeros((B, 128), np.float32)
    for b, (seed, n) in enumerate(seqs):
        pose[b, :n], eps[b] = tc.seq_inputs(seed, n)
    dev = torch.device('cuda:0')
    return torch.from_numpy(pose).to(dev), torch.from_numpy(eps).to(dev), [n for _, n in seqs]


def _infer(h, seqs, pad=0.0, **kw):
    pose, eps, lens = _inputs(seqs, pad)
    out = h.infer(pose, None, lens, traj_eps=eps, infill=False, traj=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, seqs, ref, tol, what, fails, worst):
    """Every sequence of the batch against its own fp64 result; rows past its end exactly zero."""
    for b, (seed, n) in enumerate(seqs):
        got = {k: out[k][b] for k in ('local_traj', 'trans', 'orient')}
        if not all(np.isfinite(v).all() for v in got.values()):
            fails.append('%s, slot %d (seed %d, length %d): non-finite output' % (what, b, seed, n))
            continue
        for k, e in tc.errors(got, ref(seed, n), n).items():
            worst[k] = max(worst.get(k, 0.0), e)
            if not e <= tol[k]:
                fails.append('%s, slot %d (seed %d, length %d): %s off by %.2e (tolerance %.2e)' % (what, b, seed, n, k, e, tol[k]))
        if any(np.count_nonzero(v[n:]) for v in got.values()):
            fails.append('%s, slot %d (length %d): rows past the end are not zero' % (what, b, n))


ROUTES = [('default', B, max_len) for B, max_len in tc.ROUTE_BATCHES] + [('fp32', 1, None), ('fp32', 7, None), ('fp32', 523, None)]


@pytest.mark.parametrize('kind,B,max_len', ROUTES)
def test_every_sequence_on_every_route_matches_fp64(handles, ref, kind, B, max_len):
    """B = 1: lstm_kernel, gemm_small_kernel.  B = 7 with a 300-frame sequence: 2100 rows >= SMALL_ROWS, the split GEMM and the fused decoder
    rows.  B = 40 with every length <= 63: 2520 rows but max_len < 64, the fused decoder rows are off; B = 33 with max_len 64: the other side
    of that edge.  B = 511 / 512 / 523: lstm_mfma_kernel off / on / on with a partly empty last group of 16, EVERY slot checked."""
    seqs = tc.route_seqs(B, max_len)
    assert max(n for _, n in seqs) == (max_len or 300) and (max_len is None or B * max_len >= 2048)
    out = _infer(handles[kind], seqs)
    fails, worst = [], {}
    _check(out, seqs, ref, tc.TOL, 'B=%d' % B, fails, worst)
    print('%s handle, B=%d, max_len=%d: worst error vs fp64 %s (tolerances %s)' % (kind, B, max(n for _, n in seqs),
          ', '.join('%s %.2e' % kv for kv in sorted(worst.items())), ', '.join('%s %.1e' % (k, tc.TOL[k]) for k in sorted(worst))))
    assert not fails, fails[:10]


@pytest.mark.parametrize('B', [7, 523])
def test_padding_never_leaks(handles, B):
    """NaN in every body-pose entry past a sequence's end: the same bits as the zero-padded call, and zeros in the padded rows."""
    seqs = tc.tiling(B)
    zero, nan = _infer(handles['default'], seqs), _infer(handles['default'], seqs, pad=float('nan'))
    for k in zero:
        assert np.isfinite(zero[k]).all() and np.array_equal(zero[k], nan[k]), k
        for b, (_, n) in enumerate(seqs):
            assert not np.count_nonzero(zero[k][b, n:]), (k, b)


@pytest.mark.parametrize('B', [7, 523])
def test_a_permuted_batch_gives_every_slot_the_same_bits(handles, B):
    """Within one route a sequence's result does not depend on its slot or on its neighbours (the 15 others of its lstm_mfma_kernel group)."""
    seqs = tc.tiling(B)
    perm = np.random.default_rng(B).permutation(B)
    a, p = _infer(handles['default'], seqs), _infer(handles['default'], [seqs[i] for i in perm])
    bad = [(k, int(i)) for k in a for j, i in enumerate(perm) if not np.array_equal(p[k][j, :seqs[i][1]], a[k][i, :seqs[i][1]])]
    assert not bad, bad[:10]


def test_coschedule_flag_changes_nothing_without_the_infiller(handles):
    """The predictor always runs the LDS kernels (enqueue_infer): GLAMR_NETS_COSCHEDULE with the infiller off is the same call."""
    seqs = tc.tiling(48)
    a, c = _infer(handles['default'], seqs), _infer(handles['default'], seqs, coschedule=True)
    for k in a:
        assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize('B', [7, 523])
def test_the_replayed_graph_equals_the_plain_launches(handles, B):
    """On a stream of its own (the legacy default stream cannot be captured, glamr_nets_infer) the identical call -- same geometry, same
    buffers -- runs as plain launches the first time, is captured into a HIP graph and launched from it the second time and replayed the
    third: all three equal, bit for bit, a call with the same inputs on OTHER buffers, which the library has never seen and so launches
    plainly.  Every output is filled with NaN before each call: a replay has to write every entry again.  (The library keeps its graphs to
    itself; that the second and third calls are graph launches follows from its rule, not from an observation made here.)"""
    from glamr_amd import _lib
    h = handles['default']
    seqs = tc.tiling(B)
    dev = torch.device('cuda:0')
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        pose, eps, lens = _inputs(seqs)
        T = pose.shape[1]
        new = lambda: dict(local_traj=torch.empty(B, T, 11, device=dev), trans=torch.empty(B, T, 3, device=dev), orient=torch.empty(B, T, 3, device=dev),
                           ws=torch.empty(_lib.lib().glamr_nets_workspace_bytes(h.h, B, T), dtype=torch.uint8, device=dev), persistent=False)
        assert stream.cuda_stream != 0 and torch.cuda.current_stream(dev).cuda_stream == stream.cuda_stream
        first = new()                                   # kept alive: the allocator must not hand its addresses to `bufs`
        plain = {k: v.clone() for k, v in h.infer(pose, None, lens, traj_eps=eps, infill=False, traj=True, buffers=first).items()}
        bufs, runs = new(), []
        for _ in range(3):
            for k in ('local_traj', 'trans', 'orient'):
                bufs[k].fill_(float('nan'))
            out = h.infer(pose, None, lens, traj_eps=eps, infill=False, traj=True, buffers=bufs)
            runs.append({k: v.clone() for k, v in out.items()})
        stream.synchronize()
    for k in plain:
        assert torch.isfinite(plain[k]).all(), k
        for i, r in enumerate(runs):
            assert torch.equal(r[k], plain[k]), (k, 'call %d' % (i + 1))


# ---- glamr_nets_traj_clip: INFER, TRAIN, RECON -----------------------------------------------------------------------------------------------

def _clip(h, B, T, mode, valid_len=0):
    ins = [tc.clip_inputs(i, T) for i in range(B)]
    dev = torch.device('cuda:0')
    st = lambda j: torch.from_numpy(np.stack([x[j] for x in ins])).to(dev)
    out = h.traj_clip(MODES[mode], in_body_pose=st(0), trans=st(2), orient=st(3), eps=None if mode == 'recon' else st(1), valid_len=valid_len)
    return {CLIP_KEYS[k]: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('kind,B,T,valid_len', [('default', 2, 100, 0), ('default', 32, 100, 0), ('default', 523, 100, 0), ('default', 8, 300, 0),
                                                ('default', 2, 100, 70), ('default', 8, 300, 230), ('fp32', 32, 100, 0)])
def test_traj_clip_matches_fp64_in_every_mode(handles, ref, kind, B, T, valid_len):
    """Distinct clips with their own ground-truth root trajectory: global -> local rows, posterior, prior, the latent the decoder used, raw and
    first-row-pinned local rows, translation, orientation (as rotation matrices) and its quaternion (up to sign), per sequence.  B = 32:
    3200 rows, the split GEMM and fused decoder rows under the posterior encoder's two bi-LSTMs; B = 523: lstm_mfma_kernel.  valid_len < T:
    the joint rows of frames >= valid_len are zero and every network still runs over T frames (the chunk padding of the multi-step path)."""
    fails, report = [], []
    for mode in ('infer', 'train', 'recon'):
        got, want = _clip(handles[kind], B, T, mode, valid_len), ref.clip(B, T, mode, valid_len)
        assert ('q_z' in got) == (mode != 'infer') and set(want) <= set(got)
        worst = {}
        for b in range(B):
            for k, e in tc.errors({k: v[b] for k, v in got.items()}, {k: v[b] for k, v in want.items()}).items():
                worst[k] = max(worst.get(k, 0.0), e)
                if not e <= tc.CLIP_TOL[k]:
                    fails.append('%s, sequence %d: %s off by %.2e (tolerance %.2e)' % (mode, b, k, e, tc.CLIP_TOL[k]))
        report.append('%s: %s' % (mode, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    print('%s handle, traj_clip B=%d T=%d valid_len=%d, worst error vs fp64\n  %s' % (kind, B, T, valid_len, '\n  '.join(report)))
    assert not fails, fails[:10]


def test_traj_clip_on_the_sweep_exposes_prior_and_raw_rows(handles, ref):
    """The sweep's sequences, grouped by length, through traj_clip in INFER mode: the prior, the latent and the raw rows that glamr_nets_infer
    does not return, against the same cached fp64 results the route tests use."""
    dev = torch.device('cuda:0')
    fails, worst = [], {}
    for T in sorted(set(n for _, n in tc.SWEEP)):
        seqs = [s for s in tc.SWEEP if s[1] == T]
        pose, eps, _ = _inputs(seqs)
        out = handles['default'].traj_clip(MODES['infer'], in_body_pose=pose, eps=eps)
        got = {CLIP_KEYS[k]: v.cpu().numpy() for k, v in out.items()}
        for b, (seed, n) in enumerate(seqs):
            for k, e in tc.errors({k: v[b] for k, v in got.items()}, ref(seed, n)).items():
                worst[k] = max(worst.get(k, 0.0), e)
                if not e <= tc.TOL[k]:
                    fails.append('seed %d, length %d: %s off by %.2e (tolerance %.2e)' % (seed, n, k, e, tc.TOL[k]))
    print('traj_clip INFER on the sweep: worst error vs fp64 %s' % ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))
    assert {'p_z', 'z', 'raw', 'local_traj', 'trans', 'rot', 'quat'} <= set(worst) and not fails, fails[:10]


# ---- glamr_traj_local_to_global alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', sorted(tc.L2G_TOL))
def test_local_to_global_matches_fp64(T):
    """Headings that wrap past +-pi every few frames, rotations by pi (quaternion w ~ 0: the branch choice of rotmat_to_quat), 6D rows far
    from orthonormal.  T is not bounded by the header (the scans loop); 600 is twice the longest clip of the pipeline."""
    from glamr_amd.models.priors import local_to_global
    loc = tc.l2g_inputs(T)
    trans, orient, quat = local_to_global(torch.from_numpy(loc).to(torch.device('cuda:0')))
    got = {'trans': trans.cpu().numpy(), 'orient': orient.cpu().numpy(), 'quat': quat.cpu().numpy()}
    assert all(np.isfinite(v).all() for v in got.values())
    e = tc.errors(got, tc.local_to_global(loc))
    print('local_to_global, T=%d: %s (tolerances %s)' % (T, ', '.join('%s %.2e' % kv for kv in sorted(e.items())),
                                                          ', '.join('%s %.1e' % kv for kv in sorted(tc.L2G_TOL[T].items()))))
    assert all(e[k] <= tc.L2G_TOL[T][k] for k in e), e


# ---- the infiller's large-batch kernels on distinct data -------------------------------------------------------------------------------------

def test_infiller_on_distinct_sequences_plain_and_coscheduled(handles, asset_root):
    """69 sequences of their own seed and length (vc.ROUTE_SEQS): 3450 window rows, the fused and the co-schedulable fragment-major kernels,
    which the fixture tests reach with replicated sequences only -- a kernel that reads sequence j's rows for sequence i passes those."""
    dev = torch.device('cuda:0')
    seqs = vc.ROUTE_SEQS[:69]
    net = vc.Reference(asset_root).net
    B, T = len(seqs), max(n for _, n in seqs)
    pose, vis, eps = torch.zeros(B, T, 69), torch.zeros(B, T), torch.zeros(B, vc.n_windows(T), 128)
    want = []
    for b, (seed, n) in enumerate(seqs):
        inp = mg.net_inputs(n, seed)
        pose[b, :n] = torch.from_numpy(inp['in_body_pose'][0])
        vis[b, :n] = torch.from_numpy(inp['frame_mask'][0]).float()
        eps[b, :vc.n_windows(n)] = torch.from_numpy(inp['in_motion_latent'])
        with torch.no_grad():
            d = net.inference({'in_body_pose': torch.tensor(inp['in_body_pose'], dtype=torch.float64), 'frame_mask': torch.tensor(inp['frame_mask']),
                               'in_motion_latent': torch.tensor(inp['in_motion_latent'], dtype=torch.float64)}, sample_num=1, multi_step=True)
        want.append(d['infer_out_body_pose'][0, 0].numpy())
    fails = []
    for cos in (False, True):
        got = handles['default'].infer(pose.to(dev), vis.to(dev), [n for _, n in seqs], motion_eps=eps.to(dev), infill=True, traj=False,
                                       coschedule=cos)['pose'].cpu().numpy()
        errs = [float(np.abs(got[b, :n] - want[b]).max()) for b, (_, n) in enumerate(seqs)]
        fails += ['coschedule=%s, sequence %d (length %d): pose %.2e from fp64' % (cos, b, seqs[b][1], e) for b, e in enumerate(errs) if not e < POSE_TOL]
        fails += ['coschedule=%s, sequence %d: rows past the end are not zero' % (cos, b) for b, (_, n) in enumerate(seqs) if np.count_nonzero(got[b, n:])]
        print('infiller on 69 distinct sequences, coschedule=%s: worst pose error vs fp64 %.2e' % (cos, max(errs)))
    assert not fails, fails[:10]
