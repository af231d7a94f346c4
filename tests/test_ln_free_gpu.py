"""The co-schedulable LayerNorm (csrc/nn_free.hpp: ln_free_kernel, one wave per 16-row half of a 32-row fragment-major block, every value read
once) and the staging copies between caller rows and the padded pose buffer (csrc/nets.hip: pose_in_kernel, pose_out_kernel), through the C ABI.

The LayerNorm is reached at FEW rows -- where its partial blocks are -- through glamr_nets_infiller_window with GLAMR_NETS_FREE=1: windows have
50 rows per sequence, so 1, 2, 3 and 21 sequences give 50 = 32 + 16 + 2 rows (a half block with 2 live rows), 100 = 3 x 32 + 4 (an odd number of
halves), 150 = 4 x 32 + 16 + 6 and 1050 = 32 x 32 + 26 (both halves of the last block partial / live).  The prior's LayerNorms run on 2 rows per
sequence: 2, 4, 6 and 42 rows (one half with 2 live rows ... a whole block plus 10).

The staging copies are compared exactly with a NumPy re-statement of their indexing.  pose_in_kernel is reached at max_len 2, 31 and 300 through
glamr_nets_traj_clip; pose_out_kernel only runs inside glamr_nets_infer, which admits max_len > 10 and lengths > 10: its cases are max_len 11
(the smallest admitted, in place of 2), 31 and 300, with ragged lengths that include sequences shorter than one 50-frame window."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, PAST, CUR, XLD, NZ = 50, 10, 30, 96, 128


@pytest.fixture(scope='module')
def priors(asset_root):
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(asset_root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    return MotionPriorsHandle(sd['inf'], sd['trj'], rest, synth.SMPL_PARENTS, torch.device('cuda:0'))


def _tpad(max_len):
    """tpad_of (csrc/nets.hip): the pose buffer holds the last window of the longest possible sequence"""
    return max(max_len, (max(1, (max_len - PAST + CUR - 1) // CUR) - 1) * CUR + WIN)


def _window_inputs(B):
    g = torch.Generator().manual_seed(100 + B)
    dev = torch.device('cuda:0')
    pose = torch.randn(B, WIN, 69, generator=g) * 0.2
    mask = torch.ones(B, WIN)
    for b in range(B):                               # a different gap of invisible frames per sequence
        mask[b, 12 + b % 7:25 + b % 11] = 0
    return (pose * mask[:, :, None]).to(dev), mask.to(dev), torch.randn(B, NZ, generator=g).to(dev)


def _window(priors, B, ws, want_context=True):
    """glamr_nets_infiller_window (GLAMR_VAE_INFER) on the workspace `ws`; returns its outputs"""
    from glamr_amd import _lib
    from glamr_amd.models import priors as P
    L = _lib.lib()
    dev = torch.device('cuda:0')
    pose, mask, eps = _window_inputs(B)
    out = {'out_body_pose': torch.empty((B, CUR, 69), device=dev), 'p_z': torch.empty((B, 2, NZ), device=dev), 'z': torch.empty((B, NZ), device=dev)}
    if want_context:
        out['context'] = torch.empty((B, WIN, 256), device=dev)
    io = _lib.InfillerIO(_lib.ptr(pose), None, _lib.ptr(mask), _lib.ptr(eps), _lib.ptr(out.get('context')), None, _lib.ptr(out['p_z']), _lib.ptr(out['z']),
                         _lib.ptr(out['out_body_pose']))
    _lib.check(L.glamr_nets_infiller_window(priors.h, B, P.VAE_INFER, ctypes.byref(io), _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    return out


def _workspace(priors, B, T, seed=None):
    """a workspace of the call's size; seed: filled with finite random floats in [1, 2) (a poison no kernel can reproduce by accident)"""
    from glamr_amd import _lib
    n = _lib.lib().glamr_nets_workspace_bytes(priors.h, B, T)
    assert n % 4 == 0
    dev = torch.device('cuda:0')
    if seed is None:
        return torch.zeros(n, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(n // 4, generator=g, device=dev) + 1.0).view(torch.uint8)


@pytest.mark.parametrize('B', [1, 2, 3, 21])
def test_window_on_the_coschedulable_kernels_matches_the_lds_kernels(priors, monkeypatch, B):
    """The same window on the LDS kernels' path and on the co-schedulable kernels: every output within the 2e-5 tests/test_nets_gpu.py holds that
    comparison to (test_coschedulable_kernels_match_reference_at_batch_size).  The context is the second encoder layer's last LayerNorm as it stands;
    prior and output went through twelve more.  A poisoned workspace gives the same bits: no live row depends on a padded one."""
    monkeypatch.setenv('GLAMR_NETS_FREE', '0')
    lds = _window(priors, B, _workspace(priors, B, WIN))
    monkeypatch.setenv('GLAMR_NETS_FREE', '1')
    free = _window(priors, B, _workspace(priors, B, WIN))
    d = {k: float((free[k].double() - lds[k].double()).abs().max()) for k in lds}
    print('co-schedulable window, %d sequences (%d rows) vs the LDS kernels: %s' % (B, B * WIN, ', '.join('%s %.2e' % kv for kv in sorted(d.items()))))
    assert all(torch.isfinite(v).all() for v in free.values())
    assert max(d.values()) < 2e-5
    assert d['context'] > 0.0                        # (the other kernels did run: LayerNorm sums in a different order)
    poisoned = _window(priors, B, _workspace(priors, B, WIN, seed=7))
    for k in free:
        assert torch.equal(free[k], poisoned[k]), k


@pytest.mark.parametrize('B', [1, 2, 3, 21])
def test_padded_rows_of_the_fragment_major_buffers_stay_as_they_were(priors, monkeypatch, B):
    """Rows >= `rows` of a 32-row block are not written.  The window runs twice on workspaces poisoned with two different sets of finite random
    numbers: a byte that a kernel wrote from live data is the same after both runs, an untouched byte is its own poison, and anything
    else -- a padded row normalised and stored, say, which differs with the poison it was computed from -- fails."""
    monkeypatch.setenv('GLAMR_NETS_FREE', '1')
    p1, p2 = _workspace(priors, B, WIN, seed=11), _workspace(priors, B, WIN, seed=12)
    w1, w2 = p1.clone(), p2.clone()
    _window(priors, B, w1, want_context=False)
    _window(priors, B, w2, want_context=False)
    untouched = (w1 == p1) & (w2 == p2)             # byte by byte: the key mask is a byte array
    written = ~untouched
    print('co-schedulable window, %d sequences: %d bytes written, %d untouched' % (B, int(written.sum()), int(untouched.sum())))
    assert int(written.sum()) > B * WIN * 256 * 3    # (the call did run on these workspaces)
    bad = written & (w1 != w2)
    assert int(bad.sum()) == 0, 'first differing byte at %d' % int(torch.nonzero(bad)[0])
    # the activation buffers hold 32 spare rows and the encoder's blocks are partly padded: whole padded rows must have survived in them
    assert int(untouched.sum()) > 32 * 256 * 4


@pytest.mark.parametrize('max_len', [2, 31, 300])
def test_pose_in_is_the_padded_copy(priors, max_len):
    """pose_in_kernel: [B][max_len][69] -> [B][Tpad][96] at the start of the workspace, zero in the padding columns and in the frames past max_len
    (glamr_nets_traj_clip on in_body_pose; nothing else writes that buffer there)."""
    from glamr_amd import _lib
    from glamr_amd.models import priors as P
    L = _lib.lib()
    dev = torch.device('cuda:0')
    B = 5
    g = torch.Generator().manual_seed(max_len)
    body = (torch.randn(B, max_len, 69, generator=g) * 0.3).to(dev)
    eps = torch.randn(B, NZ, generator=g).to(dev)
    out = {k: torch.empty((B, max_len, 11), device=dev) for k in ('out_local_traj', 'out_orig_local_traj')}
    pz, z = torch.empty((B, 2 * NZ), device=dev), torch.empty((B, NZ), device=dev)
    io = _lib.TrajIO(_lib.ptr(body), None, None, None, _lib.ptr(eps), None, 0, None, None, _lib.ptr(pz), _lib.ptr(z), _lib.ptr(out['out_orig_local_traj']),
                     _lib.ptr(out['out_local_traj']), None, None, None)
    ws = _workspace(priors, B, max_len, seed=3)
    _lib.check(L.glamr_nets_traj_clip(priors.h, B, max_len, P.VAE_INFER, ctypes.byref(io), _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    Tpad = _tpad(max_len)
    got = ws.view(torch.float32)[:B * Tpad * XLD].view(B, Tpad, XLD).cpu().numpy()
    want = np.zeros((B, Tpad, XLD), dtype=np.float32)
    want[:, :max_len, :69] = body.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert torch.isfinite(out['out_local_traj']).all()


@pytest.mark.parametrize('max_len', [11, 31, 300])
def test_pose_out_is_the_masked_copy_of_the_pose_buffer(priors, max_len):
    """pose_out_kernel: out_pose[b][t][:] = the 69 columns of the pose buffer's row for t < lens[b], zero beyond (glamr_nets_infer, infiller only:
    the buffer at the start of the workspace is what the windows left).  Frames the infiller never generates (the first 10) and the padding of the
    buffer are pose_in_kernel's."""
    from glamr_amd import _lib
    from glamr_amd.models import priors as P
    L = _lib.lib()
    dev = torch.device('cuda:0')
    lens = {11: [11, 11, 11], 31: [31, 11, 20, 31, 17], 300: [300, 11, 37, 299, 64, 251]}[max_len]      # 11, 17, 20, 37: shorter than one window
    B = len(lens)
    g = torch.Generator().manual_seed(1000 + max_len)
    body = torch.randn(B, max_len, 69, generator=g) * 0.2
    vis = torch.ones(B, max_len)
    for b, n in enumerate(lens):
        vis[b, n:] = 0
        vis[b, 12:min(n, 12 + 9 * b)] = 0
    body = (body * vis[:, :, None]).to(dev)
    vis = vis.to(dev)
    n_win = P.num_windows(max_len)
    meps = torch.randn(B, n_win, NZ, generator=g).to(dev)
    out_pose = torch.full((B, max_len, 69), 7.0, device=dev)
    lens_np = np.ascontiguousarray(lens, dtype=np.int32)
    ws = _workspace(priors, B, max_len, seed=5)
    _lib.check(L.glamr_nets_infer(priors.h, B, max_len, _lib.ptr(lens_np), _lib.ptr(body), _lib.ptr(vis), _lib.ptr(meps), n_win, None, _lib.ptr(out_pose), None, None,
                                  None, P.NETS_INFILL, _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    Tpad = _tpad(max_len)
    buf = ws.view(torch.float32)[:B * Tpad * XLD].view(B, Tpad, XLD).cpu().numpy()
    want = np.zeros((B, max_len, 69), dtype=np.float32)
    for b, n in enumerate(lens):
        want[b, :n] = buf[b, :n, :69]
    got = out_pose.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    src = body.cpu().numpy()
    assert np.array_equal(buf[:, :PAST, :69].view(np.int32), src[:, :PAST].view(np.int32))
    assert not buf[:, :, 69:].any() and not buf[:, max_len:].any()
    for b, n in enumerate(lens):                     # the generated frames are there, and are not the input
        assert np.isfinite(got[b]).all() and not np.array_equal(got[b, PAST:n], src[b, PAST:n])
