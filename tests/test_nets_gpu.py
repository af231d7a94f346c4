"""MI355X parity of the motion-prior kernels (glamr_nets_infer through the C ABI): infiller + trajectory predictor outputs vs
fixtures produced by the UNMODIFIED reference with the same supplied latents.  Tolerance 1e-4 (BASELINE.json / SURVEY.md 8c)."""
import glob
import os
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from oracle.port import build

pytestmark = pytest.mark.gpu


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


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.mark.parametrize('T', [120, 300])
def test_joint_inference_matches_reference(priors, golden, T):
    g = golden('nets')
    dev = torch.device('cuda:0')
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    out = priors.infer(b['in_body_pose'], b['frame_mask'], [T], motion_eps=b['in_motion_latent'][None], traj_eps=b['in_traj_latent'])
    e = (_err(out['pose'][0].cpu(), g['T%d_body_pose' % T][0, 0]), _err(out['local_traj'][0].cpu(), g['T%d_local_traj' % T][:, 0, 0]),
         _err(out['trans'][0].cpu(), g['T%d_trans' % T][0, 0]), _err(out['orient'][0].cpu(), g['T%d_orient' % T][0, 0]))
    print('priors vs reference, T=%d: body pose %.2e, local trajectory %.2e, translation %.2e, orientation %.2e' % ((T,) + e))
    assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 2e-4 and e[3] < 2e-4


def test_single_padded_window(priors, golden):
    g = golden('nets')
    dev = torch.device('cuda:0')
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(40).items()}
    out = priors.infer(b['in_body_pose'], b['frame_mask'], [40], motion_eps=b['in_motion_latent'][None], traj_eps=None, traj=False)
    assert _err(out['pose'][0].cpu(), g['T40_body_pose'][0, 0]) < 1e-4


def test_ragged_batch_equals_single_runs(priors):
    """Sequences of different lengths in one padded batch must give what each gives alone (padding never leaks)."""
    dev = torch.device('cuda:0')
    lens = [300, 47, 120, 211]
    T = max(lens)
    ins = [mg.net_inputs(n, seed=i) for i, n in enumerate(lens)]
    pose = torch.zeros(len(lens), T, 69, device=dev)
    vis = torch.zeros(len(lens), T, device=dev)
    nw = max(x['in_motion_latent'].shape[0] for x in ins)
    meps = torch.zeros(len(lens), nw, 128, device=dev)
    teps = torch.zeros(len(lens), 128, device=dev)
    for i, x in enumerate(ins):
        pose[i, :lens[i]] = torch.tensor(x['in_body_pose'][0])
        vis[i, :lens[i]] = torch.tensor(x['frame_mask'][0]).float()
        meps[i, :x['in_motion_latent'].shape[0]] = torch.tensor(x['in_motion_latent'])
        teps[i] = torch.tensor(x['in_traj_latent'][0])
    batch = priors.infer(pose, vis, lens, motion_eps=meps, traj_eps=teps)
    for i, x in enumerate(ins):
        n = lens[i]
        single = priors.infer(pose[i:i + 1, :n].contiguous(), vis[i:i + 1, :n].contiguous(), [n], motion_eps=meps[i:i + 1], traj_eps=teps[i:i + 1])
        for key in ('pose', 'local_traj', 'trans', 'orient'):
            assert _err(batch[key][i, :n].cpu(), single[key][0].cpu()) < 1e-5, (i, key)
            assert float(batch[key][i, n:].abs().max()) == 0.0 if n < T else True


def test_large_batch_recurrence_equals_small_batch(priors):
    """Batches of 512+ sequences run the bi-LSTM on the matrix cores (16 sequences per workgroup, lstm_mfma_kernel); smaller ones
    one sequence per workgroup.  Same numbers up to the summation order of the recurrent product."""
    dev = torch.device('cuda:0')
    base = [97, 47, 120, 64, 11, 100]
    B = 523                                          # not a multiple of 16: the last workgroup is partly empty
    lens = [base[i % len(base)] for i in range(B)]
    T = max(lens)
    ins = [mg.net_inputs(n, seed=i) for i, n in enumerate(base)]
    pose = torch.zeros(B, T, 69, device=dev)
    vis = torch.zeros(B, T, device=dev)
    nw = max(x['in_motion_latent'].shape[0] for x in ins)
    meps = torch.zeros(B, nw, 128, device=dev)
    teps = torch.zeros(B, 128, device=dev)
    for i in range(B):
        x = ins[i % len(base)]
        pose[i, :lens[i]] = torch.tensor(x['in_body_pose'][0])
        vis[i, :lens[i]] = torch.tensor(x['frame_mask'][0]).float()
        meps[i, :x['in_motion_latent'].shape[0]] = torch.tensor(x['in_motion_latent'])
        teps[i] = torch.tensor(x['in_traj_latent'][0])
    big = priors.infer(pose, vis, lens, motion_eps=meps, traj_eps=teps)
    small = priors.infer(pose[:len(base)].contiguous(), vis[:len(base)].contiguous(), lens[:len(base)], motion_eps=meps[:len(base)].contiguous(),
                         traj_eps=teps[:len(base)].contiguous())
    for i in (0, 1, 5, 7, 300, 517, 522):
        j, n = i % len(base), lens[i]
        for key in ('local_traj', 'trans', 'orient', 'pose'):
            assert _err(big[key][i, :n].cpu(), small[key][j, :n].cpu()) < 2e-5, (i, key)


# ---- training-mode forward(data) and inference(recon=True) of the drop-in classes ---------------------------------------------------

@pytest.fixture(scope='module')
def joint_model(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    dev = torch.device('cuda:0')
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(dev)
    mt = MotionTrajJointModel(None, dev, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))
    mt.mfiller.noise_device = mt.traj_predictor.noise_device = 'cpu'      # the fixtures were drawn by the reference on the CPU generator
    return mt


def _close(got, ref, tol, what):
    e = _err(got.detach().cpu() if torch.is_tensor(got) else got, ref)
    assert e < tol, '%s: %.3g' % (what, e)


def _quat_close(got, ref, tol, what):
    q = got.detach().cpu().numpy()
    assert np.minimum(np.abs(q - ref), np.abs(q + ref)).max() < tol, what


def test_infiller_forward_and_recon_match_reference(joint_model, golden):
    """MotionInfillerVAE.forward(data) (motion_infiller_vae.py:478-482) and the one-shot inference(recon=True) (:659-666) on the device,
    against the unmodified reference (tests/golden/nets_train.npz), every key the CPU restatement is held to, 1e-4."""
    g = golden('nets_train')
    x = mg.train_inputs()['infiller']
    inf = joint_model.mfiller
    d = inf.init_batch_data({k: torch.tensor(v) for k, v in x.items()})
    torch.manual_seed(1234)
    d = inf.forward(d)
    for k in ('q_z_dist', 'p_z_dist'):
        _close(d[k].mu, g['inf_%s_mu' % k], 1e-4, k + ' mu')
        _close(d[k].logvar, g['inf_%s_logvar' % k], 1e-4, k + ' logvar')
    _close(d['context'], g['inf_context'], 1e-4, 'context')
    _close(d['q_z_samp'], g['inf_q_z_samp'], 1e-4, 'posterior sample')
    _close(d['train_out_body_pose_tp'], g['inf_train_out_body_pose_tp'], 1e-4, 'train output')
    _close(d['train_out_pose_tp'], g['inf_train_out_pose_tp'], 1e-4, 'train output with root')
    assert inf(inf.init_batch_data({k: torch.tensor(v) for k, v in x.items()}))['train_out_pose_tp'].shape == (40, 2, 72)      # __call__ = forward
    d = inf.inference({k: torch.tensor(v) for k, v in x.items()}, sample_num=3, recon=True, multi_step=False)
    _close(d['recon_out_body_pose'], g['inf_recon_out_body_pose'], 1e-4, 'reconstruction')
    assert d['infer_out_body_pose'].shape == (2, 3, 40, 69) and d['infer_out_pose'].shape == (2, 3, 40, 72)
    assert d['pose'].shape == (2, 40, 72) and d['trans'].shape == (2, 40, 3)                  # the future frames are cut (:664-666)
    assert torch.equal(d['infer_out_body_pose'][:, 0, :10], torch.tensor(x['pose'][:, :10, 3:] * x['pose_mask'][:, :10, 3:]).to(d['infer_out_body_pose'].device))


def test_trajectory_forward_and_recon_match_reference(joint_model, golden):
    """TrajPredVAE.forward(data) (traj_pred_vae.py:378-382) and inference(recon=True) (:537-548) on the device vs the reference."""
    g = golden('nets_train')
    x = mg.train_inputs()['traj']
    trj = joint_model.traj_predictor
    d = trj.init_batch_data({k: torch.tensor(v) for k, v in x.items()})
    torch.manual_seed(4321)
    d = trj.forward(d)
    _close(d['local_traj_tp'], g['trj_local_traj_tp'], 1e-4, 'global -> local trajectory')
    for k in ('q_z_dist', 'p_z_dist'):
        _close(d[k].mu, g['trj_%s_mu' % k], 1e-4, k + ' mu')
        _close(d[k].logvar, g['trj_%s_logvar' % k], 1e-4, k + ' logvar')
    _close(d['q_z_samp'], g['trj_q_z_samp'], 1e-4, 'posterior sample')
    _close(d['train_out_local_traj_tp'], g['trj_train_out_local_traj_tp'], 1e-4, 'train output (local)')
    _close(d['train_out_trans_tp'], g['trj_train_out_trans_tp'], 2e-4, 'train output (translation)')
    _quat_close(d['train_out_orient_q_tp'], g['trj_train_out_orient_q_tp'], 2e-4, 'train output (orientation, up to the quaternion sign)')
    d = trj.inference({k: torch.tensor(v) for k, v in x.items()}, sample_num=2, recon=True)
    _close(d['recon_out_local_traj_tp'], g['trj_recon_out_local_traj_tp'], 1e-4, 'reconstruction (local)')
    _close(d['recon_out_trans'], g['trj_recon_out_trans'], 2e-4, 'reconstruction (translation)')
    from tests.grecon_common import _rot_err
    assert _rot_err(d['recon_out_orient'].cpu().numpy(), g['trj_recon_out_orient']) < 2e-4
    assert d['infer_out_trans'].shape == (2, 2, 100, 3) and d['infer_out_local_traj_tp'].shape == (100, 2, 2, 11)


def test_multi_step_paths_with_reconstruction_match_reference(joint_model, golden):
    """Chunked trajectory inference (traj_pred_vae.py:498-519: 130 frames = a full chunk + a zero-padded one, heading carried over),
    sliding-window reconstruction of the infiller (motion_infiller_vae.py:589-632) and the joint model with recon=True
    (motion_traj_joint_model.py:73-145, incl. init_xy / init_heading) vs the reference."""
    from tests.grecon_common import _rot_err
    g = golden('nets_train')
    y = mg.multi_step_inputs()
    tt = lambda dct: {k: torch.tensor(v) for k, v in dct.items()}
    d = joint_model.traj_predictor.inference(tt(y['traj']), sample_num=1, recon=True, multi_step=True)
    # (the sampled outputs cannot be compared: get_seg_data :487-496 copies only '*tp*' keys into a chunk, so the reference ignores a
    #  supplied in_traj_latent there and draws from torch's generator)
    assert d['infer_out_local_traj_tp'].shape == g['trjms_infer_out_local_traj_tp'].shape and d['infer_out_trans'].shape == g['trjms_infer_out_trans'].shape
    assert torch.isfinite(d['infer_out_trans']).all()
    _close(d['recon_out_local_traj_tp'], g['trjms_recon_out_local_traj_tp'], 1e-4, 'chunked reconstruction: local rows')
    _close(d['recon_out_trans'], g['trjms_recon_out_trans'], 3e-4, 'chunked reconstruction: translation')
    assert _rot_err(d['recon_out_orient'].cpu().numpy(), g['trjms_recon_out_orient']) < 3e-4
    d = joint_model.mfiller.inference(tt(y['infiller']), sample_num=1, recon=True, multi_step=True)
    _close(d['infer_out_body_pose'], g['infms_infer_out_body_pose'], 1e-4, 'sliding windows: samples')
    _close(d['recon_out_body_pose'], g['infms_recon_out_body_pose'], 1e-4, 'sliding windows: reconstruction')
    _close(d['recon_out_pose'], g['infms_recon_out_pose'], 1e-4, 'sliding windows: reconstruction with root')
    d = joint_model.inference(tt(y['joint']), sample_num=2, recon=True)
    for k, tol in (('infer_out_body_pose', 1e-4), ('infer_out_trans', 3e-4), ('infer_out_local_traj_tp', 1e-4), ('recon_out_body_pose', 1e-4),
                   ('recon_out_trans', 3e-4), ('recon_out_local_traj_tp', 1e-4)):
        _close(d[k], g['joint_' + k], tol, 'joint model ' + k)
    assert _rot_err(d['infer_out_orient'].cpu().numpy(), g['joint_infer_out_orient']) < 3e-4
    assert _rot_err(d['recon_out_orient'].cpu().numpy(), g['joint_recon_out_orient']) < 3e-4


def test_split_gemm_path_matches_reference_at_batch_size(priors, golden):
    """Tall activations (M >= 2048 rows) take the fp16-split MFMA GEMM (nn_kernels.hpp gemm_split_kernel: fp32 results from three
    v_mfma_f32_32x32x16_f16 per k step); a single sequence takes the plain fp32 MFMA kernel.  The same sequence replicated 64 times must
    still match the unmodified reference to 1e-4 -- and the small-batch kernel to a few 1e-6."""
    g = golden('nets')
    dev = torch.device('cuda:0')
    T, B = 300, 64
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    one = priors.infer(b['in_body_pose'], b['frame_mask'], [T], motion_eps=b['in_motion_latent'][None], traj_eps=b['in_traj_latent'])
    rep = lambda t: t.expand(B, *t.shape[1:]).contiguous()
    out = priors.infer(rep(b['in_body_pose']), rep(b['frame_mask']), [T] * B, motion_eps=rep(b['in_motion_latent'][None]), traj_eps=rep(b['in_traj_latent']))
    e = (_err(out['pose'][B - 1].cpu(), g['T300_body_pose'][0, 0]), _err(out['local_traj'][B - 1].cpu(), g['T300_local_traj'][:, 0, 0]),
         _err(out['trans'][B - 1].cpu(), g['T300_trans'][0, 0]), _err(out['orient'][B - 1].cpu(), g['T300_orient'][0, 0]))
    d = max(_err(out[k][B - 1].cpu(), one[k][0].cpu()) for k in ('pose', 'local_traj', 'trans', 'orient'))
    print('split GEMM (batch %d) vs reference: body pose %.2e, local trajectory %.2e, translation %.2e, orientation %.2e; vs the fp32 MFMA kernel %.2e' % ((B,) + e + (d,)))
    assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 2e-4 and e[3] < 2e-4
    assert torch.equal(out['pose'][0], out['pose'][B - 1])          # and every copy of the sequence gets the same bits


def test_coschedulable_kernels_match_reference_at_batch_size(priors, golden):
    """GLAMR_NETS_COSCHEDULE (infer(..., coschedule=True)): the infiller on the kernels that fit beside a resident optimiser-stage workgroup --
    no LDS, one wave per workgroup, fragment-major activations (csrc/nn_free.hpp: gemm_free_kernel, ln_free_kernel, attention_free_kernel).
    64 copies of the reference sequence (a ragged tail included: 64 x 50 and 64 x 30 window rows, 3200 = 100 whole 32-row blocks, so a second
    batch of 41 sequences covers the partial last block) must match the unmodified reference to 1e-4 and the LDS kernels to a few 1e-6."""
    g = golden('nets')
    dev = torch.device('cuda:0')
    T = 300
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    rep = lambda t, B: t.expand(B, *t.shape[1:]).contiguous()
    for B in (64, 41):
        args = (rep(b['in_body_pose'], B), rep(b['frame_mask'], B), [T] * B)
        kw = dict(motion_eps=rep(b['in_motion_latent'][None], B), traj_eps=rep(b['in_traj_latent'], B))
        lds = priors.infer(*args, **kw)
        out = priors.infer(*args, coschedule=True, **kw)
        e = (_err(out['pose'][B - 1].cpu(), g['T300_body_pose'][0, 0]), _err(out['local_traj'][B - 1].cpu(), g['T300_local_traj'][:, 0, 0]),
             _err(out['trans'][B - 1].cpu(), g['T300_trans'][0, 0]), _err(out['orient'][B - 1].cpu(), g['T300_orient'][0, 0]))
        d = max(_err(out[k].cpu(), lds[k].cpu()) for k in ('pose', 'local_traj', 'trans', 'orient'))
        print('co-schedulable kernels (batch %d) vs reference: body pose %.2e, local trajectory %.2e, translation %.2e, orientation %.2e; vs the LDS kernels %.2e' % ((B,) + e + (d,)))
        assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 2e-4 and e[3] < 2e-4 and d < 2e-5
        assert d > 0.0                                               # (the other kernels did run: LayerNorm sums in a different order)
        assert torch.equal(out['pose'][0], out['pose'][B - 1])
    # ragged lengths: every sequence as if alone
    lens = [300, 251, 40, 133] * 12
    Bn = len(lens)
    pose = rep(b['in_body_pose'], Bn).clone()
    vis = rep(b['frame_mask'], Bn).clone()
    for i, n in enumerate(lens):
        pose[i, n:] = 0
        vis[i, n:] = 0
    kw = dict(motion_eps=rep(b['in_motion_latent'][None], Bn), traj_eps=rep(b['in_traj_latent'], Bn))
    lds = priors.infer(pose, vis, lens, **kw)
    out = priors.infer(pose, vis, lens, coschedule=True, **kw)
    d = max(_err(out[k].cpu(), lds[k].cpu()) for k in ('pose', 'local_traj', 'trans', 'orient'))
    print('co-schedulable kernels, ragged batch of %d: vs the LDS kernels %.2e' % (Bn, d))
    assert d < 2e-5


def test_fused_layer_kernels_match_reference_at_batch_size(joint_model, golden):
    """At M >= 2048 rows the transformer blocks run as fused kernels (qkv_attention_kernel: projections + attention with Q / K / V in
    registers; rows_fused_kernel: out-projection + residual + LayerNorm, feed-forward with the hidden rows on chip).  The training-mode pass
    of the infiller on the two reference windows replicated to 64 sequences must reproduce the reference's context, posterior, prior, sample
    and output -- quantities that go through every fused block (encoder self-attention, decoder self- and cross-attention) -- to 1e-4."""
    g = golden('nets_train')
    x = mg.train_inputs()['infiller']
    rep = {k: torch.tensor(np.concatenate([v] * 32, axis=0)) for k, v in x.items()}
    inf = joint_model.mfiller
    d = inf.init_batch_data(rep)
    torch.manual_seed(1234)
    eps2 = torch.randn((2, 128))                                 # the reference drew (2, 128) under this seed
    d = inf._window_pass(d, 1, eps=eps2.repeat(32, 1).to(inf.device))
    for i in (0, 1, 62, 63):
        j = i % 2
        for k in ('q_z_dist', 'p_z_dist'):
            _close(d[k].mu[i], g['inf_%s_mu' % k][j], 1e-4, k + ' mu')
            _close(d[k].logvar[i], g['inf_%s_logvar' % k][j], 1e-4, k + ' logvar')
        _close(d['context'][:, i], g['inf_context'][:, j], 1e-4, 'context')
        _close(d['q_z_samp'][i], g['inf_q_z_samp'][j], 1e-4, 'posterior sample')
        _close(d['train_out_body_pose_tp'][:, i], g['inf_train_out_body_pose_tp'][:, j], 1e-4, 'train output')
    e = max(_err(d['context'][:, i].cpu(), g['inf_context'][:, i % 2]) for i in range(64))
    print('fused layers, 64 windows: context vs reference %.2e' % e)


def test_handle_close_releases_device_memory(asset_root, priors):
    """glamr_nets_destroy frees the weights (two fp16 planes + the fp32 copy of every layer) and the captured launch graphs of a
    handle: creating, using and closing handles repeatedly must not grow the device footprint, and the surviving handle still works."""
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(asset_root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    dev = torch.device('cuda:0')
    from glamr_amd.models.priors import num_windows, NZ
    pose = torch.zeros((2, 120, 69), device=dev)
    vis = torch.ones((2, 120), device=dev)
    meps = torch.zeros((2, num_windows(120), NZ), device=dev)
    teps = torch.zeros((2, NZ), device=dev)

    def cycle():
        h = MotionPriorsHandle(sd['inf'], sd['trj'], rest, synth.SMPL_PARENTS, dev)
        out = h.infer(pose, vis, [120, 120], motion_eps=meps, traj_eps=teps)
        assert torch.isfinite(out['pose']).all()
        h.close()
        assert h.h is None
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    assert free0 - free1 < 8 << 20, 'three create / close cycles kept %.1f MB' % ((free0 - free1) / 2**20)
    assert torch.isfinite(priors.infer(pose, vis, [120, 120], motion_eps=meps, traj_eps=teps)['pose']).all()


@pytest.mark.parametrize('T', [120, 300])
def test_infiller_gradient_wrt_the_latent_matches_reference_autograd(priors, golden, T):
    """The infiller INSIDE an optimisation loop (latent-optimisation mode, global_recon_model.py:434-437): glamr_nets_infill_taped reproduces
    the inference output, and glamr_nets_infill_backward the gradient torch autograd gives for `in_motion_latent` through every window's
    decoder, reparameterisation, prior and context encoder and through the autoregression between windows -- against the unmodified
    reference (tests/golden/nets_latent.npz; L = sum(W * infer_out_body_pose))."""
    g = golden('nets_latent')
    dev = torch.device('cuda:0')
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    eps = b['in_motion_latent'][None]
    pose, tape = priors.infill_taped(b['in_body_pose'], b['frame_mask'], [T], eps)
    plain = priors.infer(b['in_body_pose'], b['frame_mask'], [T], motion_eps=eps, traj_eps=None, traj=False)['pose']
    assert _err(pose.cpu(), plain.cpu()) < 2e-5                                   # same network, unfused launch sequence
    assert _err(pose[0].cpu(), g['T%d_body_pose' % T]) < 1e-4
    W = torch.tensor(mg.latent_loss_weights(T), device=dev)[None]
    grad = priors.infill_backward(tape, W)[0].cpu().numpy()
    ref = g['T%d_grad_latent' % T]
    err = np.abs(grad - ref).max()
    print('d/d motion_latent, T=%d (%d windows): max abs err %.2e (largest gradient %.3f)' % (T, ref.shape[0], err, np.abs(ref).max()))
    assert grad.shape == ref.shape and err < 2e-4 * max(1.0, np.abs(ref).max())
    # two different sequences in one batch: each gets the gradient it gets alone
    b2 = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T - 37, seed=1).items()}
    pose_in = torch.zeros(2, T, 69, device=dev)
    vis = torch.zeros(2, T, device=dev)
    pose_in[0], vis[0] = b['in_body_pose'][0], b['frame_mask'][0]
    pose_in[1, :T - 37], vis[1, :T - 37] = b2['in_body_pose'][0], b2['frame_mask'][0]
    eps2 = torch.zeros(2, eps.shape[1], 128, device=dev)
    eps2[0] = eps[0]
    eps2[1, :b2['in_motion_latent'].shape[0]] = b2['in_motion_latent']
    _, tape2 = priors.infill_taped(pose_in, vis, [T, T - 37], eps2)
    W2 = torch.zeros(2, T, 69, device=dev)
    W2[0] = W[0]
    W2[1, :T - 37] = W[0, :T - 37]
    both = priors.infill_backward(tape2, W2).cpu().numpy()
    assert np.abs(both[0] - grad).max() < 1e-5
    _, tape_b = priors.infill_taped(b2['in_body_pose'], b2['frame_mask'], [T - 37], b2['in_motion_latent'][None])
    alone = priors.infill_backward(tape_b, W[:, :T - 37].contiguous())[0].cpu().numpy()
    assert np.abs(both[1, :alone.shape[0]] - alone).max() < 1e-5


@pytest.mark.parametrize('lens', [[120], [300, 47, 120]])
def test_taped_pose_is_the_plain_pose_bit_for_bit_in_small_batches(priors, lens):
    """Below SMALL_ROWS / 50 sequences the plain infiller runs the separate kernels the tape always runs, through the same window forward
    (infiller_window of nets.hip, once on workspace aliases and once on the tape's slots): the two poses are the same bits."""
    dev = torch.device('cuda:0')
    T = max(lens)
    ins = [mg.net_inputs(n, seed=i) for i, n in enumerate(lens)]
    pose = torch.zeros(len(lens), T, 69, device=dev)
    vis = torch.zeros(len(lens), T, device=dev)
    meps = torch.zeros(len(lens), max(x['in_motion_latent'].shape[0] for x in ins), 128, device=dev)
    for i, x in enumerate(ins):
        pose[i, :lens[i]] = torch.tensor(x['in_body_pose'][0])
        vis[i, :lens[i]] = torch.tensor(x['frame_mask'][0]).float()
        meps[i, :x['in_motion_latent'].shape[0]] = torch.tensor(x['in_motion_latent'])
    taped, _ = priors.infill_taped(pose, vis, lens, meps)
    plain = priors.infer(pose, vis, lens, motion_eps=meps, traj_eps=None, traj=False)['pose']
    assert torch.equal(taped, plain)


def test_range_analysis_selects_the_fp32_kernels_for_a_checkpoint_outside_fp16(asset_root, priors, golden, monkeypatch):
    """The fp16-split kernels hold every fp32 operand as two fp16 numbers: fine for O(1) activations and O(0.05) weights, wrong above 65 504.
    glamr_nets_create bounds, from the weights alone, every value those kernels could convert; a checkpoint that can leave fp16's range runs
    the plain fp32 kernels everywhere (slower, never wrong).  Checked three ways: the shipped (default-initialised) checkpoints keep the fast
    path; a LayerNorm gain x 3e4 (rows of ~1e5 entering a feed-forward block) switches the handle to fp32 and its outputs equal the CPU oracle's
    with the same weights -- while the split kernels, forced onto that checkpoint, do not."""
    import ctypes
    from glamr_amd import _lib
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    from oracle.port import nets as onets
    dev = torch.device('cuda:0')
    wc = (ctypes.c_double * 2)()
    assert _lib.lib().glamr_nets_precision(priors.h, wc) == 0
    print('shipped checkpoints: worst-case converted activation %.0f, largest weight %.3f -> fp16-split kernels' % (wc[0], wc[1]))
    assert wc[0] < 3e4 and wc[1] < 10
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(asset_root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    big = {k: v.clone() for k, v in sd['inf'].items()}
    big['context_encoder.temporal_net.layers.0.norm1.weight'] *= 3.0e4           # rows of ~1e5 enter the first feed-forward block: beyond fp16
    import logging
    seen = []
    handler = logging.Handler()
    handler.emit = lambda record: seen.append((record.levelno, record.getMessage()))
    logging.getLogger('glamr_amd').addHandler(handler)
    try:
        hb = MotionPriorsHandle(big, sd['trj'], rest, synth.SMPL_PARENTS, dev)
    finally:
        logging.getLogger('glamr_amd').removeHandler(handler)
    assert _lib.lib().glamr_nets_precision(hb.h, wc) == 1 and wc[0] > 3e4
    # the selection is SAID: a warning names the fp32 family and the bound that ruled the fp16 planes out
    assert hb.fp32_only and hb.precision_bound > 3e4 and not priors.fp32_only
    assert any(lvl == logging.WARNING and 'plain fp32 kernels' in msg for lvl, msg in seen), seen
    T = 120
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    B = 48                                                                            # 48 x 50 rows >= 2048: the shapes the split kernels would take
    pose, vis = b['in_body_pose'].repeat(B, 1, 1), b['frame_mask'].repeat(B, 1)
    eps = b['in_motion_latent'][None].repeat(B, 1, 1)
    out = hb.infer(pose, vis, [T] * B, motion_eps=eps, traj_eps=b['in_traj_latent'].repeat(B, 1))
    assert torch.isfinite(out['pose']).all() and torch.equal(out['pose'][0], out['pose'][B - 1])
    ora = onets.MotionInfillerVAE().eval()
    ora.load_state_dict({k: v.float() for k, v in big.items() if not k.startswith('smpl.')}, strict=True)
    with torch.no_grad():
        d = ora.inference({'in_body_pose': b['in_body_pose'].cpu(), 'frame_mask': b['frame_mask'].cpu(), 'in_motion_latent': b['in_motion_latent'].cpu()},
                          sample_num=1, multi_step=True)
    err = _err(out['pose'][0].cpu(), d['infer_out_body_pose'][0, 0])
    print('LayerNorm gain x 3e4 (rows ~1e5): fp32 kernels vs CPU oracle %.2e' % err)
    assert err < 1e-4
    # ... and what the split kernels would have made of it (analysis overridden): not the right values
    monkeypatch.setenv('GLAMR_NETS_FORCE_FP16', '1')
    hw = MotionPriorsHandle(big, sd['trj'], rest, synth.SMPL_PARENTS, dev)
    monkeypatch.delenv('GLAMR_NETS_FORCE_FP16')
    assert _lib.lib().glamr_nets_precision(hw.h, None) == 0
    bad = hw.infer(pose, vis, [T] * B, motion_eps=eps, traj_eps=b['in_traj_latent'].repeat(B, 1))['pose'][0].cpu()
    wrong = (not bool(torch.isfinite(bad).all())) or _err(bad, d['infer_out_body_pose'][0, 0]) > 1e-3
    print('the fp16-split kernels on the same checkpoint: finite %s, error %.2e' % (bool(torch.isfinite(bad).all()), _err(torch.nan_to_num(bad), d['infer_out_body_pose'][0, 0])))
    assert wrong
    hw.close()
    hb.close()


def test_forced_fp32_kernels_match_the_reference(asset_root, golden, monkeypatch):
    import ctypes
    from glamr_amd import _lib
    from glamr_amd.models.priors import MotionPriorsHandle
    from glamr_amd.utils import synth
    monkeypatch.setenv('GLAMR_NETS_FORCE_FP32', '1')
    dev = torch.device('cuda:0')
    sd = {}
    for name, sub in (('inf', 'motion_filler/motion_infiller_demo'), ('trj', 'traj_pred/traj_pred_demo')):
        path = sorted(glob.glob(os.path.join(asset_root, 'results', sub, 'version_*', 'checkpoints', '*best*.ckpt')))[-1]
        sd[name] = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    md = synth.make_smpl_model()
    rest = (md['J_regressor'].astype(np.float64) @ md['v_template'].astype(np.float64)).astype(np.float32)
    hf = MotionPriorsHandle(sd['inf'], sd['trj'], rest, synth.SMPL_PARENTS, dev)
    assert _lib.lib().glamr_nets_precision(hf.h, None) == 1
    g = golden('nets')
    T, B = 300, 600                                                                    # 600 sequences: the batch sizes of the MFMA LSTM and the fused kernels
    b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T).items()}
    out = hf.infer(b['in_body_pose'].repeat(B, 1, 1), b['frame_mask'].repeat(B, 1), [T] * B, motion_eps=b['in_motion_latent'][None].repeat(B, 1, 1),
                   traj_eps=b['in_traj_latent'].repeat(B, 1))
    e = (_err(out['pose'][B - 1].cpu(), g['T%d_body_pose' % T][0, 0]), _err(out['local_traj'][B - 1].cpu(), g['T%d_local_traj' % T][:, 0, 0]),
         _err(out['trans'][B - 1].cpu(), g['T%d_trans' % T][0, 0]))
    print('fp32-only kernels at batch 600 vs reference: body pose %.2e, local trajectory %.2e, translation %.2e' % e)
    assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 2e-4
    hf.close()


def test_graph_cache_and_resident_sets_are_bounded(priors):
    """The priors replay a call they have seen twice as a HIP graph, keyed by geometry and buffer addresses; the handle keeps at most 24
    graphs (least recently used evicted, its executable destroyed) and the Python side at most three resident buffer sets per stream: a
    dataset of videos of many lengths must not grow device memory or graph count without bound.  30 geometries, each called twice on its
    own persistent buffers; the first one -- evicted by then -- still gives the values it gave before."""
    dev = torch.device('cuda:0')
    outs = {}
    bufs = {}
    for T in range(41, 71):
        b = {k: torch.tensor(v, device=dev) for k, v in mg.net_inputs(T, seed=T).items()}
        nw = b['in_motion_latent'].shape[0]
        rs = dict(pose=torch.empty(1, T, 69, device=dev), local_traj=torch.empty(1, T, 11, device=dev), trans=torch.empty(1, T, 3, device=dev),
                  orient=torch.empty(1, T, 3, device=dev),
                  ws=torch.empty(_ws_bytes(priors, 1, T), dtype=torch.uint8, device=dev), persistent=False)
        bufs[T] = (b, rs)
        for _ in range(2):          # second call: captured
            o = priors.infer(b['in_body_pose'], b['frame_mask'], [T], motion_eps=b['in_motion_latent'][None], traj_eps=b['in_traj_latent'], buffers=rs)
        outs[T] = {k: v.clone() for k, v in o.items()}
    b, rs = bufs[41]
    for _ in range(3):              # plain, captured again, replayed
        o = priors.infer(b['in_body_pose'], b['frame_mask'], [41], motion_eps=b['in_motion_latent'][None], traj_eps=b['in_traj_latent'], buffers=rs)
        for k in o:
            assert torch.equal(o[k], outs[41][k]), k
    # resident sets: least recently used dropped beyond three per stream
    for i, T in enumerate((50, 60, 70, 80, 90)):
        priors.resident_set(2, T, 3)
    sid = torch.cuda.current_stream(dev).cuda_stream
    assert len(priors._ring[sid]) == priors.RESIDENT_GEOMETRIES == 3 and (2, 50, 3) not in priors._ring[sid] and (2, 90, 3) in priors._ring[sid]
    first = priors.resident_set(2, 90, 3)
    assert first['uses'] == 2 and first['persistent']          # a set tells the library to capture from its second use on


def _ws_bytes(priors, B, T):
    from glamr_amd import _lib
    return _lib.lib().glamr_nets_workspace_bytes(priors.h, B, T)
