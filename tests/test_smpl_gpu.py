"""MI355X parity tests of the SMPL kernels (glamr_smpl_* through the ctypes ABI) against the fp32 CPU restatement and the reference-generated
fixtures.  Against the restatement on the same inputs the bound is the measured one of tests/smpl_ref_common.py (16 x the restatement's own
rounding against fp64, 1.2e-5 to 1.8e-5 m at ~1 m) plus one such rounding for the fp32 reference itself; against the fixture files, whose
reference is the fp32 reference run, and for the rigid-root identity (two device results and a torch rotation) it stays 1e-4 m (BASELINE.json
north_star).  The comparison against fp64, the call variants, the pose families and the per-(frame, joint) gradient measures are in
tests/test_smpl_fp64_gpu.py."""
import os
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from oracle.port import build
from tests import smpl_ref_common as sc

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _tol(name, model='fixture'):
    """Anchored call at ~1 m against the fp32 restatement: the device's 16 floors against fp64 plus the restatement's own one."""
    return (sc.FLOOR_FACTOR + 1) * sc.FWD_FLOOR[model]['1m_noscale'][name]


@pytest.fixture(scope='module')
def models(asset_root):
    from glamr_amd.lib.models.smpl import SMPL
    ora = build.load_smpl(asset_root)
    dev = torch.device('cuda:0')
    mine = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk', create_transl=False,
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(dev)
    return ora, mine, dev


def _err(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def test_smpl_matches_reference_fixture(models, golden):
    ora, mine, dev = models
    g = golden('smpl')
    x = {k: torch.tensor(v, device=dev) for k, v in mg.seeded_inputs('smpl').items()}
    out = mine(global_orient=x['pose'][:, :3], body_pose=x['pose'][:, 3:], betas=x['betas'], root_trans=x['trans'],
               root_scale=x['scale'], return_full_pose=True)
    assert _err(out.joints, torch.tensor(g['joints'])) < TOL
    assert _err(out.vertices[:, ::mg.VERT_STRIDE], torch.tensor(g['verts_sub'])) < TOL
    out2 = mine(global_orient=x['pose'][:, :3], body_pose=x['pose'][:, 3:], betas=x['betas'], return_full_pose=True)
    assert _err(out2.joints, torch.tensor(g['joints_noanchor'])) < TOL
    assert _err(out2.vertices[:, ::mg.VERT_STRIDE], torch.tensor(g['verts_noanchor_sub'])) < TOL
    out3 = mine(global_orient=x['pose'][:, :3], body_pose=x['pose'][:, 3:], betas=x['betas'], root_trans=x['trans'], orig_joints=True)
    assert _err(out3.joints, torch.tensor(g['joints_orig24'])) < TOL
    fk = mine.get_joints(global_orient=x['pose'][:, :3], body_pose=x['pose'][:, 3:], betas=x['betas'], root_trans=x['trans'])
    assert _err(fk, torch.tensor(g['fk_joints'])) < TOL


@pytest.mark.parametrize('B', [1, 31, 300, 333])
def test_smpl_matches_oracle_full_mesh(models, B):
    """Every vertex and joint, ragged batch sizes (tile padding), at the BASELINE frame count."""
    ora, mine, dev = models
    gen = torch.Generator().manual_seed(B)
    pose = torch.randn(B, 72, generator=gen) * 0.35
    betas = torch.randn(B, 10, generator=gen)
    trans = torch.randn(B, 3, generator=gen)
    ref = ora(global_orient=pose[:, :3], body_pose=pose[:, 3:], betas=betas, root_trans=trans, return_full_pose=True)
    out = mine(global_orient=pose[:, :3].to(dev), body_pose=pose[:, 3:].to(dev), betas=betas.to(dev), root_trans=trans.to(dev))
    assert out.vertices.shape == (B, 6890, 3) and out.joints.shape == (B, 26, 3)
    assert _err(out.joints, ref.joints) < _tol('joints')
    assert _err(out.vertices, ref.vertices) < _tol('verts')
    # joints-only call: skins only the vertices the mapped joints depend on (a different summation grouping of the regressed
    # joints, hence last-bit differences from the full-mesh call)
    j_only = mine(global_orient=pose[:, :3].to(dev), body_pose=pose[:, 3:].to(dev), betas=betas.to(dev), root_trans=trans.to(dev),
                  return_verts=False)
    assert j_only.vertices is None
    assert _err(j_only.joints, out.joints) < 2e-6
    assert _err(j_only.joints, ref.joints) < _tol('joints')


def test_smpl_rigid_root_identity_full_size(models):
    """Size-independent property: with re-anchoring, a root rotation acts rigidly about joint 0."""
    ora, mine, dev = models
    B = 300
    gen = torch.Generator().manual_seed(5)
    body = (torch.randn(B, 69, generator=gen) * 0.3).to(dev)
    betas = torch.randn(B, 10, generator=gen).to(dev)
    trans = torch.randn(B, 3, generator=gen).to(dev)
    orient = (torch.randn(B, 3, generator=gen)).to(dev)
    zero = torch.zeros(B, 3, device=dev)
    a = mine(global_orient=zero, body_pose=body, betas=betas, root_trans=zero)
    b = mine(global_orient=orient, body_pose=body, betas=betas, root_trans=trans)
    from oracle.smplx_lbs import batch_rodrigues
    R = batch_rodrigues(orient.cpu()).to(dev)
    assert _err(torch.einsum('bij,bvj->bvi', R, a.vertices) + trans[:, None], b.vertices) < TOL
    assert _err(torch.einsum('bij,bvj->bvi', R, a.joints) + trans[:, None], b.joints) < TOL


@pytest.mark.parametrize('B', [1, 37, 300, 19200])
def test_root_relative_joints_are_the_zero_orientation_forward_bit_for_bit(models, B):
    """SMPL.root_relative_joints (GLAMR_SMPL_BODY_POSE_ONLY: the optimiser's cached joints without the (B,72) concatenation and the zero
    arrays) against forward(global_orient=0, root_trans=0, return_verts=False): the same kernels on the same numbers."""
    ora, mine, dev = models
    gen = torch.Generator().manual_seed(11 + B)
    body = (torch.randn(B, 69, generator=gen) * 0.3).to(dev)
    betas = torch.randn(B, 10, generator=gen).to(dev)
    zero = torch.zeros(B, 3, device=dev)
    a = mine(global_orient=zero, body_pose=body, betas=betas, root_trans=zero, return_verts=False).joints
    b = mine.root_relative_joints(body, betas)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        mine.root_relative_joints(body[:, :60], betas)


def test_smpl_backward_root(models):
    ora, mine, dev = models
    B = 40
    gen = torch.Generator().manual_seed(11)
    body = torch.randn(B, 69, generator=gen) * 0.3
    betas = torch.randn(B, 10, generator=gen)
    orient = torch.randn(B, 3, generator=gen)
    orient[0] = 0.0
    trans = torch.randn(B, 3, generator=gen)
    scale = torch.rand(B, generator=gen) + 0.5
    wj = torch.randn(B, 26, 3, generator=gen)
    wv = torch.randn(B, 6890, 3, generator=gen) * 0.01

    def run(model, d):
        o, t, s = orient.clone().to(d).requires_grad_(True), trans.clone().to(d).requires_grad_(True), scale.clone().to(d).requires_grad_(True)
        out = model(global_orient=o, body_pose=body.to(d), betas=betas.to(d), root_trans=t, root_scale=s)
        loss = (out.joints * wj.to(d)).sum() + (out.vertices * wv.to(d)).sum()
        loss.backward()
        return o.grad.cpu(), t.grad.cpu(), s.grad.cpu()

    ref = run(ora, torch.device('cpu'))
    got = run(mine, dev)
    for r, g, name in zip(ref, got, ('orient', 'trans', 'scale')):
        scale_ = max(1.0, r.abs().max().item())
        assert (r - g).abs().max().item() / scale_ < 2e-4, name


@pytest.mark.parametrize('variant', ['joints+verts anchored', 'joints only anchored', 'plain call', 'orig joints'])
def test_smpl_backward_wrt_body_pose_and_betas(models, variant):
    """The GENERAL backward (glamr_smpl_backward): gradients w.r.t. the whole pose, the shape coefficients, root translation and scale from
    gradients of joints and vertices -- skinning, blend shapes, kinematic chain, joint regression and re-anchoring in reverse -- against
    torch autograd through the CPU restatement (oracle/port/smpl.py over oracle/smplx_lbs.py).  Variants: the full mesh, the joints-only
    tiling (picked + virtual vertices: what the latent-optimisation loop differentiates), the call without root_trans, the 24 chain joints."""
    ora, mine, dev = models
    B = 37
    gen = torch.Generator().manual_seed(21)
    body = torch.randn(B, 69, generator=gen) * 0.3
    betas = torch.randn(B, 10, generator=gen)
    orient = torch.randn(B, 3, generator=gen)
    orient[0] = 0.0
    body[1] = 0.0
    trans = torch.randn(B, 3, generator=gen)
    scale = torch.rand(B, generator=gen) + 0.5
    anchored = 'anchored' in variant
    with_verts = variant in ('joints+verts anchored', 'plain call')
    orig = variant == 'orig joints'
    wj = torch.randn(B, 24 if orig else 26, 3, generator=gen)
    wv = torch.randn(B, 6890, 3, generator=gen) * 0.01

    def run(model, d):
        o, bp, be = (x.clone().to(d).requires_grad_(True) for x in (orient, body, betas))
        t, s = trans.clone().to(d).requires_grad_(True), scale.clone().to(d).requires_grad_(True)
        kw = dict(root_trans=t, root_scale=s) if anchored else {}
        if orig:
            kw = dict(root_trans=t, orig_joints=True)
        if model is mine and not with_verts:
            kw['return_verts'] = False
        out = model(global_orient=o, body_pose=bp, betas=be, **kw)
        loss = (out.joints * wj.to(d)).sum()
        if with_verts:
            loss = loss + (out.vertices * wv.to(d)).sum()
        loss.backward()
        grads = {'orient': o.grad, 'body_pose': bp.grad, 'betas': be.grad}
        if anchored or orig:
            grads['trans'] = t.grad
        if anchored:
            grads['scale'] = s.grad
        return {k: v.cpu() for k, v in grads.items()}

    ref = run(ora, torch.device('cpu'))
    got = run(mine, dev)
    for name, r in ref.items():
        g = got[name]
        assert g.shape == r.shape and torch.isfinite(g).all(), name
        err = (r - g).abs().max().item() / max(1.0, r.abs().max().item())
        print('%s: d/d%s relative error %.2e (largest %.2e)' % (variant, name, err, r.abs().max().item()))
        assert err < 2e-4, (variant, name, err)
    assert ref['body_pose'].abs().max() > 1e-3 and ref['betas'].abs().max() > 1e-3


def test_sparse_regressors_as_the_real_model_stores_them(tmp_path):
    """The published SMPL pickle keeps J_regressor as a scipy.sparse matrix with ~200 non-zeros per joint, and J_regressor_extra is as sparse.
    A model of that kind (the synthetic one cut to the 200 largest weights per joint, rows renormalised, stored as CSC) through the loader,
    the full-mesh tiling, the virtual-vertex tiling of the joints-only call (24 virtual vertices per regressed joint built FROM the sparse
    rows) and the general backward -- against the CPU restatement on the same files."""
    import pickle
    import scipy.sparse as sp
    from glamr_amd.utils import synth
    from glamr_amd.lib.models.smpl import SMPL
    from oracle.port.smpl import SMPL as OracleSMPL
    md = synth.make_smpl_model()

    def cut(R, keep=200):
        R = np.array(R, dtype=np.float64)
        for r in range(R.shape[0]):
            small = np.argsort(R[r])[:-keep]
            R[r, small] = 0.0
            R[r] /= R[r].sum()
        return R.astype(np.float32)
    Jr, Jx = cut(md['J_regressor']), cut(md['J_regressor_extra'])
    assert (Jr != 0).sum(1).max() <= 200 and (Jx != 0).sum(1).max() <= 200
    mdir = tmp_path / 'data' / 'body_models' / 'smpl'
    os.makedirs(mdir)
    model = {k: v for k, v in md.items() if k != 'J_regressor_extra' and not k.startswith('_')}
    model['J_regressor'] = sp.csc_matrix(Jr)
    with open(mdir / 'SMPL_NEUTRAL.pkl', 'wb') as f:
        pickle.dump(model, f, protocol=2)
    np.save(tmp_path / 'data' / 'J_regressor_extra.npy', Jx)
    dev = torch.device('cuda:0')
    mine = SMPL(str(mdir), pose_type='body26fk', extra_regressor_path=str(tmp_path / 'data' / 'J_regressor_extra.npy')).to(dev)
    ora = OracleSMPL(str(mdir), pose_type='body26fk', extra_regressor_path=str(tmp_path / 'data' / 'J_regressor_extra.npy'))
    gen = torch.Generator().manual_seed(3)
    B = 45
    pose, betas, trans = torch.randn(B, 72, generator=gen) * 0.4, torch.randn(B, 10, generator=gen), torch.randn(B, 3, generator=gen)
    ref = ora(global_orient=pose[:, :3], body_pose=pose[:, 3:], betas=betas, root_trans=trans)
    full = mine(global_orient=pose[:, :3].to(dev), body_pose=pose[:, 3:].to(dev), betas=betas.to(dev), root_trans=trans.to(dev))
    jonly = mine(global_orient=pose[:, :3].to(dev), body_pose=pose[:, 3:].to(dev), betas=betas.to(dev), root_trans=trans.to(dev), return_verts=False)
    e = (_err(full.joints, ref.joints), _err(full.vertices, ref.vertices), _err(jonly.joints, ref.joints))
    print('sparse regressors: joints %.2e, vertices %.2e, joints-only tiling %.2e' % e)
    # (the fixture model with cut regressors: between the two models of the common module, held to the looser of their bounds)
    tj, tv = (max(_tol(n, 'fixture'), _tol(n, 'conditioned')) for n in ('joints', 'verts'))
    assert e[0] < tj and e[1] < tv and e[2] < tj
    # gradients w.r.t. body pose / betas through the joints-only tiling
    wj = torch.randn(B, 26, 3, generator=gen)
    bp_c, be_c = pose[:, 3:].clone().requires_grad_(True), betas.clone().requires_grad_(True)
    (ora(global_orient=pose[:, :3], body_pose=bp_c, betas=be_c, root_trans=trans).joints * wj).sum().backward()
    bp_g, be_g = pose[:, 3:].clone().to(dev).requires_grad_(True), betas.clone().to(dev).requires_grad_(True)
    (mine(global_orient=pose[:, :3].to(dev), body_pose=bp_g, betas=be_g, root_trans=trans.to(dev), return_verts=False).joints * wj.to(dev)).sum().backward()
    for a, b, name in ((bp_g.grad.cpu(), bp_c.grad, 'body_pose'), (be_g.grad.cpu(), be_c.grad, 'betas')):
        assert (a - b).abs().max().item() / max(1.0, b.abs().max().item()) < 2e-4, name
