"""fp64 reference of SMPL skinning and its gradients (oracle.port.smpl.SMPL in .double(): forward, get_joints and autograd all run in fp64),
the two models and the pose families the device tests run, the error measures, the mutations that show those tests can fail, and the
tolerances, each 16 x the rounding of the fp32 CPU restatement against the fp64 one (the layout of tests/traj_ref_common.py).

Two models.  'fixture' is glamr_amd.utils.synth.make_smpl_model() as every other test loads it: dense skinning weights, posedirs at sigma = 0.002
(the whole pose-blend product is a sub-centimetre term).  'conditioned' is the same model with posedirs x 5 (sigma = 0.01, the published model's
order), skinning weights cut to the 4 largest per vertex and both regressors cut to 200 non-zeros per joint, stored as the published pickle
stores them (scipy CSC): a fault in the low fp16 plane of the blend directions moves its vertices five times further.

`lbs_core` / `finish` restate the forward of oracle/smplx_lbs.py and oracle/port/smpl.py so that a mutation can be placed inside it;
tests/test_smpl_ref.py pins the unmutated restatement to the port's own forward bit for bit."""
import copy
import math
import os
import pickle
import numpy as np
import torch

from oracle.port import build
from oracle.port.smpl import BODY26FK_MAP
from oracle.smplx_lbs import SMPL_EXTRA_VERTEX_IDS, batch_rigid_transform, batch_rodrigues, blend_shapes, vertices2joints

MODELS = ('fixture', 'conditioned')
POSEDIRS_GAIN, WEIGHTS_KEPT, REGRESSOR_KEPT = 5.0, 4, 200


# ---- the models -------------------------------------------------------------------------------------------------------------------------
def write_conditioned_assets(root):
    """<root>/data/body_models/smpl/SMPL_NEUTRAL.pkl and <root>/data/J_regressor_extra.npy of the conditioned model.  Returns root."""
    import scipy.sparse as sp
    from glamr_amd.utils import synth
    md = synth.make_smpl_model()

    def cut(R, keep):
        R = np.array(R, dtype=np.float64)
        for r in range(R.shape[0]):
            R[r, np.argsort(R[r])[:-keep]] = 0.0
            R[r] /= R[r].sum()
        return R.astype(np.float32)
    mdir = os.path.join(root, 'data', 'body_models', 'smpl')
    os.makedirs(mdir, exist_ok=True)
    model = {k: v for k, v in md.items() if k != 'J_regressor_extra' and not k.startswith('_')}
    model['posedirs'] = (md['posedirs'].astype(np.float64) * POSEDIRS_GAIN).astype(np.float32)
    model['weights'] = cut(md['weights'], WEIGHTS_KEPT)
    model['J_regressor'] = sp.csc_matrix(cut(md['J_regressor'], REGRESSOR_KEPT))
    with open(os.path.join(mdir, 'SMPL_NEUTRAL.pkl'), 'wb') as f:
        pickle.dump(model, f, protocol=2)
    np.save(os.path.join(root, 'data', 'J_regressor_extra.npy'), cut(md['J_regressor_extra'], REGRESSOR_KEPT))
    return root


def model_root(name, asset_root, tmp_root):
    """Asset directory of model `name`: the session's synthetic assets, or the conditioned files written under tmp_root."""
    return asset_root if name == 'fixture' else write_conditioned_assets(str(tmp_root))


def reference(root, dtype=torch.float64):
    """The CPU restatement on the files under `root`, in `dtype`."""
    m = copy.deepcopy(build.load_smpl(root))
    return m.double() if dtype == torch.float64 else m


# ---- the frames -------------------------------------------------------------------------------------------------------------------------
# Frame i of every batch is the same frame whatever the batch size (its own generator): a batch of B frames is the prefix of a longer one, and
# one fp64 result serves every size.  Families cycle so that 8 frames already hold all three.
FAMILIES = ('generic', 'small', 'large', 'generic', 'small', 'large', 'generic', 'large')
GRAD_FAMILIES = ('generic', 'large', 'small', 'generic', 'small', 'large', 'small', 'generic')
SMALL_LEVELS = (1e-2, 1e-3, 1e-4, 1e-6, 'zero', 'single')
LARGE_ANGLES = (math.pi - 1e-3, math.pi, math.pi + 0.5, 2 * math.pi - 1e-3, 7.0)
SEED = 20240


def _generic_pose(rng):
    p = 0.6 * rng.normal(size=(24, 3))
    for j in range(24):
        while np.linalg.norm(p[j]) < 0.05:
            p[j] = 0.6 * rng.normal(size=3)
    return p


def frames(B, families=FAMILIES):
    """B distinct frames as fp32 arrays: pose (B,72), betas (B,10), scale (B,), trans1 / trans50 (B,3), and `label` per frame: 'generic',
    'large' or 'small:<level>'.
      generic  0.6 randn per component, a joint with an angle below 0.05 rad drawn again;
      small    the whole frame at 1e-2, 1e-3, 1e-4, 1e-6 rad (level x randn), an exact-zero frame, a frame with ONE non-zero (generic) joint;
      large    a generic frame with three joints (the root among them in every other frame) at pi - 1e-3, pi, pi + 0.5, 2 pi - 1e-3 and 7.0 rad,
               about random axes and about the coordinate axes in turn;
      betas 1.5 randn, frames 5 and 13 of every 16 at +-5 (alternating signs); root_scale U(0.5, 1.5), frame 3 at 0.05; translation ~ 1 m
      (randn) and ~ 50 m (40 to 60 m along a random direction)."""
    out = {k: [] for k in ('pose', 'betas', 'scale', 'trans1', 'trans50')}
    labels = []
    for i in range(B):
        rng = np.random.default_rng([SEED, i])
        fam = families[i % len(families)]
        n = (i // len(families)) * families.count(fam) + families[:i % len(families)].count(fam)        # how many of its family came before
        pose, label = _generic_pose(rng), fam
        if fam == 'small':
            lvl = SMALL_LEVELS[n % len(SMALL_LEVELS)]
            label = 'small:%s' % lvl
            if lvl == 'zero':
                pose = np.zeros((24, 3))
            elif lvl == 'single':
                j = (7 * n + 3) % 24
                keep, pose = pose[j].copy(), np.zeros((24, 3))
                pose[j] = keep
            else:
                pose = lvl * rng.normal(size=(24, 3))
        elif fam == 'large':
            js = [0] if n % 2 == 0 else []
            while len(js) < 3:
                j = int(rng.integers(1, 24))
                if j not in js:
                    js.append(j)
            for t, j in enumerate(js):
                axis = rng.normal(size=3)
                axis /= np.linalg.norm(axis)
                if (n + t) % 2 == 1:
                    axis = np.eye(3)[((n + t) // 2) % 3] * (1.0 if (n + t) % 4 == 1 else -1.0)
                pose[j] = axis * LARGE_ANGLES[(n + t) % len(LARGE_ANGLES)]
        betas = 1.5 * rng.normal(size=10)
        if i % 16 in (5, 13):
            betas = 5.0 * np.where(np.arange(10) % 2 == 0, 1.0, -1.0) * (1.0 if i % 16 == 5 else -1.0)
        scale = 0.05 if i == 3 else rng.uniform(0.5, 1.5)
        d = rng.normal(size=3)
        out['pose'].append(pose.reshape(72))
        out['betas'].append(betas)
        out['scale'].append(scale)
        out['trans1'].append(rng.normal(size=3))
        out['trans50'].append(d / np.linalg.norm(d) * rng.uniform(40.0, 60.0))
        labels.append(label)
    out = {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}
    out['label'] = labels
    return out


def group(label):
    """Tolerance group of a frame: 'main' (generic and large angles) or its own small-angle level."""
    return 'main' if label in ('generic', 'large') else label


GROUPS = ('main',) + tuple('small:%s' % l for l in SMALL_LEVELS)


# ---- the forward, with room for a mutation ----------------------------------------------------------------------------------------------
MUTATIONS = ('a', 'b', 'c', 'd', 'e', 'f')
GRAD_MUTATIONS = ('g1', 'g2', 'g3')
MUTATION_NAMES = {'a': 'posedirs rounded to fp16', 'b': 'shapedirs rounded to fp16',
                  'c': 'one 8-wide k step of the blend product zeroed for one 32-vertex tile', 'd': 'pose features of joint 23 dropped',
                  'e': "one joint's skinning transform from the neighbouring frame", 'f': 'pivot from chain joint 0 instead of output joint 0',
                  'g1': "joint 22's d/d pose x 1.01", 'g2': 'd/d betas without the joint regression', 'g3': 'Rodrigues backward without (gx.r)/theta^2'}
C_TILE, C_K0 = 100, 112          # mutation (c): vertices 3200..3231, feature entries 112..119 (k step 0 of the upper lane half): pose features 102..109
E_JOINT = 5                      # mutation (e)


class _Rodrigues(torch.autograd.Function):
    """oracle.smplx_lbs.batch_rodrigues with the backward written out the way rodrigues_smplx_bwd (glamr_amd/csrc/smpl.hip) writes it, so that
    one of its terms can be dropped (mutation g3).  tests/test_smpl_ref.py holds the complete form to autograd through batch_rodrigues."""

    @staticmethod
    def forward(ctx, r, drop):
        ctx.save_for_backward(r)
        ctx.drop = drop
        return batch_rodrigues(r)

    @staticmethod
    def backward(ctx, gR):
        r, = ctx.saved_tensors
        g = gR.reshape(-1, 9).unbind(1)
        a = r + 1e-8
        angle = a.norm(dim=1)
        inv = 1.0 / angle
        x, y, z = (r * inv[:, None]).unbind(1)
        s, c = torch.sin(angle), torch.cos(angle)
        c1 = 1.0 - c
        g_s = -z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]
        g_c1 = -(y * y + z * z) * g[0] + x * y * (g[1] + g[3]) + x * z * (g[2] + g[6]) - (x * x + z * z) * g[4] + y * z * (g[5] + g[7]) - (x * x + y * y) * g[8]
        gx = s * (g[7] - g[5]) + c1 * (y * (g[1] + g[3]) + z * (g[2] + g[6]) - 2.0 * x * (g[4] + g[8]))
        gy = s * (g[2] - g[6]) + c1 * (x * (g[1] + g[3]) + z * (g[5] + g[7]) - 2.0 * y * (g[0] + g[8]))
        gz = s * (g[3] - g[1]) + c1 * (x * (g[2] + g[6]) + y * (g[5] + g[7]) - 2.0 * z * (g[0] + g[4]))
        tot = g_s * c + g_c1 * s
        if not ctx.drop:
            tot = tot - (gx * r[:, 0] + gy * r[:, 1] + gz * r[:, 2]) * inv * inv
        return torch.stack([gx, gy, gz], 1) * inv[:, None] + (tot * inv)[:, None] * a, None


def lbs_core(m, pose, betas, mut=None, rodrigues_fn=False):
    """oracle.smplx_lbs.lbs on the buffers of `m`, operation for operation: (vertices (B,V,3), posed chain joints (B,24,3)), not anchored."""
    B, dt = pose.shape[0], pose.dtype
    posedirs, shapedirs = m.posedirs, m.shapedirs
    if mut == 'a':
        posedirs = posedirs.half().to(dt)
    if mut == 'b':
        shapedirs = shapedirs.half().to(dt)
    disp = blend_shapes(betas, shapedirs)
    v_shaped = m.v_template + disp
    J = vertices2joints(m.J_regressor, m.v_template + disp.detach() if mut == 'g2' else v_shaped)
    R = (_Rodrigues.apply(pose.view(-1, 3), mut == 'g3') if (rodrigues_fn or mut == 'g3') else batch_rodrigues(pose.view(-1, 3))).view([B, -1, 3, 3])
    feat = (R[:, 1:, :, :] - torch.eye(3, dtype=dt)).view([B, -1])
    if mut == 'd':
        feat = torch.cat([feat[:, :22 * 9], torch.zeros_like(feat[:, 22 * 9:])], dim=1)
    offs = torch.matmul(feat, posedirs).view(B, -1, 3)
    if mut == 'c':
        k0, v0 = C_K0 - 10, C_TILE * 32
        offs = offs.clone()
        offs[:, v0:v0 + 32] -= torch.matmul(feat[:, k0:k0 + 8], posedirs[k0:k0 + 8].view(8, -1, 3)[:, v0:v0 + 32].reshape(8, 96)).view(B, 32, 3)
    v_posed = offs + v_shaped
    Jt, A = batch_rigid_transform(R, J, m.parents, dtype=dt)
    if mut == 'e':
        A = torch.cat([A[:, :E_JOINT], torch.roll(A[:, E_JOINT:E_JOINT + 1], -1, 0), A[:, E_JOINT + 1:]], dim=1)
    W = m.lbs_weights.unsqueeze(dim=0).expand([B, -1, -1])
    T = torch.matmul(W, A.view(B, 24, 16)).view(B, -1, 4, 4)
    v_homo = torch.matmul(T, torch.unsqueeze(torch.cat([v_posed, torch.ones([B, v_posed.shape[1], 1], dtype=dt)], dim=2), dim=-1))
    return v_homo[:, :, :3, 0], Jt


def finish(m, verts, Jt, trans=None, scale=None, orig=False, mut=None, joint_map=None):
    """oracle.port.smpl.SMPL.forward after the LBS: picked vertices, extra-regressed joints, joint selection, re-anchoring."""
    if orig:
        joints = Jt
    else:
        picked = torch.index_select(verts, 1, torch.tensor(SMPL_EXTRA_VERTEX_IDS, dtype=torch.long))
        extra = vertices2joints(m.J_regressor_extra, verts)
        jm = torch.tensor(BODY26FK_MAP if joint_map is None else list(joint_map), dtype=torch.long)
        joints = torch.cat([Jt, picked, extra], dim=1)[:, jm, :]
    if trans is not None:
        if scale is None:
            scale = torch.ones_like(trans[:, 0])
        pivot = Jt[:, [0], :] if mut == 'f' else joints[:, [0], :]
        verts = (verts - pivot) * scale[:, None, None] + trans[:, None, :]
        joints = (joints - pivot) * scale[:, None, None] + trans[:, None, :]
    return verts, joints


def forward(m, pose, betas, trans=None, scale=None, orig=False, mut=None, joint_map=None, rodrigues_fn=False):
    v, Jt = lbs_core(m, pose, betas, mut, rodrigues_fn)
    return finish(m, v, Jt, trans, scale, orig, mut, joint_map)


def _t(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt)


def dtype_of(m):
    return m.v_template.dtype


# the outputs the forward tests compare, as (key, how it is called)
FWD_KEYS = ('plain', '1m', '1m_noscale', '50m', 'orig', 'rootrel', 'fk', 'fk_anchored')
CHUNK = 64


def forward_outputs(m, fr, mut=None, joint_map=None, keys=FWD_KEYS):
    """Every compared output of the frames `fr` in the dtype of `m`, as fp64 numpy: {key: {'verts': (B,V,3), 'joints': (B,n,3)}} --
      plain        forward without root_trans;
      1m / 50m     anchored with root_scale at the two translation regimes;  1m_noscale: anchored without root_scale;
      orig         orig_joints=True, anchored at 1 m without scale (24 chain joints);
      rootrel      zero global orientation, zero root_trans, joints only (SMPL.root_relative_joints);
      fk / fk_anchored   get_joints without / with root_trans (1 m, with scale).
    The LBS runs once per 64 frames and every anchoring is applied to its result, as the port does."""
    dt, B = dtype_of(m), fr['pose'].shape[0]
    acc = {k: {} for k in keys}

    def put(k, name, x):
        acc[k].setdefault(name, []).append(x.double().numpy())
    with torch.no_grad():
        for b0 in range(0, B, CHUNK):
            sl = slice(b0, min(B, b0 + CHUNK))
            pose, betas, scale = _t(fr['pose'][sl], dt), _t(fr['betas'][sl], dt), _t(fr['scale'][sl], dt)
            t1, t50 = _t(fr['trans1'][sl], dt), _t(fr['trans50'][sl], dt)
            # (mutation (e) takes the neighbour inside the chunk: the mutation batches are one chunk)
            v, Jt = lbs_core(m, pose, betas, mut)
            for k, kw in (('plain', {}), ('1m', dict(trans=t1, scale=scale)), ('1m_noscale', dict(trans=t1)), ('50m', dict(trans=t50, scale=scale)),
                          ('orig', dict(trans=t1, orig=True))):
                if k in keys:
                    vv, jj = finish(m, v, Jt, mut=mut, joint_map=joint_map, **kw)
                    if k != 'orig':
                        put(k, 'verts', vv)
                    put(k, 'joints', jj)
            if 'rootrel' in keys:
                zp = torch.cat([torch.zeros_like(pose[:, :3]), pose[:, 3:]], dim=1)
                put('rootrel', 'joints', forward(m, zp, betas, trans=torch.zeros_like(t1), mut=mut, joint_map=joint_map)[1])
            if 'fk' in keys:
                put('fk', 'joints', m.get_joints(global_orient=pose[:, :3], body_pose=pose[:, 3:]))
            if 'fk_anchored' in keys:
                put('fk_anchored', 'joints', m.get_joints(global_orient=pose[:, :3], body_pose=pose[:, 3:], root_trans=t1, root_scale=scale))
    return {k: {n: np.concatenate(x) for n, x in d.items()} for k, d in acc.items()}


def forward_errors(got, ref):
    """Largest absolute difference in metres per (key, output), over the frames both hold."""
    return {k: {n: float(np.abs(np.asarray(got[k][n], np.float64) - ref[k][n][:len(got[k][n])]).max()) for n in ref[k] if n in got[k]}
            for k in ref if k in got}


# ---- gradients --------------------------------------------------------------------------------------------------------------------------
VARIANTS = ('joints+verts anchored', 'joints only anchored', 'plain call', 'orig joints', 'g_verts only', 'g_joints only')
ROUTES = ('root', 'general')     # root: only global_orient, root_trans, root_scale require gradients (glamr_smpl_backward_root); general: all
GRAD_B = 40                      # the gradient batch; the device tests run its prefixes of 1, 33 and 40 frames


def variant_spec(variant):
    """(anchored with scale, orig_joints, joints enter the loss, vertices enter the loss, vertices are computed)"""
    orig = variant == 'orig joints'
    anchored = variant != 'plain call' and not orig
    lv = variant in ('joints+verts anchored', 'plain call', 'g_verts only')
    lj = variant != 'g_verts only'
    return anchored, orig, lj, lv, variant != 'joints only anchored' and not orig


def loss_weights(B, variant):
    """Weights of the linear loss sum(joints wj) + sum(vertices wv): randn and 0.01 randn (fp32), the same for every prefix of the batch."""
    gen = torch.Generator().manual_seed(77 + VARIANTS.index(variant))
    wj = torch.randn(GRAD_B, 24 if variant == 'orig joints' else 26, 3, generator=gen)
    wv = torch.randn(GRAD_B, 6890, 3, generator=gen) * 0.01
    return wj[:B], wv[:B]


def gradients(call, fr, variant, route, dt, dev='cpu'):
    """Gradients of the loss of `variant` through call(orient, body, betas, trans, scale, orig, want_verts) -> (verts or None, joints), as fp64
    numpy: pose (B,24,3) (root route: (B,1,3), the global orientation), betas (B,10), trans (B,3), scale (B,) -- those that exist for the variant
    and the route.  The plain call has no root route: without root_trans every gradient goes through the general backward."""
    anchored, orig, lj, lv, want_verts = variant_spec(variant)
    B = fr['pose'].shape[0]
    mk = lambda a, g: _t(a, dt).to(dev).requires_grad_(g)
    gen_ = route == 'general'
    o, bp, be = mk(fr['pose'][:, :3], True), mk(fr['pose'][:, 3:], gen_), mk(fr['betas'], gen_)
    t = mk(fr['trans1'], True) if (anchored or orig) else None
    s = mk(fr['scale'], True) if anchored else None
    verts, joints = call(o, bp, be, t, s, orig, want_verts)
    wj, wv = loss_weights(B, variant)
    loss = 0.0
    if lj:
        loss = loss + (joints * wj.to(dt).to(dev)).sum()
    if lv:
        loss = loss + (verts * wv.to(dt).to(dev)).sum()
    loss.backward()
    g = {'pose': torch.cat([o.grad, bp.grad], dim=1).view(B, 24, 3) if gen_ else o.grad.view(B, 1, 3)}
    if gen_:
        g['betas'] = be.grad
    if t is not None:
        g['trans'] = t.grad
    if s is not None:
        g['scale'] = s.grad
    return {k: v.detach().cpu().double().numpy() for k, v in g.items()}


def reference_call(m, mut=None, rodrigues_fn=False):
    def call(o, bp, be, t, s, orig, want_verts):
        return forward(m, torch.cat([o, bp], dim=1), be, t, s, orig, mut, rodrigues_fn=rodrigues_fn)
    return call


def variants_of(route):
    return [v for v in VARIANTS if not (route == 'root' and v == 'plain call')]


# Absolute floor of the relative measures: an entry whose fp64 norm is below GRAD_FLOOR x the MEDIAN non-zero norm of its tensor ((frame, joint)
# entries of d/d pose, frames of the others) is held to tolerance x that floor instead of tolerance x its own norm.  The median, not the
# maximum: the root's gradient is a lever over the whole body, 20 to 40 x the typical joint's, and a floor of 1e-3 x the maximum sat above 1.5
# to 3.4 % of the entries.  At 1e-3 x the median the smallest non-zero entry of every variant (1.1e-3 of the median, an end joint of the
# orig-joints loss) stays above it: the floor keeps exact zeros (joints no loss term reaches) out of the division and nothing else, which
# tests/test_smpl_ref.py asserts as "at most 1 % of the non-zero entries under the floor".
GRAD_FLOOR = 1e-3


def grad_errors(got, ref):
    """{name: (per-entry relative error, share of non-zero entries under the floor)}: pose per (frame, joint) |d|_2 / max(|g64|_2, floor), betas and trans
    per frame the same, scale per frame |d| / max(|g64|, floor)."""
    out = {}
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64)[:len(r)]
        if k == 'scale':
            n, d = np.abs(r), np.abs(g - r)
        else:
            n, d = np.linalg.norm(r, axis=-1), np.linalg.norm(g - r, axis=-1)
        floor = GRAD_FLOOR * np.median(n[n > 0])
        out[k] = (d / np.maximum(n, floor), float((n[n > 0] < floor).mean()))
    return out


def worst_by_group(name, err, labels):
    """Largest entry of a per-frame error array (B,) or (B,J) per tolerance group of its frames.  Only d/d pose has a small-angle regime of its
    own (1 - cos theta cancelling in the Rodrigues backward); the rounding of the other gradients does not depend on the pose family, and their
    floor is taken over all frames ('all') rather than over the two or three frames of one small-angle level."""
    out = {}
    for b, lab in enumerate(labels[:len(err)]):
        g = group(lab) if name == 'pose' else 'all'
        out[g] = max(out.get(g, 0.0), float(np.max(err[b])))
    return out


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------
# Each is FLOOR_FACTOR x the largest error of the fp32 restatement against the fp64 one over the frames the device tests run: 4 x for the
# split-fp16 products' 2^-22 per product against fp32's 2^-24, times 4 x for the summation order (the factor of tests/traj_ref_common.py).
# Measured on one thread, rounded up to two digits; `python -m tests.smpl_ref_common` prints the tables to paste here, and
# tests/test_smpl_ref.py measures them again and fails when a floor leaves [1/2, 2] x its constant.
FLOOR_FACTOR = 16
FWD_B = 257                      # the forward floors: frames(257), of which the device tests run prefixes

FWD_FLOOR, GRAD_FLOORS = {}, {}
FWD_FLOOR['fixture'] = {
    'plain': {'verts': 1.1e-06, 'joints': 5.2e-07},          # 1.070e-06, 5.184e-07
    '1m': {'verts': 1.1e-06, 'joints': 7.5e-07},             # 1.085e-06, 7.460e-07
    '1m_noscale': {'verts': 1.0e-06, 'joints': 5.8e-07},     # 9.942e-07, 5.705e-07
    '50m': {'verts': 2.6e-06, 'joints': 2.4e-06},            # 2.591e-06, 2.348e-06
    'orig': {'joints': 4.2e-07},                             # 4.115e-07
    'rootrel': {'joints': 7.9e-07},                          # 7.820e-07
    'fk': {'joints': 3.6e-07},                               # 3.585e-07
    'fk_anchored': {'joints': 4.9e-07},                      # 4.801e-07
}
GRAD_FLOORS['fixture'] = {
    'pose': {'main': 3.1e-05, 'small:0.0001': 1.3e-03, 'small:0.001': 1.5e-04, 'small:0.01': 2.5e-05, 'small:1e-06': 1.1e-05, 'small:single': 1.7e-05, 'small:zero': 2.0e-05},
    # 3.090e-05, 1.227e-03, 1.402e-04, 2.444e-05, 1.080e-05, 1.640e-05, 1.986e-05
    'betas': {'all': 8.8e-07},      # 8.734e-07
    'trans': {'all': 1.9e-06},      # 1.865e-06
    'scale': {'all': 4.9e-05},      # 4.869e-05  (gdot / scale, and a sum over the mesh that cancels)
}
FWD_FLOOR['conditioned'] = {
    'plain': {'verts': 7.5e-07, 'joints': 5.1e-07},          # 7.410e-07, 5.061e-07
    '1m': {'verts': 8.2e-07, 'joints': 7.2e-07},             # 8.158e-07, 7.184e-07
    '1m_noscale': {'verts': 7.0e-07, 'joints': 5.4e-07},     # 6.928e-07, 5.358e-07
    '50m': {'verts': 2.6e-06, 'joints': 2.3e-06},            # 2.514e-06, 2.283e-06
    'orig': {'joints': 4.4e-07},                             # 4.396e-07
    'rootrel': {'joints': 4.0e-07},                          # 3.957e-07
    'fk': {'joints': 3.5e-07},                               # 3.449e-07
    'fk_anchored': {'joints': 4.7e-07},                      # 4.617e-07
}
GRAD_FLOORS['conditioned'] = {
    'pose': {'main': 1.2e-05, 'small:0.0001': 5.4e-04, 'small:0.001': 9.3e-05, 'small:0.01': 2.0e-05, 'small:1e-06': 1.1e-05, 'small:single': 6.1e-06, 'small:zero': 5.7e-06},
    # 1.137e-05, 5.351e-04, 9.219e-05, 1.999e-05, 1.095e-05, 6.086e-06, 5.654e-06
    'betas': {'all': 9.5e-07},      # 9.428e-07
    'trans': {'all': 1.9e-06},      # 1.865e-06
    'scale': {'all': 1.8e-05},      # 1.773e-05
}


def fwd_tol(model, key, name):
    return FLOOR_FACTOR * FWD_FLOOR[model][key][name]


def grad_tol(model, name, grp):
    return FLOOR_FACTOR * GRAD_FLOORS[model][name][grp if name == 'pose' else 'all']


class single_thread:
    """The fp32 restatement on one thread: its rounding then does not depend on how many cores the machine has."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def measure_forward_floor(m32, ref64, fr):
    with single_thread():
        return forward_errors(forward_outputs(m32, fr), ref64)


def reference_gradients(m, fr, mut=None):
    """{variant: gradients} of the general route (every input requires a gradient; the root route's are the same numbers)."""
    return {v: gradients(reference_call(m, mut), fr, v, 'general', dtype_of(m)) for v in VARIANTS}


def measure_grad_floor(m32, g64, fr):
    """{name: {group: floor}}: the fp32 restatement's gradients against the fp64 ones, worst over the six variants."""
    acc = {}
    with single_thread():
        g32 = reference_gradients(m32, fr)
    for v in VARIANTS:
        for name, (err, _) in grad_errors(g32[v], g64[v]).items():
            for grp, e in worst_by_group(name, err, fr['label']).items():
                acc.setdefault(name, {})[grp] = max(acc.get(name, {}).get(grp, 0.0), e)
    return acc


def _round_up(x):
    if x == 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e, 12)


if __name__ == '__main__':          # the floors behind FWD_FLOOR and GRAD_FLOORS on this machine's CPU build of torch
    import tempfile
    asset_root = build.ensure_synthetic_assets(os.environ.get('GLAMR_ASSET_ROOT') or tempfile.mkdtemp())
    fr, gfr = frames(FWD_B), frames(GRAD_B, GRAD_FAMILIES)
    for name in MODELS:
        root = model_root(name, asset_root, tempfile.mkdtemp())
        m64, m32 = reference(root), reference(root, torch.float32)
        f = measure_forward_floor(m32, forward_outputs(m64, fr), fr)
        print("FWD_FLOOR[%r] = {" % name)
        for k in FWD_KEYS:
            print("    %r: {%s},        # %s" % (k, ', '.join('%r: %.1e' % (n, _round_up(e)) for n, e in f[k].items()), ', '.join('%.3e' % e for e in f[k].values())))
        print('}')
        g = measure_grad_floor(m32, reference_gradients(m64, gfr), gfr)
        print("GRAD_FLOORS[%r] = {" % name)
        for k in ('pose', 'betas', 'trans', 'scale'):
            print("    %r: {%s}," % (k, ', '.join('%r: %.1e' % (grp, _round_up(e)) for grp, e in sorted(g[k].items()))))
            print("    # %s" % ', '.join('%.3e' % e for _, e in sorted(g[k].items())))
        print('}')
