"""Shared by tests/test_init_ref.py (CPU) and tests/test_init_gpu.py (MI355X): a numpy float64 restatement of the four entry points of
glamr_amd/csrc/init.hip -- glamr_init_prepare, glamr_init_scenes_ex (+ glamr_init_scatter_pose), glamr_init_cam_all_frames, glamr_check_inputs --
written from what GlobalReconOptimizer.init_data does (global_recon_model.py:76-317 of the reference, pinned by oracle/port): scipy's
Rotation.from_matrix(..).as_rotvec() and interp1d(.., assume_sorted=True, fill_value='extrapolate') on float64 copies of the float32 inputs, the
kornia / torch_transform operators in numpy at float64.  Also: builders of the raw batch arrays (slots, T, ...) of every test case, the float32
port run on the same cases with the same prior outputs, D_REF -- the port's own distance to the float64 restatement per case and compared array,
the basis of every tolerance (tol = 4 d_ref + 1 float32 ulp of the array's largest value) -- and the launch helpers, one entry point each.

`python -m tests.init_ref_common` prints the D_REF table from scratch."""
import ctypes
import numpy as np

F64 = np.float64
ULP = float(np.finfo(np.float32).eps)             # spacing of float32 at 1: ulp(x) <= ULP * |x|
PI_ULP = 2.4e-7                                   # one float32 ulp at pi
NEAR_PI = 1e-3                                    # rotation vectors this close to angle pi are compared as rotation matrices ...
NEAR_PI_TOL = 5e-7                                # ... at this bound
TOL_FACTOR = 4
ILL_HEADING, ILL_COS = 0.2, 0.98                  # interpolated heading vector shorter than / interpolated 6D columns closer to parallel than
BASE = np.array([0.5, 0.5, 0.5, 0.5])
MUTATIONS = ('extrap_pair', 'quat_branch', 'no_wflip', 'inv34', 'base_heading', 'dh_origin', 'rel_ij', 'kp_remap', 'nets_shift')


def ulp_of(a):
    return ULP * float(np.abs(a).max()) if np.size(a) else 0.0


def tol_of(d_ref, ref):
    return TOL_FACTOR * d_ref + ulp_of(ref)


# =====================================================================================================================================
# operators (lib/utils/konia_transform.py, lib/utils/torch_transform.py, traj_pred/utils/traj_utils.py), float64 numpy, quaternions (w, x, y, z)
# =====================================================================================================================================

def _sdiv(num, den, eps=1e-6):
    return num / np.where(np.abs(den) < eps, den + eps, den)


def safe_atan2(y, x, eps=1e-6):
    tiny = (np.abs(y) < eps) & (np.abs(x) < eps)
    return np.arctan2(np.where(tiny, y + eps, y), x)


def aa_to_rotmat(aa):
    v = np.asarray(aa, F64).reshape(-1, 3)
    th2 = (v * v).sum(-1, keepdims=True)
    th = np.sqrt(np.maximum(th2, 1e-6))
    w = v / (th + 1e-6)
    wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    c, s = np.cos(th), np.sin(th)
    k = 1.0 - c
    normal = np.concatenate([c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k, wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k,
                             -wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k], 1)
    rx, ry, rz = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    one = np.ones_like(rx)
    taylor = np.concatenate([one, -rz, ry, rz, one, -rx, -ry, rx, one], 1)
    return np.where(th2 > 1e-6, normal, taylor).reshape(np.shape(aa)[:-1] + (3, 3))


def rotmat_to_quat(R, eps=1e-6):
    m = np.asarray(R, F64).reshape(np.shape(R)[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i:i + 1] for i in range(9)]
    tr = m00 + m11 + m22
    sq = np.sqrt(np.maximum(tr + 1.0, eps)) * 2.0
    q_tr = np.concatenate([0.25 * sq, _sdiv(m21 - m12, sq), _sdiv(m02 - m20, sq), _sdiv(m10 - m01, sq)], -1)
    sq = np.sqrt(np.maximum(1.0 + m00 - m11 - m22, eps)) * 2.0
    q_x = np.concatenate([_sdiv(m21 - m12, sq), 0.25 * sq, _sdiv(m01 + m10, sq), _sdiv(m02 + m20, sq)], -1)
    sq = np.sqrt(np.maximum(1.0 + m11 - m00 - m22, eps)) * 2.0
    q_y = np.concatenate([_sdiv(m02 - m20, sq), _sdiv(m01 + m10, sq), 0.25 * sq, _sdiv(m12 + m21, sq)], -1)
    sq = np.sqrt(np.maximum(1.0 + m22 - m00 - m11, eps)) * 2.0
    q_z = np.concatenate([_sdiv(m10 - m01, sq), _sdiv(m02 + m20, sq), _sdiv(m12 + m21, sq), 0.25 * sq], -1)
    inner = np.where(m11 > m22, q_y, q_z)
    mid = np.where((m00 > m11) & (m00 > m22), q_x, inner)
    return np.where(tr > 0.0, q_tr, mid)


def quat_to_rotmat(q):
    q = np.asarray(q, F64)
    qn = q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-12)
    w, x, y, z = [qn[..., i] for i in range(4)]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    return np.stack([1.0 - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w, ty * x + tz * w, 1.0 - (tx * x + tz * z), tz * y - tx * w,
                     tz * x - ty * w, tz * y + tx * w, 1.0 - (tx * x + ty * y)], -1).reshape(q.shape[:-1] + (3, 3))


def quat_to_aa(q, eps=1e-6):
    c, q1, q2, q3 = [np.asarray(q, F64)[..., i] for i in range(4)]
    s2 = q1 * q1 + q2 * q2 + q3 * q3
    s = np.sqrt(np.maximum(s2, eps))
    two_theta = 2.0 * np.where(c < 0.0, safe_atan2(-s, -c), safe_atan2(s, c))
    k = np.where(s2 > 0.0, _sdiv(two_theta, s, eps), 2.0)
    return np.stack([q1 * k, q2 * k, q3 * k], -1)


def aa_to_quat(aa, eps=1e-6):
    aa = np.asarray(aa, F64)
    th2 = (aa * aa).sum(-1, keepdims=True)
    th = np.sqrt(np.maximum(th2, eps))
    pos = th2 > 0.0
    k = np.where(pos, _sdiv(np.sin(th * 0.5), th, eps), 0.5)
    return np.concatenate([np.where(pos, np.cos(th * 0.5), 1.0), aa * k], -1)


def quat_mul(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F64), np.asarray(b, F64))
    w1, x1, y1, z1 = [a[..., i] for i in range(4)]
    w2, x2, y2, z2 = [b[..., i] for i in range(4)]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_conj(q):
    return np.asarray(q, F64) * np.array([1.0, -1.0, -1.0, -1.0])


def unit(x, eps=1e-9):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), eps)


def sixd_to_rotmat(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = unit(a1)
    b2 = unit(a2 - (b1 * a2).sum(-1, keepdims=True) * b1)
    return np.stack([b1, b2, np.cross(b1, b2)], -1)


def rotmat_to_6d(R):
    return np.concatenate([R[..., 0], R[..., 1]], -1)


def make_transform(R, trans):
    M = np.zeros(R.shape[:-2] + (4, 4))
    M[..., :3, :3], M[..., :3, 3], M[..., 3, 3] = R, trans, 1.0
    return M


def invert_transform(M, mut=None):
    out = np.zeros_like(M)
    out[..., :3, :3] = np.swapaxes(M[..., :3, :3], -1, -2)
    out[..., :3, 3] = -M[..., :3, 3] if mut == 'inv34' else -np.einsum('...j,...ji->...i', M[..., :3, 3], M[..., :3, :3])
    out[..., 3, 3] = 1.0
    return out


def heading_of(q):
    return 2 * safe_atan2(q[..., 3], q[..., 0])


def heading_quat_of(q):
    z = np.zeros_like(q[..., 0])
    return unit(np.stack([q[..., 0], z, z, q[..., 3]], -1))


def heading_to_quat(theta):
    z = np.zeros_like(theta)
    return aa_to_quat(np.stack([z, z, theta], -1))


def heading_to_vec(theta):
    return np.stack([np.cos(theta), np.sin(theta)], -1)


def flat34(M):
    return M[..., :3, :].reshape(M.shape[:-2] + (12,))


def rodrigues(r):
    """Exact exponential map, for comparing rotation vectors as rotations."""
    r = np.asarray(r, F64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -r[..., 2], r[..., 1], r[..., 2], -r[..., 0], -r[..., 1], r[..., 0]
    a = np.where(th < 1e-8, 1.0, np.sin(th) / np.where(th < 1e-8, 1.0, th))
    b = np.where(th < 1e-8, 0.5, (1 - np.cos(th)) / np.where(th < 1e-8, 1.0, th * th))
    return np.eye(3) + a * K + b * (K @ K)


def rotvec(M, mut=None):
    """scipy Rotation.from_matrix(M).as_rotvec() (global_recon_model.py:105-108).  The mutated variants restate scipy's algorithm (nearest rotation by
    SVD, quaternion from the dominant of (m00, m11, m22, trace), positive-w canonical form) with one defect."""
    M = np.asarray(M, F64).reshape(-1, 3, 3)
    if mut not in ('quat_branch', 'no_wflip', 'manual'):
        from scipy.spatial.transform import Rotation
        return Rotation.from_matrix(M).as_rotvec()
    U, _, Vt = np.linalg.svd(M)
    X = U @ Vt
    tr = np.trace(X, axis1=1, axis2=2)
    choice = np.argmax(np.stack([X[:, 0, 0], X[:, 1, 1], X[:, 2, 2], tr], -1), -1)
    q = np.zeros((len(X), 4))                      # (x, y, z, w)
    for n in range(len(X)):
        i = choice[n]
        if i == 3:
            q[n] = (X[n, 2, 1] - X[n, 1, 2], X[n, 0, 2] - X[n, 2, 0], X[n, 1, 0] - X[n, 0, 1], 1 + tr[n])
        else:
            j, k = (i + 1) % 3, (i + 2) % 3
            if mut == 'quat_branch' and i == 1:
                j, k = k, j
            q[n, i], q[n, j], q[n, k], q[n, 3] = 1 - tr[n] + 2 * X[n, i, i], X[n, j, i] + X[n, i, j], X[n, k, i] + X[n, i, k], X[n, k, j] - X[n, j, k]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if mut != 'no_wflip':
        q[q[:, 3] < 0] *= -1
    s = np.linalg.norm(q[:, :3], axis=1)
    angle = 2 * np.arctan2(s, q[:, 3])
    small = angle <= 1e-3
    scale = np.where(small, 2 + angle ** 2 / 12 + 7 * angle ** 4 / 2880, angle / np.where(small, 1.0, np.sin(angle / 2)))
    return q[:, :3] * scale[:, None]


def interp(idx, y, n, mut=None, x_dtype=F64):
    """interp1d(idx, y, axis=0, assume_sorted=True, fill_value='extrapolate') on arange(n).  A single point (what filter_pose can leave; scipy
    refuses it) is held constant.  x_dtype float32 with float32 y is the reference's own arithmetic (:132-136)."""
    from scipy.interpolate import interp1d
    y = np.asarray(y)
    if len(idx) == 1:
        return np.repeat(y[:1], n, 0)
    out = interp1d(np.asarray(idx).astype(x_dtype), y, axis=0, assume_sorted=True, fill_value='extrapolate')(np.arange(n, dtype=x_dtype))
    if mut == 'extrap_pair' and len(idx) > 2:      # frames beyond the last point continue the line through the two points before it
        a, b = idx[-3], idx[-2]
        for t in range(idx[-1] + 1, n):
            out[t] = y[-2] + (y[-2] - y[-3]) * ((t - b) / (b - a))
    return out


def interp_orient_sep_heading(q_vis, vis):
    """traj_utils.py:120-141.  Returns the interpolated quaternions and the frames at which the interpolation is ill-conditioned."""
    q = quat_mul(q_vis, quat_conj(BASE))
    hq = heading_quat_of(q)
    hvec = heading_to_vec(heading_of(q))
    loc6 = rotmat_to_6d(quat_to_rotmat(quat_mul(quat_conj(hq), q)))
    idx = np.flatnonzero(vis)
    hv, l6 = interp(idx, hvec, len(vis)), interp(idx, loc6, len(vis))
    a1, a2 = l6[:, :3], l6[:, 3:]
    cosang = np.abs((a1 * a2).sum(-1)) / np.maximum(np.linalg.norm(a1, axis=-1) * np.linalg.norm(a2, axis=-1), 1e-300)
    ill = (np.linalg.norm(hv, axis=-1) < ILL_HEADING) | (cosang > ILL_COS)
    qi = quat_mul(heading_to_quat(safe_atan2(hv[:, 1], hv[:, 0])), rotmat_to_quat(sixd_to_rotmat(l6)))
    return quat_mul(qi, BASE), ill


def local_heading_cols(q, mut=None):
    """Columns 9-10 of traj_global2local_heading (traj_utils.py:44-62): (cos, sin) of the per-frame heading change, row 0 absolute."""
    if mut != 'base_heading':
        q = quat_mul(q, quat_conj(BASE))
    h = heading_of(q)
    return heading_to_vec(np.concatenate([h[:1], h[1:] - h[:-1]]))


# =====================================================================================================================================
# the four entry points
# =====================================================================================================================================

def kp_map():
    from oracle.port.grecon import SMPL_TO_BODY26FK
    return np.asarray(SMPL_TO_BODY26FK)


def filter_pose(orient_cam, visible):
    """global_recon_model.py:250-262"""
    q = aa_to_quat(orient_cam)
    w = quat_mul(q[1:], quat_conj(q[:-1]))[:, 0]
    jump = np.arccos(np.clip(2 * w * w - 1, -1 + 1e-6, 1 - 1e-6))
    ind = np.flatnonzero((jump > np.pi / 3) & (visible[1:] != 0)) + 1
    for i in ind:
        if visible[i - 1]:
            if i + 1 < len(q) and visible[i + 1] and (i + 1) not in ind:
                visible[i - 1] = 0
            else:
                visible[i] = 0


def ref_prepare(raw, filter=True, mut=None):
    """glamr_init_prepare: (slots, T, ...) float64 arrays, rows at or beyond seq_len and empty slots zero."""
    n_slots, T = raw['exist'].shape
    z = lambda *s: np.zeros((n_slots, T) + s)
    o = dict(visible_orig=z(), visible=z(), smpl_pose=z(69), smpl_beta=z(10), orient_cam=z(3), trans_cam=z(3), kp_2d=z(26, 2), kp_score=z(26),
             base_orient=z(3), base_trans=z(3), nets_pose=z(69), nets_vis=z(), fr_start=np.zeros(n_slots, np.int64), fr_end=np.ones(n_slots, np.int64),
             detected=np.zeros((n_slots, T), bool))
    m = kp_map()
    src = np.roll(m[:, 1], 1) if mut == 'kp_remap' else m[:, 1]
    for s in range(n_slots):
        n = int(raw['seq_len'][s])
        idx = np.flatnonzero(raw['exist'][s, :n])
        if len(idx) < 2:
            continue
        fs, fe = idx[0], idx[-1] + 1
        o['fr_start'][s], o['fr_end'][s] = fs, fe
        o['visible_orig'][s, :n] = o['visible'][s, :n] = raw['exist'][s, :n]
        o['detected'][s, idx] = True
        aa = rotvec(raw['rot'][s, idx], mut).reshape(len(idx), 72)
        vals = [aa, raw['betas'][s, idx].astype(F64), raw['trans'][s, idx].astype(F64)]
        if len(idx) < n:
            vals = [interp(idx, v, n, mut) for v in vals]
        o['orient_cam'][s, :n], o['smpl_pose'][s, :n], o['smpl_beta'][s, :n], o['trans_cam'][s, :n] = vals[0][:, :3], vals[0][:, 3:], vals[1], vals[2]
        kp = raw['kp'][s, idx].reshape(len(idx), 24, 2).astype(F64)
        o['kp_2d'][s, idx[:, None], m[None, :, 0]] = kp[:, src]
        o['kp_score'][s, idx[:, None], m[None, :, 0]] = 1.0
        if filter:
            filter_pose(o['orient_cam'][s, :n], o['visible'][s, :n])
        o['base_orient'][s, :n] = quat_to_aa(rotmat_to_quat(aa_to_rotmat(o['orient_cam'][s, :n])))
        o['base_trans'][s, :n] = o['trans_cam'][s, :n]
        if mut == 'nets_shift':
            o['nets_pose'][s, fs:fe], o['nets_vis'][s, fs:fe] = o['smpl_pose'][s, fs:fe], o['visible'][s, fs:fe]
        else:
            o['nets_pose'][s, :fe - fs], o['nets_vis'][s, :fe - fs] = o['smpl_pose'][s, fs:fe], o['visible'][s, fs:fe]
    return o


SCENE_INPUTS = ('visible', 'orient_cam', 'trans_cam', 'base_orient', 'base_trans', 'smpl_pose', 'fr_start', 'fr_end')


def ref_scenes(geo, prep, priors, flags=0, mut=None):
    """glamr_init_scenes_ex on the outputs of the preparation (any float type; computed in float64) and the prior outputs (rows [0, n) of a slot).
    flags: 1 = GLAMR_INIT_TRAJ_FROM_CAM.  Also returns `ill` (slots, T): frames whose interpolated heading is ill-conditioned, and `zero_cam` (S)."""
    S, P, T = geo['S'], geo['P'], geo['T']
    f = lambda k: np.asarray(prep[k], F64).copy()
    vis, oc, tc = f('visible'), f('orient_cam'), f('trans_cam')
    o = dict(smpl_pose=f('smpl_pose'), base_orient=f('base_orient'), base_trans=f('base_trans'), traj_local_pred=np.zeros((S * P, T, 11)),
             person2cam=np.zeros((S * P, T, 12)), rel_transform_cam=np.zeros((S, P, P, T, 12)), cam_pose=np.zeros((S, T, 12)),
             ill=np.zeros((S * P, T), bool), zero_cam=np.zeros(S, bool), fr_start=np.asarray(prep['fr_start']), fr_end=np.asarray(prep['fr_end']))
    for si in range(S):
        n, np_ = int(geo['seq_len'][si]), int(geo['n_persons'][si])
        ptc = {}
        for p in range(np_):
            s = si * P + p
            fs, fe = int(prep['fr_start'][s]), int(prep['fr_end'][s])
            o['smpl_pose'][s, fs:fe], o['base_orient'][s, fs:fe], o['base_trans'][s, fs:fe] = (priors[k][s, :fe - fs] for k in ('n_pose', 'n_orient', 'n_trans'))
            o['traj_local_pred'][s, :fe - fs] = priors['n_local'][s, :fe - fs]
            ptc[p] = make_transform(aa_to_rotmat(oc[s, :n]), tc[s, :n])
            o['person2cam'][s, :n] = flat34(invert_transform(ptc[p], mut))
        for i in range(np_):
            for j in range(np_):
                if i != j:
                    a, b = (j, i) if mut == 'rel_ij' else (i, j)
                    o['rel_transform_cam'][si, i, j, :n] = flat34(invert_transform(ptc[a]) @ ptc[b])
        # initial camera from the first person at the first frame anybody is seen in (:294-317)
        s0 = si * P
        start = np.flatnonzero((vis[s0:s0 + np_, :n] == 1).any(0))[0]
        cand = make_transform(aa_to_rotmat(o['base_orient'][s0, start]), o['base_trans'][s0, start]) @ invert_transform(ptc[0][start]) * float(vis[s0, start] == 1)
        o['zero_cam'][si] = vis[s0, start] != 1
        cand[:3, :3] = sixd_to_rotmat(rotmat_to_6d(cand[:3, :3]))
        o['cam_pose'][si, :n] = flat34(invert_transform(cand))
        # heading of the trajectory prior from the camera (:273-292), base pose off the camera outside the existence range (:325-351)
        for p in range(np_):
            s = si * P + p
            fs, fe = int(prep['fr_start'][s]), int(prep['fr_end'][s])
            w = cand @ ptc[p]
            v = vis[s, :n] == 1
            qi, o['ill'][s, :n] = interp_orient_sep_heading(rotmat_to_quat(w[v][:, :3, :3]), v)
            cols = local_heading_cols(qi[fs:fe] if mut == 'dh_origin' else qi, mut)
            o['traj_local_pred'][s, :fe - fs, 9:] = cols if mut == 'dh_origin' else cols[fs:fe]
            if flags & 1:
                out = np.ones(n, bool)
                out[fs:fe] = False
                o['base_orient'][s, :n][out], o['base_trans'][s, :n][out] = quat_to_aa(qi)[out], w[out][:, :3, 3]
    return o


def ref_cam_all_frames(geo, vis, person2cam, orient_world, trans_world):
    """init_cam_pose(all_frames=True) on the frames the first person is seen in: (S, T, 12) float64 and the mask (S, T) of those frames."""
    S, P, T = geo['S'], geo['P'], geo['T']
    out, seen = np.zeros((S, T, 12)), np.zeros((S, T), bool)
    for si in range(S):
        n, s0 = int(geo['seq_len'][si]), si * P
        p2c = np.zeros((n, 4, 4))
        p2c[:, :3, :], p2c[:, 3, 3] = np.asarray(person2cam[s0, :n], F64).reshape(n, 3, 4), 1.0
        inf = make_transform(aa_to_rotmat(np.asarray(orient_world[s0, :n], F64)), np.asarray(trans_world[s0, :n], F64)) @ p2c
        inf[:, :3, :3] = sixd_to_rotmat(rotmat_to_6d(inf[:, :3, :3]))
        out[si, :n], seen[si, :n] = flat34(invert_transform(inf)), vis[s0, :n] == 1
    return out, seen


def port_cam_all_frames(geo, vis, person2cam, orient_world, trans_world):
    """The float32 port's init_cam_pose(all_frames=True), for the frames no float64 statement exists for (zero matrices re-orthonormalised)."""
    import torch
    from oracle.port import grecon, transforms as tf
    S, P, T = geo['S'], geo['P'], geo['T']
    out = np.zeros((S, T, 12), np.float32)
    for si in range(S):
        n, s0, np_ = int(geo['seq_len'][si]), si * P, int(geo['n_persons'][si])
        p2c = torch.zeros((n, 4, 4))
        p2c[:, :3, :], p2c[:, 3, 3] = torch.from_numpy(np.ascontiguousarray(person2cam[s0, :n], np.float32)).view(n, 3, 4), 1.0
        v = torch.from_numpy(vis[s0:s0 + np_, :n] == 1)
        first = {'person_transform_world': tf.make_transform(torch.from_numpy(np.ascontiguousarray(orient_world[s0, :n], np.float32)),
                                                             torch.from_numpy(np.ascontiguousarray(trans_world[s0, :n], np.float32)), 'axis_angle'),
                 'person2cam': p2c, 'vis_frames': v[0]}
        data = {'person_data': {0: first}, 'fr_num_persons': v.sum(0), 'cam_pose': torch.zeros((n, 4, 4)), 'cam_pose_inv': torch.zeros((n, 4, 4))}
        grecon.GlobalReconOptimizer.init_cam_pose(None, data, all_frames=True)
        out[si, :n] = data['cam_pose'][:, :3, :].reshape(n, 12).numpy()
    return out


def ref_check_inputs(raw, K):
    """glamr_check_inputs: (2, slots) -- [0] a detected frame holds a matrix with |R R^T - I| > 1e-2 (or not comparable), [1] a non-finite value."""
    n_slots, T = raw['exist'].shape
    v = np.zeros((2, n_slots), np.int32)
    for s in range(n_slots):
        for t in np.flatnonzero(raw['exist'][s]):
            R = raw['rot'][s, t].reshape(24, 3, 3).astype(F64)
            with np.errstate(invalid='ignore'):
                g = np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3))
                v[0, s] |= int(not (g <= 1e-2).all())
            v[1, s] |= int(not all(np.isfinite(a).all() for a in (raw['rot'][s, t], raw['betas'][s, t], raw['trans'][s, t], raw['kp'][s, t], K[s, t])))
    return v


# =====================================================================================================================================
# test cases: raw batch arrays (slots, T, ...), float32, built directly
# =====================================================================================================================================

def _axis_rot(axis, angle):
    return rodrigues(np.asarray(axis, F64) / np.linalg.norm(axis) * angle)


def special_rotations(rng):
    """The matrices of the preparation case, float64: the three non-trace quaternion branches at {1e-2, 1e-4, 1e-6} from pi (both signs of the
    extracted w), the trace branch, the series switch of the rotation vector at 1e-3 +- 1e-5 and 1e-8; each clean and with element noise that brings
    |R R^T - I| to 9e-3 (the admission bound of glamr_check_inputs is 1e-2)."""
    mats = []
    for d in (1e-2, 1e-4, 1e-6):
        for k in range(3):
            for sign in (1.0, -1.0):
                ax = rng.uniform(-0.35, 0.35, 3)
                ax[k] = sign
                mats.append(_axis_rot(ax, np.pi - d))
    for _ in range(12):
        mats.append(_axis_rot(rng.normal(size=3), rng.uniform(0.1, 2.0)))
    for a in (1e-3 + 1e-5, 1e-3 - 1e-5, 1e-8):
        mats.append(_axis_rot(rng.normal(size=3), a))
    noisy = []
    for R in mats:
        N = rng.uniform(-1, 1, (3, 3))
        e = np.abs((R + N) @ (R + N).T - np.eye(3)).max()       # grows (almost) linearly with the scale of N: two secant steps
        sc = 1.0
        for _ in range(30):
            e = np.abs((R + sc * N) @ (R + sc * N).T - np.eye(3)).max()
            sc *= 9e-3 / e
        noisy.append(R + sc * N)
    return np.stack(mats + noisy)


def _walker(rng, T, heading, cam_tilt=0.04):
    """Camera-frame root rotation / translation of an upright person with the given world heading per frame, seen by a static camera, and its
    world pose (what the trajectory prior would return).  The layout of glamr_amd.utils.synth.make_in_dict."""
    t = np.arange(T) / 30.0
    R0 = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]]) @ _axis_rot([1, 0, 0], cam_tilt)
    base_r = np.array([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]])
    z3 = np.zeros(T)
    sway = rodrigues(0.05 * np.stack([np.sin(1.1 * t + rng.uniform(0, 6)), np.sin(0.7 * t + 1.0), z3], 1))
    Rw = rodrigues(np.stack([z3, z3, heading], 1)) @ base_r @ sway
    xy = np.cumsum(np.stack([np.cos(heading), np.sin(heading)], 1) * 0.02, 0) + rng.uniform(-1, 1, 2)
    tw = np.concatenate([xy, 0.92 + 0.02 * np.sin(9 * t)[:, None]], 1)
    return R0.T @ Rw, (tw - np.array([-4.2, 0.0, 1.3])) @ R0, Rw, tw


def _empty_raw(S, P, T):
    f = lambda *s: np.full((S * P, T) + s, np.nan, np.float32)        # rows without a detection hold NaN: nothing may read them
    return dict(seq_len=np.zeros(S * P, np.int32), exist=np.zeros((S * P, T), np.float32), rot=f(24, 9), betas=f(10), trans=f(3), kp=f(48),
                K=np.zeros((S * P, T, 9), np.float32))


def _geo(S, P, T, n_persons, seq_len):
    return dict(S=S, P=P, T=T, n_persons=np.asarray(n_persons, np.int32), seq_len=np.asarray(seq_len, np.int32))


def _fill_person(raw, s, n_fr, det, rng, heading, specials=None, jump=None):
    """Slot s: detections at frames `det`; smooth root rotation, body joints drawn round-robin from `specials` (or generic)."""
    T = raw['exist'].shape[1]
    Rc, tc, Rw, tw = _walker(rng, T, heading)
    raw['seq_len'][s] = n_fr
    raw['exist'][s, det] = 1.0
    rot = np.zeros((T, 24, 3, 3))
    rot[:, 0] = Rc
    if jump is not None:                             # frames [a, b) turned about the body's own up axis
        rot[jump[0]:jump[1], 0] = rot[jump[0]:jump[1], 0] @ _axis_rot([0, 1, 0], jump[2])
    for t in range(T):
        for j in range(1, 24):
            rot[t, j] = specials[(t * 23 + j + 7 * s) % len(specials)] if specials is not None else _axis_rot(rng.normal(size=3), rng.uniform(0.0, 1.2))
    raw['rot'][s, det] = rot[det].reshape(len(det), 24, 9)
    raw['betas'][s, det] = rng.normal(size=(len(det), 10)) * 0.5
    raw['trans'][s, det] = tc[det] + rng.normal(size=(len(det), 3)) * 0.01
    raw['kp'][s, det] = rng.uniform(0, 1900, (len(det), 48))
    K = np.array([1000, 0, 960, 0, 1000, 540, 0, 0, 1], np.float32)
    raw['K'][s, det] = K
    return Rw, tw


def _heading(rng, T, turn=None):
    t = np.arange(T) / 30.0
    h = 0.3 * np.sin(0.9 * t + rng.uniform(0, 6.28)) + rng.uniform(-0.4, 0.4)
    if turn is not None:                             # turns by `angle` over frames [a, b]
        a, b, angle = turn
        h = h + angle * np.clip((np.arange(T) - a) / (b - a), 0, 1)
    return h


def _frames(*ranges, drop=()):
    return np.array([t for a, b in ranges for t in range(a, b) if t not in drop], np.int64)


def _priors(rng, geo, raw, world):
    """Random arrays in place of the networks' outputs (rows [0, n) of each slot); orientation and translation near the walker's world pose so that
    the initial camera is a plausible one."""
    n_slots, T = raw['exist'].shape
    pr = dict(n_pose=rng.normal(size=(n_slots, T, 69)) * 0.3, n_local=rng.normal(size=(n_slots, T, 11)), n_trans=np.zeros((n_slots, T, 3)), n_orient=np.zeros((n_slots, T, 3)))
    for s, (Rw, tw) in world.items():
        idx = np.flatnonzero(raw['exist'][s])
        fs, n = idx[0], idx[-1] + 1 - idx[0]
        pr['n_orient'][s, :n] = rotvec(Rw[fs:fs + n] @ rodrigues(rng.normal(size=(n, 3)) * 0.02))
        pr['n_trans'][s, :n] = tw[fs:fs + n] + rng.normal(size=(n, 3)) * 0.01
    return {k: v.astype(np.float32) for k, v in pr.items()}


def build_case(name):
    """-> dict(geo, raw, priors, filter).  Every case is one batch."""
    rng = np.random.default_rng({'prep': 11, 'prep300': 12, 'single': 13, 'scene': 14, 'synth': 15}[name])
    world = {}
    if name == 'prep':
        # T = 40, three slots per scene, one of them empty in scenes 0 and 2; scene 2 is shorter than the batch (33 frames)
        S, P, T = 3, 3, 40
        geo, raw = _geo(S, P, T, [2, 3, 2], [40, 40, 33]), _empty_raw(S, P, T)
        sp = special_rotations(rng)
        plan = {0: (40, _frames((0, 40))),                                      # all frames detected
                1: (40, _frames((5, 34), drop=(9, 11, 12, 20))),                # first detection at frame 5, one-frame gaps, a two-frame gap, gap at the end
                3: (40, np.array([4, 34])),                                     # exactly two detections, 30 frames apart
                4: (40, _frames((0, 12), (25, 40))),
                5: (40, _frames((0, 40), drop=(1, 38))),                        # one-frame gaps next to both ends
                6: (33, _frames((3, 30), drop=(4,))),                           # gap at the start and at the end, seq_len < T
                7: (33, _frames((0, 33)))}                                      # all of a shorter sequence
        for s, (n, det) in plan.items():
            world[s] = _fill_person(raw, s, n, det, rng, _heading(rng, T), specials=sp)
    elif name == 'prep300':
        S, P, T = 1, 1, 300                                                     # the 256-thread loops take a second trip
        geo, raw = _geo(S, P, T, [1], [300]), _empty_raw(S, P, T)
        world[0] = _fill_person(raw, 0, 300, _frames((3, 120), (150, 290), drop=(260, 270)), rng, _heading(rng, T), specials=special_rotations(rng))
    elif name == 'single':
        # person 1 is detected in frames 10 and 11 only, turned by 90 degrees between them: filter_pose leaves frame 10 alone
        S, P, T = 1, 2, 40
        geo, raw = _geo(S, P, T, [2], [40]), _empty_raw(S, P, T)
        world[0] = _fill_person(raw, 0, 40, _frames((0, 40), drop=(20, 21)), rng, _heading(rng, T))
        world[1] = _fill_person(raw, 1, 40, np.array([10, 11]), rng, _heading(rng, T), jump=(11, T, np.pi / 2))
    elif name == 'scene':
        # T = 48, scenes of 1, 2 and 3 persons padded to 3; scene 2 is 45 frames long
        S, P, T = 3, 3, 48
        geo, raw = _geo(S, P, T, [1, 2, 3], [48, 48, 45]), _empty_raw(S, P, T)
        # scene 0: the heading turns by 3.3 rad (plus its own swing) across the visibility gap [15, 31): the interpolated heading vector passes near the origin
        world[0] = _fill_person(raw, 0, 48, _frames((0, 15), (31, 48)), rng, _heading(rng, T, turn=(14, 31, 3.3)))
        # scene 1: person 1 exists in [7, 39)
        world[3] = _fill_person(raw, 3, 48, _frames((0, 48), drop=(22, 23, 24)), rng, _heading(rng, T))
        world[4] = _fill_person(raw, 4, 48, _frames((7, 39), drop=(20,)), rng, _heading(rng, T))
        # scene 2: person 0 is detected from frame 0 but turned by 90 degrees there, so filter_pose drops that frame; person 1 is seen in it -- the
        # zero camera (the product of person 0's world pose and person->camera transform at frame 0, a generic matrix, times its visibility 0)
        world[6] = _fill_person(raw, 6, 45, _frames((0, 45)), rng, _heading(rng, T), jump=(0, 1, np.pi / 2))
        world[7] = _fill_person(raw, 7, 45, _frames((0, 40), drop=(10, 11)), rng, _heading(rng, T))
        world[8] = _fill_person(raw, 8, 45, _frames((11, 45)), rng, _heading(rng, T))
    elif name == 'synth':
        return synth_case()
    else:
        raise KeyError(name)
    return dict(name=name, geo=geo, raw=raw, priors=_priors(rng, geo, raw, world), filter=True)


def synth_case():
    """Two ordinary scenes of glamr_amd.utils.synth.make_in_dict (100 frames; one with two persons, person 1 trimmed to [17, 83)) as one raw batch."""
    from glamr_amd.utils import synth
    md = synth.make_smpl_model()
    dicts = [synth.make_in_dict(seed=3, num_frames=100, num_persons=1, smpl_model=md),
             synth.trim_person(synth.make_in_dict(seed=5, num_frames=100, num_persons=2, smpl_model=md), 1, 17, 83)]
    S, P, T = 2, 2, 100
    geo, raw = _geo(S, P, T, [1, 2], [100, 100]), _empty_raw(S, P, T)
    for si, d in enumerate(dicts):
        for p, src in d['est'].items():
            s, det = si * P + p, np.flatnonzero(src['bboxes_dict']['exist'])
            raw['seq_len'][s] = T
            raw['exist'][s, det] = 1.0
            for k, key, w in (('rot', 'smpl_pose_quat_wroot', 216), ('betas', 'smpl_beta', 10), ('trans', 'root_trans', 3), ('K', 'cam_K', 9)):
                raw[k][s, det] = src[key].reshape(raw[k][s, det].shape)
            raw['kp'][s, det] = src['kp_2d'][:, :24].reshape(len(det), 48)
    rng = np.random.default_rng(16)
    n_slots = S * P
    pr = dict(n_pose=rng.normal(size=(n_slots, T, 69)) * 0.3, n_local=rng.normal(size=(n_slots, T, 11)), n_trans=rng.normal(size=(n_slots, T, 3)),
              n_orient=rng.normal(size=(n_slots, T, 3)) * 0.8)
    return dict(name='synth', geo=geo, raw=raw, priors={k: v.astype(np.float32) for k, v in pr.items()}, filter=True)


def to_in_dicts(case):
    """The raw batch as the dictionaries GlobalReconOptimizer.init_data takes (pose_est/hybrik_demo/demo.py:317-354)."""
    geo, raw, out = case['geo'], case['raw'], []
    for si in range(geo['S']):
        est = {}
        for p in range(int(geo['n_persons'][si])):
            s, n = si * geo['P'] + p, int(geo['seq_len'][si])
            det = np.flatnonzero(raw['exist'][s, :n])
            est[p] = {'bboxes_dict': {'exist': raw['exist'][s, :n].astype(np.float64)}, 'smpl_pose_quat_wroot': raw['rot'][s, det].reshape(len(det), -1, 4).copy(),
                      'smpl_beta': raw['betas'][s, det].copy(), 'root_trans': raw['trans'][s, det].copy(), 'kp_2d': raw['kp'][s, det].reshape(len(det), 24, 2).copy(),
                      'cam_K': raw['K'][s, det].reshape(len(det), 3, 3).copy()}
        out.append({'est': est, 'gt': {}, 'gt_meta': {}, 'seq_name': 'case%d' % si})
    return out


# =====================================================================================================================================
# the float32 port (oracle/port, pinned to the reference) on a case, with the same prior outputs
# =====================================================================================================================================

def run_port(case, world=None):
    """oracle.port's init_data per scene with the case's prior outputs in place of the networks.  Returns float32 arrays in the batch layout:
    the outputs of the preparation under 'prep', those of the scene initialisation under 'scene', plus 'cam_pose_all' (flag_init_cam_all_frames;
    `world` = (orient_world, trans_world) replaces the world poses it starts from, None: the port's own).  A scene holding a person with a single
    visible frame is skipped (its rows stay zero, 'skipped' names it): scipy's interp1d has no answer for one point."""
    import torch
    from oracle.port import grecon, transforms as tf
    geo, pri = case['geo'], case['priors']
    S, P, T = geo['S'], geo['P'], geo['T']
    n_slots = S * P
    z = lambda *s: np.zeros((n_slots, T) + s, np.float32)
    prep = dict(visible_orig=z(), visible=z(), smpl_pose=z(69), smpl_beta=z(10), orient_cam=z(3), trans_cam=z(3), kp_2d=z(26, 2), kp_score=z(26),
                base_orient=z(3), base_trans=z(3), nets_pose=z(69), nets_vis=z(), fr_start=np.zeros(n_slots, np.int64), fr_end=np.ones(n_slots, np.int64))
    scene = dict(smpl_pose=z(69), base_orient=z(3), base_trans=z(3), traj_local_pred=z(11), person2cam=z(12), rel_transform_cam=np.zeros((S, P, P, T, 12), np.float32),
                 cam_pose=np.zeros((S, T, 12), np.float32), traj_cam_orient=z(3), traj_cam_trans=z(3))
    cam_all = np.zeros((S, T, 12), np.float32)
    skipped = []
    npy = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)

    class SingleFrame(Exception):
        pass

    class Nets:
        def inference(self, batch, sample_num=1):
            s = self.order.pop(0)
            n = batch['in_body_pose'].shape[1]
            prep['nets_pose'][s, :n], prep['nets_vis'][s, :n] = npy(batch['in_body_pose'][0]), npy(batch['frame_mask'][0])
            t = lambda k: torch.from_numpy(pri[k][s, :n].copy())
            return {'infer_out_body_pose': t('n_pose')[None, None], 'infer_out_local_traj_tp': t('n_local')[:, None, None], 'infer_out_orient': t('n_orient')[None, None],
                    'infer_out_trans': t('n_trans')[None, None]}

    class Port(grecon.GlobalReconOptimizer):
        def infer_motion_traj(self, d):
            s = self.mt_model.order[0]
            n = len(npy(d['visible']))
            for k, key in (('smpl_pose', 'smpl_pose'), ('base_orient', 'smpl_orient_world_base'), ('base_trans', 'root_trans_world_base'), ('visible', 'visible'),
                           ('visible_orig', 'visible_orig'), ('smpl_beta', 'smpl_beta'), ('orient_cam', 'smpl_orient_cam'), ('trans_cam', 'root_trans_cam'),
                           ('kp_2d', 'kp_2d'), ('kp_score', 'kp_2d_score')):
                prep[k][s, :n] = npy(d[key])
            prep['fr_start'][s], prep['fr_end'][s] = int(d['fr_start']), int(d['fr_end'])
            super().infer_motion_traj(d)

        def init_cam_pose(self, data, all_frames=False):
            si, n = self.si, data['cam_pose'].shape[0]
            for p, d in data['person_data'].items():
                s = si * P + p
                if not all_frames:
                    scene['base_orient'][s, :n], scene['base_trans'][s, :n] = npy(d['smpl_orient_world_base']), npy(d['root_trans_world_base'])
                elif p == 0 and world is not None:
                    d['person_transform_world'] = tf.make_transform(torch.from_numpy(world[0][s, :n].copy()), torch.from_numpy(world[1][s, :n].copy()), 'axis_angle')
            super().init_cam_pose(data, all_frames)
            (cam_all if all_frames else scene['cam_pose'])[si, :n] = npy(data['cam_pose'])[:, :3, :].reshape(n, 12)
            if not all_frames:        # get_traj_from_cam (:325-351) with the port's operators
                if any(int(d['vis_frames'].sum()) < 2 for d in data['person_data'].values()):
                    raise SingleFrame()
                for p, d in data['person_data'].items():
                    s = si * P + p
                    w = torch.matmul(data['cam_pose_inv'], d['person_transform_cam'])
                    qi = tf.interp_orient_sep_heading(tf.rotmat_to_quat(w[:, :3, :3].contiguous())[d['vis_frames']], d['vis_frames'])
                    scene['traj_cam_orient'][s, :n], scene['traj_cam_trans'][s, :n] = npy(tf.quat_to_aa(qi)), npy(w[:, :3, 3])

        def forward(self, data, opt_variables, opt_meta):
            pass

    nets = Nets()
    specs = dict(flag_infer_motion_traj=True, flag_pred_traj=True, est_type='hybrik', flag_filter_pose=bool(case['filter']), flag_init_cam_all_frames=True)
    port = Port({'grecon_model_specs': specs, 'opt_stage_specs': {}}, None, nets)
    for si, in_dict in enumerate(to_in_dicts(case)):
        port.si = si
        nets.order = [si * P + p for p in in_dict['est']]
        try:
            data = port.init_data(in_dict)
        except SingleFrame:
            skipped.append(si)
            continue
        n = data['seq_len']
        for p, d in data['person_data'].items():
            s = si * P + p
            fs, fe = int(d['fr_start']), int(d['fr_end'])
            scene['smpl_pose'][s, :n] = npy(d['smpl_pose'])
            scene['traj_local_pred'][s, :fe - fs] = npy(d['traj_local_pred'])
            scene['person2cam'][s, :n] = npy(d['person2cam'])[:, :3, :].reshape(n, 12)
        for (i, j), M in (data['rel_transform_cam'] or {}).items():
            scene['rel_transform_cam'][si, i, j, :n] = npy(M)[:, :3, :].reshape(n, 12)
    return dict(prep=prep, scene=scene, cam_pose_all=cam_all, skipped=skipped)


def world_poses(case):
    """Random world poses of every slot, the inputs of glamr_init_cam_all_frames."""
    rng = np.random.default_rng(77)
    n_slots, T = case['raw']['exist'].shape
    return (rng.normal(size=(n_slots, T, 3)) * 0.8).astype(np.float32), rng.normal(size=(n_slots, T, 3)).astype(np.float32)


# =====================================================================================================================================
# comparisons: which values of which array, measured the same way for the port (d_ref) and for the kernels
# =====================================================================================================================================

def rot_err(a, b):
    """Largest element difference of the rotations of two arrays of rotation vectors."""
    return np.abs(rodrigues(a) - rodrigues(b)).max((-1, -2))


def row_mask(geo, per_slot=True):
    """Rows below seq_len of real persons (slots, T), or of scenes (S, T)."""
    S, P, T = geo['S'], geo['P'], geo['T']
    m = np.arange(T)[None] < np.asarray(geo['seq_len'])[:, None]
    if not per_slot:
        return m
    return (m[:, None, :] & (np.arange(P)[None] < np.asarray(geo['n_persons'])[:, None])[:, :, None]).reshape(S * P, T)


def prep_errors(got, ref, geo):
    """{array: (error, reference values compared)} of the preparation.  Slots detected in every frame hold the converted rotation vectors as they are
    ('pose det': elementwise, away from angle pi; 'pose pi': within NEAR_PI of it, as rotations).  Every frame of a slot with a gap, the detected ones
    too, is an output of the interpolation (interp1d evaluated AT a point returns (y_hi - y_lo) + y_lo in float32): the array names."""
    rows = row_mask(geo)
    n_det, nonempty = ref['detected'].sum(1), ref['visible_orig'].sum(1) > 0
    whole = (n_det == np.repeat(np.asarray(geo['seq_len']), geo['P'])) & nonempty            # slots detected in every frame: no interpolation
    det, itp = ref['detected'] & rows & whole[:, None], rows & (nonempty & ~whole)[:, None]
    full_ref = np.concatenate([ref['orient_cam'], ref['smpl_pose']], -1).reshape(ref['orient_cam'].shape[:2] + (24, 3))
    full_got = np.concatenate([got['orient_cam'], got['smpl_pose']], -1).astype(F64).reshape(full_ref.shape)
    near = det[..., None] & (np.linalg.norm(full_ref, axis=-1) > np.pi - NEAR_PI)
    e = {}
    d = np.abs(full_got - full_ref)
    far = det[..., None] & ~near
    e['pose det'] = (float(d[far].max()) if far.any() else 0.0, full_ref[far])
    e['pose pi'] = (float(rot_err(full_got[near], full_ref[near]).max()) if near.any() else 0.0, np.ones(1))
    for k in ('orient_cam', 'smpl_pose', 'smpl_beta', 'trans_cam', 'base_trans'):
        m = itp if k != 'base_trans' else rows
        e[k] = (float(np.abs(got[k].astype(F64) - ref[k])[m].max()) if m.any() else 0.0, ref[k][m])
    e['base_orient'] = (float(rot_err(got['base_orient'][rows], ref['base_orient'][rows]).max()), np.ones(1))
    fs_fe = [(int(a), int(b)) for a, b in zip(ref['fr_start'], ref['fr_end'])]
    m = np.zeros(rows.shape, bool)
    for s, (a, b) in enumerate(fs_fe):
        m[s, :b - a] = ref['visible_orig'][s].sum() > 0
    e['nets_pose'] = (float(np.abs(got['nets_pose'].astype(F64) - ref['nets_pose'])[m].max()), ref['nets_pose'][m])
    return e


PREP_EXACT = ('kp_2d', 'kp_score', 'visible_orig', 'visible', 'fr_start', 'fr_end', 'nets_vis')


def scene_errors(got, ref, geo, flag_ref=None):
    """{array: (error, reference values compared)} of the scene initialisation.  Camera-dependent arrays leave out the zero-camera scenes (compared with
    the port instead) and, for the heading columns, the ill-conditioned frames and their successors.  flag_ref: the reference of a
    GLAMR_INIT_TRAJ_FROM_CAM run -- adds the base pose of the frames outside the existence ranges."""
    S, P, T = geo['S'], geo['P'], geo['T']
    rows, srows = row_mask(geo), row_mask(geo, False)
    cam_ok = np.repeat(~ref['zero_cam'], P)[:, None] & rows
    e = {}
    ab = lambda k, m: (float(np.abs(np.asarray(got[k], F64) - ref[k])[m].max()) if m.any() else 0.0, ref[k][m])
    e['person2cam'] = ab('person2cam', rows)
    e['rel_transform_cam'] = ab('rel_transform_cam', np.broadcast_to(srows[:, None, None], (S, P, P, T)))
    e['cam_pose'] = ab('cam_pose', srows & ~ref['zero_cam'][:, None])
    e['smpl_pose'] = ab('smpl_pose', rows)
    e['base_trans'] = ab('base_trans', rows)
    e['base_orient'] = (float(rot_err(np.asarray(got['base_orient'], F64)[rows], ref['base_orient'][rows]).max()), np.ones(1))
    e['traj 0-8'] = (float(np.abs(np.asarray(got['traj_local_pred'], F64) - ref['traj_local_pred'])[..., :9].max()), ref['traj_local_pred'][..., :9])
    m = np.zeros((S * P, T), bool)                     # rows e of traj_local_pred whose frames fs + e and fs + e - 1 are well-conditioned
    for s in range(S * P):
        fs, fe = int(ref['fr_start'][s]), int(ref['fr_end'][s])
        if cam_ok[s, 0]:
            bad = ref['ill'][s].copy()
            bad[1:] |= ref['ill'][s, :-1]
            m[s, :fe - fs] = ~bad[fs:fe]
    e['traj 9-10'] = (float(np.abs(np.asarray(got['traj_local_pred'], F64) - ref['traj_local_pred'])[..., 9:][m].max()), np.ones(1))
    if flag_ref is not None:
        out = cam_ok & ~ref['ill']
        for s in range(S * P):
            out[s, int(ref['fr_start'][s]):int(ref['fr_end'][s])] = False
        e['flag base_trans'] = (float(np.abs(np.asarray(got['flag_base_trans'], F64) - flag_ref['base_trans'])[out].max()) if out.any() else 0.0, flag_ref['base_trans'][out])
        e['flag base_orient'] = (float(rot_err(np.asarray(got['flag_base_orient'], F64)[out], flag_ref['base_orient'][out]).max()) if out.any() else 0.0, np.ones(1))
    return e


def skipped_share(ref, geo):
    """Share of a case's frames (rows below seq_len of real persons, zero-camera scenes aside) the heading comparison leaves out."""
    rows = row_mask(geo) & np.repeat(~ref['zero_cam'], geo['P'])[:, None]
    return float((ref['ill'] & rows).sum()) / max(1, int(rows.sum()))


def references(case):
    """The float64 outputs of every entry point on a case, computed once: prep, the float32 inputs of the scene kernel made from it, scene without and
    with GLAMR_INIT_TRAJ_FROM_CAM, and the all-frames cameras from world_poses()."""
    prep = ref_prepare(case['raw'], case['filter'])
    f32 = {k: (prep[k].astype(np.float32) if prep[k].dtype == F64 else prep[k]) for k in SCENE_INPUTS}
    scene, scene_flag = ref_scenes(case['geo'], f32, case['priors']), ref_scenes(case['geo'], f32, case['priors'], flags=1)
    ow, tw = world_poses(case)
    p2c32 = scene['person2cam'].astype(np.float32)
    cam_all, seen = ref_cam_all_frames(case['geo'], f32['visible'], p2c32, ow, tw)
    return dict(prep=prep, scene_inputs=f32, scene=scene, scene_flag=scene_flag, cam_all=cam_all, cam_all_seen=seen, person2cam32=p2c32, world=(ow, tw))


def measure_d_ref(case, refs=None):
    """The float32 port's distance to the float64 restatement, per compared array of the case: {'prep': {...}, 'scene': {...}, 'cam_all': x}.  A scene
    the port cannot run (a single visible frame) takes no part; the case 'single' measures the other scenes' arrays only where one remains."""
    refs = refs or references(case)
    geo = case['geo']
    port = run_port(case, refs['world'])
    assert not port['skipped'] or case['name'] == 'single'
    out = {'prep': {k: v[0] for k, v in prep_errors(port['prep'], refs['prep'], geo).items()}}
    if port['skipped']:
        # the scene arrays of 'single' are measured with filter_pose off (the port then runs: person 1 keeps its two detections).  person2cam,
        # rel_transform_cam, cam_pose and the base pose are the same functions of the same values either way; the heading columns are the float32
        # arithmetic of the same visible frames, linearly extrapolated there and held constant here.
        case = dict(case, filter=False)
        refs, port = references(case), run_port(case, refs['world'])
    got = dict(port['scene'], flag_base_trans=port['scene']['traj_cam_trans'], flag_base_orient=port['scene']['traj_cam_orient'])
    out['scene'] = {k: v[0] for k, v in scene_errors(got, refs['scene'], geo, refs['scene_flag']).items()}
    out['cam_all'] = float(np.abs(port['cam_pose_all'].astype(F64) - refs['cam_all'])[refs['cam_all_seen']].max())
    return out


def tolerance(case_name, stage, key, ref_values):
    """The bound of one compared array: the issue's fixed bounds for the converted rotation vectors, 4 d_ref + 1 ulp of the largest value otherwise."""
    if key == 'pose det':
        return PI_ULP
    if key == 'pose pi':
        return NEAR_PI_TOL
    d = D_REF[case_name][stage]
    return tol_of(d if key is None else d[key], ref_values)


# the port's distance to float64 (measure_d_ref), printed by `python -m tests.init_ref_common`; tests/test_init_ref.py measures it again and asserts
# every entry within [1/2, 2] x (the largest of ~1e4 float32 roundings moves by that much between libm / BLAS builds, not more)
D_REF = {'prep': {'cam_all': 2.92e-06,
          'prep': {'base_orient': 8.21e-07,
                   'base_trans': 2.38e-07,
                   'nets_pose': 4.51e-07,
                   'orient_cam': 4.79e-07,
                   'pose det': 1.19e-07,
                   'pose pi': 1.17e-07,
                   'smpl_beta': 3.28e-07,
                   'smpl_pose': 2.14e-06,
                   'trans_cam': 2.38e-07},
          'scene': {'base_orient': 9.34e-07,
                    'base_trans': 5.96e-08,
                    'cam_pose': 7.29e-07,
                    'flag base_orient': 1.24e-06,
                    'flag base_trans': 7.77e-07,
                    'person2cam': 2.06e-06,
                    'rel_transform_cam': 9.4e-07,
                    'smpl_pose': 1.91e-06,
                    'traj 0-8': 0.0,
                    'traj 9-10': 6.14e-07}},
 'prep300': {'cam_all': 4.77e-06,
             'prep': {'base_orient': 1.65e-06,
                      'base_trans': 4.77e-07,
                      'nets_pose': 4.17e-07,
                      'orient_cam': 1.66e-06,
                      'pose det': 0.0,
                      'pose pi': 0.0,
                      'smpl_beta': 8.94e-07,
                      'smpl_pose': 5.11e-06,
                      'trans_cam': 4.77e-07},
             'scene': {'base_orient': 1.66e-06,
                       'base_trans': 0.0,
                       'cam_pose': 7.72e-07,
                       'flag base_orient': 3.52e-06,
                       'flag base_trans': 1.93e-06,
                       'person2cam': 4.49e-06,
                       'rel_transform_cam': 0.0,
                       'smpl_pose': 3.81e-06,
                       'traj 0-8': 0.0,
                       'traj 9-10': 9.05e-07}},
 'scene': {'cam_all': 1.73e-06,
           'prep': {'base_orient': 2.43e-06,
                    'base_trans': 2.38e-07,
                    'nets_pose': 1.77e-07,
                    'orient_cam': 2.38e-06,
                    'pose det': 1.18e-07,
                    'pose pi': 8.24e-08,
                    'smpl_beta': 1.31e-06,
                    'smpl_pose': 1.44e-06,
                    'trans_cam': 2.38e-07},
           'scene': {'base_orient': 2.53e-06,
                     'base_trans': 0.0,
                     'cam_pose': 6.99e-07,
                     'flag base_orient': 2.13e-06,
                     'flag base_trans': 5.95e-07,
                     'person2cam': 3.2e-06,
                     'rel_transform_cam': 2.35e-06,
                     'smpl_pose': 1.91e-06,
                     'traj 0-8': 0.0,
                     'traj 9-10': 6.95e-07}},
 'single': {'cam_all': 1.37e-06,
            'prep': {'base_orient': 3.96e-06,
                     'base_trans': 1.59e-07,
                     'nets_pose': 9.57e-08,
                     'orient_cam': 3.94e-06,
                     'pose det': 0.0,
                     'pose pi': 0.0,
                     'smpl_beta': 2e-06,
                     'smpl_pose': 2.89e-06,
                     'trans_cam': 1.59e-07},
            'scene': {'base_orient': 3.98e-06,
                      'base_trans': 0.0,
                      'cam_pose': 6.72e-07,
                      'flag base_orient': 2.34e-06,
                      'flag base_trans': 1.27e-06,
                      'person2cam': 2.23e-05,
                      'rel_transform_cam': 5.85e-06,
                      'smpl_pose': 3.81e-06,
                      'traj 0-8': 0.0,
                      'traj 9-10': 5.68e-07}},
 'synth': {'cam_all': 2.75e-06,
           'prep': {'base_orient': 4.86e-06,
                    'base_trans': 2.27e-07,
                    'nets_pose': 2.47e-08,
                    'orient_cam': 5.41e-06,
                    'pose det': 0.0,
                    'pose pi': 0.0,
                    'smpl_beta': 0.0,
                    'smpl_pose': 1.97e-07,
                    'trans_cam': 2.27e-07},
           'scene': {'base_orient': 4.84e-06,
                     'base_trans': 0.0,
                     'cam_pose': 6.18e-07,
                     'flag base_orient': 1.54e-06,
                     'flag base_trans': 4.97e-07,
                     'person2cam': 8.17e-06,
                     'rel_transform_cam': 8.09e-06,
                     'smpl_pose': 1.94e-07,
                     'traj 0-8': 0.0,
                     'traj 9-10': 2.97e-06}}}


# =====================================================================================================================================
# launch helpers (MI355X): each calls exactly one entry point
# =====================================================================================================================================

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _raw_struct(raw):
    from glamr_amd import _lib
    n_slots, T = raw['exist'].shape
    keep = {k: _dev(raw[k]) for k in ('seq_len', 'exist', 'rot', 'betas', 'trans', 'kp', 'K')}
    rb = _lib.RawBatch()
    rb.n_slots, rb.max_len = n_slots, T
    for name, k in (('seq_len', 'seq_len'), ('exist', 'exist'), ('rotmats', 'rot'), ('betas', 'betas'), ('root_trans', 'trans'), ('kp_2d', 'kp')):
        setattr(rb, name, ctypes.c_void_p(keep[k].data_ptr()))
    return rb, keep


def _scene_batch(geo, fill=None):
    import torch
    from glamr_amd.global_recon import packing
    S, P, T = geo['S'], geo['P'], geo['T']
    packed = packing.PackedScenes.empty(S, P, T, torch.device('cuda:0'), with_rel=True)
    packed.t['n_persons'].copy_(_dev(geo['n_persons']))
    packed.t['seq_len'].copy_(_dev(geo['seq_len']))
    packed.t['j_local'] = torch.zeros(1, device='cuda:0')
    for k, v in (fill or {}).items():
        packed.t[k].copy_(_dev(np.asarray(v, np.float32 if packed.t[k].dtype == torch.float32 else np.int32)).view(packed.t[k].shape))
    return packed


def _person_arrays(geo, fill=None):
    import torch
    from glamr_amd import _lib
    from glamr_amd.global_recon import packing
    n, T = geo['S'] * geo['P'], geo['T']
    t = packing.carve_zeros([('visible_orig', torch.float32, (n, T)), ('smpl_pose', torch.float32, (n, T, 69)), ('smpl_beta', torch.float32, (n, T, 10)),
                             ('trans_cam', torch.float32, (n, T, 3)), ('nets_pose', torch.float32, (n, T, 69)), ('nets_vis', torch.float32, (n, T))], torch.device('cuda:0'))
    for k, v in (fill or {}).items():
        t[k].copy_(_dev(np.asarray(v, np.float32)))
    pa = _lib.PersonArrays()
    for k, ten in t.items():
        setattr(pa, k, ctypes.c_void_p(ten.data_ptr()))
    return pa, t


def _workspace(geo):
    import torch
    from glamr_amd import _lib
    return torch.zeros(_lib.lib().glamr_init_workspace_bytes(geo['S'] * geo['P'], geo['T']), dtype=torch.uint8, device='cuda:0')


def _host(t):
    return t.detach().cpu().numpy().copy()


def launch_prepare(case):
    """glamr_init_prepare on the raw batch -> its outputs as numpy arrays named like ref_prepare's."""
    import torch
    from glamr_amd import _lib
    geo = case['geo']
    rb, keep = _raw_struct(case['raw'])
    packed, (pa, pt), ws = _scene_batch(geo), _person_arrays(geo), _workspace(geo)
    sb = packed.struct()
    fo = _lib.FilterOpts(int(bool(case['filter'])), 0, 0.0, 0)
    _lib.check(_lib.lib().glamr_init_prepare(ctypes.byref(rb), ctypes.byref(sb), ctypes.byref(pa), ctypes.byref(fo), _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    out = {k: _host(pt[k]) for k in ('visible_orig', 'smpl_pose', 'smpl_beta', 'trans_cam', 'nets_pose', 'nets_vis')}
    out.update({k: _host(packed.t[k]) for k in ('orient_cam', 'kp_2d', 'kp_score', 'base_orient', 'base_trans', 'fr_start', 'fr_end')})
    out['visible'] = _host(packed.t['vis'])
    return out


def _scene_setup(geo, inp):
    packed = _scene_batch(geo, dict(vis=inp['visible'], orient_cam=inp['orient_cam'], base_orient=inp['base_orient'], base_trans=inp['base_trans'],
                                    fr_start=inp['fr_start'], fr_end=inp['fr_end']))
    pa, pt = _person_arrays(geo, dict(trans_cam=inp['trans_cam'], smpl_pose=inp['smpl_pose']))
    return packed, pa, pt


def launch_scenes(geo, inp, priors, flags=0):
    """glamr_init_scenes_ex on the (float32) outputs of a preparation and the prior outputs."""
    import torch
    from glamr_amd import _lib
    packed, pa, pt = _scene_setup(geo, inp)
    ws, sb = _workspace(geo), packed.struct()
    pr = {k: _dev(v) for k, v in priors.items()}
    _lib.check(_lib.lib().glamr_init_scenes_ex(ctypes.byref(sb), ctypes.byref(pa), _lib.ptr(pr['n_pose']), _lib.ptr(pr['n_local']), _lib.ptr(pr['n_trans']),
                                               _lib.ptr(pr['n_orient']), int(flags), _lib.ptr(ws), _lib.current_stream()))
    torch.cuda.synchronize()
    out = {k: _host(packed.t[k]) for k in ('base_orient', 'base_trans', 'traj_local_pred', 'person2cam', 'rel_transform_cam', 'cam_pose')}
    out['smpl_pose'] = _host(pt['smpl_pose'])
    return out


def launch_scatter_pose(geo, inp, priors):
    """glamr_init_scatter_pose alone -> smpl_pose."""
    import torch
    from glamr_amd import _lib
    packed, pa, pt = _scene_setup(geo, inp)
    sb, n_pose = packed.struct(), _dev(priors['n_pose'])
    _lib.check(_lib.lib().glamr_init_scatter_pose(ctypes.byref(sb), ctypes.byref(pa), _lib.ptr(n_pose), _lib.current_stream()))
    torch.cuda.synchronize()
    return _host(pt['smpl_pose'])


def launch_cam_all_frames(geo, vis, person2cam, orient_world, trans_world, prefill):
    """glamr_init_cam_all_frames -> cam_pose (S, T, 12); `prefill` is what cam_pose holds before the launch."""
    import torch
    from glamr_amd import _lib
    packed = _scene_batch(geo, dict(vis=vis, person2cam=person2cam, orient_world=orient_world, trans_world=trans_world, cam_pose=prefill))
    sb = packed.struct()
    _lib.check(_lib.lib().glamr_init_cam_all_frames(ctypes.byref(sb), _lib.current_stream()))
    torch.cuda.synchronize()
    return _host(packed.t['cam_pose'])


def launch_check_inputs(raw):
    """glamr_check_inputs -> verdict (2, slots)."""
    import torch
    from glamr_amd import _lib
    rb, keep = _raw_struct(raw)
    verdict = torch.full((2, raw['exist'].shape[0]), -1, dtype=torch.int32, device='cuda:0')
    _lib.check(_lib.lib().glamr_check_inputs(ctypes.byref(rb), _lib.ptr(keep['K']), _lib.ptr(verdict), _lib.current_stream()))
    torch.cuda.synchronize()
    return _host(verdict)


def check_inputs_raw():
    """2 slots x 7 frames of valid values (14 rows: not a multiple of the 4 rows of a block); slot 0 frame 3 is undetected."""
    rng = np.random.default_rng(21)
    raw = _empty_raw(1, 2, 7)
    for k in ('rot', 'betas', 'trans', 'kp'):
        raw[k][:] = 0.0
    raw['seq_len'][:] = 7
    raw['exist'][:] = 1.0
    raw['exist'][0, 3] = 0.0
    raw['rot'][:] = rodrigues(rng.normal(size=(2, 7, 24, 3))).reshape(2, 7, 24, 9)
    raw['betas'][:], raw['trans'][:], raw['kp'][:] = rng.normal(size=(2, 7, 10)), rng.normal(size=(2, 7, 3)), rng.uniform(0, 1900, (2, 7, 48))
    raw['K'][:] = np.array([1000, 0, 960, 0, 1000, 540, 0, 0, 1], np.float32)
    return raw


# (array, flat index within a frame's row) at every boundary of the kernel's hand-written lane map: rotation lanes 0 and 23 (first and last element), keypoint
# values 0 / 39 (lanes 24 / 63) and 40 / 47 (the second trip, lanes 0 / 7), the last beta, translation and intrinsics value
CHECK_INJECTIONS = (('rot', 0), ('rot', 23 * 9 + 8), ('kp', 0), ('kp', 39), ('kp', 40), ('kp', 47), ('betas', 9), ('trans', 2), ('K', 8))


def threshold_matrices():
    """[(3x3 float32, fails the 1e-2 orthonormality check)]: one Gram entry at 0.0099 / 0.0101, off the diagonal and on it, built in float64; the
    float32 matrix is on the intended side by 9e-5, a thousand float32 roundings."""
    out = []
    for a in (0.0099, 0.0101):
        for M in (np.array([[1, 0, 0], [a, np.sqrt(1 - a * a), 0], [0, 0, 1.0]]), np.diag([np.sqrt(1 + a), 1.0, 1.0])):
            M32 = M.astype(np.float32)
            g = np.abs(M32.astype(F64) @ M32.astype(F64).T - np.eye(3)).max()
            assert abs(g - a) < 1e-6 and abs(g - 1e-2) > 9e-5
            out.append((M32, a > 1e-2))
    return out


CASES = ('prep', 'prep300', 'single', 'scene')

if __name__ == '__main__':
    import pprint
    pprint.pprint({name: {k: ({a: float('%.2e' % b) for a, b in v.items()} if isinstance(v, dict) else float('%.2e' % v)) for k, v in measure_d_ref(build_case(name)).items()}
                   for name in CASES + ('synth',)}, width=170)
