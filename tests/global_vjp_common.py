"""fp64 reference of the local-to-global step's vector-Jacobian product, the product glamr_traj_local_to_global_backward computes: torch
autograd of oracle.port.transforms.local_to_global_traj followed by quat_to_aa, for L = sum(G_t * trans) + sum(G_o * orient) + sum(G_q * orient_q)
per sequence.  Inputs, screening, upstream patterns, mutations and tolerances of tests/test_global_vjp_ref.py (CPU: the algorithm of
csrc/traj_global_bwd.hpp on the host runtime) and tests/test_global_vjp_gpu.py (the kernel).

Tolerances follow the project's rule: FLOOR_FACTOR = 16 x the error of the SAME autograd run in float32 against float64, relative to the
largest reference entry of the sequence, separately for the column groups 0-1, 2, 3-8 and 9-10; per case the worst over its sequences and
upstream patterns.  The floors are constants below (`python -m tests.global_vjp_common` prints them); the CPU test measures them again and
fails outside [1/2, 2] x the constant.  A floor of exactly 0 (column 2 is a copy of g_trans's z; one frame's columns 0-1 are g_trans's own
x, y) asks for the exact result."""
import numpy as np
import torch

from oracle.port import transforms as tf

FLOOR_FACTOR = 16
GROUPS = {'xy': slice(0, 2), 'z': slice(2, 3), 'rot': slice(3, 9), 'heading': slice(9, 11)}
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 513)      # the scan's lane, wave and 256-thread chunk boundaries, and three chunks
BATCHES = {'ragged3': (64, 257, 3), 'ragged5': (513, 1, 255, 300, 65)}      # padded to the longest
PATTERNS = ('all', 'trans', 'orient', 'orient_q', 'onehot')
MARGIN = 1e-3            # every branch condition of rotmat_to_quat / quat_to_aa at least this far from switching in the fp64 forward ...
MARGIN_NEAR_PI = 1e-5    # ... except the sign condition `c < 0` of quat_to_aa on the frames PLACED within 1e-4 of angle pi (|c| ~ 5e-5: with the
#                          1e-3 margin the family could not exist); those frames sit in sequences whose heading stays small, so fp32 and fp64
#                          agree on the branch by two orders of magnitude
CANDIDATES = 4           # seeds tried per case; the first that passes the screening is the case
MAX_DROPPED_SHARE = 0.25

MUTATIONS = {'no_suffix': 'no suffix sum of the heading gradient', 'no_dR': 'dR/dtheta term of the displacement dropped',
             'theta_t': 'theta_t instead of theta_{t-1} in the rotation of row t', 'row0': 'row 0 rotated',
             'aa_as_vec': 'g_orient taken as the quaternion\'s vector part (no quat_to_aa_bwd)', 'pad_rows': 'rows at or beyond the length counted'}


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _qmul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def _q2R(q):
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def _aa2q(axis, angle):
    return np.concatenate([np.cos(angle / 2)[..., None], axis * np.sin(angle / 2)[..., None]], axis=-1)


def _raw6(R, rng):
    """Un-normalised 6D rows of rotation matrices R (k,3,3): the first two columns, each scaled, the second with a share of the first."""
    k = R.shape[0]
    a1 = R[:, :, 0] * rng.uniform(0.6, 1.5, (k, 1))
    a2 = R[:, :, 1] * rng.uniform(0.6, 1.5, (k, 1)) + R[:, :, 0] * rng.uniform(-0.3, 0.3, (k, 1))
    return np.concatenate([a1, a2], axis=-1)


def sequence(n, seed, kind):
    """One sequence of n local rows (n, 11) fp32 and the mask (n,) of its frames placed within 1e-4 of angle pi.  kind: bit 0 = large turns
    (up to +-2 rad per frame, one sign, so the running heading passes hundreds of radians; else decoder-like heading vectors of non-unit
    length near (1, 0)), bit 1 = some heading vectors of length 1e-3.  Frames are dealt to the families in runs: decoder-like rows, 6D rows
    for each of rotmat_to_quat's four branches (8 frames each from 64 frames on, one from 5 on), world orientations within 1e-2 and (small headings only)
    1e-4 of angle pi, one row with dxy = 0."""
    rng = np.random.default_rng(1000 + seed)
    turny, tiny = bool(kind & 1), bool(kind & 2)
    L = np.zeros((n, 11))
    L[:, :2] = 0.03 * rng.normal(size=(n, 2))
    L[:, 2] = 0.9 + 0.05 * rng.normal(size=n)
    if turny:
        ang = rng.uniform(0.5, 2.0, n) * (1 if seed % 4 < 2 else -1)
        flip = rng.random(n) < 0.1
        ang[flip] = -ang[flip]
        L[:, 9:] = rng.uniform(0.5, 1.5, (n, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    else:
        L[:, 9:] = np.stack([1.0 + 0.1 * rng.normal(size=n), 0.05 * rng.normal(size=n)], axis=-1)
    if tiny:
        idx = rng.permutation(n)[:max(1, n // 16)]
        L[idx, 9:] = 1e-3 * _unit(L[idx, 9:])
    L[:, 9:] = L[:, 9:].astype(np.float32)
    # families of the 6D rows: 0 decoder-like (raw rows around the identity: branch 0, trace > 0), 1-3 one of rotmat_to_quat's other branches,
    # 4 / 5 a WORLD orientation within 1e-2 / 1e-4 of angle pi (the local rotation that gives q_w = heading (x) local (x) base)
    theta = np.cumsum(np.arctan2(L[:, 10].astype(np.float64), L[:, 9].astype(np.float64)))
    order = rng.permutation(n)
    run = 8 if n >= 64 else (1 if n >= 5 else 0)
    fam = np.zeros(n, int)
    for k, f in enumerate((1, 2, 3, 4) + (() if turny else (5,))):
        fam[order[k * run:(k + 1) * run]] = f
    base_c = np.array([0.5, -0.5, -0.5, -0.5])

    def draw(f, idx):
        k = len(idx)
        if f == 0:
            return (np.array([1.0, 0, 0, 0, 1.0, 0]) + 0.2 * rng.normal(size=(k, 6))) * rng.uniform(0.7, 1.3, (k, 1))
        if f <= 3:
            axis = np.zeros((k, 3))
            axis[:, f - 1] = 1.0
            return _raw6(_q2R(_aa2q(_unit(axis + 0.2 * rng.normal(size=axis.shape)), rng.uniform(2.4, 3.0, k))), rng)
        lo, hi = ((4e-3, 1e-2), (2.5e-5, 1e-4))[f - 4]
        qw = _aa2q(_unit(rng.normal(size=(k, 3))), np.pi - rng.uniform(lo, hi, k) * rng.choice([-1.0, 1.0], k))
        hq_c = np.stack([np.cos(theta[idx] / 2), 0.0 * idx, 0.0 * idx, -np.sin(theta[idx] / 2)], axis=-1)
        return _raw6(_q2R(_qmul(_qmul(hq_c, qw), base_c)), rng)

    # a frame whose draw lands within twice the screening margin of a branch condition is drawn again (the case is still screened as a whole)
    todo = np.arange(n)
    for _ in range(8):
        for f in range(6):
            idx = todo[fam[todo] == f]
            if len(idx):
                L[idx, 3:9] = draw(f, idx).astype(np.float32)
        todo = np.nonzero(frame_margins(L, fam == 5) < 2.0)[0]
        if len(todo) == 0:
            break
    near = fam == 5
    if n >= 2:
        L[n // 2, :2] = 0.0
    return L.astype(np.float32), near


def frame_margins(L32, near, want_branch=False):
    """Distance of every branch condition of rotmat_to_quat and quat_to_aa from switching in the fp64 forward of one sequence, per frame and
    relative to its bound (>= 1 passes the screening)[, the rotmat_to_quat branch per frame]."""
    L = torch.tensor(np.asarray(L32, np.float64))
    m = tf.sixd_to_rotmat(L[:, 3:9]).reshape(-1, 9).numpy()
    m00, m11, m22 = m[:, 0], m[:, 4], m[:, 8]
    tr = m00 + m11 + m22
    first = np.minimum(m00 - m11, m00 - m22)                 # > 0: branch 1
    br = np.where(tr > 0, 0, np.where(first > 0, 1, np.where(m11 > m22, 2, 3)))
    marg = np.abs(tr)
    low = tr <= 0
    marg = np.where(low, np.minimum(marg, np.abs(first)), marg)
    marg = np.where(low & (first <= 0), np.minimum(marg, np.abs(m11 - m22)), marg)
    # the chosen candidate's clamp (sqrt argument against eps) and its safe divisions (|2 sqrt| against eps)
    arg = np.select([br == 0, br == 1, br == 2], [tr + 1.0, 1.0 + m00 - m11 - m22, 1.0 + m11 - m00 - m22], 1.0 + m22 - m00 - m11)
    marg = np.minimum(marg, arg - 1e-6)
    _, q = tf.local_to_global_traj(L)
    q = q.numpy()
    c, s2 = q[:, 0], (q[:, 1:] ** 2).sum(-1)
    rel = np.minimum(marg, s2 - 1e-6) / MARGIN                    # s2 > 0, its clamp at eps and the division by s
    rel = np.minimum(rel, np.abs(c) / np.where(near, MARGIN_NEAR_PI, MARGIN))
    return (rel, br) if want_branch else rel


def branch_margins(L32, near):
    """(smallest frame margin of the sequence, the rotmat_to_quat branch per frame)"""
    rel, br = frame_margins(L32, near, want_branch=True)
    return float(rel.min()), br


def _case_specs():
    specs = [('T%d' % n, (n,)) for n in LENGTHS] + list(BATCHES.items())
    out, k = [], 0
    for name, lens in specs:
        out.append((name, lens, k))
        k += len(lens)
    return out


_CASES = {}


def cases():
    """{name: dict(L (B,T,11) fp32 -- every row filled, the padded ones as well --, lens, seed)} and the screening statistics
    (generated, dropped).  Built once."""
    if not _CASES:
        generated = dropped = 0
        lst = {}
        for name, lens, k in _case_specs():
            for cand in range(CANDIDATES):
                generated += 1
                T = max(lens)
                L = np.zeros((len(lens), T, 11), np.float32)
                ok, brs = True, []
                for b, n in enumerate(lens):
                    seq, near = sequence(T, 100 * cand + k + b, kind=(k + b) % 4)          # T rows: the padded rows are finite as well
                    if n < T:      # the near-pi and branch frames were placed for the full heading sum: redo them for the rows that count
                        seq[:n], near = sequence(n, 100 * cand + k + b, kind=(k + b) % 4)
                    marg, br = branch_margins(seq[:n], near[:n])
                    ok &= marg >= 1.0
                    brs.append(br)
                    L[b] = seq
                if ok:
                    lst[name] = dict(L=L, lens=tuple(lens), seed=cand, branches=brs)
                    break
                dropped += 1
        _CASES.update(cases=lst, generated=generated, dropped=dropped)
    return _CASES


def upstream(case, pattern, nan_pad=True, scale=1.0):
    """(G_t, G_o, G_q) fp32 for one case -- None for an array the pattern does not give --; rows at or beyond a length hold NaN
    (nan_pad False: the randn they were drawn as)."""
    L, lens = case['L'], case['lens']
    B, T = L.shape[:2]
    rng = np.random.default_rng(7 + T + 31 * B)
    G = [rng.normal(size=(B, T, w)).astype(np.float32) for w in (3, 3, 4)]
    if pattern == 'onehot':      # the longest path back to row 0
        G[0][:] = 0.0
        for b, n in enumerate(lens):
            G[0][b, n - 1, 0] = 1.0
    keep = {'all': (0, 1, 2), 'trans': (0,), 'orient': (1,), 'orient_q': (2,), 'onehot': (0,)}[pattern]
    out = []
    for i, g in enumerate(G):
        if i not in keep:
            out.append(None)
            continue
        g = g * np.float32(scale)
        if nan_pad:
            for b, n in enumerate(lens):
                g[b, n:] = np.nan
        out.append(g)
    return tuple(out)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def _graft(value, grad_of):
    """`value`'s numbers with `grad_of`'s gradient."""
    return value.detach() + (grad_of - grad_of.detach())


def _forward(L, mut=None):
    """oracle.port.transforms.local_to_global_traj + quat_to_aa for one sequence (n, 11); `mut` changes the BACKWARD only."""
    if mut is None or mut == 'pad_rows':
        trans, q = tf.local_to_global_traj(L)
        return trans, tf.quat_to_aa(q), q
    base = torch.tensor(tf._BASE, dtype=L.dtype)
    dxy_h, z = L[..., :2], L[..., 2]
    dh = tf.vec_to_heading(L[..., -2:])
    h = torch.cumsum(dh, dim=0)
    if mut == 'no_suffix':
        h = _graft(h, dh)
    hr = h.detach() if mut == 'no_dR' else h
    rest = tf._rot2d(dxy_h[1:], hr[:-1])
    if mut == 'theta_t':
        rest = _graft(rest, tf._rot2d(dxy_h[1:], h[1:].detach()) + tf._rot2d(dxy_h[1:].detach(), h[:-1]))
    first = dxy_h[:1]
    if mut == 'row0':
        first = _graft(first, tf._rot2d(dxy_h[:1], -h[:1].detach()))
    xy = torch.cumsum(torch.cat([first, rest], dim=0), dim=0)
    trans = torch.cat([xy, z.unsqueeze(-1)], dim=-1)
    q = tf.quat_mul(tf.heading_to_quat(h), tf.sixd_to_quat(L[..., 3:-2]))
    q = tf.quat_mul(q, base.expand_as(q))
    aa = tf.quat_to_aa(q)
    if mut == 'aa_as_vec':
        aa = _graft(aa, q[..., 1:])
    return trans, aa, q


def reference(case, pattern, dtype=torch.float64, mut=None, scale=1.0):
    """dL/d local_traj (B, T, 11) as fp64 numbers (rows at or beyond a length zero) by autograd in `dtype`."""
    L32, lens = case['L'], case['lens']
    G = upstream(case, pattern, nan_pad=False, scale=scale)
    out = np.zeros(L32.shape, np.float64)
    for b, n in enumerate(lens):
        n = L32.shape[1] if mut == 'pad_rows' else n
        L = torch.tensor(L32[b, :n], dtype=dtype).requires_grad_(True)
        outs = _forward(L, mut)
        loss = sum((torch.tensor(g[b, :n], dtype=dtype) * o).sum() for g, o in zip(G, outs) if g is not None)
        (gl,) = torch.autograd.grad(loss, L)
        out[b, :lens[b]] = gl.double().numpy()[:lens[b]]
    return out


def errors(got, ref, lens):
    """Worst error over the sequences per column group, each relative to the sequence's largest reference entry of the group."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = {}
    for k, c in GROUPS.items():
        worst = 0.0
        for b, n in enumerate(lens):
            scale = np.abs(ref[b, :n, c]).max()
            worst = max(worst, float(np.abs(got[b, :n, c] - ref[b, :n, c]).max() / (scale if scale > 0 else 1.0)))
        out[k] = worst
    return out


_REF = {}


def ref64(name, pattern):
    """The fp64 reference of a case, computed once and left unchanged."""
    if (name, pattern) not in _REF:
        _REF[(name, pattern)] = reference(cases()['cases'][name], pattern)
    return _REF[(name, pattern)]


def measure_floor(name):
    """fp32 autograd against fp64, worst over the upstream patterns, per group (one thread: the rounding does not depend on the machine's cores)."""
    from tests.traj_ref_common import single_thread
    case = cases()['cases'][name]
    acc = {k: 0.0 for k in GROUPS}
    with single_thread():
        for pattern in PATTERNS:
            e = errors(reference(case, pattern, torch.float32), ref64(name, pattern), case['lens'])
            acc = {k: max(acc[k], e[k]) for k in GROUPS}
    return acc


# fp32 autograd of the port against fp64 (one thread), rounded up to two digits; tests/test_global_vjp_ref.py measures them again
FLOOR = {
    'T1':      {'xy': 0.0e+00, 'z': 0.0e+00, 'rot': 1.6e-07, 'heading': 3.4e-07},      # 0.000e+00, 0.000e+00, 1.557e-07, 3.284e-07
    'T2':      {'xy': 5.9e-08, 'z': 0.0e+00, 'rot': 3.7e-07, 'heading': 4.7e-06},      # 5.657e-08, 0.000e+00, 3.510e-07, 4.437e-06
    'T3':      {'xy': 5.7e-08, 'z': 0.0e+00, 'rot': 4.2e-07, 'heading': 1.6e-07},      # 5.434e-08, 0.000e+00, 3.967e-07, 1.530e-07
    'T63':     {'xy': 1.9e-06, 'z': 0.0e+00, 'rot': 1.0e-06, 'heading': 1.5e-06},      # 1.829e-06, 0.000e+00, 9.552e-07, 1.396e-06
    'T64':     {'xy': 9.7e-08, 'z': 0.0e+00, 'rot': 2.0e-07, 'heading': 2.7e-07},      # 9.210e-08, 0.000e+00, 1.862e-07, 2.553e-07
    'T65':     {'xy': 2.9e-06, 'z': 0.0e+00, 'rot': 9.8e-07, 'heading': 1.5e-06},      # 2.715e-06, 0.000e+00, 9.356e-07, 1.465e-06
    'T255':    {'xy': 8.6e-08, 'z': 0.0e+00, 'rot': 2.4e-07, 'heading': 3.4e-07},      # 8.146e-08, 0.000e+00, 2.284e-07, 3.261e-07
    'T256':    {'xy': 1.3e-05, 'z': 0.0e+00, 'rot': 2.3e-06, 'heading': 4.5e-06},      # 1.237e-05, 0.000e+00, 2.192e-06, 4.272e-06
    'T257':    {'xy': 1.2e-07, 'z': 0.0e+00, 'rot': 3.8e-07, 'heading': 1.9e-07},      # 1.126e-07, 0.000e+00, 3.637e-07, 1.797e-07
    'T300':    {'xy': 1.8e-05, 'z': 0.0e+00, 'rot': 2.7e-06, 'heading': 4.4e-06},      # 1.671e-05, 0.000e+00, 2.575e-06, 4.175e-06
    'T513':    {'xy': 1.7e-07, 'z': 0.0e+00, 'rot': 2.4e-07, 'heading': 2.2e-07},      # 1.621e-07, 0.000e+00, 2.241e-07, 2.107e-07
    'ragged3': {'xy': 3.3e-06, 'z': 0.0e+00, 'rot': 1.0e-06, 'heading': 1.3e-06},      # 3.124e-06, 0.000e+00, 9.779e-07, 1.265e-06
    'ragged5': {'xy': 1.6e-05, 'z': 0.0e+00, 'rot': 4.6e-06, 'heading': 4.3e-06},      # 1.548e-05, 0.000e+00, 4.368e-06, 4.074e-06
}


def tol(name):
    return {k: FLOOR_FACTOR * v for k, v in FLOOR[name].items()}


if __name__ == '__main__':
    st = cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    for name in st['cases']:
        f = measure_floor(name)
        up = {k: (0.0 if v == 0 else float('%.1e' % (v * 1.05))) for k, v in f.items()}
        print("    %-10s {%s},      # %s" % ("'%s':" % name, ', '.join("'%s': %.1e" % (k, up[k]) for k in GROUPS), ', '.join('%.3e' % f[k] for k in GROUPS)))
