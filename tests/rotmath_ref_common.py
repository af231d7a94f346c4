"""fp64 reference of every primitive of glamr_amd/csrc/rotmath.hpp (the functions of oracle/port/transforms.py and oracle.smplx_lbs.batch_rodrigues
in torch.float64 on the fp32 inputs, gradients by autograd), the named input groups the CPU and the device tests run, the conditions those inputs
must meet, the error measure, the floors (the fp32 restatement's own rounding against the fp64 one) behind every tolerance, the mutations that show
the tests can fail, and the file format of tools/rotmath_probe.hip (the layout of tests/smpl_ref_common.py).

Conditions on the inputs (tests/test_rotmath_ref.py asserts them for every row):
  * no decision quantity lies within a relative 1e-3 of its threshold: theta^2, s^2 and sqrt_clamped's argument against 1e-6, |x| and |den| against 1e-6,
    norms against 1e-9 (1e-12 for quat_to_rotmat); a computed quantity that is compared with ZERO (the trace, the w of rotmat_to_aa's intermediate
    quaternion) is at least ZERO_MARGIN = 32 fp32 ulps of its O(1) operands away from it; comparisons of two inputs (c < 0, the diagonal ties,
    theta^2 > 0) are exact in every precision.  Every row's branches, computed in fp32 and in fp64, agree;
  * a group is only a test where the fp32 restatement keeps its digits: every floor is <= 1e-3.  Two regimes fail that and are left out: the gradient
    of rot6d_to_rotmat at a column angle of 0.01 (2.3e-3), and the gradient of aa_to_rotmat_s below 1e-3 rad (2.0e-3: 1 - cos cancels and smplx has
    no Taylor branch) -- for the latter the groups 'tiny' and 'zero' check the forward value and that the gradient is finite (GRAD_FINITE_ONLY);
  * a gradient row is only a test where the question is well-conditioned (grad_condition() <= GRAD_COND_MAX = 16: at most four of the 24 bits
    lost).  Two primitives have rows that are not, for N(0,1) upstream gradients.  normalize3: where g lies within 1 / 16 rad of the input's
    direction the two terms of (g - (g.x^) x^) / n cancel, the error of ANY fp32 evaluation is that condition number times a rounding of random
    size, and the maximum over a group is the lottery of its one worst row (one row at 38 among 512 N(0,1) pairs).  heading_quat: its gradient is a
    scalar measured against itself, (g3 cos(theta/2) - g0 sin(theta/2)) / 2, which N(0,1) pairs bring arbitrarily close to zero (2500 in one of 512
    rows); its condition number with respect to theta is also what a backward-stable evaluation -- exact for an angle one ulp away, which is all a
    one-ulp root leaves of th = sqrt(theta^2) -- may err by.  A floor measured on such a row says nothing about another correct order of
    operations.  Such rows are drawn out (1 to 2 of 512 for normalize3, about one in ten for heading_quat).  Measured with them left in: the g++
    build at 4.46 x floor in normalize3 'scale1e-3' (the median row at 1.03 x); heading_quat 'twopi' at 40 x floor on the two fast device builds,
    one row with g3 = -0.007 whose angle v_sqrt_f32 returned one ulp off;
  * the exactly (anti)parallel 6D columns of the detection-gap wake-up (a legitimate one-ulp sensitivity of the fast builds) are no
    tolerance group: wakeup_rows() feeds the bit-equality test of the IEEE build only.

Error measure, forward and gradient alike: per row |got - ref64|_inf / |ref64 row|_inf, a row whose fp64 reference is entirely zero must come out
exactly zero (else the row's error is inf, as it is for a NaN), a group's error is the maximum over its rows.  Upstream gradients are N(0,1) from the
group's seed."""
import ctypes
import functools
import math
import zlib
import numpy as np
import torch

from oracle.port import transforms as tf
from oracle.smplx_lbs import batch_rodrigues

# (name, inputs, outputs, has a backward): the table tools/rotmath_probe.hip prints; the id of a primitive is its position
TABLE = (('rot6d_to_rotmat', 6, 9, 1), ('rotmat_to_quat', 9, 4, 1), ('quat_to_aa', 4, 3, 1), ('aa_to_quat', 3, 4, 1), ('aa_to_rotmat_k', 3, 9, 1),
         ('aa_to_rotmat_s', 3, 9, 1), ('rotmat_to_aa', 9, 3, 1), ('quat_mul', 8, 4, 1), ('atan2s', 2, 1, 1), ('normalize3', 3, 3, 1),
         ('quat_to_rotmat', 4, 9, 0), ('quat_rotate', 7, 3, 0), ('quat_heading', 4, 1, 0), ('quat_heading_q', 4, 4, 0), ('heading_quat', 1, 4, 1),
         ('sdiv', 2, 1, 1), ('sqrt_clamped', 1, 1, 1), ('mat3_mul', 18, 9, 1), ('quat_mul_plain', 8, 4, 0),
         ('div', 2, 1, 0), ('sqrt_rn', 1, 1, 0), ('sincos', 1, 2, 0))
SPEC = {n: (i, nin, nout, bool(b)) for i, (n, nin, nout, b) in enumerate(TABLE)}
PRIMS = tuple(n for n, _, _, _ in TABLE[:19])          # the rotation primitives; the last three entries are the operand arrays
SEED = 20241
N_ROWS = 512
EPS32 = 2.0 ** -24
ZERO_MARGIN = 32 * 2.0 ** -23
REL_MARGIN = 1e-3


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
# Restatements with room for a mutation; tests/test_rotmath_ref.py pins each unmutated one to the port's function bit for bit, in both dtypes.
def _safe_div(num, den, eps=1e-6, bump=True):
    """lib/utils/konia_transform.py:340-343"""
    return num / (torch.where(den.abs() < eps, den + eps, den) if bump else den)


def _safe_atan2(y, x, eps=1e-6, bump=True):
    """lib/utils/torch_transform.py:63-67"""
    return tf.safe_atan2(y, x, eps) if bump else torch.atan2(y, x)


def _sqrt_clamped(a, eps=1e-6, pass_below=False):
    """sqrt(clamp_min(a, eps)) as lib/utils/konia_transform.py writes it in :349-443, :560-630 and :753-826; torch's clamp passes the gradient where a >= eps"""
    c = a.clamp_min(eps)
    return torch.sqrt(c.detach() + (a - a.detach()) if pass_below else c)


def _unit(x, eps=1e-9, norm_term_below=False, clamp=True):
    """lib/utils/torch_transform.py:6-7"""
    n = x.norm(p=2, dim=-1)
    d = n.clamp(min=eps) if clamp else n
    if norm_term_below:
        d = d.detach() + (n - n.detach())
    return x / d.unsqueeze(-1)


def _aa_to_rotmat_k(aa, bump=1e-6, taylor=1e-6):
    """lib/utils/konia_transform.py:234-313"""
    theta2 = (aa * aa).sum(-1, keepdim=True)
    theta = torch.sqrt(theta2.clamp_min(1e-6))
    w = aa / (theta + bump)
    wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    c, s = torch.cos(theta), torch.sin(theta)
    k = 1.0 - c
    normal = torch.cat([c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k, wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k,
                        -wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k], dim=1)
    rx, ry, rz = aa[:, 0:1], aa[:, 1:2], aa[:, 2:3]
    one = torch.ones_like(rx)
    tay = torch.cat([one, -rz, ry, rz, one, -rx, -ry, rx, one], dim=1)
    big = (theta2 > taylor).to(aa.dtype)
    return big * normal + (1 - big) * tay


def _rotmat_to_quat(m, eps=1e-6, always0=False):
    """lib/utils/konia_transform.py:349-443"""
    if not always0:
        return tf.rotmat_to_quat(m.view(-1, 3, 3), eps)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[..., i:i + 1] for i in range(9)]
    sq = torch.sqrt((m00 + m11 + m22 + 1.0).clamp_min(eps)) * 2.0
    return torch.cat([0.25 * sq, _safe_div(m21 - m12, sq), _safe_div(m02 - m20, sq), _safe_div(m10 - m01, sq)], dim=-1)


def _quat_to_aa(q, eps=1e-6, flip=True):
    """lib/utils/konia_transform.py:560-630"""
    c, q1, q2, q3 = q.unbind(-1)
    s2 = q1 * q1 + q2 * q2 + q3 * q3
    s = torch.sqrt(s2.clamp_min(eps))
    two_theta = 2.0 * (torch.where(c < 0.0, tf.safe_atan2(-s, -c), tf.safe_atan2(s, c)) if flip else tf.safe_atan2(s, c))
    k = torch.where(s2 > 0.0, _safe_div(two_theta, s, eps), 2.0 * torch.ones_like(s))
    return torch.stack([q1 * k, q2 * k, q3 * k], dim=-1)


def _aa_to_quat(aa, eps=1e-6, half_upto=0.0):
    """lib/utils/konia_transform.py:753-826; half_upto: k = 0.5 while theta^2 <= half_upto (the reference: only at theta^2 = 0)"""
    th2 = (aa * aa).sum(-1, keepdim=True)
    th = torch.sqrt(th2.clamp_min(eps))
    half = th * 0.5
    pos = th2 > 0.0
    k = torch.where(th2 > half_upto, _safe_div(torch.sin(half), th, eps), 0.5 * torch.ones_like(half))
    w = torch.where(pos, torch.cos(half), torch.ones_like(half))
    return torch.cat([w, aa * k], dim=-1)


def _heading_quat_of(q, clamp=True):
    """lib/utils/torch_transform.py:180-185"""
    z = torch.zeros_like(q[..., 0])
    return _unit(torch.stack([q[..., 0], z, z, q[..., 3]], dim=-1), clamp=clamp)


def _quat_mul_plain(x):
    """The Hamilton product written out term by term: what rotmath.hpp's quat_mul_bwd multiplies with (the reference has only the 9-multiplication
    arrangement of lib/utils/torch_transform.py:10-28, which is quat_mul)."""
    a0, a1, a2, a3, b0, b1, b2, b3 = x.unbind(-1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], dim=-1)


def _quat_to_rotmat_raw(q):
    """lib/utils/konia_transform.py:470-555 WITHOUT its normalisation (a mutation)"""
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)


def _heading_quat(x):
    """lib/utils/torch_transform.py:200-204"""
    z = torch.zeros_like(x[:, 0])
    return _aa_to_quat(torch.stack([z, z, x[:, 0]], dim=-1))


REF = {
    'rot6d_to_rotmat': lambda x: tf.sixd_to_rotmat(x).reshape(-1, 9),                                 # torch_transform.py:220-227
    'rotmat_to_quat': _rotmat_to_quat,
    'quat_to_aa': _quat_to_aa,
    'aa_to_quat': _aa_to_quat,
    'aa_to_rotmat_k': _aa_to_rotmat_k,
    'aa_to_rotmat_s': lambda x: batch_rodrigues(x).reshape(-1, 9),                                    # smplx.lbs.batch_rodrigues
    'rotmat_to_aa': lambda x: _quat_to_aa(_rotmat_to_quat(x)),                                        # konia_transform.py:316-339
    'quat_mul': lambda x: tf.quat_mul(x[:, :4], x[:, 4:]),                                            # torch_transform.py:10-28
    'atan2s': lambda x: _safe_atan2(x[:, 0], x[:, 1]).unsqueeze(-1),
    'normalize3': _unit,
    'quat_to_rotmat': lambda x: tf.quat_to_rotmat(x).reshape(-1, 9),                                  # konia_transform.py:470-555
    'quat_rotate': lambda x: tf.quat_rotate(x[:, :4], x[:, 4:]),                                      # torch_transform.py:38-45
    'quat_heading': lambda x: tf.heading_of(x).unsqueeze(-1),                                         # torch_transform.py:172-177
    'quat_heading_q': _heading_quat_of,
    'heading_quat': _heading_quat,
    'sdiv': lambda x: _safe_div(x[:, 0:1], x[:, 1:2]),
    'sqrt_clamped': _sqrt_clamped,
    'mat3_mul': lambda x: torch.matmul(x[:, :9].reshape(-1, 3, 3), x[:, 9:].reshape(-1, 3, 3)).reshape(-1, 9),
    'quat_mul_plain': _quat_mul_plain,
}
# what the unmutated restatements above must equal bit for bit (tests/test_rotmath_ref.py)
PORT = {
    'rotmat_to_quat': lambda x: tf.rotmat_to_quat(x.view(-1, 3, 3)), 'quat_to_aa': tf.quat_to_aa, 'aa_to_quat': tf.aa_to_quat,
    'aa_to_rotmat_k': lambda x: tf.aa_to_rotmat(x).reshape(-1, 9), 'rotmat_to_aa': lambda x: tf.rotmat_to_aa(x.view(-1, 3, 3)),
    'atan2s': lambda x: tf.safe_atan2(x[:, 0], x[:, 1]).unsqueeze(-1), 'normalize3': tf.unit, 'quat_heading_q': tf.heading_quat_of,
    'heading_quat': lambda x: tf.heading_to_quat(x[:, 0]), 'sdiv': lambda x: tf._safe_div(x[:, 0:1], x[:, 1:2]),
}

# name: (primitive, the group that must catch it, the mutated fp64 reference)
MUTATIONS = {
    'sqrt_clamped passes the gradient below the clamp': ('sqrt_clamped', 'below', lambda x: _sqrt_clamped(x, pass_below=True)),
    'sdiv without its eps bump': ('sdiv', 'below+', lambda x: _safe_div(x[:, 0:1], x[:, 1:2], bump=False)),
    'atan2s without its eps bump': ('atan2s', 'both_tiny', lambda x: _safe_atan2(x[:, 0], x[:, 1], bump=False).unsqueeze(-1)),
    'quat_to_aa without the c < 0 flip': ('quat_to_aa', '-generic', lambda x: _quat_to_aa(x, flip=False)),
    'rotmat_to_quat always on branch 0': ('rotmat_to_quat', 'pi', lambda x: _rotmat_to_quat(x, always0=True)),
    'aa_to_rotmat_k divides by theta': ('aa_to_rotmat_k', 'small', lambda x: _aa_to_rotmat_k(x, bump=0.0)),
    'aa_to_rotmat_k on the Taylor branch up to 1e-2': ('aa_to_rotmat_k', 'small', lambda x: _aa_to_rotmat_k(x, taylor=1e-4)),
    'normalize3 with the norm term below the clamp': ('normalize3', 'below', lambda x: _unit(x, norm_term_below=True)),
    'quat_heading_q without its 1e-9 clamp': ('quat_heading_q', 'below', lambda x: _heading_quat_of(x, clamp=False)),
    'aa_to_quat with k = 0.5 up to theta = 1e-2': ('aa_to_quat', 'small', lambda x: _aa_to_quat(x, half_upto=1e-4)),
    # the functions that had no test: one plain error each
    'quat_to_rotmat without the normalisation': ('quat_to_rotmat', 'scaled', lambda x: _quat_to_rotmat_raw(x)),
    'quat_rotate by the conjugate': ('quat_rotate', 'generic', lambda x: tf.quat_rotate(tf.quat_conj(x[:, :4]), x[:, 4:])),
    'quat_heading without the factor 2': ('quat_heading', 'generic', lambda x: 0.5 * REF['quat_heading'](x)),
    'heading_quat about the x axis': ('heading_quat', 'generic', lambda x: _heading_quat(x)[:, [0, 3, 2, 1]]),
    'mat3_mul with its factors swapped': ('mat3_mul', 'generic', lambda x: REF['mat3_mul'](torch.cat([x[:, 9:], x[:, :9]], dim=1))),
    'quat_mul_plain with its factors swapped': ('quat_mul_plain', 'generic', lambda x: _quat_mul_plain(torch.cat([x[:, 4:], x[:, :4]], dim=1))),
}


class single_thread:
    """The fp32 restatement on one thread: its rounding then does not depend on how many cores the machine has."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def ref_eval(prim, x, gout, dtype=torch.float64, fn=None):
    """(forward (n, nout), gradient (n, nin) or None) of the reference in `dtype` on the fp32 rows x, as fp64 numpy."""
    fn = fn or REF[prim]
    xt = torch.tensor(np.asarray(x, np.float32)).to(dtype).requires_grad_(SPEC[prim][3])
    with single_thread():
        out = fn(xt).reshape(x.shape[0], -1)
        if SPEC[prim][3]:
            out.backward(torch.tensor(np.asarray(gout, np.float32)).to(dtype))
    return out.detach().double().numpy(), (xt.grad.double().numpy() if SPEC[prim][3] else None)


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------
ANGLES = {'generic': (0.2, 3.0), 'pi': (math.pi - 1e-2, math.pi + 1e-2), 'twopi': (2 * math.pi - 1e-2, 2 * math.pi), 'small': (1.001e-3, 1e-2),
          'tiny': (1e-5, 0.999e-3)}
GRAD_FINITE_ONLY = {('aa_to_rotmat_s', 'tiny'), ('aa_to_rotmat_s', 'zero')}


def _rng(prim, group):
    return np.random.default_rng([SEED, zlib.crc32(('%s/%s' % (prim, group)).encode())])


def _axes(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _logu(rng, lo, hi, shape):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), shape))


def _aa(rng, n, lo, hi):
    return _axes(rng, n) * rng.uniform(lo, hi, (n, 1))


def _rot64(aa):
    """Exact (fp64) rotation matrices of axis-angle rows, row-major (n, 9)."""
    th = np.linalg.norm(aa, axis=1)
    a = aa / np.maximum(th, 1e-300)[:, None]
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    R = np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)
    return R.reshape(-1, 9)


def _quat64(aa):
    th = np.linalg.norm(aa, axis=1, keepdims=True)
    return np.concatenate([np.cos(th / 2), np.sin(th / 2) * aa / np.maximum(th, 1e-300)], axis=1)


def _angle_groups(prim, to=lambda aa: aa, zero=True, n=N_ROWS):
    g = {name: to(_aa(_rng(prim, name), n, lo, hi)) for name, (lo, hi) in ANGLES.items()}
    if zero:
        g['zero'] = to(np.zeros((1, 3)))
    return g


def _with_negated(g):
    out = dict(g)
    out.update({'-' + k: -v for k, v in g.items()})
    return out


def _rotmat_groups(prim):
    g = _angle_groups(prim, _rot64)
    off = [0, 0, 0, 0, 0, 0, 0, 0, 0]
    for k in (1, 2, 3, 5, 6, 7):
        off[k] = 1.0
    off = np.asarray(off)
    for sgn in '+-':                                    # 2 pi / 3 about assorted axes moved to a trace of +-[1e-5, 1e-2], off-diagonals perturbed by 1e-3
        rng = _rng(prim, 'trace' + sgn)
        t = _logu(rng, 1e-5, 1e-2, N_ROWS) * (1.0 if sgn == '+' else -1.0)
        g['trace' + sgn] = _rot64(_axes(rng, N_ROWS) * np.arccos((t - 1.0) / 2.0)[:, None]) + 1e-3 * rng.normal(size=(N_ROWS, 9)) * off
    for (i, j, k) in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):  # near pi, diagonal entries i and j (the two largest) differ by +-[1e-5, 1e-2]
        for sgn in '+-':
            name = 'tie%d%d%s' % (i, j, sgn)
            rng = _rng(prim, name)
            th = math.pi + _signs(rng, N_ROWS) * rng.uniform(1e-3, 1e-2, N_ROWS)
            d = _logu(rng, 1e-5, 1e-2, N_ROWS) * (1.0 if sgn == '+' else -1.0) / (1.0 - np.cos(th))
            u = rng.uniform(0.05, 0.25, N_ROWS)
            a = np.zeros((N_ROWS, 3))
            a[:, i], a[:, j], a[:, k] = np.sqrt((1 - u) / 2 + d / 2), np.sqrt((1 - u) / 2 - d / 2), np.sqrt(u)
            g[name] = _rot64(a * _signs(rng, (N_ROWS, 3)) * th[:, None])
    g['zero_matrix'] = np.zeros((1, 9))                 # the camera of an unseen frame: branch 3, q = (0, 0, 0, 0.5)
    rng = _rng(prim, 'offmanifold')                     # slightly off-manifold, like the reference's products (tests/test_rotmath_grads.py)
    aa = rng.normal(size=(N_ROWS, 3))
    aa[: N_ROWS // 4] *= 2.5
    g['offmanifold'] = _rot64(aa) + 1e-3 * rng.normal(size=(N_ROWS, 9))
    return g


def _xy_groups(prim):
    g = {}
    rng = _rng(prim, 'generic')
    g['generic'] = rng.normal(size=(N_ROWS, 2))
    rng = _rng(prim, 'both_tiny')                       # both at scale 3e-7: the eps branch
    g['both_tiny'] = _logu(rng, 1e-7, 9e-7, (N_ROWS, 2)) * _signs(rng, (N_ROWS, 2))
    for name, col in (('y_tiny', 0), ('x_tiny', 1)):    # one below 1e-6, the other above
        rng = _rng(prim, name)
        v = _logu(rng, 2e-6, 1.0, (N_ROWS, 2)) * _signs(rng, (N_ROWS, 2))
        v[:, col] = _logu(rng, 1e-8, 9e-7, N_ROWS) * _signs(rng, N_ROWS)
        g[name] = v
    rng = _rng(prim, 'axes')                            # the four axis directions
    r = rng.uniform(0.5, 2.0, 64)
    g['axes'] = np.concatenate([np.stack([0 * r, r], 1), np.stack([0 * r, -r], 1), np.stack([r, 0 * r], 1), np.stack([-r, 0 * r], 1)])
    rng = _rng(prim, 'scale1e-5')
    g['scale1e-5'] = 1e-5 * rng.normal(size=(N_ROWS, 2))
    return g


def _rot6d_groups(prim):
    g = {}
    for name, s in (('scale1e-3', 1e-3), ('scale1', 1.0), ('scale1e3', 1e3)):
        g[name] = s * _rng(prim, name).normal(size=(N_ROWS, 6))
    for phi in (1.0, 0.1, 0.03):                        # angle between the two columns, both signs of their dot product
        for sgn in '+-':
            name = 'angle%g%s' % (phi, sgn)
            rng = _rng(prim, name)
            a1 = _axes(rng, N_ROWS)
            nrm = np.cross(a1, _axes(rng, N_ROWS))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            a2 = (1.0 if sgn == '+' else -1.0) * math.cos(phi) * a1 + math.sin(phi) * nrm
            g[name] = np.concatenate([a1 * rng.uniform(0.5, 2.0, (N_ROWS, 1)), a2 * rng.uniform(0.5, 2.0, (N_ROWS, 1))], axis=1)
    g['zero'] = np.zeros((1, 6))
    rng = _rng(prim, 'zero_column')
    v = rng.normal(size=(64, 6))
    v[:32, :3] = 0.0
    v[32:, 3:] = 0.0
    g['zero_column'] = v
    v = np.zeros((12, 6))                               # +-1e-3 on one axis of one column, the other column zero
    for r in range(12):
        v[r, r // 2] = 1e-3 if r % 2 == 0 else -1e-3
    g['axis_column'] = v
    return g


def wakeup_rows():
    """6D rows whose components are all +-lr (the first Adam steps of the zero cameras of a detection gap): all 64 sign patterns at five
    learning rates -- 16 of the 64 have exactly (anti)parallel columns."""
    rows = []
    for lr in (3e-4, 1e-3, 2e-3, 5e-3, 1e-2):
        for m in range(64):
            rows.append([np.float32(lr) * (1.0 if (m >> b) & 1 else -1.0) for b in range(6)])
    return np.asarray(rows, dtype=np.float32)


def _norm_rows(rng, n, lo, hi, dim=3):
    v = rng.normal(size=(n, dim))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * _logu(rng, lo, hi, (n, 1))


def _candidates(prim):
    if prim in ('aa_to_quat', 'aa_to_rotmat_k', 'aa_to_rotmat_s'):
        return _angle_groups(prim)
    if prim == 'heading_quat':
        return _angle_groups(prim, lambda aa: (np.linalg.norm(aa, axis=1) * np.sign(aa[:, 0] + 1e-300))[:, None])
    if prim in ('quat_to_aa', 'quat_to_rotmat'):
        g = _with_negated(_angle_groups(prim, _quat64))
        if prim == 'quat_to_rotmat':                     # not normalised, and the zero quaternion (normalised with eps 1e-12: the identity comes out)
            rng = _rng(prim, 'scaled')
            g['scaled'] = _quat64(_aa(rng, N_ROWS, 0.2, 3.0)) * _logu(rng, 0.1, 10.0, (N_ROWS, 1)) * _signs(rng, (N_ROWS, 1))
            g['null'] = np.zeros((1, 4))
        return g
    if prim in ('rotmat_to_quat', 'rotmat_to_aa'):
        return _rotmat_groups(prim)
    if prim == 'rot6d_to_rotmat':
        return _rot6d_groups(prim)
    if prim == 'normalize3':
        g = {name: s * _rng(prim, name).normal(size=(N_ROWS, 3)) for name, s in (('scale1e-3', 1e-3), ('scale1', 1.0), ('scale1e3', 1e3))}
        g['below'] = _norm_rows(_rng(prim, 'below'), N_ROWS, 1e-12, 5e-10)
        g['above'] = _norm_rows(_rng(prim, 'above'), N_ROWS, 2e-9, 1e-8)
        g['zero'] = np.zeros((1, 3))
        return g
    if prim == 'atan2s':
        return _xy_groups(prim)
    if prim == 'quat_heading':                          # (z, w) as atan2s's (y, x); x and y of the quaternion are not read
        out = {}
        for name, yx in _xy_groups(prim).items():
            q = _rng(prim, name + '/xy').normal(size=(yx.shape[0], 4))
            q[:, 3], q[:, 0] = yx[:, 0], yx[:, 1]
            out[name] = q
        return out
    if prim == 'sdiv':
        g = {}
        for name, lo, hi, sg in (('generic', 1e-2, 1e2, None), ('below+', 1e-8, 9e-7, 1.0), ('below-', 1e-8, 9e-7, -1.0), ('above+', 1.1e-6, 1e-5, 1.0),
                                 ('above-', 1.1e-6, 1e-5, -1.0)):
            rng = _rng(prim, name)
            den = _logu(rng, lo, hi, N_ROWS) * (_signs(rng, N_ROWS) if sg is None else sg)
            g[name] = np.stack([rng.normal(size=N_ROWS), den], axis=1)
        return g
    if prim == 'sqrt_clamped':
        rng = _rng(prim, 'below')
        below = np.concatenate([_logu(rng, 1e-8, 9.9e-7, N_ROWS), -_logu(rng, 1e-8, 1.0, 64), [0.0]])
        return {'generic': _rng(prim, 'generic').uniform(0.01, 4.0, N_ROWS)[:, None], 'below': below[:, None],
                'above': _logu(_rng(prim, 'above'), 1.01e-6, 1e-5, N_ROWS)[:, None]}
    if prim in ('quat_mul', 'quat_mul_plain'):
        return {'generic': _rng(prim, 'generic').normal(size=(N_ROWS, 8))}
    if prim == 'mat3_mul':
        return {'generic': _rng(prim, 'generic').normal(size=(N_ROWS, 18))}
    if prim == 'quat_rotate':
        rng = _rng(prim, 'generic')
        return {'generic': np.concatenate([_norm_rows(rng, N_ROWS, 1.0, 1.0, 4), rng.normal(size=(N_ROWS, 3))], axis=1),
                'nonunit': _rng(prim, 'nonunit').normal(size=(N_ROWS, 7))}
    if prim == 'quat_heading_q':
        g = {'generic': _rng(prim, 'generic').normal(size=(N_ROWS, 4))}
        rng = _rng(prim, 'small_w')                     # unit quaternions with w in +-[1e-4, 1e-2]
        q = _norm_rows(rng, N_ROWS, 1.0, 1.0, 4)
        w = _logu(rng, 1e-4, 1e-2, N_ROWS) * _signs(rng, N_ROWS)
        q[:, 1:] *= (np.sqrt(1 - w * w) / np.linalg.norm(q[:, 1:], axis=1))[:, None]
        q[:, 0] = w
        g['small_w'] = q
        rng = _rng(prim, 'wz_zero')
        q = _norm_rows(rng, 64, 1.0, 1.0, 4)
        q[:, 0] = q[:, 3] = 0.0
        g['wz_zero'] = q
        rng = _rng(prim, 'below')                       # |(w, z)| in [1e-12, 5e-10]: under the clamp
        q = _norm_rows(rng, N_ROWS, 1.0, 1.0, 4)
        q[:, [0, 3]] = _norm_rows(rng, N_ROWS, 1e-12, 5e-10, 2)
        g['below'] = q
        return g
    raise KeyError(prim)


def decisions(prim, x, dtype):
    """The quantities of the rows `x` that a branch or a clamp of `prim` looks at, evaluated in `dtype`: a list of (name, values, kind, threshold) with
    kind 'rel' (values > threshold decides; must stay a relative REL_MARGIN away), 'zero' (a computed value compared with 0: ZERO_MARGIN away, or a
    sum / difference of zeros, which is 0 in every precision) or
    'exact' (a comparison of inputs, or the positivity of a sum of squares: the same in every precision; `values` is the branch itself)."""
    t = torch.tensor(np.asarray(x, np.float32)).to(dtype)
    eps = 1e-6
    d = []

    def rel(name, v, thr):
        d.append((name, v.double().numpy(), 'rel', thr))

    def exact(name, v):
        d.append((name, v.numpy().astype(np.int64), 'exact', None))

    def r2q(m):
        tr = m[:, 0] + m[:, 4] + m[:, 8]
        br = torch.where(tr > 0, 0, torch.where((m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8]), 1, torch.where(m[:, 4] > m[:, 8], 2, 3)))
        d.append(('trace', tr.double().numpy(), 'zero', 0.0))
        exact('diagonal order', br)
        # (the sqrt argument of the branch that is TAKEN is never under 1: 1 + trace on branch 0, at least 1 + 2 max(diagonal) - trace on the others;
        # its clamp at 1e-6 only ever acts in the candidates `where` discards, and is tested on its own as sqrt_clamped)

    def q2a(q, computed):
        if computed:
            d.append(('w', q[:, 0].double().numpy(), 'zero', 0.0))
        else:
            exact('w < 0', q[:, 0] < 0)
        s2 = (q[:, 1:] ** 2).sum(-1)
        rel('s^2', s2, eps)
        exact('s^2 > 0', s2 > 0)

    if prim in ('atan2s', 'quat_heading'):
        y, xx = (t[:, 0], t[:, 1]) if prim == 'atan2s' else (t[:, 3], t[:, 0])
        rel('|y|', y.abs(), eps)
        rel('|x|', xx.abs(), eps)
    elif prim == 'sdiv':
        rel('|den|', t[:, 1].abs(), eps)
    elif prim == 'sqrt_clamped':
        rel('a', t[:, 0], eps)
    elif prim == 'normalize3':
        rel('norm', t.norm(dim=-1), 1e-9)
    elif prim == 'rot6d_to_rotmat':
        rel('|a1|', t[:, :3].norm(dim=-1), 1e-9)
        b1 = tf.unit(t[:, :3])
        rel('|u|', (t[:, 3:] - (b1 * t[:, 3:]).sum(-1, keepdim=True) * b1).norm(dim=-1), 1e-9)
    elif prim == 'rotmat_to_quat':
        r2q(t)
    elif prim == 'rotmat_to_aa':
        r2q(t)
        q2a(_rotmat_to_quat(t), True)
    elif prim == 'quat_to_aa':
        q2a(t, False)
    elif prim in ('aa_to_quat', 'aa_to_rotmat_k', 'heading_quat'):
        th2 = (t * t).sum(-1)
        rel('theta^2', th2, eps)
        exact('theta^2 > 0', th2 > 0)
    elif prim == 'quat_heading_q':
        rel('|(w, z)|', t[:, [0, 3]].norm(dim=-1), 1e-9)
    elif prim == 'quat_to_rotmat':
        rel('|q|', t.norm(dim=-1), 1e-12)
    return d


def branches(dec):
    return [(v > thr) if kind == 'rel' else (v > 0) if kind == 'zero' else v for _, v, kind, thr in dec]


def well_conditioned(prim, x):
    """Per row: every decision keeps its margin in fp32 and in fp64, and both precisions take the same branches."""
    ok = np.ones(x.shape[0], dtype=bool)
    d32, d64 = decisions(prim, x, torch.float32), decisions(prim, x, torch.float64)
    for dec in (d32, d64):
        for _, v, kind, thr in dec:
            if kind == 'rel':
                ok &= np.abs(v - thr) > REL_MARGIN * thr
            elif kind == 'zero':
                ok &= (np.abs(v) > ZERO_MARGIN) | (v == 0)
    for a, b in zip(branches(d32), branches(d64)):
        ok &= a == b
    return ok


GRAD_COND_MAX = 16.0


def grad_condition(prim, x, gout):
    """Relative condition number of a row's gradient where it can be arbitrarily bad for N(0,1) upstream gradients (1 for every other primitive: their
    cancellations depend on the angle alone and have groups of their own).
      normalize3    (g - (g.x^) x^) / n: |g| / |g_perp| = 1 / sin(angle between g and x), the cancellation between the two terms;
      heading_quat  a SCALAR, d/dtheta (g . q) = (g3 cos(theta/2) - g0 sin(theta/2)) / 2, measured against itself: its condition number with
                    respect to theta, |theta| |g0 cos + g3 sin| / (2 |g3 cos - g0 sin|), which is also what the cancellation of its two terms costs."""
    x, g = np.asarray(x, np.float64), np.asarray(gout, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        if prim == 'normalize3':
            c = (x * g).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(g, axis=1))
            return np.where(np.linalg.norm(x, axis=1) > 0, 1.0 / np.sqrt(1.0 - c * c), 1.0)
        if prim == 'heading_quat':
            th = x[:, 0]
            co, si = np.cos(th / 2), np.sin(th / 2)
            cond = np.abs(th) * np.abs(g[:, 0] * co + g[:, 3] * si) / (2.0 * np.abs(g[:, 3] * co - g[:, 0] * si))
            return np.where(th * th > 1e-6, cond, 1.0)          # (under the clamp theta only scales the constant k)
    return np.ones(x.shape[0])


@functools.lru_cache(maxsize=None)
def _rows(prim):
    """{group: (fp32 rows (n, nin), fp32 N(0,1) upstream gradients (n, nout))}: the candidates from fixed seeds, rounded to fp32, without the rows that
    sit on a threshold or whose gradient is ill-conditioned."""
    out = {}
    for name, v in _candidates(prim).items():
        x = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1, SPEC[prim][1]).astype(np.float32))
        g = _rng(prim, name + '/gout').normal(size=(x.shape[0], SPEC[prim][2])).astype(np.float32)
        keep = well_conditioned(prim, x) & (grad_condition(prim, x, g) <= GRAD_COND_MAX)
        x, g = np.ascontiguousarray(x[keep]), np.ascontiguousarray(g[keep])
        x.setflags(write=False)
        g.setflags(write=False)
        out[name] = (x, g)
    return out


def groups(prim):
    """{group: fp32 rows (n, nin)} of a primitive."""
    return {k: v[0] for k, v in _rows(prim).items()}


def upstream(prim, group):
    """N(0,1) upstream gradients (n, nout) of a group, fp32."""
    return _rows(prim)[group][1]


@functools.lru_cache(maxsize=None)
def table_rows(prim):
    """All groups of a primitive as one block: (x, gout, {group: slice})."""
    xs, gs, sl, n = [], [], {}, 0
    for name, x in groups(prim).items():
        xs.append(x)
        gs.append(upstream(prim, name))
        sl[name] = slice(n, n + x.shape[0])
        n += x.shape[0]
    return np.concatenate(xs), np.concatenate(gs), sl


@functools.lru_cache(maxsize=None)
def reference(prim, dtype=torch.float64):
    """The reference's (forward, gradient) of the whole block of a primitive, computed once and shared."""
    x, g, _ = table_rows(prim)
    out, gx = ref_eval(prim, x, g, dtype)
    out.setflags(write=False)
    if gx is not None:
        gx.setflags(write=False)
    return out, gx


# ---- the error measure ------------------------------------------------------------------------------------------------------------------
def row_errors(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        diff = np.abs(got - ref).max(axis=1)
        err = np.where(scale > 0, diff / scale, np.where(np.all(got == 0, axis=1), 0.0, np.inf))
    return np.where(np.isfinite(err), err, np.inf)


def group_errors(prim, out, gx, ref=None):
    """{group: (forward error, gradient error or None)} of a result for the whole block of `prim` against `ref` (default: the fp64 reference).  The
    gradient entry of a GRAD_FINITE_ONLY group is 0.0 where every gradient is finite and inf otherwise."""
    r_out, r_gx = ref or reference(prim)
    res = {}
    for name, sl in table_rows(prim)[2].items():
        ef = float(row_errors(out[sl], r_out[sl]).max())
        eg = None
        if SPEC[prim][3]:
            if (prim, name) in GRAD_FINITE_ONLY:
                eg = 0.0 if np.all(np.isfinite(gx[sl])) else float('inf')
            else:
                eg = float(row_errors(gx[sl], r_gx[sl]).max())
        res[name] = (ef, eg)
    return res


def measure_floors(prim):
    """The fp32 restatement on one thread against the fp64 one.  A floor under 2^-24 -- half an ulp of the fp32 numbers every result is stored in --
    is raised to it: the restatement meets some rows exactly (zeros, ones, powers of two) that no other correct order of operations has to."""
    x, g, _ = table_rows(prim)
    out, gx = ref_eval(prim, x, g, torch.float32)
    return {k: (max(f, EPS32), None if b is None else (0.0 if (prim, k) in GRAD_FINITE_ONLY else max(b, EPS32))) for k, (f, b) in group_errors(prim, out, gx).items()}


# ---- the g++ build of the header --------------------------------------------------------------------------------------------------------
def shim_eval(prim, x, gout):
    from tests import hostsim
    lib = hostsim.build('rotmath_shim')
    _, nin, nout, _ = SPEC[prim]
    x = np.ascontiguousarray(x, dtype=np.float32)
    gout = np.ascontiguousarray(gout, dtype=np.float32)
    out, gx = np.zeros((x.shape[0], nout), dtype=np.float32), np.zeros_like(x)
    fn = getattr(lib, 't_' + prim)
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    fn(x.shape[0], x.ctypes.data, gout.ctypes.data, out.ctypes.data, gx.ctypes.data)
    return out, (gx if SPEC[prim][3] else None)


@functools.lru_cache(maxsize=None)
def shim_block(prim):
    x, g, _ = table_rows(prim)
    return shim_eval(prim, x, g)


# ---- operand arrays of div_, sqrt_rn_ and sincos_ ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_operands():
    """(n, d): 1e6 pairs with |n|, |d| log-uniform in [2^-40, 2^40] and random signs (Adam's denominators of 1e-8 to 1e12; every intermediate of
    the expansion stays normal), then 4096 rows with n = 0."""
    rng = np.random.default_rng([SEED, 1])
    v = np.exp2(rng.uniform(-40, 40, (1000000 + 4096, 2))) * _signs(rng, (1000000 + 4096, 2))
    v[1000000:, 0] = 0.0
    return np.ascontiguousarray(v.astype(np.float32))


@functools.lru_cache(maxsize=None)
def sqrt_operands():
    """0, 1e6 log-uniform x over the whole normal range, the fp32 squares of 1e4 random floats and the two neighbours of each square."""
    rng = np.random.default_rng([SEED, 2])
    x = np.exp2(rng.uniform(-126, 128, 1000000)).astype(np.float32)
    x = np.clip(x, np.finfo(np.float32).tiny, np.finfo(np.float32).max)
    r = np.exp2(rng.uniform(-60, 60, 10000)).astype(np.float32)
    sq = r * r
    return np.ascontiguousarray(np.concatenate([[np.float32(0)], x, sq, np.nextafter(sq, np.float32(0)), np.nextafter(sq, np.float32(np.inf))]).astype(np.float32))


SQRT_RN_EXACT_FROM = 2.0 ** -102      # sqrt_rn_'s documented domain (rotmath.hpp): from here up no fma residual of its correction can underflow to zero
SINCOS_CASES = ((3.2, 2.0, 1.2e-7), (1000.0, 2.0, 1.2e-7), (1e5, 4.0, 1e-6))      # (|x| up to, ulp bound, absolute bound) of test_sincos_accuracy


@functools.lru_cache(maxsize=None)
def sincos_operands():
    """The inputs of tests/test_rotmath_grads.py::test_sincos_accuracy as they stand, one array per case."""
    rng = np.random.default_rng(7)
    return tuple(np.concatenate([rng.uniform(-lim, lim, 400000), np.arange(-40, 41) * (np.pi / 4), [0.0, -0.0, 1e-30, -1e-8]]).astype(np.float32)
                 for lim, _, _ in SINCOS_CASES)


# ---- tools/rotmath_probe.hip ------------------------------------------------------------------------------------------------------------
MAGIC = 0x31504d52
BUILDS = ('default', 'grecon', 'ieee')


def probe_flags(build):
    """The library's own flags (glamr_amd/build.py) for the three programs rotmath.hpp is on the device."""
    from glamr_amd import build as b
    return {'default': list(b.FLAGS), 'grecon': list(b.FLAGS) + list(b.FILE_FLAGS['grecon.hip']),
            'ieee': list(b.FLAGS) + ['-DGLAMR_ROTMATH_IEEE=1'] + list(b.FILE_FLAGS['init.hip'])}[build]


def probe_command(build, src, exe, compile_only=False):
    from glamr_amd import build as b
    return [b.HIPCC] + probe_flags(build) + (['-c'] if compile_only else []) + [src, '-o', exe]


def probe_blocks():
    """The whole input table as [(label, primitive, x, gout or None)]: one block per rotation primitive (all its groups), the wake-up columns, the
    operand arrays."""
    blocks = []
    for p in PRIMS:
        x, g, _ = table_rows(p)
        blocks.append((p, p, x, g if SPEC[p][3] else None))
    w = wakeup_rows()
    blocks.append(('wakeup', 'rot6d_to_rotmat', w, np.random.default_rng([SEED, 3]).normal(size=(w.shape[0], 9)).astype(np.float32)))
    blocks.append(('div', 'div', div_operands(), None))
    blocks.append(('sqrt_rn', 'sqrt_rn', sqrt_operands()[:, None], None))
    for i, x in enumerate(sincos_operands()):
        blocks.append(('sincos%d' % i, 'sincos', x[:, None], None))
    return blocks


def write_probe_input(path, blocks):
    with open(path, 'wb') as f:
        f.write(np.asarray([MAGIC, len(blocks)], dtype=np.int32).tobytes())
        for _, prim, x, g in blocks:
            pid, nin, nout, hasb = SPEC[prim]
            assert x.dtype == np.float32 and x.shape[1] == nin and (g is None) == (not hasb)
            f.write(np.asarray([pid, x.shape[0]], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(x).tobytes())
            if hasb:
                assert g.dtype == np.float32 and g.shape == (x.shape[0], nout)
                f.write(np.ascontiguousarray(g).tobytes())


def read_probe_output(path, blocks):
    """{label: (forward (n, nout), gradient (n, nin) or None)}"""
    data = np.fromfile(path, dtype=np.float32)
    res, at = {}, 0
    for label, prim, x, _ in blocks:
        _, nin, nout, hasb = SPEC[prim]
        n = x.shape[0]
        out = data[at:at + n * nout].reshape(n, nout)
        at += n * nout
        gx = None
        if hasb:
            gx = data[at:at + n * nin].reshape(n, nin)
            at += n * nin
        res[label] = (out, gx)
    assert at == data.size, (at, data.size)
    return res


def parse_probe_table(stdout):
    return tuple((f[2], int(f[3]), int(f[4]), int(f[5])) for f in (ln.split() for ln in stdout.splitlines()) if len(f) == 6 and f[0] == 'table')


# ---- floors and tolerances --------------------------------------------------------------------------------------------------------------
# FLOORS[primitive][group] = (forward, gradient): the measure above for the fp32 restatement against the fp64 one, on one thread, rounded up to
# two digits (the measured values in the comment).  `python -m tests.rotmath_ref_common` prints the table to paste here; tests/test_rotmath_ref.py
# measures it again and fails when a floor leaves [1/2, 2] x its constant or exceeds 1e-3.
# The tolerance is FACTOR x floor.  The exact-operator g++ build of the header reaches at most 2.5 x floor against the fp32 restatement over groups
# of this kind, because the C++ forms the same values in another order: rounded up to HOST_FACTOR = 4, which the CPU test holds the g++ build to.
# Twice that for a one-ulp hardware reciprocal and root in place of the correctly rounded ones: FACTOR = 8 for every device build.
HOST_FACTOR = 4
FACTOR = 8
FLOORS = {}
FLOORS['rot6d_to_rotmat'] = {
    'scale1e-3': (3.1e-06, 2.4e-06),  # 3.040e-06, 2.325e-06  (512 rows)
    'scale1': (1.4e-06, 1.4e-06),  # 1.303e-06, 1.399e-06  (512 rows)
    'scale1e3': (4.1e-06, 8.8e-05),  # 4.073e-06, 8.754e-05  (512 rows)
    'angle1+': (2.0e-07, 2.3e-06),  # 1.919e-07, 2.247e-06  (512 rows)
    'angle1-': (1.8e-07, 2.5e-06),  # 1.704e-07, 2.434e-06  (512 rows)
    'angle0.1+': (2.3e-06, 3.2e-05),  # 2.272e-06, 3.179e-05  (512 rows)
    'angle0.1-': (2.4e-06, 1.1e-05),  # 2.397e-06, 1.071e-05  (512 rows)
    'angle0.03+': (6.7e-06, 1.6e-04),  # 6.696e-06, 1.565e-04  (512 rows)
    'angle0.03-': (7.7e-06, 2.0e-04),  # 7.698e-06, 1.915e-04  (512 rows)
    'zero': (6.0e-08, 7.8e-08),  # 5.960e-08, 7.714e-08  (1 rows)
    'zero_column': (7.4e-08, 3.7e-07),  # 7.321e-08, 3.676e-07  (64 rows)
    'axis_column': (6.0e-08, 6.8e-08),  # 5.960e-08, 6.740e-08  (12 rows)
}
FLOORS['rotmat_to_quat'] = {
    'generic': (1.2e-07, 1.8e-07),  # 1.189e-07, 1.783e-07  (512 rows)
    'pi': (1.3e-07, 1.7e-07),  # 1.238e-07, 1.688e-07  (512 rows)
    'twopi': (6.0e-08, 1.2e-07),  # 5.960e-08, 1.124e-07  (512 rows)
    'small': (6.0e-08, 1.2e-07),  # 5.960e-08, 1.120e-07  (512 rows)
    'tiny': (6.0e-08, 1.1e-07),  # 5.960e-08, 1.061e-07  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
    'trace+': (1.6e-07, 3.5e-07),  # 1.508e-07, 3.429e-07  (512 rows)
    'trace-': (1.4e-07, 1.9e-07),  # 1.385e-07, 1.846e-07  (512 rows)
    'tie01+': (1.5e-07, 2.2e-07),  # 1.449e-07, 2.123e-07  (512 rows)
    'tie01-': (1.4e-07, 2.2e-07),  # 1.334e-07, 2.116e-07  (512 rows)
    'tie02+': (1.5e-07, 1.9e-07),  # 1.469e-07, 1.835e-07  (512 rows)
    'tie02-': (1.5e-07, 2.8e-07),  # 1.493e-07, 2.719e-07  (512 rows)
    'tie12+': (1.3e-07, 1.6e-07),  # 1.298e-07, 1.557e-07  (512 rows)
    'tie12-': (1.3e-07, 1.8e-07),  # 1.233e-07, 1.757e-07  (512 rows)
    'zero_matrix': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
    'offmanifold': (1.6e-07, 2.1e-07),  # 1.504e-07, 2.060e-07  (512 rows)
}
FLOORS['quat_to_aa'] = {
    'generic': (1.6e-07, 2.3e-07),  # 1.599e-07, 2.295e-07  (512 rows)
    'pi': (1.4e-07, 3.5e-07),  # 1.332e-07, 3.423e-07  (512 rows)
    'twopi': (1.3e-07, 2.8e-07),  # 1.283e-07, 2.725e-07  (512 rows)
    'small': (1.6e-07, 2.5e-07),  # 1.595e-07, 2.456e-07  (512 rows)
    'tiny': (8.3e-08, 8.3e-08),  # 8.287e-08, 8.282e-08  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
    '-generic': (1.4e-07, 2.8e-07),  # 1.356e-07, 2.770e-07  (512 rows)
    '-pi': (1.4e-07, 3.1e-07),  # 1.332e-07, 3.064e-07  (512 rows)
    '-twopi': (1.6e-07, 2.5e-07),  # 1.533e-07, 2.466e-07  (512 rows)
    '-small': (1.4e-07, 2.5e-07),  # 1.357e-07, 2.412e-07  (512 rows)
    '-tiny': (8.3e-08, 8.3e-08),  # 8.287e-08, 8.280e-08  (512 rows)
    '-zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
}
FLOORS['aa_to_quat'] = {
    'generic': (1.6e-07, 7.8e-07),  # 1.575e-07, 7.781e-07  (512 rows)
    'pi': (1.7e-07, 7.1e-07),  # 1.659e-07, 7.005e-07  (512 rows)
    'twopi': (2.2e-07, 2.0e-04),  # 2.136e-07, 1.944e-04  (512 rows)
    'small': (6.0e-08, 2.1e-07),  # 5.960e-08, 2.075e-07  (512 rows)
    'tiny': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
}
FLOORS['aa_to_rotmat_k'] = {
    'generic': (4.4e-07, 8.3e-07),  # 4.385e-07, 8.267e-07  (512 rows)
    'pi': (4.4e-07, 2.0e-06),  # 4.336e-07, 1.968e-06  (512 rows)
    'twopi': (6.1e-07, 3.1e-05),  # 6.078e-07, 3.089e-05  (512 rows)
    'small': (6.0e-08, 9.0e-05),  # 5.960e-08, 8.943e-05  (512 rows)
    'tiny': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
}
FLOORS['aa_to_rotmat_s'] = {
    'generic': (3.3e-07, 5.3e-07),  # 3.288e-07, 5.265e-07  (512 rows)
    'pi': (5.3e-07, 8.5e-07),  # 5.286e-07, 8.443e-07  (512 rows)
    'twopi': (4.1e-07, 5.8e-05),  # 4.075e-07, 5.727e-05  (512 rows)
    'small': (6.0e-08, 9.0e-05),  # 5.960e-08, 8.965e-05  (512 rows)
    'tiny': (6.0e-08, 0.0e+00),  # 5.960e-08, 0.000e+00  (512 rows)
    'zero': (6.0e-08, 0.0e+00),  # 5.960e-08, 0.000e+00  (1 rows)
}
FLOORS['rotmat_to_aa'] = {
    'generic': (2.5e-07, 2.7e-07),  # 2.446e-07, 2.626e-07  (512 rows)
    'pi': (1.6e-07, 3.7e-07),  # 1.514e-07, 3.652e-07  (512 rows)
    'twopi': (2.2e-07, 2.8e-07),  # 2.189e-07, 2.719e-07  (512 rows)
    'small': (2.6e-07, 3.1e-07),  # 2.549e-07, 3.060e-07  (512 rows)
    'tiny': (2.5e-07, 2.0e-07),  # 2.406e-07, 1.911e-07  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
    'trace+': (2.0e-07, 3.1e-07),  # 1.923e-07, 3.094e-07  (512 rows)
    'trace-': (2.1e-07, 3.2e-07),  # 2.017e-07, 3.198e-07  (512 rows)
    'tie01+': (2.2e-07, 3.2e-07),  # 2.106e-07, 3.158e-07  (512 rows)
    'tie01-': (1.9e-07, 3.3e-07),  # 1.863e-07, 3.214e-07  (512 rows)
    'tie02+': (1.8e-07, 3.1e-07),  # 1.775e-07, 3.042e-07  (512 rows)
    'tie02-': (1.9e-07, 3.4e-07),  # 1.889e-07, 3.336e-07  (512 rows)
    'tie12+': (2.0e-07, 3.3e-07),  # 1.940e-07, 3.230e-07  (512 rows)
    'tie12-': (1.9e-07, 4.3e-07),  # 1.866e-07, 4.257e-07  (512 rows)
    'zero_matrix': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
    'offmanifold': (2.7e-07, 3.0e-07),  # 2.601e-07, 2.929e-07  (512 rows)
}
FLOORS['quat_mul'] = {
    'generic': (3.3e-07, 2.3e-07),  # 3.295e-07, 2.275e-07  (512 rows)
}
FLOORS['atan2s'] = {
    'generic': (8.7e-08, 1.8e-07),  # 8.681e-08, 1.770e-07  (512 rows)
    'both_tiny': (1.2e-07, 1.9e-07),  # 1.103e-07, 1.869e-07  (512 rows)
    'y_tiny': (7.1e-08, 1.8e-07),  # 7.052e-08, 1.797e-07  (512 rows)
    'x_tiny': (6.6e-08, 1.7e-07),  # 6.515e-08, 1.663e-07  (512 rows)
    'axes': (6.0e-08, 1.3e-07),  # 5.960e-08, 1.254e-07  (256 rows)
    'scale1e-5': (9.5e-08, 1.8e-07),  # 9.446e-08, 1.732e-07  (512 rows)
}
FLOORS['normalize3'] = {
    'scale1e-3': (1.2e-07, 1.8e-06),  # 1.181e-07, 1.713e-06  (511 rows)
    'scale1': (1.2e-07, 2.2e-06),  # 1.158e-07, 2.171e-06  (510 rows)
    'scale1e3': (1.4e-07, 8.3e-07),  # 1.331e-07, 8.229e-07  (510 rows)
    'below': (8.4e-08, 8.6e-08),  # 8.321e-08, 8.545e-08  (512 rows)
    'above': (1.0e-07, 1.8e-06),  # 9.989e-08, 1.738e-06  (511 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
}
FLOORS['quat_to_rotmat'] = {
    'generic': (4.1e-07, None),  # 4.051e-07, None  (512 rows)
    'pi': (4.6e-07, None),  # 4.563e-07, None  (512 rows)
    'twopi': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    'small': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    'tiny': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    'zero': (6.0e-08, None),  # 5.960e-08, None  (1 rows)
    '-generic': (4.1e-07, None),  # 4.051e-07, None  (512 rows)
    '-pi': (4.6e-07, None),  # 4.563e-07, None  (512 rows)
    '-twopi': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    '-small': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    '-tiny': (6.0e-08, None),  # 5.960e-08, None  (512 rows)
    '-zero': (6.0e-08, None),  # 5.960e-08, None  (1 rows)
    'scaled': (4.1e-07, None),  # 4.095e-07, None  (512 rows)
    'null': (6.0e-08, None),  # 5.960e-08, None  (1 rows)
}
FLOORS['quat_rotate'] = {
    'generic': (2.5e-07, None),  # 2.484e-07, None  (512 rows)
    'nonunit': (4.1e-07, None),  # 4.003e-07, None  (512 rows)
}
FLOORS['quat_heading'] = {
    'generic': (1.1e-07, None),  # 1.015e-07, None  (512 rows)
    'both_tiny': (1.1e-07, None),  # 1.046e-07, None  (512 rows)
    'y_tiny': (1.1e-07, None),  # 1.014e-07, None  (512 rows)
    'x_tiny': (6.5e-08, None),  # 6.439e-08, None  (512 rows)
    'axes': (6.0e-08, None),  # 5.960e-08, None  (256 rows)
    'scale1e-5': (9.2e-08, None),  # 9.131e-08, None  (512 rows)
}
FLOORS['quat_heading_q'] = {
    'generic': (1.1e-07, None),  # 1.070e-07, None  (512 rows)
    'small_w': (1.1e-07, None),  # 1.067e-07, None  (512 rows)
    'wz_zero': (6.0e-08, None),  # 5.960e-08, None  (64 rows)
    'below': (8.5e-08, None),  # 8.450e-08, None  (512 rows)
}
FLOORS['heading_quat'] = {
    'generic': (1.1e-07, 1.6e-06),  # 1.027e-07, 1.514e-06  (497 rows)
    'pi': (9.3e-08, 6.1e-07),  # 9.227e-08, 6.000e-07  (481 rows)
    'twopi': (6.0e-08, 2.4e-07),  # 5.960e-08, 2.373e-07  (455 rows)
    'small': (6.0e-08, 3.2e-07),  # 5.960e-08, 3.183e-07  (512 rows)
    'tiny': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (512 rows)
    'zero': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (1 rows)
}
FLOORS['sdiv'] = {
    'generic': (6.0e-08, 1.3e-07),  # 5.960e-08, 1.285e-07  (512 rows)
    'below+': (1.1e-07, 2.2e-07),  # 1.016e-07, 2.175e-07  (512 rows)
    'below-': (1.1e-07, 2.0e-07),  # 1.062e-07, 1.972e-07  (512 rows)
    'above+': (6.0e-08, 1.2e-07),  # 5.960e-08, 1.170e-07  (512 rows)
    'above-': (6.0e-08, 1.3e-07),  # 5.960e-08, 1.236e-07  (512 rows)
}
FLOORS['sqrt_clamped'] = {
    'generic': (6.0e-08, 9.0e-08),  # 5.960e-08, 8.944e-08  (512 rows)
    'below': (6.0e-08, 6.0e-08),  # 5.960e-08, 5.960e-08  (577 rows)
    'above': (6.0e-08, 9.3e-08),  # 5.960e-08, 9.287e-08  (512 rows)
}
FLOORS['mat3_mul'] = {
    'generic': (1.4e-07, 1.4e-07),  # 1.353e-07, 1.352e-07  (512 rows)
}
FLOORS['quat_mul_plain'] = {
    'generic': (1.6e-07, None),  # 1.548e-07, None  (512 rows)
}


def tolerance(prim, group, factor=FACTOR):
    f, g = FLOORS[prim][group]
    return factor * f, (None if g is None else factor * g)


def _round_up(x):
    if x == 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e * (1 - 1e-12)) * 10 ** e, 12)


def _fmt(v, f):
    return 'None' if v is None else f % v


if __name__ == '__main__':          # the floors behind FLOORS on this machine's CPU build of torch
    for p in PRIMS:
        m = measure_floors(p)
        print('FLOORS[%r] = {' % p)
        for k, (f, b) in m.items():
            print('    %r: (%s, %s),  # %s, %s  (%d rows)' % (k, _fmt(_round_up(f), '%.1e'), _fmt(None if b is None else _round_up(b), '%.1e'),
                                                                   _fmt(f, '%.3e'), _fmt(b, '%.3e'), groups(p)[k].shape[0]))
        print('}')
