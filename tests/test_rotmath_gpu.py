"""MI355X: glamr_amd/csrc/rotmath.hpp as the three programs it is on the device -- the library's default flags (v_rcp_f32 / v_sqrt_f32, fused
multiply-adds), the flags of grecon.hip (approximate `/` and sqrtf as well) and -DGLAMR_ROTMATH_IEEE=1 with the flags of init.hip -- against the fp64
reference of tests/rotmath_ref_common.py on its input groups.  tools/rotmath_probe.hip is compiled once per build with the flags of
glamr_amd/build.py and run ONCE on the whole table; a compile or a run that fails is remembered and reported by every test of that build, and after a
run that faulted or hung no further build is started.

  * every primitive, forward and gradient, within FACTOR = 8 x floor of fp64 on every group; all-zero reference rows exactly zero; everything finite;
  * the IEEE build equals the g++ build of the header (tests/hostsim, exact operators, no contraction) bit for bit on the primitives that call no
    library function, their backwards, and the exactly (anti)parallel +-lr columns of the detection-gap wake-up: the claim init.hip is
    built on, and the one that lets the CPU twins of tests/hostsim speak for the device;
  * div_ and sqrt_rn_ equal numpy's correctly rounded fp32 quotient and root bit for bit; sincos_ of the two fast builds keeps the bounds of
    tests/test_rotmath_grads.py::test_sincos_accuracy."""
import os
import subprocess
import numpy as np
import pytest

from tests import rotmath_ref_common as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the primitives that call no library function (no sine / cosine / atan2): IEEE operators only, so the device build and the g++ build must agree
BIT_EQUAL = ('normalize3', 'rot6d_to_rotmat', 'rotmat_to_quat', 'quat_mul', 'quat_mul_plain', 'quat_rotate', 'quat_heading_q', 'quat_to_rotmat', 'sdiv',
             'sqrt_clamped', 'mat3_mul')
# primitive: why the compiler, not the header, keeps it from being bit-equal -- such a primitive is held to FACTOR x floor alone
BIT_EQUAL_EXCEPTIONS = {}

_STATE = {'results': {}, 'stop': None}


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp('rotmath_probe')
    blocks = rc.probe_blocks()
    rc.write_probe_input(str(d / 'in.bin'), blocks)
    return d, blocks


def _run(build, table):
    """Compiles and runs the probe of `build` once; the outcome -- results or the failure -- is kept for every later test."""
    if build in _STATE['results']:
        return _STATE['results'][build]
    d, blocks = table
    exe, outp = str(d / ('rotmath_probe_' + build)), str(d / ('out_%s.bin' % build))
    res = None
    if _STATE['stop']:
        res = 'not started: ' + _STATE['stop']
    else:
        try:
            c = subprocess.run(rc.probe_command(build, os.path.join(ROOT, 'tools', 'rotmath_probe.hip'), exe), capture_output=True, text=True, timeout=600)
            if c.returncode != 0:
                res = 'compile failed:\n' + c.stderr[-2000:]
        except subprocess.TimeoutExpired:
            res = 'compile timed out'
        if res is None:
            try:
                r = subprocess.run([exe, str(d / 'in.bin'), outp], capture_output=True, text=True, timeout=120)
                if r.returncode != 0:
                    res = 'probe exited with %d:\n%s\n%s' % (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
                    _STATE['stop'] = 'the %s build of the probe exited with %d' % (build, r.returncode)
                else:
                    res = {'table': rc.parse_probe_table(r.stdout), 'out': rc.read_probe_output(outp, blocks)}
            except subprocess.TimeoutExpired:
                res = 'probe timed out'
                _STATE['stop'] = 'the %s build of the probe timed out' % build
    _STATE['results'][build] = res
    return res


@pytest.fixture(scope='module')
def default_build(table):
    return _run('default', table)


@pytest.fixture(scope='module')
def grecon_build(table):
    return _run('grecon', table)


@pytest.fixture(scope='module')
def ieee_build(table):
    return _run('ieee', table)


def _get(request, build):
    res = request.getfixturevalue(build + '_build')
    if isinstance(res, str):
        pytest.fail('%s build: %s' % (build, res), pytrace=False)
    return res


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('build', rc.BUILDS)
def test_probe_table_is_the_reference_table(request, build):
    assert _get(request, build)['table'] == tuple(rc.TABLE)


@pytest.mark.parametrize('prim', rc.PRIMS)
@pytest.mark.parametrize('build', rc.BUILDS)
def test_primitive_is_within_eight_floors_of_fp64(request, build, prim):
    out, gx = _get(request, build)['out'][prim]
    errs = rc.group_errors(prim, out, gx)
    worst_f = max(e[0] / rc.FLOORS[prim][g][0] for g, e in errs.items())
    worst_g = max([e[1] / rc.FLOORS[prim][g][1] for g, e in errs.items() if e[1] is not None and rc.FLOORS[prim][g][1] > 0] or [0.0])
    print('%-8s %-16s achieved / floor: forward %.2f, gradient %.2f' % (build, prim, worst_f, worst_g))
    assert np.all(np.isfinite(out)) and (gx is None or np.all(np.isfinite(gx))), (build, prim)
    for grp, (ef, eg) in errs.items():
        tf_, tg = rc.tolerance(prim, grp)
        assert ef <= tf_, (build, prim, grp, 'forward', ef, tf_)
        if eg is not None:
            assert eg <= tg, (build, prim, grp, 'gradient', eg, tg)


@pytest.mark.parametrize('prim', BIT_EQUAL)
def test_ieee_build_equals_the_host_build_bit_for_bit(request, prim):
    if prim in BIT_EQUAL_EXCEPTIONS:
        return          # held to FACTOR x floor by the test above; the entry says why
    res = _get(request, 'ieee')['out']
    cases = [(prim, res[prim], rc.shim_block(prim))]
    if prim == 'rot6d_to_rotmat':
        _, _, w, g = [b for b in rc.probe_blocks() if b[0] == 'wakeup'][0]
        cases.append(('wakeup', res['wakeup'], rc.shim_eval(prim, w, g)))
    for label, (out, gx), (h_out, h_gx) in cases:
        bad = np.flatnonzero((_bits(out) != _bits(h_out)).any(axis=1))
        assert bad.size == 0, (label, 'forward', bad.size, bad[:5], out[bad[:2]], h_out[bad[:2]])
        if h_gx is not None:
            bad = np.flatnonzero((_bits(gx) != _bits(h_gx)).any(axis=1))
            assert bad.size == 0, (label, 'gradient', bad.size, bad[:5], gx[bad[:2]], h_gx[bad[:2]])


@pytest.mark.parametrize('build', rc.BUILDS)
def test_div_is_the_correctly_rounded_quotient(request, build):
    got = _get(request, build)['out']['div'][0][:, 0]
    v = rc.div_operands()
    want = v[:, 0] / v[:, 1]
    bad = np.flatnonzero(_bits(got) != _bits(want))
    print('%s: div_ differs from the IEEE quotient in %d of %d pairs' % (build, bad.size, got.size))
    assert bad.size == 0, (build, bad.size, v[bad[:5]], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize('build', rc.BUILDS)
def test_sqrt_rn_is_the_correctly_rounded_root(request, build):
    """Bit for bit on 0 and on every argument from SQRT_RN_EXACT_FROM = 2^-102 up, where no residual of the correction can underflow to zero (the
    domain rotmath.hpp documents; grecon_algo.hpp adam() is the caller, and a root under 2^-51 is half an ulp of the 1e-8 it is added to).  Below
    it the residuals are rounded to the denormal grid and the result is only within one ulp -- measured on the MI355X, all three builds alike: 1886
    of the 1e6 log-uniform normal arguments off by one ulp, every one of them below 1.8e-34 (2^-112)."""
    got = _get(request, build)['out']['sqrt_rn'][0][:, 0]
    x = rc.sqrt_operands()
    want = np.sqrt(x)
    off = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))
    bad = np.flatnonzero(off != 0)
    print('%s: sqrt_rn_ differs from the IEEE root at %d of %d arguments%s' % (build, bad.size, got.size,
                                                                                 '' if not bad.size else ', all of them <= %.3e' % x[bad].max()))
    dom = (x == 0) | (x >= rc.SQRT_RN_EXACT_FROM)
    assert dom.sum() > 0.85 * x.size
    assert not off[dom].any(), (build, x[bad[-5:]], got[bad[-5:]], want[bad[-5:]])
    assert off.max() <= 1, (build, off.max())


@pytest.mark.parametrize('build', ('default', 'grecon'))
def test_sincos_accuracy_on_the_device(request, build):
    res = _get(request, build)['out']
    for i, ((lim, tol_ulp, tol_abs), x) in enumerate(zip(rc.SINCOS_CASES, rc.sincos_operands())):
        out = res['sincos%d' % i][0]
        ref = np.stack([np.sin(x.astype(np.float64)), np.cos(x.astype(np.float64))], axis=1)
        err = np.abs(out - ref)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        big = np.abs(ref) > 1e-3                       # near a zero of the function an ulp is tiny: the absolute bound applies there
        print('%s: |x| <= %g: %.3e absolute, %.2f ulp' % (build, lim, err.max(), (err / ulp)[big].max()))
        assert err.max() < tol_abs, (build, lim, err.max())
        assert (err / ulp)[big].max() < tol_ulp, (build, lim, (err / ulp)[big].max())
        assert np.all(np.abs(out[:, 0].astype(np.float32) ** 2 + out[:, 1].astype(np.float32) ** 2 - 1.0) < 4e-7)
