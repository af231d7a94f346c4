"""The reference, the inputs and the floors of tests/rotmath_ref_common.py, checked without a GPU: the input conditions hold for every row, the
restatements that carry the mutations equal the port's functions bit for bit, every floor re-measured lies within [1/2, 2] x its constant and under
1e-3, the g++ build of glamr_amd/csrc/rotmath.hpp (tests/hostsim/rotmath_shim.cpp, exact operators) is within HOST_FACTOR x floor of fp64 on every
group, every mutation of the reference is caught by its group, and tools/rotmath_probe.hip compiles for gfx950 under the library's three flag sets."""
import os
import subprocess
import numpy as np
import pytest
import torch

from tests import rotmath_ref_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_GROUPS = {'generic', 'pi', 'twopi', 'small', 'tiny'}
# the groups the tests must at least hold, per primitive
REQUIRED = {
    'aa_to_quat': ANGLE_GROUPS | {'zero'}, 'aa_to_rotmat_k': ANGLE_GROUPS | {'zero'}, 'aa_to_rotmat_s': ANGLE_GROUPS | {'zero'},
    'heading_quat': ANGLE_GROUPS | {'zero'},
    'quat_to_aa': ANGLE_GROUPS | {'zero'} | {'-' + g for g in ANGLE_GROUPS | {'zero'}},
    'quat_to_rotmat': ANGLE_GROUPS | {'zero'} | {'-' + g for g in ANGLE_GROUPS | {'zero'}},
    'rotmat_to_quat': ANGLE_GROUPS | {'zero', 'trace+', 'trace-', 'tie01+', 'tie01-', 'tie02+', 'tie02-', 'tie12+', 'tie12-', 'offmanifold', 'zero_matrix'},
    'rotmat_to_aa': ANGLE_GROUPS | {'zero', 'trace+', 'trace-', 'tie01+', 'tie01-', 'tie02+', 'tie02-', 'tie12+', 'tie12-', 'offmanifold', 'zero_matrix'},
    'rot6d_to_rotmat': {'scale1e-3', 'scale1', 'scale1e3', 'angle1+', 'angle1-', 'angle0.1+', 'angle0.1-', 'angle0.03+', 'angle0.03-', 'zero',
                        'zero_column', 'axis_column'},
    'normalize3': {'scale1e-3', 'scale1', 'scale1e3', 'below', 'above', 'zero'},
    'atan2s': {'generic', 'both_tiny', 'y_tiny', 'x_tiny', 'axes', 'scale1e-5'},
    'quat_heading': {'generic', 'both_tiny', 'y_tiny', 'x_tiny', 'axes', 'scale1e-5'},
    'sdiv': {'generic', 'below+', 'below-', 'above+', 'above-'}, 'sqrt_clamped': {'generic', 'below', 'above'},
    'quat_mul': {'generic'}, 'quat_mul_plain': {'generic'}, 'quat_rotate': {'generic'}, 'mat3_mul': {'generic'},
    'quat_heading_q': {'generic', 'small_w', 'wz_zero', 'below'},
}


def test_every_primitive_has_its_groups_and_floors():
    assert set(REQUIRED) == set(rc.PRIMS) == set(rc.FLOORS) == set(rc.REF)
    for p in rc.PRIMS:
        g = rc.groups(p)
        assert REQUIRED[p] <= set(g), p
        assert set(g) == set(rc.FLOORS[p]), p
        assert all(v.shape[0] >= 1 and v.dtype == np.float32 for v in g.values()), p
        assert sum(v.shape[0] for v in g.values()) <= 16384, p
    assert {m[0] for m in rc.MUTATIONS.values()} <= set(rc.PRIMS)


@pytest.mark.parametrize('prim', rc.PRIMS)
def test_input_conditions(prim):
    """No row sits on a threshold, fp32 and fp64 take the same branches for every row, and every thresholded decision is taken both ways."""
    x, g, sl = rc.table_rows(prim)
    assert rc.well_conditioned(prim, x).all() and np.all(rc.grad_condition(prim, x, g) <= rc.GRAD_COND_MAX)
    d32, d64 = rc.decisions(prim, x, torch.float32), rc.decisions(prim, x, torch.float64)
    for (name, v, kind, thr), b32, b64 in zip(d64, rc.branches(d32), rc.branches(d64)):
        assert np.array_equal(b32, b64), (prim, name)
        if kind == 'rel':
            assert np.all(np.abs(v - thr) > rc.REL_MARGIN * thr), (prim, name)
            if prim != 'quat_to_rotmat':                 # (its 1e-12 clamp: only the zero quaternion is under it)
                assert b64.any() and not b64.all(), (prim, name, 'one side of the threshold is never taken')
        elif kind == 'zero':
            assert np.all((np.abs(v) > rc.ZERO_MARGIN) | (v == 0)) and b64.any() and not b64.all(), (prim, name)


def test_rotmat_to_quat_groups_sit_next_to_their_branch_boundaries():
    for prim in ('rotmat_to_quat', 'rotmat_to_aa'):
        g = rc.groups(prim)

        def branch(m):
            tr = m[:, 0] + m[:, 4] + m[:, 8]
            return np.where(tr > 0, 0, np.where((m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8]), 1, np.where(m[:, 4] > m[:, 8], 2, 3)))
        for sgn, want in (('+', {0}), ('-', {1, 2, 3})):
            m = g['trace' + sgn].astype(np.float64)
            tr = np.abs(m[:, 0] + m[:, 4] + m[:, 8])
            assert set(branch(m)) == want and tr.min() > 0.9e-5 and tr.max() < 1.1e-2
        for (i, j), (hi, lo) in (((0, 1), (1, 2)), ((0, 2), (1, 3)), ((1, 2), (2, 3))):
            for sgn, want in (('+', hi), ('-', lo)):
                m = g['tie%d%d%s' % (i, j, sgn)].astype(np.float64)
                d = np.abs(m[:, 4 * i] - m[:, 4 * j])
                assert set(branch(m)) == {want} and d.min() > 0.9e-5 and d.max() < 1.1e-2, (i, j, sgn)


@pytest.mark.parametrize('prim', sorted(rc.PORT))
def test_restatement_equals_the_port(prim):
    """The restatements that carry the mutations are the port's functions: same bits, forward and gradient, in fp32 and in fp64."""
    x, g, _ = rc.table_rows(prim)
    for dt in (torch.float32, torch.float64):
        a, b = rc.ref_eval(prim, x, g, dt), rc.ref_eval(prim, x, g, dt, fn=rc.PORT[prim])
        assert np.array_equal(a[0], b[0], equal_nan=True), (prim, dt)
        if a[1] is not None:
            assert np.array_equal(a[1], b[1], equal_nan=True), (prim, dt)


@pytest.mark.parametrize('prim', rc.PRIMS)
def test_floors_are_what_the_fp32_restatement_does(prim):
    m = rc.measure_floors(prim)
    for grp, vals in m.items():
        for what, got, const in zip(('forward', 'gradient'), vals, rc.FLOORS[prim][grp]):
            assert (got is None) == (const is None), (prim, grp, what)
            if got is None:
                continue
            print('%-16s %-12s %-8s floor %.3e  constant %.1e' % (prim, grp, what, got, const))
            assert const <= 1e-3, (prim, grp, what)
            assert 0.5 * const <= got <= 2.0 * const, (prim, grp, what, got, const)


@pytest.mark.parametrize('prim', rc.PRIMS)
def test_host_build_of_the_header_is_within_four_floors_of_fp64(prim):
    out, gx = rc.shim_block(prim)
    assert np.all(np.isfinite(out)) and (gx is None or np.all(np.isfinite(gx)))
    for grp, (ef, eg) in rc.group_errors(prim, out, gx).items():
        tf_, tg = rc.tolerance(prim, grp, rc.HOST_FACTOR)
        print('%-16s %-12s forward %.2f floors%s' % (prim, grp, ef / rc.FLOORS[prim][grp][0],
                                                      '' if not tg else ', gradient %.2f floors' % (eg / rc.FLOORS[prim][grp][1])))
        assert ef <= tf_, (prim, grp, 'forward', ef, tf_)
        if eg is not None:
            assert eg <= tg, (prim, grp, 'gradient', eg, tg)


@pytest.mark.parametrize('name', sorted(rc.MUTATIONS))
def test_mutation_of_the_reference_is_caught(name):
    """The g++ build of the real header lies outside its group's device tolerance from the mutated fp64 reference."""
    prim, grp, fn = rc.MUTATIONS[name]
    x, g, sl = rc.table_rows(prim)
    out, gx = rc.shim_block(prim)
    ef, eg = rc.group_errors(prim, out, gx, ref=rc.ref_eval(prim, x, g, fn=fn))[grp]
    tf_, tg = rc.tolerance(prim, grp)
    print('%s: forward %.3e (tolerance %.1e), gradient %s (tolerance %s)' % (name, ef, tf_, eg, tg))
    assert ef > tf_ or (eg is not None and eg > tg), name


@pytest.mark.parametrize('build', rc.BUILDS)
def test_probe_cross_compiles(build, tmp_path):
    cmd = rc.probe_command(build, os.path.join(ROOT, 'tools', 'rotmath_probe.hip'), str(tmp_path / 'rotmath_probe.o'), compile_only=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_probe_file_format_round_trips(tmp_path):
    """The writer and the reader of the probe's files agree on the layout (the probe's part is the device test's)."""
    blocks = [b for b in rc.probe_blocks() if b[0] in ('sdiv', 'quat_heading', 'wakeup')]
    rc.write_probe_input(str(tmp_path / 'in.bin'), blocks)
    raw = np.fromfile(str(tmp_path / 'in.bin'), dtype=np.int32)
    assert raw[0] == rc.MAGIC and raw[1] == 3 and raw[2] == rc.SPEC[blocks[0][1]][0] and raw[3] == blocks[0][2].shape[0]
    outs = [(rc.shim_eval(p, x, g if g is not None else np.zeros((x.shape[0], rc.SPEC[p][2]), np.float32))) for _, p, x, g in blocks]
    with open(str(tmp_path / 'out.bin'), 'wb') as f:
        for o, gx in outs:
            f.write(o.tobytes())
            if gx is not None:
                f.write(gx.tobytes())
    back = rc.read_probe_output(str(tmp_path / 'out.bin'), blocks)
    for (label, _, _, _), (o, gx) in zip(blocks, outs):
        assert np.array_equal(back[label][0], o) and (gx is None or np.array_equal(back[label][1], gx))
