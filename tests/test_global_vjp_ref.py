"""CPU: the local-to-global step's VJP (csrc/traj_global_bwd.hpp, what glamr_traj_local_to_global_backward launches) on the single-threaded host
runtime against the fp64 autograd reference of tests/global_vjp_common.py, the basis of its tolerances (floors, screening, mutations), and
the floors and the fixture of the composite chain tests/test_global_vjp_gpu.py checks through MotionTrajJointModel.inference_grad."""
import ctypes

import numpy as np
import pytest
import torch

from tests import global_vjp_chain as ch
from tests import global_vjp_common as gc
from tests import hostsim


def _p(a, t=ctypes.c_float):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def host_vjp(case, G, lens='table', serial=False):
    """The header's algorithm on the host runtime with the device's order of additions in the scans (serial: HostRT's own serial loop)."""
    lib = hostsim.build('traj_global_bwd_host')
    L = np.ascontiguousarray(case['L'], np.float32)
    B, T = L.shape[:2]
    G = [None if g is None else np.ascontiguousarray(g, np.float32) for g in G]
    out = np.full((B, T, 11), 7.0, np.float32)                  # (every entry must be overwritten)
    table = np.asarray(case['lens'], np.int32) if lens == 'table' else lens
    lib.hostsim_traj_global_bwd.restype = ctypes.c_int
    assert lib.hostsim_traj_global_bwd(B, T, _p(table, ctypes.c_int32), _p(L), _p(G[0]), _p(G[1]), _p(G[2]), _p(out), int(serial)) == 0
    return out


@pytest.mark.parametrize('name', [n for n, _, _ in gc._case_specs()])
def test_host_algorithm_matches_fp64_autograd(name):
    case = gc.cases()['cases'][name]
    tol = gc.tol(name)
    worst, serial = {k: 0.0 for k in gc.GROUPS}, {k: 0.0 for k in gc.GROUPS}
    for pattern in gc.PATTERNS:
        got = host_vjp(case, gc.upstream(case, pattern))        # NaN in every row at or beyond a length
        e = gc.errors(host_vjp(case, gc.upstream(case, pattern), serial=True), gc.ref64(name, pattern), case['lens'])
        serial = {k: max(serial[k], e[k]) for k in serial}
        for b, n in enumerate(case['lens']):
            assert (got[b, n:] == 0).all()
        assert np.isfinite(got).all()
        e = gc.errors(got, gc.ref64(name, pattern), case['lens'])
        worst = {k: max(worst[k], e[k]) for k in worst}
    print('host VJP %s: %s' % (name, ', '.join('%s %.2e (bound %.2e; serial scans %.2e)' % (k, worst[k], tol[k], serial[k]) for k in worst)))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])


def test_lengths_are_clamped_and_null_means_T():
    case = gc.cases()['cases']['ragged3']
    T = case['L'].shape[1]
    G = gc.upstream(case, 'all', nan_pad=False)
    full = dict(case, lens=(T,) * len(case['lens']))
    assert np.array_equal(host_vjp(full, G, lens=None), host_vjp(full, G))
    wild = dict(case, lens=(T + 1000, -5, T))
    got = host_vjp(wild, G)
    ref = host_vjp(dict(case, lens=(T, 0, T)), G)
    assert np.array_equal(got, ref) and (got[1] == 0).all()


def test_floors_and_screening():
    st = gc.cases()
    print('screening: %d generated, %d dropped' % (st['generated'], st['dropped']))
    assert set(st['cases']) == {n for n, _, _ in gc._case_specs()}                  # every length and both batches have a case
    assert st['dropped'] <= gc.MAX_DROPPED_SHARE * st['generated']
    # the families are there: each branch of rotmat_to_quat on at least 8 frames of every sequence of 64 frames or more, both sides of quat_to_aa's sign
    for name, case in st['cases'].items():
        for n, br in zip(case['lens'], case['branches']):
            if n >= 64:
                assert (np.bincount(br, minlength=4) >= 8).all(), (name, n)
    for name in st['cases']:
        f = gc.measure_floor(name)
        print('floor %s: %s' % (name, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], gc.FLOOR[name][k]) for k in f)))
        for k, v in f.items():
            c = gc.FLOOR[name][k]
            assert 0.5 * c <= v <= 2.0 * c, (name, k, v, c)


@pytest.mark.parametrize('mut', list(gc.MUTATIONS))
def test_mutations_of_the_reference_are_caught(mut):
    """Each mutation of the reference's backward moves some compared group of every case it touches by at least 2 tolerances."""
    st = gc.cases()['cases']
    touched = 0
    # frames a sequence needs for the mutation to touch it: a row before or after the first; for the dR/dtheta term a rotated row with a
    # displacement (row n // 2 = row 1 of two frames is the row with dxy = 0)
    need = {'no_suffix': 2, 'theta_t': 2, 'no_dR': 3}
    for name, case in st.items():
        lens, T = case['lens'], case['L'].shape[1]
        if mut == 'pad_rows' and all(n == T for n in lens):
            continue                                                    # no padded rows
        if mut in need and max(lens) < need[mut]:
            continue
        ref = gc.ref64(name, 'all')
        bad = gc.reference(case, 'all', mut=mut)
        tol = gc.tol(name)
        # per sequence the mutation touches: some group moves by 2 tolerances
        for b, n in enumerate(lens):
            if (mut == 'pad_rows' and n == T) or n < need.get(mut, 1):
                continue
            e = gc.errors(bad[b:b + 1], ref[b:b + 1], (n,))
            ratio = max(e[k] / tol[k] if tol[k] > 0 else (np.inf if e[k] > 0 else 0.0) for k in e)
            print('mutation %-9s %-8s sequence %d (%3d frames): %s -> %.3g tolerances' % (mut, name, b, n, ', '.join('%s %.2e' % kv for kv in e.items()), ratio))
            assert ratio >= 2.0, (mut, name, b, e, tol)
            touched += 1
    assert touched > 0


# ---- the composite chain of MotionTrajJointModel.inference_grad ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ch.CHAIN))
def test_chain_reference_margins_floors_and_fixture(asset_root, golden, name):
    """The fp64 composite (infiller -> FK -> predictor -> local-to-global -> SMPL joints) run again: its input seeds keep every ReLU
    pre-activation of both priors KINK away from zero, the fixture the device test reads holds its gradients, and the fp32 run's deviation is
    the stored floor within [1/2, 2]."""
    ref = ch.reference(asset_root, name)
    for b, (seed, n) in enumerate(ch.sequences(name)):
        m = ch.relu_margin(asset_root, name, b, seed)
        print('chain %s sequence %d (seed %d, %d frames): smallest |ReLU pre-activation| %.2e' % (name, b, seed, n, m))
        assert m >= ch.KINK
    g = golden(ch.FIXTURE)
    for k, v in ref.items():
        assert g[k].shape == v.shape and ch.rel_err(g[k], v) < 1e-9, k
    f = ch.measure_floor(asset_root, name)
    print('chain floor %s: %s' % (name, ', '.join('%s %.3e (constant %.1e)' % (k, f[k], ch.FLOOR[name][k]) for k in f)))
    for k, v in f.items():
        assert 0.5 * ch.FLOOR[name][k] <= v <= 2.0 * ch.FLOOR[name][k], (name, k, v)
