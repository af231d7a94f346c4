"""The fp64 VJP reference of tests/traj_vjp_common.py checked on the CPU: its restated forward against traj_ref_common.predict, its gradients
against central differences, the kink list against the ReLU margins, the tolerances against the fp32 autograd's own rounding, and the five
mutations of the backward against those tolerances -- so that tests/test_traj_vjp_gpu.py measures the device against a product that is known
to be the right one, with bounds that a broken backward exceeds."""
import numpy as np
import pytest
import torch

from tests import traj_ref_common as tc
from tests import traj_vjp_common as vc


@pytest.fixture(scope='module')
def r64(asset_root):
    return vc.Reference(asset_root)


@pytest.fixture(scope='module')
def r32(asset_root, r64):
    return vc.Reference(asset_root, torch.float32, base=r64)


def test_restated_forward_matches_predict(r64):
    worst = 0.0
    for seed, T in (vc.SMALL[0], vc.SMALL[2], vc.MFMA[5]):
        j, e = r64.inputs(seed, T)
        want = tc.predict(r64.net, torch.tensor(j, dtype=torch.float64)[:, None], e[None])['local_traj'][0]
        worst = max(worst, float(np.abs(r64(seed, T)['local_traj'] - want).max()))
    print('restated forward vs predict: %.2e' % worst)
    assert worst <= 1e-12


def test_autograd_vjp_matches_central_differences(r64):
    """T = 12, B = 2, 32 random directions per input: d L / d direction by central differences in fp64 against <gradient, direction>."""
    T, seqs = 12, [s for s in vc.SMALL if s[1] == 12][:2]
    rng = np.random.default_rng(5)
    j = torch.tensor(np.stack([r64.inputs(*s)[0] for s in seqs], axis=1), dtype=torch.float64).requires_grad_(True)
    e = torch.tensor(np.stack([r64.inputs(*s)[1] for s in seqs]), dtype=torch.float64).requires_grad_(True)
    G = torch.tensor(np.stack([vc.upstream(s[0], T, 'dense') for s in seqs], axis=1), dtype=torch.float64)
    loss = lambda jj, ee: (vc.forward(r64.net, jj, ee) * G).sum()
    ge, gj = torch.autograd.grad(loss(j, e), (e, j))
    worst = 0.0
    with torch.no_grad():
        for x, g, step in ((e, ge, 1e-5), (j, gj, 1e-6)):
            for _ in range(32):
                d = torch.tensor(rng.normal(size=tuple(x.shape)))
                args = lambda v: (j, v) if x is e else (v, e)
                fd = float(loss(*args(x + step * d)) - loss(*args(x - step * d))) / (2 * step)
                an = float((g * d).sum())
                worst = max(worst, abs(fd - an) / abs(an))
    print('autograd vs central differences: relative error %.2e' % worst)
    assert worst <= 1e-6


def test_kink_list_is_what_the_margins_say(r64):
    m = {s: r64.margin(*s) for s in vc.CANDIDATES}
    kinked = [s for s in vc.CANDIDATES if m[s] < vc.KINK]
    print('smallest ReLU input over the candidates %.2e; left out: %s' % (min(m.values()), kinked))
    assert kinked == vc.KINKED and len(set(vc.CANDIDATES)) == len(vc.CANDIDATES)
    assert len(vc.KINKED) <= vc.MAX_LEFT_OUT and vc.MAX_LEFT_OUT == len(vc.CANDIDATES) // 4


def test_pinned_entries_have_no_gradient(r64):
    seed, T = vc.SMALL[2]
    j, e = r64.inputs(seed, T)
    _, g = vc.vjp(r64.net, j, e, [vc.upstream(seed, T, 'pinned')])
    assert not np.count_nonzero(g[0][0]) and not np.count_nonzero(g[0][1])


def test_tolerances_follow_the_fp32_floor(r32, r64):
    floor = vc.floors(r32, r64)
    print('fp32 autograd vs fp64: %s (constants %s)' % (', '.join('%s %.3e' % kv for kv in sorted(floor.items())), vc.FLOOR))
    assert tc.FLOOR_FACTOR == 16 and all(vc.TOL[k] == 16 * vc.FLOOR[k] for k in vc.FLOOR)
    for k, v in floor.items():
        assert vc.FLOOR[k] / 2 <= v <= vc.FLOOR[k] * 2, (k, v, vc.FLOOR[k])


@pytest.mark.parametrize('mut', vc.MUTATIONS)
def test_a_broken_backward_exceeds_the_bounds(r64, mut):
    """Each mutation on the sweep's sequences: g_joint_pos, the output every one of them reaches (d eps leaves through the decoder and the
    reparameterisation alone), differs from the sound reference by more than the device bound; the forward values stay (to rounding: a
    grafted gradient adds and subtracts the same number)."""
    worst = 0.0
    for seed, T in vc.kept(vc.SMALL)[:10]:
        good, bad = r64(seed, T), r64(seed, T, mut, max_len=100)
        worst = max(worst, max(vc.rel_err(bad[p][1], good[p][1]) for p in ('dense', 'last')))
        assert np.abs(bad['local_traj'] - good['local_traj']).max() <= 1e-12
    print('mutation %s (%s): g_joint_pos moves by %.2e of its largest entry (bound %.2e)' % (mut, vc.MUTATION_NAMES[mut], worst, vc.TOL['g_joint_pos']))
    assert worst > vc.TOL['g_joint_pos']
