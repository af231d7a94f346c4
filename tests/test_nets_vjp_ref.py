"""The fp64 VJP reference of tests/nets_vjp_common.py pinned to the unmodified reference's latent gradients (tests/golden/nets_latent.npz),
so that tests/test_nets_vjp_gpu.py measures the device against a product that is known to be the right one."""
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from tests import nets_vjp_common as vc


@pytest.mark.parametrize('T', [120, 300])
def test_fp64_vjp_reference_matches_the_reference_fixture(asset_root, golden, T):
    g = golden('nets_latent')
    inp, W = mg.net_inputs(T), mg.latent_loss_weights(T)
    pose, grad = vc.vjp(vc.infiller(asset_root), inp, W)
    e64 = (float(np.abs(grad - g['T%d_grad_latent' % T]).max()), float(np.abs(pose - g['T%d_body_pose' % T]).max()))
    pose32, grad32 = vc.vjp(vc.infiller(asset_root, torch.float32), inp, W)
    e32 = (float(np.abs(grad32 - g['T%d_grad_latent' % T]).max()), float(np.abs(pose32 - g['T%d_body_pose' % T]).max()))
    print('VJP reference vs fixture, T=%d: fp64 gradient %.2e pose %.2e, fp32 gradient %.2e pose %.2e (largest gradient %.3f)'
          % ((T,) + e64 + e32 + (np.abs(g['T%d_grad_latent' % T]).max(),)))
    assert grad.dtype == np.float64 and grad.shape == g['T%d_grad_latent' % T].shape
    assert e64[0] < 1e-6 and e64[1] < 1e-6
    assert e32[0] < 1e-6 and e32[1] < 1e-6


def test_fp64_vjp_reference_is_linear_and_cached(asset_root):
    """ref(s G) = s ref(G): the GPU tests answer every scaled upstream gradient from one cached product."""
    T = 71
    W = mg.latent_loss_weights(T, 3)
    ref = vc.Reference(asset_root)
    _, g1 = ref(3, T, 'W', W)
    _, g2 = vc.vjp(ref.net, mg.net_inputs(T, 3), W * 1024.0)
    assert g1.shape == (vc.n_windows(T), 128) and ref(3, T, 'W', None)[1] is g1
    assert np.abs(g2 - 1024.0 * g1).max() <= 1e-12 * np.abs(g2).max()


def test_route_sweep_sequences_keep_clear_of_relu_kinks(asset_root):
    """The route sweep compares every sequence's VJP with TOL: no ReLU input of theirs may lie where an fp32 forward could cross zero."""
    ref = vc.Reference(asset_root)
    worst = min((ref.margin(seed, n), seed, n) for seed, n in vc.ROUTE_SEQS)
    print('route sweep: smallest ReLU input %.2e (seed %d, length %d)' % worst)
    assert len(vc.ROUTE_SEQS) == 69 and len(set(vc.ROUTE_SEEDS)) == 69 and worst[0] >= vc.KINK
