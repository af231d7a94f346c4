"""bench.py --dump-outputs: the sample of scenes is fixed by its seed, per-person rows follow their scene, and every array is float32 or float64."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


class _Model:
    _FETCH = ('fr_start', 'params', 'kp_2d_pred')


class _Packed:
    def __init__(self, S, P, T=5):
        self.device = torch.device('cpu')
        g = torch.Generator().manual_seed(1)
        self.t = {'fr_start': torch.arange(S * P, dtype=torch.int32), 'params': torch.randn(S, 7, generator=g),
                  'kp_2d_pred': torch.randn(S * P, T, 3, 2, generator=g)}
        if P > 1:
            self.t['rel_transform_cam'] = torch.randn(S, P, P, T, 12, generator=g)
        self.person_arrays = {'smpl_pose': torch.randn(S * P, T, 69, generator=g), 'nets_pose': torch.randn(S * P, T, 69, generator=g)}
        self.latents = (torch.randn(S * P, 2, 4, generator=g), torch.randn(S * P, 4, generator=g))


def test_sample_is_seeded_and_rows_follow_their_scene(tmp_path):
    S, P = 200, 2
    pk = _Packed(S, P)
    a, b = bench.step_outputs(_Model(), pk, S), bench.step_outputs(_Model(), pk, S)
    idx = a['scene_index'].astype(np.int64)
    assert len(idx) == bench.DUMP_SCENES and np.array_equal(idx, np.sort(np.unique(idx))) and idx.max() < S
    assert sorted(a) == sorted(b) == ['fr_start', 'kp_2d_pred', 'latent_motion', 'latent_traj', 'pa_smpl_pose', 'params', 'rel_transform_cam', 'scene_index']
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k])
    assert np.array_equal(a['params'], pk.t['params'].numpy()[idx])
    assert np.array_equal(a['kp_2d_pred'], pk.t['kp_2d_pred'].numpy().reshape(S, P, 5, 3, 2)[idx])
    assert np.array_equal(a['latent_motion'], pk.latents[0].numpy().reshape(S, P, 2, 4)[idx])
    assert np.array_equal(a['fr_start'], pk.t['fr_start'].numpy().reshape(S, P)[idx].astype(np.float64))
    bench.write_outputs(a, str(tmp_path / 'd'))
    assert np.array_equal(np.load(str(tmp_path / 'd' / 'pa_smpl_pose.npy')), a['pa_smpl_pose'])


def test_small_batch_is_written_whole():
    out = bench.step_outputs(_Model(), _Packed(3, 1), 3)
    assert np.array_equal(out['scene_index'], np.arange(3.0)) and out['params'].shape == (3, 7)
