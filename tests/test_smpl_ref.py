"""CPU: the basis of tests/test_smpl_fp64_gpu.py.  The restated forward of tests/smpl_ref_common.py is the port's, bit for bit; its written-out
Rodrigues backward is autograd's; every tolerance is 16 x the fp32 restatement's own rounding against fp64 (the constants are measured again
and must stay within [1/2, 2] x); the floor of the relative gradient measures catches at most 1 % of the non-zero entries; and every mutation of the
fp64 reference moves a compared output of every frame it touches by a stated number of tolerances.  Prints the floors and the mutation table.

The floors are reproduced by `python -m tests.smpl_ref_common` (one thread, this machine's CPU build of torch)."""
import numpy as np
import pytest
import torch

from tests import smpl_ref_common as sc

MUT_B = 16                       # the mutation batch: frames(16) -- six generic, six large, four small frames


@pytest.fixture(scope='module')
def refs(asset_root, tmp_path_factory):
    out = {}
    for name in sc.MODELS:
        root = sc.model_root(name, asset_root, tmp_path_factory.mktemp('smpl_' + name))
        out[name] = (sc.reference(root), sc.reference(root, torch.float32))
    return out


@pytest.fixture(scope='module')
def grad_refs(refs):
    fr = sc.frames(sc.GRAD_B, sc.GRAD_FAMILIES)
    return fr, {name: sc.reference_gradients(refs[name][0], fr) for name in sc.MODELS}


def test_frames_are_distinct_and_hold_every_family():
    fr = sc.frames(sc.FWD_B)
    rows = np.concatenate([fr['pose'], fr['betas'], fr['trans1']], axis=1)
    assert len(np.unique(rows, axis=0)) == sc.FWD_B
    assert set(sc.group(l) for l in fr['label'][:64]) == set(sc.GROUPS) and set(fr['label'][:8]) >= {'generic', 'large'}
    assert set(sc.group(l) for l in sc.frames(33, sc.GRAD_FAMILIES)['label']) == set(sc.GROUPS)
    ang = np.linalg.norm(fr['pose'].reshape(-1, 24, 3), axis=-1)
    for a in sc.LARGE_ANGLES:
        assert (np.abs(ang[:64, 0] - a) < 1e-5).any() and (np.abs(ang[:64, 1:] - a) < 1e-5).any(), a        # root and body, within 64 frames
    assert np.array_equal(sc.frames(9)['pose'], fr['pose'][:9])
    assert (np.abs(fr['betas']).max(1) == 5.0).sum() >= 4 and fr['scale'][3] == np.float32(0.05)


@pytest.mark.parametrize('name', sc.MODELS)
def test_restated_forward_is_the_ports(refs, name):
    m = refs[name][0]
    fr = sc.frames(9)
    dt = torch.float64
    pose, betas, trans, scale = (torch.tensor(fr[k], dtype=dt) for k in ('pose', 'betas', 'trans1', 'scale'))
    with torch.no_grad():
        for kw in ({}, dict(root_trans=trans), dict(root_trans=trans, root_scale=scale), dict(root_trans=trans, orig_joints=True)):
            ref = m(global_orient=pose[:, :3], body_pose=pose[:, 3:], betas=betas, **kw)
            v, j = sc.forward(m, pose, betas, kw.get('root_trans'), kw.get('root_scale'), kw.get('orig_joints', False))
            assert ref.vertices.dtype == dt and torch.equal(ref.vertices, v) and torch.equal(ref.joints, j), sorted(kw)
    if name == 'conditioned':
        assert int((m.lbs_weights != 0).sum(1).max()) == sc.WEIGHTS_KEPT and int((m.J_regressor != 0).sum(1).max()) <= sc.REGRESSOR_KEPT
        assert int((m.J_regressor_extra != 0).sum(1).max()) <= sc.REGRESSOR_KEPT
        assert abs(float(m.posedirs.std()) / float(refs['fixture'][0].posedirs.std()) - sc.POSEDIRS_GAIN) < 1e-6


def test_written_out_rodrigues_backward_is_autograds(refs, grad_refs):
    fr, g64 = grad_refs
    m = refs['fixture'][0]
    g = sc.gradients(sc.reference_call(m, rodrigues_fn=True), fr, 'joints+verts anchored', 'general', torch.float64)
    worst = max(float(np.max(e)) for e, _ in sc.grad_errors(g, g64['fixture']['joints+verts anchored']).values())
    print('written-out Rodrigues backward against autograd, fp64: %.1e' % worst)
    assert worst < 1e-9          # (1e-4 rad frames: 1 - cos theta keeps 8 of fp64's 16 digits)


def _band(what, floor, const):
    print('%-46s fp32 against fp64 %.3e   constant %.1e   tolerance %.1e' % (what, floor, const, sc.FLOOR_FACTOR * const))
    assert 0.5 * const <= floor <= 2.0 * const, (what, floor, const)


@pytest.mark.parametrize('name', sc.MODELS)
def test_forward_tolerances_are_16_floors(refs, name):
    m64, m32 = refs[name]
    fr = sc.frames(sc.FWD_B)
    floor = sc.measure_forward_floor(m32, sc.forward_outputs(m64, fr), fr)
    assert set(floor) == set(sc.FWD_FLOOR[name])
    for k in sc.FWD_KEYS:
        assert set(floor[k]) == set(sc.FWD_FLOOR[name][k])
        for n, e in floor[k].items():
            _band('%s, %s %s [m]' % (name, k, n), e, sc.FWD_FLOOR[name][k][n])


@pytest.mark.parametrize('name', sc.MODELS)
def test_gradient_tolerances_are_16_floors(refs, grad_refs, name):
    fr, g64 = grad_refs
    floor = sc.measure_grad_floor(refs[name][1], g64[name], fr)
    assert set(floor) == set(sc.GRAD_FLOORS[name])
    for k, d in floor.items():
        assert set(d) == set(sc.GRAD_FLOORS[name][k]), k
        for grp, e in sorted(d.items()):
            _band('%s, d/d %s, %s frames [relative]' % (name, k, grp), e, sc.GRAD_FLOORS[name][k][grp])


@pytest.mark.parametrize('name', sc.MODELS)
def test_gradient_floor_catches_at_most_one_percent(grad_refs, name):
    """On the reference alone: the share of non-zero entries whose fp64 norm is under GRAD_FLOOR x the median of its tensor."""
    fr, g64 = grad_refs
    for v in sc.VARIANTS:
        for k, (_, share) in sc.grad_errors(g64[name][v], g64[name][v]).items():
            print('%s, %s, d/d %s: %.2f %% of the entries under the floor' % (name, v, k, 100 * share))
            assert share <= 0.01, (v, k, share)


# by how many tolerances each mutation has to move the most-moved compared output of EVERY frame it touches, per model (None: not asserted on
# that model, the other one carries it).  (a) and (b) are ROUNDINGS of a matrix to 2^-11 of its entries: they cannot move anything by 10
# tolerances of 16 fp32 floors, only by a few -- measured 2.4 to 6.5 for (a) on the conditioned model and 1.5 to 8.4 for (b) on the fixture
# model; what is asserted is that every touched frame fails its comparison with a margin.  (a) on the fixture model (posedirs of sigma 0.002:
# the lost plane is 1e-5 m, 0.1 to 1 tolerance) is NOT caught there: the conditioned model carries it.
MOVES = {'a': (None, 2), 'b': (1.4, 1.4), 'c': (10, 10), 'd': (10, 10), 'e': (10, 10), 'f': (10, 10)}


def _touched(m, fr):
    """Frames a mutation can change: (c) and (d) act through pose features, which a small-angle frame does not have at the size of a tolerance
    (1e-2 rad x posedirs 0.002 is 2e-5 m) -- asserted on the generic and large frames; the others on every frame."""
    main = [b for b, l in enumerate(fr['label']) if sc.group(l) == 'main']
    if m in 'ab':        # (frame 3 has root_scale 0.05: whatever moves its mesh moves the anchored output twenty times less, under one tolerance)
        return [b for b in (main if m == 'a' else range(len(fr['label']))) if fr['scale'][b] >= 0.5]
    return main if m in 'cd' else list(range(len(fr['label'])))


@pytest.mark.parametrize('m', sc.MUTATIONS)
def test_every_forward_mutation_moves_an_output(refs, m):
    """Vertices and joints of the anchored call at ~1 m, every vertex compared, against FWD_TOL of that call.  Least-moved touched frame, in
    tolerances (fixture / conditioned): printed, copied to DESIGN.md.  (a) on the fixture model sits AT the tolerance (posedirs of sigma 0.002:
    the lost plane is 1e-5 m) -- the conditioned model carries it."""
    fr = sc.frames(MUT_B)
    for i, name in enumerate(sc.MODELS):
        m64 = refs[name][0]
        ref = sc.forward_outputs(m64, fr, keys=('1m',))['1m']
        got = sc.forward_outputs(m64, fr, mut=m, keys=('1m',))['1m']
        ratio = np.maximum(np.abs(got['verts'] - ref['verts']).max((1, 2)) / sc.fwd_tol(name, '1m', 'verts'),
                           np.abs(got['joints'] - ref['joints']).max((1, 2)) / sc.fwd_tol(name, '1m', 'joints'))
        t = _touched(m, fr)
        print('(%s) %s, %s model: least-moved of %d touched frames %.1f tolerances, most-moved %.0f' % (m, sc.MUTATION_NAMES[m], name, len(t), ratio[t].min(), ratio[t].max()))
        if MOVES[m][i] is not None:
            assert ratio[t].min() >= MOVES[m][i], (name, ratio[t])


@pytest.mark.parametrize('m', sc.GRAD_MUTATIONS)
def test_every_gradient_mutation_moves_a_gradient(refs, grad_refs, m):
    """(g1) on d/d pose of joint 22, (g2) on d/d betas, (g3) on d/d pose: generic and large frames of the gradient batch, the full anchored loss,
    in tolerances of the 'main' group; at least 10 on every such frame, on both models."""
    fr, g64 = grad_refs
    v = 'joints+verts anchored'
    main = [b for b, l in enumerate(fr['label']) if sc.group(l) == 'main']
    for name in sc.MODELS:
        ref = g64[name][v]
        if m == 'g1':
            got = {k: x.copy() for k, x in ref.items()}
            got['pose'][:, 22] *= 1.01
        else:
            got = sc.gradients(sc.reference_call(refs[name][0], mut=m), fr, v, 'general', torch.float64)
        key = 'betas' if m == 'g2' else 'pose'
        err = sc.grad_errors(got, ref)[key][0]
        ratio = err.reshape(len(err), -1).max(1)[main] / sc.grad_tol(name, key, 'main')
        print('(%s) %s, %s model: d/d %s of the least-moved frame %.0f tolerances, most-moved %.0f' % (m, sc.MUTATION_NAMES[m], name, key, ratio.min(), ratio.max()))
        assert ratio.min() >= 10, (name, ratio)
