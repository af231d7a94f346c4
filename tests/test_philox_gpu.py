"""MI355X tests of the priors' Philox latent streams (csrc/rng.hip) against the NumPy twin of the stream definition
(tests/philox_ref.py): raw words bit for bit, normals against float64, offsets and tails, the one-launch batch draw, and the switch
GlobalReconOptimizer.latent_source through init_resident and a captured step."""
import os

import numpy as np
import pytest
import torch

from glamr_amd import _lib
from glamr_amd.models import latent_rng
from glamr_amd.models.priors import num_windows, NZ
from glamr_amd.utils import synth
from tests import philox_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KEYS = ('kp_2d_pred', 'params', 'j_local', 'cam_pose', 'orient_world', 'trans_world', 'orient_cam_in_world', 'losses')
# max |x_gpu - x_f64|: converting a 32-bit integer to fp32 costs 2^-24 relative in u and in theta; with r <= sqrt(2 * 33 ln 2) = 6.77 the angle
# term dominates at about 2.5e-6 absolute and function evaluation adds a few ulp of 6.77.  Derived, not tuned.
NORMAL_TOL = 1e-5


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_bits_equal_the_twin_bit_for_bit():
    rs = np.random.RandomState(5)
    r64 = lambda: (int(rs.randint(0, 2 ** 32, dtype=np.uint64)) << 32) | int(rs.randint(0, 2 ** 32, dtype=np.uint64))
    cases = [(r64(), r64(), int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(0, 2 ** 32 - 5000, dtype=np.uint64)), int(rs.randint(1, 3000))) for _ in range(24)]
    cases += [(0, 0, 0, 0, 1), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 1),           # the known-answer corners: block and sub of all ones
              (r64(), r64(), 7, 2 ** 32 - 1000, 1000), (r64(), r64(), 2 ** 32 - 1, 2 ** 32 - 1 - 777, 777)]      # ranges that end at block 2^32 - 1 / 2^32 - 2
    for seed, seq_id, sub, first, n in cases:
        got = _u32(latent_rng.bits(seed, seq_id, sub, first, n, DEV))
        assert np.array_equal(got, R.bits(seed, seq_id, sub, first, n)), (seed, seq_id, sub, first, n)
    assert _u32(latent_rng.bits(0, 0, 0, 0, 1, DEV)).tolist() == [list(R.KAT[0][2])]
    assert _u32(latent_rng.bits(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 1, DEV)).tolist() == [list(R.KAT[1][2])]


def _box_muller_gpu(words):
    w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(DEV)
    out = torch.empty(w.shape, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().glamr_rng_box_muller(w.shape[0], _lib.ptr(w), _lib.ptr(out), _lib.current_stream()))
    return out.cpu().numpy()


def test_normals_against_the_float64_twin():
    """max |x_gpu - x_f64| <= 1e-5 over 2^22 draws of four streams, and over the map on chosen integers: every pair of
    x in {0, 1, 2, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 2, 2^32 - 1} (u at both ends of its range and at the switch between the two logarithm forms)
    and y at the quadrant boundaries.  Measured on the MI355X: 6.7e-7 over the four streams, 3.8e-7 on the chosen integers (printed by this test)."""
    worst = 0.0
    streams = ((0, 0, 0), (12345, 2 ** 33, 1), (2 ** 40 + 3, R.seq_id_of('seq0'), 6), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1))
    for seed, seq_id, sub in streams:
        n = 2 ** 20
        got = latent_rng.normal(seed, seq_id, sub, 0, n, DEV).cpu().numpy().astype(np.float64)
        err = float(np.abs(got - R.normals(seed, seq_id, sub, 0, n)).max())
        print('stream %s: max |gpu - f64| = %.3e over %d draws' % ((seed, seq_id, sub), err, n))
        worst = max(worst, err)
        assert err <= NORMAL_TOL, err
        # the stream call IS the map applied to the raw words
        words = R.bits(seed, seq_id, sub, 0, 4096)
        assert np.array_equal(_box_muller_gpu(words).reshape(-1), latent_rng.normal(seed, seq_id, sub, 0, 4 * 4096, DEV).cpu().numpy())
    xs = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]
    ys = [0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 30 - 1, 3 * 2 ** 30, 2 ** 32 - 1, 0x12345678, 0x9abcdef0]
    pairs = [(x, y) for x in xs for y in ys]
    words = np.array([pairs[i] + pairs[(7 * i + 3) % len(pairs)] for i in range(len(pairs))], dtype=np.uint32)        # every pair in both halves of a block
    got = _box_muller_gpu(words).astype(np.float64)
    err = float(np.abs(got - R.box_muller(words)).max())
    print('chosen integers (u and theta at the ends of their ranges): max |gpu - f64| = %.3e' % err)
    assert np.isfinite(got).all() and err <= NORMAL_TOL, err
    # x = 0xffffffff: u = 1 - 2^-33, r = 2^-16 -- not 0, which a logarithm of the rounded u would give
    r = np.hypot(got[:, 0], got[:, 1])
    last = words[:, 0] == 2 ** 32 - 1
    assert last.any() and np.allclose(r[last], 2.0 ** -16, rtol=1e-5)
    print('normals: worst max |gpu - f64| = %.3e (bound %.0e)' % (max(worst, err), NORMAL_TOL))


@pytest.mark.parametrize('seed', R.STAT_SEEDS)
def test_statistics_of_the_gpu_output(seed):
    """The four statistics of tests/test_philox_host.py on the GPU's fp32 output, same streams, same caps."""
    for seq_id in R.STAT_SEQ_IDS:
        stats = R.normal_stats(latent_rng.normal(seed, seq_id, 0, 0, R.STAT_N, DEV).cpu().numpy())
        print('seed %d seq %d: mean %.2f var %.2f kurtosis %.2f KS %.2f' % ((seed, seq_id) + stats))
        for s, cap in zip(stats, R.STAT_CAPS):
            assert s <= cap, (seed, seq_id, stats)


def test_offsets_and_tails():
    """Any first element and count: the call equals the slice of one long call bit for bit and writes nothing outside its range."""
    seed, seq_id, sub = 31337, R.seq_id_of('basketball'), 3
    full = latent_rng.normal(seed, seq_id, sub, 0, 1024, DEV).cpu().numpy()
    assert np.abs(full.astype(np.float64) - R.normals(seed, seq_id, sub, 0, 1024)).max() <= NORMAL_TOL
    poison = np.float32(-777.25)
    for pad in (4, 5):                                          # output start 16-byte aligned, and not
        for first in (0, 1, 2, 3, 5, 127, 128):
            for n in (1, 3, 4, 6, 509):
                buf = torch.full((pad + n + 8,), float(poison), dtype=torch.float32, device=DEV)
                latent_rng.normal(seed, seq_id, sub, first, n, DEV, out=buf[pad:pad + n])
                h = buf.cpu().numpy()
                assert np.array_equal(h[pad:pad + n], full[first:first + n]), (pad, first, n)
                assert (h[:pad] == poison).all() and (h[pad + n:] == poison).all(), (pad, first, n)
    # consecutive calls concatenate to what one call gives
    parts = [latent_rng.normal(seed, seq_id, sub, a, b - a, DEV).cpu().numpy() for a, b in ((0, 7), (7, 130), (130, 131), (131, 1024))]
    assert np.array_equal(np.concatenate(parts), full)
    # n == 0 is a no-op
    buf = torch.full((8,), float(poison), dtype=torch.float32, device=DEV)
    latent_rng.normal(seed, seq_id, sub, 3, 0, DEV, out=buf[:0])
    assert (buf.cpu().numpy() == poison).all()


def test_latents_draw_rows_do_not_depend_on_the_batch():
    seed = 2 ** 40 + 3
    A, B, C = (R.seq_id_of('A'), 0), (R.seq_id_of('B'), 5), (12, 2)            # (sequence id, person id)

    def draw(slots, nw):
        m, t = latent_rng.draw(seed, [s for s, _ in slots], [p for _, p in slots], nw, DEV)
        return m.cpu().numpy(), t.cpu().numpy()
    m3, t3 = draw([A, B, C], 3)
    for k, (sid, pid) in enumerate((A, B, C)):
        # row (slot, window, k) = element window * 128 + k of stream (seq_id, 2 * person_id); the predictor's row is stream + 1
        assert np.array_equal(m3[k].reshape(-1), latent_rng.normal(seed, sid, 2 * pid, 0, 3 * NZ, DEV).cpu().numpy())
        assert np.array_equal(t3[k], latent_rng.normal(seed, sid, 2 * pid + 1, 0, NZ, DEV).cpu().numpy())
        mr, tr = R.latents(seed, sid, pid, 3)
        assert np.abs(m3[k] - mr).max() <= NORMAL_TOL and np.abs(t3[k] - tr).max() <= NORMAL_TOL
    # permuting, dropping, duplicating slots changes no surviving row
    m, t = draw([C, A], 3)
    assert np.array_equal(m[0], m3[2]) and np.array_equal(m[1], m3[0]) and np.array_equal(t[0], t3[2]) and np.array_equal(t[1], t3[0])
    m, t = draw([B], 3)
    assert np.array_equal(m[0], m3[1]) and np.array_equal(t[0], t3[1])
    m, t = draw([B, A, B], 3)
    assert np.array_equal(m[0], m3[1]) and np.array_equal(m[2], m3[1]) and np.array_equal(m[1], m3[0]) and np.array_equal(t[2], t3[1])
    # padding slots are zero, and move nothing
    m, t = draw([A, (A[0], -1), B, (0, -1)], 3)
    assert not m[1].any() and not t[1].any() and not m[3].any() and not t[3].any()
    assert np.array_equal(m[0], m3[0]) and np.array_equal(m[2], m3[1]) and np.array_equal(t[2], t3[1])
    # more windows: the first three unchanged
    m8, t8 = draw([A, B, C], 8)
    assert np.array_equal(m8[:, :3], m3) and np.array_equal(t8, t3) and m8[:, 3:].any()
    # another seed: other numbers
    m, _ = latent_rng.draw(seed + 1, [A[0]], [A[1]], 3, DEV)
    assert not np.array_equal(m.cpu().numpy()[0], m3[0])


@pytest.fixture(scope='module')
def make_model(asset_root):
    from glamr_amd.global_recon.models import model_dict
    from glamr_amd.global_recon.configs import get_config
    from glamr_amd.lib.models.smpl import SMPL
    from glamr_amd.models.prior_models import MotionTrajJointModel
    smpl = SMPL(os.path.join(asset_root, 'data', 'body_models', 'smpl'), pose_type='body26fk',
                extra_regressor_path=os.path.join(asset_root, 'data', 'J_regressor_extra.npy')).to(DEV)
    mt = MotionTrajJointModel(None, DEV, None, smpl=smpl, results_root=os.path.join(asset_root, 'results'))

    def make(cfg_id='glamr_dynamic'):
        return model_dict['global_recon_model'](get_config(cfg_id), DEV, None, smpl=smpl, mt_model=mt)
    return make


@pytest.fixture(scope='module')
def seqs():
    md = synth.make_smpl_model()
    return (synth.make_in_dict(seed=61, num_frames=96, num_persons=2, smpl_model=md, seq_name='two_people'),
            synth.make_in_dict(seed=62, num_frames=140, num_persons=1, smpl_model=md, seq_name='long_one'),
            synth.make_in_dict(seed=63, num_frames=96, num_persons=1, smpl_model=md, seq_name='short_one'))


def _step(model, batch, latents=None, max_iters=3):
    """stage_inputs + optimize_resident; returns (rin, packed, clones of the latents: they live in the priors' resident arrays, which the next
    step on this stream overwrites)."""
    rin = model.stage_inputs(batch, latents)
    _, packed = model.optimize_resident(rin, max_iters=max_iters)
    torch.cuda.synchronize()
    return rin, packed, tuple(x.clone() for x in packed.latents)


def test_philox_latents_through_the_model(make_model, seqs):
    A, B, C = seqs
    model = make_model()
    assert model.latent_source == 'torch'
    with pytest.raises(ValueError):
        model.latent_source = 'bogus'
    model.latent_source, model.latent_seed = 'philox', 11
    rin, packed, (meps, teps) = _step(model, [A, B, C])
    P, nw = rin.P, meps.shape[1]
    assert P == 2 and nw == num_windows(int(rin.lens.max())) and meps.shape[0] == 3 * P
    # packed.latents = the direct draw (slot = scene * P + person; the second slot of a one-person scene is padding)
    sids = [R.seq_id_of(n) for n in ('two_people', 'long_one', 'short_one')]
    slot_seq, slot_person = [sids[0], sids[0], sids[1], sids[1], sids[2], sids[2]], [0, 1, 0, -1, 0, -1]
    dm, dt = latent_rng.draw(11, slot_seq, slot_person, nw, DEV)
    assert torch.equal(meps, dm) and torch.equal(teps, dt)
    for k in (0, 1, 2, 4):
        mr, tr = R.latents(11, slot_seq[k], slot_person[k], nw)
        assert np.abs(meps[k].cpu().numpy() - mr).max() <= NORMAL_TOL and np.abs(teps[k].cpu().numpy() - tr).max() <= NORMAL_TOL
    assert not meps[3].any() and not teps[5].any()
    first = {k: v.clone() for k, v in packed.t.items() if torch.is_tensor(v)}
    # the same batch handed those latents explicitly under the default source: every array bit for bit
    hm, ht = meps.cpu().numpy(), teps.cpu().numpy()
    given = [{idx: {'motion': hm[si * P + pi], 'traj': ht[si * P + pi][None]} for pi, idx in enumerate(ids)} for si, ids in enumerate(rin.ids)]
    model.latent_source = 'torch'
    _, packed2, (m2, t2) = _step(model, [A, B, C], given)
    assert torch.equal(m2, meps) and torch.equal(t2, teps)
    assert set(first) == set(k for k, v in packed2.t.items() if torch.is_tensor(v)) and len(first) > 20
    for k, v in first.items():
        assert torch.equal(v, packed2.t[k]), k
    # a sequence alone gets the latents it gets inside the batch (fewer windows there: the batch was padded to the longest sequence)
    model.latent_source = 'philox'
    rin_a, _, (ma, ta) = _step(model, [A])
    nwa = ma.shape[1]
    assert nwa < nw and torch.equal(ma, meps[:2, :nwa]) and torch.equal(ta, teps[:2])
    _, _, (mc, tc) = _step(model, [C, B])
    assert torch.equal(mc[0], meps[4]) and torch.equal(mc[1], meps[2]) and torch.equal(tc[0], teps[4]) and torch.equal(tc[1], teps[2])
    # a person dropped from a scene does not move the other: person 1 of A alone
    only1 = dict(A, est={1: A['est'][1]})
    _, _, (m1, t1) = _step(model, [only1])
    assert torch.equal(m1[0], meps[1, :m1.shape[1]]) and torch.equal(t1[0], teps[1])
    # an explicit in_dict['seq_id'] is the sequence id whichever source was set when the batch was STAGED
    withid = dict(C, seq_id=2 ** 40 + 17)
    _, _, (mi, ti) = _step(model, [withid])
    want_m, want_t = latent_rng.draw(11, [2 ** 40 + 17], [0], mi.shape[1], DEV)
    assert torch.equal(mi, want_m) and torch.equal(ti, want_t) and not torch.equal(ti[0], teps[4])
    model.latent_source = 'torch'
    rin_t = model.stage_inputs([withid])
    model.latent_source = 'philox'
    _, packed_t = model.optimize_resident(rin_t, max_iters=3)
    torch.cuda.synchronize()
    assert rin_t.latent_seq_ids is not None and torch.equal(packed_t.latents[0], want_m) and torch.equal(packed_t.latents[1], want_t)
    # another seed: other latents; the host-side path (init_data_batch_host) draws the same numbers
    model.latent_seed = 12
    _, _, (mb, _) = _step(model, [A])
    assert not torch.equal(mb, ma)
    model.latent_seed = 11
    seen, orig = {}, model.mt_model.infer_padded

    def spy(body_pose, visible, lens, m, t, **kw):
        seen['m'], seen['t'] = m.clone(), t.clone()
        return orig(body_pose, visible, lens, m, t, **kw)
    model.mt_model.infer_padded = spy
    try:
        model.init_data_batch_host([A, C])                         # rows: A person 0, A person 1, C person 0 (no padding slots there)
    finally:
        del model.mt_model.infer_padded
    torch.cuda.synchronize()
    nwh = seen['m'].shape[1]
    assert seen['m'].shape[0] == 3 and torch.equal(seen['m'], meps[[0, 1, 4], :nwh]) and torch.equal(seen['t'], teps[[0, 1, 4]])


def test_default_source_depends_on_the_batch_and_is_untouched(make_model, seqs):
    """Under the default source a person's draw is decided by its slot in the batch -- the defect 'philox' removes -- and the draws are exactly
    torch.randn's in today's order (the guard that the default path did not move)."""
    A, B, C = seqs
    model = make_model()
    assert model.latent_source == 'torch'
    torch.manual_seed(5)
    rin, _, (meps, teps) = _step(model, [A, B, C])
    torch.manual_seed(5)
    want_m = torch.randn(tuple(meps.shape), device=DEV)
    want_t = torch.randn(tuple(teps.shape), device=DEV)
    assert torch.equal(meps, want_m) and torch.equal(teps, want_t)
    torch.manual_seed(5)
    _, _, (mb, tb) = _step(model, [B, A])                        # A moved from slots 0-1 to slots 2-3
    nwb = min(mb.shape[1], meps.shape[1])
    assert not torch.equal(mb[2:4, :nwb], meps[0:2, :nwb]) and not torch.equal(tb[2:4], teps[0:2])


def test_captured_step_follows_the_seed_without_recapture(make_model):
    """capture_resident under 'philox': one captured step replayed under seeds s1, s2, s1 (glamr_rng_set_seed on the step's stream, no
    re-capture) gives the latents and outputs of plain launches under s1, s2, s1 bit for bit; outputs poisoned between replays."""
    md = synth.make_smpl_model()
    model = make_model()
    model.latent_source, model.latent_seed = 'philox', 3
    batch = [synth.make_in_dict(seed=70 + i, num_frames=96, num_persons=1, smpl_model=md) for i in range(5)]
    st = torch.cuda.Stream()
    rin = model.stage_inputs(batch)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        model.optimize_resident(rin, max_iters=6)                  # first run on this stream: allocations, attribute calls
    torch.cuda.synchronize()
    rg = model.capture_resident(rin, max_iters=6, stream=st, check=True)
    assert rg.before_replay is not None
    s1, s2 = 1234567, 2 ** 63 + 9
    seen = []
    for seed in (s1, s2, s1):
        model.latent_seed = seed
        with torch.cuda.stream(st):
            _, ref = model.optimize_resident(rin, max_iters=6)     # plain launches under this seed
        torch.cuda.synchronize()
        want = {k: ref.t[k].clone() for k in KEYS}
        want_lat = tuple(x.clone() for x in ref.latents)
        for k in KEYS:
            rg.packed.t[k].fill_(float('nan'))
        for x in rg.packed.latents:
            x.fill_(float('nan'))
        torch.cuda.synchronize()
        rg.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(rg.packed.t[k], want[k]), (seed, k)
        assert all(torch.equal(a, b) for a, b in zip(rg.packed.latents, want_lat))
        mr, _ = R.latents(seed, R.seq_id_of(batch[0]['seq_name']), 0, want_lat[0].shape[1])
        assert np.abs(want_lat[0][0].cpu().numpy() - mr).max() <= NORMAL_TOL
        seen.append((want_lat, want['kp_2d_pred']))
    assert not torch.equal(seen[0][0][0], seen[1][0][0]) and not torch.equal(seen[0][1], seen[1][1])
    assert torch.equal(seen[0][0][0], seen[2][0][0]) and torch.equal(seen[0][1], seen[2][1])


def test_stand_alone_priors_honour_the_switch(make_model):
    """MotionTrajJointModel.inference under 'philox': row b is the sequence (its name hashed when given, else the row index), sample k the
    person id -- a row's result does not depend on the rows around it."""
    model = make_model()
    mt = model.mt_model
    g = torch.Generator().manual_seed(3)
    pose = (torch.randn(3, 70, 69, generator=g) * 0.2).to(DEV)
    mask = torch.ones(3, 70, device=DEV)
    try:
        mt.latent_source, mt.latent_seed = 'philox', 21
        full = mt.inference({'in_body_pose': pose, 'frame_mask': mask, 'seq_name': ['a', 'b', 'c']}, sample_num=2)
        one = mt.inference({'in_body_pose': pose[1:2], 'frame_mask': mask[1:2], 'seq_name': 'b'}, sample_num=2)
        # (the networks may pick other kernels for another batch size: the DRAWS are what must agree, and other draws move the results by far more)
        close = lambda a, b: bool(torch.allclose(a, b, atol=1e-3, rtol=0))
        for k in ('infer_out_body_pose', 'infer_out_trans', 'infer_out_orient'):
            assert close(full[k][1], one[k][0]), k
        assert not torch.equal(full['infer_out_trans'][1, 0], full['infer_out_trans'][1, 1])          # the samples differ
        again = mt.inference({'in_body_pose': pose, 'frame_mask': mask, 'seq_name': ['a', 'b', 'c']}, sample_num=2)
        assert torch.equal(again['infer_out_trans'], full['infer_out_trans'])
        # without names the row index is the sequence id
        anon = mt.inference({'in_body_pose': pose, 'frame_mask': mask}, sample_num=1)
        anon0 = mt.inference({'in_body_pose': pose[:1], 'frame_mask': mask[:1]}, sample_num=1)
        assert close(anon['infer_out_trans'][0], anon0['infer_out_trans'][0]) and not close(anon['infer_out_trans'][0], full['infer_out_trans'][0, 0])
        # the two priors called on their own draw the same streams
        inf = mt.mfiller.inference({'in_body_pose': pose, 'frame_mask': mask, 'seq_name': ['a', 'b', 'c']}, sample_num=2, multi_step=True)
        assert close(inf['infer_out_body_pose'], full['infer_out_body_pose'])
        tr = mt.traj_predictor.inference({'in_body_pose': full['infer_out_body_pose'][:, 0].contiguous(), 'seq_name': ['a', 'b', 'c']}, sample_num=2)
        assert close(tr['infer_out_trans'][:, 0], full['infer_out_trans'][:, 0])
    finally:
        mt.latent_source, mt.latent_seed = 'torch', 0


def _spy(obj, name, record):
    """Records the `eps` every call of obj.<name> is given (clones), until the returned function is called."""
    orig = getattr(obj, name)

    def wrapped(*args, **kw):
        if kw.get('eps') is not None:
            record.append(kw['eps'].clone())
        return orig(*args, **kw)
    setattr(obj, name, wrapped)
    return lambda: delattr(obj, name)


def _stream_rows(seed, sids, persons, prior, first_elem=0):
    return torch.stack([latent_rng.normal(seed, s, 2 * p + prior, first_elem, NZ, DEV) for s, p in zip(sids, persons)])


def test_joint_model_general_path_keeps_the_stream_contract(make_model):
    """MotionTrajJointModel.inference with 'pose' / 'trans' in the batch (and with recon=True) goes infiller -> pred_trajectory -> predictor over
    a batch of FLATTENED (row, sample) pairs.  The latents the predictor actually uses there (the eps handed to _clip_pass) are those of
    (the row's sequence, sample k as person): bit for bit the streams of the one-call path, for a named row alone and inside a batch."""
    from oracle import make_golden as mg
    mt = make_model().mt_model
    y = mg.multi_step_inputs()['infiller']
    g = torch.Generator().manual_seed(9)
    full = {k: torch.tensor(v) for k, v in y.items() if k in ('pose', 'pose_mask', 'frame_mask')}
    full['trans'] = torch.randn(2, 85, 3, generator=g)
    names, S, seed = ['first', 'second'], 3, 77
    try:
        mt.latent_source, mt.latent_seed = 'philox', seed
        for recon in (False, True):
            used = {}
            for tag, rows in (('batch', [0, 1]), ('alone', [1])):
                rec = []
                undo = _spy(mt.traj_predictor, '_clip_pass', rec)
                try:
                    out = mt.inference(dict({k: v[rows] for k, v in full.items()}, seq_name=[names[r] for r in rows]), sample_num=S, recon=recon)
                finally:
                    undo()
                assert len(rec) == 1 and rec[0].shape == (len(rows) * S, NZ), [r.shape for r in rec]      # (the reconstruction pass draws nothing)
                assert out['infer_out_trans'].shape[:2] == (len(rows), S) and bool(torch.isfinite(out['infer_out_trans']).all())
                used[tag] = rec[0].view(len(rows), S, NZ)
                sids = [R.seq_id_of(names[r]) for r in rows]
                want = _stream_rows(seed, [s for s in sids for _ in range(S)], [k for _ in sids for k in range(S)], latent_rng.PRIOR_TRAJ)
                assert torch.equal(rec[0], want), (tag, recon)
                # ... which are the one-call path's trajectory draws of the same named rows
                assert torch.equal(used[tag], latent_rng.draw_samples(seed, {'seq_name': [names[r] for r in rows]}, len(rows), S, 0, DEV)[1])
            assert torch.equal(used['alone'][0], used['batch'][1]) and not torch.equal(used['batch'][0], used['batch'][1])
        # without names the row index is the sequence id in BOTH priors and in both paths: row 1 / sample 2 is stream (1, person 2), not (1 * S + 2, person 0)
        rec = []
        undo = _spy(mt.traj_predictor, '_clip_pass', rec)
        try:
            mt.inference(dict(full), sample_num=S)
        finally:
            undo()
        assert torch.equal(rec[0], _stream_rows(seed, [0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2], latent_rng.PRIOR_TRAJ))
        # explicit per-row ids win over names
        rec = []
        undo = _spy(mt.traj_predictor, '_clip_pass', rec)
        try:
            mt.inference(dict(full, seq_name=names, seq_id=[5, 2 ** 63 + 1]), sample_num=2)
        finally:
            undo()
        assert torch.equal(rec[0], _stream_rows(seed, [5, 5, 2 ** 63 + 1, 2 ** 63 + 1], [0, 1, 0, 1], latent_rng.PRIOR_TRAJ))
    finally:
        mt.latent_source, mt.latent_seed = 'torch', 0


def test_single_window_clip_and_chunked_draws(make_model):
    """The remaining stand-alone draws: MotionInfillerVAE.inference(multi_step=False) (one window: elements [0, 128) of the infiller stream),
    TrajPredVAE.inference through _clip_pass, and its chunked form (chunk c: elements [128 c, 128 (c + 1)) of the trajectory stream)."""
    from oracle import make_golden as mg
    mt = make_model().mt_model
    x, y = mg.train_inputs(), mg.multi_step_inputs()
    tt = lambda d: {k: torch.tensor(v) for k, v in d.items() if not k.startswith('in_')}
    names, seed = ['p', 'q'], 5
    sids = [R.seq_id_of(n) for n in names]
    try:
        mt.latent_source, mt.latent_seed = 'philox', seed
        rec = []
        undo = _spy(mt.mfiller, '_window_pass', rec)
        try:
            d = mt.mfiller.inference(dict(tt(x['infiller']), seq_name=names), sample_num=3, multi_step=False)
        finally:
            undo()
        assert d['infer_out_body_pose'].shape == (2, 3, 40, 69) and len(rec) == 1
        assert torch.equal(rec[0], _stream_rows(seed, [s for s in sids for _ in range(3)], [0, 1, 2] * 2, latent_rng.PRIOR_INFILLER))
        rec = []
        undo = _spy(mt.traj_predictor, '_clip_pass', rec)
        try:
            d = mt.traj_predictor.inference(dict(tt(x['traj']), seq_name=names), sample_num=2)
            assert d['infer_out_trans'].shape == (2, 2, 100, 3) and len(rec) == 1
            assert torch.equal(rec[0], _stream_rows(seed, [sids[0], sids[0], sids[1], sids[1]], [0, 1, 0, 1], latent_rng.PRIOR_TRAJ))
            # 130 frames = two chunks of 100: chunk c draws elements [128 c, 128 (c + 1))
            del rec[:]
            d = mt.traj_predictor.inference(dict(tt(y['traj']), seq_name=names), sample_num=2, multi_step=True)
            assert bool(torch.isfinite(d['infer_out_trans']).all()) and len(rec) == 2
            for c in (0, 1):
                assert torch.equal(rec[c], _stream_rows(seed, [sids[0], sids[0], sids[1], sids[1]], [0, 1, 0, 1], latent_rng.PRIOR_TRAJ, first_elem=c * NZ)), c
            assert not torch.equal(rec[0], rec[1])
        finally:
            undo()
    finally:
        mt.latent_source, mt.latent_seed = 'torch', 0
