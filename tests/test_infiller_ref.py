"""CPU: the basis of tests/test_infiller_gpu.py.  The restated forward of tests/infiller_ref_common.py is the port's; both checkpoints keep
the fp16-split kernels; the floor tables are what this machine measures; the fp32 port is inside every tolerance; and every mutation of the
fp64 reference moves a compared output of every sequence it touches by at least 2 tolerances."""
import numpy as np
import pytest
import torch

from oracle import make_golden as mg
from tests import infiller_ref_common as ic

# the sliding-window inference over fewer sequences than the tables were measured over (ic.ALL_SEQS): a subset that holds every length
# edge, every mask kind and the long sequences; the three window modes over all of ic.ROUTE_SEQS, as the tables (one batched forward:
# the fp32 port's rounding depends on the batch it runs in); the re-measured floors are held to [1/2, 2] x the tables
FLOOR_SEQS = ic.ROUTE_SEQS[:24] + ic.LONG_SEQS
MARGIN = 2.0
# what the shipped checkpoint cannot show, and why the conditioned one exists: with U(+-1/sqrt(fan_in)) weights attention is close to
# uniform, a softmax scale of 1.01 in the encoder moves the least-moved sequence by 0.8 tolerances (context), the most-moved by less than 2
SHIPPED_BLIND = ('q_enc',)


@pytest.fixture(scope='module')
def r64(asset_root):
    return {c: ic.Reference(asset_root, conditioned=c == 'conditioned') for c in ic.CHECKPOINTS}


@pytest.fixture(scope='module')
def r32(asset_root):
    return {c: ic.Reference(asset_root, torch.float32, c == 'conditioned') for c in ic.CHECKPOINTS}


def test_sequences_are_net_inputs_and_distinct():
    """Kind 'gap' is mg.net_inputs bit for bit (pose, mask, latent draws); no two slots of any batch hold the same data."""
    for seed, T, kind in [s for s in ic.ALL_SEQS if s[2] == 'gap'][:6]:
        a, b = mg.net_inputs(T, seed), ic.seq_inputs(seed, T, kind)
        assert np.array_equal(a['in_body_pose'][0], b['pose']) and np.array_equal(a['frame_mask'][0], b['vis']) and np.array_equal(a['in_motion_latent'], b['eps'])
    assert len(set(s[0] for s in ic.ALL_SEQS)) == len(ic.ALL_SEQS)
    lens = set(s[1] for s in ic.ROUTE_SEQS)
    assert {11, 40, 41, 70, 71} <= lens and max(lens) <= 100 and set(s[2] for s in ic.ROUTE_SEQS[:24]) == set(ic.KINDS)
    s = ic.seq_inputs(501, 71, 'straddle')['vis']
    assert s[34] == 1 and not s[35:45].any() and s[45] == 1          # generated frames 35..39 of window 0, 40..44 of window 1
    assert not ic.window_inputs((502, 71, 'blind'))['frame_mask'][ic.PAST:].any()


@pytest.mark.parametrize('ckpt', ic.CHECKPOINTS)
def test_restated_forward_is_the_ports(asset_root, ckpt):
    """inference(multi_step=True) and the training-mode pass of MotionInfillerVAE().double() against the restatement with the port's own
    position table (1e-13: torch's attention and the restated one sum in different orders); the table the reference uses instead differs
    from the port's by what fp32 arithmetic loses in pos * mul."""
    net = ic.port(asset_root, conditioned=ckpt == 'conditioned')
    R = ic.Reference(asset_root, conditioned=ckpt == 'conditioned', port_table=True)
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    for seq in (ic.ROUTE_SEQS[1], ic.ROUTE_SEQS[3], ic.LONG_SEQS[0]):
        inp = ic.seq_inputs(*seq)
        with torch.no_grad():
            d = net.inference({'in_body_pose': f64(inp['pose'][None]), 'frame_mask': f64(inp['vis'][None]), 'in_motion_latent': f64(inp['eps'])}, sample_num=1,
                              multi_step=True)
        assert d['infer_out_body_pose'].dtype == torch.float64
        assert np.abs(d['infer_out_body_pose'][0, 0].numpy() - R.infer(seq)['pose']).max() < 1e-13, seq
    seq = ic.ROUTE_SEQS[4]
    w = ic.window_inputs(seq)
    with torch.no_grad():
        data = net.init_batch_data({'in_body_pose': f64(w['in_body_pose'][None]), 'frame_mask': f64(w['frame_mask'][None]),
                                    'pose': torch.cat([torch.zeros(1, ic.WIN, 3, dtype=torch.float64), f64(w['body_pose'][None])], -1)})
        net.context_encoder(data)
        net.data_encoder(data)
        for mode in ('train', 'recon'):
            data['q_z_samp'] = data['q_z_dist'].sample(f64(w['eps'][None]))
            net.data_decoder(data, mode=mode)
            mine = R.window(seq, mode)
            got = {'pose': data[mode + '_out_body_pose_tp'][ic.PAST:, 0], 'context': data['context'][:, 0], 'q_z': torch.stack([data['q_z_dist'].mu[0], data['q_z_dist'].logvar[0]]),
                   'p_z': torch.stack([data['p_z_dist'].mu[0], data['p_z_dist'].logvar[0]])}
            e = ic.errors({k: v.numpy() for k, v in got.items()}, mine)
            assert set(e) == {'pose', 'context', 'q_z', 'p_z'} and max(e.values()) < 1e-13, (mode, e)
    d = (ic.pos_table(ic.WIN, 0, torch.float64, port=True) - ic.pos_table(ic.WIN, 0, torch.float64)).abs().max()
    assert 1e-7 < float(d) < 1e-5, d


def test_both_checkpoints_stay_inside_the_fp16_range_analysis(asset_root):
    """The infiller lines of the range analysis, restated: 3288 for the shipped checkpoint, 19727 under GAINS -- below 3e4, the handle keeps
    the fp16-split kernels (asserted again on the device, from glamr_nets_precision)."""
    for c, want in (('shipped', 3288), ('conditioned', 19727)):
        worst, wmax = ic.range_bound(ic.load_state_dict(asset_root, c == 'conditioned'))
        print('%s checkpoint: worst-case converted activation %.0f, largest weight %.3f' % (c, worst, wmax))
        assert abs(worst - want) < 1 and worst < ic.FP16_LIMIT and wmax < ic.FP16_LIMIT


@pytest.mark.parametrize('ckpt', ic.CHECKPOINTS)
def test_floors_are_reproduced_and_fp32_is_inside_every_tolerance(asset_root, r32, r64, ckpt):
    """Floor (a), fp32 port against fp64, and floor (b), two fp16 planes per product operand against fp64, measured again: each within
    [1/2, 2] x its table entry; every tolerance is 16 x floor (a) and at least 3 x floor (b) -- the split kernels' number format has room."""
    a = ic.floors(r32[ckpt], r64[ckpt], FLOOR_SEQS)
    b = ic.floors(ic.Reference(asset_root, conditioned=ckpt == 'conditioned', split=True), r64[ckpt], FLOOR_SEQS)
    for name, got, table in (('(a) fp32 port', a, ic.FLOOR_A[ckpt]), ('(b) fp16 hi + lo operands', b, ic.FLOOR_B[ckpt])):
        print('%s checkpoint, floor %s vs fp64: %s' % (ckpt, name, ', '.join('%s %.3e' % kv for kv in sorted(got.items()))))
        assert set(got) == set(table) == set(ic.KEYS)
        bad = {k: (got[k], table[k]) for k in got if not (np.isfinite(got[k]) and 0.5 * table[k] <= got[k] <= 2.0 * table[k])}
        assert not bad, 'floor %s left [1/2, 2] x its table entry: %s' % (name, bad)
    for k in ic.KEYS:
        assert ic.TOL[ckpt][k] == ic.FLOOR_FACTOR * ic.FLOOR_A[ckpt][k] and a[k] <= ic.TOL[ckpt][k] and 3 * ic.FLOOR_B[ckpt][k] <= ic.TOL[ckpt][k], k


def _touched(m, seq):
    return not (m == 'past' and ic.n_windows(seq[1]) < 2)


def _ratios(R, tol, m):
    """Per sweep sequence the mutation touches: (tolerances moved on the most-moved compared output, that output, the sequence).  Compared:
    the pose of the whole sequence (glamr_nets_infer, the taped forward) and context, p_z, z of window 0 (glamr_nets_infiller_window)."""
    out = []
    for i, seq in enumerate(ic.SWEEP):
        if not _touched(m, seq):
            continue
        e = ic.errors(ic.window0(R.infer(seq, m, ic.SWEEP[(i + 1) % len(ic.SWEEP)])), ic.window0(R.infer(seq)))
        k = max(e, key=lambda k: e[k] / tol[k])
        out.append((e[k] / tol[k], k, seq))
    return sorted(out)


@pytest.mark.parametrize('m', ic.MUTATIONS)
def test_every_mutation_moves_an_output_by_2_tolerances(r64, m):
    """On EVERY sequence of the sweep the mutation touches (all of them; 'past' needs a second window), on both checkpoints, at least one
    compared output moves by 2 x its tolerance or more: a kernel with that defect and otherwise within one tolerance fails.  The one
    exception is recorded, not hidden: SHIPPED_BLIND on the shipped checkpoint (asserted to be below the margin there, so that the list
    cannot go stale).  No sequence is left out of the sweep."""
    for ckpt in ic.CHECKPOINTS:
        r = _ratios(r64[ckpt], ic.TOL[ckpt], m)
        assert len(r) >= (22 if m == 'past' else len(ic.SWEEP))
        print('%s checkpoint, (%s) %s: least-moved sequences, in tolerances: %s' % (ckpt, m, ic.MUTATION_NAMES[m], ', '.join('%.1f x %s %s' % x for x in r[:3])))
        if ckpt == 'shipped' and m in SHIPPED_BLIND:
            assert r[0][0] < MARGIN, r[:3]
        else:
            assert r[0][0] >= MARGIN, r[:5]
