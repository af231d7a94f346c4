"""The priors' latent draws from per-sequence Philox streams (csrc/rng.hip): thin wrappers of the glamr_rng_* / glamr_latents_draw
entry points plus the host-side bookkeeping of the stream definition (sequence ids, the per-slot table).  Everything numeric happens in the
library's kernels; there is no host implementation here."""
import hashlib

import numpy as np
import torch

from .. import _lib
from .priors import NZ

SOURCES = ('torch', 'philox')
PRIOR_INFILLER, PRIOR_TRAJ = 0, 1
_MASK64 = (1 << 64) - 1


def check_source(value):
    if value not in SOURCES:
        raise ValueError('latent_source must be one of %s, got %r' % (SOURCES, value))
    return value


def seq_id_of(seq_name):
    """The default 64-bit sequence id: the first 8 bytes (little endian) of blake2b(seq_name, digest_size=8)."""
    return int.from_bytes(hashlib.blake2b(str(seq_name).encode(), digest_size=8).digest(), 'little')


def seq_id_for(in_dict):
    """An explicit `seq_id` entry of the input dictionary wins over the hash of its `seq_name`."""
    sid = in_dict.get('seq_id') if hasattr(in_dict, 'get') else None
    return int(sid) & _MASK64 if sid is not None else seq_id_of(in_dict['seq_name'])


def person_id_of(key):
    """The integer key of `person_data` (not the slot position: dropping a person does not move the others)."""
    try:
        pid = int(key)
    except (TypeError, ValueError):
        raise ValueError("latent_source 'philox' needs integer person keys, got %r" % (key,)) from None
    if pid != key or not 0 <= pid < 2 ** 30:
        raise ValueError("latent_source 'philox' needs person keys in [0, 2^30), got %r" % (key,))
    return pid


def slot_table(seq_ids, person_ids, device):
    """(seq_ids uint64 as int64 bits, person_ids int32) on `device`; person id < 0 = padding slot."""
    s = np.asarray([int(x) & _MASK64 for x in seq_ids], dtype=np.uint64).view(np.int64)
    p = np.asarray(person_ids, dtype=np.int32)
    assert s.shape == p.shape
    return torch.from_numpy(s).to(device, non_blocking=True), torch.from_numpy(p).to(device, non_blocking=True)


def new_seed_word(device):
    """The 8 bytes of device memory the draw kernel reads its seed from."""
    return torch.zeros(1, dtype=torch.int64, device=device)


def set_seed(seed_dev, seed):
    """glamr_rng_set_seed on the current stream."""
    _lib.check(_lib.lib().glamr_rng_set_seed(_lib.ptr(seed_dev), int(seed) & _MASK64, _lib.current_stream()))


def draw_into(seed_dev, seq_ids_dev, person_ids_dev, n_windows, meps, teps):
    """glamr_latents_draw on the current stream: meps (n_slots, n_windows, 128), teps (n_slots, 128), fp32, contiguous."""
    n_slots = int(person_ids_dev.shape[0])
    assert meps.dtype == torch.float32 and teps.dtype == torch.float32
    assert tuple(meps.shape) == (n_slots, n_windows, NZ) and tuple(teps.shape) == (n_slots, NZ), (meps.shape, teps.shape, n_slots, n_windows)
    _lib.check(_lib.lib().glamr_latents_draw(_lib.ptr(seed_dev), _lib.ptr(seq_ids_dev), _lib.ptr(person_ids_dev), n_slots, int(n_windows), _lib.ptr(meps), _lib.ptr(teps),
                                             _lib.current_stream()))


def draw(seed, seq_ids, person_ids, n_windows, device):
    """Fresh (meps, teps) for host lists of sequence / person ids under `seed` (table upload + seed + ONE draw launch)."""
    device = torch.device(device)
    with torch.cuda.device(device):
        s, p = slot_table(seq_ids, person_ids, device)
        word = new_seed_word(device)
        set_seed(word, seed)
        meps = torch.empty((len(person_ids), int(n_windows), NZ), dtype=torch.float32, device=device)
        teps = torch.empty((len(person_ids), NZ), dtype=torch.float32, device=device)
        draw_into(word, s, p, n_windows, meps, teps)
    return meps, teps


def batch_ids(batch, B):
    """(sequence id, first person id) of every row of a stand-alone priors batch.  Sequence: the row's entry of `batch['seq_id']` (explicit
    ids, one per row), else the hash of its entry of `batch['seq_name']` (one name per row; a plain string for a batch of one), else the row
    index.  Person: sample k of row r draws as person `batch['person_id'][r] + k` (default 0 + k) -- MotionTrajJointModel.pred_trajectory
    flattens (row, sample) into rows of one sample each and says so with these two entries, so that the predictor draws the streams the
    one-call path gives the same (row, sample)."""
    get = batch.get if hasattr(batch, 'get') else (lambda k: None)
    ids, names, persons = get('seq_id'), get('seq_name'), get('person_id')
    if ids is not None:
        ids = [int(x) & _MASK64 for x in (ids.tolist() if hasattr(ids, 'tolist') else ids)] if not isinstance(ids, int) else [ids & _MASK64]
    elif names is not None:
        ids = [seq_id_of(n) for n in ([names] if isinstance(names, str) else names)]
    else:
        ids = list(range(B))
    persons = [0] * B if persons is None else [person_id_of(x) for x in (persons.tolist() if hasattr(persons, 'tolist') else persons)]
    if len(ids) != B or len(persons) != B:
        raise ValueError('the batch has %d rows, %d sequence ids / names and %d person ids' % (B, len(ids), len(persons)))
    return ids, persons


def draw_samples(seed, batch, B, sample_num, n_windows, device):
    """The stand-alone priors' draws (`.inference` of prior_models), ONE launch: sample k of a row plays the person id (batch_ids).  Returns meps
    (B, S, n_windows, 128), teps (B, S, 128)."""
    sids, base = batch_ids(batch, B)
    meps, teps = draw(seed, [s for s in sids for _ in range(sample_num)], [p + k for p in base for k in range(sample_num)], n_windows, device)
    return meps.view(B, sample_num, int(n_windows), NZ), teps.view(B, sample_num, NZ)


def traj_chunk_samples(seed, batch, B, sample_num, chunk, device):
    """The trajectory predictor's draws of chunk `chunk` of its chunked inference, (B, S, 128): elements [128 chunk, 128 (chunk + 1)) of the
    (row, sample)'s trajectory stream.  Chunk 0 -- every call but the later chunks of a sequence longer than one chunk -- is draw_samples' one
    launch; a later chunk takes one glamr_rng_normal per (row, sample): the batch draw has no element offset."""
    if chunk == 0:
        return draw_samples(seed, batch, B, sample_num, 0, device)[1]
    sids, base = batch_ids(batch, B)
    e = torch.empty((B, sample_num, NZ), dtype=torch.float32, device=device)
    for r in range(B * sample_num):
        b, k = divmod(r, sample_num)
        normal(seed, sids[b], 2 * (base[b] + k) + PRIOR_TRAJ, chunk * NZ, NZ, device, out=e[b, k])
    return e


def normal(seed, seq_id, sub, first_elem, n, device, out=None):
    """glamr_rng_normal: elements [first_elem, first_elem + n) of one stream."""
    if out is None:
        out = torch.empty(int(n), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().glamr_rng_normal(int(seed) & _MASK64, int(seq_id) & _MASK64, int(sub), int(first_elem), int(n), _lib.ptr(out), _lib.current_stream()))
    return out


def bits(seed, seq_id, sub, first_block, n_blocks, device):
    """glamr_rng_bits: the raw Philox words of blocks [first_block, first_block + n_blocks), (n_blocks, 4) int32 bit patterns."""
    out = torch.empty((int(n_blocks), 4), dtype=torch.int32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().glamr_rng_bits(int(seed) & _MASK64, int(seq_id) & _MASK64, int(sub), int(first_block), int(n_blocks), _lib.ptr(out), _lib.current_stream()))
    return out
