"""TEST INFRASTRUCTURE: a NumPy restatement of the latent-stream definition -- Philox4x32-10 in uint64 arithmetic, the
(block, sub, seq_id) counter layout, Box-Muller in float64 from the same integers.  The reference the library's kernels (csrc/rng.hip) and the
host build of csrc/rng_algo.hpp are checked against; the product never imports it (it is no CPU fallback)."""
import hashlib

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
NZ = 128

# Random123 known-answer vectors of philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of 32-bit values held in uint64 -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK32 for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = np.uint64(M0) * c0                   # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def stream_blocks(seed, seq_id, sub, block):
    """Words of the blocks `block` (array) of sub-stream `sub` of sequence `seq_id` under `seed`: (..., 4) uint32.  All arguments broadcast."""
    seed, seq_id = np.asarray(seed, dtype=np.uint64), np.asarray(seq_id, dtype=np.uint64)
    w = philox4x32_10(np.asarray(block, dtype=np.uint64), np.asarray(sub, dtype=np.uint64), seq_id & MASK32, seq_id >> np.uint64(32), seed & MASK32, seed >> np.uint64(32))
    return np.stack(w, axis=-1)


def bits(seed, seq_id, sub, first_block, n_blocks):
    return stream_blocks(np.uint64(seed), np.uint64(seq_id), sub, np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64))


def box_muller(words):
    """(..., 4) uint32 -> (..., 4) float64: pairs (0,1), (2,3); u = (x + 0.5) 2^-32, theta = 2 pi (y + 0.5) 2^-32."""
    w = np.asarray(words).astype(np.float64)
    out = np.empty(w.shape, np.float64)
    for a in (0, 2):
        u = (w[..., a] + 0.5) * 2.0 ** -32
        th = 2.0 * np.pi * ((w[..., a + 1] + 0.5) * 2.0 ** -32)
        r = np.sqrt(-2.0 * np.log(u))
        out[..., a], out[..., a + 1] = r * np.cos(th), r * np.sin(th)
    return out


def normals(seed, seq_id, sub, first_elem, n):
    """Elements [first_elem, first_elem + n) of one stream, float64."""
    b0, b1 = first_elem // 4, (first_elem + n + 3) // 4
    x = box_muller(bits(seed, seq_id, sub, b0, b1 - b0)).reshape(-1)
    return x[first_elem - 4 * b0:first_elem - 4 * b0 + n]


def latents(seed, seq_id, person_id, n_windows):
    """(meps (n_windows, 128), teps (128)) of one person, float64."""
    return normals(seed, seq_id, 2 * person_id, 0, n_windows * NZ).reshape(n_windows, NZ), normals(seed, seq_id, 2 * person_id + 1, 0, NZ)


def seq_id_of(name):
    return int.from_bytes(hashlib.blake2b(name.encode(), digest_size=8).digest(), 'little')


def _ndtr(x):
    try:
        from scipy.special import ndtr
        return ndtr(x)
    except ImportError:
        import torch
        return torch.special.ndtr(torch.from_numpy(x)).numpy()


STAT_SEEDS = (0, 1, 7, 12345, 2 ** 40 + 3)
STAT_SEQ_IDS = (0, 1, 1023, 2 ** 33)
STAT_N = 2 ** 20
STAT_CAPS = (4.0, 4.0, 4.0, 1.95)          # |mean| sqrt(n), |var - 1| / sqrt(2/n), |kurtosis - 3| / sqrt(96/n), sqrt(n) D_KS (0.1 % point of Kolmogorov's distribution)


def normal_stats(x):
    """The four standardised statistics of a sample that should be N(0, 1) (float64 arithmetic whatever the input type)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    mean = x.mean()
    d = x - mean
    var = (d ** 2).mean()
    kurt = (d ** 4).mean() / var ** 2
    cdf = _ndtr(np.sort(x))
    i = np.arange(1, n + 1, dtype=np.float64)
    dks = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    return abs(mean) * np.sqrt(n), abs(var - 1.0) / np.sqrt(2.0 / n), abs(kurt - 3.0) / np.sqrt(96.0 / n), np.sqrt(n) * dks
