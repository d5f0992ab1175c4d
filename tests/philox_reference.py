"""Host restatement of the device random streams ("The random stream as a contract"), numpy only.

Philox4x32-10 is written here from its definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11, section 3.3 and the Random123 constants), not from csrc/common.h: one round maps the counter (c0, c1, c2, c3) under the
key (k0, k1) to

    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

with the 64-bit products M0 c0 and M1 c2, and the key is bumped by (W0, W1) modulo 2^32 between rounds; ten rounds.

How the project lays its values on the words (the contract the GPU tests hold the kernels to):

    counter = (index lo, index hi, offset lo, offset hi)      key = (seed lo, seed hi)
    u  = (w0 >> 8) * 2^-24                                     uniform in [0, 1), a multiple of 2^-24; a Bernoulli bit is u < p
    z  = sqrt(-2 ln u1) * cos(2 pi u2),  u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (w1 >> 8) * 2^-24

Every integer step runs on numpy uint64 arrays with uint64 constants, so no operand is promoted to float64 or int64, and every
product of two 32-bit values fits the 64 bits it is computed in; the only wrap, the key bump, is masked explicitly."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # key increments (golden ratio, sqrt(3) - 1)
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)
_8 = np.uint64(8)
TWO_M24 = 2.0 ** -24


def _u64(x):
    """x (python ints below 2^64, or an integer array) as a uint64 array; negative values and 2^64 or more are refused."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return x
    a = np.asarray(x, dtype=object)
    flat = [int(v) for v in a.reshape(-1)]
    if any(v < 0 or v >= 1 << 64 for v in flat):
        raise ValueError("seed, offset and index are unsigned 64-bit values")
    return np.array(flat, dtype=np.uint64).reshape(a.shape)


def philox4x32_10(seed, offset, index):
    """uint32 [..., 4]: the four output words of Philox4x32-10 for counter (index lo, index hi, offset lo, offset hi) and key
    (seed lo, seed hi).  ``seed``, ``offset`` and ``index`` broadcast against each other (usually two scalars and an index
    array)."""
    seed, offset, index = np.broadcast_arrays(_u64(seed), _u64(offset), _u64(index))
    c0, c1 = index & _LO, index >> _32
    c2, c3 = offset & _LO, offset >> _32
    k0, k1 = seed & _LO, seed >> _32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + W0) & _LO, (k1 + W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, offset, n):
    """uint32 [n, 4]: the words of elements 0 .. n-1 of stream (seed, offset)."""
    return philox4x32_10(seed, offset, np.arange(int(n), dtype=np.uint64))


def uniform_from_word(w0):
    """float32: (w0 >> 8) * 2^-24, exact (24 bits fit the fp32 significand)."""
    return ((np.asarray(w0, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * TWO_M24).astype(np.float32)


def u1_from_word(w0):
    """float64: ((w0 >> 8) + 1) * 2^-24 in (0, 1], the argument of the Box-Muller logarithm (exact in fp32 as well)."""
    return ((np.asarray(w0, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * TWO_M24


def normal_from_words(w0, w1):
    """float64 Box-Muller on the device's inputs: ``w0`` makes the radius, ``w1`` the angle.  The angle is the device's single
    fp32 product float32(2 pi) * u2, done in numpy float32; logarithm, square root and cosine are float64."""
    arg = (np.float32(6.2831855) * uniform_from_word(w1)).astype(np.float32)
    return np.sqrt(-2.0 * np.log(u1_from_word(w0))) * np.cos(arg.astype(np.float64))


def uniform(seed, offset, n):
    """float32 [n]: what rows 0 .. n-1 of a call keyed (seed, offset) draw for their Bernoulli bits."""
    return uniform_from_word(words(seed, offset, n)[:, 0])


def normal(seed, offset, n):
    """float64 [n]: what rows 0 .. n-1 of a call keyed (seed, offset) draw for the DDPM noise, to float64 accuracy."""
    w = words(seed, offset, n)
    return normal_from_words(w[:, 0], w[:, 1])


def _instance_words(instance_rows, instance_seeds, offset):
    rows = [int(v) for v in np.asarray(instance_rows).reshape(-1)]
    seeds = [int(v) for v in np.asarray(instance_seeds, dtype=object).reshape(-1)]
    if len(rows) != len(seeds) + 1 or rows[0] != 0 or any(b < a for a, b in zip(rows, rows[1:])):
        raise ValueError("instance_rows must be [B + 1] non-decreasing offsets starting at 0, instance_seeds [B]")
    parts = [words(s, offset, rows[b + 1] - rows[b]) for b, s in enumerate(seeds)]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), np.uint32)


def instance_uniform(instance_rows, instance_seeds, offset):
    """float32 [instance_rows[-1]]: row r of instance b takes element r - instance_rows[b] of key instance_seeds[b]; an empty
    instance contributes nothing."""
    return uniform_from_word(_instance_words(instance_rows, instance_seeds, offset)[:, 0])


def instance_normal(instance_rows, instance_seeds, offset):
    """float64 [instance_rows[-1]]: the per-instance streams of ``normal``."""
    w = _instance_words(instance_rows, instance_seeds, offset)
    return normal_from_words(w[:, 0], w[:, 1])
