"""The host restatement of the random streams (tests/philox_reference.py) against the published known answers of
philox4x32-10 and against a scalar Python-int implementation: what the GPU tests of test_gpu_philox_exact.py compare the
kernels with must itself be right.  CPU only."""
import numpy as np
import pytest

import philox_reference as P

# Random123 known answers (kat_vectors, philox4x32 10): counter words c0..c3, key words k0 k1 -> output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
M32 = 0xFFFFFFFF


def _scalar_philox(seed, offset, index):
    """Plain Python integers, one counter at a time."""
    c = [index & M32, index >> 32, offset & M32, offset >> 32]
    k = [seed & M32, seed >> 32]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers_and_word_layout(ctr, key, want):
    """index = c0 | c1 << 32, offset = c2 | c3 << 32, seed = k0 | k1 << 32."""
    index, offset, seed = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
    got = P.philox4x32_10(seed, offset, index)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(v) for v in got] == list(want)
    assert _scalar_philox(seed, offset, index) == list(want)


def test_third_vector_is_the_documented_triple():
    got = P.philox4x32_10(0x299f31d0a4093822, 0x0370734413198a2e, 0x85a308d3243f6a88)
    assert [int(v) for v in got] == list(KAT[2][2])


def test_every_word_of_counter_and_key_matters():
    """Exchanging index / offset, or the halves of any of the three, gives other words (a restatement that mixed them up
    could still pass the two symmetric known answers)."""
    s, o, i = 0x299f31d0a4093822, 0x0370734413198a2e, 0x85a308d3243f6a88
    base = P.philox4x32_10(s, o, i).tolist()
    sw = lambda v: ((v & M32) << 32) | (v >> 32)
    for other in [(s, i, o), (sw(s), o, i), (s, sw(o), i), (s, o, sw(i)), (o, s, i)]:
        assert P.philox4x32_10(*other).tolist() != base


def test_vectorised_equals_scalar_on_random_triples():
    """1000 random (seed, offset, index): 64-bit values, indices above 2^32, offsets on both sides of 2^32 and at the carry."""
    rng = np.random.default_rng(20240607)
    seeds = [int(v) for v in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    offsets = [int(v) for v in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    indices = [int(v) for v in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    for j, v in enumerate([0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]):
        offsets[j] = v
        indices[100 + j] = v
        seeds[200 + j] = v
    offsets[300:400] = [int(v) for v in rng.integers(0, 1 << 32, 100)]                 # below 2^32
    indices[400:500] = [int(v) for v in rng.integers(1 << 32, 1 << 40, 100)]           # above 2^32
    assert sum(v < 1 << 32 for v in offsets) >= 100 and sum(v >= 1 << 32 for v in offsets) >= 100
    assert sum(v > 1 << 32 for v in indices) >= 100
    got = P.philox4x32_10(np.array(seeds, dtype=np.uint64), np.array(offsets, dtype=np.uint64),
                          np.array(indices, dtype=np.uint64))
    assert got.shape == (1000, 4)
    want = np.array([_scalar_philox(s, o, i) for s, o, i in zip(seeds, offsets, indices)], dtype=np.uint64)
    np.testing.assert_array_equal(got.astype(np.uint64), want)
    # scalars broadcast against an index array, python ints of any size are taken exactly
    s, o = seeds[0], offsets[5]
    got = P.philox4x32_10(s, o, np.array(indices[:50], dtype=np.uint64))
    np.testing.assert_array_equal(got.astype(np.uint64), np.array([_scalar_philox(s, o, i) for i in indices[:50]], dtype=np.uint64))
    with pytest.raises(ValueError):
        P.philox4x32_10(-1, 0, 0)
    with pytest.raises(ValueError):
        P.philox4x32_10(0, 1 << 64, 0)


def test_uniform_and_box_muller_inputs():
    n = 100_000
    w = P.words(11, 0, n)
    u = P.uniform(11, 0, n)
    assert u.dtype == np.float32 and u.shape == (n,)
    assert (u >= 0).all() and (u < 1).all()
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.round(k))                                   # multiples of 2^-24
    np.testing.assert_array_equal(k.astype(np.uint64), w[:, 0].astype(np.uint64) >> np.uint64(8))      # the TOP 24 bits of word 0
    u1 = P.u1_from_word(w[:, 0])
    assert (u1 > 0).all() and (u1 <= 1).all()
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1)     # exact in fp32 as on the device
    # the extremes of the word
    assert P.uniform_from_word(np.uint32(0xFFFFFFFF)) == np.float32(1 - 2.0 ** -24) and P.uniform_from_word(np.uint32(0xFF)) == 0
    assert P.u1_from_word(np.uint32(0xFFFFFFFF)) == 1.0 and P.u1_from_word(np.uint32(0)) == 2.0 ** -24
    z = P.normal(11, 0, n)
    assert z.dtype == np.float64 and np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2))
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    # radius from word 0, angle from word 1, by one fp32 product
    j = 12345
    arg = np.float32(6.2831855) * np.float32((int(w[j, 1]) >> 8) * 2.0 ** -24)
    assert z[j] == np.sqrt(-2 * np.log(((int(w[j, 0]) >> 8) + 1) * 2.0 ** -24)) * np.cos(np.float64(arg))
    assert not np.array_equal(P.normal_from_words(w[:, 1], w[:, 0]), z)


@pytest.mark.parametrize("rows", [[0, 0, 5, 12], [0, 5, 5, 12], [0, 5, 12, 12], [0, 0, 0, 7, 7], [0, 9], [0, 0]])
def test_instance_streams_are_concatenated_solo_streams(rows):
    seeds = [0x299f31d0a4093822, 11, (1 << 63) - 1, 1 << 40][:len(rows) - 1]
    off = (1 << 32) - 1
    u = P.instance_uniform(rows, seeds, off)
    z = P.instance_normal(rows, seeds, off)
    assert u.shape == z.shape == (rows[-1],) and u.dtype == np.float32 and z.dtype == np.float64
    for b, s in enumerate(seeds):
        n = rows[b + 1] - rows[b]
        np.testing.assert_array_equal(u[rows[b]:rows[b + 1]], P.uniform(s, off, n))
        np.testing.assert_array_equal(z[rows[b]:rows[b + 1]], P.normal(s, off, n))
    if rows[-1]:
        np.testing.assert_array_equal(u, np.concatenate([P.uniform(s, off, rows[b + 1] - rows[b]) for b, s in enumerate(seeds)]))
    with pytest.raises(ValueError):
        P.instance_uniform([0, 5, 3], [1, 2], 0)
    with pytest.raises(ValueError):
        P.instance_uniform([0, 5], [1, 2], 0)
