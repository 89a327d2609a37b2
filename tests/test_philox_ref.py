"""tests/philox_ref.py is the reference tests/test_gpu_dropout_stream.py holds every dropout stream to; this file holds
the reference itself to the published known-answer vectors of Philox4x32-10 (the Random123 distribution's kat_vectors),
to the 64-bit counter / key split include/r4r.h words, and to the keep rate a fair generator must show."""
import math

import numpy as np
import pytest

import philox_ref as P

# (counter words, key words) -> output words
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('c,k,want', KNOWN_ANSWERS)
def test_known_answer_vectors(c, k, want):
    assert P.philox4x32_10_scalar(c, k) == want
    got = P.philox4x32_10(np.array([c], dtype=np.uint64), np.array(k, dtype=np.uint64))
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert tuple(int(x) for x in got[0]) == want


def test_known_answer_vectors_as_one_batch():
    """Per-row keys, and rows that do not leak into each other."""
    c = np.array([v[0] for v in KNOWN_ANSWERS], dtype=np.uint64)
    k = np.array([v[1] for v in KNOWN_ANSWERS], dtype=np.uint64)
    assert np.array_equal(P.philox4x32_10(c, k), np.array([v[2] for v in KNOWN_ANSWERS], dtype=np.uint32))


def test_sixty_four_bit_split():
    assert P.counter_words(2 ** 32 - 1) == (0xffffffff, 0, 0, 0)
    assert P.counter_words(2 ** 32) == (0, 1, 0, 0)
    assert P.counter_words((0x12345 << 32) | 0x89abcdef) == (0x89abcdef, 0x12345, 0, 0)
    assert P.key_words(0xFEDCBA9800000001) == (0x00000001, 0xFEDCBA98)
    # the all-zero vector IS the project's (seed 0, position 0)
    assert tuple(int(x) for x in P.words(0, 0, 1)[0]) == KNOWN_ANSWERS[0][2]
    # a range across 2^32: c1 takes the carry, and the batch form equals the scalar form position by position
    seed, first, count = 0xFEDCBA9800000001, 2 ** 32 - 3, 7
    got = P.words(seed, first, count)
    for j in range(count):
        want = P.philox4x32_10_scalar(P.counter_words(first + j), P.key_words(seed))
        assert tuple(int(x) for x in got[j]) == want, j
    # ... a dropped high word would repeat these: positions 2^32 apart, and seeds that differ in the high word only
    assert not np.array_equal(P.words(seed, 5, 4), P.words(seed, 5 + 2 ** 32, 4))
    assert not np.array_equal(P.words(seed, 5, 4), P.words(seed & 0xffffffff, 5, 4))
    # ... and a range that wraps 2^64 goes on at position 0
    wrap = P.words(seed, 2 ** 64 - 2, 4)
    assert np.array_equal(wrap[:2], P.words(seed, 2 ** 64 - 2, 2)) and np.array_equal(wrap[2:], P.words(seed, 0, 2))


def test_uniform_and_keep_rule():
    w = np.array([0, 0xff, 0x100, 0x80000000, 0xffffffff], dtype=np.uint32)
    u = P.uniform(w)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]
    assert P.keep(w, 0.5).tolist() == [False, False, False, True, True]      # kept when u >= p: 0.5 itself is kept
    assert P.keep(w, 0.0).all()
    assert float(P.scale(0.5)) == 2.0 and P.scale(0.2).dtype == np.float32


def test_engine_and_op_streams_index_the_same_words():
    seed, at = 0x9E3779B97F4A7C15, 2 ** 32 - 2
    w = P.words(seed, at, 5)
    assert np.array_equal(P.engine_keep(seed, at, 5, 0.5), P.keep(w[:, 0], 0.5))
    for n in (1, 3, 4, 5, 18):
        got = P.op_keep(seed, at, n, 0.2)
        assert got.shape == (n,) and got.dtype == np.bool_
        assert np.array_equal(got, P.keep(w.reshape(-1)[:n], 0.2)), n
        # element i: word i % 4 of counter at + i // 4
        for i in range(n):
            assert got[i] == P.keep(P.words(seed, at + i // 4, 1)[0, i % 4], 0.2)


@pytest.mark.parametrize('p', [0.2, 0.5])
def test_keep_rate(p):
    """10^5 draws: the count of kept ones is Binomial(n, 1 - p'), p' = the float32 threshold rounded up to the 2^-24
    grid of u (|p' - p| < 2^-23: 0.01 of a draw at this n); within five standard deviations, for each stream form."""
    n = 100000
    sd = math.sqrt(n * p * (1.0 - p))
    for kept in (P.engine_keep(0x5EED5EED, 12345, n, p), P.op_keep(0x5EED5EED, 12345, n, p)):
        assert kept.shape == (n,)
        assert abs(int(kept.sum()) - n * (1.0 - p)) <= 5.0 * sd
