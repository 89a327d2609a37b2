"""Philox4x32-10 in plain numpy, written from the algorithm's definition (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11), and the project's use of it as include/r4r.h words it.  The role of
tests/conv_ref.py: an independent reference the device's dropout streams are held to, itself held to the published
known-answer vectors by tests/test_philox_ref.py.

One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to

    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

with hi / lo the halves of the 64-bit product; the key is bumped by (W0, W1) between rounds; ten rounds.

The project's mapping (include/r4r.h): a 64-bit stream position `ctr` is the counter (ctr & 0xffffffff, ctr >> 32, 0, 0),
a 64-bit seed the key (seed & 0xffffffff, seed >> 32); a word w becomes u = float32(w >> 8) * 2^-24 in [0, 1) and the
draw is KEPT when u >= float32(p).  The fused native steps take the first word of counter `offset + b * ND + k`; the
stand-alone op r4r_dropout_fwd gives element i word i % 4 of counter `offset + i // 4`."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def philox4x32_10(c, k):
    """c: counters [n, 4] (or [4]), k: key [2] or keys [n, 2], all 32-bit words -> uint32 [n, 4]."""
    c = np.atleast_2d(np.asarray(c, dtype=np.uint64)) & np.uint64(MASK32)
    k = np.atleast_2d(np.asarray(k, dtype=np.uint64)) & np.uint64(MASK32)
    c0, c1, c2, c3 = (c[:, j].copy() for j in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    lo, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(ROUNDS):
        p0 = np.uint64(M0) * c0                              # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + np.uint64(W0)) & lo, (k1 + np.uint64(W1)) & lo
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def philox4x32_10_scalar(c, k):
    """The same function on one counter with Python integers (no numpy): the vectorised form's cross-check."""
    c0, c1, c2, c3 = (int(x) & MASK32 for x in c)
    k0, k1 = (int(x) & MASK32 for x in k)
    for _ in range(ROUNDS):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return (c0, c1, c2, c3)


def counter_words(ctr):
    """64-bit stream position -> (ctr & 0xffffffff, ctr >> 32, 0, 0)."""
    ctr = int(ctr) & MASK64
    return (ctr & MASK32, ctr >> 32, 0, 0)


def key_words(seed):
    """64-bit seed -> (seed & 0xffffffff, seed >> 32)."""
    seed = int(seed) & MASK64
    return (seed & MASK32, seed >> 32)


def words(seed, first_counter, count):
    """The four words of the `count` consecutive stream positions from `first_counter` (mod 2^64) -> uint32 [count, 4]."""
    first = int(first_counter) & MASK64
    if first + int(count) <= MASK64:
        ctr = np.uint64(first) + np.arange(int(count), dtype=np.uint64)
    else:                                                    # a range that wraps 2^64: position by position
        ctr = np.array([(first + j) & MASK64 for j in range(int(count))], dtype=np.uint64)
    c = np.zeros((int(count), 4), dtype=np.uint64)
    c[:, 0] = ctr & np.uint64(MASK32)
    c[:, 1] = ctr >> np.uint64(32)
    return philox4x32_10(c, key_words(seed))


def uniform(w):
    """u = float32(w >> 8) * 2^-24: exact in float32 (24 bits), in [0, 1)."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep(w, p):
    return uniform(w) >= np.float32(p)


def engine_keep(seed, first_counter, count, p):
    """bool [count]: draw j is the first word of counter first_counter + j (the fused native steps)."""
    return keep(words(seed, first_counter, count)[:, 0], p)


def op_keep(seed, offset, n, p):
    """bool [n]: element i takes word i % 4 of counter offset + i // 4 (r4r_dropout_fwd)."""
    groups = (int(n) + 3) // 4
    return keep(words(seed, offset, groups).reshape(-1)[:int(n)], p)


def scale(p):
    """The multiplier of a kept draw, float32(1) / (float32(1) - float32(p))."""
    return np.float32(1) / (np.float32(1) - np.float32(p))
