"""The rule of include/r4r.h, "What-if documents", as a plain Python loop: what r4r_tower_build_variants and
data._np_docs_masked are tested against, and the synthetic pool the tests share."""
import numpy as np

SLOTS = 64


def variant_doc(tok, rev_off, first, owner, drop, occ, T):
    """One row: the document of ``owner`` without the reviews whose bit is set in ``drop`` (a Python int, any sign),
    with word 0 at the positions of ``occ`` inside [0, T)."""
    doc = [0] * T
    if 0 <= owner < len(first) - 1:
        rb, re = int(first[owner]), int(first[owner + 1])
        words = []
        for s in range(re - rb):
            if s < SLOTS and (int(drop) >> s) & 1:
                continue
            words.extend(int(t) for t in tok[int(rev_off[rb + s]):int(rev_off[rb + s + 1])])
        for p, w in enumerate(words[:T]):
            doc[p] = w
    for p in occ:
        if 0 <= int(p) < T:
            doc[int(p)] = 0
    return doc


def variant_docs(tok, rev_off, first, ids, drop, occ, T):
    """[n, T] int64.  ``drop``: n ints or None; ``occ``: n lists of positions or None."""
    n = len(ids)
    return np.array([variant_doc(tok, rev_off, first, int(ids[r]), 0 if drop is None else int(drop[r]),
                                 () if occ is None else occ[r], T) for r in range(n)], dtype=np.int64).reshape(n, T)


def remaining_doc(tok, rev_off, first, owner, removed, T):
    """The same document restated: the list of the REMAINING reviews, joined, cut and padded."""
    rb, re = int(first[owner]), int(first[owner + 1])
    left = [s for s in range(re - rb) if s not in set(removed)]
    words = [int(t) for s in left for t in tok[int(rev_off[rb + s]):int(rev_off[rb + s + 1])]]
    return (words + [0] * T)[:T]


COUNTS = (0, 1, 2, 63, 64, 65, 70)                          # the reviews of the synthetic pool's owners


def synthetic_pool(seed=7):
    """(tok int32, rev_off, first, counts): owners with 0, 1, 2, 63, 64, 65 and 70 reviews of 0 .. 6 words (empty
    reviews included; the first review of the 2-review owner is empty), word ids from 1 up: 0 is the padding alone."""
    rng = np.random.RandomState(seed)
    lens = []
    for c in COUNTS:
        l = rng.randint(0, 7, size=c)
        if c == 2:
            l[0] = 0
        if c >= 63:
            l[5] = 0
        lens.append(l)
    lens = np.concatenate(lens).astype(np.int64)
    first = np.zeros(len(COUNTS) + 1, np.int64)
    np.cumsum(COUNTS, out=first[1:])
    rev_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=rev_off[1:])
    tok = rng.randint(1, 1000, size=int(rev_off[-1])).astype(np.int32)
    return tok, rev_off, first, np.array(COUNTS, np.int64)


def as_signed(mask):
    """A 64-bit mask as the int64 a tensor holds."""
    mask &= (1 << 64) - 1
    return mask - (1 << 64) if mask >= (1 << 63) else mask
