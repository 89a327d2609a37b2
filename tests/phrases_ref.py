"""The host statement of include/r4r.h's "Phrase explanations" that the phrase tests hold the kernel to: sequential
loops in ascending f over numpy arrays, nothing vectorised away, nothing taken from the code under test."""
from fractions import Fraction

import numpy as np


def round_f32(x):
    """A Fraction rounded ONCE to the nearest float32, ties to even (overflow is not handled: the tests stay finite)."""
    if x == 0:
        return np.float32(0.0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) <= a < 2^(e+1)
    if a >= Fraction(2) ** e:
        e += 1                                                       # 2^(e-1) <= a < 2^e
    ulp = max(e - 24, -149)                                          # (subnormals keep the smallest exponent)
    q = round(a / Fraction(2) ** ulp)                                # Python rounds a Fraction half to even
    return np.float32(sign * float(Fraction(q) * Fraction(2) ** ulp))    # q 2^ulp has at most 24 bits: exact


def fma32(a, b, c):
    """fmaf(a, b, c): the exact a b + c, rounded once."""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def phrases_ref(pooled, argmax, wt, T, K):
    """-> (positions int32 [N, K], scores float32 [N, K], filters int32 [N, K], windows int32 [N]).

    Filter f of row n is live iff 0 <= argmax[n, f] < T + 2.  A window's score runs over its live filters in ascending
    f from 0.0f: ``wt`` None: acc = acc + pooled (np.float32 adds); else acc = fmaf(wt, pooled, acc), wt [F] or [N, F].
    The list: score descending, ties by ascending position; the fill is (-1, 0.0, 0)."""
    pooled = np.asarray(pooled, dtype=np.float32)
    argmax = np.asarray(argmax)
    N, F = pooled.shape
    if wt is not None:
        wt = np.asarray(wt, dtype=np.float32)
        wt = np.broadcast_to(wt, (N, F))
    pos = np.full((N, K), -1, np.int32)
    score = np.zeros((N, K), np.float32)
    filters = np.zeros((N, K), np.int32)
    windows = np.zeros(N, np.int32)
    for n in range(N):
        acc, cnt = {}, {}
        for f in range(F):
            p = int(argmax[n, f])
            if not 0 <= p < T + 2:
                continue
            a = acc.get(p, np.float32(0.0))
            acc[p] = np.float32(a + pooled[n, f]) if wt is None else fma32(wt[n, f], pooled[n, f], a)
            cnt[p] = cnt.get(p, 0) + 1
        order = sorted(acc, key=lambda p: (-float(acc[p]), p))
        windows[n] = len(order)
        for k, p in enumerate(order[:K]):
            pos[n, k], score[n, k], filters[n, k] = p, acc[p], cnt[p]
    return pos, score, filters, windows


def tokens_ref(pos, idx, T):
    """top_tok of the listed positions ``pos`` [N, K] over the documents ``idx`` [N, T]: idx[n, p - 2 + j] inside the
    document, -1 in the conv's zero padding and for a fill entry."""
    pos, idx = np.asarray(pos), np.asarray(idx)
    N, K = pos.shape
    tok = np.full((N, K, 3), -1, np.int64)
    for n in range(N):
        for k in range(K):
            if pos[n, k] < 0:
                continue
            for j in range(3):
                t = int(pos[n, k]) - 2 + j
                if 0 <= t < T:
                    tok[n, k, j] = idx[n, t]
    return tok


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
