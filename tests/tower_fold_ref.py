"""The rules of include/r4r.h, "Document fold", as plain numpy fp32 loops: every window of a variant document (the
brute force), the review-segment fold that r4r_fold_segments / r4r_fold_compose implement, and the greedy search of
r4r_fold_search_*.  ``P`` is the projected table [V, 3, F] fp32, ``b`` the conv bias [F] fp32; token -1 is a tap outside
the document."""
import numpy as np

from tower_variants_ref import SLOTS, variant_doc

f32 = np.float32
OUTSIDE = -1


def win(P, b, a, c, d):
    """((r0 + r1) + r2) + b for the window over tokens (a, c, d); a tap outside adds an exact zero row."""
    z = np.zeros_like(b)
    r0 = P[a, 0] if a >= 0 else z
    r1 = P[c, 1] if c >= 0 else z
    r2 = P[d, 2] if d >= 0 else z
    return ((r0 + r1) + r2) + b


def relu(best):
    return np.where(best > 0, best, f32(0)).astype(f32)


def brute(P, b, doc):
    """pooled [F]: the maximum over all len(doc) + 2 windows, then best > 0 ? best : +0."""
    T = len(doc)
    best = np.full_like(b, -np.inf)
    for p in range(T + 2):
        t = [int(doc[q]) if 0 <= q < T else OUTSIDE for q in (p - 2, p - 1, p)]
        best = np.maximum(best, win(P, b, *t))
    return relu(best)


def seg(P, b, r):
    """The maximum over the windows that lie inside the review ``r``; -inf below three words."""
    best = np.full_like(b, -np.inf)
    for q in range(2, len(r)):
        best = np.maximum(best, win(P, b, int(r[q - 2]), int(r[q - 1]), int(r[q])))
    return best


def fold(P, b, runs, segs, T):
    """pooled [F] by the fold.  ``runs``: the kept reviews in order (the tail as one last run); ``segs``: each run's
    cached maximum, or None where it has none -> (pooled, the windows evaluated)."""
    best = np.full_like(b, -np.inf)
    pos, p2, p1, n = 0, OUTSIDE, OUTSIDE, 0
    for r, s in zip(runs, segs):
        if pos >= T:
            break
        if len(r) == 0:
            continue
        v = min(len(r), T - pos)
        for q in range(min(2, v)):
            cur = int(r[q])
            best = np.maximum(best, win(P, b, p2, p1, cur))
            n += 1
            p2, p1 = p1, cur
        if v == len(r) and s is not None:
            best = np.maximum(best, s)
        else:
            for q in range(2, v):
                best = np.maximum(best, win(P, b, int(r[q - 2]), int(r[q - 1]), int(r[q])))
                n += 1
        if v >= 2:
            p2, p1 = int(r[v - 2]), int(r[v - 1])
        pos += v
    for q in range(min(T - pos, 3)):                            # the padding's word 0
        best = np.maximum(best, win(P, b, p2, p1, 0))
        n += 1
        p2, p1 = p1, 0
    for q in range(2):                                          # the two windows that hang over the end
        best = np.maximum(best, win(P, b, p2, p1, OUTSIDE))
        n += 1
        p2, p1 = p1, OUTSIDE
    return relu(best), n


# ---------------------------------------------------------------- over a review pool
def reviews_of(tok, rev_off, first, owner):
    """The owner's reviews as token lists; an owner outside the pool has none."""
    if not 0 <= owner < len(first) - 1:
        return []
    rb, re = int(first[owner]), int(first[owner + 1])
    return [[int(t) for t in tok[int(rev_off[rb + s]):int(rev_off[rb + s + 1])]] for s in range(re - rb)]


def pool_runs(tok, rev_off, first, owner, drop, S=SLOTS, slots=SLOTS):
    """(runs, cached): the kept reviews of the first ``slots`` in order, then the rest as one run; ``cached[j]`` is the
    kept review's slot where it is below ``S`` (it has a cached maximum), else None."""
    revs = reviews_of(tok, rev_off, first, owner)
    runs, cached = [], []
    for s, r in enumerate(revs[:slots]):
        if (int(drop) >> s) & 1:
            continue
        runs.append(r)
        cached.append(s if s < S else None)
    runs.append([t for r in revs[slots:] for t in r])
    cached.append(None)
    return runs, cached


def seg_table(P, b, tok, rev_off, first, ids, S):
    """r4r_fold_segments' output [n, S, F]."""
    out = np.full((len(ids), S, len(b)), -np.inf, f32)
    for i, owner in enumerate(ids):
        for s, r in enumerate(reviews_of(tok, rev_off, first, int(owner))[:S]):
            out[i, s] = seg(P, b, r)
    return out


def fold_pool(P, b, tok, rev_off, first, owner, drop, T, S=SLOTS, segs=None):
    """One row of r4r_fold_compose by the fold; ``segs`` [S, F]: the owner's row of ``seg_table`` (made when None)."""
    if segs is None:
        segs = seg_table(P, b, tok, rev_off, first, [owner], S)[0]
    runs, cached = pool_runs(tok, rev_off, first, owner, drop, S)
    return fold(P, b, runs, [None if s is None else segs[s] for s in cached], T)[0]


def brute_pool(P, b, tok, rev_off, first, owner, drop, T):
    """The same row over every window of ``tower_variants_ref.variant_doc``'s document."""
    return brute(P, b, variant_doc(tok, rev_off, first, owner, drop, (), T))


def ptab3(ptab, F):
    """The device's ptab [V, PS] as [V, 3, F]."""
    return np.ascontiguousarray(np.asarray(ptab)[:, :3 * F]).reshape(len(ptab), 3, F)


# ---------------------------------------------------------------- the search
ITEM = 64


def crossed(score, target, direction):
    score, target = f32(score), f32(target)
    return bool(score < target) if direction == 0 else bool(score > target)


def candidates(lens, mask, cand, S, T):
    """The slots of one side that are a step: set in ``cand`` (None: the side is not searched), not yet removed, below
    min(count, S), not empty and starting before T in the CURRENT document."""
    out, start = [], 0
    if cand is None:
        return out
    for s, n in enumerate(lens[:min(S, SLOTS)]):
        gone = (int(mask) >> s) & 1
        if (int(cand) >> s) & 1 and not gone and n > 0 and start < T:
            out.append(s)
        if not gone:
            start += n
    return out


def better(sa, ca, sb, cb, direction):
    """Is candidate (sb, cb) better than (sa, ca)?  ca None: there is none yet."""
    if ca is None:
        return True
    na, nb = bool(np.isnan(sa)), bool(np.isnan(sb))
    if na != nb:
        return na
    if na or f32(sa) == f32(sb):
        return cb < ca
    return bool(sb < sa) if direction == 0 else bool(sb > sa)


def search(score, lens_u, lens_i, S_u, S_i, T, start_u, start_i, cand_u, cand_i, target, direction, budget):
    """One pair's greedy search.  ``score(mask_u, mask_i)`` -> fp32; ``lens_*``: the lengths of the owner's first 64
    reviews -> (order [B], scores [B + 1], steps, crossed) with the fills of include/r4r.h."""
    mu, mi = int(start_u), int(start_i)
    s = f32(score(mu, mi))
    order, scores = [-1] * budget, [s] * (budget + 1)
    steps, hit = 0, crossed(s, target, direction)
    while not hit and steps < budget:
        best_s, best_c = None, None
        for slot in candidates(lens_u, mu, cand_u, S_u, T):
            sc = f32(score(mu | (1 << slot), mi))
            if better(best_s, best_c, sc, slot, direction):
                best_s, best_c = sc, slot
        for slot in candidates(lens_i, mi, cand_i, S_i, T):
            sc = f32(score(mu, mi | (1 << slot)))
            if better(best_s, best_c, sc, ITEM + slot, direction):
                best_s, best_c = sc, ITEM + slot
        if best_c is None:
            break
        if best_c < ITEM:
            mu |= 1 << best_c
        else:
            mi |= 1 << (best_c - ITEM)
        order[steps] = best_c
        steps += 1
        scores[steps:] = [best_s] * (budget + 1 - steps)
        hit = crossed(best_s, target, direction)
    return order, scores, steps, hit


def brute_docs(P, b, docs):
    """``brute`` over the rows of docs [n, T] at once: every window's value in the kernel's order of adds, then the
    maximum (which does not depend on the order it is taken in) -> pooled [n, F]."""
    docs = np.asarray(docs, np.int64)
    n, T = docs.shape
    Pz = np.concatenate([P, np.zeros((1,) + P.shape[1:], f32)])           # row V: a tap outside the document
    ext = np.full((n, T + 4), len(P), np.int64)
    ext[:, 2:T + 2] = docs
    out = np.empty((n, len(b)), f32)
    for r in range(n):
        a, c, d = ext[r, 0:T + 2], ext[r, 1:T + 3], ext[r, 2:T + 4]
        y = ((Pz[a, 0] + Pz[c, 1]) + Pz[d, 2]) + b[None, :]
        out[r] = relu(y.max(0))
    return out
