"""``ops.fold_search`` (include/r4r.h, "Document fold": r4r_fold_search_begin / _rows / _pick around r4r_fold_compose,
r4r_linear_fwd and r4r_pair_grad) against a host replay of the rule, with no tolerance: the replay takes every step on
the host -- tower_fold_ref's ``candidates`` and ``better`` -- and scores every candidate's mask with
``ops.fold_compose`` + r4r_linear_fwd + ``ops.pair_grad``.  Order, score bits, steps, crossed and the fills are
compared, for the three heads, one to 64 slots a side, budgets below, at and above the lists, both directions, targets
at +-inf, NaN, a step's own bits and one ulp either side of them, empty / partial / start masks, reviews that do not
show, exact ties, and a pair alone, in a batch, permuted and under a smaller budget."""
import numpy as np
import pytest
import torch

import tower_fold_ref as R
from tower_variants_ref import as_signed

pytestmark = pytest.mark.gpu
DEV = 'cuda'
V, E, F, L, P, T = 60, 8, 70, 6, 3, 20
ALL = (1 << 64) - 1
INF, NAN = float('inf'), float('nan')


def _side_pool(rng, S, owners):
    """Owners with 0 .. S (S = 64: up to 70) reviews of 0 .. 6 words; owner 0 has exactly S, owner 1 starts with two
    IDENTICAL reviews (removing either leaves the same document: an exact tie) -- where S allows."""
    counts = [S] + [int(rng.randint(0, (70 if S == 64 else S) + 1)) for _ in range(owners - 1)]
    lens = [rng.randint(0, 7, size=c) for c in counts]
    if S >= 2:
        counts[1] = max(counts[1], 2)
        lens[1] = np.concatenate([[3, 3], rng.randint(0, 7, size=counts[1] - 2)])
    flat = np.concatenate(lens).astype(np.int64)
    rev_off = np.concatenate([[0], np.cumsum(flat)]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    tok = rng.randint(0, V, size=int(rev_off[-1])).astype(np.int32)
    if S >= 2:
        at = int(rev_off[first[1]])
        tok[at + 3:at + 6] = tok[at:at + 3]
    return tok, rev_off, first, [[int(x) for x in l[:64]] for l in lens]


def _head(kind, rng_t, n_p):
    r = lambda *s: torch.randn(*s, generator=rng_t).to(DEV)
    if kind == 'fm':
        return dict(V=r(2 * L, 8) * 0.3, lw=r(2 * L), q_bias=r(n_p))
    if kind == 'mlp':
        return dict(W0=r(L, 2 * L) * 0.5, b0=r(L) * 0.1, w3=r(L), q_bias=r(n_p), c_bias=r(n_p))
    return dict(W0=r(L, 2 * L) * 0.5, b0=r(L) * 0.1, W2=r(L, L) * 0.5, b2=r(L) * 0.1, V=r(2 * P + L, 8) * 0.3,
                lw=r(2 * P + L), q_bias=r(n_p), xu=r(n_p, P), xi=r(n_p, P))


PER_PAIR = ('q_bias', 'c_bias', 'xu', 'xi')


def _setup(kind, S_u, S_i, n_p, seed):
    from reviews4rec_amd import ops
    rng, g = np.random.RandomState(seed), torch.Generator().manual_seed(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    table = torch.randn(V, E, generator=g).to(DEV)
    sides, lens = [], []
    for S in (S_u, S_i):
        owners = 4
        tok, rev_off, first, ln = _side_pool(rng, S, owners)
        conv_w, conv_b = (torch.randn(F, 1, 3, E, generator=g) * 0.3).to(DEV), (torch.randn(F, generator=g) * 0.1).to(DEV)
        fc_w, fc_b = (torch.randn(L, F, generator=g) * 0.2).to(DEV), (torch.randn(L, generator=g) * 0.1).to(DEV)
        pool = (t(np.concatenate([tok, np.zeros(1, np.int32)])), t(rev_off), t(first), None)
        ids = t(np.arange(owners, dtype=np.int64)[::-1].copy())           # ids in another order than the indices
        ptab = ops.fold_project(table, conv_w)
        seg = ops.fold_segments(ptab, conv_b, pool, ids, S)
        sides.append(dict(ptab=ptab, conv_b=conv_b, seg=seg, pool=pool, ids=ids, fc_w=fc_w, fc_b=fc_b))
        lens.append([ln[o] for o in range(owners)][::-1])                 # by index into ids
    own = [rng.randint(0, 4, size=n_p).astype(np.int64) for _ in range(2)]
    own[0][:2], own[1][:2] = (3, 2)[:min(2, n_p)], (3, 2)[:min(2, n_p)]   # owner 0 (index 3) and the tie owner (index 2)
    masks = {}
    for name, S in (('start_u', S_u), ('start_i', S_i), ('cand_u', S_u), ('cand_i', S_i)):
        m = []
        for p in range(n_p):
            kindm = (p + (7 if 'cand' in name else 0)) % 5
            if name.startswith('start'):
                m.append(0 if kindm < 3 else int(rng.randint(0, 1 << min(S, 30))) | (1 << 63 if kindm == 4 else 0))
            else:
                m.append((ALL, ALL, int(rng.randint(0, 1 << min(S, 30))) | (ALL >> S << S if S < 64 else 0), 0,
                          ALL & ~1)[kindm] if p >= 2 else ALL)
        masks[name] = np.array([as_signed(x) for x in m], np.int64)
    head = _head(kind, g, n_p)
    return dict(kind=kind, sides=sides, lens=lens, own=own, masks=masks, head=head, S=(S_u, S_i), n_p=n_p, t=t)


def _search(s, target, direction, budget, sel=None, cand=True):
    from reviews4rec_amd import ops
    sel = np.arange(s['n_p']) if sel is None else np.asarray(sel)
    t = s['t']
    head = {k: (v[torch.from_numpy(sel).to(DEV)].contiguous() if k in PER_PAIR else v) for k, v in s['head'].items()}
    m = {k: t(v[sel]) for k, v in s['masks'].items()}
    out = ops.fold_search(s['kind'], head, s['sides'][0], s['sides'][1], t(s['own'][0][sel]), t(s['own'][1][sel]),
                          t(np.asarray(target, np.float32)[sel]), direction, budget, T, start_u=m['start_u'],
                          start_i=m['start_i'], cand_u=m['cand_u'] if cand else None, cand_i=m['cand_i'])
    return [o.cpu().numpy() for o in out]


def _score_rows(s, rows):
    """The scores of [(pair, mask_u, mask_i)] by compose + fc + pair_grad: one call of each, the rows as they come."""
    from reviews4rec_amd import ops
    t = s['t']
    pair = np.array([r[0] for r in rows], np.int64)
    z = []
    for side, col in ((0, 1), (1, 2)):
        drop = t(np.array([as_signed(r[col]) for r in rows], np.int64))
        z.append(ops.fold_latents(s['sides'][side], t(s['own'][side][pair]), T, drop=drop))
    at = torch.from_numpy(pair).to(DEV)
    head = {k: (v[at].contiguous() if k in PER_PAIR else v) for k, v in s['head'].items()}
    idx = torch.arange(len(rows), dtype=torch.int64, device=DEV)
    return ops.pair_grad(s['kind'], z[0], z[1], idx, idx, want=('score',), **head)['score'].cpu().numpy()


def _replay(s, target, direction, budget, cand=True):
    """The rule on the host, every pair in step: -> order, scores, steps, crossed as ``ops.fold_search`` returns them."""
    n_p, (S_u, S_i) = s['n_p'], s['S']
    u64 = lambda x: int(x) & ALL
    mu = [u64(x) for x in s['masks']['start_u']]
    mi = [u64(x) for x in s['masks']['start_i']]
    cu = [u64(x) if cand else None for x in s['masks']['cand_u']]
    ci = [u64(x) for x in s['masks']['cand_i']]
    lens_u = [s['lens'][0][o] for o in s['own'][0]]
    lens_i = [s['lens'][1][o] for o in s['own'][1]]
    s0 = _score_rows(s, [(p, mu[p], mi[p]) for p in range(n_p)])
    order = np.full((n_p, budget), -1, np.int32)
    scores = np.repeat(s0[:, None], budget + 1, 1).astype(np.float32)
    steps = np.zeros(n_p, np.int32)
    hit = np.array([R.crossed(s0[p], target[p], direction) for p in range(n_p)])
    done = hit.copy()
    for _ in range(budget):
        rows, spans = [], []
        for p in range(n_p):
            at = len(rows)
            if not done[p]:
                rows += [(p, mu[p] | (1 << c), mi[p], c) for c in R.candidates(lens_u[p], mu[p], cu[p], S_u, T)]
                rows += [(p, mu[p], mi[p] | (1 << c), R.ITEM + c) for c in R.candidates(lens_i[p], mi[p], ci[p], S_i, T)]
            spans.append((at, len(rows)))
        if not rows:
            break
        sc = _score_rows(s, rows)
        for p, (a, b) in enumerate(spans):
            if done[p]:
                continue
            if a == b:
                done[p] = True
                continue
            best_s = best_c = None
            for r in range(a, b):
                if R.better(best_s, best_c, sc[r], rows[r][3], direction):
                    best_s, best_c = sc[r], rows[r][3]
            if best_c < R.ITEM:
                mu[p] |= 1 << best_c
            else:
                mi[p] |= 1 << (best_c - R.ITEM)
            order[p, steps[p]] = best_c
            steps[p] += 1
            scores[p, steps[p]:] = best_s
            hit[p] = R.crossed(best_s, target[p], direction)
            done[p] = hit[p] or steps[p] >= budget
    return order, scores, steps, hit.astype(np.int32)


def _targets(s, direction, budget):
    """Per pair, in turn: never / always crossed, NaN, the bits of the pair's first step, one ulp either side."""
    n_p = s['n_p']
    never = np.full(n_p, -INF if direction == 0 else INF, np.float32)
    _, free, _, _ = _search(s, never, direction, budget)
    one = free[:, 1]
    kinds = [never, -never, np.full(n_p, NAN, np.float32), one, np.nextafter(one, np.float32(INF)),
             np.nextafter(one, np.float32(-INF)), free[:, min(2, budget)]]
    return np.array([kinds[p % len(kinds)][p] for p in range(n_p)], np.float32), free


def _equal(got, want):
    for g, w, name in zip(got, want, ('order', 'scores', 'steps', 'crossed')):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert g.tobytes() == w.tobytes(), (name, np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:8])


CASES = [('fm', 1, 1, 5, 1, 0), ('mlp', 5, 5, 257, 2, 1), ('pfm', 12, 5, 5, 12, 0), ('fm', 64, 64, 5, 64, 0),
         ('mlp', 12, 12, 5, 64, 1), ('pfm', 5, 5, 1, 5, 1), ('fm', 5, 12, 40, 5, 0)]


@pytest.mark.parametrize('kind, S_u, S_i, n_p, budget, direction', CASES)
def test_the_search_is_the_host_replay_of_the_rule(kind, S_u, S_i, n_p, budget, direction):
    s = _setup(kind, S_u, S_i, n_p, seed=S_u * 100 + S_i + n_p)
    target, free = _targets(s, direction, budget)
    got = _search(s, target, direction, budget)
    want = _replay(s, target, direction, budget)
    print('%s S=%d/%d n_p=%d B=%d dir=%d: steps %s, crossed %d' % (kind, S_u, S_i, n_p, budget, direction,
                                                                     np.bincount(want[2]).tolist(), int(want[3].sum())))
    _equal(got, want)
    _equal(_search(s, np.full(n_p, -INF if direction == 0 else INF, np.float32), direction, budget),
           _replay(s, np.full(n_p, -INF if direction == 0 else INF, np.float32), direction, budget))
    assert (got[0] >= -1).all() and (got[2] <= budget).all()
    if S_u >= 2 and n_p >= 2 and budget >= 1:                 # the tie owner's pair: both of its first two reviews
        o, sc, st, _ = _search(s, np.full(n_p, NAN, np.float32), direction, budget)      # are candidates, never slot 1 first
        taken = [c for c in o[1][:st[1]] if c < R.ITEM]
        assert 1 not in taken or taken.index(0) < taken.index(1)


def test_a_pair_alone_in_a_batch_permuted_and_under_a_smaller_budget():
    s = _setup('mlp', 12, 5, 9, seed=3)
    for direction in (0, 1):
        target, _ = _targets(s, direction, 7)
        whole = _search(s, target, direction, 7)
        perm = np.random.RandomState(1).permutation(9)
        _equal(_search(s, target, direction, 7, sel=perm), [w[perm] for w in whole])
        for p in (0, 4):
            _equal(_search(s, target, direction, 7, sel=[p]), [w[p:p + 1] for w in whole])
        for B in (1, 2, 6):                                  # a budget is the prefix of a larger one
            o, sc, st, cr = _search(s, target, direction, B)
            cut = np.minimum(whole[2], B)
            assert np.array_equal(st, cut)
            for p in range(9):
                assert np.array_equal(o[p, :st[p]], whole[0][p, :st[p]]) and (o[p, st[p]:] == -1).all()
                assert sc[p, :st[p] + 1].tobytes() == whole[1][p, :st[p] + 1].tobytes()
                assert (sc[p, st[p]:].view(np.int32) == sc[p, st[p]].view(np.int32)).all()
                assert cr[p] == int(R.crossed(sc[p, st[p]], target[p], direction))


def test_one_side_alone_is_the_search_with_no_candidate_on_the_other():
    s = _setup('pfm', 5, 12, 6, seed=8)
    target = np.full(6, -INF, np.float32)
    _equal(_search(s, target, 0, 12, cand=False), _replay(s, target, 0, 12, cand=False))
    got = _search(s, target, 0, 12, cand=False)
    assert ((got[0] == -1) | (got[0] >= R.ITEM)).all()
