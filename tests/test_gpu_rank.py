"""Full-catalogue ranks on the device: r4r_rank_dot (csrc/topk.hip, include/r4r.h "Catalogue recommendation"),
recommend.Catalogue.rank and eval.eval_catalogue on top of it.

The reference is numpy on float64 scores with the header's total order: the rank of target t for query row u is the
number of candidates j != t whose score is neither -inf nor NaN, that are not excluded for u, and with
s_j > s_t || (s_j == s_t && j < t); -1 when the target's own score is -inf or NaN.  With inputs that are multiples of
1/8 (biases: of 1/64) every partial sum is exact in fp32 for D <= 256, so the kernel must return exactly that count.
With real-valued inputs the reference is the same order over the fp32 bits r4r_pair_dot returns for ALL pairs: the
MFMA scan is the scalar chain, so the ranks are demanded exactly there too, with no tolerance; the a-priori bound of
tests/test_gpu_recommend.py (dot_bound) only brackets them against float64 as a sanity check."""
import functools

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from test_gpu_recommend import (EXACT, _all_pairs, _tiny_model, dot_bound, dyadic, real_inputs, ref_scores, small_chunk,
                                topk)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------- the reference ranks
def ref_ranks(s, qi, ti, excl=None):
    """s: scores [n_q, n_c] (float64, or the fp32 bits of r4r_pair_dot), pairs (qi[p], ti[p]), excl = (off, ids) per
    query ROW -> int64 [n_p]."""
    n_c = s.shape[1]
    ids = np.arange(n_c)
    out = np.empty(len(qi), np.int64)
    with np.errstate(invalid='ignore'):
        for p, (u, t) in enumerate(zip(qi.tolist(), ti.tolist())):
            row, st = s[u], s[u, t]
            if not st > -np.inf:                              # -inf or NaN
                out[p] = -1
                continue
            ahead = (row > st) | ((row == st) & (ids < t))    # (false for -inf and NaN: st is neither)
            if excl is not None:
                e = excl[1][excl[0][u]:excl[0][u + 1]]
                ahead[e[(e >= 0) & (e < n_c)]] = False
            ahead[t] = False
            out[p] = int(ahead.sum())
    return out


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Ranker:
    """r4r_rank_dot over numpy tables, uploaded once; c goes to the device with a row stride of D + pad (NaN pad)."""

    def __init__(self, q, qb, c, cb, excl=None, pad=3):
        self.n_q, self.D = q.shape
        self.n_c, self.stride = c.shape[0], self.D + pad
        self.cs = torch.full((max(self.n_c, 1), max(self.stride, 1)), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.D:
            self.cs[:self.n_c, :self.D] = _dev(c)
        self.q = _dev(q.reshape(-1) if q.size else np.zeros(1, np.float32))
        self.qb, self.cb = _dev(qb), _dev(cb)
        self.excl = None if excl is None else (_dev(excl[0]), _dev(np.concatenate([excl[1], np.zeros(1, np.int64)])))

    def __call__(self, qi, ti, chunk=0, excl=True):
        from reviews4rec_amd import _lib
        from reviews4rec_amd._lib import ptr
        n_p = len(qi)
        qid, tid = _dev(np.asarray(qi, np.int64)), _dev(np.asarray(ti, np.int64))
        ranks = torch.full((n_p,), -7, dtype=torch.int64, device=DEV)
        sc = torch.full((n_p,), 7.0, dtype=torch.float32, device=DEV)
        eo, ei = self.excl if (excl and self.excl is not None) else (None, None)
        _lib.call('r4r_rank_dot', ptr(self.q), self.n_q, ptr(self.qb), ptr(self.cs), self.n_c, self.stride, ptr(self.cb),
                  self.D, ptr(qid), ptr(tid), n_p, ptr(eo), ptr(ei), chunk, ptr(ranks), ptr(sc))
        torch.cuda.synchronize()
        return ranks.cpu().numpy(), sc.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def random_lists(rng, n_q, n_c, longest=40):
    """A CSR of ascending distinct ids per query row, some rows empty."""
    lists = [np.sort(rng.permutation(n_c)[:rng.integers(0, min(n_c, longest) + 1)]).astype(np.int64) for _ in range(n_q)]
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, np.concatenate(lists + [np.zeros(0, np.int64)])


# ---------------------------------------------------------------- 1. exact arithmetic
RANK_EXACT = sorted({(n, n_c, D) for n, n_c, D, _ in EXACT} |
                    {(511, 257, 5), (512, 4099, 64), (577, 1000, 128), (513, 300, 256), (600, 255, 0),
                     # the target kernel's last 256-thread workgroup exactly full / holding one pair, 65 candidates
                     (256, 65, 5), (257, 65, 8)})


@functools.lru_cache(maxsize=None)
def exact_case(n_p, n_c, D):
    """Inputs, pairs, exclusions and the float64 reference of one exact case (computed once, never modified)."""
    rng = np.random.default_rng(n_p * 1000003 + n_c * 131 + D * 7 + 1)
    n_q = (n_p + 1) // 2
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    cb[rng.random(n_c) < 0.1] = -np.inf                                               # a tenth is ineligible
    qi, ti = rng.integers(0, n_q, n_p), rng.integers(0, n_c, n_p)
    excl = random_lists(rng, n_q, n_c)
    s = ref_scores(q, qb, c, cb)
    for a in (q, c, qb, cb, qi, ti, s) + excl:
        a.setflags(write=False)
    return dict(q=q, c=c, qb=qb, cb=cb, qi=qi, ti=ti, excl=excl, s=s,
                free=ref_ranks(s, qi, ti), masked=ref_ranks(s, qi, ti, excl))


def test_the_exact_cases_hold_ties_on_both_sides_and_unranked_targets():
    """On the reference alone: the generator must produce what the exact test is there to catch."""
    assert len(RANK_EXACT) == 50
    lower = higher = unranked = 0
    for n_p, n_c, D in RANK_EXACT:
        k = exact_case(n_p, n_c, D)
        s, qi, ti = k['s'], k['qi'], k['ti']
        ok = k['free'] >= 0
        tied = s[qi[ok]] == s[qi[ok], ti[ok]][:, None]                                # [pairs, n_c]; the targets are finite
        ids = np.arange(n_c)[None, :]
        lower += bool((tied & (ids < ti[ok][:, None])).any())
        higher += bool((tied & (ids > ti[ok][:, None])).any())
        unranked += bool((k['free'] == -1).any())
        assert np.array_equal((k['free'] == -1), (k['masked'] == -1))
    assert lower >= 20 and higher >= 20 and unranked >= 10, (lower, higher, unranked)


@pytest.mark.parametrize('n_p, n_c, D', RANK_EXACT)
def test_exact_inputs_give_the_reference_rank(n_p, n_c, D):
    k = exact_case(n_p, n_c, D)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(k['s'].astype(np.float32).astype(np.float64), k['s'])   # exact in fp32
    want_sc = k['s'][k['qi'], k['ti']].astype(np.float32)
    call = Ranker(k['q'], k['qb'], k['c'], k['cb'], excl=k['excl'])
    chunks = (0, small_chunk(n_c))
    assert n_c < 3 or -(-n_c // chunks[1]) >= 3
    for chunk in chunks:
        for excl in (False, True):
            ranks, sc = call(k['qi'], k['ti'], chunk, excl=excl)
            want = k['masked'] if excl else k['free']
            assert np.array_equal(ranks, want), (chunk, excl, np.argwhere(ranks != want)[:5].ravel())
            assert np.array_equal(bits(sc), bits(want_sc)), (chunk, excl)


def test_null_biases_count_as_zero():
    k = exact_case(33, 4099, 64)
    s = ref_scores(k['q'], None, k['c'], None)
    ranks, sc = Ranker(k['q'], None, k['c'], None, excl=k['excl'])(k['qi'], k['ti'], small_chunk(4099))
    assert np.array_equal(ranks, ref_ranks(s, k['qi'], k['ti'], k['excl']))
    assert np.array_equal(bits(sc), bits(s[k['qi'], k['ti']].astype(np.float32)))


# ---------------------------------------------------------------- 2. degenerate rankings
@pytest.mark.parametrize('case', ['all equal', 'every candidate -inf', 'NaN', 'one candidate', 'the same pair twice'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_p, n_c, D = 17, (1 if case == 'one candidate' else 300), 8
    n_q = 9
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 1.0)
    qi, ti = rng.integers(0, n_q, n_p), rng.integers(0, n_c, n_p)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
        cb[rng.permutation(n_c)[:30]] = -np.inf
        ti[:3] = np.nonzero(np.isneginf(cb))[0][:3]
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    elif case == 'NaN':
        c[41], c[42, 3] = np.nan, np.nan
        q[0] = 0.0                                                                   # 0 * NaN is NaN all the same
        cb[43] = np.nan
        ti[:6], qi[:6] = [41, 42, 43, 41, 42, 43], [0, 0, 0, 1, 2, 3]
    elif case == 'the same pair twice':
        qi[9:], ti[9:] = qi[:8], ti[:8]
    s = ref_scores(q, qb, c, cb)
    want = ref_ranks(s, qi, ti)
    if case == 'all equal':
        el = ~np.isneginf(cb)
        assert (want[:3] == -1).all() and (want[3:] == [int(el[:t].sum()) for t in ti[3:]]).all()
    if case == 'every candidate -inf':
        assert (want == -1).all()
    if case == 'NaN':
        assert (want[:6] == -1).all() and (want[6:] >= 0).all()
    if case == 'one candidate':
        assert (want == 0).all()
    call = Ranker(q, qb, c, cb)
    for chunk in (0, 64, 7):
        ranks, sc = call(qi, ti, chunk)
        assert np.array_equal(ranks, want), (case, chunk)
        assert np.array_equal(sc, s[qi, ti].astype(np.float32), equal_nan=True), (case, chunk)
        if case == 'the same pair twice':
            assert np.array_equal(ranks[9:], ranks[:8]) and np.array_equal(bits(sc[9:]), bits(sc[:8]))


# ---------------------------------------------------------------- 3. exclusions
def test_exclusions():
    rng = np.random.default_rng(6)
    n_q, n_c, D = 6, 1000, 8
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 1.0)
    cb[rng.permutation(n_c)[:100]] = -np.inf
    cb[77] = np.nan
    dead = np.nonzero(~np.isfinite(cb))[0].astype(np.int64)
    live = np.nonzero(np.isfinite(cb))[0].astype(np.int64)
    s = ref_scores(q, qb, c, cb)
    n_p = 60
    qi = np.repeat(np.arange(n_q), 10)
    ti = rng.choice(live, n_p)
    ti[7], ti[17] = dead[0], 77                                                      # unranked targets stay unranked
    free = ref_ranks(s, qi, ti)
    best = [int(np.nanargmax(np.where(np.isfinite(s[u]), s[u], -np.inf))) for u in range(n_q)]
    lists = [np.zeros(0, np.int64),                                                  # an empty list
             np.unique(np.concatenate([ti[10:20], [best[1]]])),                      # the row's own targets and its best
             np.arange(n_c, dtype=np.int64),                                         # everything: rank 0
             np.sort(rng.permutation(n_c)[:300]).astype(np.int64),                   # long, across every chunk boundary
             dead.copy(),                                                            # ineligible ids only
             np.unique(np.concatenate([dead[:40], live[:200]]))]                     # both kinds
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want = ref_ranks(s, qi, ti, excl)
    ok = free >= 0
    assert np.array_equal(want[:10], free[:10]) and np.array_equal(want[40:50], free[40:50])
    assert (want[20:30] == 0).all() and (want[ok] <= free[ok]).all() and (want[30:40] < free[30:40]).any()
    assert want[7] == -1 and want[17] == -1 and (want[10:17] >= 0).all()            # an excluded target is still ranked
    assert (want[10:20][free[10:20] > 0] < free[10:20][free[10:20] > 0]).all()       # ... and the best of row 1 is gone
    call = Ranker(q, qb, c, cb, excl=excl)
    for chunk in (0, 64, 333):
        ranks, sc = call(qi, ti, chunk)
        assert np.array_equal(ranks, want), (chunk, np.argwhere(ranks != want)[:5].ravel())
        assert np.array_equal(sc, s[qi, ti].astype(np.float32), equal_nan=True), chunk
        assert np.array_equal(call(qi, ti, chunk, excl=False)[0], free), chunk
        # five pairs: waves of the exclusion kernel's last workgroup have no pair.  Rows 2 (1000 excluded ids, the targets
        # among them) and 3 (300): the kernel's lane loop takes 16 and 5 trips
        five = slice(28, 33)
        ranks, sc = call(qi[five], ti[five], chunk)
        assert np.array_equal(ranks, want[five]) and np.array_equal(sc, s[qi[five], ti[five]].astype(np.float32), equal_nan=True), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
def pair_bits(q, qb, c, cb, rows):
    """r4r_pair_dot for every (query row of `rows`, candidate) pair -> float32 [len(rows), n_c]."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    n_q, D = q.shape
    n_c = c.shape[0]
    qd = _dev(q if D else np.zeros((n_q, 1), np.float32))
    cd = _dev(c if D else np.zeros((n_c, 1), np.float32))
    qbd, cbd = _dev(qb), _dev(cb)
    qi = _dev(np.repeat(np.asarray(rows, np.int64), n_c))
    ci = _dev(np.tile(np.arange(n_c, dtype=np.int64), len(rows)))
    out = torch.empty(len(rows) * n_c, dtype=torch.float32, device=DEV)
    _lib.call('r4r_pair_dot', ptr(qd), n_q, ptr(qbd), ptr(cd), n_c, D, ptr(cbd), D, ptr(qi), ptr(ci), len(rows) * n_c,
              ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(rows), n_c)


@pytest.mark.parametrize('n_p', [33, 513])
@pytest.mark.parametrize('D', [0, 1, 3, 10, 64, 100, 256])
def test_real_valued_ranks_are_the_order_of_the_pair_scores(D, n_p):
    n_c, n_q = 4099, (n_p + 1) // 2
    q, qb, c, cb = real_inputs(D, n_q=n_q, n_c=n_c, seed=3)
    rng = np.random.default_rng(7 * D + n_p)
    qi, ti = rng.integers(0, n_q, n_p), rng.integers(0, n_c, n_p)
    excl = random_lists(rng, n_q, n_c)
    s32 = pair_bits(q, qb, c, cb, np.arange(n_q))                                    # ALL n_q x n_c scores, fp32 bits
    want = {False: ref_ranks(s32, qi, ti), True: ref_ranks(s32, qi, ti, excl)}
    call = Ranker(q, qb, c, cb, excl=excl)
    for chunk in (0, small_chunk(n_c)):
        for with_excl in (False, True):
            ranks, sc = call(qi, ti, chunk, excl=with_excl)
            assert np.array_equal(ranks, want[with_excl]), (chunk, with_excl, int((ranks != want[with_excl]).sum()))
            assert np.array_equal(bits(sc), bits(s32[qi, ti])), (chunk, with_excl)
    # the sanity interval against float64: surely ahead <= rank <= others - surely behind
    s64 = ref_scores(q, qb, c, cb)
    tol = dot_bound(q, np.abs(qb), c, cb, D)
    lo_t, hi_t = (s64 - tol)[qi, ti][:, None], (s64 + tol)[qi, ti][:, None]
    others = np.ones((n_p, n_c), bool)
    others[np.arange(n_p), ti] = False
    surely_ahead = (((s64 - tol)[qi] > hi_t) & others).sum(1)
    surely_behind = (((s64 + tol)[qi] < lo_t) & others).sum(1)
    assert (surely_ahead <= want[False]).all() and (want[False] <= n_c - 1 - surely_behind).all()
    assert (np.abs(s32[qi, ti].astype(np.float64) - s64[qi, ti]) <= tol[qi, ti]).all()


# ---------------------------------------------------------------- 5. invariance
@pytest.mark.parametrize('D', [10, 64, 256])
def test_grouping_and_chunking_do_not_change_a_rank(D):
    n_c, n_q, n_p = 4099, 33, 200
    q, qb, c, cb = real_inputs(D, n_q=n_q, n_c=n_c, seed=4)
    rng = np.random.default_rng(D)
    qi, ti = rng.integers(0, n_q, n_p), rng.integers(0, n_c, n_p)
    call = Ranker(q, qb, c, cb, excl=random_lists(rng, n_q, n_c))
    want = call(qi, ti, 0)
    assert (want[0] >= 0).all() and len(set(want[0].tolist())) > 100

    def same(got, what):
        assert np.array_equal(got[0], want[0]), what
        assert np.array_equal(bits(got[1]), bits(want[1])), what

    cat = lambda parts: (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    for chunk in (500, 4099, 77):
        same(call(qi, ti, chunk), ('all at once', chunk))
        same(cat([call(qi[a:b], ti[a:b], chunk) for a, b in ((0, 100), (100, 200))]), ('halves', chunk))
    same(cat([call(qi[p:p + 1], ti[p:p + 1], 500) for p in range(n_p)]), 'one by one')
    # ... and inside a call of 712 pairs, which runs the 64-pair tiles where D <= 128
    more_q, more_t = rng.integers(0, n_q, 512), rng.integers(0, n_c, 512)
    got = call(np.concatenate([more_q[:300], qi, more_q[300:]]), np.concatenate([more_t[:300], ti, more_t[300:]]), 0)
    same((got[0][300:500], got[1][300:500]), 'inside 712 pairs')


# ---------------------------------------------------------------- 6. agreement with the lists
@pytest.mark.parametrize('D', [10, 64])
def test_every_slot_of_a_list_has_its_position_as_rank(D):
    n_q, n_c, K = 33, 4099, 128
    q, qb, c, cb = real_inputs(D, seed=5)
    cb[::7] = -np.inf
    excl = random_lists(np.random.default_rng(D + 1), n_q, n_c, longest=200)
    call = Ranker(q, qb, c, cb, excl=excl)
    for with_excl in (False, True):
        ids, sc = topk(q, qb, c, cb, K, 0, excl=excl if with_excl else None)
        assert (ids >= 0).all()
        ranks, rsc = call(np.repeat(np.arange(n_q), K), ids.reshape(-1), 0, excl=with_excl)
        assert np.array_equal(ranks.reshape(n_q, K), np.tile(np.arange(K), (n_q, 1))), with_excl
        assert np.array_equal(bits(rsc), bits(sc.reshape(-1))), with_excl


# ---------------------------------------------------------------- 7. end to end on tests/golden/tiny
@pytest.mark.parametrize('mt', ['MF_dot', 'bias_only', 'deepconn'])
def test_catalogue_rank_on_tiny_against_the_oracle(mt, tmp_path):
    import oracle
    from reviews4rec_amd import Catalogue, eval_catalogue, ranking_metrics
    hp, train, test, model, W = _tiny_model(mt, tmp_path)
    U, I = hp['total_users'], hp['total_items']
    u, i, data = _all_pairs(hp, test)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    if mt == 'deepconn':
        tol = 1e-5 + 1e-5 * np.abs(s64)                       # the project's eval tolerance (test_gpu_models.py)
    else:
        D = hp['latent_size'] if mt == 'MF_dot' else 0
        q = W['user_embedding.weight'].numpy()[:U] if D else np.zeros((U, 0), np.float32)
        c = W['item_embedding.weight'].numpy()[:I] if D else np.zeros((I, 0), np.float32)
        qterms = np.abs(W['user_bias'].numpy()[:U]) + abs(float(W['global_bias']))
        tol = dot_bound(q, qterms, c, W['item_bias'].numpy()[:I], D)
    cat = Catalogue(model, hp, train)
    el = np.zeros(I, bool)
    el[sorted({int(r[1]) for r in train.data})] = True
    seen = np.zeros((U, I), bool)
    for r in train.data:
        seen[int(r[0]), int(r[1])] = True
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    by_exclude = {}
    for exclude in (True, False):
        ranks, sc = cat.rank(u, i, exclude_seen=exclude)
        assert ranks.device.type == 'cuda' and ranks.dtype == torch.int64 and sc.dtype == torch.float32
        ranks, sc = ranks.cpu().numpy().reshape(U, I), sc.cpu().numpy().reshape(U, I)
        by_exclude[exclude] = ranks
        assert np.array_equal(ranks == -1, np.broadcast_to(~el[None, :], (U, I)))    # -1 exactly on ineligible items
        assert np.array_equal(bits(sc), bits(got))                                   # score_pairs' bits
        counted = np.broadcast_to(el[None, :], (U, I)) & ~(seen if exclude else np.zeros_like(seen))
        # exactly the numpy order over score_pairs' bits (-inf on ineligible items; an excluded target keeps its rank)
        csr = (np.concatenate([[0], np.cumsum(seen.sum(1))]).astype(np.int64), np.nonzero(seen)[1].astype(np.int64))
        want = ref_ranks(got, u, i, csr if exclude else None).reshape(U, I)
        assert np.array_equal(ranks, want), (mt, exclude, int((ranks != want).sum()))
        # inside the interval the float64 oracle forward and the tolerance allow
        for uu in range(U):
            lo, hi = s64[uu] - tol[uu], s64[uu] + tol[uu]
            for ii in np.nonzero(el)[0]:
                others = counted[uu].copy()
                others[ii] = False
                ahead, behind = int((lo[others] > hi[ii]).sum()), int((hi[others] < lo[ii]).sum())
                assert ahead <= ranks[uu, ii] <= int(others.sum()) - behind, (mt, exclude, uu, ii)
    assert (by_exclude[True] <= by_exclude[False]).all()
    # eval_catalogue == ranking_metrics of those ranks on the test rows
    tu, ti = test.data[:, 0].astype(np.int64), test.data[:, 1].astype(np.int64)
    m = ranking_metrics(by_exclude[True][tu, ti], (1, 5, 10))
    want = {'cat_' + k: round(100.0 * v, 2) for k, v in m.items() if k not in ('ranked', 'unranked')}
    want.update(cat_ranked=m['ranked'], cat_unranked=m['unranked'])
    for kw in (dict(catalogue=cat), dict()):
        res = eval_catalogue(model, train, test, hp, ks=(1, 5, 10), **kw)
        assert res == want, (res, want)
    assert res['cat_ranked'] + res['cat_unranked'] == len(test.data) and res['cat_ranked'] > 0
    # ids may arrive as lists or device tensors
    a = cat.rank(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    b = cat.rank(u.tolist(), i.tolist())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[0].cpu().numpy().reshape(U, I), by_exclude[True])
    empty = cat.rank([], [])
    assert empty[0].shape == (0,) and empty[0].dtype == torch.int64 and empty[1].shape == (0,)
    with pytest.raises(ValueError):
        cat.rank([0], [cat.n_c])
    with pytest.raises(ValueError):
        cat.rank([0, 1], [0])


# ---------------------------------------------------------------- 8. engines
def test_a_rank_pass_leaves_the_deepconn_training_state():
    """Train, rank, continue == training never interrupted: weights, moments, offset, step_count, bit for bit."""
    from reviews4rec_amd import Catalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=52)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('deepconn', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = Catalogue(model, hp, reader, engine=engine, tower_batch=50)
            items = cat.eligible[np.arange(300) % len(cat.eligible)]
            ranks, sc = cat.rank(np.arange(300), items)
            assert (ranks >= 0).all() and torch.isfinite(sc).all() and model.training
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K


# ---------------------------------------------------------------- 9. main.main
@pytest.mark.parametrize('mt', ['MF_dot', 'deepconn'])
def test_main_reports_the_catalogue_metrics_of_the_trained_model(mt, tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import eval_catalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    meta, z = _fixture(mt, 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    hp = tiny_hp(mt, root, log_file=str(tmp_path / 'log'), model_path=str(tmp_path / 'model'), catalogue_metrics_k=[1, 5])
    final = M.main(hp)
    keys = {'cat_HR@1', 'cat_HR@5', 'cat_NDCG@1', 'cat_NDCG@5', 'cat_MRR', 'cat_ranked', 'cat_unranked'}
    assert keys <= set(final) and 'MSE' in final and not any(k.endswith('@10') for k in final)
    assert 'cat_MRR' in open(hp['log_file']).read()
    train, test, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(torch.load(hp['model_path'], map_location='cpu'))
    want = eval_catalogue(model.cuda().eval(), train, test, hp, ks=[1, 5])
    assert set(want) == keys and {k: final[k] for k in keys} == want
    assert want['cat_ranked'] + want['cat_unranked'] == len(test.data)
