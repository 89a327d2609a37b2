"""NARRE's catalogue on the device: r4r_topk_hmlp / r4r_pair_hmlp / r4r_rank_hmlp (csrc/topk_hmlp.hip, include/r4r.h
"Catalogue recommendation: product-MLP heads") and recommend.NarreCatalogue on top of them.

The reference ordering is test_gpu_recommend.py's (float64 scores, np.lexsort on (id, -score), the exclusions applied,
the -1 / -inf fill) over

    score(u, i) = sum_j w_j max(sum_m W[j][m] q[u][m] c[i][m] + b_j, 0) + c_bias[i] + q_bias[u]

With q, c, W, w multiples of 1/4 in [-1, 1] and b and the biases multiples of 1/64, every intermediate is exact in fp32
up to D = H = 64 (x in 1/16; y in 1/64, |y| <= 65; h in 1/256, |h| < 2^13), so the kernel must return EXACTLY that
list; with real-valued inputs the a-priori bound of test 4 decides what is demanded."""
import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from test_gpu_recommend import check_lists, dyadic, mask_excluded, ref_lists, small_chunk

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the reference scores
def _hidden(q, c, W):
    """y [n_q, n_c, H] in float64; a NaN anywhere in x makes every y of the pair NaN, as the fmaf chain does."""
    x = q.astype(np.float64)[:, None, :] * c.astype(np.float64)[None, :, :]
    with np.errstate(invalid='ignore'):
        y = x @ W.astype(np.float64).T
    y[np.isnan(x).any(-1)] = np.nan
    return x, y


def ref_scores(q, qb, c, cb, W, b, w, check_exact=False):
    """float64; fmaxf's NaN rule (a NaN hidden sum counts as 0), NaN in a bias propagates."""
    n_q, n_c, H = q.shape[0], c.shape[0], W.shape[0]
    s = np.zeros((n_q, n_c), np.float64)
    b64 = np.zeros(H) if b is None else b.astype(np.float64)
    for u0 in range(0, n_q, 8):                               # (8 queries at a time: [8, n_c, 64] float64 at most)
        x, y = _hidden(q[u0:u0 + 8], c, W)
        with np.errstate(invalid='ignore'):
            z = np.fmax(y + b64, 0.0)
        h = z @ w.astype(np.float64)
        if check_exact:
            absh = z @ np.abs(w.astype(np.float64))
            assert np.array_equal(x * 16, np.round(x * 16)) and np.array_equal(y * 64, np.round(y * 64))
            assert (np.abs(y + b64) <= 65).all() if H else True
            assert np.array_equal(h * 256, np.round(h * 256)) and (absh < 2 ** 13).all()
        s[u0:u0 + 8] = h
    if cb is not None:
        s = s + cb.astype(np.float64)[None, :]
    if qb is not None:
        s = s + qb.astype(np.float64)[:, None]
    return s


def hmlp_bound(q, qb, c, cb, W, b, w):
    """(D + H + 8) 2^-24 M[u][i], M = sum_j |w_j| (sum_m |W_jm| |q_m c_m| + |b_j|) + |c_bias| + |q_bias|: see test 4."""
    D, H = q.shape[1], W.shape[0]
    ax = np.abs(q.astype(np.float64))[:, None, :] * np.abs(c.astype(np.float64))[None, :, :]
    M = (ax @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))) @ np.abs(w.astype(np.float64))
    M = M + np.abs(cb.astype(np.float64))[None, :] + np.abs(qb.astype(np.float64))[:, None]
    return (D + H + 8) * EPS * M


# ---------------------------------------------------------------- the calls
def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # (a copy: the shared inputs are read-only)


class Tables:
    """The inputs on the device; c with a row stride of D + pad (the pad holds NaN)."""

    def __init__(self, q, qb, c, cb, W, b, w, pad=3):
        self.n_q, self.D = q.shape
        self.n_c, self.H = c.shape[0], W.shape[0]
        self.stride = self.D + pad
        self.c = torch.full((max(self.n_c, 1), max(self.stride, 1)), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.D:
            self.c[:self.n_c, :self.D] = _dev(c)
        self.q = _dev(q.reshape(-1) if self.D else np.zeros(1, np.float32))
        self.W = _dev(W.reshape(-1) if self.D * self.H else np.zeros(1, np.float32))
        self.w = _dev(w if self.H else np.zeros(1, np.float32))
        self.b = None if b is None else _dev(b if self.H else np.zeros(1, np.float32))
        self.qb, self.cb = _dev(qb), _dev(cb)

    def head(self):
        from reviews4rec_amd._lib import ptr
        return (ptr(self.q), self.n_q, ptr(self.qb), ptr(self.c), self.n_c, self.stride, ptr(self.cb), ptr(self.W),
                ptr(self.b), ptr(self.w), self.D, self.H)


def _excl(excl):
    if excl is None:
        return None, None
    return _dev(excl[0]), _dev(np.concatenate([excl[1], np.zeros(1, np.int64)]))


def topk(t, K, chunk=0, excl=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    eo, ei = _excl(excl)
    ids = torch.full((t.n_q, K), -7, dtype=torch.int64, device=DEV)
    sc = torch.full((t.n_q, K), 7.0, dtype=torch.float32, device=DEV)
    nb = _lib.lib().r4r_topk_hmlp_ws_bytes(t.n_q, t.n_c, K, chunk)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_topk_hmlp', *t.head(), ptr(eo), ptr(ei), K, chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def pairs(t, qi, ci):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    qd, cd = _dev(qi.astype(np.int64)), _dev(ci.astype(np.int64))
    out = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_pair_hmlp', *t.head(), ptr(qd), ptr(cd), len(qi), ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rank(t, qi, ti, chunk=0, excl=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    eo, ei = _excl(excl)
    qd, td = _dev(qi.astype(np.int64)), _dev(ti.astype(np.int64))
    r = torch.full((len(qi),), -7, dtype=torch.int64, device=DEV)
    s = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_rank_hmlp', *t.head(), ptr(qd), ptr(td), len(qi), ptr(eo), ptr(ei), chunk, ptr(r), ptr(s))
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy()


def exact_inputs(rng, n_q, n_c, D, H):
    q, c = dyadic(rng, (n_q, D), 0.25, 1.0), dyadic(rng, (n_c, D), 0.25, 1.0)
    W, w = dyadic(rng, (H, D), 0.25, 1.0), dyadic(rng, (H,), 0.25, 1.0)
    b = dyadic(rng, (H,), 1 / 64, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    return q, qb, c, cb, W, b, w


_REAL = {}


def real_inputs(D, H, n_q=33, n_c=4099, seed=None):
    """Standard-normal tables; the default shape is computed once and shared, never written to."""
    key = (D, H, n_q, n_c, seed)
    if key not in _REAL:
        rng = np.random.default_rng(17 * D + H if seed is None else seed)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        _REAL[key] = (f(n_q, D), (4 + f(n_q)).astype(np.float32), f(n_c, D), (0.3 * f(n_c)).astype(np.float32),
                      f(H, D), f(H), f(H))
        for a in _REAL[key]:
            a.setflags(write=False)
    return _REAL[key]


# ---------------------------------------------------------------- 1. exact arithmetic
N_Q, N_C = [1, 3, 4, 5, 15, 16, 17, 33, 65], [1, 15, 16, 17, 63, 64, 65, 257, 4099]
DS, HS, KS = [0, 1, 3, 4, 5, 6, 32, 33, 63, 64], [0, 1, 6, 15, 16, 17, 32, 48, 63, 64], [1, 5, 10, 128]
EXACT = sorted({(N_Q[t % 9], N_C[(2 * t) % 9], DS[t % 10], HS[(3 * t + t // 10) % 10], KS[t % 4]) for t in range(30)} |
               {(33, 4099, 64, 64, 128),   # the largest instantiation: 16 MFMAs over the width, four tiles of hidden units
                (1, 4099, 0, 0, 5),        # a pure bias ranking
                (17, 257, 0, 17, 10),      # no input width: z = max(b, 0)
                (16, 4099, 33, 0, 5),      # no hidden units
                (65, 4099, 6, 6, 10),      # tests/golden/tiny's shape; 16 query tiles and one row
                (5, 4099, 32, 32, 10),     # one query past the tile
                (4, 65, 63, 63, 5),        # the tile exactly; one column / one hidden unit below the limits
                (3, 64, 5, 17, 1),         # one query below the tile; a second tile of hidden units with one row
                (33, 257, 64, 48, 10),     # three tiles of hidden units (also run with NULL b and NULL biases)
                (17, 65, 8, 16, 5),        # D and H exactly at the smallest instantiation
                (15, 63, 9, 33, 128)})     # one past it in both


@pytest.mark.parametrize('n_q, n_c, D, H, K', EXACT)
def test_exact_inputs_give_the_reference_list_bit_for_bit(n_q, n_c, D, H, K):
    assert 38 <= len(EXACT) <= 44
    rng = np.random.default_rng(n_q * 1000003 + n_c * 131 + D * 7 + H * 1009 + K)
    q, qb, c, cb, W, b, w = exact_inputs(rng, n_q, n_c, D, H)
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb, W, b, w, check_exact=True), K)
    assert np.array_equal(want_sc.astype(np.float32).astype(np.float64), want_sc)     # exact in fp32
    t = Tables(q, qb, c, cb, W, b, w)                                                 # c_stride = D + 3, NaN in the pad
    for chunk in (0, small_chunk(n_c)):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (chunk, np.argwhere(ids != want_ids)[:5])
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk                  # (as floats: -0.0 == 0.0)
    if (n_q, n_c, D, H, K) == (33, 257, 64, 48, 10):                                  # NULL b and NULL biases count as 0
        ids, sc = topk(Tables(q, None, c, None, W, None, w, pad=0), K, small_chunk(n_c))
        want_ids, want_sc = ref_lists(ref_scores(q, None, c, None, W, None, w), K)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc.astype(np.float32))


# ---------------------------------------------------------------- 2. degenerate rankings, 3. exclusions
@pytest.mark.parametrize('case', ['all equal', 'K above the eligible count', 'every candidate -inf', 'NaN rows'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_q, n_c, D, H, K = 17, 300, 6, 5, 10
    q, qb, c, cb, W, b, w = exact_inputs(rng, n_q, n_c, D, H)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
        q[:] = q[:1]
    elif case == 'K above the eligible count':
        cb[rng.permutation(n_c)[7:]] = -np.inf                                       # seven eligible rows
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    else:
        c[41], c[42, 1] = np.nan, np.nan      # a NaN hidden sum counts as 0: the rows rank by their biases alone
        q[0, 1] = 0.0                         # (0 * NaN is NaN all the same)
        cb[41], cb[42] = 30.0, -30.0           # ... 41 on top of every list, 42 on none
        cb[43] = np.nan                       # through c_bias the row is dropped
    s = ref_scores(q, qb, c, cb, W, b, w)
    want_ids, want_sc = ref_lists(s, K)
    if case == 'all equal':
        assert (want_ids == np.arange(K)[None, :]).all()
    if case == 'K above the eligible count':
        assert (want_ids[:, 7:] == -1).all() and (want_ids[:, :7] >= 0).all()
    if case == 'every candidate -inf':
        assert (want_ids == -1).all()
    if case == 'NaN rows':
        assert np.array_equal(s[:, 41], 30.0 + qb.astype(np.float64)) and np.isnan(s[:, 43]).all()
        assert not np.isin(want_ids, [42, 43]).any() and (want_ids[:, 0] == 41).all()
    t = Tables(q, qb, c, cb, W, b, w)
    for chunk in (0, 64, 7):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (case, chunk)
        assert np.array_equal(sc, want_sc.astype(np.float32)), (case, chunk)


def test_exclusions():
    rng = np.random.default_rng(6)
    n_q, n_c, D, H, K = 5, 1000, 6, 5, 10
    q, qb, c, cb, W, b, w = exact_inputs(rng, n_q, n_c, D, H)
    s = ref_scores(q, qb, c, cb, W, b, w)
    free_ids, _ = ref_lists(s, K)
    lists = [np.zeros(0, np.int64),                                                  # an empty list
             free_ids[1, :1].copy(),                                                 # the would-be winner
             np.arange(n_c, dtype=np.int64),                                         # everything
             np.union1d(np.arange(64, 192), free_ids[3, :4]).astype(np.int64),       # empties the chunks [64, 128), [128, 192)
             np.sort(free_ids[4]).astype(np.int64)]                                  # the whole free top-K
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_ids, want_sc = ref_lists(mask_excluded(s, excl), K)
    assert np.array_equal(want_ids[0], free_ids[0]) and want_ids[1, 0] == free_ids[1, 1]
    assert (want_ids[2] == -1).all() and not np.isin(want_ids[3], lists[3]).any()
    assert not np.isin(want_ids[4], free_ids[4]).any()
    t = Tables(q, qb, c, cb, W, b, w)
    for chunk in (0, 64, 333):
        ids, sc = topk(t, K, chunk, excl=excl)
        assert np.array_equal(ids, want_ids), chunk
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
@pytest.mark.parametrize('D, H', [(6, 6), (32, 32), (64, 64)])
def test_real_valued_inputs_within_the_a_priori_bound(D, H):
    """The bound, to first order in eps = 2^-24 and relative to M[u][i] = sum_j |w_j| (sum_m |W_jm| |q_m c_m| + |b_j|) +
    |c_bias| + |q_bias|, which dominates every partial sum's magnitude:
      1           the rounding of x_m = q_m c_m, carried through |W_jm| into y_j
      D + 1       the D fmaf of the chain over m and the addition of b_j
      (ReLU is 1-Lipschitz: z_j inherits y_j's error and adds none)
      H / 4 + 2   the H / 4 fmaf of an h_g chain and the two levels of the tree (h_0 + h_1) + (h_2 + h_3)
      2           the additions of c_bias and q_bias
    together D + H / 4 + 6 <= D + H + 8 roundings."""
    K = 10
    q, qb, c, cb, W, b, w = real_inputs(D, H)
    s64 = ref_scores(q, qb, c, cb, W, b, w)
    tol = hmlp_bound(q, qb, c, cb, W, b, w)
    t = Tables(q, qb, c, cb, W, b, w)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(t, K, chunk)
        rows, got = np.nonzero(ids >= 0)[0], ids[ids >= 0]
        err = np.abs(sc[ids >= 0].astype(np.float64) - s64[rows, got]) / tol[rows, got]
        print('D=%d H=%d chunk=%d: worst |error| / bound over the lists = %.3f' % (D, H, chunk, float(err.max())))
        demanded = check_lists(ids, sc, s64, tol, K, 'D=%d H=%d chunk=%d' % (D, H, chunk))
        print('rows whose ids were demanded: %d of 33' % demanded)
        assert demanded >= 20, demanded


# ---------------------------------------------------------------- 5. the pair kernel
@pytest.mark.parametrize('D, H', [(0, 0), (3, 5), (6, 6), (32, 32), (33, 17), (64, 64)])
def test_pair_scores_have_the_bits_of_the_ranking(D, H):
    """The MFMA chain of the scan against the scalar chain of r4r_pair_hmlp, real-valued inputs, no tolerance."""
    K = 10
    # (against 65 candidates: 256 pairs fill the last 256-thread workgroup of the pair kernel exactly, 257 leave one pair
    # in it)
    for n_c, counts in ((4099, (33 * K,)), (65, (256, 257))):
        q, qb, c, cb, W, b, w = real_inputs(D, H, n_c=n_c)
        t = Tables(q, qb, c, cb, W, b, w)
        ids, sc = topk(t, K, 0)
        assert (ids >= 0).all()
        for n in counts:
            out = pairs(t, np.repeat(np.arange(33), K)[:n], ids.reshape(-1)[:n])
            assert np.array_equal(out.view(np.uint32), sc.reshape(-1)[:n].view(np.uint32)), (n_c, n)


# ---------------------------------------------------------------- 6. batching invariance
@pytest.mark.parametrize('D, H', [(6, 6), (64, 64)])
def test_batching_and_chunking_do_not_change_a_bit(D, H):
    K = 10
    q, qb, c, cb, W, b, w = real_inputs(D, H)
    rng = np.random.default_rng(H)
    lists = [np.sort(rng.permutation(4099)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(33)]
    off = np.zeros(34, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids_all = np.concatenate(lists)

    def sub(a, b_):
        return (off[a:b_ + 1] - off[a], ids_all[off[a]:off[b_]])

    def run(a, b_, chunk):
        return topk(Tables(q[a:b_], qb[a:b_], c, cb, W, b, w), K, chunk, excl=sub(a, b_))

    want = run(0, 33, 0)
    bits = lambda r: (r[0], r[1].view(np.uint32))
    for chunk in (500, small_chunk(4099)):
        got = run(0, 33, chunk)
        assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want))), chunk
    for chunk in (0, 500):
        halves = [run(a, b_, chunk) for a, b_ in ((0, 17), (17, 33))]
        singles = [run(u, u + 1, chunk) for u in range(33)]
        for parts in (halves, singles):
            got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
            assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want))), chunk


# ---------------------------------------------------------------- 7. ranks
def host_ranks(S, qi, ti, excl):
    """The count of candidates ahead of the target under the order, from the pair kernel's scores S [n_q, n_c]."""
    out = np.zeros(len(qi), np.int64)
    ids = np.arange(S.shape[1])
    for p, (u, t) in enumerate(zip(qi, ti)):
        st = S[u, t]
        if not st > -np.inf:
            out[p] = -1
            continue
        with np.errstate(invalid='ignore'):
            ok = S[u] > -np.inf
            if excl is not None:
                ok[excl[1][excl[0][u]:excl[0][u + 1]]] = False
            ok[t] = False
            out[p] = int((ok & ((S[u] > st) | ((S[u] == st) & (ids < t)))).sum())
    return out


@pytest.mark.parametrize('n_p, n_c, D, H', [(1, 65, 3, 5), (3, 257, 6, 6), (4, 65, 0, 5), (5, 4099, 6, 6), (17, 4099, 32, 32),
                                            (130, 65, 9, 17), (65, 4099, 64, 64), (17, 257, 5, 0),
                                            # the target kernel's last 256-thread workgroup exactly full / holding one pair
                                            (256, 65, 3, 5), (257, 65, 6, 6),
                                            # waves of the exclusion kernel's last workgroup without a pair (below)
                                            (5, 257, 6, 6)])
def test_ranks_are_the_count_of_candidates_ahead(n_p, n_c, D, H):
    rng = np.random.default_rng(700 + n_p + n_c + H)
    n_q = 9
    q, qb, c, cb, W, b, w = (a.copy() for a in real_inputs(D, H, n_q=n_q, n_c=n_c, seed=800 + n_p + D))
    c[5] = c[3]                                              # exact ties: rows 3 and 5 score alike for every query
    cb[5] = cb[3]
    cb[7] = -np.inf                                          # an ineligible row
    t = Tables(q, qb, c, cb, W, b, w)
    S = pairs(t, np.repeat(np.arange(n_q), n_c), np.tile(np.arange(n_c), n_q)).reshape(n_q, n_c)
    qi, ti = rng.integers(0, n_q, n_p), rng.integers(0, n_c, n_p)
    lists = [np.sort(rng.permutation(n_c)[:rng.integers(0, 50)]).astype(np.int64) for _ in range(n_q)]
    lists[0] = np.zeros(0, np.int64)
    if n_p >= 17:
        qi[:6], ti[:6] = [2, 2, 2, 4, 4, 1], [3, 5, 3, 7, 3, lists[1][0] if len(lists[1]) else 0]
        # (pairs sharing row 2, the pair (2, 3) twice, the tie partners 3 / 5, the -inf target 7, a target on its row's
        # exclusion list)
        lists[1] = np.union1d(lists[1], [ti[5]]).astype(np.int64)
    if (n_p, n_c) == (5, 257):
        # two lists of 100 ids (the lane loop of the exclusion kernel takes a second trip), one holding its pair's target
        qi[:2] = [1, 2]
        lists[1] = np.union1d(np.setdiff1d(rng.permutation(n_c), [ti[0]])[:99], [ti[0]]).astype(np.int64)
        lists[2] = np.sort(np.setdiff1d(rng.permutation(n_c), [ti[1]])[:100]).astype(np.int64)
        assert len(lists[1]) == len(lists[2]) == 100 and ti[0] in lists[1] and ti[1] not in lists[2]
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_score = S[qi, ti]
    for ex in (None, excl):
        want = host_ranks(S, qi, ti, ex)
        if n_p >= 17:
            assert want[3] == -1 and want[0] == want[2] and want[1] == want[0] + (0 if ex is not None and 3 in lists[2] else 1)
        for chunk in (0, 64, small_chunk(n_c)):
            r, s = rank(t, qi, ti, chunk, ex)
            assert np.array_equal(r, want), (ex is not None, chunk, np.argwhere(r != want)[:5])
            assert np.array_equal(s.view(np.uint32), want_score.view(np.uint32))


# ---------------------------------------------------------------- 7a. every dispatch class, lists and ranks
def test_every_dispatch_class_gives_the_reference_lists_and_ranks():
    """Both sides of every boundary of HMLP_DISPATCH crossed, each class through mfma_scan_kernel and
    mfma_rank_scan_kernel once per chunking: n_q = 5 is a full tile and a ragged one, n_c = 37 two full slabs and five
    rows; chunk 0 is one chunk, 16 three with the merge."""
    n_q, n_c, K = 5, 37, 3
    cases = []
    for D in (8, 9, 16, 17, 32, 33, 64):                      # every reference first: exact on the host, no device call
        for H in (16, 17, 32, 33, 48, 49, 64):
            inputs = exact_inputs(np.random.default_rng(D * 7 + H * 1009), n_q, n_c, D, H)
            S = ref_scores(*inputs, check_exact=True)
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S)         # exact in fp32
            cases.append((D, H, inputs, S))
    qi = np.arange(n_q)
    ti = qi % n_c
    for D, H, inputs, S in cases:
        want_ids, want_sc = ref_lists(S, K)
        want_rank = host_ranks(S, qi, ti, None)
        t = Tables(*inputs)
        for chunk in (0, 16):
            ids, sc = topk(t, K, chunk)
            assert np.array_equal(ids, want_ids), (D, H, chunk, np.argwhere(ids != want_ids)[:5])
            assert np.array_equal(sc.view(np.uint32), want_sc.astype(np.float32).view(np.uint32)), (D, H, chunk)
            r, rs = rank(t, qi, ti, chunk)
            assert np.array_equal(r, want_rank), (D, H, chunk, r, want_rank)
            assert np.array_equal(rs.view(np.uint32), S[qi, ti].astype(np.float32).view(np.uint32)), (D, H, chunk)


# ---------------------------------------------------------------- 8. NARRE on tests/golden/tiny
def _tiny(tmp_path):
    import reviews4rec_amd
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp('NARRE', root), device=DEV)
    W = _weights(_fixture('NARRE', 'e2e')[1], 'best/')
    model = reviews4rec_amd.get_model_class('NARRE')(hp)
    model.load_state_dict(W, strict=True)
    return hp, train, test, model.cuda().eval(), W


def test_narre_catalogue_on_tiny_against_the_oracle(tmp_path):
    import oracle
    from reviews4rec_amd import NarreCatalogue, eval_catalogue
    from reviews4rec_amd import main as M
    hp, train, test, model, W = _tiny(tmp_path)
    assert (hp['latent_size'], hp['narre_num_reviews'], hp['narre_num_words']) == (6, 10, 6)
    U, I, K = hp['total_users'], hp['total_items'], 5
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    none = np.full(len(u), -1, np.int64)
    data = [torch.from_numpy(np.ascontiguousarray(f)) for f in test._review_fields_host(u, i, none, none, none)]
    data = data + [torch.from_numpy(u), torch.from_numpy(i)]
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    cat = NarreCatalogue(model, hp, train)
    eligible = sorted({int(r[1]) for r in train.data})
    assert cat.eligible.tolist() == eligible and cat.c.shape == (I, 6) and cat.W.shape == (6, 6)
    # (a) score_pairs against the float64 oracle forward, within the project's eval tolerance
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    tol = 1e-5 + 1e-5 * np.abs(s64)
    el = np.zeros(I, bool)
    el[eligible] = True
    worst = float((np.abs(got[:, el] - s64[:, el]) / tol[:, el]).max())
    print('NARRE: score_pairs against the oracle, worst |difference| / tolerance = %.3f' % worst)
    assert (np.abs(got[:, el] - s64[:, el]) <= tol[:, el]).all(), worst
    assert np.isneginf(got[:, ~el]).all()
    # (b) ... and against the package's own forward and the native engine's predict on the same pairs
    dev_data = [d.to(DEV) for d in data]
    engine = M.make_engine(dict(hp, engine='native'), model)
    assert engine is not None and hasattr(engine, 'predict')
    with torch.no_grad():
        outs = [('forward', model(dev_data)),
                ('predict', torch.cat([engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone()
                                       for a in range(0, U * I, 96)]))]
        for name, out in outs:
            mine = out.reshape(U, I).cpu().numpy().astype(np.float64)
            worst = float((np.abs(got[:, el] - mine[:, el]) / tol[:, el]).max())
            print('NARRE: score_pairs against %s, worst |difference| / tolerance = %.3f' % (name, worst))
            assert (np.abs(got[:, el] - mine[:, el]) <= tol[:, el]).all(), (name, worst)
    # (c) the lists, (d) the ranks
    seen = {}
    for r in train.data:
        seen.setdefault(int(r[0]), set()).add(int(r[1]))
    users = np.arange(U, dtype=np.int64)
    for exclude in (True, False):
        ids, sc = cat.recommend(users, k=K, exclude_seen=exclude)
        assert ids.device.type == 'cuda' and ids.dtype == torch.int64 and sc.dtype == torch.float32
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        masked = np.where(el[None, :], s64, -np.inf)
        if exclude:
            for uu, items in seen.items():
                masked[uu, sorted(items)] = -np.inf
        check_lists(ids, sc, masked, tol, K, 'NARRE exclude=%s' % exclude)
        assert np.isin(ids[ids >= 0], eligible).all()
        if exclude:
            assert not any(int(x) in seen.get(uu, ()) for uu in range(U) for x in ids[uu])
        flat = ids.reshape(-1)
        again = cat.score_pairs(np.repeat(users, K)[flat >= 0], flat[flat >= 0]).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), sc.reshape(-1)[flat >= 0].view(np.uint32))
        # the rank of an item is its position in the whole list, wherever the list holds it
        full, fsc = cat.recommend(users, k=128, exclude_seen=exclude)
        ranks, rsc = cat.rank(u, i, exclude_seen=exclude)
        assert ranks.device.type == 'cuda' and ranks.dtype == torch.int64 and rsc.dtype == torch.float32
        full, ranks = full.cpu().numpy(), ranks.cpu().numpy().reshape(U, I)
        assert np.array_equal(rsc.cpu().numpy().view(np.uint32), got.reshape(-1).view(np.uint32))
        assert (ranks[:, ~el] == -1).all() and (ranks[:, el] >= 0).all()
        held = 0
        for uu in range(U):
            for pos, item in enumerate(full[uu]):
                if item >= 0:
                    assert ranks[uu, item] == pos, (uu, item, pos)
                    held += 1
        assert held >= U
    # candidates= overrides the default set; tower_batch= only batches the refresh
    few = NarreCatalogue(model, hp, train, candidates=np.array(eligible[:3]))
    ids, _ = few.recommend(users[:4], k=K, exclude_seen=False)
    assert sorted(ids[0].cpu().tolist()) == [-1, -1] + eligible[:3]
    small = NarreCatalogue(model, hp, train, tower_batch=5)
    assert torch.equal(small.c, cat.c) and torch.equal(small.c_bias, cat.c_bias)
    assert torch.equal(small.score_pairs(u, i), cat.score_pairs(u, i))
    # ids may arrive as a device tensor
    a = cat.recommend(torch.from_numpy(users).to(DEV), k=K)
    b = cat.recommend(users.tolist(), k=K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        cat.recommend(users, k=129)
    with pytest.raises(ValueError):
        cat.score_pairs(users[:2], users[:3])
    with pytest.raises(ValueError):
        cat.rank(users[:2], users[:3])
    # the full-catalogue metrics go through the class
    m = eval_catalogue(model, train, test, hp, ks=[1, 5], catalogue=cat)
    assert set(m) == {'cat_HR@1', 'cat_HR@5', 'cat_NDCG@1', 'cat_NDCG@5', 'cat_MRR', 'cat_ranked', 'cat_unranked'}
    assert m['cat_ranked'] + m['cat_unranked'] == len(test.data) and m['cat_ranked'] > 0


# ---------------------------------------------------------------- 9. training state
def test_a_recommend_pass_leaves_the_narre_training_state():
    """Train, recommend and rank, continue == training never interrupted: weights, moments, offset, step_count, bit for
    bit (dropout 0.5: a moved stream would show)."""
    from reviews4rec_amd import NarreCatalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=53)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('NARRE', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = NarreCatalogue(model, hp, reader, engine=engine, tower_batch=50)
            ids, sc = cat.recommend(np.arange(300), k=5)
            assert (ids[:, 0] >= 0).all() and torch.isfinite(sc[:, 0]).all() and model.training
            items = cat.eligible[np.arange(300) % len(cat.eligible)]
            ranks, rs = cat.rank(np.arange(300), items)
            assert (ranks >= 0).all() and torch.isfinite(rs).all() and model.training
            again = cat.score_pairs(np.arange(300), items)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), rs.cpu().numpy().view(np.uint32))
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K


def test_the_engine_is_flushed_before_the_cache_is_read(monkeypatch):
    """refresh() brings an engine's pending updates in (flush(), where the engine has one) before it reads a weight."""
    from reviews4rec_amd import NarreCatalogue, ops
    from test_gpu_span import build, tiny_corpus
    hp, reader, model, engine = build('NARRE', tiny_corpus(seed=54))
    order = []
    inner = ops.narre_attention
    monkeypatch.setattr(ops, 'narre_attention', lambda *a, **k: (order.append('read'), inner(*a, **k))[1])

    class Flushing:
        def flush(self):
            order.append('flush')

    cat = NarreCatalogue(model.eval(), hp, reader, engine=Flushing())
    assert order[0] == 'flush' and order.count('flush') == 1 and 'read' in order
    del order[:]
    cat.refresh()
    assert order[0] == 'flush' and order.count('flush') == 1 and 'read' in order
    del order[:]
    NarreCatalogue(model, hp, reader, engine=engine)          # NARRE's own engine keeps no update pending: nothing to call
    assert 'flush' not in order and 'read' in order
