"""The TransNets' catalogue on the device: r4r_topk_rfm / r4r_pair_rfm / r4r_rank_rfm (csrc/topk_rfm.hip, include/r4r.h
"Catalogue recommendation: ReLU-FM heads") and recommend.TransNetCatalogue on top of them.

The reference ordering is test_gpu_recommend.py's (float64 scores, np.lexsort on (id, -score), the exclusions applied,
the -1 / -inf fill) over

    x_m = max(q[u][m] + c[i][m], 0)  m < H,   x_m = q[u][m] + c[i][m]  H <= m < H + P,   y = W x + b
    score(u, i) = sum_j y_j (s_j y_j + l_j) + c_bias[i] + q_bias[u]

With q and c multiples of 1/2 in [-1/2, 1/2], W multiples of 1/2 in [-1, 1] with at most 8 non-zeros per row, b multiples
of 1/4 in [-1, 1], s in {1/2, -1/2, 0}, l in {0, 1} and the biases multiples of 1/64, every intermediate is exact in fp32
up to (H, P, M) = (64, 16, 80): x in 1/2, |x| <= 1; y in 1/4, |y| <= 9; e y in 1/32, |e y| <= 50; 80 of them stay below
2^12 at 1/32.  So the kernel must return EXACTLY that list; with real-valued inputs the a-priori bound of test 4 decides
what is demanded."""
import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from test_gpu_recommend import check_lists, dyadic, mask_excluded, ref_lists, small_chunk

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the reference scores
def _inputs(q, c, H, split=False):
    """x [n_q, n_c, D] in float64: fmaxf's NaN rule on the first H columns (a NaN sum counts as 0), plain behind them.
    split: |q| + |c| in place of |x| (what bounds the rounding of the TABLES, which the sum may cancel)."""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    if split:
        return np.abs(q64)[:, None, :] + np.abs(c64)[None, :, :]
    x = q64[:, None, :] + c64[None, :, :]
    with np.errstate(invalid='ignore'):
        x[..., :H] = np.fmax(x[..., :H], 0.0)
    return x


def ref_scores(q, qb, c, cb, W, b, s, l, H, check_exact=False):
    """float64; a NaN in a plain column or in a bias propagates (every y of the pair is NaN, as the fmaf chain's)."""
    n_q, n_c, M = q.shape[0], c.shape[0], W.shape[0]
    out = np.zeros((n_q, n_c), np.float64)
    b64 = np.zeros(M) if b is None else b.astype(np.float64)
    W64, s64, l64 = W.astype(np.float64), s.astype(np.float64), l.astype(np.float64)
    for u0 in range(0, n_q, 8):                               # (8 queries at a time: [8, n_c, 80] float64 at most)
        x = _inputs(q[u0:u0 + 8], c, H)
        bad = np.isnan(x).any(-1)
        with np.errstate(invalid='ignore'):
            y = np.where(bad[..., None], 0.0, np.nan_to_num(x) @ W64.T) + b64
            term = y * (s64 * y + l64)
        if check_exact:
            assert np.array_equal(x * 2, np.round(x * 2)) and (np.abs(x) <= 1).all()
            assert np.array_equal(y * 4, np.round(y * 4)) and (np.abs(y) <= 9).all()
            assert np.array_equal(term * 32, np.round(term * 32)) and (np.abs(term) <= 50).all()
        t = term.sum(-1)
        if M:
            t[bad] = np.nan
        out[u0:u0 + 8] = t
    with np.errstate(invalid='ignore'):
        if cb is not None:
            out = out + cb.astype(np.float64)[None, :]
        if qb is not None:
            out = out + qb.astype(np.float64)[:, None]
    return out


def rfm_bound(q, qb, c, cb, W, b, s, l, H, fold=False):
    """(2 D + M + 16) 2^-24 Mag[u][i], Mag = sum_j (|s_j| Y_j^2 + |l_j| Y_j) + |c_bias| + |q_bias|, Y_j = sum_m |W_jm| |x_m|
    + |b_j|: see test 4.  fold: the tables are themselves one rounding of float64 numbers (test 8) -- |x_m| becomes
    |q_m| + |c_m| (the sum may cancel what was rounded) and four roundings are added: each y_j carries 2 more (W and x, or
    b), and y_j enters its term twice."""
    D, M = q.shape[1], W.shape[0]
    mag = np.zeros((q.shape[0], c.shape[0]), np.float64)
    for u0 in range(0, q.shape[0], 8):
        Y = np.abs(_inputs(q[u0:u0 + 8], c, H, split=fold)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))
        mag[u0:u0 + 8] = (np.abs(s.astype(np.float64)) * Y * Y + np.abs(l.astype(np.float64)) * Y).sum(-1)
    mag = mag + np.abs(cb.astype(np.float64))[None, :] + np.abs(qb.astype(np.float64))[:, None]
    return (2 * D + M + 16 + (4 if fold else 0)) * EPS * mag


# ---------------------------------------------------------------- the calls
def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # (a copy: the shared inputs are read-only)


class Tables:
    """The inputs on the device; c with a row stride of D + pad (the pad holds NaN)."""

    def __init__(self, q, qb, c, cb, W, b, s, l, H, pad=3):
        self.n_q, self.D = q.shape
        self.n_c, self.M = c.shape[0], W.shape[0]
        self.H, self.P = H, self.D - H
        self.stride = self.D + pad
        self.c = torch.full((max(self.n_c, 1), max(self.stride, 1)), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.D:
            self.c[:self.n_c, :self.D] = _dev(c)
        self.q = _dev(q.reshape(-1) if self.D else np.zeros(1, np.float32))
        self.W = _dev(W.reshape(-1) if self.D * self.M else np.zeros(1, np.float32))
        self.s = _dev(s if self.M else np.zeros(1, np.float32))
        self.l = _dev(l if self.M else np.zeros(1, np.float32))
        self.b = None if b is None else _dev(b if self.M else np.zeros(1, np.float32))
        self.qb, self.cb = _dev(qb), _dev(cb)

    def head(self):
        from reviews4rec_amd._lib import ptr
        return (ptr(self.q), self.n_q, ptr(self.qb), ptr(self.c), self.n_c, self.stride, ptr(self.cb), ptr(self.W),
                ptr(self.b), ptr(self.s), ptr(self.l), self.H, self.P, self.M)


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
    nb = _lib.lib().r4r_topk_rfm_ws_bytes(t.n_q, t.n_c, K, chunk)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_topk_rfm', *t.head(), ptr(eo), ptr(ei), K, chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def pairs(t, qi, ci):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    qd, cd = _dev(qi.astype(np.int64)), _dev(ci.astype(np.int64))
    out = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_pair_rfm', *t.head(), ptr(qd), ptr(cd), len(qi), ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rank(t, qi, ti, chunk=0, excl=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    eo, ei = _excl(excl)
    qd, td = _dev(qi.astype(np.int64)), _dev(ti.astype(np.int64))
    r = torch.full((len(qi),), -7, dtype=torch.int64, device=DEV)
    s = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_rank_rfm', *t.head(), ptr(qd), ptr(td), len(qi), ptr(eo), ptr(ei), chunk, ptr(r), ptr(s))
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy()


def exact_inputs(rng, n_q, n_c, H, P, M):
    """-> (q, qb, c, cb, W, b, s, l) within the module docstring's grid."""
    D = H + P
    q, c = dyadic(rng, (n_q, D), 0.5, 0.5), dyadic(rng, (n_c, D), 0.5, 0.5)
    W = np.zeros((M, D), np.float32)
    for j in range(M):                                        # at most 8 non-zeros per row
        cols = rng.permutation(D)[:8]
        W[j, cols] = dyadic(rng, (len(cols),), 0.5, 1.0)
    b = dyadic(rng, (M,), 0.25, 1.0)
    s = rng.choice(np.array([0.5, -0.5, 0.0], np.float32), size=M)
    l = rng.choice(np.array([0.0, 1.0], np.float32), size=M)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    return q, qb, c, cb, W, b, s, l


_REAL = {}


def real_inputs(H, P, M, n_q=33, n_c=4099, seed=7, gain=1.0, spread=0.3):
    """Standard-normal tables and a head laid out as fold_transnet_head's (eight rows at s = +1/2, then s = -1/2, a last
    row at l = 1), rows of W of norm about ``gain``, candidate biases of deviation ``spread``; computed once per key and
    shared, never written to."""
    key = (H, P, M, n_q, n_c, seed, gain, spread)
    if key not in _REAL:
        D = H + P
        rng = np.random.default_rng(seed)
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
        s = np.zeros(M, np.float32)
        s[:min(8, M)], s[8:max(M - 1, 8)] = 0.5, -0.5
        l = np.zeros(M, np.float32)
        l[M - 1:] = 1.0
        _REAL[key] = (f(n_q, D), (4 + f(n_q)).astype(np.float32), f(n_c, D), (spread * f(n_c)).astype(np.float32),
                      (f(M, D) * (gain / np.sqrt(max(D, 1)))).astype(np.float32), (0.1 * f(M)).astype(np.float32), s, l)
        for a in _REAL[key]:
            a.setflags(write=False)
    return _REAL[key]


# ---------------------------------------------------------------- 1. exact arithmetic
# (a wave holds 4 queries, 2 in the instantiations with H + P > 40 and M > 32: n_q on both sides of both)
N_Q, N_C = [1, 2, 3, 4, 5, 15, 16, 17, 33], [1, 15, 16, 17, 63, 64, 65, 257, 4099]
HS, PS, MS, KS = [0, 1, 3, 4, 5, 6, 32, 33, 63, 64], [0, 1, 8, 16], [0, 1, 15, 16, 17, 73, 79, 80], [1, 5, 10, 128]
EXACT = sorted({(N_Q[t % 9], N_C[(2 * t) % 9], HS[t % 10], PS[(t + t // 4) % 4], MS[(3 * t + t // 8) % 8], KS[t % 4])
                for t in range(28)} |
               {(33, 4099, 64, 16, 80, 128),  # the largest instantiation: 20 MFMAs over the width, five row tiles
                (65, 4099, 6, 0, 15, 10),     # transnet on tests/golden/tiny; 17 query tiles
                (17, 257, 6, 8, 15, 10),      # transnet++ on tests/golden/tiny
                (5, 4099, 64, 8, 73, 10),     # transnet++ at the engine's limit: two queries per wave, one past two tiles
                (3, 65, 64, 0, 73, 5),        # transnet at the limit: one query past the tile of two
                (2, 64, 63, 16, 79, 1),       # the tile of two exactly; the ReLU / plain split inside MFMA step 15
                (1, 4099, 0, 0, 0, 5),        # a pure bias ranking
                (17, 257, 0, 0, 17, 10),      # no input width: y = b
                (16, 4099, 33, 1, 0, 5),      # no rows: the biases alone
                (4, 65, 0, 16, 16, 5),        # plain columns only: no ReLU
                (33, 257, 32, 8, 41, 10),     # three row tiles (also run with NULL b and NULL biases)
                (17, 65, 8, 0, 16, 5),        # D and M exactly at the smallest instantiation
                (15, 63, 5, 4, 33, 128),      # one past it in both; the split inside MFMA step 1
                (5, 257, 36, 4, 80, 10)})     # D = 40: the widest instantiation that still holds four queries


@pytest.mark.parametrize('n_q, n_c, H, P, M, K', EXACT)
def test_exact_inputs_give_the_reference_list_bit_for_bit(n_q, n_c, H, P, M, K):
    assert 38 <= len(EXACT) <= 44
    rng = np.random.default_rng(n_q * 1000003 + n_c * 131 + H * 7 + P * 3001 + M * 1009 + K)
    q, qb, c, cb, W, b, s, l = exact_inputs(rng, n_q, n_c, H, P, M)
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb, W, b, s, l, H, check_exact=True), K)
    assert np.array_equal(want_sc.astype(np.float32).astype(np.float64), want_sc)     # exact in fp32
    t = Tables(q, qb, c, cb, W, b, s, l, H)                                           # c_stride = D + 3, NaN in the pad
    for chunk in (0, small_chunk(n_c)):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (chunk, np.argwhere(ids != want_ids)[:5])
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk                  # (as floats: -0.0 == 0.0)
    if (n_q, n_c, H, P, M, K) == (33, 257, 32, 8, 41, 10):                            # NULL b and NULL biases count as 0
        ids, sc = topk(Tables(q, None, c, None, W, None, s, l, H, pad=0), K, small_chunk(n_c))
        want_ids, want_sc = ref_lists(ref_scores(q, None, c, None, W, None, s, l, H), K)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc.astype(np.float32))


# ---------------------------------------------------------------- 2. degenerate rankings, 3. exclusions
@pytest.mark.parametrize('case', ['all equal', 'K above the eligible count', 'every candidate -inf', 'NaN rows'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_q, n_c, H, P, M, K = 17, 300, 6, 8, 15, 10
    q, qb, c, cb, W, b, s, l = exact_inputs(rng, n_q, n_c, H, P, M)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
        q[:] = q[:1]
    elif case == 'K above the eligible count':
        cb[rng.permutation(n_c)[7:]] = -np.inf                                       # seven eligible rows
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    else:
        c[41], c[42, H + 2] = np.nan, np.nan  # a NaN propagates: y is NaN, the score is NaN, the row is on no list
        cb[41], cb[42] = 30.0, 30.0           # ... whatever its bias
        cb[43] = np.nan                       # through c_bias the row is dropped as well
        c[44, 1], cb[44] = np.nan, 1000.0      # under the ReLU alone fmaxf takes a NaN sum as 0: the row stays, on top
    sc64 = ref_scores(q, qb, c, cb, W, b, s, l, H)
    want_ids, want_sc = ref_lists(sc64, K)
    if case == 'all equal':
        assert (want_ids == np.arange(K)[None, :]).all()
    if case == 'K above the eligible count':
        assert (want_ids[:, 7:] == -1).all() and (want_ids[:, :7] >= 0).all()
    if case == 'every candidate -inf':
        assert (want_ids == -1).all()
    if case == 'NaN rows':
        assert np.isnan(sc64[:, [41, 42, 43]]).all() and np.isfinite(sc64[:, 44]).all()
        assert not np.isin(want_ids, [41, 42, 43]).any() and (want_ids[:, 0] == 44).all()
    t = Tables(q, qb, c, cb, W, b, s, l, H)
    for chunk in (0, 64, 7):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (case, chunk)
        assert np.array_equal(sc, want_sc.astype(np.float32)), (case, chunk)
    if case == 'NaN rows':                                    # ... and its rank is -1; it is ahead of nobody
        qi, ti = np.arange(8) % n_q, np.array([41, 42, 43, 44, 0, 41, 42, 44])
        S = pairs(t, np.repeat(np.arange(n_q), n_c), np.tile(np.arange(n_c), n_q)).reshape(n_q, n_c)
        assert np.isnan(S[:, [41, 42, 43]]).all()
        for chunk in (0, 64, 7):
            r, _ = rank(t, qi, ti, chunk)
            assert np.array_equal(r, host_ranks(S, qi, ti, None)), chunk
            assert r[[0, 1, 2, 5, 6]].tolist() == [-1] * 5 and r[3] == r[7] == 0 and r[4] >= 1


def test_exclusions():
    rng = np.random.default_rng(6)
    n_q, n_c, H, P, M, K = 5, 1000, 6, 8, 15, 10
    q, qb, c, cb, W, b, s, l = exact_inputs(rng, n_q, n_c, H, P, M)
    sc64 = ref_scores(q, qb, c, cb, W, b, s, l, H)
    free_ids, _ = ref_lists(sc64, K)
    lists = [np.zeros(0, np.int64),                                                  # an empty list
             free_ids[1, :1].copy(),                                                 # the would-be winner
             np.arange(n_c, dtype=np.int64),                                         # everything
             np.union1d(np.arange(64, 192), free_ids[3, :4]).astype(np.int64),       # empties the chunks [64, 128), [128, 192)
             np.sort(free_ids[4]).astype(np.int64)]                                  # the whole free top-K
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_ids, want_sc = ref_lists(mask_excluded(sc64, excl), K)
    assert np.array_equal(want_ids[0], free_ids[0]) and want_ids[1, 0] == free_ids[1, 1]
    assert (want_ids[2] == -1).all() and not np.isin(want_ids[3], lists[3]).any()
    assert not np.isin(want_ids[4], free_ids[4]).any()
    t = Tables(q, qb, c, cb, W, b, s, l, H)
    for chunk in (0, 64, 333):
        ids, sc = topk(t, K, chunk, excl=excl)
        assert np.array_equal(ids, want_ids), chunk
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
SHAPES = [(6, 8, 15), (32, 0, 41), (64, 8, 73)]


@pytest.mark.parametrize('H, P, M', SHAPES)
def test_real_valued_inputs_within_the_a_priori_bound(H, P, M):
    """The bound, to first order in eps = 2^-24 and relative to Mag[u][i] = sum_j (|s_j| Y_j^2 + |l_j| Y_j) + |c_bias| +
    |q_bias| with Y_j = sum_m |W_jm| |x_m| + |b_j|, which dominates every partial sum's magnitude.  With D = H + P and
    T_j = |s_j| Y_j^2 + |l_j| Y_j:
      y_j        1 (the rounding of x_m = q_m + c_m, carried through |W_jm|; the ReLU is 1-Lipschitz and maps 0 to 0, so
                 x_m keeps its RELATIVE error) + D (the fmaf chain over m) + 1 (the addition of b_j): (D + 2) eps Y_j
      e_j        = s_j y_j + l_j inherits |s_j| (D + 2) eps Y_j and adds one rounding of at most eps (|s_j| Y_j + |l_j|)
      e_j y_j    |e_j| dy_j + |y_j| de_j <= (D + 2) eps T_j + (D + 2) eps |s_j| Y_j^2 + eps T_j <= (2 D + 5) eps T_j;
                 its own rounding is the fmaf of the t_g chain
      the sum    at most 20 fmaf of a t_g chain (M <= 80: five tiles of four rows per lane group), the two levels of the
                 tree (t_0 + t_1) + (t_2 + t_3) and the additions of c_bias and q_bias: M / 4 + 8 roundings at most, each
                 relative to a partial sum that Mag dominates
    together (2 D + 5) + (M / 4 + 8) <= 2 D + M + 16 roundings.
    Mag sums 8 + L squares of opposite signs, so at L = 64 the bound is wide against the gaps between ten neighbours out
    of 4099 wherever the squares decide the order: the float64 reference alone, on the host, demands the ids of 4 to 10 rows
    of 33 with rows of W of norm 1 and candidate biases of deviation 0.3 (the inputs of tests 5 to 7), and of 22 to 33
    over seeds 0 .. 7 with norm 1/4 and deviation 3; seed 7 gives 33, 33 and 33 at the three shapes."""
    K = 10
    q, qb, c, cb, W, b, s, l = real_inputs(H, P, M, gain=0.25, spread=3.0)
    s64 = ref_scores(q, qb, c, cb, W, b, s, l, H)
    tol = rfm_bound(q, qb, c, cb, W, b, s, l, H)
    t = Tables(q, qb, c, cb, W, b, s, l, H)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(t, K, chunk)
        rows, got = np.nonzero(ids >= 0)[0], ids[ids >= 0]
        err = np.abs(sc[ids >= 0].astype(np.float64) - s64[rows, got]) / tol[rows, got]
        print('H=%d P=%d M=%d chunk=%d: worst |error| / bound over the lists = %.3f' % (H, P, M, chunk, float(err.max())))
        demanded = check_lists(ids, sc, s64, tol, K, 'H=%d P=%d M=%d chunk=%d' % (H, P, M, chunk))
        print('rows whose ids were demanded: %d of 33' % demanded)
        assert demanded >= 20, demanded
    # the inputs of tests 5 to 7 (rows of W of norm 1, candidate biases of deviation 0.3): here the squares decide the
    # order, the same bound holds for every score and every list must be valid under it; how many rows have their ids
    # demanded is printed, not capped (4 to 10 of 33 at L = 64, see above)
    a = real_inputs(H, P, M)
    s64, tol = ref_scores(*a, H), rfm_bound(*a, H)
    ids, sc = topk(Tables(*a, H), K, small_chunk(4099))
    rows, got = np.nonzero(ids >= 0)[0], ids[ids >= 0]
    err = np.abs(sc[ids >= 0].astype(np.float64) - s64[rows, got]) / tol[rows, got]
    demanded = check_lists(ids, sc, s64, tol, K, 'H=%d P=%d M=%d, norm 1' % (H, P, M))
    print('H=%d P=%d M=%d, rows of W of norm 1: worst |error| / bound over the lists = %.3f, rows whose ids were demanded: '
          '%d of 33' % (H, P, M, float(err.max()), demanded))


# ---------------------------------------------------------------- 5. the pair kernel
@pytest.mark.parametrize('H, P, M', [(0, 0, 0), (3, 2, 5), (6, 0, 15), (6, 8, 15), (32, 0, 41), (33, 3, 17), (64, 8, 73),
                                     (64, 16, 80)])
def test_pair_scores_have_the_bits_of_the_ranking(H, P, M):
    """The MFMA chain of the scan against the scalar chain of r4r_pair_rfm, real-valued inputs, no tolerance."""
    K = 10
    # (against 65 candidates: 256 pairs fill the last 256-thread workgroup of the pair kernel exactly, 257 leave one pair
    # in it)
    for n_c, counts in ((4099, (33 * K,)), (65, (256, 257))):
        q, qb, c, cb, W, b, s, l = real_inputs(H, P, M, n_c=n_c)
        t = Tables(q, qb, c, cb, W, b, s, l, H)
        ids, sc = topk(t, K, 0)
        assert (ids >= 0).all()
        for n in counts:
            out = pairs(t, np.repeat(np.arange(33), K)[:n], ids.reshape(-1)[:n])
            assert np.array_equal(out.view(np.uint32), sc.reshape(-1)[:n].view(np.uint32)), (n_c, n)


# ---------------------------------------------------------------- 6. batching invariance
@pytest.mark.parametrize('H, P, M', [(6, 8, 15), (64, 8, 73)])
def test_batching_and_chunking_do_not_change_a_bit(H, P, M):
    K = 10
    q, qb, c, cb, W, b, s, l = real_inputs(H, P, M)
    rng = np.random.default_rng(M)
    lists = [np.sort(rng.permutation(4099)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(33)]
    off = np.zeros(34, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids_all = np.concatenate(lists)

    def sub(a, b_):
        return (off[a:b_ + 1] - off[a], ids_all[off[a]:off[b_]])

    def run(a, b_, chunk):
        return topk(Tables(q[a:b_], qb[a:b_], c, cb, W, b, s, l, H), K, chunk, excl=sub(a, b_))

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


@pytest.mark.parametrize('n_p, n_c, H, P, M', [(1, 65, 3, 2, 5), (3, 257, 6, 0, 15), (4, 65, 0, 0, 5), (5, 4099, 6, 8, 15),
                                               (17, 4099, 32, 0, 41), (130, 65, 9, 3, 17), (65, 4099, 64, 8, 73),
                                               (17, 257, 5, 1, 0), (33, 257, 64, 16, 80),
                                               # the target kernel's last 256-thread workgroup exactly full / holding one pair
                                               (256, 65, 3, 2, 5), (257, 65, 6, 8, 15),
                                               # waves of the exclusion kernel's last workgroup without a pair (below)
                                               (5, 257, 6, 8, 15)])
def test_ranks_are_the_count_of_candidates_ahead(n_p, n_c, H, P, M):
    rng = np.random.default_rng(700 + n_p + n_c + M)
    n_q = 9
    q, qb, c, cb, W, b, s, l = (a.copy() for a in real_inputs(H, P, M, n_q=n_q, n_c=n_c, seed=800 + n_p + H))
    c[5] = c[3]                                              # exact ties: rows 3 and 5 score alike for every query
    cb[5] = cb[3]
    cb[7] = -np.inf                                          # an ineligible row
    t = Tables(q, qb, c, cb, W, b, s, l, H)
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
    np.cumsum([len(x) for x in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_score = S[qi, ti]
    for ex in (None, excl):
        want = host_ranks(S, qi, ti, ex)
        if n_p >= 17:
            assert want[3] == -1 and want[0] == want[2] and want[1] == want[0] + (0 if ex is not None and 3 in lists[2] else 1)
        for chunk in (0, 64, small_chunk(n_c)):
            r, sc = rank(t, qi, ti, chunk, ex)
            assert np.array_equal(r, want), (ex is not None, chunk, np.argwhere(r != want)[:5])
            assert np.array_equal(sc.view(np.uint32), want_score.view(np.uint32))


# ---------------------------------------------------------------- 7a. every dispatch class, lists and ranks
def test_every_dispatch_class_gives_the_reference_lists_and_ranks():
    """Both sides of every rfm_kt / rfm_mt boundary crossed (the classes with two queries per wave among them), each
    through mfma_scan_kernel and mfma_rank_scan_kernel once per chunking: n_q = 5 is a full tile and a ragged one at
    either tile width, n_c = 37 two full slabs and five rows; chunk 0 is one chunk, 16 three with the merge."""
    n_q, n_c, K = 5, 37, 3
    shapes = [(min(D, 64), D - min(D, 64), M) for D in (8, 9, 16, 17, 40, 41, 80) for M in (16, 17, 32, 33, 48, 49, 80)]
    cases = []
    for H, P, M in shapes:                                    # every reference first: exact on the host, no device call
        inputs = exact_inputs(np.random.default_rng(H * 7 + P * 3001 + M * 1009), n_q, n_c, H, P, M)
        S = ref_scores(*inputs, H, check_exact=True)
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)             # exact in fp32
        cases.append((H, P, M, inputs, S))
    qi = np.arange(n_q)
    ti = qi % n_c
    for H, P, M, inputs, S in cases:
        want_ids, want_sc = ref_lists(S, K)
        want_rank = host_ranks(S, qi, ti, None)
        t = Tables(*inputs, H)
        for chunk in (0, 16):
            ids, sc = topk(t, K, chunk)
            assert np.array_equal(ids, want_ids), (H, P, M, chunk, np.argwhere(ids != want_ids)[:5])
            assert np.array_equal(sc.view(np.uint32), want_sc.astype(np.float32).view(np.uint32)), (H, P, M, chunk)
            r, rs = rank(t, qi, ti, chunk)
            assert np.array_equal(r, want_rank), (H, P, M, chunk, r, want_rank)
            assert np.array_equal(rs.view(np.uint32), S[qi, ti].astype(np.float32).view(np.uint32)), (H, P, M, chunk)


# ---------------------------------------------------------------- 8. both TransNets on tests/golden/tiny
def _tiny(mt, tmp_path):
    import reviews4rec_amd
    from reviews4rec_amd.data import load_data
    from test_transnet_catalogue_host import tiny_weights
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(dict(tiny_hp('transnet++', root), model_type=mt), device=DEV)
    W = tiny_weights(mt)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(W, strict=True)
    return hp, train, test, model.cuda().eval(), W


@pytest.mark.parametrize('mt', ['transnet', 'transnet++'])
def test_transnet_catalogue_on_tiny_against_the_oracle(mt, tmp_path):
    import oracle
    from reviews4rec_amd import TransNetCatalogue, eval_catalogue
    from reviews4rec_amd import main as M
    from test_transnet_catalogue_host import all_pairs
    hp, train, test, model, W = _tiny(mt, tmp_path)
    assert hp['latent_size'] == 6
    U, I, K = hp['total_users'], hp['total_items'], 5
    u, i, data = all_pairs(hp, test)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp)[0].numpy().astype(np.float64).reshape(U, I)
    cat = TransNetCatalogue(model, hp, train)
    eligible = sorted({int(r[1]) for r in train.data})
    H, P, Mr = 6, (8 if mt == 'transnet++' else 0), 15
    assert cat.eligible.tolist() == eligible and cat.c.shape == (I, H + P) and cat.W.shape == (Mr, H + P)
    assert (cat.H, cat.P, cat.M) == (H, P, Mr)
    el = np.zeros(I, bool)
    el[eligible] = True
    # (a) score_pairs against the float64 oracle forward, within test 4's a-priori bound evaluated on the folded tables
    # plus the fold's one rounding (rfm_bound(fold=True)); the worst difference relative to the project's eval tolerance
    # 1e-5 + 1e-5 |s| is reported, not asserted
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    users = np.arange(U, dtype=np.int64)
    qt, qbt = cat._queries(torch.from_numpy(users))
    num = lambda t: t.cpu().numpy()
    tol = rfm_bound(num(qt), num(qbt), num(cat.c), np.where(el, num(cat.c_bias), 0.0).astype(np.float32), num(cat.W),
                    num(cat.b), num(cat.s), num(cat.l), H, fold=True)
    eval_tol = 1e-5 + 1e-5 * np.abs(s64)
    diff = np.abs(got[:, el] - s64[:, el])
    print('%s: score_pairs against the oracle, worst |difference| / bound = %.3f, / eval tolerance = %.3f'
          % (mt, float((diff / tol[:, el]).max()), float((diff / eval_tol[:, el]).max())))
    assert (diff <= tol[:, el]).all()
    assert np.isneginf(got[:, ~el]).all()
    # (b) ... and against the package's own forward and the native engine's predict on the same pairs: each of them is
    # within the project's eval tolerance of the oracle (test_tiny_eval.py), the catalogue within its bound
    dev_data = [d.to(DEV) for d in data]
    engine = M.make_engine(dict(hp, engine='native'), model)
    assert engine is not None and hasattr(engine, 'predict')
    with torch.no_grad():
        outs = [('forward', model(dev_data)[0]),
                ('predict', torch.cat([engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone()
                                       for a in range(0, U * I, 96)]))]
        for name, out in outs:
            mine = out.reshape(U, I).cpu().numpy().astype(np.float64)
            d = np.abs(got[:, el] - mine[:, el])
            print('%s: score_pairs against %s, worst |difference| / (bound + eval tolerance) = %.3f, / eval tolerance = %.3f'
                  % (mt, name, float((d / (tol + eval_tol)[:, el]).max()), float((d / eval_tol[:, el]).max())))
            assert (d <= (tol + eval_tol)[:, el]).all(), name
    # (c) the lists, (d) the ranks
    seen = {}
    for r in train.data:
        seen.setdefault(int(r[0]), set()).add(int(r[1]))
    for exclude in (True, False):
        ids, sc = cat.recommend(users, k=K, exclude_seen=exclude)
        assert ids.device.type == 'cuda' and ids.dtype == torch.int64 and sc.dtype == torch.float32
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        masked = np.where(el[None, :], s64, -np.inf)
        if exclude:
            for uu, items in seen.items():
                masked[uu, sorted(items)] = -np.inf
        check_lists(ids, sc, masked, tol, K, '%s exclude=%s' % (mt, exclude))
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
    few = TransNetCatalogue(model, hp, train, candidates=np.array(eligible[:3]))
    ids, _ = few.recommend(users[:4], k=K, exclude_seen=False)
    assert sorted(ids[0].cpu().tolist()) == [-1, -1] + eligible[:3]
    small = TransNetCatalogue(model, hp, train, tower_batch=5)
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
@pytest.mark.parametrize('mt', ['transnet', 'transnet++'])
def test_a_recommend_pass_leaves_the_transnet_training_state(mt):
    """Train, recommend and rank, continue == training never interrupted: weights, moments, offset, step_count, bit for
    bit (dropout 0.5: a moved stream would show)."""
    from reviews4rec_amd import TransNetCatalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=53)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build(mt, corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = TransNetCatalogue(model, hp, reader, engine=engine, tower_batch=50)
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
    from reviews4rec_amd import TransNetCatalogue, ops
    from test_gpu_span import build, tiny_corpus
    hp, reader, model, engine = build('transnet++', tiny_corpus(seed=54))
    order = []
    inner = ops.textcnn_fwd_raw
    monkeypatch.setattr(ops, 'textcnn_fwd_raw', lambda *a, **k: (order.append('read'), inner(*a, **k))[1])

    class Flushing:
        def flush(self):
            order.append('flush')

    cat = TransNetCatalogue(model.eval(), hp, reader, engine=Flushing())
    assert order[0] == 'flush' and order.count('flush') == 1 and 'read' in order
    del order[:]
    cat.refresh()
    assert order[0] == 'flush' and order.count('flush') == 1 and 'read' in order
    del order[:]
    TransNetCatalogue(model, hp, reader, engine=None)         # no engine: nothing to call
    assert 'flush' not in order and 'read' in order
