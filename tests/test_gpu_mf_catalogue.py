"""MF's catalogue on the device: r4r_topk_pfm / r4r_pair_pfm / r4r_rank_pfm (csrc/topk_pfm.hip, include/r4r.h
"Catalogue recommendation: product-FM heads") and recommend.MFCatalogue on top of them.

The reference ordering is test_gpu_recommend.py's (float64 scores, np.lexsort on (id, -score), the exclusions applied,
the -1 / -inf fill) over

    x_m = max(q[u][m] + c[i][m], 0)  m < H,   x_m = q[u][m] c[i][m]  H <= m < D = H + G,   y = W x + b
    score(u, i) = sum_j s_j y_j^2 + sum_m x_m (g_m x_m + e_m) + c_bias[i] + q_bias[u]

With q and c multiples of 1/2 in [-1/2, 1/2], W multiples of 1/2 in [-1, 1] with at most 8 non-zeros per row, b and e
multiples of 1/4 in [-1, 1], s and g in {1/2, -1/2, 0} and the biases multiples of 1/64, every intermediate is exact in fp32
up to (H, G, M) = (64, 64, 128): x in 1/4, |x| <= 1 (a product is +-1/4 or 0); y in 1/8, |y| <= 9; s y in 1/16 and s y^2 in
1/128, at most 40.5; g x + e in 1/8 and x (g x + e) in 1/32, at most 1.5; 128 + 128 of them stay below 2^13 at 1/128.  So
the kernel must return EXACTLY that list; with real-valued inputs the a-priori bound of test 4 decides what is demanded.

The library cannot say which instantiation ran, so the shapes are chosen from csrc/topk_pfm.hip's dispatch table (the
smallest of <3, 1> <4, 1> <8, 2> <16, 4> <32, 8> = <MFMA steps, row tiles> with D <= 4 steps and M <= 16 tiles):
(0, 0, 0), (6, 6, 12), (5, 3, 7), (4, 4, 16) -> <3, 1>;  (8, 8, 16) -> <4, 1>;  (16, 16, 32) -> <8, 2>;  (32, 32, 64),
(0, 64, 16) -> <16, 4>;  (64, 64, 128), (64, 0, 128) -> <32, 8>.  Every instantiation holds 4 queries per wave and 4 waves
per workgroup: n_q = 1, 3, 4, 5 lie around the wave's tile, 16, 17 and 33 around the workgroup's."""
import numpy as np
import pytest
import torch

from test_gpu_recommend import check_lists, dyadic, mask_excluded, ref_lists, small_chunk
from test_gpu_transnet_catalogue import host_ranks

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the reference scores
def _inputs(q, c, H, split=False):
    """x [n_q, n_c, D] in float64: fmaxf's NaN rule on the first H columns (a NaN sum counts as 0), products behind them
    (a NaN stays).  split: |q| + |c| in place of |relu(q + c)| (what bounds the rounding of the TABLES)."""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid='ignore'):
        if split:
            lo = np.abs(q64)[:, None, :H] + np.abs(c64)[None, :, :H]
        else:
            lo = np.fmax(q64[:, None, :H] + c64[None, :, :H], 0.0)
        return np.concatenate([lo, q64[:, None, H:] * c64[None, :, H:]], -1)


def _opt(a, n):
    return np.zeros(n) if a is None else a.astype(np.float64)


def ref_scores(q, qb, c, cb, W, b, s, g, e, H, check_exact=False):
    """float64; a NaN in a product column or in a bias propagates (the column sum is NaN whatever g and e hold)."""
    n_q, n_c, M, D = q.shape[0], c.shape[0], W.shape[0], q.shape[1]
    out = np.zeros((n_q, n_c), np.float64)
    W64, s64, b64, g64, e64 = W.astype(np.float64), s.astype(np.float64), _opt(b, M), _opt(g, D), _opt(e, D)
    for u0 in range(0, n_q, 8):                               # (8 queries at a time: [8, n_c, 128] float64 at most)
        x = _inputs(q[u0:u0 + 8], c, H)
        bad = np.isnan(x).any(-1)
        x = np.nan_to_num(x)
        y = x @ W64.T + b64
        rows, cols = s64 * y * y, x * (g64 * x + e64)
        if check_exact:
            assert np.array_equal(x * 4, np.round(x * 4)) and (np.abs(x) <= 1).all()
            assert np.array_equal(y * 8, np.round(y * 8)) and (np.abs(y) <= 9).all()
            assert np.array_equal(s64 * y * 16, np.round(s64 * y * 16))
            assert np.array_equal(rows * 128, np.round(rows * 128)) and (np.abs(rows) <= 40.5).all()
            assert np.array_equal((g64 * x + e64) * 8, np.round((g64 * x + e64) * 8))
            assert np.array_equal(cols * 32, np.round(cols * 32)) and (np.abs(cols) <= 1.5).all()
        t = rows.sum(-1) + cols.sum(-1)
        t[bad] = np.nan
        out[u0:u0 + 8] = t
    with np.errstate(invalid='ignore'):
        if cb is not None:
            out = out + cb.astype(np.float64)[None, :]
        if qb is not None:
            out = out + qb.astype(np.float64)[:, None]
    return out


def roundings(D, M, fold=False):
    return 2 * D + -(-D // 4) + -(-M // 4) + 10 + (8 if fold else 0)


def pfm_bound(q, qb, c, cb, W, b, s, g, e, H, fold=False):
    """roundings(D, M) 2^-24 Mag[u][i], Mag = sum_j |s_j| Y_j^2 + sum_m (|g_m| X_m^2 + |e_m| X_m) + |c_bias| + |q_bias|,
    X_m = |x_m|, Y_j = sum_m |W_jm| X_m + |b_j|: see test 4.  fold: the tables are themselves one rounding of float64
    numbers (test 8) -- X_m becomes |q_m| + |c_m| under the ReLU (the sum may cancel what was rounded) and eight roundings
    are added: x_m carries 2 more at most (q and c), W_jm one, so y_j 3 more and its square 6; g_m x_m^2 5, a bias 1."""
    D, M = q.shape[1], W.shape[0]
    mag = np.zeros((q.shape[0], c.shape[0]), np.float64)
    for u0 in range(0, q.shape[0], 8):
        X = np.abs(_inputs(q[u0:u0 + 8], c, H, split=fold))
        Y = X @ np.abs(W.astype(np.float64)).T + np.abs(_opt(b, M))
        mag[u0:u0 + 8] = (np.abs(s.astype(np.float64)) * Y * Y).sum(-1) + (np.abs(_opt(g, D)) * X * X + np.abs(_opt(e, D)) * X).sum(-1)
    mag = mag + np.abs(cb.astype(np.float64))[None, :] + np.abs(qb.astype(np.float64))[:, None]
    return roundings(D, M, fold) * EPS * mag


# ---------------------------------------------------------------- the calls
def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # (a copy: the shared inputs are read-only)


class Tables:
    """The inputs on the device; c with a row stride of D + pad (the pad holds NaN)."""

    def __init__(self, q, qb, c, cb, W, b, s, g, e, H, pad=3):
        self.n_q, self.D = q.shape
        self.n_c, self.M = c.shape[0], W.shape[0]
        self.H, self.G = H, self.D - H
        self.stride = self.D + pad
        self.c = torch.full((max(self.n_c, 1), max(self.stride, 1)), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.D:
            self.c[:self.n_c, :self.D] = _dev(c)
        some = lambda a, n: None if a is None else _dev(a if n else np.zeros(1, np.float32))
        self.q = _dev(q.reshape(-1) if self.D else np.zeros(1, np.float32))
        self.W = _dev(W.reshape(-1) if self.D * self.M else np.zeros(1, np.float32))
        self.s, self.b = some(s, self.M), some(b, self.M)
        self.g, self.e = some(g, self.D), some(e, self.D)
        self.qb, self.cb = _dev(qb), _dev(cb)

    def head(self):
        from reviews4rec_amd._lib import ptr
        return (ptr(self.q), self.n_q, ptr(self.qb), ptr(self.c), self.n_c, self.stride, ptr(self.cb), ptr(self.W),
                ptr(self.b), ptr(self.s), ptr(self.g), ptr(self.e), self.H, self.G, self.M)


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
    nb = _lib.lib().r4r_topk_pfm_ws_bytes(t.n_q, t.n_c, K, chunk)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_topk_pfm', *t.head(), ptr(eo), ptr(ei), K, chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def pairs(t, qi, ci):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    qd, cd = _dev(qi.astype(np.int64)), _dev(ci.astype(np.int64))
    out = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_pair_pfm', *t.head(), ptr(qd), ptr(cd), len(qi), ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rank(t, qi, ti, chunk=0, excl=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    eo, ei = _excl(excl)
    qd, td = _dev(qi.astype(np.int64)), _dev(ti.astype(np.int64))
    r = torch.full((len(qi),), -7, dtype=torch.int64, device=DEV)
    s = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_rank_pfm', *t.head(), ptr(qd), ptr(td), len(qi), ptr(eo), ptr(ei), chunk, ptr(r), ptr(s))
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy()


def exact_inputs(rng, n_q, n_c, H, G, M):
    """-> (q, qb, c, cb, W, b, s, g, e) within the module docstring's grid."""
    D = H + G
    q, c = dyadic(rng, (n_q, D), 0.5, 0.5), dyadic(rng, (n_c, D), 0.5, 0.5)
    W = np.zeros((M, D), np.float32)
    for j in range(M):                                        # at most 8 non-zeros per row
        cols = rng.permutation(D)[:8]
        W[j, cols] = dyadic(rng, (len(cols),), 0.5, 1.0)
    b, e = dyadic(rng, (M,), 0.25, 1.0), dyadic(rng, (D,), 0.25, 1.0)
    s = rng.choice(np.array([0.5, -0.5, 0.0], np.float32), size=M)
    g = rng.choice(np.array([0.5, -0.5, 0.0], np.float32), size=D)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    return q, qb, c, cb, W, b, s, g, e


_REAL = {}


def real_inputs(H, G, M, n_q=33, n_c=4099, seed=7, gain=1.0, spread=0.3):
    """Standard-normal tables and a head laid out as fold_mf_head's (the first half of the rows at s = +1/2, the second at
    -1/2; g = 0 under the ReLU and negative behind it), rows of W of norm about ``gain``, candidate biases of deviation
    ``spread``; computed once per key and shared, never written to."""
    key = (H, G, M, n_q, n_c, seed, gain, spread)
    if key not in _REAL:
        D = H + G
        rng = np.random.default_rng(seed)
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
        s = np.full(M, -0.5, np.float32)
        s[:(M + 1) // 2] = 0.5
        g = (-0.5 * gain * gain / max(D, 1) * f(D) ** 2).astype(np.float32)
        g[:H] = 0.0
        _REAL[key] = (f(n_q, D), (4 + f(n_q)).astype(np.float32), f(n_c, D), (spread * f(n_c)).astype(np.float32),
                      (f(M, D) * (gain / np.sqrt(max(D, 1)))).astype(np.float32), (0.1 * f(M)).astype(np.float32), s, g,
                      (f(D) * (gain / np.sqrt(max(D, 1)))).astype(np.float32))
        for a in _REAL[key]:
            a.setflags(write=False)
    return _REAL[key]


# ---------------------------------------------------------------- 1. exact arithmetic
SHAPES_EXACT = [(0, 0, 0), (6, 6, 12), (5, 3, 7), (4, 4, 16), (8, 8, 16), (16, 16, 32), (32, 32, 64), (64, 64, 128),
                (64, 0, 128), (0, 64, 16)]
N_Q, N_C, KS = [1, 3, 4, 5, 17, 33], [1, 15, 16, 17, 65, 257], [1, 10, 128]
EXACT = sorted({(N_Q[(t + t // 10) % 6], N_C[(t + t // 6) % 6]) + SHAPES_EXACT[t % 10] + (KS[(t + t // 10) % 3],)
                for t in range(30)} |
               {(33, 4099, 64, 64, 128, 128),   # the largest instantiation, nine query tiles in three workgroups
                (65, 4099, 6, 6, 12, 10),       # MF on tests/golden/mf_full.npz; 17 query tiles: the last workgroup holds one
                (16, 257, 8, 8, 16, 10),        # four full tiles: one full workgroup
                (5, 4099, 32, 32, 64, 10),
                (4, 1, 64, 64, 128, 1), (5, 15, 64, 0, 128, 10), (3, 17, 0, 64, 16, 128)})


def test_the_exact_cases_cover_every_edge():
    """The table above, not a case of it: every query count, catalogue size and K with some shape, and every shape
    (hence every instantiation) with each K."""
    assert {k[0] for k in EXACT} >= set(N_Q) and {k[1] for k in EXACT} >= set(N_C)
    assert {k[2:] for k in EXACT} >= {sh + (K,) for sh in SHAPES_EXACT for K in KS}


@pytest.mark.parametrize('n_q, n_c, H, G, M, K', EXACT)
def test_exact_inputs_give_the_reference_list_bit_for_bit(n_q, n_c, H, G, M, K):
    rng = np.random.default_rng(n_q * 1000003 + n_c * 131 + H * 7 + G * 3001 + M * 1009 + K)
    a = exact_inputs(rng, n_q, n_c, H, G, M)
    want_ids, want_sc = ref_lists(ref_scores(*a, H, check_exact=True), K)
    assert np.array_equal(want_sc.astype(np.float32).astype(np.float64), want_sc)     # exact in fp32
    t = Tables(*a, H)                                                                 # c_stride = D + 3, NaN in the pad
    for chunk in (0, small_chunk(n_c)):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (chunk, np.argwhere(ids != want_ids)[:5])
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk                  # (as floats: -0.0 == 0.0)
    if (n_q, n_c, H, G, M, K) in ((16, 257, 8, 8, 16, 10), (5, 4099, 32, 32, 64, 10)):
        # NULL b, g, e and NULL biases count as 0
        q, qb, c, cb, W, b, s, g, e = a
        ids, sc = topk(Tables(q, None, c, None, W, None, s, None, None, H, pad=0), K, small_chunk(n_c))
        want_ids, want_sc = ref_lists(ref_scores(q, None, c, None, W, None, s, None, None, H), K)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc.astype(np.float32))


# ---------------------------------------------------------------- 2. degenerate rankings, 3. exclusions
@pytest.mark.parametrize('case', ['all equal', 'K above the eligible count', 'every candidate -inf', 'NaN rows'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_q, n_c, H, G, M, K = 17, 300, 6, 6, 12, 10
    q, qb, c, cb, W, b, s, g, e = exact_inputs(rng, n_q, n_c, H, G, M)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
        q[:] = q[:1]
        qb[:] = qb[:1]
    elif case == 'K above the eligible count':
        cb[rng.permutation(n_c)[7:]] = -np.inf                                       # seven eligible rows
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    else:
        c[41], c[42, H + 2] = np.nan, np.nan  # a NaN in a product column: the score is NaN, the row is on no list
        cb[41], cb[42] = 30.0, 30.0           # ... whatever its bias
        cb[43] = np.nan                       # through c_bias the row is dropped as well
        c[44, 1], cb[44] = np.nan, 1000.0      # under the ReLU alone fmaxf takes a NaN sum as 0: the row stays, on top
    a = (q, qb, c, cb, W, b, s, g, e)
    sc64 = ref_scores(*a, H)
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
    t = Tables(*a, H)
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
    n_q, n_c, H, G, M, K = 5, 1000, 6, 6, 12, 10
    a = exact_inputs(rng, n_q, n_c, H, G, M)
    sc64 = ref_scores(*a, H)
    free_ids, _ = ref_lists(sc64, K)
    lists = [np.zeros(0, np.int64),                                                  # an empty list
             free_ids[1, :1].copy(),                                                 # the would-be winner
             np.arange(n_c, dtype=np.int64),                                         # everything
             np.union1d(np.arange(64, 192), free_ids[3, :4]).astype(np.int64),       # empties the chunks [64, 128), [128, 192)
             np.sort(free_ids[4]).astype(np.int64)]                                  # the whole free top-K
    assert len(lists[3]) > 64
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_ids, want_sc = ref_lists(mask_excluded(sc64, excl), K)
    assert np.array_equal(want_ids[0], free_ids[0]) and want_ids[1, 0] == free_ids[1, 1]
    assert (want_ids[2] == -1).all() and not np.isin(want_ids[3], lists[3]).any()
    assert not np.isin(want_ids[4], free_ids[4]).any()
    t = Tables(*a, H)
    for chunk in (0, 64, 333):
        ids, sc = topk(t, K, chunk, excl=excl)
        assert np.array_equal(ids, want_ids), chunk
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
SHAPES = [(6, 6, 12), (32, 32, 64), (64, 64, 128)]
FAMILY = dict(gain=0.25, spread=3.0)          # chosen on the host, before any device run: see the docstring below
DEMANDED_AT_LEAST = {(6, 6, 12): 25, (32, 32, 64): 20, (64, 64, 128): 10}


def demanded_by_float64(s64, tol, K):
    """Rows of s64 whose K + 1 best float64 scores lie more than twice the row's largest bound apart: what check_lists
    demands the ids of.  Needs no device."""
    n = 0
    for u in range(s64.shape[0]):
        ok = s64[u] > -np.inf
        ranked = np.sort(s64[u, ok])[::-1][:K + 1]
        n += int((ranked[:-1] - ranked[1:]).min() > 2 * float(tol[u, ok].max()))
    return n


@pytest.mark.parametrize('H, G, M', SHAPES)
def test_real_valued_inputs_within_the_a_priori_bound(H, G, M):
    """The bound, to first order in eps = 2^-24 and relative to Mag[u][i] = sum_j |s_j| Y_j^2 + sum_m (|g_m| X_m^2 +
    |e_m| X_m) + |c_bias| + |q_bias| with X_m = |x_m| and Y_j = sum_m |W_jm| X_m + |b_j|, which dominates every partial
    sum's magnitude.  With D = H + G:
      x_m        1: the rounding of q_m + c_m (the ReLU is 1-Lipschitz and maps 0 to 0, so x_m keeps its RELATIVE error)
                 or of q_m c_m
      y_j        1 (x_m, carried through |W_jm|) + D (the fmaf chain over m) + 1 (the addition of b_j): (D + 2) eps Y_j
      s_j y_j    one more rounding: (D + 3) eps |s_j| Y_j
      s_j y_j^2  |s_j y_j| dy_j + |y_j| d(s_j y_j) <= (2 D + 5) eps |s_j| Y_j^2; its own rounding is the fmaf of the t_k
                 chain
      column m   g_m x_m + e_m inherits |g_m| eps X_m and adds one rounding of at most eps (|g_m| X_m + |e_m|); times x_m
                 that is (2 |g_m| X_m + |e_m|) eps X_m + (|g_m| X_m + |e_m|) eps X_m <= 3 eps (|g_m| X_m^2 + |e_m| X_m)
      the sums   at most ceil(M / 4) fmaf of a t_k chain and ceil(D / 4) of a v_k chain, t_k + v_k, the two levels of the
                 tree and the additions of c_bias and q_bias: ceil(M / 4) + ceil(D / 4) + 5 roundings, each relative to a
                 partial sum that Mag dominates
    together max(2 D + 5, 3) + ceil(M / 4) + ceil(D / 4) + 5 = 2 D + ceil(D / 4) + ceil(M / 4) + 10 roundings.
    Mag sums 2 L squares of opposite signs, so with rows of W of norm 1 the bound is wide against the gaps between ten
    neighbours out of 4099: the float64 reference alone, on the host, demands the ids of 31 to 33, 14 to 23 and 1 to 5 rows of
    33 at the three shapes over seeds 0 .. 7 with norm 1 and candidate biases of deviation 0.3 (the inputs of tests 5 to 7;
    there the count is printed, not asserted).  With norm 1/4 and deviation 3 (FAMILY, chosen from these host counts) it
    demands, seed by seed 0 .. 7,
        (6, 6, 12)      33 32 33 33 32 32 33 33
        (32, 32, 64)    30 27 33 29 29 30 29 27
        (64, 64, 128)   23 19 18 19 15 21 21 20
    25, 20 and 10 are asserted of the kernel at seed 7, and five more of the reference itself."""
    K = 10
    a = real_inputs(H, G, M, **FAMILY)
    s64, tol = ref_scores(*a, H), pfm_bound(*a, H)
    assert demanded_by_float64(s64, tol, K) >= DEMANDED_AT_LEAST[(H, G, M)] + 5       # the reference alone, with room
    t = Tables(*a, H)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(t, K, chunk)
        rows, got = np.nonzero(ids >= 0)[0], ids[ids >= 0]
        err = np.abs(sc[ids >= 0].astype(np.float64) - s64[rows, got]) / tol[rows, got]
        print('H=%d G=%d M=%d chunk=%d: worst |error| / bound over the lists = %.3f' % (H, G, M, chunk, float(err.max())))
        demanded = check_lists(ids, sc, s64, tol, K, 'H=%d G=%d M=%d chunk=%d' % (H, G, M, chunk))
        print('rows whose ids were demanded: %d of 33' % demanded)
        assert demanded >= DEMANDED_AT_LEAST[(H, G, M)], demanded
    # the inputs of tests 5 to 7 (rows of W of norm 1, candidate biases of deviation 0.3): here the squares decide the
    # order, the same bound holds for every score and every list must be valid under it; how many rows have their ids
    # demanded is printed, not capped
    a = real_inputs(H, G, M)
    s64, tol = ref_scores(*a, H), pfm_bound(*a, H)
    ids, sc = topk(Tables(*a, H), K, small_chunk(4099))
    rows, got = np.nonzero(ids >= 0)[0], ids[ids >= 0]
    err = np.abs(sc[ids >= 0].astype(np.float64) - s64[rows, got]) / tol[rows, got]
    demanded = check_lists(ids, sc, s64, tol, K, 'H=%d G=%d M=%d, norm 1' % (H, G, M))
    print('H=%d G=%d M=%d, rows of W of norm 1: worst |error| / bound over the lists = %.3f, rows whose ids were demanded: '
          '%d of 33' % (H, G, M, float(err.max()), demanded))


# ---------------------------------------------------------------- 5. the pair kernel
@pytest.mark.parametrize('H, G, M', SHAPES_EXACT)
def test_pair_scores_have_the_bits_of_the_ranking(H, G, M):
    """The MFMA chain of the scan against the scalar chain of r4r_pair_pfm, real-valued inputs, no tolerance."""
    K = 10
    # (against 65 candidates: 256 pairs fill the last 256-thread workgroup of the pair kernel exactly, 257 leave one pair
    # in it)
    for n_c, counts in ((4099, (33 * K,)), (65, (256, 257))):
        a = real_inputs(H, G, M, n_c=n_c)
        t = Tables(*a, H)
        ids, sc = topk(t, K, 0)
        assert (ids >= 0).all()
        for n in counts:
            out = pairs(t, np.repeat(np.arange(33), K)[:n], ids.reshape(-1)[:n])
            assert np.array_equal(out.view(np.uint32), sc.reshape(-1)[:n].view(np.uint32)), (n_c, n)


# ---------------------------------------------------------------- 6. batching invariance
@pytest.mark.parametrize('H, G, M', [(6, 6, 12), (64, 64, 128)])
def test_batching_and_chunking_do_not_change_a_bit(H, G, M):
    K = 10
    q, qb, c, cb, W, b, s, g, e = real_inputs(H, G, M)
    rng = np.random.default_rng(M)
    lists = [np.sort(rng.permutation(4099)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(33)]
    off = np.zeros(34, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids_all = np.concatenate(lists)

    def sub(a, b_):
        return (off[a:b_ + 1] - off[a], ids_all[off[a]:off[b_]])

    def run(a, b_, chunk):
        return topk(Tables(q[a:b_], qb[a:b_], c, cb, W, b, s, g, e, H), K, chunk, excl=sub(a, b_))

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
@pytest.mark.parametrize('n_p, n_c, H, G, M', [(1, 65, 5, 3, 7), (3, 257, 6, 6, 12), (4, 65, 0, 0, 0), (5, 4099, 8, 8, 16),
                                               (17, 4099, 16, 16, 32), (130, 65, 32, 32, 64), (65, 4099, 64, 64, 128),
                                               (17, 257, 64, 0, 128), (33, 257, 0, 64, 16),
                                               # the target kernel's last 256-thread workgroup exactly full / holding one pair
                                               (256, 65, 5, 3, 7), (257, 65, 6, 6, 12),
                                               # waves of the exclusion kernel's last workgroup without a pair (below)
                                               (5, 257, 6, 6, 12)])
def test_ranks_are_the_count_of_candidates_ahead(n_p, n_c, H, G, M):
    rng = np.random.default_rng(700 + n_p + n_c + M)
    n_q = 9
    q, qb, c, cb, W, b, s, g, e = (a.copy() for a in real_inputs(H, G, M, n_q=n_q, n_c=n_c, seed=800 + n_p + H))
    c[5] = c[3]                                              # exact ties: rows 3 and 5 score alike for every query
    cb[5] = cb[3]
    cb[7] = -np.inf                                          # an ineligible row
    t = Tables(q, qb, c, cb, W, b, s, g, e, H)
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


# ---------------------------------------------------------------- 8. MF with the weights of tests/golden/mf_full.npz
class Ratings:
    """What a catalogue reads of a data reader: the rating rows and the two count tables."""

    def __init__(self, rows):
        self.data = np.asarray(rows, np.float64).reshape(-1, 3)
        self.user_count, self.item_count = {}, {}
        for u, i, _ in self.data:
            self.user_count[int(u)] = self.user_count.get(int(u), 0) + 1
            self.item_count[int(i)] = self.item_count.get(int(i), 0) + 1


def test_mf_catalogue_on_the_golden_weights_against_the_oracle():
    import oracle
    import reviews4rec_amd
    from helpers import Golden
    from reviews4rec_amd import MFCatalogue, eval_catalogue, ranking_metrics
    from reviews4rec_amd import main as M
    gold = Golden('mf_full')
    hp, W = dict(gold.hp), gold.params()
    L, U, I, K = hp['latent_size'], hp['total_users'], hp['total_items'], 5
    assert (L, U, I) == (6, 30, 20)
    rng = np.random.default_rng(8)
    eligible = sorted(rng.permutation(I)[:15].tolist())                              # five items without a training rating
    rows = sorted({(int(rng.integers(0, U)), int(rng.choice(eligible))) for _ in range(90)})
    rows += [(0, i) for i in eligible if i not in {r[1] for r in rows}]
    train = Ratings([(u, i, 3.0) for u, i in rows])
    test = Ratings([(int(rng.integers(0, U)), int(rng.integers(0, I)), 4.0) for _ in range(40)])
    model = reviews4rec_amd.get_model_class('MF')(hp)
    model.load_state_dict(W, strict=True)
    model = model.cuda().eval()
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    data = [torch.zeros((len(u), 1), dtype=torch.int64) for _ in range(5)] + [torch.from_numpy(u), torch.from_numpy(i)]
    P64 = {k: v.double() for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    cat = MFCatalogue(model, hp, train)
    assert cat.eligible.tolist() == eligible and cat.c.shape == (I + 1, 2 * L) and cat.W.shape == (2 * L, 2 * L)
    assert (cat.H, cat.G, cat.M, cat.n_c) == (L, L, 2 * L, I + 1)
    el = np.zeros(I, bool)
    el[eligible] = True
    # (a) score_pairs against the float64 oracle forward, within test 4's a-priori bound evaluated on the folded tables
    # plus the fold's own rounding (pfm_bound(fold=True)), and within the project's eval tolerance
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    users = np.arange(U, dtype=np.int64)
    qt, qbt = cat._queries(torch.from_numpy(users))
    num = lambda t: t.cpu().numpy()
    cb = np.where(np.isfinite(num(cat.c_bias)), num(cat.c_bias), 0.0).astype(np.float32)
    tol = pfm_bound(num(qt), num(qbt), num(cat.c), cb, num(cat.W), num(cat.b), num(cat.s), num(cat.g), num(cat.e), L,
                    fold=True)[:, :I]
    eval_tol = 1e-5 + 1e-5 * np.abs(s64)
    diff = np.abs(got[:, el] - s64[:, el])
    print('score_pairs against the oracle, worst |difference| / bound = %.3f, / eval tolerance = %.3f'
          % (float((diff / tol[:, el]).max()), float((diff / eval_tol[:, el]).max())))
    assert (diff <= tol[:, el]).all()
    assert np.isneginf(got[:, ~el]).all()
    # (b) ... and against the package's own eval forward and the native engine's predict on the same pairs
    dev_data = [d.to(DEV) for d in data]
    engine = M.make_engine(dict(hp, engine='native'), model)
    assert engine is not None and hasattr(engine, 'predict')
    with torch.no_grad():
        outs = [('forward', model(dev_data)),
                ('predict', torch.cat([engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone()
                                       for a in range(0, U * I, 96)]))]
        for name, out in outs:
            mine = out.reshape(U, I).cpu().numpy().astype(np.float64)
            d = np.abs(got[:, el] - mine[:, el])
            print('score_pairs against %s, worst |difference| / eval tolerance = %.3f'
                  % (name, float((d / eval_tol[:, el]).max())))
            assert (d <= eval_tol[:, el]).all(), name
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
        check_lists(ids, sc, masked, tol, K, 'exclude=%s' % exclude)
        assert np.isin(ids[ids >= 0], eligible).all()
        if exclude:
            assert not any(int(x) in seen.get(uu, ()) for uu in range(U) for x in ids[uu])
        flat = ids.reshape(-1)
        again = cat.score_pairs(np.repeat(users, K)[flat >= 0], flat[flat >= 0]).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), sc.reshape(-1)[flat >= 0].view(np.uint32))
        # the rank of an item is its position in the whole list, wherever the list holds it ...
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
        # ... and the host's sort of the float64 scores wherever their gaps exceed the bound
        order = np.argsort(-masked, axis=1, kind='stable')
        for uu in range(U):
            srt = masked[uu, order[uu]]
            n = int((srt > -np.inf).sum())
            clear = n < 2 or (srt[:n - 1] - srt[1:n]).min() > 2 * float(tol[uu, el].max())
            if clear:
                assert full[uu, :n].tolist() == order[uu, :n].tolist(), uu
    # candidates= overrides the default set
    few = MFCatalogue(model, hp, train, candidates=np.array(eligible[:3]))
    ids, _ = few.recommend(users[:4], k=K, exclude_seen=False)
    assert sorted(ids[0].cpu().tolist()) == [-1, -1] + eligible[:3]
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
    # the full-catalogue metrics go through the class: ranking_metrics over rank()'s own ranks of the test rows
    m = eval_catalogue(model, train, test, hp, ks=[1, 5], catalogue=cat)
    assert set(m) == {'cat_HR@1', 'cat_HR@5', 'cat_NDCG@1', 'cat_NDCG@5', 'cat_MRR', 'cat_ranked', 'cat_unranked'}
    tr, _ = cat.rank(test.data[:, 0].astype(np.int64), test.data[:, 1].astype(np.int64), exclude_seen=True)
    want = ranking_metrics(tr, [1, 5])
    assert m['cat_ranked'] == want['ranked'] > 0 and m['cat_unranked'] == want['unranked'] > 0
    assert m['cat_ranked'] + m['cat_unranked'] == len(test.data)
    for k in ('HR@1', 'HR@5', 'NDCG@1', 'NDCG@5', 'MRR'):
        assert m['cat_' + k] == round(100.0 * want[k], 2), k


# ---------------------------------------------------------------- 9. training state
def test_a_catalogue_pass_leaves_the_mf_training_state_and_sees_the_flushed_tables():
    """Train a span, recommend and rank, train another == training never interrupted: weights, moments, offset,
    step_count, bit for bit (dropout 0.5: a moved stream would show).  The lists taken in between are those of a fresh
    model loaded from that moment's state_dict: the blocked sweeps' pending rows were flushed before either side was
    read."""
    import reviews4rec_amd
    from reviews4rec_amd import MFCatalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=55)
    K = 5
    users = np.arange(300)
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('MF', corpus, dropout=0.5)
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = MFCatalogue(model, hp, reader, engine=engine)
            ids, sc = cat.recommend(users, k=5)
            assert (ids[:, 0] >= 0).all() and torch.isfinite(sc[:, 0]).all() and model.training
            items = cat.eligible[users % len(cat.eligible)]
            ranks, rs = cat.rank(users, items)
            assert (ranks >= 0).all() and torch.isfinite(rs).all() and model.training
            again = cat.score_pairs(users, items)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), rs.cpu().numpy().view(np.uint32))
            fresh = reviews4rec_amd.get_model_class('MF')(hp)
            fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
            other = MFCatalogue(fresh.cuda().eval(), hp, reader)
            ids2, sc2 = other.recommend(users, k=5)
            assert torch.equal(ids, ids2) and torch.equal(sc.view(torch.int32), sc2.view(torch.int32))
            ranks2, rs2 = other.rank(users, items)
            assert torch.equal(ranks, ranks2) and torch.equal(rs.view(torch.int32), rs2.view(torch.int32))
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K


def test_pending_table_updates_are_flushed_on_both_sides():
    """The native step's blocked sweeps leave table rows behind until flush(): MFCatalogue(engine=engine) must see the
    tables a fresh MFCatalogue sees after an explicit flush -- at refresh() (the item side) and again at every call (the
    query side, after more deferred steps and NO refresh)."""
    from reviews4rec_amd import MFCatalogue
    from test_gpu_span import build, tiny_corpus
    corpus = tiny_corpus(seed=56)
    users = np.arange(300, dtype=np.int64)
    got = []
    for explicit in (False, True):
        hp, reader, model, engine = build('MF', corpus)
        model.train()
        batches = iter(reader.iter())
        for _ in range(5):
            engine.train_step(*next(batches), defer_sweep=True)
        assert engine._pending() is not None                  # five steps into a period: updates are pending
        if explicit:
            engine.flush()
            assert engine._pending() is None
        cat = MFCatalogue(model, hp, reader, engine=None if explicit else engine)
        assert engine._pending() is None
        ids, sc = cat.recommend(users, k=7)
        for _ in range(3):
            engine.train_step(*next(batches), defer_sweep=True)
        assert engine._pending() is not None
        if explicit:
            engine.flush()
        q, qb = cat._queries(torch.from_numpy(users))         # (no refresh: the item side is the cache)
        assert engine._pending() is None
        got.append((ids.cpu(), sc.cpu(), q.cpu(), qb.cpu(), model.item_embedding.weight.detach().cpu().clone(),
                    model.user_embedding.weight.detach().cpu().clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert (got[0][0] >= 0).all()
