"""The ReLU-sum catalogue on the device: r4r_topk_relu / r4r_pair_relu / r4r_rank_relu (csrc/topk_relu.hip, include/r4r.h
"Catalogue recommendation: ReLU-sum heads") and recommend.ReluCatalogue on top of them.

The reference ordering is test_gpu_recommend.py's (float64 scores, np.lexsort on (id, -score), the exclusions applied,
the -1 / -inf fill) over

    score(u, i) = sum_{j<H} w_j max(q[u][j] + c[i][j], 0) + sum_{j<P} q[u][H + j] c[i][H + j] + c_bias[i] + q_bias[u]

With inputs that are multiples of 1/8 (biases: of 1/64) every partial sum is exact in fp32 up to H = P = 128, so the
kernel must return EXACTLY that list; with real-valued inputs the a-priori bound (H + P + 4) 2^-24 M[u][i],
M = sum_j |w_j| (|q_j| + |c_j|) + sum_j |qp_j cp_j| + |c_bias| + |q_bias| (one rounding in the add, at most H in the
chain or P in the dot, three in the final additions, to first order) decides what is demanded."""
import os

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from test_gpu_recommend import check_lists, dyadic, mask_excluded, ref_lists, small_chunk

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the reference scores
def ref_scores(q, qb, c, cb, w, H):
    """float64; fmaxf's NaN rule (a NaN sum in a hidden column counts as 0), NaN elsewhere propagates."""
    q64, c64, w64 = q.astype(np.float64), c.astype(np.float64), w.astype(np.float64)
    s = np.zeros((q.shape[0], c.shape[0]), np.float64)
    with np.errstate(invalid='ignore'):
        for j in range(H):
            s += w64[j] * np.fmax(q64[:, j, None] + c64[None, :, j], 0.0)
        s = s + q64[:, H:] @ c64[:, H:].T
        if cb is not None:
            s = s + cb.astype(np.float64)[None, :]
        if qb is not None:
            s = s + qb.astype(np.float64)[:, None]
    return s


def relu_bound(q, qb, c, cb, w, H):
    P = q.shape[1] - H
    aq, ac, aw = np.abs(q.astype(np.float64)), np.abs(c.astype(np.float64)), np.abs(w.astype(np.float64))
    M = (aq[:, :H] @ aw)[:, None] + (ac[:, :H] @ aw)[None, :] + aq[:, H:] @ ac[:, H:].T
    M = M + np.abs(cb.astype(np.float64))[None, :] + np.abs(qb.astype(np.float64))[:, None]
    return (H + P + 4) * EPS * M


# ---------------------------------------------------------------- the calls
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Tables:
    """The inputs on the device; c with a row stride of H + P + pad (the pad holds NaN)."""

    def __init__(self, q, qb, c, cb, w, H, pad=3):
        self.n_q, self.HP = q.shape
        self.n_c, self.H, self.P = c.shape[0], H, q.shape[1] - H
        self.stride = self.HP + pad
        self.c = torch.full((max(self.n_c, 1), max(self.stride, 1)), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.HP:
            self.c[:self.n_c, :self.HP] = _dev(c)
        self.q = _dev(q.reshape(-1) if self.HP else np.zeros(1, np.float32))
        self.w = _dev(w if H else np.zeros(1, np.float32))
        self.qb, self.cb = _dev(qb), _dev(cb)

    def head(self):
        from reviews4rec_amd._lib import ptr
        return (ptr(self.q), self.n_q, ptr(self.qb), ptr(self.c), self.n_c, self.stride, ptr(self.cb), ptr(self.w),
                self.H, self.P)


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
    nb = _lib.lib().r4r_topk_relu_ws_bytes(t.n_q, t.n_c, K, chunk)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_topk_relu', *t.head(), ptr(eo), ptr(ei), K, chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def pairs(t, qi, ci):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    qd, cd = _dev(qi.astype(np.int64)), _dev(ci.astype(np.int64))
    out = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_pair_relu', *t.head(), ptr(qd), ptr(cd), len(qi), ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def rank(t, qi, ti, chunk=0, excl=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    eo, ei = _excl(excl)
    qd, td = _dev(qi.astype(np.int64)), _dev(ti.astype(np.int64))
    r = torch.full((len(qi),), -7, dtype=torch.int64, device=DEV)
    s = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_rank_relu', *t.head(), ptr(qd), ptr(td), len(qi), ptr(eo), ptr(ei), chunk, ptr(r), ptr(s))
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy()


def exact_inputs(rng, n_q, n_c, H, P):
    q, c, w = dyadic(rng, (n_q, H + P), 0.125, 1.0), dyadic(rng, (n_c, H + P), 0.125, 1.0), dyadic(rng, (H,), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    return q, qb, c, cb, w


def real_inputs(H, P, n_q=33, n_c=4099, rng=None):
    rng = np.random.default_rng(17 * H + P) if rng is None else rng
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    qa, ca, w, qp, cp = f(n_q, H), f(n_c, H), f(H), f(n_q, P), f(n_c, P)
    return np.hstack([qa, qp]), (4 + f(n_q)).astype(np.float32), np.hstack([ca, cp]), (0.3 * f(n_c)).astype(np.float32), w


# ---------------------------------------------------------------- 1. exact arithmetic
N_Q, N_C = [1, 15, 16, 17, 33, 65], [1, 63, 64, 65, 255, 257, 4099]
HS, PS, KS = [0, 1, 3, 4, 5, 10, 32, 33, 64, 100, 128], [0, 1, 5, 10, 64, 128], [1, 5, 10, 128]
EXACT = sorted({(N_Q[t % 6], N_C[(3 * t) % 7], HS[t % 11], PS[(5 * t + t // 6) % 6], KS[t % 4]) for t in range(30)} |
               {(33, 4099, 128, 128, 128), (1, 4099, 0, 0, 5), (17, 257, 0, 10, 10), (16, 4099, 0, 128, 5), (33, 255, 64, 0, 10),
                (65, 4099, 10, 0, 128),
                # the query tile is 16 rows (15 / 16 / 17 above, 65 = four tiles and one row); a wave takes 64 candidates
                # (63 / 64 / 65 above); the columns stream in blocks of 8 with a one-column tail loop:
                (17, 65, 7, 0, 5),          # H one below the block: the tail loop alone
                (16, 257, 8, 7, 10),        # H at the block, P one below it
                (15, 64, 9, 8, 5),          # H one above (a block and a one-column tail), P at the block
                (33, 4099, 16, 9, 10),      # two blocks; P one above the block
                (1, 63, 15, 17, 1)})        # a block and a seven-column tail; two blocks and one


@pytest.mark.parametrize('n_q, n_c, H, P, K', EXACT)
def test_exact_inputs_give_the_reference_list_bit_for_bit(n_q, n_c, H, P, K):
    assert 38 <= len(EXACT) <= 44
    rng = np.random.default_rng(n_q * 1000003 + n_c * 131 + H * 7 + P * 1009 + K)
    q, qb, c, cb, w = exact_inputs(rng, n_q, n_c, H, P)
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb, w, H), K)
    assert np.array_equal(want_sc.astype(np.float32).astype(np.float64), want_sc)     # exact in fp32
    t = Tables(q, qb, c, cb, w, H)
    for chunk in (0, small_chunk(n_c)):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (chunk, np.argwhere(ids != want_ids)[:5])
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk                  # (as floats: -0.0 == 0.0)
    if (n_q, n_c, H, P, K) == (33, 255, 64, 0, 10):                                   # NULL biases count as 0
        ids, sc = topk(Tables(q, None, c, None, w, H), K, small_chunk(n_c))
        want_ids, want_sc = ref_lists(ref_scores(q, None, c, None, w, H), K)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc.astype(np.float32))


# ---------------------------------------------------------------- 2. H = 0 is r4r_topk_dot at D = P
@pytest.mark.parametrize('P', [0, 10, 64, 128])
def test_without_hidden_columns_the_scores_are_topk_dot_s(P):
    import test_gpu_recommend as R
    q, qb, c, cb, w = real_inputs(0, P, rng=np.random.default_rng(900 + P))
    t = Tables(q, qb, c, cb, w, 0)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(t, 10, chunk)
        want_ids, want_sc = R.topk(q, qb, c, cb, 10, chunk)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)), chunk


# ---------------------------------------------------------------- 3. degenerate rankings and exclusions
@pytest.mark.parametrize('case', ['all equal', 'K above the eligible count', 'every candidate -inf', 'a NaN row'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_q, n_c, H, P, K = 17, 300, 5, 3, 10
    q, qb, c, cb, w = exact_inputs(rng, n_q, n_c, H, P)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
        q[:] = q[:1]
    elif case == 'K above the eligible count':
        cb[rng.permutation(n_c)[7:]] = -np.inf                                       # seven eligible rows
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    else:
        c[41], c[42, H + 1] = np.nan, np.nan                                         # (NaN reaches the score through the dot)
        q[0, H:] = 0.0                                                               # 0 * NaN is NaN all the same
        cb[43] = np.nan
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb, w, H), K)
    if case == 'all equal':
        assert (want_ids == np.arange(K)[None, :]).all()
    if case == 'K above the eligible count':
        assert (want_ids[:, 7:] == -1).all() and (want_ids[:, :7] >= 0).all()
    if case == 'every candidate -inf':
        assert (want_ids == -1).all()
    if case == 'a NaN row':
        assert not np.isin(want_ids, [41, 42, 43]).any()
    t = Tables(q, qb, c, cb, w, H)
    for chunk in (0, 64, 7):
        ids, sc = topk(t, K, chunk)
        assert np.array_equal(ids, want_ids), (case, chunk)
        assert np.array_equal(sc, want_sc.astype(np.float32)), (case, chunk)


def test_exclusions():
    rng = np.random.default_rng(6)
    n_q, n_c, H, P, K = 5, 1000, 5, 3, 10
    q, qb, c, cb, w = exact_inputs(rng, n_q, n_c, H, P)
    s = ref_scores(q, qb, c, cb, w, H)
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
    t = Tables(q, qb, c, cb, w, H)
    for chunk in (0, 64, 333):
        ids, sc = topk(t, K, chunk, excl=excl)
        assert np.array_equal(ids, want_ids), chunk
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
@pytest.mark.parametrize('H, P', [(1, 0), (10, 0), (10, 10), (64, 64), (128, 128)])
def test_real_valued_inputs_within_the_a_priori_bound(H, P):
    K = 10
    q, qb, c, cb, w = real_inputs(H, P)
    s64 = ref_scores(q, qb, c, cb, w, H)
    tol = relu_bound(q, qb, c, cb, w, H)
    t = Tables(q, qb, c, cb, w, H)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(t, K, chunk)
        got = ids[ids >= 0]
        err = np.abs(sc[ids >= 0].astype(np.float64) - s64[np.nonzero(ids >= 0)[0], got]) / tol[np.nonzero(ids >= 0)[0], got]
        print('H=%d P=%d chunk=%d: worst |error| / bound over the lists = %.3f' % (H, P, chunk, float(err.max())))
        demanded = check_lists(ids, sc, s64, tol, K, 'H=%d P=%d chunk=%d' % (H, P, chunk))
        print('rows whose ids were demanded: %d of 33' % demanded)
        assert demanded >= 20, demanded


# ---------------------------------------------------------------- 5. the pair kernel
@pytest.mark.parametrize('H, P', [(0, 0), (3, 0), (10, 10), (64, 64), (128, 128)])
def test_pair_scores_have_the_bits_of_the_ranking(H, P):
    K = 10
    # (against 65 candidates: 256 pairs fill the last 256-thread workgroup of the pair kernel exactly, 257 leave one pair
    # in it)
    for n_c, counts in ((4099, (33 * K,)), (65, (256, 257))):
        q, qb, c, cb, w = real_inputs(H, P, n_c=n_c, rng=np.random.default_rng(300 + 17 * H + P))
        t = Tables(q, qb, c, cb, w, H)
        ids, sc = topk(t, K, 0)
        assert (ids >= 0).all()
        for n in counts:
            out = pairs(t, np.repeat(np.arange(33), K)[:n], ids.reshape(-1)[:n])
            assert np.array_equal(out.view(np.uint32), sc.reshape(-1)[:n].view(np.uint32)), (n_c, n)


# ---------------------------------------------------------------- 6. batching invariance
@pytest.mark.parametrize('H, P', [(10, 0), (64, 64)])
def test_batching_and_chunking_do_not_change_a_bit(H, P):
    K = 10
    q, qb, c, cb, w = real_inputs(H, P, rng=np.random.default_rng(500 + 17 * H + P))
    rng = np.random.default_rng(H)
    lists = [np.sort(rng.permutation(4099)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(33)]
    off = np.zeros(34, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids_all = np.concatenate(lists)

    def sub(a, b):
        return (off[a:b + 1] - off[a], ids_all[off[a]:off[b]])

    def run(a, b, chunk):
        return topk(Tables(q[a:b], qb[a:b], c, cb, w, H), K, chunk, excl=sub(a, b))

    want = run(0, 33, 0)
    bits = lambda r: (r[0], r[1].view(np.uint32))
    for chunk in (500, 4099, small_chunk(4099)):
        got = run(0, 33, chunk)
        assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want))), chunk
    for chunk in (0, 500):
        halves = [run(a, b, chunk) for a, b in ((0, 17), (17, 33))]
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


@pytest.mark.parametrize('n_p, n_c, H, P', [(1, 65, 3, 0), (17, 4099, 10, 10), (65, 65, 0, 5), (130, 4099, 64, 64),
                                            (130, 65, 9, 7), (17, 4099, 128, 128),
                                            # the target kernel's last 256-thread workgroup exactly full / holding one pair
                                            (256, 65, 3, 5), (257, 65, 10, 0),
                                            # waves of the exclusion kernel's last workgroup without a pair (below)
                                            (5, 257, 10, 10)])
def test_ranks_are_the_count_of_candidates_ahead(n_p, n_c, H, P):
    rng = np.random.default_rng(700 + n_p + n_c + H)
    n_q = 9
    q, qb, c, cb, w = real_inputs(H, P, n_q=n_q, n_c=n_c, rng=rng)
    c[5] = c[3]                                              # exact ties: rows 3 and 5 score alike for every query
    cb[5] = cb[3]
    cb[7] = -np.inf                                          # an ineligible row
    t = Tables(q, qb, c, cb, w, H)
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


# ---------------------------------------------------------------- 8. the models on tests/golden/tiny
def _tiny(mt, stage, tmp_path):
    import oracle
    import reviews4rec_amd
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    root = materialise_tiny(tmp_path)
    extra = {} if stage is None else {'neumf_stage': stage}
    train, test, val, hp = load_data(tiny_hp(mt, root, **extra), device=DEV)
    if stage in ('GMF', 'MLP'):
        W = oracle.init_params(hp, seed=3)
    else:
        W = _weights(_fixture(mt, 'e2e')[1], 'best/')
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(W, strict=True)
    return hp, train, test, model.cuda().eval(), W


def _all_pairs(hp, test, review):
    U, I = hp['total_users'], hp['total_items']
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    if review:
        none = np.full(len(u), -1, np.int64)
        fields = [torch.from_numpy(np.ascontiguousarray(f)) for f in test._review_fields_host(u, i, none, none, none)]
    else:
        fields = [torch.zeros((len(u), 1), dtype=torch.int64) for _ in range(5)]
    return u, i, fields + [torch.from_numpy(u), torch.from_numpy(i)]


@pytest.mark.parametrize('mt, stage', [('deepconn++', None), ('NeuMF', None), ('NeuMF', 'GMF'), ('NeuMF', 'MLP')])
def test_relu_catalogue_on_tiny_against_the_oracle(mt, stage, tmp_path):
    import oracle
    from reviews4rec_amd import ReluCatalogue
    from reviews4rec_amd import main as M
    hp, train, test, model, W = _tiny(mt, stage, tmp_path)
    U, I, K = hp['total_users'], hp['total_items'], 5
    u, i, data = _all_pairs(hp, test, mt == 'deepconn++')
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    cat = ReluCatalogue(model, hp, train)
    eligible = sorted({int(r[1]) for r in train.data})
    assert cat.eligible.tolist() == eligible
    # (a) score_pairs against the float64 oracle forward, within the project's eval tolerance
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    tol = 1e-5 + 1e-5 * np.abs(s64)
    el = np.zeros(I, bool)
    el[eligible] = True
    worst = float((np.abs(got[:, el] - s64[:, el]) / tol[:, el]).max())
    print('%s %s: score_pairs against the oracle, worst |difference| / tolerance = %.3f' % (mt, stage, worst))
    assert (np.abs(got[:, el] - s64[:, el]) <= tol[:, el]).all(), worst
    assert np.isneginf(got[:, ~el]).all()
    # (b) ... and against the package's own forward and the native engine's predict on the same pairs
    dev_data = [d.to(DEV) for d in data]
    engine = M.make_engine(dict(hp, engine='native'), model)
    with torch.no_grad():
        outs = [('forward', model(dev_data))]
        if engine is not None and hasattr(engine, 'predict'):
            outs.append(('predict', torch.cat([engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone()
                                               for a in range(0, U * I, 96)])))
        for name, out in outs:
            mine = out.reshape(U, I).cpu().numpy().astype(np.float64)
            worst = float((np.abs(got[:, el] - mine[:, el]) / tol[:, el]).max())
            print('%s %s: score_pairs against %s, worst |difference| / tolerance = %.3f' % (mt, stage, name, worst))
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
    # candidates= overrides the default set
    few = ReluCatalogue(model, hp, train, candidates=np.array(eligible[:3]))
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


# ---------------------------------------------------------------- 9. engines
def test_pending_idnet_table_updates_are_flushed_first():
    """IdNetEngine's blocked sweeps leave table chunks behind until flush(): ReluCatalogue(engine=engine) must see the
    tables a fresh ReluCatalogue sees after an explicit flush."""
    from reviews4rec_amd import ReluCatalogue
    from test_gpu_span import build, tiny_corpus
    corpus = tiny_corpus(seed=51)
    users = np.arange(300, dtype=np.int64)
    got = []
    for explicit in (False, True):
        hp, reader, model, engine = build('NeuMF', corpus)
        model.train()
        for step, (data, y) in enumerate(reader.iter()):
            engine.train_step(data, y, defer_sweep=True)
            if step == 4:
                break
        assert engine._pending() is not None                  # five steps into a period: updates are pending
        if explicit:
            engine.flush()
            assert engine._pending() is None
        cat = ReluCatalogue(model, hp, reader, engine=None if explicit else engine)
        assert engine._pending() is None
        ids, sc = cat.recommend(users, k=7)
        got.append((ids.cpu(), sc.cpu(), model.mlp_item_embedding.weight.detach().cpu().clone(),
                    model.gmf_item_embedding.weight.detach().cpu().clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert (got[0][0] >= 0).all()


def test_a_recommend_pass_leaves_the_deepconnpp_training_state():
    """Train, recommend and rank, continue == training never interrupted: weights, moments, offset, step_count, bit for
    bit (dropout 0.5: a moved stream would show)."""
    from reviews4rec_amd import ReluCatalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=52)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('deepconn++', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = ReluCatalogue(model, hp, reader, engine=engine, tower_batch=50)
            ids, sc = cat.recommend(np.arange(300), k=5)
            assert (ids[:, 0] >= 0).all() and torch.isfinite(sc[:, 0]).all() and model.training
            items = cat.eligible[np.arange(300) % len(cat.eligible)]
            ranks, rs = cat.rank(np.arange(300), items)
            assert (ranks >= 0).all() and torch.isfinite(rs).all() and model.training
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K


# ---------------------------------------------------------------- 10. main.main
def test_main_serves_deepconnpp_through_both_hooks(tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import ReluCatalogue, eval_catalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    mt = 'deepconn++'
    meta, z = _fixture(mt, 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    hp = tiny_hp(mt, root, log_file=str(tmp_path / 'log'), model_path=str(tmp_path / 'model'), recommend_k=3,
                 recommend_path=str(tmp_path / 'lists.npz'), catalogue_metrics_k=[1, 5])
    final = M.main(hp)
    keys = {'cat_HR@1', 'cat_HR@5', 'cat_NDCG@1', 'cat_NDCG@5', 'cat_MRR', 'cat_ranked', 'cat_unranked'}
    assert keys <= set(final) and 'MSE' in final and not any(k.endswith('@10') for k in final)
    assert 'cat_MRR' in open(hp['log_file']).read()
    assert os.path.exists(str(tmp_path / 'lists.npz'))
    train, test, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(torch.load(hp['model_path'], map_location='cpu'))
    cat = ReluCatalogue(model.cuda().eval(), hp, train)
    want = eval_catalogue(model, train, test, hp, ks=[1, 5], catalogue=cat)
    assert set(want) == keys and {k: final[k] for k in keys} == want
    assert want['cat_ranked'] + want['cat_unranked'] == len(test.data)
    f = np.load(str(tmp_path / 'lists.npz'))
    users = np.array(sorted({int(r[0]) for r in train.data}), np.int64)
    assert np.array_equal(f['users'], users) and f['items'].shape == f['scores'].shape == (len(users), 3)
    ids, sc = cat.recommend(users, k=3)
    assert np.array_equal(f['items'], ids.cpu().numpy())
    assert np.array_equal(f['scores'].view(np.uint32), sc.cpu().numpy().view(np.uint32))
