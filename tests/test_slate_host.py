"""Slates (include/r4r.h, "Slates"), the parts that need no GPU: the refusals, sizes and constants of
r4r_slate_topk_<form> / r4r_slate_rank_<form>, recommend.slates_csr, recommend.sample_negatives (its uniformity against a
bound derived here, not measured) and eval.eval_sampled's bookkeeping over a stand-in catalogue."""
import ctypes

import numpy as np
import pytest
import torch

FORMS = ('dot', 'relu', 'hmlp', 'rfm', 'pfm')
# the head arguments of a form after (q, n_q, q_bias, c, n_c, c_stride): names, well-formed values (p = a pointer), and
# one width past its limit
HEADS = {
    'dot': (('c_bias', 'D'), dict(D=8), dict(D=257, c_stride=300)),
    'relu': (('c_bias', 'w', 'H', 'P'), dict(H=4, P=4), dict(H=129, c_stride=300)),
    'hmlp': (('c_bias', 'W', 'b', 'w', 'D', 'H'), dict(D=8, H=8), dict(H=65)),
    'rfm': (('c_bias', 'W', 'b', 's', 'l', 'H', 'P', 'M'), dict(H=4, P=4, M=8), dict(M=81)),
    'pfm': (('c_bias', 'W', 'b', 's', 'g', 'e', 'H', 'G', 'M'), dict(H=4, G=4, M=8), dict(M=129)),
}


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(lib, kind, form, **kw):
    """r4r_slate_<kind>_<form> with well-formed defaults (host addresses: every refusal precedes the first
    dereference) -> (rc, message, the buffer every pointer points at)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    names, ints, _ = HEADS[form]
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, q_idx=p, t_idx=p, slate_off=p, slate_ids=p, n_s=7, n_p=7,
             max_len=1000, excl_off=None, excl_ids=None, K=10, ws=p, ws_bytes=1 << 40, out_ids=p, out_scores=p, out_rank=p,
             out_score=p)
    a.update({k: p for k in names})
    a.update(ints)
    a.update(kw)
    head = [a[k] for k in ('q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride') + names]
    if kind == 'topk':
        tail = [a[k] for k in ('q_idx', 'slate_off', 'slate_ids', 'n_s', 'max_len', 'excl_off', 'excl_ids', 'K', 'ws',
                               'ws_bytes', 'out_ids', 'out_scores')]
    else:
        tail = [a[k] for k in ('q_idx', 't_idx', 'slate_off', 'slate_ids', 'n_p', 'max_len', 'excl_off', 'excl_ids',
                               'out_rank', 'out_score')]
    rc = getattr(lib, 'r4r_slate_%s_%s' % (kind, form))(*head, *tail, None)
    return rc, lib.r4r_last_error() or b'', buf


def test_symbols_are_declared_exported_and_take_the_pair_calls_head(lib):
    from reviews4rec_amd import _lib
    decl = _lib.parse_header()
    assert decl['r4r_slate_piece'][0] is ctypes.c_int and decl['r4r_slate_piece'][2] == []
    assert decl['r4r_slate_ws_bytes'][0] is ctypes.c_size_t and decl['r4r_slate_ws_bytes'][2] == ['n_s', 'max_len', 'K']
    for form in FORMS:
        pair = decl['r4r_pair_' + form][2]
        head = pair[:pair.index('q_idx')]
        assert head[6:] == list(HEADS[form][0])
        assert decl['r4r_slate_topk_' + form][2] == head + [
            'q_idx', 'slate_off', 'slate_ids', 'n_s', 'max_len', 'excl_off', 'excl_ids', 'K', 'ws', 'ws_bytes', 'out_ids',
            'out_scores', 'stream']
        assert decl['r4r_slate_rank_' + form][2] == head + [
            'q_idx', 't_idx', 'slate_off', 'slate_ids', 'n_p', 'max_len', 'excl_off', 'excl_ids', 'out_rank', 'out_score',
            'stream']
        assert hasattr(lib, 'r4r_slate_topk_' + form) and hasattr(lib, 'r4r_slate_rank_' + form)
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * Slates:'):]
    assert 'eval.py:64-92' in section and 'data.py:375-447' in section


def test_sizes_and_constants(lib):
    piece = lib.r4r_slate_piece()
    assert piece >= 64 and piece % 64 == 0
    for K in (1, 10, 128):
        for max_len in (0, 1, piece - 1, piece):
            assert lib.r4r_slate_ws_bytes(1000, max_len, K) == 0
        assert lib.r4r_slate_ws_bytes(1000, piece + 1, K) == 1000 * 2 * K * 12
        assert lib.r4r_slate_ws_bytes(7, 4099, K) == 7 * -(-4099 // piece) * K * 12
        assert lib.r4r_slate_ws_bytes(1 << 20, 3 * piece, K) == (1 << 20) * 3 * K * 12
    assert lib.r4r_slate_ws_bytes(0, 4099, 10) == 0


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('kind', ['topk', 'rank'])
def test_refusals_need_no_gpu(lib, kind, form):
    n = 'n_s' if kind == 'topk' else 'n_p'
    outs = ('out_ids', 'out_scores') if kind == 'topk' else ('out_rank', 'out_score')
    name = ('slate_%s_%s' % (kind, form)).encode()
    keep = ctypes.create_string_buffer(16)
    cases = [({n: -1}, b'negative'), (dict(max_len=-1), b'negative'), (dict(n_q=-1), b'negative'), (dict(n_c=-1), b'negative'),
             (dict(q_idx=None), b'null'), (dict(slate_off=None), b'null'), (dict(slate_ids=None), b'null'),
             ({outs[0]: None}, b'output'), ({outs[1]: None}, b'output'),
             (dict(excl_off=ctypes.addressof(keep)), b'excl'), (dict(excl_ids=ctypes.addressof(keep)), b'excl'),
             (dict(n_q=0), b'empty'), (dict(c_stride=7), b'c_stride'),
             ({n: 1 << 31}, b'grid'), ({n: 1 << 30, 'max_len': 1 << 20}, b'grid'),
             (HEADS[form][2], list(HEADS[form][2])[0].encode())]
    if kind == 'topk':
        cases += [(dict(K=0), b'K'), (dict(K=129), b'K')]
    else:
        cases += [(dict(t_idx=None), b'null')]
    for kw, word in cases:
        rc, msg, buf = _call(lib, kind, form, **kw)
        assert rc == -1 and word in msg and msg.startswith(name), (kw, rc, msg)
        assert buf.raw == b'\0' * 64                         # (no GPU here: a launch would have failed otherwise)


@pytest.mark.parametrize('form', FORMS)
def test_a_workspace_one_byte_short_is_refused_as_such(lib, form):
    R4R_ERR_WORKSPACE = -3
    piece = lib.r4r_slate_piece()
    need = lib.r4r_slate_ws_bytes(7, piece + 1, 10)
    assert need == 7 * 2 * 10 * 12
    rc, msg, buf = _call(lib, 'topk', form, max_len=piece + 1, ws_bytes=need - 1)
    assert rc == R4R_ERR_WORKSPACE and b'workspace' in msg and msg.startswith(b'slate_topk_' + form.encode()), (rc, msg)
    assert buf.raw == b'\0' * 64
    rc, msg, _ = _call(lib, 'topk', form, max_len=piece + 1, ws=None)
    assert rc == R4R_ERR_WORKSPACE and b'workspace' in msg
    # a single piece needs none
    rc, msg, _ = _call(lib, 'topk', form, max_len=piece, ws=None, ws_bytes=0, n_s=0)
    assert rc == 0, msg


@pytest.mark.parametrize('form', FORMS)
def test_nothing_to_do_is_ok_with_null_pointers(lib, form):
    nul = dict(q_idx=None, t_idx=None, slate_off=None, slate_ids=None, ws=None, ws_bytes=0, out_ids=None, out_scores=None,
               out_rank=None, out_score=None)
    for kind, n in (('topk', 'n_s'), ('rank', 'n_p')):
        for kw in ({n: 0}, dict({n: 0}, **nul), dict({n: 0}, n_q=0, **nul), dict(n_c=0)):
            rc, msg, buf = _call(lib, kind, form, **kw)
            assert rc == 0, (kind, kw, msg)
            assert buf.raw == b'\0' * 64


# ---------------------------------------------------------------- slates_csr
def test_slates_csr_takes_a_padded_block_and_a_csr():
    import reviews4rec_amd
    from reviews4rec_amd.recommend import slates_csr
    assert reviews4rec_amd.slates_csr is slates_csr
    block = np.array([[5, 3, -1, 9], [-1, -1, -1, -1], [0, 1, 2, 3], [-7, 8, -1, -1]])
    want_off, want_ids = [0, 3, 3, 7, 8], [5, 3, 9, 0, 1, 2, 3, 8]
    for given in (block, torch.from_numpy(block), block.astype(np.int32), block.tolist(),
                  (np.array(want_off), np.array(want_ids)), (want_off, torch.tensor(want_ids))):
        off, ids, longest = slates_csr(given, 4, 10)
        assert off.dtype == np.int64 and ids.dtype == np.int64 and isinstance(longest, int)
        assert off.tolist() == want_off and ids.tolist() == want_ids and longest == 4
    off, ids, longest = slates_csr(np.zeros((3, 0), np.int64), 3, 10)
    assert off.tolist() == [0, 0, 0, 0] and len(ids) == 0 and longest == 0
    for nothing in (([0], []), np.zeros((0, 4), np.int64), []):
        off, ids, longest = slates_csr(nothing, 0, 10)
        assert off.tolist() == [0] and len(ids) == 0 and longest == 0
    # the same id in two slates is no repeat
    assert slates_csr(np.array([[1, 2], [2, 1]]), 2, 3)[2] == 2


@pytest.mark.parametrize('given, n, word', [
    (np.array([[1, 2, 1]]), 1, 'repeated'), (([0, 2, 5], [4, 3, 7, 3, 7]), 2, 'repeated'),
    (np.array([[1, 10]]), 1, 'outside'), (([0, 1], [-1]), 1, 'outside'), (([0, 1], [10]), 1, 'outside'),
    (np.array([[1, 2], [3, 4]]), 3, 'rows'), (([0, 1, 2], [1, 2]), 3, 'rows'),
    (([0, 2, 1], [1, 2]), 2, 'ascend'), (([0, 1, 3], [1, 2]), 2, 'ascend'), (np.array([1, 2, 3]), 3, '2-D'),
    (np.array([[0.5, 1.0]]), 1, 'integer'),
])
def test_slates_csr_refuses(given, n, word):
    from reviews4rec_amd.recommend import slates_csr
    with pytest.raises(ValueError, match=word):
        slates_csr(given, n, 10)


# ---------------------------------------------------------------- sample_negatives
def _seen(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, np.array([i for l in lists for i in sorted(l)], np.int64)


def test_sample_negatives_draws_distinct_unseen_eligible_ids():
    import reviews4rec_amd
    from reviews4rec_amd.recommend import sample_negatives, slates_csr
    assert reviews4rec_amd.sample_negatives is sample_negatives
    rng = np.random.default_rng(0)
    n_items, n_users, N = 500, 40, 20
    eligible = np.sort(rng.permutation(n_items)[:300])
    lists = [set(rng.permutation(n_items)[:rng.integers(0, 60)].tolist()) for _ in range(n_users)]
    lists[3] = set(eligible[:290].tolist())                    # a pool of 10 (9 where the positive is in it): below N
    lists[4] = set(eligible.tolist())                          # an empty pool
    seen = _seen(lists)
    users = np.concatenate([rng.integers(0, n_users, 400), [3, 3, 4, 4]])
    items = np.concatenate([rng.choice(eligible, 400), [eligible[295], eligible[0], eligible[7], 499]])
    off, ids = sample_negatives(users, items, eligible, seen, N, seed=5)
    assert off.dtype == np.int64 and ids.dtype == np.int64 and off[0] == 0 and off[-1] == len(ids)
    slates_csr((off, ids), len(users), n_items)                # distinct, in range
    el = set(eligible.tolist())
    for p, (u, i) in enumerate(zip(users.tolist(), items.tolist())):
        s = ids[off[p]:off[p + 1]]
        pool = el - lists[u] - {i}
        assert (np.diff(s) > 0).all() and set(s.tolist()) <= pool, p
        assert len(s) == min(N, len(pool)), (p, len(s), len(pool))
    assert [int(off[p + 1] - off[p]) for p in range(400, 404)] == [9, 10, 0, 0]
    assert (np.diff(off)[:400] == N).sum() > 300
    # a function of its arguments only
    again = sample_negatives(users.tolist(), torch.from_numpy(items), eligible, seen, N, seed=5)
    assert np.array_equal(again[0], off) and np.array_equal(again[1], ids)
    other = sample_negatives(users, items, eligible, seen, N, seed=6)
    assert np.array_equal(other[0], off) and not np.array_equal(other[1], ids)
    # nothing asked for, nobody asking
    off0, ids0 = sample_negatives(users, items, eligible, seen, 0, seed=5)
    assert off0.tolist() == [0] * (len(users) + 1) and len(ids0) == 0
    off0, ids0 = sample_negatives([], [], eligible, seen, N, seed=5)
    assert off0.tolist() == [0] and len(ids0) == 0


def test_sample_negatives_is_uniform_over_the_pool():
    """One user, a pool of 9 ids, N = 4, n = 20,000 rows: a pool id is in a row's slate with probability 4 / 9,
    independently over the rows, so its count is Binomial(n, 4 / 9): mean n N / 9 = 8888.9, sigma = sqrt(n 4/9 5/9) =
    70.3.  Every count within 6 sigma (a false alarm: below 2e-8 over the nine ids) -- a condition on the sampler
    derived here, not measured.  The pool is a small part of the eligible ids, so most draws are rejected: the
    rejection must not favour any id either."""
    from reviews4rec_amd.recommend import sample_negatives
    eligible = np.arange(0, 60, 2)                             # 30 ids
    pool = np.array([4, 10, 12, 26, 30, 38, 44, 52, 58])
    positive = 20
    seen = _seen([set(), sorted(set(eligible.tolist()) - set(pool.tolist()) - {positive})])
    n, N = 20000, 4
    off, ids = sample_negatives(np.ones(n, np.int64), np.full(n, positive), eligible, seen, N, seed=11)
    assert (np.diff(off) == N).all()
    counts = np.bincount(ids, minlength=60)
    assert counts.sum() == counts[pool].sum() == n * N
    mean, sigma = n * N / 9.0, np.sqrt(n * (N / 9.0) * (1 - N / 9.0))
    assert (np.abs(counts[pool] - mean) <= 6 * sigma).all(), (counts[pool], mean, sigma)


# ---------------------------------------------------------------- eval_sampled
class _Reader:
    def __init__(self, data, negs=None):
        self.data, self.negs = data, negs


class _FixedCatalogue:
    """Catalogue's surface as eval_sampled uses it, with the ranks given."""

    def __init__(self, ranks, eligible, seen):
        self.ranks, self.eligible, self.seen, self.calls = ranks, np.asarray(eligible, np.int64), seen, []

    def rank_among(self, users, items, slates, exclude_seen=True):
        self.calls.append((np.asarray(users).tolist(), np.asarray(items).tolist(), slates, exclude_seen))
        return torch.tensor(self.ranks, dtype=torch.int64), torch.zeros(len(self.ranks))


def test_eval_sampled_over_given_ranks():
    import reviews4rec_amd
    from reviews4rec_amd.eval import eval_sampled
    from reviews4rec_amd.recommend import sample_negatives
    assert reviews4rec_amd.eval_sampled is eval_sampled
    test = _Reader(np.array([[3, 7, 5.0], [3, 8, 1.0], [0, 2, 4.0], [1, 2, 4.0], [5, 5, 2.0], [6, 1, 3.0]]))
    eligible = np.arange(12)
    seen = _seen([set(), set(range(10)), set(), {0, 1}, set(), set(), set(range(12))])   # users 1 and 6: pools of 2 and 0
    cat = _FixedCatalogue([0, 1, 4, 9, 10, -1], eligible, seen)
    m = eval_sampled(None, None, test, {}, n_negatives=3, seed=1, catalogue=cat)
    assert len(cat.calls) == 1                                                          # ONE rank_among call
    users, items, slates, exclude = cat.calls[0]
    assert users == [3, 3, 0, 1, 5, 6] and items == [7, 8, 2, 2, 5, 1] and exclude is False
    want = sample_negatives(np.array(users), np.array(items), eligible, seen, 3, 1)
    assert np.array_equal(slates[0], want[0]) and np.array_equal(slates[1], want[1])
    assert np.diff(want[0]).tolist() == [3, 3, 3, 2, 3, 0]
    assert set(m) == {'samp_HR@1', 'samp_HR@5', 'samp_HR@10', 'samp_NDCG@1', 'samp_NDCG@5', 'samp_NDCG@10', 'samp_MRR',
                      'samp_ranked', 'samp_unranked', 'samp_short'}
    assert (m['samp_HR@1'], m['samp_HR@5'], m['samp_HR@10']) == (20.0, 60.0, 80.0)
    assert m['samp_NDCG@10'] == 46.14 and m['samp_MRR'] == 37.82                        # percent, two places, like cat_*
    assert m['samp_ranked'] == 5 and m['samp_unranked'] == 1 and m['samp_short'] == 2
    assert set(eval_sampled(None, None, test, {}, n_negatives=3, ks=[3], catalogue=cat)) == {
        'samp_HR@3', 'samp_NDCG@3', 'samp_MRR', 'samp_ranked', 'samp_unranked', 'samp_short'}
    with pytest.raises(ZeroDivisionError):                                              # like eval.py:90
        eval_sampled(None, None, _Reader(test.data[:2]), {}, catalogue=_FixedCatalogue([-1, -1], eligible, seen))
    with pytest.raises(ValueError):
        eval_sampled(None, None, test, {}, catalogue=cat, negatives='other')


def test_eval_sampled_takes_the_datasets_own_negatives():
    from reviews4rec_amd.eval import eval_sampled
    negs = {4: ([9, 2], [1, 3, 5, 7, 11]), 0: ([6], [8, 8, 6, 2, 0]), 2: ([1], [0, 2, 3, 4, 5])}
    cat = _FixedCatalogue([0, 3, -1], np.arange(12), _seen([set()] * 5))
    m = eval_sampled(None, None, _Reader(None, negs), {}, ks=(1,), catalogue=cat, negatives='dataset')
    users, items, (off, ids), exclude = cat.calls[0]
    assert users == [4, 0, 2] and items == [9, 6, 1] and exclude is False
    assert off.tolist() == [0, 5, 8, 13] and ids.tolist() == [1, 3, 5, 7, 11, 0, 2, 8, 0, 2, 3, 4, 5]
    assert m == {'samp_HR@1': 50.0, 'samp_NDCG@1': 50.0, 'samp_MRR': 62.5, 'samp_ranked': 2, 'samp_unranked': 1,
                 'samp_short': 1}
