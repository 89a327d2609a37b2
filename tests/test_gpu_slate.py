"""Slates on the device: r4r_slate_topk_<form> / r4r_slate_rank_<form> (csrc/slate_device.h, include/r4r.h "Slates") for
the five score forms.

Nothing here has a tolerance.  The reference is the fp32 BITS r4r_pair_<form> returns for every (query row, candidate)
pair, computed once per form, head and catalogue size and shared: a list is the host sort of its slate's entries by
(score descending, id ascending) with the entries dropped that the header drops (ids outside [0, n_c), ids excluded for
the slate's query row, scores of -inf or NaN), a rank is the host count of the entries other than the target ahead of
it.  A slate that is the whole catalogue must give r4r_topk_<form>'s and r4r_rank_<form>'s results bit for bit.

Heads: the form's shape on tests/golden/tiny and its largest instantiation (for relu: NeuMF on tiny, H = P = 6, which
that file's EXACT does not list; the others are listed in each file's EXACT); dot at D = 0, 5 and 256."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_mf_catalogue as PFM
import test_gpu_narre_catalogue as HMLP
import test_gpu_relu_catalogue as RELU
import test_gpu_transnet_catalogue as RFM
from test_gpu_rank import random_lists
from test_gpu_recommend import dyadic

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_Q = 33
TIED = 40                           # candidates of an exact case that share one row: equal bits by construction


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the dot form's tables and calls (the others: their files')
class DotTables:
    """The inputs on the device; c with a row stride of D + pad (the pad holds NaN)."""

    def __init__(self, q, qb, c, cb, pad=3):
        self.n_q, self.D = q.shape
        self.n_c, self.stride = c.shape[0], self.D + pad
        self.c = torch.full((max(self.n_c, 1), self.stride), float('nan'), dtype=torch.float32, device=DEV)
        if self.n_c and self.D:
            self.c[:self.n_c, :self.D] = _dev(c)
        self.q = _dev(q.reshape(-1) if self.D else np.zeros(1, np.float32))
        self.qb, self.cb = _dev(qb), _dev(cb)

    def head(self):
        from reviews4rec_amd._lib import ptr
        return (ptr(self.q), self.n_q, ptr(self.qb), ptr(self.c), self.n_c, self.stride, ptr(self.cb), self.D)


def _excl(excl):
    if excl is None:
        return None, None
    return _dev(excl[0]), _dev(np.concatenate([excl[1], np.zeros(1, np.int64)]))


class DOT:
    Tables = DotTables

    @staticmethod
    def real_inputs(D, n_q=N_Q, n_c=4099):
        rng = np.random.default_rng(100 + D)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        return f(n_q, D), (4 + f(n_q)).astype(np.float32), f(n_c, D), (0.3 * f(n_c)).astype(np.float32)

    @staticmethod
    def exact_inputs(rng, n_q, n_c, D):
        return (dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c, D), 0.125, 1.0),
                dyadic(rng, (n_c,), 1 / 64, 0.25))

    @staticmethod
    def pairs(t, qi, ci):
        from reviews4rec_amd import _lib
        from reviews4rec_amd._lib import ptr
        qd, cd = _dev(qi.astype(np.int64)), _dev(ci.astype(np.int64))
        out = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
        _lib.call('r4r_pair_dot', *t.head(), ptr(qd), ptr(cd), len(qi), ptr(out))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    @staticmethod
    def topk(t, K, chunk=0, excl=None):
        from reviews4rec_amd import _lib
        from reviews4rec_amd._lib import ptr
        eo, ei = _excl(excl)
        ids = torch.full((t.n_q, K), -7, dtype=torch.int64, device=DEV)
        sc = torch.full((t.n_q, K), 7.0, dtype=torch.float32, device=DEV)
        nb = _lib.lib().r4r_topk_dot_ws_bytes(t.n_q, t.n_c, K, chunk)
        ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
        _lib.call('r4r_topk_dot', *t.head(), ptr(eo), ptr(ei), K, chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))
        torch.cuda.synchronize()
        return ids.cpu().numpy(), sc.cpu().numpy()

    @staticmethod
    def rank(t, qi, ti, chunk=0, excl=None):
        from reviews4rec_amd import _lib
        from reviews4rec_amd._lib import ptr
        eo, ei = _excl(excl)
        qd, td = _dev(qi.astype(np.int64)), _dev(ti.astype(np.int64))
        r = torch.full((len(qi),), -7, dtype=torch.int64, device=DEV)
        s = torch.full((len(qi),), 7.0, dtype=torch.float32, device=DEV)
        _lib.call('r4r_rank_dot', *t.head(), ptr(qd), ptr(td), len(qi), ptr(eo), ptr(ei), chunk, ptr(r), ptr(s))
        torch.cuda.synchronize()
        return r.cpu().numpy(), s.cpu().numpy()


# form -> (its file, the trailing arguments of Tables after the inputs: a function of the shape)
FORMS = {
    'dot': (DOT, lambda sh: ()),
    'relu': (RELU, lambda sh: (sh[0],)),
    'hmlp': (HMLP, lambda sh: ()),
    'rfm': (RFM, lambda sh: (sh[0],)),
    'pfm': (PFM, lambda sh: (sh[0],)),
}
HEADS = [('dot', (0,)), ('dot', (5,)), ('dot', (256,)),
         ('relu', (6, 6)), ('relu', (128, 128)),
         ('hmlp', (6, 6)), ('hmlp', (64, 64)),
         ('rfm', (6, 0, 15)), ('rfm', (64, 16, 80)),
         ('pfm', (6, 6, 12)), ('pfm', (64, 64, 128))]
HEAD_IDS = ['%s-%s' % (f, 'x'.join(map(str, sh))) for f, sh in HEADS]
heads = pytest.mark.parametrize('form, shape', HEADS, ids=HEAD_IDS)


def test_the_heads_are_tinys_and_the_largest_of_each_files_exact_cases():
    assert {k[2:4] for k in RELU.EXACT} >= {(128, 128)} and {k[2:4] for k in HMLP.EXACT} >= {(6, 6), (64, 64)}
    assert {k[2:5] for k in RFM.EXACT} >= {(6, 0, 15), (64, 16, 80)} and {k[2:5] for k in PFM.EXACT} >= {(6, 6, 12), (64, 64, 128)}


# ---------------------------------------------------------------- the calls under test
def slate_topk(form, t, q_idx, off, ids, K, max_len=None, excl=None, n_s=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    n_s = len(q_idx) if n_s is None else n_s
    max_len = int(np.diff(off).max()) if max_len is None and len(off) > 1 else int(max_len or 0)
    eo, ei = _excl(excl)
    qd, od, idd = _dev(np.asarray(q_idx, np.int64)), _dev(off), _dev(np.concatenate([ids, np.zeros(1, np.int64)]))
    out_i = torch.full((len(q_idx), K), -7, dtype=torch.int64, device=DEV)
    out_s = torch.full((len(q_idx), K), 7.0, dtype=torch.float32, device=DEV)
    nb = _lib.lib().r4r_slate_ws_bytes(n_s, max_len, K)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_slate_topk_' + form, *t.head(), ptr(qd), ptr(od), ptr(idd), n_s, max_len, ptr(eo), ptr(ei), K, ptr(ws),
              int(nb), ptr(out_i), ptr(out_s))
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_s.cpu().numpy()


def slate_rank(form, t, q_idx, t_idx, off, ids, max_len=None, excl=None, n_p=None):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    n_p = len(q_idx) if n_p is None else n_p
    max_len = int(np.diff(off).max()) if max_len is None and len(off) > 1 else int(max_len or 0)
    eo, ei = _excl(excl)
    qd, td = _dev(np.asarray(q_idx, np.int64)), _dev(np.asarray(t_idx, np.int64))
    od, idd = _dev(off), _dev(np.concatenate([ids, np.zeros(1, np.int64)]))
    r = torch.full((len(q_idx),), -7, dtype=torch.int64, device=DEV)
    s = torch.full((len(q_idx),), 7.0, dtype=torch.float32, device=DEV)
    _lib.call('r4r_slate_rank_' + form, *t.head(), ptr(qd), ptr(td), ptr(od), ptr(idd), n_p, max_len, ptr(eo), ptr(ei),
              ptr(r), ptr(s))
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy()


# ---------------------------------------------------------------- the reference, on the host over the pair bits
def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, np.concatenate([np.asarray(l, np.int64) for l in lists] + [np.zeros(0, np.int64)])


def _counted(S, u, entries, excl):
    """The entries of a slate of query row u that are listed / counted, and their scores."""
    e = np.asarray(entries, np.int64)
    e = e[(e >= 0) & (e < S.shape[1])]
    if excl is not None:
        e = e[~np.isin(e, excl[1][excl[0][u]:excl[0][u + 1]])]
    with np.errstate(invalid='ignore'):
        e = e[S[u, e] > -np.inf]                               # (false for NaN)
    return e, S[u, e].astype(np.float64)


def ref_lists(S, q_idx, lists, K, excl=None):
    ids = np.full((len(lists), K), -1, np.int64)
    sc = np.full((len(lists), K), -np.inf, np.float32)
    for s, (u, entries) in enumerate(zip(q_idx, lists)):
        e, v = _counted(S, u, entries, excl)
        top = np.lexsort((e, -v))[:K]
        ids[s, :len(top)], sc[s, :len(top)] = e[top], S[u, e[top]]
    return ids, sc


def ref_ranks(S, q_idx, t_idx, lists, excl=None):
    out = np.empty(len(lists), np.int64)
    for p, (u, t, entries) in enumerate(zip(q_idx, t_idx, lists)):
        st = float(S[u, t])
        if not st > -np.inf:
            out[p] = -1
            continue
        e, v = _counted(S, u, entries, excl)
        v, e = v[e != t], e[e != t]
        out[p] = int(((v > st) | ((v == st) & (e < t))).sum())
    return out


@functools.lru_cache(maxsize=None)
def case(form, shape, n_c, exact=False):
    """Tables, every pair's bits [N_Q, n_c], exclusion lists and slates of one form, head and catalogue size: computed
    once, shared, never modified."""
    from reviews4rec_amd import _lib
    mod, extra = FORMS[form]
    rng = np.random.default_rng(1000 * n_c + 7 * sum(shape) + len(form) + (1 if exact else 0))
    tied = np.sort(rng.permutation(n_c)[:TIED])
    if exact:
        # dyadic tables (plenty of ties by arithmetic), and TIED candidates that are ONE row with one bias far above the
        # others': the same bits for every query whatever the chain, at the top of every list that holds them
        inputs = list(mod.exact_inputs(rng, N_Q, n_c, *shape))
        inputs[2], inputs[3] = np.array(inputs[2]), np.array(inputs[3])
        inputs[2][tied], inputs[3][tied] = inputs[2][tied[0]], 2.0 ** 20
    else:
        inputs = [np.array(a) for a in mod.real_inputs(*shape, n_q=N_Q, n_c=n_c)]
    cb = np.array(inputs[3])
    dead = rng.random(n_c) < 0.1
    dead[tied] &= not exact
    cb[dead] = -np.inf                                         # a tenth of the rows is ineligible
    inputs[3] = cb
    t = mod.Tables(*inputs, *extra(shape))
    S = mod.pairs(t, np.repeat(np.arange(N_Q), n_c), np.tile(np.arange(n_c), N_Q)).reshape(N_Q, n_c)
    excl = random_lists(rng, N_Q, n_c)
    P = _lib.lib().r4r_slate_piece()
    # two slates of every length, over ids that reach past both ends of the catalogue; several slates per query row
    universe = np.arange(-70, max(n_c, 4099) + 70)
    lengths = [0, 1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1, 4099]
    lists = [rng.permutation(universe)[:n].astype(np.int64) for n in lengths + lengths[::-1]]
    q_idx = rng.integers(0, N_Q, len(lists))
    q_idx[1], q_idx[2] = q_idx[0], q_idx[0]
    u_all = int(np.argmax(np.diff(excl[0])))                   # ... and one slate whose every entry is excluded
    lists.append(excl[1][excl[0][u_all]:excl[0][u_all + 1]].copy())
    q_idx = np.append(q_idx, u_all)
    S.setflags(write=False)
    return dict(t=t, S=S, excl=excl, lists=lists, q_idx=q_idx, P=P, cb=cb, tied=tied)


def check_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5].tolist())
    assert np.array_equal(bits(got[1]), bits(want[1])), what


# ---------------------------------------------------------------- 1. lists against the pair bits
@pytest.mark.parametrize('n_c', [4099, 257])
@heads
def test_lists_are_the_host_sort_of_the_pair_bits(form, shape, n_c):
    k = case(form, shape, n_c)
    t, S, lists, q_idx = k['t'], k['S'], k['lists'], k['q_idx']
    off, ids = csr(lists)
    assert len(lists[-1]) > 0 and (np.diff(off) > 128).any() and (np.diff(off) < 5).any()
    for K in (1, 5, 10, 128):
        for excl in (None, k['excl']):
            want = ref_lists(S, q_idx, lists, K, excl)
            got = slate_topk(form, t, q_idx, off, ids, K, excl=excl)
            check_lists(got, want, (K, excl is not None))
            assert ((got[0] == -1) == np.isneginf(got[1])).all()                       # unused slots: (-1, -inf)
            assert (got[0][0] == -1).all()                                             # the empty slate
            if excl is not None:
                assert (got[0][-1] == -1).all()                                        # every entry excluded
            elif K == 128:
                assert (got[0][-1] >= 0).any() and (got[0] == -1).any() and (got[0][:, -1] >= 0).any()
    # 1, 3, 4, 5 slates.  Slates 2 .. 6 are single pieces: four of them fill the four waves of one workgroup, five leave
    # the last workgroup one wave; from slate 7 on a call has several pieces per slate
    assert max(len(l) for l in lists[2:7]) <= k['P'] < len(lists[7])
    want = ref_lists(S, q_idx, lists, 10, k['excl'])
    for first, n_s in ((4, 1), (7, 3), (2, 4), (2, 5), (8, 4)):
        sub = lists[first:first + n_s]
        got = slate_topk(form, t, q_idx[first:first + n_s], *csr(sub), 10, excl=k['excl'])
        check_lists(got, (want[0][first:first + n_s], want[1][first:first + n_s]), ('n_s', n_s))


# ---------------------------------------------------------------- 2. exact ties
@heads
def test_exact_ties_are_ordered_by_ascending_id(form, shape):
    """Dyadic inputs, and TIED candidates with the same bits by construction, spread evenly over each slate: equal
    scores in different lanes and in different pieces.  The order among them must be by ascending id."""
    n_c = 4099
    k = case(form, shape, n_c, True)
    t, S, P, tied = k['t'], k['S'], k['P'], k['tied']
    rng = np.random.default_rng(11)
    others = np.setdiff1d(np.arange(n_c), tied)
    lists = []
    for n in (65, P + 1, 2 * P + 1, 4099, 4099):
        m = min(TIED, n // 2)
        l = np.empty(n, np.int64)
        at = np.linspace(0, n - 1, m).astype(np.int64)         # (distinct: n >= 2 m)
        l[at] = rng.permutation(tied)[:m]
        l[np.setdiff1d(np.arange(n), at)] = rng.permutation(others)[:n - m]
        lists.append(l)
    q_idx = rng.integers(0, N_Q, len(lists))
    off, ids = csr(lists)
    for K in (10, 128):
        want = ref_lists(S, q_idx, lists, K)
        for s, l in enumerate(lists):                          # on the reference alone: the ties are there, and spread
            m = min(TIED, len(l) // 2, K)
            assert np.isin(want[0][s, :m], tied).all() and (np.diff(want[0][s, :m]) > 0).all()
            assert len(set(bits(want[1][s, :m]).tolist())) == 1
            where = np.nonzero(np.isin(l, want[0][s, :m]))[0]
            assert len(set((where % 64).tolist())) > 1 and (len(l) <= 2 * P or len(set((where // P).tolist())) > 1)
        check_lists(slate_topk(form, t, q_idx, off, ids, K), want, K)
    ti = np.array([l[np.isin(l, tied)][-1] for l in lists])    # a tied target: the ties with a lower id are ahead of it
    want = ref_ranks(S, q_idx, ti, lists)
    assert (want > 0).any()
    got = slate_rank(form, t, q_idx, ti, off, ids)
    assert np.array_equal(got[0], want)


# ---------------------------------------------------------------- 3. the whole catalogue as a slate
@heads
def test_a_whole_catalogue_slate_gives_the_scans_lists_and_ranks(form, shape):
    n_c = 4099
    k = case(form, shape, n_c)
    mod, t = FORMS[form][0], k['t']
    off = np.arange(N_Q + 1, dtype=np.int64) * n_c
    ids = np.tile(np.arange(n_c, dtype=np.int64), N_Q)
    rows = np.arange(N_Q)
    rng = np.random.default_rng(3)
    n_p = 40
    qi, ti = rng.integers(0, N_Q, n_p), rng.choice(np.nonzero(np.isfinite(k['cb']))[0], n_p)
    ti[:4] = np.nonzero(np.isneginf(k['cb']))[0][:4]            # unranked targets
    p_off = np.arange(n_p + 1, dtype=np.int64) * n_c
    p_ids = np.tile(np.arange(n_c, dtype=np.int64), n_p)
    for excl in (None, k['excl']):
        for K in (10, 128):
            want = mod.topk(t, K, 0, excl)
            assert (want[0] >= 0).all()
            check_lists(slate_topk(form, t, rows, off, ids, K, excl=excl), want, (K, excl is not None))
        want = mod.rank(t, qi, ti, 0, excl)
        got = slate_rank(form, t, qi, ti, p_off, p_ids, excl=excl)
        assert (want[0][:4] == -1).all() and (want[0][4:] >= 0).all()
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), excl is not None


# ---------------------------------------------------------------- 4. ranks against the host count
@pytest.mark.parametrize('n_c', [4099, 257])
@heads
def test_ranks_are_the_host_count_over_the_pair_bits(form, shape, n_c):
    k = case(form, shape, n_c)
    t, S, lists, q_idx = k['t'], k['S'], k['lists'], k['q_idx']
    off, ids = csr(lists)
    rng = np.random.default_rng(5)
    live = np.nonzero(np.isfinite(k['cb']))[0]
    dead = np.nonzero(np.isneginf(k['cb']))[0]
    ti = rng.choice(live, len(lists))                                                  # mostly not in the slate
    inside = [s for s, l in enumerate(lists) if len(np.intersect1d(l, live))]
    for s in inside[::2]:
        ti[s] = rng.choice(np.intersect1d(lists[s], live))                             # a target that is in its slate
    ti[3], ti[5] = dead[0], dead[1]                                                    # targets at -inf
    for excl in (None, k['excl']):
        want = ref_ranks(S, q_idx, ti, lists, excl)
        got = slate_rank(form, t, q_idx, ti, off, ids, excl=excl)
        assert np.array_equal(got[0], want), (excl is not None, np.argwhere(got[0] != want)[:5].ravel())
        assert np.array_equal(bits(got[1]), bits(S[q_idx, ti]))
        assert want[3] == want[5] == -1 and want[0] == 0 and (want > 0).any()        # -inf: -1; the empty slate: 0
    assert any(ti[s] in lists[s] for s in inside) and any(ti[s] not in lists[s] for s in range(len(lists)))
    # 1, 3, 4, 5 pairs (slates 2 .. 6 are single pieces: one full workgroup, and one wave in the last)
    want = ref_ranks(S, q_idx, ti, lists, k['excl'])
    for first, n_p in ((9, 1), (7, 3), (2, 4), (2, 5), (8, 4)):
        sl = slice(first, first + n_p)
        got = slate_rank(form, t, q_idx[sl], ti[sl], *csr(lists[sl]), excl=k['excl'])
        assert np.array_equal(got[0], want[sl]), n_p


# ---------------------------------------------------------------- 5. what the results do not depend on
@heads
def test_results_depend_on_the_inputs_only(form, shape):
    k = case(form, shape, 4099)
    t, lists, q_idx, excl = k['t'], k['lists'], k['q_idx'], k['excl']
    off, ids = csr(lists)
    longest = int(np.diff(off).max())
    rng = np.random.default_rng(9)
    ti = rng.integers(0, 4099, len(lists))
    want_l = slate_topk(form, t, q_idx, off, ids, 10, excl=excl)
    want_r = slate_rank(form, t, q_idx, ti, off, ids, excl=excl)

    def same(got_l, got_r, what):
        check_lists(got_l, want_l, what)
        assert np.array_equal(got_r[0], want_r[0]) and np.array_equal(bits(got_r[1]), bits(want_r[1])), what

    for max_len in (1, longest, 3 * longest):                  # understated, exact, overstated
        same(slate_topk(form, t, q_idx, off, ids, 10, max_len=max_len, excl=excl),
             slate_rank(form, t, q_idx, ti, off, ids, max_len=max_len, excl=excl), ('max_len', max_len))
    mixed = csr([rng.permutation(l) for l in lists])
    same(slate_topk(form, t, q_idx, *mixed, 10, excl=excl), slate_rank(form, t, q_idx, ti, *mixed, excl=excl), 'permuted')
    h = 9
    halves_l = [slate_topk(form, t, q_idx[a], *csr(lists[a]), 10, excl=excl) for a in (slice(0, h), slice(h, None))]
    halves_r = [slate_rank(form, t, q_idx[a], ti[a], *csr(lists[a]), excl=excl) for a in (slice(0, h), slice(h, None))]
    cat = lambda parts: tuple(np.concatenate([p[j] for p in parts]) for j in (0, 1))
    same(cat(halves_l), cat(halves_r), 'two calls')
    # a K-th best that only the rounds past the first piece hold: max_len = 1 with K = 128
    check_lists(slate_topk(form, t, q_idx, off, ids, 128, max_len=1, excl=excl),
                slate_topk(form, t, q_idx, off, ids, 128, excl=excl), 'K = 128, understated')


# ---------------------------------------------------------------- 6. outputs
@pytest.mark.parametrize('form', sorted(FORMS))
def test_calls_without_slates_leave_the_outputs_untouched(form):
    shape = [sh for f, sh in HEADS if f == form][1]
    k = case(form, shape, 257)
    t, lists, q_idx = k['t'], k['lists'], k['q_idx']
    off, ids = csr(lists)
    got = slate_topk(form, t, q_idx, off, ids, 10, n_s=0)
    assert (got[0] == -7).all() and (got[1] == 7.0).all()
    got = slate_rank(form, t, q_idx, np.zeros(len(lists), np.int64), off, ids, n_p=0)
    assert (got[0] == -7).all() and (got[1] == 7.0).all()
    # ... and a call over the first three writes the first three rows only
    got = slate_topk(form, t, q_idx, off, ids, 10, n_s=3)
    assert (got[0][3:] == -7).all() and (got[1][3:] == 7.0).all() and (got[0][:3] != -7).all()
    got = slate_rank(form, t, q_idx, np.zeros(len(lists), np.int64), off, ids, n_p=3)
    assert (got[0][3:] == -7).all() and (got[1][3:] == 7.0).all() and (got[0][:3] != -7).all()
