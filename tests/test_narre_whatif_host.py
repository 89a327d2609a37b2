"""NARRE what-if scores (include/r4r.h, "NARRE what-if scores"), the parts that need no GPU: narre_whatif_ref's
restatement against a plain float64 NARRE eval forward fed the LOADER's own ``skip``-built inputs (``data._np_reviews`` /
``_np_neighbours``), its bounds against a float32 evaluation in another summation order at every shape and seed
tests/test_gpu_narre_whatif.py uses (the bounds can be met, and the ReLU margins hold there), the mutants the bounds must
catch, every refusal of the two entry points (host addresses that are never dereferenced) and the argument checks of
``NarreCatalogue.what_if`` / ``leave_one_out`` / ``deletion_curve``."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from head_ref import compare
from narre_whatif_ref import (ARGS, BARE_CASES, CASES, CHAIN_CASES, EDGE_SHAPES, LOGIT_CASES, MUTANTS, N_I, N_U, chain_case,
                              edge_case, logit_case, logits_f32, logits_ref, pad_inputs, select, whatif_case, whatif_f32,
                              whatif_f32_of, whatif_ref, whatif_ref_of)

OK, ERR_ARG = 0, -1
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
ALL = N_U * N_I
R, W, L = 10, 6, 5                                          # the loader's neighbour lists are 10 wide: R is 10


# ---------------------------------------------------------------- the reference is the loader's `skip`
class _Side:
    """A synthetic pool whose owners have 0, 1, R - 1, R, R + 1 and 2 R reviews, a stand-in float64 tower (any function
    of a review's W tokens serves: the what-if never looks inside it) and float64 attention parameters."""

    def __init__(self, seed, counts, other_rows):
        from reviews4rec_amd.data import _Pool
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
        reviews = {o: [torch.randint(1, 30, (int(torch.randint(1, 2 * W, (1,), generator=g)),), generator=g).tolist()
                       for _ in range(c)] for o, c in enumerate(counts)}
        self.pool = _Pool(reviews, len(counts))
        self.pad = other_rows - 1                            # total + 1 of the other side
        self.pool.nb = torch.randint(0, other_rows - 1, (len(self.pool.nb),), generator=g).numpy().astype(np.int64)
        self.emb, self.proj, self.shift = rnd(30, 7), rnd(7, L) * 0.5, rnd(L) * 0.1
        self.p = dict(W0=rnd(L, 2 * L) * 0.4, b0=rnd(L) * 0.1, w3=rnd(L) * 0.4, b3=rnd(1), other_table=rnd(other_rows, L),
                      own=rnd(len(counts), L))

    def tower(self, docs):
        """docs int64 [..., W] -> float64 [..., L]; the pad word 0 takes part like any other, as in the real tower."""
        e = self.emb[torch.from_numpy(np.ascontiguousarray(docs))]
        return torch.tanh(e.sum(-2) @ self.proj + (e[..., 0, :] * e[..., -1, :]).sum(-1, keepdim=True)) + self.shift

    def span(self, owner):
        return self.pool.first[owner:owner + 1], self.pool.first[owner + 1:owner + 2]

    def loader_inputs(self, owner, skip):
        """What a training rating of this owner sees with its own review ``skip`` removed (data.py:144-172, 275-279)."""
        from reviews4rec_amd.data import _np_neighbours, _np_reviews
        rb, re = self.span(owner)
        sk = np.array([skip], np.int64)
        return (self.tower(_np_reviews(self.pool.tok, self.pool.rev_off, rb, re, sk, R, W))[0],
                torch.from_numpy(_np_neighbours(self.pool.nb, rb, re, sk, self.pad))[0])

    def slots(self, S):
        """Every owner's first S reviews, nothing removed -> ``whatif_ref``'s side (float64 throughout)."""
        from reviews4rec_amd.data import _np_review_slots
        rb, re = self.pool.first[:-1], self.pool.first[1:]
        docs, nb = _np_review_slots(self.pool.tok, self.pool.rev_off, self.pool.nb, rb, re, 0, S, W, self.pad)
        z, nb = self.tower(docs), torch.from_numpy(nb)
        z_pad = self.tower(np.zeros((W,), np.int64))
        lg = logits_ref(dict(self.p, z=z, nb=nb))['logit'][0]
        lp = logits_ref(dict(self.p, z=z_pad.reshape(1, 1, L), nb=torch.tensor([[self.pad]])))['logit'][0]
        return dict(z=z, logit=lg, z_pad=z_pad, logit_pad=float(lp.reshape(())), R=R, own=self.p['own'])

    def attended(self, z, nb, owner):
        """NARRE.py:53-64 and 115-119 in float64 on explicit lists: z [R, L], nb [R] -> p [L]."""
        p = self.p
        other = p['other_table'][nb]
        logits = torch.relu(torch.cat([z, other], -1) @ p['W0'].T + p['b0']) @ p['w3'] + p['b3']
        return (torch.softmax(logits, 0)[:, None] * z).sum(0) + p['own'][owner]

    def remaining(self, owner, drops):
        """The numpy 'remaining list' restatement: the owner's reviews without ``drops``, the first R, padded."""
        from reviews4rec_amd.data import _np_review_slots
        rb, re = self.span(owner)
        count = int(re[0] - rb[0])
        keep = [r for r in range(count) if r not in drops][:R]
        docs, nb = _np_review_slots(self.pool.tok, self.pool.rev_off, self.pool.nb, rb, re, 0, max(count, 1), W, self.pad)
        z = self.tower(docs)[0]
        rows = [z[r] for r in keep] + [self.tower(np.zeros((W,), np.int64))] * (R - len(keep))
        ids = [int(nb[0, r]) for r in keep] + [self.pad] * (R - len(keep))
        return torch.stack(rows), torch.tensor(ids)


COUNTS = (0, 1, R - 1, R, R + 1, 2 * R)


@pytest.fixture(scope='module')
def world():
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    user, item = _Side(1, COUNTS, len(COUNTS) + 2), _Side(2, COUNTS[::-1], len(COUNTS) + 2)
    head = dict(W1=rnd(L, L) * 0.4, b1=rnd(L) * 0.1, w=rnd(L) * 0.4, q_bias=rnd(len(COUNTS)), c_bias=rnd(len(COUNTS)))
    return user, item, head


def _score(head, pu, pi, u, i):
    """NARRE.py:38-46, 121-124 in float64."""
    return torch.relu((pu * pi) @ head['W1'].T + head['b1']) @ head['w'] + head['q_bias'][u] + head['c_bias'][i]


def test_the_helper_is_the_loader_with_nothing_removed(world):
    from reviews4rec_amd.data import _np_neighbours, _np_review_slots, _np_reviews
    for side in world[:2]:
        pool = side.pool
        rb, re = pool.first[:-1], pool.first[1:]
        none = np.full(len(rb), -1, np.int64)
        docs, nb = _np_review_slots(pool.tok, pool.rev_off, pool.nb, rb, re, 0, 10, W, side.pad)
        assert np.array_equal(docs, _np_reviews(pool.tok, pool.rev_off, rb, re, none, 10, W))
        assert np.array_equal(nb, _np_neighbours(pool.nb, rb, re, none, side.pad))
        more, nb_more = _np_review_slots(pool.tok, pool.rev_off, pool.nb, rb, re, 10, 23, W, side.pad)
        whole = _np_reviews(pool.tok, pool.rev_off, rb, re, none, 23, W)
        assert np.array_equal(more, whole[:, 10:]) and tuple(nb_more.shape) == (len(rb), 13)
        assert int((nb_more != side.pad).sum()) == sum(max(c - 10, 0) for c in (re - rb))
        assert docs.dtype == np.int64 and nb.dtype == np.int64


def test_every_single_skip_is_the_loaders_own_removal(world):
    """For every owner and every single ``skip`` -- on one side, then on both -- the reference with S = R + 1 equals a
    plain float64 NARRE eval forward fed ``_np_reviews`` / ``_np_neighbours`` with that ``skip``."""
    user, item, head = world
    su, si = user.slots(R + 1), item.slots(R + 1)
    n = len(COUNTS)
    checked = 0
    for u, i in itertools.product(range(n), range(n)):
        skips_u = [-1] + list(range(user.pool.first[u + 1] - user.pool.first[u]))
        skips_i = [-1] + list(range(item.pool.first[i + 1] - item.pool.first[i]))
        pairs = [(a, -1) for a in skips_u] + [(-1, b) for b in skips_i] + list(zip(skips_u, skips_i[::-1]))
        mask = lambda s: 0 if s < 0 else 1 << s
        du = torch.tensor([[mask(a) for a, _ in pairs]], dtype=torch.int64)
        di = torch.tensor([[mask(b) for _, b in pairs]], dtype=torch.int64)
        got = whatif_ref(su, si, torch.tensor([u]), torch.tensor([i]), du, di, head['W1'], head['b1'], head['w'],
                         head['q_bias'], head['c_bias'])['score'][0][0]
        for v, (a, b) in enumerate(pairs):
            want = _score(head, user.attended(*user.loader_inputs(u, a), u), item.attended(*item.loader_inputs(i, b), i), u, i)
            assert abs(float(got[v] - want)) <= 1e-12 * max(1.0, abs(float(want))), (u, i, a, b)
            checked += 1
    assert checked > 400


def test_several_drops_are_the_remaining_list(world):
    user, item, head = world
    S = R + 3
    su, si = user.slots(S), item.slots(S)
    drops = [(), (0,), (0, 1, 2), (1, 9, 10), (2, 11, 12), (9, 10, 12), (0, 5, 19), (12,), (3, 4)]
    bits = lambda d: sum(1 << r for r in d)
    for u, i in itertools.product(range(len(COUNTS)), range(len(COUNTS))):
        du = torch.tensor([[bits(d) for d in drops]], dtype=torch.int64)
        di = torch.tensor([[bits(d) for d in drops[::-1]]], dtype=torch.int64)
        got = whatif_ref(su, si, torch.tensor([u]), torch.tensor([i]), du, di, head['W1'], head['b1'], head['w'],
                         head['q_bias'], head['c_bias'])['score'][0][0]
        for v, (a, b) in enumerate(zip(drops, drops[::-1])):
            want = _score(head, user.attended(*user.remaining(u, a), u), item.attended(*item.remaining(i, b), i), u, i)
            assert abs(float(got[v] - want)) <= 1e-12 * max(1.0, abs(float(want))), (u, i, a, b)
    # select() itself, on lists written out by hand
    assert select(np.array([0b0110]), 4, 2).tolist() == [[0, 3]]
    assert select(np.array([0b0111]), 4, 3).tolist() == [[3, 4, 4]]
    assert select(np.array([-1, 1 << 4, -(1 << 63)]), 4, 2).tolist() == [[4, 4], [0, 1], [0, 1]]
    assert select(np.array([-(1 << 63)]), 64, 64)[0].tolist() == list(range(63)) + [64]


# ---------------------------------------------------------------- the bounds can be met, and the margins hold
def test_float32_in_another_order_stays_inside_the_bounds_at_every_gpu_shape():
    """A case's inputs do not depend on n_p, and a pair's masks go with the pair: the twelve pairs are every (pair,
    variant) the GPU test sees.  ``whatif_ref`` and ``logits_ref`` assert the ReLU margins -- of t for EVERY variant."""
    worst = {'logit': 0.0, 'score': 0.0, 'bare': 0.0, 'edge': 0.0, 'chain': 0.0}
    for case in LOGIT_CASES:
        s = logit_case(case)
        worst['logit'] = max(worst['logit'], compare('logits %r' % (case,), logits_f32(s), *logits_ref(s)['logit']))
        compare('pad logit %r' % (case,), logits_f32(pad_inputs(s)), *logits_ref(pad_inputs(s))['logit'])
    for case in CASES:
        d = whatif_case(case, n_p=ALL)
        worst['score'] = max(worst['score'], compare('what-if %r' % (case,), whatif_f32_of(d), *whatif_ref_of(d)['score']))
    for case in BARE_CASES:
        for how in (dict(biases=False, own=False), dict(biases=False), dict(own=False)):
            d = whatif_case(case, n_p=ALL, **how)
            worst['bare'] = max(worst['bare'], compare('bare %r' % (case,), whatif_f32_of(d), *whatif_ref_of(d)['score']))
    for shape in EDGE_SHAPES:
        d = edge_case(*shape)
        worst['edge'] = max(worst['edge'], compare('edge %r' % (shape,), whatif_f32_of(d), *whatif_ref_of(d)['score']))
    for case in CHAIN_CASES:
        d, ref_sides = chain_case(case)
        got_sides = {}
        for name in ('user', 'item'):
            raw = d['raw_' + name]
            got_sides[name] = dict(d[name], logit=logits_f32(raw), logit_pad=float(logits_f32(pad_inputs(raw)).reshape(())))
        rest = [d[k] for k in ARGS[2:]]
        worst['chain'] = max(worst['chain'], compare('chain %r' % (case,), whatif_f32(got_sides['user'], got_sides['item'], *rest),
                                                     *whatif_ref(ref_sides['user'], ref_sides['item'], *rest)['score']))
    assert all(0.0 < v <= 1.0 for v in worst.values()), worst
    print('what-if: worst float32 (numpy, descending order) error / bound: '
          + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


# ---------------------------------------------------------------- the bounds catch wrong formulas
MUTANT_CASES = [(10, 12, 10, 12, 33, 15, 257), (5, 7, 10, 12, 32, 21, 5), (10, 64, 10, 64, 33, 16, 5), (33, 40, 33, 40, 32, 16, 257)]


@pytest.mark.parametrize('case', MUTANT_CASES, ids=lambda c: 'Ru%d-Su%d-Ri%d-Si%d-L%d-V%d-n%d' % c)
@pytest.mark.parametrize('mutant', MUTANTS)
def test_mutants_fall_outside(case, mutant):
    assert case in CASES
    assert set(MUTANTS) == {'no_renorm', 'pad_without_logit', 'no_slide', 'sides_swapped', 'bits_reversed', 'no_own'}
    d = whatif_case(case, n_p=ALL)
    with pytest.raises(AssertionError, match='beyond their bound'):
        compare(mutant, whatif_f32_of(d, mutant), *whatif_ref_of(d)['score'])


# ---------------------------------------------------------------- the entry points' refusals
@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(lib, name, args):
    from reviews4rec_amd import _lib
    names = _lib.parse_header()[name][2]
    assert list(args) == names, (list(args), names)         # the dict IS the header's argument list
    return getattr(lib, name)(*args.values())


def logit_args(**kw):
    a = dict(z=PTR, nb=PTR, other_table=PTR, other_rows=7, W0=PTR, b0=PTR, w3=PTR, b3=PTR, logit=PTR, N=5, S=12, L=32,
             stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def whatif_args(**kw):
    a = dict(z_u=PTR, logit_u=PTR, own_u=PTR, z_pad_u=PTR, logit_pad_u=0.5, n_u=3, S_u=12, R_u=10, z_i=PTR, logit_i=PTR,
             own_i=PTR, z_pad_i=PTR, logit_pad_i=-0.5, n_i=4, S_i=11, R_i=10, u_idx=PTR, i_idx=PTR, drop_u=PTR, drop_i=PTR,
             n_p=7, V=21, q_bias=PTR, c_bias=PTR, W1=PTR, b1=PTR, w=PTR, L=32, out_score=PTR, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def test_the_library_exports_the_symbols_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    ints = dict(other_rows=ctypes.c_int64, N=ctypes.c_int64, n_u=ctypes.c_int64, n_i=ctypes.c_int64, n_p=ctypes.c_int64,
                S=ctypes.c_int, L=ctypes.c_int, V=ctypes.c_int, S_u=ctypes.c_int, R_u=ctypes.c_int, S_i=ctypes.c_int,
                R_i=ctypes.c_int, logit_pad_u=ctypes.c_float, logit_pad_i=ctypes.c_float)
    for name, args in (('r4r_narre_logits', logit_args()), ('r4r_narre_whatif', whatif_args())):
        assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
        assert decls[name][2] == list(args)
        for arg, t in zip(decls[name][2], decls[name][1]):
            assert t is ints.get(arg, ctypes.c_void_p), (name, arg)
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * NARRE what-if scores:'):]
    for cite in ('NARRE.py:53-64', 'NARRE.py:24-36', 'NARRE.py:38-46, 115-124', 'data.py:144-172', 'data.py:275-279',
                 'ascending slot order', 'not on V'):
        assert cite in section, cite


@pytest.mark.parametrize('over, word', [
    (dict(N=-1), b'N='), (dict(other_rows=-1), b'other_rows='), (dict(S=0), b'S='), (dict(S=65), b'S='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(z=None), b'null'), (dict(nb=None), b'null'), (dict(W0=None), b'null'),
    (dict(b0=None), b'null'), (dict(w3=None), b'null'), (dict(b3=None), b'null'), (dict(other_table=None), b'other_table'),
    (dict(logit=None), b'logit'),
])
def test_owner_pass_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_narre_logits', logit_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_logits') and word in msg, (over, got, msg)


@pytest.mark.parametrize('over, word', [
    (dict(S_u=0), b'S_u='), (dict(S_u=65), b'S_u='), (dict(S_i=0), b'S_i='), (dict(S_i=65), b'S_i='),
    (dict(R_u=0), b'R_u='), (dict(R_u=13), b'R_u='), (dict(R_i=0), b'R_i='), (dict(R_i=12), b'R_i='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(V=0), b'V='), (dict(V=-3), b'V='),
    (dict(n_u=-1), b'n_u='), (dict(n_i=-1), b'n_i='), (dict(n_p=-1), b'n_p='), (dict(n_p=1 << 31, V=1), b'n_p='),
    (dict(n_p=(1 << 31) // 21 + 1), b'n_p='),
    (dict(z_u=None), b'z_u'), (dict(logit_u=None), b'logit_u'), (dict(z_pad_u=None), b'z_pad_u'),
    (dict(z_i=None), b'z_i'), (dict(logit_i=None), b'logit_i'), (dict(z_pad_i=None), b'z_pad_i'),
    (dict(u_idx=None), b'null'), (dict(i_idx=None), b'null'), (dict(W1=None), b'null'), (dict(b1=None), b'null'),
    (dict(w=None), b'null'), (dict(out_score=None), b'out_score'), (dict(n_u=0), b'n_u='), (dict(n_i=0), b'n_i='),
])
def test_variant_pass_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_narre_whatif', whatif_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_whatif') and word in msg, (over, got, msg)


def test_nothing_to_do_is_ok_and_enqueues_nothing(lib):
    assert _call(lib, 'r4r_narre_logits', logit_args(N=0)) == OK
    assert _call(lib, 'r4r_narre_logits', logit_args(N=0, z=None, nb=None, W0=None, logit=None, other_table=None)) == OK
    assert _call(lib, 'r4r_narre_logits', logit_args(N=0, L=65)) == ERR_ARG           # the shape is still checked
    assert _call(lib, 'r4r_narre_whatif', whatif_args(n_p=0)) == OK
    nul = {k: None for k, v in whatif_args().items() if v == PTR}
    assert _call(lib, 'r4r_narre_whatif', whatif_args(n_p=0, n_u=0, n_i=0, **nul)) == OK
    assert _call(lib, 'r4r_narre_whatif', whatif_args(n_p=0, R_u=13)) == ERR_ARG
    assert (lib.r4r_last_error() or b'').startswith(b'r4r_narre_whatif')
    # the largest call the limits allow is not refused for its size: n_p V = 2^31 - 1 (no pairs, so nothing runs)
    assert _call(lib, 'r4r_narre_whatif', whatif_args(n_p=0, V=(1 << 31) - 1)) == OK


# ---------------------------------------------------------------- the catalogue's argument checks
def test_what_if_leave_one_out_and_deletion_curve_check_their_arguments_before_anything_runs():
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(reviews4rec_amd.NarreCatalogue, 'NARRE')       # five owners a side, one review each; a flush raises
    cat.dev = torch.device('cpu')
    assert reviews4rec_amd.WhatIf._fields == ('scores', 'base')
    assert reviews4rec_amd.LeaveOneOut._fields == ('base', 'without_user', 'without_item', 'delta_user', 'delta_item',
                                                   'live_user', 'live_item')
    assert reviews4rec_amd.DeletionCurve._fields[:2] == ('scores', 'aopc')
    reached = pytest.raises(AssertionError, match='flushed before')      # every check passed: the pass would start
    for call in (cat.what_if, cat.leave_one_out, cat.deletion_curve):
        with pytest.raises(ValueError, match='2 users against 1 items'):
            call([0, 1], [0])
        for users, items in (([0], [5]), ([-1], [0]), ([7], [0])):
            with pytest.raises(KeyError):
                call(users, items)
        with reached:
            call([0, 1], [2, 3])
    ok = torch.tensor([[1, 0], [0, 1]], dtype=torch.int64)
    bad_drops = ([[0]],                                        # one list for two pairs
                 [[0], [1]], [[0], [-1]], [[0], [64]], [[0], [True]], [[0], [0.0]],     # outside the owner's one review
                 [[0], 0], 'mask', 3,
                 [[[0]], [[0], []]],                           # one variant against two
                 ok.to(torch.int32), ok.to(torch.float32), ok[0], ok[:1], torch.zeros((2, 0), dtype=torch.int64))
    for side in ('drop_user', 'drop_item'):
        for drop in bad_drops:
            with pytest.raises(ValueError, match=side):
                cat.what_if([0, 1], [2, 3], **{side: drop})
        for drop in ([[0], []], [[[0], []], [[], [0]]], ok, ok.numpy(), ([0], [0])):
            with reached:
                cat.what_if([0, 1], [2, 3], **{side: drop})
    with pytest.raises(ValueError, match='2 variants per pair, drop_item 1'):
        cat.what_if([0, 1], [2, 3], drop_user=ok, drop_item=ok[:, :1])
    masks, most = cat._whatif_drops([[[0]], [[]]], torch.tensor([0, 1]), 'user', 'drop_user')
    assert masks.tolist() == [[1], [0]] and most == 1 and masks.dtype == torch.int64
    masks, most = cat._whatif_drops(torch.tensor([[-1, 7]]), torch.tensor([0]), 'item', 'drop_item')
    assert masks.tolist() == [[-1, 7]] and most == 64
    assert cat._whatif_drops(None, torch.tensor([0]), 'item', 'drop_item') == (None, 0)
    for kw in (dict(side='items'), dict(side=None), dict(direction='sideways'), dict(by='gradient'), dict(by=None),
               dict(by=torch.zeros(2, 9)), dict(by=torch.zeros(3, 10)), dict(by=torch.zeros(2, 10, dtype=torch.int64)),
               dict(by=[[0.0] * 10] * 2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cat.deletion_curve([0, 1], [2, 3], **kw)
    for kw in (dict(by='attention'), dict(by='rev', side='item', direction='down'), dict(by=torch.zeros(2, 10)),
               dict(by=np.zeros((2, 10), np.float32))):
        with reached:
            cat.deletion_curve([0, 1], [2, 3], **kw)
