"""NARRE Shapley values (include/r4r.h, "NARRE Shapley values"), the parts that need no GPU: narre_shapley_ref's
coalition form against the permutation definition, the axioms on constructed tables, the coefficients' zero sum, the
mask-from-coalition rule against a literal loop, the condition that keeps the GPU test from being vacuous at every one of
its cases, the header's section and the argument checks of ``NarreCatalogue.shapley``."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from narre_shapley_ref import (CASES, MAX_PLAYERS, build_case, chunks_of, coalition_masks, coefficients, exact_weights,
                               phi_bound, players_of, shapley_by_permutations, shapley_from_values, weights)


@pytest.mark.parametrize('n', range(1, 8))
def test_coalition_form_equals_the_permutation_definition(n):
    g = np.random.default_rng(n)
    for scale in (1.0, 1e-3, 1e4):
        v = g.standard_normal(1 << n) * scale + 3.0
        a, b = shapley_from_values(v, n), shapley_by_permutations(v, n)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(v - v[-1]).max(), (n, scale)
        # values beyond 2^n are not read
        assert np.array_equal(shapley_from_values(np.concatenate([v, [np.nan] * 3]), n), a)


def test_axioms_on_constructed_tables():
    n = 5
    c = np.arange(1 << n)
    bit = lambda t: (c >> t) & 1
    g = np.random.default_rng(0)
    # efficiency: the shares add up to v(all) - v(none)
    v = g.standard_normal(1 << n)
    assert abs(shapley_from_values(v, n).sum() - (v[-1] - v[0])) <= 1e-14 * np.abs(v).sum()
    # an additive game: each player's share is its own weight
    wts = np.array([0.5, -2.0, 0.0, 3.25, 1.0])
    v = 7.0 + sum(wts[t] * bit(t) for t in range(n))
    assert np.abs(shapley_from_values(v, n) - wts).max() <= 1e-14
    # the null player (2 changes no value) gets exactly nothing beside the rounding; symmetric players (0, 1) get the same
    v = 2.0 * (bit(0) | bit(1)) + 1.5 * bit(3) * bit(4) - 0.25 * (bit(0) + bit(1)) * bit(3)
    phi = shapley_from_values(v, n)
    assert abs(phi[2]) <= 1e-15 and abs(phi[0] - phi[1]) <= 1e-15 and abs(phi[0]) > 0.1
    assert np.abs(phi - shapley_by_permutations(v, n)).max() <= 1e-14
    # a constant game: nothing at all, whatever the constant (the centred form)
    assert not shapley_from_values(np.full(1 << n, 1e9), n).any()
    # n = 1: phi = v(1) - v(0); n = 0: no player
    assert shapley_from_values([2.0, 5.0], 1).tolist() == [3.0] and shapley_from_values([4.0], 0).shape == (0,)


@pytest.mark.parametrize('n', range(1, MAX_PLAYERS + 1))
def test_the_coefficients_of_a_player_sum_to_zero(n):
    a = exact_weights(n)
    assert a[0] == 0 and a[n + 1] == 0 and len(a) == n + 2
    comb = [1]
    for k in range(1, n):
        comb.append(comb[-1] * (n - k) // k)                  # C(n - 1, k)
    # t in c with |c| = k: C(n - 1, k - 1) coalitions; t not in c with |c| = k: C(n - 1, k)
    inside = sum(comb[k - 1] * a[k] for k in range(1, n + 1))
    outside = sum(comb[k] * a[k + 1] for k in range(0, n))
    assert inside == 1 and outside == 1 and inside - outside == Fraction(0)
    for k in range(1, n + 1):                                 # the kernel's form: 1 / (n C(n - 1, k - 1)), one division
        assert a[k] == Fraction(1, n * comb[k - 1]) and weights(n)[k] == 1.0 / (n * comb[k - 1])
    if n <= 12:
        coef = coefficients(n)
        assert coef.shape == (n, 1 << n) and np.abs(coef.sum(1)).max() <= (1 << n) * 2.0 ** -53
        assert np.abs(np.abs(coef).sum(1) - 2.0).max() <= (1 << n) * 2.0 ** -52
    assert chunks_of(n) == max(1, (1 << n) // 1024)


def test_masks_from_coalitions_against_a_literal_loop():
    g = np.random.default_rng(3)
    seen = set()
    for trial in range(200):
        S_u, S_i = int(g.integers(1, 65)), int(g.integers(1, 65))
        P = int(g.integers(1, 9))
        rnd = lambda: int.from_bytes(g.bytes(8), 'little')    # 64 random bits; the ands thin them out
        start_u, start_i = rnd() & rnd() & rnd(), rnd() & rnd() & rnd()
        play_u, play_i = rnd() & rnd(), rnd() & rnd() & rnd()
        if trial % 3 == 0:
            play_u |= start_u                                 # bits shared with start
        if trial % 5 == 0:
            play_i = 0
        n, n_u, mu, mi = coalition_masks(start_u, start_i, play_u, play_i, S_u, S_i, P)
        # the literal rule
        su, si = start_u & ((1 << S_u) - 1), start_i & ((1 << S_i) - 1)
        slots_u = [s for s in range(S_u) if (play_u >> s) & 1 and not (start_u >> s) & 1]
        slots_i = [s for s in range(S_i) if (play_i >> s) & 1 and not (start_i >> s) & 1]
        players = ([('u', s) for s in slots_u] + [('i', s) for s in slots_i])[:P]
        assert n == len(players) <= P and n_u == sum(1 for side, _ in players if side == 'u')
        assert players_of(start_u, start_i, play_u, play_i, S_u, S_i, P)[2] == [(0 if a == 'u' else 1, s) for a, s in players]
        assert len(mu) == len(mi) == 1 << n
        for c in range(1 << n):
            a, b = su, si
            for t, (side, s) in enumerate(players):
                if not (c >> t) & 1:                          # player t is absent: its slot is removed
                    if side == 'u':
                        a |= 1 << s
                    else:
                        b |= 1 << s
            assert int(mu[c]) & ((1 << 64) - 1) == a and int(mi[c]) & ((1 << 64) - 1) == b, (trial, c)
        assert int(mu[-1]) & ((1 << 64) - 1) == su and int(mi[-1]) & ((1 << 64) - 1) == si      # every player present
        seen.add((n == P and len(slots_u) + len(slots_i) > P, n_u == 0, n_u == n))
    assert {s[0] for s in seen} == {True, False} and any(s[1] for s in seen) and any(s[2] for s in seen)


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_gpu_cases_are_not_vacuous(name):
    """``build_case`` asserts it; here once more in words: at least half of the case's players carry a float64 share
    of more than 1,000 of their own bounds, and the sum of a pair's shares is what its players carry together."""
    d = build_case(name)
    strong, players = d['strong']
    print('%s: %d of %d players above 1,000 bounds' % (name, strong, players))
    assert 2 * strong >= players > 0
    for k, r in d['ref'].items():
        assert r['values'].shape == (1 << r['n'],) and r['phi'].shape == (r['n'],)
        bound, M = phi_bound(r['values'], r['n'])
        assert (bound <= 1.3e-7 * M + 1e-44).all()             # 2 ulp of fp32 and a little: the float64 terms are small
        if r['n']:
            assert abs(r['phi'].sum() - (r['values'][-1] - r['values'][0])) <= 1e-12 * max(M.max(), 1e-30)
    specs = list(CASES.values())
    assert {s['shape'][4] for s in specs} >= {8, 16, 17, 32, 33, 48, 49, 64}
    assert {s['shape'][0] for s in specs} >= {1, 2, 3, 10}
    assert {sum(p) for s in specs for p in s['players'][:min(s['n_p'], 12)]} >= {0, 1, 2, 4, 5, 9, 10, 11, 12, 16}
    assert {p for s in specs for p in s['players']} >= {(1, 1), (3, 2), (10, 6), (0, 5)}


# ---------------------------------------------------------------- the header and the library
@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


ARGS = ('z_u logit_u own_u z_pad_u logit_pad_u n_u S_u R_u z_i logit_i own_i z_pad_i logit_pad_i n_i S_i R_i u_idx i_idx '
        'start_u start_i play_u play_i P n_p q_bias c_bias W1 b1 w L out_phi_u out_phi_i out_base out_empty out_n '
        'out_values scratch stream').split()


def test_the_library_exports_the_symbol_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib, ops
    decls = _lib.parse_header()
    ints = dict(n_u=ctypes.c_int64, n_i=ctypes.c_int64, n_p=ctypes.c_int64, L=ctypes.c_int, S_u=ctypes.c_int,
                R_u=ctypes.c_int, S_i=ctypes.c_int, R_i=ctypes.c_int, P=ctypes.c_int, logit_pad_u=ctypes.c_float,
                logit_pad_i=ctypes.c_float)
    name = 'r4r_narre_shapley'
    assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
    assert decls[name][2] == ARGS
    for arg, t in zip(decls[name][2], decls[name][1]):
        assert t is ints.get(arg, ctypes.c_void_p), (name, arg)
    assert ops.NARRE_SHAPLEY_MAX_PLAYERS == MAX_PLAYERS == 16
    text = open(_lib.HEADER_PATH).read()
    assert text.index(' * NARRE counterfactual search:') < text.index(' * NARRE Shapley values:') < text.index(' * What-if documents:')
    section = text[text.index(' * NARRE Shapley values:'):text.index(' * What-if documents:')]
    for cite in ('NARRE.py:53-64', 'NARRE.py:38-46, 115-124', 'data.py:144-172', 'data.py:275-279', 'PRESENT',
                 'ascending chunk order', 'No float atomics', 'rounded to fp32 once', '+0.0f'):
        assert cite in section, cite


# ---------------------------------------------------------------- the catalogue's argument checks
def _many_reviews(cat, per):
    """The bare catalogue's five owners a side with ``per`` reviews each."""
    import types
    pool = types.SimpleNamespace(first=np.arange(6, dtype=np.int64) * per, owners=5)
    cat.reader = types.SimpleNamespace(store=types.SimpleNamespace(users=pool, items=pool))


def test_shapley_checks_its_arguments_before_anything_runs():
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(reviews4rec_amd.NarreCatalogue, 'NARRE')       # five owners a side, one review each; a flush raises
    cat.dev = torch.device('cpu')
    assert reviews4rec_amd.Shapley._fields == ('phi_user', 'phi_item', 'base', 'empty_user', 'empty_item', 'live_user',
                                               'live_item', 'values')
    reached = pytest.raises(AssertionError, match='flushed before')      # every check passed: the pass would start
    for side in ('items', None, 'pair', 0):
        with pytest.raises(ValueError, match='side'):
            cat.shapley([0, 1], [2, 3], side=side)
    for side in ('user', 'item'):
        with pytest.raises(ValueError, match='joint'):
            cat.shapley([0, 1], [2, 3], side=side, joint=True)
    with pytest.raises(ValueError, match='2 users against 1 items'):
        cat.shapley([0, 1], [0])
    for users, items in (([0], [5]), ([-1], [0]), ([7], [0])):
        with pytest.raises(KeyError):
            cat.shapley(users, items)
    for kw in (dict(), dict(side='user'), dict(side='item', slide=False), dict(joint=True), dict(values=True)):
        with reached:
            cat.shapley([0, 1], [2, 3], **kw)
    with reached:
        cat.deletion_curve([0, 1], [2, 3], by='shapley')
    with pytest.raises(ValueError, match="'rev', 'attention', 'shapley'"):
        cat.deletion_curve([0, 1], [2, 3], by='gradient')
    # ten reviews an owner: a joint game would have 20 players
    _many_reviews(cat, 10)
    with pytest.raises(ValueError, match='at most 16 players.*has 20'):
        cat.shapley([0, 1], [2, 3], joint=True)
    for kw in (dict(), dict(side='user'), dict(side='item')):  # the one-side games have 10
        with reached:
            cat.shapley([0, 1], [2, 3], **kw)
    _many_reviews(cat, 8)                                      # 16 players: the limit itself
    with reached:
        cat.shapley([0, 1], [2, 3], joint=True)
    # every other class refuses, with the reason and the way out
    for cls, mt in (('Catalogue', 'deepconn'), ('ReluCatalogue', 'deepconn++'), ('TransNetCatalogue', 'transnet++'),
                    ('MFCatalogue', 'MF')):
        other = _bare(getattr(reviews4rec_amd, cls), mt)
        with pytest.raises(RuntimeError, match='new document.*leave_one_out'):
            other.shapley([0], [0])
