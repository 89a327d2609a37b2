"""NARRE counterfactual search (include/r4r.h, "NARRE counterfactual search"), the parts that need no GPU:
narre_search_ref's greedy rule against narre_whatif_ref's leave-one-out, its prefix property, the selected-only rule, an
exhaustive scan of all masks at S <= 6, the condition that keeps the GPU test's float64 comparison from being vacuous,
every refusal of the entry point (host addresses that are never dereferenced) and the argument checks of
``NarreCatalogue.counterfactual``."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from narre_search_ref import (CASES, F64_CASES, INF, ITEM, NAN, agreement, as_i64, better, case_inputs, scorer32, scorer64,
                              search_inputs, search_of, selected_bits)
from narre_whatif_ref import N_I, N_U

OK, ERR_ARG = 0, -1
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
ALL = N_U * N_I


def test_the_case_lists_hold_what_the_gpu_test_must_see():
    assert {(c[0], c[1]) for c in CASES} | {(c[2], c[3]) for c in CASES} >= {(1, 1), (1, 3), (5, 5), (10, 12), (10, 20),
                                                                          (33, 40), (64, 64)}
    assert any((c[0], c[1]) != (c[2], c[3]) for c in CASES)
    assert {c[4] for c in CASES} == {1, 16, 17, 33, 64}
    assert {c[5] for c in CASES} >= {1, 2, 64} and any(c[5] == c[0] for c in CASES)
    assert {c[6] for c in CASES} == {1, 5, 257}
    assert set(F64_CASES) <= set(CASES)
    for case in CASES:                                        # the owner pass's ReLU margins hold at every case's seed
        assert case_inputs(case, n_p=1)['shape'] == (case[1], case[0], case[3], case[2])
    # the step's comparison: strictly better only, a number over a NaN, a NaN over nothing
    assert better(1.0, None, False) and better(NAN, None, True) and better(2.0, NAN, False) and better(-2.0, NAN, True)
    assert not better(NAN, 1.0, False) and not better(NAN, 1.0, True) and not better(NAN, NAN, False)
    assert better(0.5, 1.0, False) and not better(1.0, 1.0, False) and not better(0.0, -0.0, False)
    assert better(1.5, 1.0, True) and not better(1.0, 1.0, True) and not better(0.5, 1.0, True)
    assert selected_bits(0b0110, 4, 2) == 0b1001 and selected_bits(0, 5, 3) == 0b111 and selected_bits(0b1111, 4, 2) == 0


@pytest.mark.parametrize('direction', (0, 1))
def test_budget_one_is_the_arg_best_of_leave_one_out(direction):
    d = search_inputs(5, 7, 10, 12, 16, ALL)
    fn = scorer64(d)
    got = search_of(fn, d, direction, 1, target=torch.full((ALL,), NAN))
    S_u, R_u, S_i, R_i = d['shape']
    checked = 0
    for p in range(ALL):
        mu, mi = int(d['start_u'][p]) & ((1 << S_u) - 1), int(d['start_i'][p]) & ((1 << S_i) - 1)
        cu, ci = int(d['cand_u'][p]) & ~mu, int(d['cand_i'][p]) & ~mi
        one = [(s, mu | (1 << s), mi) for s in range(S_u) if (selected_bits(mu, S_u, R_u) & cu) >> s & 1]
        one += [(ITEM + s, mu, mi | (1 << s)) for s in range(S_i) if (selected_bits(mi, S_i, R_i) & ci) >> s & 1]
        if not one:
            assert got['steps'][p] == 0 and got['order'][p, 0] == -1
            continue
        u, i = d['u_idx'][p:p + 1].expand(len(one)), d['i_idx'][p:p + 1].expand(len(one))
        sc = fn(u, i, torch.tensor([as_i64(a) for _, a, _ in one]), torch.tensor([as_i64(b) for _, _, b in one]))[0]
        k = int(torch.argmax(sc) if direction else torch.argmin(sc))       # the first of equals: the lowest c
        assert got["order"][p, 0] == one[k][0] and abs(got["scores"][p, 1] - float(sc[k])) <= 1e-12
        checked += 1
    assert checked >= 10


def test_a_search_is_the_prefix_of_the_same_search_with_a_larger_budget():
    d = search_inputs(5, 7, 10, 12, 16, ALL)
    for direction in (0, 1):
        runs = {B: search_of(scorer32(d), d, direction, B) for B in (1, 2, 5, 6)}
        for B, B2 in ((1, 2), (2, 5), (5, 6)):
            a, b = runs[B], runs[B2]
            assert np.array_equal(a['order'], b['order'][:, :B])
            assert np.array_equal(a['scores'], b['scores'][:, :B + 1], equal_nan=True)
            assert np.array_equal(a['steps'], np.minimum(b['steps'], B))
        assert runs[6]['steps'].max() == 6 and runs[6]['steps'].min() == 0


def test_a_slot_outside_the_selected_list_is_never_a_step():
    """S > R and every bit a candidate: each step's slot is among the first R clear slots at that step, and an owner's
    search ends when the budget or the list is used up -- never by walking into the unattended slots first."""
    d = search_inputs(3, 8, 2, 6, 16, ALL)
    every = torch.full((ALL,), -1, dtype=torch.int64)
    none = torch.zeros(ALL, dtype=torch.int64)
    got = search_of(scorer32(d), d, 0, 14, start_u=none, start_i=none, cand_u=every, cand_i=every,
                    target=torch.full((ALL,), -INF))
    assert (got['steps'] == 14).all() and not got['crossed'].any()      # 8 + 6 slots, each removed once
    for p in range(ALL):
        mu = mi = 0
        for c in got['order'][p].tolist():
            if c < ITEM:
                assert (selected_bits(mu, 8, 3) >> c) & 1, (p, c, bin(mu))
                mu |= 1 << c
            else:
                assert (selected_bits(mi, 6, 2) >> (c - ITEM)) & 1, (p, c, bin(mi))
                mi |= 1 << (c - ITEM)
        assert mu == 0xff and mi == 0x3f


@pytest.mark.parametrize('direction', (0, 1))
def test_exhaustive_scan_of_all_masks_at_small_S(direction):
    """S = 6 and 5: all 2^6 x 2^5 mask pairs of every pair scored in float64.  ``steps`` is never below the fewest
    removals that cross, and where ``crossed`` is set the final masks really cross."""
    d = search_inputs(3, 6, 2, 5, 16, ALL, seed=1)            # (seed 0 leaves a pre-activation inside its ReLU margin)
    fn = scorer64(d)
    none = torch.zeros(ALL, dtype=torch.int64)
    every = torch.full((ALL,), -1, dtype=torch.int64)
    masks = list(itertools.product(range(64), range(32)))
    mu = torch.tensor([a for a, _ in masks]), torch.tensor([b for _, b in masks])
    bits = np.array([bin(a).count('1') + bin(b).count('1') for a, b in masks])
    hit = 0
    for p in range(ALL):
        u, i = d['u_idx'][p:p + 1].expand(len(masks)), d['i_idx'][p:p + 1].expand(len(masks))
        sc = fn(u, i, mu[0], mu[1])[0].numpy()
        base = sc[0]
        for shift in (0.05, 0.3, 1.0):
            tgt = base + shift if direction else base - shift
            got = search_of(fn, dict(d, u_idx=d['u_idx'][p:p + 1], i_idx=d['i_idx'][p:p + 1]), direction, 11,
                            start_u=none[:1], start_i=none[:1], cand_u=every[:1], cand_i=every[:1],
                            target=torch.tensor([tgt]))
            ok = sc > tgt if direction else sc < tgt
            least = bits[ok].min() if ok.any() else None
            if got['crossed'][0]:
                assert least is not None and got['steps'][0] >= least
                final = sc[masks.index((got['mask_u'][0], got['mask_i'][0]))]
                assert abs(final - got["scores"][0, got["steps"][0]]) <= 1e-12 and (final > tgt if direction else final < tgt)
                hit += 1
            else:
                assert got['steps'][0] == 11 and got['mask_u'][0] == 63 and got['mask_i'][0] == 31
    assert hit >= 6


def test_float32_in_another_order_picks_the_float64_best():
    """The condition that keeps the GPU test's float64 comparison from being vacuous, at its shapes and seeds: along the
    float64 search, a float32 numpy restatement in ANOTHER summation order picks the float64 best in at least 90 % of
    the steps (and the float64 scorer's ReLU margins hold for every candidate it scores: ``whatif_ref`` asserts them).
    Measured: 281 of 281 steps (down) and 213 of 214 (up) over the six cases."""
    for direction in (0, 1):
        taken = same = 0
        for case in F64_CASES:
            d = case_inputs(case, n_p=ALL)
            _, n, ok = agreement(d, direction, case[5])
            assert n > 0
            taken, same = taken + n, same + ok
        print('direction %d: float32 picks the float64 best in %d of %d steps' % (direction, same, taken))
        assert same >= 0.9 * taken, (direction, same, taken)


# ---------------------------------------------------------------- the entry point's refusals
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


def search_args(**kw):
    a = dict(z_u=PTR, logit_u=PTR, own_u=PTR, z_pad_u=PTR, logit_pad_u=0.5, n_u=3, S_u=12, R_u=10, z_i=PTR, logit_i=PTR,
             own_i=PTR, z_pad_i=PTR, logit_pad_i=-0.5, n_i=4, S_i=11, R_i=10, u_idx=PTR, i_idx=PTR, start_u=PTR,
             start_i=PTR, cand_u=PTR, cand_i=PTR, target=PTR, direction=0, budget=10, n_p=7, q_bias=PTR, c_bias=PTR,
             W1=PTR, b1=PTR, w=PTR, L=32, out_order=PTR, out_scores=PTR, out_steps=PTR, out_crossed=PTR, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def test_the_library_exports_the_symbol_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    ints = dict(n_u=ctypes.c_int64, n_i=ctypes.c_int64, n_p=ctypes.c_int64, L=ctypes.c_int, S_u=ctypes.c_int,
                R_u=ctypes.c_int, S_i=ctypes.c_int, R_i=ctypes.c_int, direction=ctypes.c_int, budget=ctypes.c_int,
                logit_pad_u=ctypes.c_float, logit_pad_i=ctypes.c_float)
    name, args = 'r4r_narre_search', search_args()
    assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
    assert decls[name][2] == list(args)
    for arg, t in zip(decls[name][2], decls[name][1]):
        assert t is ints.get(arg, ctypes.c_void_p), (name, arg)
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * NARRE counterfactual search:'):text.index(' * What-if documents:')]
    for cite in ('NARRE.py:53-64', 'NARRE.py:38-46, 115-124', 'data.py:144-172', 'data.py:275-279', 'CURRENTLY SELECTED',
                 'ties (float ==) to the lowest c', 'prefix'):
        assert cite in section, cite


@pytest.mark.parametrize('over, word', [
    (dict(S_u=0), b'S_u='), (dict(S_u=65), b'S_u='), (dict(S_i=0), b'S_i='), (dict(S_i=65), b'S_i='),
    (dict(R_u=0), b'R_u='), (dict(R_u=13), b'R_u='), (dict(R_i=0), b'R_i='), (dict(R_i=12), b'R_i='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(budget=0), b'budget='), (dict(budget=65), b'budget='),
    (dict(budget=-1), b'budget='), (dict(direction=2), b'direction='), (dict(direction=-1), b'direction='),
    (dict(n_u=-1), b'n_u='), (dict(n_i=-1), b'n_i='), (dict(n_p=-1), b'n_p='), (dict(n_p=1 << 31, budget=1), b'n_p='),
    (dict(n_p=(1 << 31) // 11 + 1), b'n_p='),
    (dict(z_u=None), b'z_u'), (dict(logit_u=None), b'logit_u'), (dict(z_pad_u=None), b'z_pad_u'),
    (dict(z_i=None), b'z_i'), (dict(logit_i=None), b'logit_i'), (dict(z_pad_i=None), b'z_pad_i'),
    (dict(u_idx=None), b'null'), (dict(i_idx=None), b'null'), (dict(target=None), b'target'), (dict(W1=None), b'null'),
    (dict(b1=None), b'null'), (dict(w=None), b'null'), (dict(out_order=None), b'out_order'),
    (dict(out_scores=None), b'out_scores'), (dict(out_steps=None), b'out_steps'), (dict(out_crossed=None), b'out_crossed'),
    (dict(n_u=0), b'n_u='), (dict(n_i=0), b'n_i='),
])
def test_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_narre_search', search_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_search') and word in msg, (over, got, msg)


def test_nothing_to_do_is_ok_and_enqueues_nothing(lib):
    assert _call(lib, 'r4r_narre_search', search_args(n_p=0)) == OK
    nul = {k: None for k, v in search_args().items() if v == PTR}
    assert _call(lib, 'r4r_narre_search', search_args(n_p=0, n_u=0, n_i=0, **nul)) == OK
    assert _call(lib, 'r4r_narre_search', search_args(n_p=0, R_u=13)) == ERR_ARG      # the shape is still checked
    assert _call(lib, 'r4r_narre_search', search_args(n_p=0, budget=65)) == ERR_ARG
    assert (lib.r4r_last_error() or b'').startswith(b'r4r_narre_search')


# ---------------------------------------------------------------- the catalogue's argument checks
def test_counterfactual_checks_its_arguments_before_anything_runs():
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(reviews4rec_amd.NarreCatalogue, 'NARRE')       # five owners a side, one review each; a flush raises
    cat.dev = torch.device('cpu')
    assert reviews4rec_amd.Counterfactual._fields == ('removed_user', 'removed_item', 'order', 'scores', 'steps',
                                                      'crossed', 'base', 'target')
    for cls in ('Catalogue', 'ReluCatalogue', 'TransNetCatalogue'):
        assert not hasattr(getattr(reviews4rec_amd, cls), 'counterfactual')
    reached = pytest.raises(AssertionError, match='flushed before')      # every check passed: the pass would start
    with pytest.raises(ValueError, match='2 users against 1 items'):
        cat.counterfactual([0, 1], [0], target=3.0)
    for users, items in (([0], [5]), ([-1], [0]), ([7], [0])):
        with pytest.raises(KeyError):
            cat.counterfactual(users, items, target=3.0)
    for kw, word in ((dict(), 'exactly one of target and k'), (dict(target=3.0, k=2), 'exactly one of target and k'),
                     (dict(k=0, side='item'), 'k = 0'), (dict(k=128, side='item'), 'k = 128'),
                     (dict(k=True, side='item'), 'k = True'), (dict(k=2.0, side='item'), 'k = 2.0'),
                     (dict(k=3), 'every item'), (dict(k=3, side='user'), 'every item'),
                     (dict(k=3, side='item', direction='up'), "direction='down' only"),
                     (dict(target=3.0, side='items'), 'side'), (dict(target=3.0, side=None), 'side'),
                     (dict(target=3.0, direction='sideways'), 'direction'),
                     (dict(target=3.0, budget=0), 'budget'), (dict(target=3.0, budget=65), 'budget'),
                     (dict(target=3.0, budget=2.0), 'budget'), (dict(target=3.0, budget=True), 'budget'),
                     (dict(target=torch.zeros(3)), 'target holds 3 values for 2 pairs'),
                     (dict(target='high'), 'target must be'), (dict(target=True), 'target must be')):
        with pytest.raises(ValueError, match=word):
            cat.counterfactual([0, 1], [2, 3], **kw)
    for kw in (dict(target=3.0), dict(target=torch.tensor([1.0, 2.0]), direction='up', side='user', budget=64),
               dict(target=np.array([1.0, NAN]), slide=False, budget=1), dict(target=[1.0, 2.0], side='item'),
               dict(k=1, side='item'), dict(k=127, side='item', budget=3)):
        with reached:
            cat.counterfactual([0, 1], [2, 3], **kw)
