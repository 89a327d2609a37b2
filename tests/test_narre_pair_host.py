"""NARRE pair gradients (include/r4r.h, "NARRE pair gradients"), the parts that need no GPU: narre_pair_ref's closed
forms against torch.autograd in float64 through a plain restatement of NARRE.py's eval forward composed with the tower
fc, its bounds against a float32 evaluation in another summation order at every shape and seed
tests/test_gpu_narre_pair.py uses (the bounds can be met, and the ReLU margins hold there), the mutants the bounds must
catch, every refusal of the two entry points (host addresses that are never dereferenced) and ``explain_words``'
per-review weights."""
import ctypes

import pytest
import torch

from head_ref import attention_ref, compare_all
from narre_pair_ref import (MUTANTS, N_I, N_U, OWNER_CASES, PAIR_CASES, PAIR_OUTPUTS, gather_other, owner_case,
                            owner_f32, owner_inputs, owner_ref, pair_case, pair_f32_of, pair_inputs, pair_ref, pair_ref_of,
                            side_of, with_zero_slot)

OK, ERR_ARG = 0, -1
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
ALL = N_U * N_I


# ---------------------------------------------------------------- the closed forms are the gradients
def _forward64(raw, pooled, fc_bias):
    """NARRE.py:95-119 for one side in float64: pooled [N, R, F] -> (p [N, L], z, logits)."""
    f = lambda t: t.to(torch.float64)
    z = pooled @ f(raw['fc']).T + fc_bias                                       # TextCNN's fc (eval: no dropout)
    cat_input = torch.cat([z, gather_other(raw['other_table'], raw['nb'])], dim=-1)
    hidden = torch.relu(cat_input @ f(raw['W0']).T + f(raw['b0']))
    logits = hidden @ f(raw['w3']).reshape(-1) + f(raw['b3']).reshape(())
    scores = torch.softmax(logits, dim=-1)
    return torch.sum(scores.unsqueeze(-1) * z, dim=1) + f(raw['own_table'])[raw['owner']], z, logits


@pytest.mark.parametrize('R_u, R_i, L, F', [(1, 1, 7, 9), (5, 10, 7, 9), (10, 10, 33, 100), (64, 5, 64, 112)])
def test_the_closed_forms_equal_autograd_in_float64(R_u, R_i, L, F):
    d = pair_inputs(R_u, R_i, L, F, n_p=ALL)
    f = lambda t: t.to(torch.float64)
    g = torch.Generator().manual_seed(5)
    sides, leaves = {}, {}
    for name, raw, R in (('user', d['raw_user'], R_u), ('item', d['raw_item'], R_i)):
        N = raw['z'].shape[0]
        bias = torch.randn(L, generator=g, dtype=torch.float64)
        # pooled features whose latents ARE the case's z: the least-squares preimage, then z recomputed from it
        pooled = torch.linalg.lstsq(f(raw['fc']), (f(raw['z']) - bias).reshape(N * R, L).T).solution.T.reshape(N, R, F)
        pooled = pooled.clone().requires_grad_()
        p, z, logits = _forward64(raw, pooled, bias)
        leaves[name] = (pooled, p, z, logits)
        ref = owner_ref(dict(raw, z=z.detach()))
        sides[name] = side_of(ref, raw, bounds=False)           # (values alone: autograd has no roundings to carry)
        # the owner pass: D_r is d logit_r / d z_r
        for n in range(N):
            for r in range(R):
                gz, = torch.autograd.grad(logits[n, r], z, retain_graph=True)
                assert float((gz[n, r] - ref['D'][0][n, r]).abs().max()) <= 1e-12 * max(1.0, float(gz.abs().max()))
                rest = gz.clone()
                rest[n, r] = 0.0
                assert float(rest.abs().max()) == 0.0           # a slot's logit depends on that slot's latent only
        assert float((ref['E'][0] - ref['D'][0] @ f(raw['fc'])).abs().max()) <= 1e-12
        assert float((ref['dz'][0] - (ref['D'][0] * z.detach()).sum(-1)).abs().max()) <= 1e-12
    u, i = d['u_idx'], d['i_idx']
    ref = pair_ref(sides['user'], sides['item'], u, i, d['W1'], d['b1'], d['w'], d['q_bias'], d['c_bias'])
    (pool_u, p_u, z_u, lg_u), (pool_i, p_i, z_i, lg_i) = leaves['user'], leaves['item']
    for n in range(ALL):
        un, in_ = int(u[n]), int(i[n])
        cat = p_u[un] * p_i[in_]                                                # NARRE.py:122-124
        rating = torch.relu(cat @ f(d['W1']).T + f(d['b1'])) @ f(d['w']).reshape(-1)
        score = rating + f(d['q_bias'])[un] + f(d['c_bias'])[in_]
        grads = torch.autograd.grad(score, [pool_u, pool_i, p_u, p_i, z_u, z_i, lg_u, lg_i], retain_graph=True)
        gpu, gpi, gp_u, gp_i, gz_u, gz_i, gl_u, gl_i = grads
        want = dict(score=score.detach(), w_user=gpu[un], w_item=gpi[in_], g_user=gp_u[un], g_item=gp_i[in_],
                    rev_user=(gz_u[un] * z_u[un].detach()).sum(-1), rev_item=(gz_i[in_] * z_i[in_].detach()).sum(-1),
                    glogit_user=gl_u[un], glogit_item=gl_i[in_])
        assert set(want) == set(PAIR_OUTPUTS)
        for name, val in want.items():
            got = ref[name][0][n]
            assert float((got - val).abs().max()) <= 1e-12 * max(1.0, float(val.abs().max())), (name, n)
        others = torch.arange(N_U) != un
        assert float(gpu[others].abs().max()) == 0.0
    for name in ('glogit_user', 'glogit_item'):                                  # sum_r delta_r = 0, within its bound
        val, bound = ref[name]
        assert bool((val.sum(1).abs() <= bound.sum(1)).all()), name


def test_the_attention_part_carries_attention_refs_bounds():
    """owner_ref's a and o are head_ref.attention_ref's a_save and out, values and bounds."""
    raw = owner_inputs(0, 5, 10, 33, 100)
    ref = owner_ref(raw)
    other = gather_other(raw['other_table'], raw['nb'])
    att = attention_ref(raw['z'], other, raw['W0'], raw['b0'], raw['w3'].reshape(1, -1), raw['b3'], None,
                        torch.zeros(5, 33))
    for mine, theirs in (('attn', 'a_save'), ('pooled_attn', 'out')):
        assert torch.equal(ref[mine][0], att[theirs][0]) and torch.equal(ref[mine][1], att[theirs][1]), mine


# ---------------------------------------------------------------- the bounds can be met, and the margins hold
def test_float32_in_another_order_stays_inside_the_owner_bounds_at_every_gpu_shape():
    """``owner_ref`` asserts the ReLU margins of every case, as it is and with ``with_zero_slot``."""
    worst, each = 0.0, {}
    for case in OWNER_CASES:
        for s in (owner_case(case), with_zero_slot(owner_case(case))):
            worst = max(worst, compare_all('owner %r' % (case,), owner_f32(s), owner_ref(s), each=each))
    assert 0.0 < worst <= 1.0
    print('owner pass: worst float32 (numpy, descending order) error / bound %.3f' % worst)


def test_float32_in_another_order_stays_inside_the_pair_bounds_at_every_gpu_shape():
    """The inputs of a case do not depend on n_p and the indices past the first twelve repeat the twelve pairs, so the
    twelve pairs are every pair the GPU test sees; ``pair_ref`` and ``owner_ref`` assert the ReLU margins."""
    worst = {}
    for case in PAIR_CASES:
        for biases in (True, False):
            d = pair_case(case, n_p=ALL, biases=biases)
            each = {}
            compare_all('pair %r' % (case,), pair_f32_of(d), pair_ref_of(d), each=each)
            for k, v in each.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(PAIR_OUTPUTS) and 0.0 < max(worst.values()) <= 1.0
    print('pair pass: worst float32 (numpy, descending order) error / bound: '
          + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize('R_u, R_i, L, F, seed', [(10, 10, 8, 100, 0), (5, 10, 7, 9, 0), (1, 3, 16, 64, 0)])
def test_the_bounds_carried_from_pass_to_pass_hold_for_the_chain(R_u, R_i, L, F, seed):
    """The composition a catalogue runs: the float32 owner pass feeding the float32 pair pass, against the float64 chain
    with the owner pass's bounds carried into the pair pass (``side_of``).  The carried bounds are first-order worst
    cases and grow with L: the shapes are the small ones the catalogue test on tests/golden/tiny meets."""
    from narre_pair_ref import pair_f32
    d = pair_inputs(R_u, R_i, L, F, n_p=ALL, seed=seed)
    got_sides, ref_sides = [], []
    for raw in (d['raw_user'], d['raw_item']):
        o32, o64 = owner_f32(raw), owner_ref(raw)
        got_sides.append(dict(p=o32['out'], z=raw['z'], attn=o32['attn'], E=o32['E'], dz=o32['dz'], fc=raw['fc']))
        ref_sides.append(side_of(o64, raw))
    args = (d['u_idx'], d['i_idx'], d['W1'], d['b1'], d['w'], d['q_bias'], d['c_bias'])
    worst = compare_all('chain', pair_f32(got_sides[0], got_sides[1], *args), pair_ref(ref_sides[0], ref_sides[1], *args))
    assert 0.0 < worst <= 1.0


# ---------------------------------------------------------------- the bounds catch wrong formulas
def _outside(got, ref, names, what):
    for name in names:
        with pytest.raises(AssertionError, match='beyond their bound'):
            compare_all(what, got, ref, names=[name])


MUTANT_SHAPES = [c[:4] for c in PAIR_CASES if c[0] == c[1] >= 5 and c[2] >= 31 and c[3] >= 64][::3]


@pytest.mark.parametrize('R_u, R_i, L, F', MUTANT_SHAPES + [(5, 10, 32, 100)])
def test_pair_mutants_fall_outside(R_u, R_i, L, F):
    case = next(c for c in PAIR_CASES if c[:4] == (R_u, R_i, L, F))
    d = pair_case(case, n_p=ALL)
    ref = pair_ref_of(d)
    both = lambda *names: tuple(n + s for n in names for s in ('_user', '_item'))
    assert {'no_dot', 'gu_with_pu', 'direct_without_a', 'fc_swapped'} <= set(MUTANTS)
    _outside(pair_f32_of(d, 'no_dot'), ref, both('glogit', 'rev', 'w'), 'delta without - dot')
    _outside(pair_f32_of(d, 'gu_with_pu'), ref, ('g_user', 'glogit_user', 'rev_user', 'w_user'), 'g_u formed with p_u')
    compare_all('g_u with p_u', pair_f32_of(d, 'gu_with_pu'), ref, names=['score', 'g_item', 'w_item', 'rev_item'])
    _outside(pair_f32_of(d, 'direct_without_a'), ref, both('rev', 'w'), 'the direct term without a_r')
    _outside(pair_f32_of(d, 'fc_swapped'), ref, both('w'), 'fc swapped')
    compare_all('fc swapped', pair_f32_of(d, 'fc_swapped'), ref, names=['score'] + list(both('g', 'glogit', 'rev')))


@pytest.mark.parametrize('N, R, L, F', [c for c in OWNER_CASES if c[1] > 1 and c[2] > 1][::4])
def test_owner_mutants_fall_outside(N, R, L, F):
    s = owner_case((N, R, L, F))
    _outside(owner_f32(s, 'w0_other_half'), owner_ref(s), ('D', 'E', 'dz'), 'W0[:, L:] in the place of W0[:, :L]')
    compare_all('other half', owner_f32(s, 'w0_other_half'), owner_ref(s), names=['attn', 'pooled_attn', 'out'])
    z = with_zero_slot(s)
    ref = owner_ref(z)
    assert not bool(ref.aux['on'][0, -1].any()) and float(ref.aux['pre'][0, -1].abs().max()) == 0.0
    assert float(ref['D'][1][0, -1].abs().max()) == 0.0                         # an exact zero: no allowance at all
    _outside(owner_f32(z, 'mask_ge'), ref, ('D', 'E'), 'a >= mask on an exact-zero unit')
    compare_all('zero slot', owner_f32(z), ref)


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


def jac_args(**kw):
    a = dict(z=PTR, nb=PTR, other_table=PTR, other_rows=7, own_table=PTR, owner=PTR, W0=PTR, b0=PTR, w3=PTR, b3=PTR, fc=PTR,
             F=100, attn=PTR, pooled_attn=PTR, out=PTR, D=PTR, E=PTR, dz=PTR, N=5, R=10, L=32, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def pair_args(**kw):
    a = dict(p_u=PTR, z_u=PTR, attn_u=PTR, E_u=PTR, dz_u=PTR, fc_u=PTR, n_u=3, R_u=10, p_i=PTR, z_i=PTR, attn_i=PTR, E_i=PTR,
             dz_i=PTR, fc_i=PTR, n_i=4, R_i=10, u_idx=PTR, i_idx=PTR, n_p=7, q_bias=PTR, c_bias=PTR, W1=PTR, b1=PTR, w=PTR,
             L=32, F=100, out_score=PTR, g_user=PTR, g_item=PTR, glogit_user=PTR, glogit_item=PTR, rev_user=PTR,
             rev_item=PTR, w_user=PTR, w_item=PTR, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def test_the_library_exports_the_symbols_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    for name, args in (('r4r_narre_attn_jac', jac_args()), ('r4r_narre_pair_grad', pair_args())):
        assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
        assert decls[name][2] == list(args)
        ints = dict(other_rows=ctypes.c_int64, N=ctypes.c_int64, n_u=ctypes.c_int64, n_i=ctypes.c_int64,
                    n_p=ctypes.c_int64, R=ctypes.c_int, L=ctypes.c_int, F=ctypes.c_int, R_u=ctypes.c_int, R_i=ctypes.c_int)
        for arg, t in zip(decls[name][2], decls[name][1]):
            assert t is ints.get(arg, ctypes.c_void_p), (name, arg)
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * NARRE pair gradients:'):]
    for cite in ('NARRE.py:53-64', 'NARRE.py:24-36', 'Fixed fp32 order', 'r4r_narre_explain\'s bits'):
        assert cite in section, cite


@pytest.mark.parametrize('over, word', [
    (dict(N=-1), b'N='), (dict(other_rows=-1), b'other_rows='),
    (dict(R=0), b'R='), (dict(R=65), b'R='), (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(F=0), b'F='), (dict(F=113), b'F='),
    (dict(own_table=None), b'own_table'), (dict(owner=None), b'own_table'), (dict(fc=None), b'fc'),
    (dict(z=None), b'null'), (dict(nb=None), b'null'), (dict(W0=None), b'null'), (dict(b0=None), b'null'),
    (dict(w3=None), b'null'), (dict(b3=None), b'null'), (dict(other_table=None), b'other_table'),
    (dict(attn=None, pooled_attn=None, out=None, D=None, E=None, dz=None), b'no output'),
])
def test_owner_pass_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_narre_attn_jac', jac_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_attn_jac') and word in msg, (over, got, msg)


@pytest.mark.parametrize('over, word', [
    (dict(R_u=0), b'R_u='), (dict(R_u=65), b'R_u='), (dict(R_i=0), b'R_i='), (dict(R_i=65), b'R_i='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(F=0), b'F='), (dict(F=113), b'F='),
    (dict(n_u=-1), b'n_u='), (dict(n_i=-1), b'n_i='), (dict(n_p=-1), b'n_p='), (dict(n_p=1 << 31), b'n_p='),
    (dict(fc_u=None), b'w_user without fc_u'), (dict(fc_i=None), b'w_item without fc_i'),
    (dict(E_u=None), b'w_user without E_u'), (dict(E_i=None), b'w_item without E_i'),
    (dict(dz_u=None), b'rev_user without dz_u'), (dict(dz_i=None), b'rev_item without dz_i'),
    (dict(z_u=None), b'z_u'), (dict(attn_u=None), b'attn_u'), (dict(z_i=None), b'z_i'), (dict(attn_i=None), b'attn_i'),
    (dict(p_u=None), b'null'), (dict(p_i=None), b'null'), (dict(u_idx=None), b'null'), (dict(i_idx=None), b'null'),
    (dict(W1=None), b'null'), (dict(b1=None), b'null'), (dict(w=None), b'null'),
    (dict(n_u=0), b'n_u='), (dict(n_i=0), b'n_i='),
])
def test_pair_pass_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_narre_pair_grad', pair_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_pair_grad') and word in msg, (over, got, msg)


def test_nothing_to_do_is_ok_and_enqueues_nothing(lib):
    assert _call(lib, 'r4r_narre_attn_jac', jac_args(N=0)) == OK
    assert _call(lib, 'r4r_narre_attn_jac', jac_args(N=0, z=None, nb=None, W0=None, attn=None, out=None, D=None, E=None,
                                                     dz=None, pooled_attn=None, fc=None)) == OK
    assert _call(lib, 'r4r_narre_attn_jac', jac_args(N=0, L=65)) == ERR_ARG          # the shape is still checked
    assert _call(lib, 'r4r_narre_pair_grad', pair_args(n_p=0)) == OK
    nul = {k: None for k in pair_args() if k not in ('n_u', 'R_u', 'n_i', 'R_i', 'n_p', 'L', 'F', 'stream')}
    assert _call(lib, 'r4r_narre_pair_grad', pair_args(n_p=0, n_u=0, n_i=0, **nul)) == OK
    assert _call(lib, 'r4r_narre_pair_grad', pair_args(n_p=0, F=113)) == ERR_ARG
    assert _call(lib, 'r4r_narre_pair_grad', pair_args(n_p=0, fc_u=None)) == ERR_ARG
    # a side whose outputs are not asked for needs none of its review tensors
    assert (lib.r4r_last_error() or b'').startswith(b'r4r_narre_pair_grad')


# ---------------------------------------------------------------- explain_words' per-review weights
def test_explain_words_takes_one_row_of_weights_per_review_for_narre_only():
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(reviews4rec_amd.NarreCatalogue, 'NARRE')
    cat.dev = torch.device('cpu')
    tower = cat.model.user_conv
    w = torch.arange(2 * 10 * 100, dtype=torch.float32).reshape(2, 10, 100)
    got = cat._phrase_weights(tower, w, 2, 10)
    assert tuple(got.shape) == (20, 100) and torch.equal(got, w.reshape(20, 100))      # one row per review, in order
    assert tuple(cat._phrase_weights(tower, w[:, 0], 2, 10).shape) == (20, 100)          # [n, F] still repeats
    for bad in (torch.zeros(2, 9, 100), torch.zeros(2, 10, 99), torch.zeros(3, 10, 100), torch.zeros(2, 10, 100, 1),
                torch.zeros(2, 10, 100, dtype=torch.float64)):
        with pytest.raises(ValueError, match='weights'):
            cat.explain_words([0, 1], k=3, weights=bad)                                 # (the engine's flush would raise)
    other = _bare(reviews4rec_amd.Catalogue, 'deepconn')
    with pytest.raises(ValueError, match='weights'):                                    # no per-review rows without reviews
        other.explain_words([0], k=3, weights=torch.zeros(1, 1, 100))
    assert reviews4rec_amd.PairReviews._fields == (
        'w_user', 'w_item', 'rev_user', 'rev_item', 'glogit_user', 'glogit_item', 'attention_user', 'attention_item',
        'live_user', 'live_item', 'scores')
    for k, r, direction in ((0, None, 'up'), (3, 0, 'up'), (3, 11, 'up'), (3, True, 'up'), (3, None, 'sideways'), (101, 2, 'down')):
        with pytest.raises(ValueError):
            cat.explain_pair_reviews([0], [0], k=k, reviews=r, direction=direction)
    with pytest.raises(ValueError, match='2 users against 1 items'):
        cat.pair_reviews([0, 1], [0])
    with pytest.raises(KeyError):
        cat.pair_reviews([0], [5])
    with pytest.raises(KeyError):
        cat.explain_pair_reviews([-1], [0], k=3)
