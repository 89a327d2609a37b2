"""r4r_narre_explain on the device (csrc/narre_explain.hip, include/r4r.h "NARRE explanations"): the eval-mode review
attention for R, L up to 64 that keeps its weights and lists every owner's heaviest live slots.

What decides: head_ref.attention_ref, the float64 restatement of NARRE.attention with per-element a-priori bounds that
assume no summation order (tests/head_ref.py), for `out` and `attn`; explain_ref (tests/test_narre_explain_host.py), the
numpy statement of the list rules, over the kernel's OWN attn bits for the lists; bit equality for everything the
contract says does not depend on N, on the owners sharing a call, on K or on the outputs asked for.

Inputs are seeded and scaled as head_ref.attention_inputs scales them (W0, w3 ~ 0.4 N(0, 1), b0 ~ 0.1 N(0, 1), the rest
standard normal).  attention_ref asserts that every ReLU pre-activation is outside its rounding bound of zero; at
257 x 64 x 64 = a million pre-activations no seed passes that by luck (about 50 land inside), so the review rows that
hold one are drawn again from the same generator until none does -- the seed's own continuation, never a wider bound."""
import numpy as np
import pytest
import torch

import head_ref as hr
from test_narre_explain_host import explain_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 1), (10, 6), (10, 32), (10, 33), (33, 17), (32, 32), (64, 64)]
NS = [1, 5, 257]
ROWS = 37                      # rows of other_table


# ---------------------------------------------------------------- inputs and calls
_INPUTS = {}


def inputs(R, L, N, seed=0):
    """dict of CPU tensors: z [N, R, L], nb [N, R] in [0, ROWS), table [ROWS, L], own [N + 3, L], owner [N], W0, b0, w3,
    b3.  Computed once per key and shared, never written to."""
    key = (R, L, N, seed)
    if key in _INPUTS:
        return _INPUTS[key]
    g = hr._gen(22, R, L, N, seed)
    W0 = torch.randn((L, 2 * L), generator=g) * 0.4
    b0 = torch.randn(L, generator=g) * 0.1
    w3 = torch.randn((1, L), generator=g) * 0.4
    b3 = torch.randn(1, generator=g)
    z = torch.randn((N, R, L), generator=g)
    table = torch.randn((ROWS, L), generator=g)
    own = torch.randn((N + 3, L), generator=g)
    nb = torch.randint(0, ROWS, (N, R), generator=g)
    owner = torch.randperm(N + 3, generator=g)[:N]
    for _ in range(50):                                       # (the module docstring: rows with a marginal ReLU, again)
        cat = torch.cat([z, table[nb]], -1).double()
        pre = cat @ W0.double().T + b0.double()
        M = cat.abs() @ W0.double().abs().T + b0.double().abs()
        bad = (~((pre.abs() > 2 * (2 * L + 1) * hr.U32 * M) | (M == 0))).any(-1)
        if not bool(bad.any()):
            break
        z[bad] = torch.randn((int(bad.sum()), L), generator=g)
    else:
        raise AssertionError('no margin after 50 redraws')
    _INPUTS[key] = dict(z=z, nb=nb, table=table, own=own, owner=owner, W0=W0, b0=b0, w3=w3, b3=b3)
    return _INPUTS[key]


_REFS = {}


def reference(R, L, N, seed=0):
    """attention_ref of inputs(R, L, N, seed), once."""
    key = (R, L, N, seed)
    if key not in _REFS:
        d = inputs(R, L, N, seed)
        _REFS[key] = hr.attention_ref(d['z'], d['table'][d['nb']], d['W0'], d['b0'], d['w3'], d['b3'], None,
                                      torch.zeros((N, L)))
    return _REFS[key]


def run(d, own=False, live=None, K=0, out=True, attn=True, sel=None, **over):
    """ops.narre_explain over the inputs ``d`` (``over`` replaces entries, ``sel`` picks owners) -> CPU tensors
    (out, attn, top_slot, top_w), None where not asked for."""
    from reviews4rec_amd import ops
    d = dict(d, **over)
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    t = lambda a: a.contiguous().to(DEV)
    lv = None if live is None else t(pick(torch.as_tensor(live, dtype=torch.int32)))
    res = ops.narre_explain(t(pick(d['z'])), t(pick(d['nb'])), t(d['table']), t(d['W0']), t(d['b0']), t(d['w3']), t(d['b3']),
                            own_table=t(d['own']) if own else None, owner=t(pick(d['owner'])) if own else None,
                            live=lv, k=K, want_out=out, want_attn=attn)
    torch.cuda.synchronize()
    return tuple(None if r is None else r.cpu() for r in res)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('R, L', SHAPES)
def test_out_and_attn_within_the_float64_bounds(R, L):
    """out and attn against attention_ref's per-element bounds; with own_table, out takes one more rounding:
    2^-24 (|out| + |own|)."""
    worst = 0.0
    for N in NS:
        d, ref = inputs(R, L, N), reference(R, L, N)
        out, attn, _, _ = run(d)
        r_out = hr.compare('out R=%d L=%d N=%d' % (R, L, N), out, *ref['out'])
        r_attn = hr.compare('attn R=%d L=%d N=%d' % (R, L, N), attn, *ref['a_save'])
        # rows sum to 1: a_r = e_r / den (1 + eps), den = sum e (1 + delta), |delta| <= (R - 1) 2^-24, |eps| <= 2^-24
        assert bool((attn >= 0).all()) and float((attn.double().sum(1) - 1).abs().max()) <= (R + 1) * hr.U32
        own_rows = d['own'][d['owner']].double()
        val = ref['out'][0] + own_rows
        bound = ref['out'][1] + hr.U32 * (ref['out'][0].abs() + own_rows.abs())
        out2, attn2, _, _ = run(d, own=True)
        r_own = hr.compare('out + own R=%d L=%d N=%d' % (R, L, N), out2, val, bound)
        assert same_bits(attn2, attn)
        print('R=%d L=%d N=%d: worst error / bound  out %.3f  attn %.3f  out + own %.3f' % (R, L, N, r_out, r_attn, r_own))
        worst = max(worst, r_out, r_attn, r_own)
    print('R=%d L=%d: worst error / bound over N in %r: %.3f' % (R, L, NS, worst))


# ---------------------------------------------------------------- 2. the lists
def _with_twins(d, R):
    """Slot pairs with the same z row and the same neighbour id: in different halves of the wave where R allows, and in
    different places of a staged group of four."""
    z, nb = d['z'].clone(), d['nb'].clone()
    pairs = [(a, b) for a, b in ((0, 32), (5, 63), (1, 9), (2, 7), (0, R - 1)) if a < b < R]
    for n in range(z.shape[0]):
        a, b = pairs[n % len(pairs)] if pairs else (0, 0)
        z[n, b], nb[n, b] = z[n, a], nb[n, a]
    return dict(d, z=z, nb=nb), pairs


@pytest.mark.parametrize('R, L', [(1, 1), (10, 6), (33, 17), (64, 64)])
def test_lists_are_exactly_the_rule_over_the_kernels_own_weights(R, L):
    N = R + 6
    base = inputs(R, L, N, seed=1)
    d, pairs = _with_twins(base, R)
    live = np.concatenate([np.arange(R + 1), [R, R, max(R - 1, 0), 1, 0]]).astype(np.int32)[:N]
    assert set(live.tolist()) == set(range(R + 1))            # every value 0..R
    ref = hr.attention_ref(d['z'], d['table'][d['nb']], d['W0'], d['b0'], d['w3'], d['b3'], None, torch.zeros((N, L)))
    w64, dw = ref['a_save']
    _, attn, _, _ = run(d)
    hr.compare('attn', attn, w64, dw)
    for n in range(N):                                        # twins: equal bits, wherever they sit
        if pairs:
            a, b = pairs[n % len(pairs)]
            assert same_bits(attn[n, a], attn[n, b]), (n, a, b)
    for K in sorted({1, min(3, R), R}):
        for lv in (live, None):
            _, attn_k, slot, w = run(d, live=lv, K=K)
            assert same_bits(attn_k, attn)
            want_slot, want_w = explain_ref(attn.numpy(), lv, K)
            assert slot.dtype == torch.int32 and np.array_equal(slot.numpy(), want_slot), (K, lv is None)
            assert np.array_equal(w.numpy().view(np.uint32), want_w.view(np.uint32)), (K, lv is None)
            # the order is the float64 order wherever the bounds tell two weights apart
            s = slot.long()
            for j in range(K - 1):
                both = (s[:, j] >= 0) & (s[:, j + 1] >= 0)
                rows = both.nonzero().reshape(-1)
                a, b = s[rows, j], s[rows, j + 1]
                assert bool((w64[rows, a] + dw[rows, a] >= w64[rows, b] - dw[rows, b]).all()), (K, j)
            lvs = np.full(N, R) if lv is None else lv
            assert np.array_equal((slot.numpy() >= 0).sum(1), np.minimum(lvs, K))
            assert bool((s < torch.as_tensor(lvs)[:, None]).all())                  # no padded slot is listed


@pytest.mark.parametrize('R, L', [(10, 6), (64, 64), (33, 40)])
def test_equal_weights_list_ascending_slots(R, L):
    """W0 = w3 = 0: every logit is b3, every weight 1 / R within the float64 bound, and the list is 0, 1, 2, ..."""
    N = 5
    d = dict(inputs(R, L, N, seed=2))
    d['W0'], d['w3'] = torch.zeros_like(d['W0']), torch.zeros_like(d['w3'])
    ref = hr.attention_ref(d['z'], d['table'][d['nb']], d['W0'], d['b0'], d['w3'], d['b3'], None, torch.zeros((N, L)))
    assert bool((ref['a_save'][0] == 1.0 / R).all())
    live = np.array([R, R - 1, 3, 1, 0], np.int32)
    _, attn, slot, w = run(d, live=live, K=R)
    hr.compare('attn', attn, *ref['a_save'])
    assert bool((attn == attn[0, 0]).all())
    for n in range(N):
        assert slot[n].tolist() == list(range(live[n])) + [-1] * (R - live[n])
        assert bool((w[n, :live[n]] == attn[0, 0]).all()) and bool((w[n, live[n]:] == 0).all())


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize('R, L', [(10, 6), (10, 33), (64, 64)])
def test_an_owners_results_depend_on_that_owner_only(R, L):
    N, K = 23, min(3, R)
    d = inputs(R, L, N, seed=3)
    live = (np.arange(N) % (R + 1)).astype(np.int32)
    out, attn, slot, w = run(d, own=True, live=live, K=K)
    # permuted owners
    perm = torch.randperm(N, generator=hr._gen(23, R, L))
    got = run(d, own=True, live=live, K=K, sel=perm)
    for a, b in zip(got, (out, attn, slot, w)):
        assert same_bits(a, b[perm])
    # a call split in two, and every owner alone
    for cuts in ([0, 9, N], list(range(N + 1))):
        parts = [run(d, own=True, live=live, K=K, sel=slice(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        for j, whole in enumerate((out, attn, slot, w)):
            assert same_bits(torch.cat([p[j] for p in parts]), whole), (len(cuts), j)
    # another K: the common places hold the same bits
    for K2 in (1, R):
        o2, a2, s2, w2 = run(d, own=True, live=live, K=K2)
        k = min(K, K2)
        assert same_bits(o2, out) and same_bits(a2, attn)
        assert same_bits(s2[:, :k], slot[:, :k]) and same_bits(w2[:, :k], w[:, :k])
    # outputs not asked for change nothing of the rest
    o3, a3, s3, w3 = run(d, own=True, live=live, K=K, out=False)
    assert o3 is None and same_bits(a3, attn) and same_bits(s3, slot) and same_bits(w3, w)
    o4, a4, s4, w4 = run(d, own=True, live=live, K=K, attn=False)
    assert a4 is None and same_bits(o4, out) and same_bits(s4, slot) and same_bits(w4, w)
    o5, a5, s5, w5 = run(d, own=True, live=live, K=0)
    assert s5 is None and w5 is None and same_bits(o5, out) and same_bits(a5, attn)
    o6, a6, _, _ = run(d, own=True, live=None, K=K)
    assert same_bits(o6, out) and same_bits(a6, attn)          # live decides the lists only


@pytest.mark.parametrize('R, L', [(10, 6), (64, 64)])
def test_a_neighbour_id_outside_the_table_reads_as_a_row_of_zeros(R, L):
    N, K = 9, min(3, R)
    d = inputs(R, L, N, seed=4)
    nb = d['nb'].clone()
    outside = [-1, ROWS, 2 ** 40, -2 ** 40, 2 ** 31, 2 ** 32 + 3]
    for n in range(N):
        for j, r in enumerate(range(n % 3, R, 4)):
            nb[n, r] = outside[(n + j) % len(outside)]
    nb[N - 1] = ROWS                                          # an owner with no neighbour inside
    bad = (nb < 0) | (nb >= ROWS)
    assert int(bad.sum()) > N
    zeros_table = torch.cat([d['table'], torch.zeros((1, L))])
    want = run(d, own=True, K=K, nb=torch.where(bad, torch.full_like(nb, ROWS), nb), table=zeros_table)
    got = run(d, own=True, K=K, nb=nb)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


# ---------------------------------------------------------------- 4. the op-by-op kernel
@pytest.mark.parametrize('R, L', [(10, 6), (32, 32)])
def test_agreement_with_the_op_by_op_forward(R, L):
    """Where r4r_narre_attn_fwd takes the shape, its a_save and out and this kernel's attn and out are two fp32
    evaluations of one float64 value: they differ by at most the sum of the two sides' bounds.  Not bit equality."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    for N in (5, 257):
        d, ref = inputs(R, L, N), reference(R, L, N)
        out, attn, _, _ = run(d)
        t = lambda a: a.contiguous().to(DEV)
        z, other = t(d['z']), t(d['table'][d['nb']])
        W0, b0, w3, b3 = t(d['W0']), t(d['b0']), t(d['w3']), t(d['b3'])
        old_out = torch.empty((N, L), dtype=torch.float32, device=DEV)
        old_h = torch.empty((N, R, L), dtype=torch.float32, device=DEV)
        old_a = torch.empty((N, R), dtype=torch.float32, device=DEV)
        _lib.call('r4r_narre_attn_fwd', ptr(z), ptr(other), ptr(W0), ptr(b0), ptr(w3), ptr(b3), None, ptr(old_out),
                  ptr(old_h), ptr(old_a), N, R, L)
        torch.cuda.synchronize()
        r1 = hr.compare('attn against a_save', attn, old_a.cpu().double(), 2 * ref['a_save'][1])
        r2 = hr.compare('out against out', out, old_out.cpu().double(), 2 * ref['out'][1])
        print('R=%d L=%d N=%d: |new - old| / (sum of bounds)  attn %.3f  out %.3f' % (R, L, N, r1 / 2, r2 / 2))
