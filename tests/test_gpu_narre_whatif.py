"""r4r_narre_logits and r4r_narre_whatif on the device (csrc/narre_whatif.hip; include/r4r.h, "NARRE what-if scores"),
through ops.narre_logits / ops.narre_whatif.

What decides: narre_whatif_ref's float64 restatements with per-element a-priori bounds that assume no summation order,
for every element; bit equality for everything the contract says a logit or a variant does not depend on (N, S, the
slot's position; V, the variant's column, n_p, who shares the call, how a mask spells a list); and the exact cases
(w = 0, NULL biases, NULL own).  The shapes, seeds and inputs are narre_whatif_ref's, the ones
tests/test_narre_whatif_host.py shows to meet the ReLU margins and to be reachable in float32."""
import pytest
import torch

from head_ref import C_EXPF, TINY, U32, bits_equal, compare
from narre_whatif_ref import (ALL_BITS, ARGS, BARE_CASES, BIT63, CASES, CHAIN_CASES, EDGE_SHAPES, LOGIT_CASES, N_I, N_U,
                              chain_case, edge_case, edge_masks, logit_case, logits_ref, pad_inputs, whatif_case,
                              whatif_ref, whatif_ref_of)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASE_ID = lambda c: 'Ru%d-Su%d-Ri%d-Si%d-L%d-V%d-n%d' % c


def logits(s, sel=None):
    """ops.narre_logits over an owner pass's inputs (``sel`` picks owners) -> a CPU tensor [N, S]."""
    from reviews4rec_amd import ops
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    t = lambda a: a.contiguous().to(DEV)
    return ops.narre_logits(t(pick(s['z'])), t(pick(s['nb'])), t(s['other_table']), t(s['W0']), t(s['b0']), t(s['w3']),
                            t(s['b3'])).cpu()


def scores(d, sel=None, cols=None, **over):
    """ops.narre_whatif over a case (``sel`` picks pairs, ``cols`` variant columns, ``over`` replaces entries) -> CPU."""
    from reviews4rec_amd import ops
    d = dict(d, **over)
    t = lambda a: None if a is None else a.contiguous().to(DEV)
    side = lambda s: dict(z=t(s['z']), logit=t(s['logit']), z_pad=t(s['z_pad']), own=t(s.get('own')),
                          logit_pad=s['logit_pad'], R=s['R'])
    pick = lambda a: a if a is None or sel is None else a[sel]
    col = lambda a: a if a is None or cols is None else a[:, cols]
    return ops.narre_whatif(side(d['user']), side(d['item']), t(pick(d['u_idx'])), t(pick(d['i_idx'])),
                            t(col(pick(d['drop_u']))), t(col(pick(d['drop_i']))), t(d['W1']), t(d['b1']), t(d['w']),
                            q_bias=t(d['q_bias']), c_bias=t(d['c_bias'])).cpu()


# ---------------------------------------------------------------- the owner pass
@pytest.mark.parametrize('case', LOGIT_CASES, ids=lambda c: 'N%d-S%d-L%d' % c)
def test_logits_against_float64_and_narre_explain(case):
    from reviews4rec_amd import ops
    N, S, L = case
    s = logit_case(case)
    assert int(s['nb'][0, S - 1]) == -1                          # an id outside the table: a row of zeros
    got = logits(s)
    assert tuple(got.shape) == (N, S) and got.dtype == torch.float32
    val, bound = logits_ref(s)['logit']
    print('logits %r: worst error / bound %.3f' % (case, compare('logits %r' % (case,), got, val, bound)))
    # the padding slot of a side: N = 1, S = 1 on z_pad and the pad id
    pad = pad_inputs(s)
    compare('pad logit %r' % (case,), logits(pad), *logits_ref(pad)['logit'])
    # the float64 softmax of the returned logits against the weights r4r_narre_explain keeps: both sets of logits lie
    # within `bound` of the float64 ones, so within 2 bound of each other; then head_ref.attention_ref's softmax rule
    t = lambda a: a.contiguous().to(DEV)
    _, attn, _, _ = ops.narre_explain(t(s['z']), t(s['nb']), t(s['other_table']), t(s['W0']), t(s['b0']), t(s['w3']),
                                      t(s['b3']), want_out=False)
    lg = got.double()
    a = torch.softmax(lg, dim=1)
    spread = lg.max(1).values - lg.min(1).values + 4 * bound.max(1).values
    rho = 2 * bound.max(1).values + U32 * spread + C_EXPF * U32
    da = a * torch.expm1(2 * rho + (S + 1) * U32)[:, None] + 2 * TINY
    compare('softmax of the logits against narre_explain %r' % (case,), attn.cpu(), a, da)


@pytest.mark.parametrize('case', [c for c in LOGIT_CASES if c[0] == 9], ids=lambda c: 'N%d-S%d-L%d' % c)
def test_logit_bits_depend_on_the_slot_alone(case):
    N, S, L = case
    s = logit_case(case)
    full = logits(s)
    for sel in (slice(0, 1), slice(0, 4), slice(4, 9), slice(8, 9)):      # calls of 1, 4, 5 and 1 owners
        assert bits_equal(logits(s, sel=sel), full[sel]), sel
    # every slot alone: N S owners of one slot
    alone = dict(s, z=s['z'].reshape(N * S, 1, L), nb=s['nb'].reshape(N * S, 1))
    assert bits_equal(logits(alone).reshape(N, S), full)
    # the slots in reverse order, and each owner's slots twice (S' = 2 S where that fits): the position does not count
    rev = dict(s, z=s['z'].flip(1), nb=s['nb'].flip(1))
    assert bits_equal(logits(rev).flip(1).contiguous(), full)
    if 2 * S <= 64:
        twice = dict(s, z=torch.cat([s['z'], s['z']], 1), nb=torch.cat([s['nb'], s['nb']], 1))
        got = logits(twice)
        assert bits_equal(got[:, :S].contiguous(), full) and bits_equal(got[:, S:].contiguous(), full)


# ---------------------------------------------------------------- the variant pass
_WORST = {'score': 0.0}


@pytest.mark.parametrize('case', CASES, ids=CASE_ID)
def test_scores_against_float64(case):
    R_u, S_u, R_i, S_i, L, V, n_p = case
    d = whatif_case(case)
    got = scores(d)
    assert tuple(got.shape) == (n_p, V) and got.dtype == torch.float32
    ratio = compare('what-if %r' % (case,), got, *whatif_ref_of(d)['score'])
    _WORST['score'] = max(_WORST['score'], ratio)
    print('what-if %r: error / bound %.3f, worst so far %.3f' % (case, ratio, _WORST['score']))
    # w = 0: exactly the summed biases
    zero = scores(d, w=torch.zeros_like(d['w']))
    assert bits_equal(zero, (d['q_bias'][d['u_idx']] + d['c_bias'][d['i_idx']])[:, None].expand(n_p, V).contiguous())


@pytest.mark.parametrize('case', BARE_CASES, ids=CASE_ID)
def test_null_biases_and_null_own(case):
    d = whatif_case(case, biases=False, own=False)
    assert d['q_bias'] is None and d['user']['own'] is None
    compare('what-if, bare %r' % (case,), scores(d), *whatif_ref_of(d)['score'])
    for over in (dict(biases=False), dict(own=False)):           # (the biases do not reach a ReLU: the margins are the same)
        d = whatif_case(case, **over)
        compare('what-if %r %r' % (case, over), scores(d), *whatif_ref_of(d)['score'])


@pytest.mark.parametrize('R, S, L', EDGE_SHAPES)
def test_every_edge_mask(R, S, L):
    """One variant per edge mask on the user side against a walk of the same masks on the item side: nothing, every
    single bit, bit S - 1, bit 63, a bit >= S, all bits, fewer than R slots left."""
    edge = edge_masks(S, R)
    assert 0 in edge and ALL_BITS in edge and BIT63 in edge and all((1 << s) in edge or s == 63 for s in range(S))
    assert S == 64 or (1 << S) in edge
    d = edge_case(R, S, L)
    n_p = N_U * N_I
    got = scores(d)
    print('edge masks R %d S %d L %d: error / bound %.3f' % (R, S, L, compare('edge masks', got, *whatif_ref_of(d)['score'])))
    # how a mask spells a list does not count: bits at or beyond S, bits on slots that would not have been selected
    low = (1 << S) - 1
    i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    same = [(0, i64(~low & ((1 << 64) - 1))), (ALL_BITS, i64(low)), (1, i64(1 | (~low & ((1 << 64) - 1))))]
    if S >= R + 2:
        same += [(1, i64(1 | (1 << (S - 1)))), (0, i64(1 << (S - 1))), (2, i64(2 | (1 << (R + 1))))]
    a = torch.tensor([x for x, _ in same], dtype=torch.int64)[None, :].expand(n_p, len(same)).contiguous()
    b = torch.tensor([y for _, y in same], dtype=torch.int64)[None, :].expand(n_p, len(same)).contiguous()
    plain = torch.zeros_like(a)
    assert bits_equal(scores(d, drop_u=a, drop_i=plain), scores(d, drop_u=b, drop_i=plain))
    assert bits_equal(scores(d, drop_u=plain, drop_i=a), scores(d, drop_u=plain, drop_i=b))
    # NULL masks are all-zero masks
    assert bits_equal(scores(d, drop_u=None, drop_i=a), scores(d, drop_u=plain, drop_i=a))
    assert bits_equal(scores(d, drop_u=None, drop_i=None), scores(d, drop_u=plain[:, :1].contiguous(), drop_i=None))


@pytest.mark.parametrize('case', [c for c in CASES if c[6] == 257][::3] + [CASES[-1]], ids=CASE_ID)
def test_a_variants_bits_do_not_depend_on_the_call(case):
    R_u, S_u, R_i, S_i, L, V, _ = case
    n = 257
    d = whatif_case(case, n_p=n)
    full = scores(d)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    assert bits_equal(scores(d, sel=perm), full[perm])                                # permuted pairs
    for sel in (slice(0, 1), slice(1, 65), slice(65, 130), slice(256, 257)):          # calls of 1, 64, 65 and 1 pairs
        assert bits_equal(scores(d, sel=sel), full[sel]), sel
    cols = torch.randperm(V, generator=torch.Generator().manual_seed(4))
    assert bits_equal(scores(d, cols=cols), full[:, cols])                            # permuted variant columns
    for v in sorted({0, V // 2, V - 1}):                                              # a variant alone: V = 1
        assert bits_equal(scores(d, cols=slice(v, v + 1)), full[:, v:v + 1]), v


def test_seventeen_variants_at_once_and_as_sixteen_plus_one():
    case = next(c for c in CASES if c[5] == 17 and c[4] >= 32 and c[0] >= 10)
    d = whatif_case(case, n_p=12)
    full = scores(d)
    assert full.shape[1] == 17
    both = torch.cat([scores(d, cols=slice(0, 16)), scores(d, cols=slice(16, 17))], 1)
    assert bits_equal(both, full)
    # the same variant in every column gives one value per pair
    col = torch.full((16,), 5)
    rep = scores(d, cols=col)
    assert bits_equal(rep, full[:, 5:6].expand(12, 16).contiguous())


@pytest.mark.parametrize('case', CHAIN_CASES, ids=lambda c: 'Ru%d-Su%d-Ri%d-Si%d-L%d-V%d' % c)
def test_the_two_passes_chained(case):
    """The composition a catalogue runs: the device's logits feeding the variant pass, against the float64 chain with
    the owner pass's bounds carried through the softmax (dlogit, dlogit_pad)."""
    d, ref_sides = chain_case(case)
    dev_sides = {}
    for name in ('user', 'item'):
        raw = d['raw_' + name]
        dev_sides[name] = dict(d[name], logit=logits(raw), logit_pad=float(logits(pad_inputs(raw)).reshape(())))
    ref = whatif_ref(ref_sides['user'], ref_sides['item'], *(d[k] for k in ARGS[2:]))
    ratio = compare('chain', scores(d, user=dev_sides['user'], item=dev_sides['item']), *ref['score'])
    print('the two passes chained %r: error / bound %.3f' % (case, ratio))
