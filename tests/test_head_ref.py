"""The head-op checkers (tests/head_ref.py) tested on their own, without a GPU.

On the inputs of every case of tests/test_gpu_head_ops.py:
  - the same op computed in fp32 on the CPU with plain ATen passes its checker -- the reference alone stays inside the
    bound, which is what justifies each c (the bounds are loose: the fp32 results sit far inside them);
  - so, because the bounds are loose, every defect the shapes are aimed at is emulated on an otherwise exact float64
    result rounded to fp32, and the checker must reject it at every shape it applies to;
  - the ReLU margin holds for every seeded case (the references assert it before they compare anything)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ref as hr


def exact(ref):
    """What a perfect kernel would return: the float64 values rounded once to fp32."""
    return {k: v.float() for k, (v, _) in ref.items()}


def rejects(what, got, ref, names):
    with pytest.raises(AssertionError, match='beyond their bound'):
        hr.compare_all(what, got, ref, names)


def leaves(*ts):
    return [t.clone().requires_grad_(True) for t in ts]


# ------------------------------------------------------------------------------------------------------------ linear
def linear32(x, w, b, gy, relu):
    x, w, b = leaves(x, w, b)
    y = F.linear(x, w, b)
    y = F.relu(y) if relu else y
    y.backward(gy)
    return dict(y=y.detach(), g_x=x.grad, g_w=w.grad, g_b=b.grad)


@pytest.mark.parametrize('relu', [False, True], ids=['id', 'relu'])
@pytest.mark.parametrize('case', hr.LINEAR_CASES + ['zeros'], ids=str)
def test_linear_fp32_reference_is_inside_the_bound(case, relu):
    inp = hr.linear_zero_inputs() if case == 'zeros' else hr.linear_inputs(case)
    ref = hr.linear_ref(*inp, relu)                          # asserts the ReLU margin
    assert hr.compare_all('exact', exact(ref), ref) <= 1.0
    print('linear %s relu=%d fp32/bound %.3g' % (case, relu, hr.compare_all('linear', linear32(*inp, relu), ref)))
    if case == 'zeros' and relu:
        on = ref.aux['on']
        assert not bool(on[[1, 2, 4]].any()) and bool(on[[0, 3, 5]].any())
        assert bool((ref['g_x'][0][[1, 2, 4]] == 0).all())


def _rows(case):
    shape = case[0]
    return int(np.prod(shape)) if isinstance(shape, tuple) else shape


SPLIT_CASES = [c for c in hr.LINEAR_CASES if hr.linear_splits(_rows(c))[0] > 1]
RAGGED_CASES = [c for c in SPLIT_CASES if _rows(c) % hr.linear_splits(_rows(c))[1]]


def test_the_split_cases_are_the_ones_meant():
    assert [_rows(c) for c in SPLIT_CASES] == [257, 128, 129, 191, 2047, 2048, 2049, 2111, 4100, 130]
    assert [_rows(c) for c in RAGGED_CASES] == [257, 129, 191, 2047, 2049, 2111, 4100]
    assert hr.linear_splits(4100) == (32, 129) and hr.linear_splits(127) == (1, 127) and hr.linear_splits(0) == (1, 1)
    assert [hr.attn_splits(r) for r in (130, 260, 8200, 9000, 0)] == [(1, 130), (2, 130), (64, 129), (64, 141), (1, 1)]


@pytest.mark.parametrize('relu', [False, True], ids=['id', 'relu'])
@pytest.mark.parametrize('case', RAGGED_CASES, ids=str)
def test_linear_rejects_a_dropped_last_row_of_a_ragged_split(case, relu):
    ref = hr.linear_ref(*hr.linear_inputs(case), relu)
    geff, x2 = ref.aux['geff'], ref.aux['x2']
    got = exact(ref)
    got['g_w'] = (ref['g_w'][0] - geff[-1][:, None] * x2[-1][None, :]).float()
    got['g_b'] = (ref['g_b'][0] - geff[-1]).float()
    rejects('linear', got, ref, ['g_w'])
    rejects('linear', got, ref, ['g_w', 'g_b'])


@pytest.mark.parametrize('relu', [False, True], ids=['id', 'relu'])
@pytest.mark.parametrize('case', SPLIT_CASES, ids=str)
def test_linear_rejects_a_split_partial_added_twice(case, relu):
    ref = hr.linear_ref(*hr.linear_inputs(case), relu)
    geff, x2 = ref.aux['geff'], ref.aux['x2']
    ns, per = hr.linear_splits(x2.shape[0])
    for sp in (0, ns - 1):
        sl = slice(sp * per, min((sp + 1) * per, x2.shape[0]))
        got = exact(ref)
        got['g_w'] = (ref['g_w'][0] + geff[sl].T @ x2[sl]).float()
        got['g_b'] = (ref['g_b'][0] + geff[sl].sum(0)).float()
        rejects('linear', got, ref, ['g_w'])
        rejects('linear', got, ref, ['g_b'])


@pytest.mark.parametrize('relu', [False, True], ids=['id', 'relu'])
@pytest.mark.parametrize('case', [c for c in hr.LINEAR_CASES if c[2] >= 2], ids=str)
def test_linear_rejects_the_bias_column_of_the_neighbouring_output(case, relu):
    ref = hr.linear_ref(*hr.linear_inputs(case), relu)
    got = exact(ref)
    got['g_b'] = torch.roll(got['g_b'], 1)
    rejects('linear', got, ref, ['g_b'])


def test_linear_rejects_a_mask_applied_forward_but_not_backward():
    inp = hr.linear_zero_inputs()
    ref = hr.linear_ref(*inp, True)
    unmasked = hr.linear_ref(*inp, False)
    got = exact(ref)
    for name in ('g_x', 'g_w', 'g_b'):
        rejects('linear', dict(got, **{name: unmasked[name][0].float()}), ref, [name])


# ---------------------------------------------------------------------------------------------------------------- FM
def fm32(x, V, lw, lb, go):
    x, V, lw, lb = leaves(x, V, lw, lb)
    out = 0.5 * ((x @ V) ** 2 - (x * x) @ (V * V)).sum(1) + F.linear(x, lw, lb).squeeze(-1)
    out.backward(go)
    return dict(out=out.detach(), g_x=x.grad, g_V=V.grad, g_lin_w=lw.grad, g_lin_b=lb.grad)


@pytest.mark.parametrize('case', hr.FM_CASES, ids=str)
def test_fm_fp32_reference_is_inside_the_bound(case):
    inp = hr.fm_inputs(case)
    ref = hr.fm_ref(*inp)
    assert hr.compare_all('exact', exact(ref), ref) <= 1.0
    print('fm %s fp32/bound %.3g' % (case, hr.compare_all('fm', fm32(*inp), ref)))


@pytest.mark.parametrize('case', [c for c in hr.FM_CASES if c[1] > 64], ids=str)
def test_fm_rejects_slot_1_inputs_missing(case):
    """Inputs 64..127 (slot 1 of every lane) left out of s_k, in the forward, in g_x and in g_V one at a time; and
    read for s_k but their rows of g_V never written."""
    ref = hr.fm_ref(*hr.fm_inputs(case))
    x, V, lw, lb, go = (ref.aux[k] for k in ('x', 'V', 'lw', 'lb', 'go'))
    keep = torch.ones(x.shape[1], dtype=torch.float64)
    keep[64:128] = 0
    s = (x * keep) @ V
    g1 = go[:, None]
    bad = dict(out=0.5 * (s * s - (x * x) @ (V * V)).sum(1) + x @ lw + lb,
               g_x=g1 * (s @ V.T - x * (V * V).sum(1) + lw),
               g_V=x.T @ (g1 * s) - (g1 * x * x).sum(0)[:, None] * V)
    for name, val in bad.items():
        rejects('fm', dict(exact(ref), **{name: val.float()}), ref, [name])
    gV = ref['g_V'][0].clone()
    gV[64:128] = 0
    rejects('fm', dict(exact(ref), g_V=gV.float()), ref, ['g_V'])


@pytest.mark.parametrize('case', [c for c in hr.FM_CASES if c[0] > 1], ids=str)
def test_fm_rejects_a_lost_example_in_the_parameter_gradients(case):
    """fm_bwd_p deals examples to 4 row groups: the last example left out of g_V, g_lin_w and g_lin_b."""
    inp = hr.fm_inputs(case)
    ref = hr.fm_ref(*inp)
    less = hr.fm_ref(inp[0][:-1], inp[1], inp[2], inp[3], inp[4][:-1])
    for name in ('g_V', 'g_lin_w', 'g_lin_b'):
        rejects('fm', dict(exact(ref), **{name: less[name][0].float()}), ref, [name])


# --------------------------------------------------------------------------------------- rowdot, bias head, scatters
@pytest.mark.parametrize('case', hr.ROWDOT_CASES, ids=str)
def test_rowdot_fp32_reference_is_inside_the_bound(case):
    a, c, go = hr.rowdot_inputs(case)
    ref = hr.rowdot_ref(a, c, go)
    a32, c32 = leaves(a, c)
    out = (a32 * c32).sum(1)
    out.backward(go)
    print('rowdot %s fp32/bound %.3g' % (case, hr.compare_all('rowdot', dict(out=out.detach(), g_a=a32.grad, g_c=c32.grad), ref)))
    if case[1] > 64:                                         # the second trip of the d += 64 loop lost
        rejects('rowdot', dict(out=(a[:, :64].double() * c[:, :64].double()).sum(1).float()), ref, ['out'])


@pytest.mark.parametrize('U', [3, 1])
@pytest.mark.parametrize('N', hr.BIAS_NS)
@pytest.mark.parametrize('form', ['r_ids', 'ids', 'r'])
def test_bias_head_fp32_reference_is_inside_the_bound(form, N, U):
    r, ub, ib, gb, uid, iid, go = hr.bias_head_inputs(N, U)
    r = None if form == 'ids' else r
    if form == 'r':
        ub = ib = uid = iid = None
    ref = hr.bias_head_ref(r, ub, ib, gb, uid, iid, go)
    ps = {k: t.clone().requires_grad_(True) for k, t in (('r', r), ('ub', ub), ('ib', ib), ('gb', gb)) if t is not None}
    out = ps['gb'].expand(N)
    if ub is not None:
        out = ps['ub'][uid] + ps['ib'][iid] + out
    if r is not None:
        out = ps['r'] + out
    out.backward(go)
    got = dict(out=out.detach(), g_global=ps['gb'].grad)
    if ub is not None:
        got.update(g_user_bias=ps['ub'].grad, g_item_bias=ps['ib'].grad)
    print('bias_head %s N=%d U=%d fp32/bound %.3g' % (form, N, U, hr.compare_all('bias_head', got, ref)))
    if N == 257:                                             # element 256 missing from the 257-element sum
        rejects('bias_head', dict(g_global=go[:256].double().sum().float().reshape(1)), ref, ['g_global'])


@pytest.mark.parametrize('case', hr.EMBED_CASES, ids=str)
def test_dense_scatter_fp32_reference_is_inside_the_bound(case):
    table, idx, g = hr.embed_inputs(case)
    val, bound = hr.multiplicity_sum(idx, g, hr.EMBED_ROWS)
    got = torch.zeros_like(table).index_add_(0, idx, g)
    print('scatter %s fp32/bound %.3g' % (case, hr.compare('scatter', got, val, bound)))
    assert bool((bound[7] == 0).all()) and bool((val[7] == 0).all())
    lost = val.clone()
    lost[hr.EMBED_ROWS - 1] = 0                              # the last entry's row never written
    with pytest.raises(AssertionError, match='beyond their bound'):
        hr.compare('scatter', lost.float(), val, bound)


@pytest.mark.parametrize('case', hr.ORDERED_CASES, ids=str)
def test_ordered_scatter_reference_and_the_descending_mutant(case):
    D, n, layout = case
    idx, rows = hr.ordered_inputs(D, n, layout)
    want = hr.ordered_scatter_np(idx.numpy(), rows.numpy(), hr.EMBED_ROWS)
    val, bound = hr.multiplicity_sum(idx, rows, hr.EMBED_ROWS)
    hr.compare('ordered', torch.from_numpy(want), val, bound)        # a sequential fp32 sum is one valid order
    assert hr.bits_equal(want, hr.ordered_scatter_np(idx.numpy(), rows.numpy(), hr.EMBED_ROWS))
    if layout == 'all':
        assert not want.any()
        return
    if layout == 'dups':
        assert int((idx == hr.EMBED_ROWS - 1).sum()) == len({e for e in (0, 63, 64, 65, n - 1) if e < n})
    if n >= 64:                                              # three or more duplicates of some row: the order shows in the bits
        assert not hr.bits_equal(want, hr.ordered_scatter_np(idx.numpy(), rows.numpy(), hr.EMBED_ROWS, descending=True))
    assert not hr.bits_equal(np.float32([0.0]), np.float32([-0.0]))


# ------------------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize('case', hr.TLOSS_CASES, ids=str)
def test_transform_loss_fp32_reference_is_inside_the_bound(case):
    a, b, gup = hr.tloss_inputs(case)
    ref = hr.transform_loss_ref(a, b, gup)
    a32, b32 = leaves(a, b)
    out = (a32 - b32).pow(2).sum(-1).mean()
    out.backward(torch.tensor(gup))
    print('transform_loss %s fp32/bound %.3g' % (case, hr.compare_all('tloss', dict(out=out.detach(), g_a=a32.grad, g_b=b32.grad), ref)))
    if case == (257, 1):                                     # element 256 missing from the 257-element sum
        lost = ((a.double() - b.double())[:256] ** 2).sum() / 257
        rejects('tloss', dict(out=lost.float()), ref, ['out'])


@pytest.mark.parametrize('N', hr.MSE_NS)
def test_mse_fp32_reference_is_inside_the_bound(N):
    out, y = hr.vector_inputs(N, 0)
    denom = N + 3
    ref = hr.mse_ref(out, y, denom)
    print('mse %d fp32/bound %.3g' % (N, hr.compare_all('mse', dict(se=(out - y) ** 2, g=2 * (out - y) / denom), ref)))
    rejects('mse', dict(g=(2 * (out.double() - y.double()) / N).float()), ref, ['g'])     # denom taken for N


# --------------------------------------------------------------------------------------------------- NARRE attention
def attention32(x, o, W0, b0, w3, b3, mult, go):
    x, o, W0, b0, w3, b3 = leaves(x, o, W0, b0, w3, b3)
    h = F.relu(F.linear(torch.cat([x, o], -1), W0, b0))
    h = h if mult is None else h * mult
    a = torch.softmax(F.linear(h, w3, b3).squeeze(-1), dim=1)
    out = (a.unsqueeze(-1) * x).sum(1)
    out.backward(go)
    return dict(out=out.detach(), h_save=h.detach(), a_save=a.detach(), g_x=x.grad, g_other=o.grad, g_W0=W0.grad,
                g_b0=b0.grad, g_w3=w3.grad, g_b3=b3.grad)


ATTN_IDS = [(name, dropout) for name in hr.ATTN_CASES for dropout in (False, True)]


@pytest.mark.parametrize('name,dropout', ATTN_IDS)
def test_attention_fp32_reference_is_inside_the_bound(name, dropout):
    inp = hr.attention_inputs(name, dropout)
    ref = hr.attention_ref(*inp)                             # asserts the ReLU margin
    assert hr.compare_all('exact', exact(ref), ref) <= 1.0
    print('attention %s dropout=%d fp32/bound %.3g' % (name, dropout, hr.compare_all('attention', attention32(*inp), ref)))
    N, R, L, kind = hr.ATTN_CASES[name]
    sc, a = ref.aux['sc'], ref['a_save'][0]
    if kind == 'big':
        assert 60 < float(sc.max()) - float(sc.min()) and 90 < float(sc.max()) < 102, (float(sc.min()), float(sc.max()))
    if kind == 'identical' and not dropout:
        assert float((a - 1.0 / R).abs().max()) < 1e-15
    if kind == 'padded':
        pad = (inp[0] == 0).all(-1) & (inp[1] == 0).all(-1)
        assert int(pad.sum()) == sum(R - (n + 2) for n in range(N))
        assert bool((a[pad] > 100 * ref['a_save'][1][pad]).all())     # a weight the bound cannot hide


def _param_grads(G, C, S, H, w3_shape):
    return dict(g_W0=(G.T @ C).float(), g_b0=G.sum(0).float(), g_w3=(S @ H).reshape(w3_shape).float(),
                g_b3=S.sum().reshape(1).float())


@pytest.mark.parametrize('dropout', [False, True])
@pytest.mark.parametrize('name', ['rows260', 'rows8200', 'rows9000'])
def test_attention_rejects_lost_and_doubled_rows_of_a_split(name, dropout):
    inp = hr.attention_inputs(name, dropout)
    ref = hr.attention_ref(*inp)
    G, C, S, H = (ref.aux[k] for k in 'GCSH')
    rows = G.shape[0]
    ns, per = hr.attn_splits(rows)
    if rows % per:                                           # the last row of the ragged last split dropped
        got = _param_grads(G[:-1], C[:-1], S[:-1], H[:-1], inp[4].shape)
        rejects('attention', got, ref, ['g_W0', 'g_b0', 'g_w3', 'g_b3'])
        rejects('attention', got, ref, ['g_W0'])
    for sp in (0, ns - 1):                                   # one split's partial added twice
        sl = slice(sp * per, min((sp + 1) * per, rows))
        twice = _param_grads(torch.cat([G, G[sl]]), torch.cat([C, C[sl]]), torch.cat([S, S[sl]]), torch.cat([H, H[sl]]),
                             inp[4].shape)
        for k in ('g_W0', 'g_b0', 'g_w3'):
            rejects('attention', twice, ref, [k])


@pytest.mark.parametrize('name', [k for k, v in hr.ATTN_CASES.items() if v[1] > 1 and v[3] != 'identical'])
def test_attention_rejects_the_multiplier_ignored_in_the_backward_only(name):
    """(With R = 1 the softmax is constant, and with identical reviews g_out . x_r is the same for every r: either way
    the gradient at the scores is 0, none reaches the scorer and the defect cannot show.)"""
    x, o, W0, b0, w3, b3, mult, go = hr.attention_inputs(name, True)
    ref = hr.attention_ref(x, o, W0, b0, w3, b3, mult, go)
    N, R, L = x.shape
    S, on, a = ref.aux['S'].reshape(N, R), ref.aux['on'], ref.aux['a']
    G = torch.where(on, S[..., None] * w3.double().reshape(-1), torch.zeros_like(ref.aux['pre']))    # no mult
    gcat = G @ W0.double()
    got = dict(g_x=(gcat[..., :L] + a[..., None] * go.double()[:, None, :]).float(), g_other=gcat[..., L:].float())
    got.update(_param_grads(G.reshape(-1, L), ref.aux['C'], ref.aux['S'], ref.aux['H'], w3.shape))
    for k in ('g_x', 'g_other', 'g_W0', 'g_b0'):
        rejects('attention', got, ref, [k])


@pytest.mark.parametrize('dropout', [False, True])
def test_attention_rejects_a_softmax_without_the_max_subtraction(dropout):
    inp = hr.attention_inputs('big_scores', dropout)
    ref = hr.attention_ref(*inp)
    e = torch.exp(ref.aux['sc'].float())
    a = e / e.sum(1, keepdim=True)
    assert not bool(torch.isfinite(a).all())
    rejects('attention', dict(a_save=a), ref, ['a_save'])
    rejects('attention', dict(out=(a.unsqueeze(-1) * inp[0]).sum(1)), ref, ['out'])


@pytest.mark.parametrize('dropout', [False, True])
def test_attention_rejects_a_padded_review_masked_out_of_the_softmax(dropout):
    inp = hr.attention_inputs('padded', dropout)
    ref = hr.attention_ref(*inp)
    pad = (inp[0] == 0).all(-1) & (inp[1] == 0).all(-1)
    a = torch.softmax(ref.aux['sc'].masked_fill(pad, float('-inf')), dim=1)
    rejects('attention', dict(a_save=a.float()), ref, ['a_save'])
    rejects('attention', dict(out=torch.einsum('nr,nrl->nl', a, inp[0].double()).float()), ref, ['out'])
