"""The op-by-op head kernels (csrc/smallops.hip, csrc/narre.hip, reached through reviews4rec_amd/ops.py or the C ABI)
against the float64 restatements of tests/head_ref.py, at their lane, block and split edges.  Every comparison is a
derived per-element bound (c 2^-24 M, see head_ref) or bit equality; tests/test_head_ref.py shows on the CPU that an
fp32 ATen computation passes each checker at these very inputs and that the defects the shapes are aimed at do not.
Each test prints the worst error / bound of every output (`HEAD_RATIO <op>.<output> <value>`).  Runs on a real MI355X only (-m gpu)."""
import pytest
import torch

import head_ref as hr

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from reviews4rec_amd import ops
    return ops


def _lib():
    from reviews4rec_amd import _lib
    return _lib


def dev_leaves(*ts):
    return [None if t is None else t.to(DEV).requires_grad_(True) for t in ts]


def check(op, what, got, ref, names=None):
    """Every output of `got` against its bound; prints each one's worst error / bound."""
    each = {}
    hr.compare_all(what, got, ref, names, each)
    for name, ratio in each.items():
        print('HEAD_RATIO %s.%s %.4g' % (op, name, ratio))


# ------------------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize('relu', [False, True], ids=['id', 'relu'])
@pytest.mark.parametrize('case', hr.LINEAR_CASES + ['zeros'], ids=str)       # what each case targets: head_ref.LINEAR_CASES
def test_linear(case, relu):
    """'zeros': exact-zero pre-activations (zero rows, a row of negative zeros, zero bias): `s < 0.f` forward and
    `!(y > 0.f)` in linear_bwd_x_kernel / linear_bwd_w_kernel must all leave the unit off."""
    ops = _ops()
    x, w, b, gy = hr.linear_zero_inputs() if case == 'zeros' else hr.linear_inputs(case)
    ref = hr.linear_ref(x, w, b, gy, relu)
    xd, wd, bd = dev_leaves(x, w, b)
    y = ops.linear(xd, wd, bd, relu)
    assert y.shape == gy.shape
    y.backward(gy.to(DEV))
    check('linear', 'linear %s' % (case,), dict(y=y, g_x=xd.grad, g_w=wd.grad, g_b=bd.grad), ref)
    if case == 'zeros':
        dead = [1, 2, 4] if relu else []
        assert bool((y.detach()[[1, 2, 4]] == 0).all())
        assert bool((xd.grad[dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- FM
@pytest.mark.parametrize('case', hr.FM_CASES, ids=str)                        # what each case targets: head_ref.FM_CASES
def test_fm(case):
    ops = _ops()
    x, V, lw, lb, go = hr.fm_inputs(case)
    ref = hr.fm_ref(x, V, lw, lb, go)
    xd, Vd, lwd, lbd = dev_leaves(x, V, lw, lb)
    out = ops.fm(xd, Vd, lwd, lbd)
    out.backward(go.to(DEV))
    got = dict(out=out, g_x=xd.grad, g_V=Vd.grad, g_lin_w=lwd.grad, g_lin_b=lbd.grad)
    check('fm', 'fm %s' % (case,), got, ref)


# ------------------------------------------------------------------------------------------------------------ rowdot
@pytest.mark.parametrize('case', hr.ROWDOT_CASES, ids=str)                    # the `d += 64` loop of rowdot_fwd_kernel
def test_rowdot(case):
    ops = _ops()
    a, c, go = hr.rowdot_inputs(case)
    ref = hr.rowdot_ref(a, c, go)
    ad, cd = dev_leaves(a, c)
    out = ops.rowdot(ad, cd)
    out.backward(go.to(DEV))
    check('rowdot', 'rowdot %s' % (case,), dict(out=out, g_a=ad.grad, g_c=cd.grad), ref)


# --------------------------------------------------------------------------------------------------------- bias head
@pytest.mark.parametrize('U', [3, 1])
@pytest.mark.parametrize('N', hr.BIAS_NS)                                    # sum_kernel's `i += 256` loop: 1, 1, 1, 2, 4 trips
@pytest.mark.parametrize('form', ['r_ids', 'ids', 'r'])                      # bias_head_fwd_kernel's three branches (`!ub`, `r`, else)
def test_bias_head(form, N, U):
    ops = _ops()
    r, ub, ib, gb, uid, iid, go = hr.bias_head_inputs(N, U)
    r = None if form == 'ids' else r
    if form == 'r':
        ub = ib = uid = iid = None
    ref = hr.bias_head_ref(r, ub, ib, gb, uid, iid, go)
    rd, ubd, ibd, gbd = dev_leaves(r, ub, ib, gb)
    god = go.to(DEV)
    out = ops.bias_head(rd, ubd, ibd, gbd, None if uid is None else uid.to(DEV), None if iid is None else iid.to(DEV))
    out.backward(god)
    got = dict(out=out, g_global=gbd.grad)
    if ub is not None:
        got.update(g_user_bias=ubd.grad, g_item_bias=ibd.grad)
    check('bias_head', 'bias_head %s N=%d U=%d' % (form, N, U), got, ref)
    if r is not None:
        assert hr.bits_equal(rd.grad, go)                                    # g_r is the incoming gradient itself


# ------------------------------------------------------------------------------------------- embed / rebuild_dense
@pytest.mark.parametrize('case', hr.EMBED_CASES, ids=str)                     # (D, n): `if (i >= n * D) return` of both kernels
def test_embed_gather_and_dense_scatter(case):
    ops = _ops()
    table, idx, g = hr.embed_inputs(case)
    (td,) = dev_leaves(table)
    out = ops.embed(td, idx.to(DEV))
    assert hr.bits_equal(out, table[idx])
    out.backward(g.to(DEV))
    val, bound = hr.multiplicity_sum(idx, g, hr.EMBED_ROWS)
    check('embed', 'embed %s' % (case,), dict(dense_scatter=td.grad), dict(dense_scatter=(val, bound)))
    assert hr.bits_equal(td.grad[7], torch.zeros(case[0]))                   # a row nobody names: +0
    # a [2, n / 2] index keeps its leading dimensions
    if idx.numel() % 2 == 0:
        assert hr.bits_equal(ops.embed(td.detach(), idx.reshape(2, -1).to(DEV)), table[idx.reshape(2, -1)])


@pytest.mark.parametrize('case', hr.ORDERED_CASES, ids=str)
def test_ordered_scatter_is_the_sequential_sum_in_entry_order(case):
    """embed_scatter_add_ordered_kernel: the `d0 += 64` loop (D = 1, 64, 65, 130), the 64-lane-strided duplicate search
    `k += 64` with duplicates of one row at entries 0, 63, 64, 65 and n - 1, row R - 1, -1 padding in front, at the end
    and everywhere.  The contract is an order, so the check is bits: a numpy float32 loop in ascending entry order."""
    ops = _ops()
    D, n, layout = case
    idx, rows = hr.ordered_inputs(D, n, layout)
    want = hr.ordered_scatter_np(idx.numpy(), rows.numpy(), hr.EMBED_ROWS)
    a = ops.rebuild_dense(idx.to(DEV), rows.to(DEV), hr.EMBED_ROWS, D)
    out = torch.full((hr.EMBED_ROWS, D), float('nan'), device=DEV)           # a caller's buffer: every row is written
    b = ops.rebuild_dense(idx.to(DEV), rows.to(DEV), hr.EMBED_ROWS, D, out=out)
    assert b is out
    assert hr.bits_equal(a, want)
    assert hr.bits_equal(b, want)


# ------------------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize('case', hr.TLOSS_CASES, ids=str)                     # N L = 1, 255, 256, 257, 7000: sqdist_mean_fwd's `i += 256`
def test_transform_loss(case):
    ops = _ops()
    a, b, gup = hr.tloss_inputs(case)
    ref = hr.transform_loss_ref(a, b, gup)
    ad, bd = dev_leaves(a, b)
    t = ops.transform_loss(ad, bd)
    assert t.shape == ()
    t.backward(torch.tensor(gup, device=DEV))                                # an upstream gradient other than 1
    check('transform_loss', 'transform_loss %s' % (case,), dict(out=t, g_a=ad.grad, g_b=bd.grad), ref)
    assert hr.bits_equal(bd.grad, -ad.grad)


@pytest.mark.parametrize('N', hr.MSE_NS)
def test_mse(N):
    ops = _ops()
    out, y = hr.vector_inputs(N, 0)
    denom = N + 3                                                            # not N: the mean over a global batch
    ref = hr.mse_ref(out, y, denom)
    se, g = ops.mse_fwd_bwd(out.to(DEV), y.to(DEV), denom)
    check('mse', 'mse %d' % N, dict(se=se, g=g), ref)
    se2, g2 = ops.mse_fwd_bwd(out.to(DEV), y.to(DEV), denom, want_grad=False)
    assert g2 is None and hr.bits_equal(se2, se)


@pytest.mark.parametrize('n', hr.ELEMENTWISE_NS)                             # `if (i < n)` around one 256-thread block
def test_mul_and_add_are_single_roundings(n):
    ops = _ops()
    a, b = hr.vector_inputs(n, 1)
    g, _ = hr.vector_inputs(n, 2)
    ad, bd = dev_leaves(a, b)
    m = ops.mul(ad, bd)
    m.backward(g.to(DEV))
    assert hr.bits_equal(m, a * b) and hr.bits_equal(ad.grad, g * b) and hr.bits_equal(bd.grad, g * a)
    ad, bd = dev_leaves(a, b)
    s = ops.add(ad, bd)
    s.backward(g.to(DEV))
    assert hr.bits_equal(s, a + b) and hr.bits_equal(ad.grad, g) and hr.bits_equal(bd.grad, g)


# --------------------------------------------------------------------------------------------------- NARRE attention
def attention_cabi(x, o, W0, b0, w3, b3, mult, go):
    """r4r_narre_attn_fwd / _bwd through the C ABI, so that h_save, a_save and an explicit mult are in hand."""
    L_ = _lib()
    ptr, lib = L_.ptr, L_.lib()
    N, R, L = x.shape
    x, o, W0, b0, w3, b3, go = (t.to(DEV).contiguous() for t in (x, o, W0, b0, w3, b3, go))
    mult = None if mult is None else mult.to(DEV).contiguous()
    nan = float('nan')
    got = dict(out=torch.full((N, L), nan, device=DEV), h_save=torch.full((N, R, L), nan, device=DEV),
               a_save=torch.full((N, R), nan, device=DEV), g_x=torch.full((N, R, L), nan, device=DEV),
               g_other=torch.full((N, R, L), nan, device=DEV), g_W0=torch.full((L, 2 * L), nan, device=DEV),
               g_b0=torch.full((L,), nan, device=DEV), g_w3=torch.full((1, L), nan, device=DEV),
               g_b3=torch.full((1,), nan, device=DEV))
    rc = lib.r4r_narre_attn_fwd(ptr(x), ptr(o), ptr(W0), ptr(b0), ptr(w3), ptr(b3), ptr(mult), ptr(got['out']),
                                ptr(got['h_save']), ptr(got['a_save']), N, R, L, L_.current_stream())
    L_.check(rc, 'r4r_narre_attn_fwd')
    ws = torch.empty(max(int(lib.r4r_narre_attn_ws_bytes(N, R, L)), 256), dtype=torch.uint8, device=DEV)
    rc = lib.r4r_narre_attn_bwd(ptr(x), ptr(o), ptr(W0), ptr(w3), ptr(mult), ptr(got['h_save']), ptr(got['a_save']), ptr(go),
                                ptr(got['g_x']), ptr(got['g_other']), ptr(got['g_W0']), ptr(got['g_b0']), ptr(got['g_w3']),
                                ptr(got['g_b3']), ptr(ws), ws.numel(), N, R, L, L_.current_stream())
    L_.check(rc, 'r4r_narre_attn_bwd')
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('dropout', [False, True], ids=['nomult', 'mult'])   # `if (mult)` forward, `mult ? ... : 1.f` backward
@pytest.mark.parametrize('name', list(hr.ATTN_CASES))                        # what each case targets: head_ref.ATTN_CASES
def test_narre_attention(name, dropout):
    inp = hr.attention_inputs(name, dropout)
    ref = hr.attention_ref(*inp)
    got = attention_cabi(*inp)
    check('narre_attention', 'attention %s' % name, got, ref)
    N, R, L, kind = hr.ATTN_CASES[name]
    if kind == 'identical' and not dropout:                                  # weights 1 / R to within the bound
        assert bool(((got['a_save'].cpu().double() - 1.0 / R).abs() <= ref['a_save'][1]).all())
    if kind == 'padded':                                                     # all-zero reviews still receive weight
        pad = (inp[0] == 0).all(-1) & (inp[1] == 0).all(-1)
        assert bool((got['a_save'].cpu()[pad] > 0).all())


def test_narre_attention_glue_draws_and_reuses_one_multiplier():
    """ops.narre_attention(training=True): the multiplier drawn in the forward (read back through DropoutState.record)
    is the one the backward applies."""
    ops = _ops()
    x, o, W0, b0, w3, b3, _, go = hr.attention_inputs('rows260', False)
    ops.DropoutState.manual_seed(11)
    ops.DropoutState.record = {}
    try:
        xd, od, W0d, b0d, w3d, b3d = dev_leaves(x, o, W0, b0, w3, b3)
        out = ops.narre_attention(xd, od, W0d, b0d, w3d, b3d, p=0.5, training=True, site='scorer')
        mult = ops.DropoutState.record['scorer']
    finally:
        ops.DropoutState.record = None
    vals = set(torch.unique(mult).tolist())
    assert vals == {0.0, 2.0}
    out.backward(go.to(DEV))
    ref = hr.attention_ref(x, o, W0, b0, w3, b3, mult, go)
    got = dict(out=out, g_x=xd.grad, g_other=od.grad, g_W0=W0d.grad, g_b0=b0d.grad, g_w3=w3d.grad, g_b3=b3d.grad)
    check('narre_attention', 'attention glue', got, ref, list(got))


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch():
    ops = _ops()
    L_ = _lib()
    ptr = L_.ptr
    one = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError, match=r'linear_bwd: n_in 256 out of range \(1\.\.255\)'):
        L_.call('r4r_linear_bwd', ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), None, 0, 1, 256, 1, 0)
    with pytest.raises(RuntimeError, match=r'fm_fwd: n=513 outside 1\.\.512'):
        ops.fm(torch.zeros((1, 513), device=DEV), torch.zeros((513, 2), device=DEV), torch.zeros((1, 513), device=DEV), one)
    with pytest.raises(RuntimeError, match=r'fm_bwd: n=513 outside 1\.\.512'):
        L_.call('r4r_fm_bwd', *[ptr(one)] * 8, 1, 513, 2)
    with pytest.raises(RuntimeError, match=r'fm_fwd: n=2 outside 1\.\.512 or k=4097 outside 1\.\.4096'):
        ops.fm(torch.zeros((1, 2), device=DEV), torch.zeros((2, 4097), device=DEV), torch.zeros((1, 2), device=DEV), one)
    for R, L in ((33, 2), (2, 33)):
        z = torch.zeros((1, R, L), device=DEV)
        with pytest.raises(RuntimeError, match=r'narre_attn_fwd: R=%d L=%d outside 1\.\.32' % (R, L)):
            ops.narre_attention(z, z, torch.zeros((L, 2 * L), device=DEV), torch.zeros(L, device=DEV),
                                torch.zeros((1, L), device=DEV), one)
        with pytest.raises(RuntimeError, match=r'narre_attn_bwd: R=%d L=%d outside 1\.\.32' % (R, L)):
            L_.call('r4r_narre_attn_bwd', *[ptr(one)] * 15, 4, 1, R, L)
    with pytest.raises(RuntimeError, match='mse_fwd_bwd: denom must be positive'):
        ops.mse_fwd_bwd(one, one, 0)


# --------------------------------------------------------------------------------------------- N = 0 through the C ABI
def test_empty_batch_gives_exact_zero_parameter_gradients():
    """r4r_linear_bwd, r4r_fm_bwd and r4r_narre_attn_bwd launch their reduction kernels for an empty batch too (`r1 =
    min(N, ...)` = 0, `for (b = rg; b < N; ...)` never entered): valid 1-element batch buffers, gradients pre-filled
    with NaN, every parameter gradient must come back as an exact zero with return code 0."""
    L_ = _lib()
    ptr, lib, st = L_.ptr, L_.lib(), L_.current_stream()
    one = torch.zeros(1, device=DEV)

    def nans(*shape):
        return torch.full(shape, float('nan'), device=DEV)

    n_in, n_out = 64, 3                                                      # the bias column alone in the second wave
    w = torch.randn((n_out, n_in), device=DEV)
    g_w, g_b = nans(n_out, n_in), nans(n_out)
    assert lib.r4r_linear_bwd_ws_bytes(0, n_in, n_out) == 0
    for relu in (0, 1):
        rc = lib.r4r_linear_bwd(ptr(one), ptr(w), ptr(one), ptr(one), ptr(one), ptr(g_w), ptr(g_b), None, 0, 0, n_in, n_out,
                                relu, st)
        assert rc == 0
        assert hr.bits_equal(g_w, torch.zeros(n_out, n_in)) and hr.bits_equal(g_b, torch.zeros(n_out))
        g_w.fill_(float('nan'))
        g_b.fill_(float('nan'))

    n, k = 65, 3                                                             # two blocks of 64 inputs
    V, lw = torch.randn((n, k), device=DEV), torch.randn((1, n), device=DEV)
    g_V, g_lw, g_lb = nans(n, k), nans(1, n), nans(1)
    rc = lib.r4r_fm_bwd(ptr(one), ptr(V), ptr(lw), ptr(one), ptr(one), ptr(g_V), ptr(g_lw), ptr(g_lb), 0, n, k, st)
    assert rc == 0
    assert hr.bits_equal(g_V, torch.zeros(n, k)) and hr.bits_equal(g_lw, torch.zeros(1, n)) and hr.bits_equal(g_lb, torch.zeros(1))

    R, L = 10, 10
    W0, w3 = torch.randn((L, 2 * L), device=DEV), torch.randn((1, L), device=DEV)
    g_W0, g_b0, g_w3, g_b3 = nans(L, 2 * L), nans(L), nans(1, L), nans(1)
    ws = torch.empty(int(lib.r4r_narre_attn_ws_bytes(0, R, L)), dtype=torch.uint8, device=DEV)
    assert ws.numel() == (L + 1) * 128 * 4
    rc = lib.r4r_narre_attn_bwd(ptr(one), ptr(one), ptr(W0), ptr(w3), None, ptr(one), ptr(one), ptr(one), ptr(one), ptr(one),
                                ptr(g_W0), ptr(g_b0), ptr(g_w3), ptr(g_b3), ptr(ws), ws.numel(), 0, R, L, st)
    assert rc == 0
    for t in (g_W0, g_b0, g_w3, g_b3):
        assert hr.bits_equal(t, torch.zeros(t.shape))
