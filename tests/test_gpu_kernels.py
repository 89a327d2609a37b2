"""Kernel-level parity: every C-ABI entry point vs the CPU oracle / a plain fp32
restatement on the same seeded inputs.  Runs on a real MI355X only (-m gpu)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle.models import textcnn_forward
from conv_ref import F16X2_EXTRA, check_pool, fp32_coef

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from reviews4rec_amd import ops
    return ops


def conv_pool_reference(idx, table, w, b):
    """Plain ATen restatement of gather -> conv -> relu -> max-pool, with indices."""
    x = F.embedding(idx, table).unsqueeze(1)
    y = F.relu(F.conv2d(x, w, b, padding=(2, 0))).squeeze(-1)          # [N, F, P]
    pooled, arg = F.max_pool1d(y, y.size(2), return_indices=True)
    return pooled.squeeze(-1), arg.squeeze(-1), y


TOWER_SHAPES = [
    # N, T, E, V
    (3, 37, 20, 50),       # E not a multiple of 16 (k padding), single tile
    (2, 300, 64, 200),     # several tiles, default embed size
    (5, 1, 4, 7),          # minimum document: P = 3
    (2, 126, 300, 90),     # P == 128 exactly one full tile, E = 300 (10 chunks, ragged last)
    (2, 127, 32, 90),      # P == 129: second tile holds one position
    (1, 1000, 300, 500),   # the BASELINE document shape
    (4, 100, 16, 60),      # NARRE review shape
    (3, 60, 50, 80),       # E = 50 (GloVe-50): not a multiple of 4 -- zero-padded rows inside ops (exact)
    (2, 40, 6, 30),        # E = 6
    (2, 200, 301, 300),    # E = 301
]


@pytest.mark.parametrize('N,T,E,V', TOWER_SHAPES)
def test_textcnn_forward_matches_aten(N, T, E, V):
    ops = _ops()
    g = torch.Generator().manual_seed(N * 1000 + T)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    idx = torch.randint(0, V, (N, T), generator=g)
    idx[0, T // 2:] = 0                                     # zero-padded tail
    ref_pooled, ref_arg, y = conv_pool_reference(idx, table, w, b)
    pooled, arg = ops.textcnn_fwd_raw(idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    pooled, arg = pooled.cpu(), arg.cpu().long()
    torch.testing.assert_close(pooled, ref_pooled, rtol=1e-5, atol=1e-6)
    # argmax: -1 exactly where the pooled value is 0; otherwise it must point at a position
    # whose conv output equals the max (ties between distinct windows are measure-zero)
    assert ((arg < 0) == (ref_pooled <= 0)).all()
    pos = arg >= 0
    picked = torch.gather(y, 2, arg.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    torch.testing.assert_close(picked[pos], ref_pooled[pos], rtol=1e-5, atol=1e-6)
    # every (n, f) against float64: pooled within its rounding bound, argmax the first of identical windows
    check_pool(idx, table, w, b, pooled, arg)


@pytest.mark.parametrize('N,T,E,V', [(70, 1000, 64, 3000), (700, 100, 64, 2000), (36, 1000, 300, 1500),
                                     (301, 300, 64, 2000), (701, 100, 64, 2000)])   # odd segment counts: a gather workgroup straddles documents
def test_textcnn_forward_auto_algorithm_at_scale(N, T, E, V):
    """>= 65536 positions (or E >= 128): R4R_CONV_AUTO runs project-then-gather inside
    r4r_textcnn_fwd (the small narrow shapes above run the direct conv); both must match ATen.  The whole suite is additionally run
    with R4R_CONV_ALGO=project / =direct pinned."""
    ops = _ops()
    g = torch.Generator().manual_seed(N + T + E)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    zipf = torch.distributions.Categorical(probs=1.0 / torch.arange(1, V + 1).float())
    idx = zipf.sample((N, T))
    fill = torch.randint(1, T + 1, (N, 1), generator=g)
    idx = torch.where(torch.arange(T)[None, :] < fill, idx, torch.zeros_like(idx))     # zero-padded tails
    ref_pooled, ref_arg, y = conv_pool_reference(idx, table, w, b)
    pooled, arg = ops.textcnn_fwd_raw(idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    pooled, arg = pooled.cpu(), arg.cpu().long()
    torch.testing.assert_close(pooled, ref_pooled, rtol=1e-5, atol=1e-6)
    assert ((arg < 0) == (ref_pooled <= 0)).all()
    pos = arg >= 0
    picked = torch.gather(y, 2, arg.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    torch.testing.assert_close(picked[pos], ref_pooled[pos], rtol=1e-5, atol=1e-6)
    check_pool(idx.to(DEV), table.to(DEV), w, b, pooled, arg)          # (float64 reference on the device)


def test_textcnn_all_negative_gives_zero_and_no_gradient():
    ops = _ops()
    V, E, T = 10, 8, 20
    table = torch.rand((V, E)) * 0.1
    w = -torch.rand((100, 1, 3, E))                         # every window negative
    b = -torch.ones(100)
    idx = torch.randint(0, V, (2, T))
    pooled, arg = ops.textcnn_fwd_raw(idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    assert (pooled == 0).all() and (arg == -1).all()
    d_w, d_b = ops.textcnn_wgrad_raw(idx.to(DEV), table.to(DEV), torch.ones((2, 100), device=DEV), arg, w.shape)
    assert (d_w == 0).all() and (d_b == 0).all()


def test_textcnn_first_index_on_ties():
    """Constant document: every interior window has the same value -> lowest index wins
    (PyTorch's max_pool picks the first maximum)."""
    ops = _ops()
    V, E, T = 4, 8, 300
    table = torch.rand((V, E)) + 0.5
    w = torch.rand((100, 1, 3, E)) * 0.1
    b = torch.zeros(100)
    idx = torch.full((1, T), 2, dtype=torch.int64)
    ref_pooled, ref_arg, _ = conv_pool_reference(idx, table, w, b)
    pooled, arg = ops.textcnn_fwd_raw(idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    torch.testing.assert_close(pooled.cpu(), ref_pooled, rtol=1e-5, atol=1e-6)
    assert (arg.cpu() == 2).all()                           # first full window is at p = 2


@pytest.mark.parametrize('N,T,E,V', TOWER_SHAPES[:5] + [(17, 60, 64, 40), (9, 60, 50, 80), (3, 40, 6, 30)])
def test_textcnn_wgrad_matches_autograd(N, T, E, V):
    ops = _ops()
    g = torch.Generator().manual_seed(7 + N + T)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w = ((torch.rand((100, 1, 3, E), generator=g) - 0.5) * 0.2).requires_grad_(True)
    b = ((torch.rand(100, generator=g) - 0.5) * 0.1).requires_grad_(True)
    idx = torch.randint(0, V, (N, T), generator=g)
    gp = torch.randn((N, 100), generator=g)
    ref_pooled, _, _ = conv_pool_reference(idx, table, w, b)
    ref_pooled.backward(gp)
    pooled, arg = ops.textcnn_fwd_raw(idx.to(DEV), table.to(DEV), w.detach().to(DEV), b.detach().to(DEV))
    d_w, d_b = ops.textcnn_wgrad_raw(idx.to(DEV), table.to(DEV), gp.to(DEV), arg, w.shape)
    torch.testing.assert_close(d_w.cpu(), w.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(d_b.cpu(), b.grad, rtol=1e-4, atol=1e-6)


def test_textcnn_rejects_bad_arguments():
    ops = _ops()
    table = torch.rand((5, 6), device=DEV)
    idx = torch.zeros((1, 4), dtype=torch.int64, device=DEV)
    # (E = 6 is accepted by the Python surface since round 3 -- padded rows; the C ABI still wants aligned
    # rows: tests/test_cabi.py -- so the loud failure checked here is the float64 table)
    with pytest.raises(RuntimeError, match='float32'):
        ops.textcnn_fwd_raw(idx, table.double(), torch.rand((100, 1, 3, 6), device=DEV), torch.rand(100, device=DEV))
    with pytest.raises(RuntimeError, match='ROCm device'):
        ops.textcnn_fwd_raw(idx.cpu(), table, torch.rand((100, 1, 3, 6), device=DEV), torch.rand(100, device=DEV))


@pytest.mark.parametrize('N,n_in,n_out,relu', [(7, 100, 10, False), (33, 20, 10, True), (1, 10, 1, False),
                                                (1280, 100, 10, False), (5, 255, 3, True)])
def test_linear_fwd_bwd(N, n_in, n_out, relu):
    ops = _ops()
    g = torch.Generator().manual_seed(N + n_in)
    x = torch.randn((N, n_in), generator=g).requires_grad_(True)
    w = (torch.randn((n_out, n_in), generator=g) * 0.1).requires_grad_(True)
    b = torch.randn(n_out, generator=g).requires_grad_(True)
    gy = torch.randn((N, n_out), generator=g)
    ref = F.linear(x, w, b)
    if relu:
        ref = F.relu(ref)
    ref.backward(gy)
    xd, wd, bd = (t.detach().to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.linear(xd, wd, bd, relu)
    y.backward(gy.to(DEV))
    torch.testing.assert_close(y.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xd.grad.cpu(), x.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(wd.grad.cpu(), w.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('N,n,k', [(9, 20, 8), (128, 10, 8), (3, 64, 64), (1, 12, 6), (7, 96, 8), (5, 128, 64), (3, 300, 5),
                                   (2, 512, 70)])      # n > 64: several inputs per lane (latent_size > 32)
def test_fm_fwd_bwd(N, n, k):
    ops = _ops()
    g = torch.Generator().manual_seed(N + n + k)
    P = {'fm.V': (torch.randn((n, k), generator=g) * 0.3).requires_grad_(True),
         'fm.lin.weight': (torch.randn((1, n), generator=g) * 0.3).requires_grad_(True),
         'fm.lin.bias': torch.randn(1, generator=g).requires_grad_(True)}
    x = torch.randn((N, n), generator=g).requires_grad_(True)
    go = torch.randn(N, generator=g)
    ref = oracle.fm_forward(P, 'fm', x)
    ref.backward(go)
    xd = x.detach().to(DEV).requires_grad_(True)
    Pd = {k2: v.detach().to(DEV).requires_grad_(True) for k2, v in P.items()}
    out = ops.fm(xd, Pd['fm.V'], Pd['fm.lin.weight'], Pd['fm.lin.bias'])
    out.backward(go.to(DEV))
    tol = 1e-5 if n <= 64 else 1e-4                        # (0.5 (s^2 - s2) cancels: the rounding grows with the input count)
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=tol, atol=tol)
    torch.testing.assert_close(xd.grad.cpu(), x.grad, rtol=1e-4, atol=tol)
    for k2 in P:
        torch.testing.assert_close(Pd[k2].grad.cpu(), P[k2].grad, rtol=1e-4, atol=1e-4, msg=lambda m: k2 + ': ' + m)


def test_embed_gather_and_dense_scatter_with_duplicates():
    ops = _ops()
    R, D = 50, 12
    table = torch.randn((R, D)).requires_grad_(True)
    idx = torch.tensor([[3, 3, 7], [49, 0, 3]])
    g = torch.randn((2, 3, D))
    ref = F.embedding(idx, table)
    ref.backward(g)
    td = table.detach().to(DEV).requires_grad_(True)
    out = ops.embed(td, idx.to(DEV))
    out.backward(g.to(DEV))
    assert torch.equal(out.detach().cpu(), ref.detach())
    torch.testing.assert_close(td.grad.cpu(), table.grad, rtol=1e-6, atol=1e-6)
    assert (td.grad.cpu()[[1, 2, 4]] == 0).all()            # untouched rows: exact zeros (dense grad)


def test_ordered_scatter_is_deterministic_and_skips_padding():
    """r4r_embed_scatter_add_ordered (the dense rebuild of the all-gathered compact lists): equals
    index_add, ignores -1 padding entries, and is bit-identical run to run with many duplicates."""
    ops = _ops()
    R, D, n = 40, 10, 600
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 7, (n,), generator=g)            # heavy duplication
    idx[::9] = -1                                           # padding entries
    rows = torch.randn((n, D), generator=g)
    keep = idx >= 0
    want = torch.zeros((R, D), dtype=torch.float64).index_add_(0, idx[keep], rows[keep].double()).float()
    a = ops.rebuild_dense(idx.to(DEV), rows.to(DEV), R, D)
    b = ops.rebuild_dense(idx.to(DEV), rows.to(DEV), R, D)
    torch.testing.assert_close(a.cpu(), want, rtol=1e-5, atol=1e-5)
    assert torch.equal(a, b)
    assert (a.cpu()[7:] == 0).all()


def test_sparse_capture_mode_matches_dense_backward():
    """With ops.SparseGradCapture on, the embedding / bias backward records compact contributions;
    rebuilding them gives the same dense gradients the default backward produces."""
    ops = _ops()
    U, I, D, N = 30, 20, 8, 50
    g = torch.Generator().manual_seed(2)
    ue, ub, ib, gb = torch.randn((U, D), generator=g), torch.randn(U, generator=g), torch.randn(I, generator=g), torch.randn(1)
    uid, iid = torch.randint(0, U, (N,), generator=g).to(DEV), torch.randint(0, I, (N,), generator=g).to(DEV)
    go = torch.randn(N, generator=g).to(DEV)

    def run():
        P = [t.clone().to(DEV).requires_grad_(True) for t in (ue, ub, ib, gb)]
        out = ops.bias_head(ops.embed(P[0], uid).sum(-1), P[1], P[2], P[3], uid, iid)
        out.backward(go)
        return P

    ref = run()
    ops.SparseGradCapture.active = True
    ops.SparseGradCapture.clear()
    try:
        P = run()
        c = ops.SparseGradCapture.contributions
        for p, r, (R, Dp) in zip(P[:3], ref[:3], ((U, D), (U, 1), (I, 1))):
            (idx, rows), = c[p.data_ptr()]
            dense = ops.rebuild_dense(idx, rows, R, Dp).view_as(r.grad)
            torch.testing.assert_close(dense, r.grad, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(P[3].grad, ref[3].grad)
    finally:
        ops.SparseGradCapture.active = False
        ops.SparseGradCapture.clear()


def test_rowdot_and_bias_head():
    ops = _ops()
    N, D, U, I = 37, 64, 20, 11
    g = torch.Generator().manual_seed(5)
    a = torch.randn((N, D), generator=g).requires_grad_(True)
    c = torch.randn((N, D), generator=g).requires_grad_(True)
    ub = torch.randn(U, generator=g).requires_grad_(True)
    ib = torch.randn(I, generator=g).requires_grad_(True)
    gb = torch.randn(1, generator=g).requires_grad_(True)
    uid = torch.randint(0, U, (N,), generator=g)
    iid = torch.randint(0, I, (N,), generator=g)
    go = torch.randn(N, generator=g)
    ref = (a * c).sum(-1) + ub[uid] + ib[iid] + gb
    ref.backward(go)
    ad, cd, ubd, ibd, gbd = (t.detach().to(DEV).requires_grad_(True) for t in (a, c, ub, ib, gb))
    out = ops.bias_head(ops.rowdot(ad, cd), ubd, ibd, gbd, uid.to(DEV), iid.to(DEV))
    out.backward(go.to(DEV))
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    for mine, theirs in ((ad, a), (cd, c), (ubd, ub), (ibd, ib), (gbd, gb)):
        torch.testing.assert_close(mine.grad.cpu(), theirs.grad, rtol=1e-5, atol=1e-5)
    # no-ID-bias form (DeepCoNN 'deepconn' head)
    r = torch.randn(N, device=DEV, requires_grad=True)
    out2 = ops.bias_head(r, None, None, gbd, None, None)
    torch.testing.assert_close(out2.detach().cpu(), r.detach().cpu() + gb.detach(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('N,R,L', [(4, 10, 10), (1, 3, 5), (65, 10, 10), (3, 32, 32)])
def test_narre_attention_fwd_bwd(N, R, L):
    ops = _ops()
    from oracle.models import _narre_attention
    g = torch.Generator().manual_seed(N + R)
    P = {'s.0.weight': (torch.randn((L, 2 * L), generator=g) * 0.4).requires_grad_(True),
         's.0.bias': (torch.randn(L, generator=g) * 0.1).requires_grad_(True),
         's.3.weight': (torch.randn((1, L), generator=g) * 0.4).requires_grad_(True),
         's.3.bias': torch.randn(1, generator=g).requires_grad_(True)}
    x = torch.randn((N, R, L), generator=g).requires_grad_(True)
    o = torch.randn((N, R, L), generator=g).requires_grad_(True)
    go = torch.randn((N, L), generator=g)
    ref = _narre_attention(P, 's', x, o, 0.0, False, None)
    ref.backward(go)
    xd, od = (t.detach().to(DEV).requires_grad_(True) for t in (x, o))
    Pd = {k: v.detach().to(DEV).requires_grad_(True) for k, v in P.items()}
    out = ops.narre_attention(xd, od, Pd['s.0.weight'], Pd['s.0.bias'], Pd['s.3.weight'], Pd['s.3.bias'])
    out.backward(go.to(DEV))
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xd.grad.cpu(), x.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(od.grad.cpu(), o.grad, rtol=1e-4, atol=1e-5)
    for k in ('s.0.weight', 's.0.bias', 's.3.weight'):
        torch.testing.assert_close(Pd[k].grad.cpu(), P[k].grad, rtol=1e-4, atol=1e-4, msg=lambda m: k + ': ' + m)
    assert Pd['s.3.bias'].grad.abs().max() < 1e-5           # softmax shift invariance: true gradient is 0


def test_dropout_kernel_statistics_and_backward():
    ops = _ops()
    ops.DropoutState.manual_seed(123)
    x = torch.ones((1000, 257), device=DEV, requires_grad=True)
    ops.DropoutState.record = {}
    y = ops.dropout(x, 0.6, True, 'site')
    mult = ops.DropoutState.record['site']
    ops.DropoutState.record = None
    vals = torch.unique(mult.cpu())
    assert set(np.round(vals.numpy(), 5).tolist()) == {0.0, 2.5}
    keep = (mult > 0).float().mean().item()
    assert abs(keep - 0.4) < 0.005
    assert torch.equal(y.detach(), x.detach() * mult)
    y.sum().backward()
    assert torch.equal(x.grad, mult)
    # a different offset gives a different mask; the same (seed, offset) reproduces it
    ops.DropoutState.manual_seed(123)
    ops.DropoutState.record = {}
    ops.dropout(x.detach(), 0.6, True, 'site')
    again = ops.DropoutState.record['site']
    ops.dropout(x.detach(), 0.6, True, 'site')
    other = ops.DropoutState.record['site']
    ops.DropoutState.record = None
    assert torch.equal(again, mult) and not torch.equal(other, mult)
    assert ops.dropout(x, 0.6, False) is x and ops.dropout(x, 0.0, True) is x


def test_mse_and_transform_loss():
    ops = _ops()
    out, y = torch.randn(77), torch.randn(77)
    se, g = ops.mse_fwd_bwd(out.to(DEV), y.to(DEV), denom=77)
    torch.testing.assert_close(se.cpu(), (out - y) ** 2, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(g.cpu(), 2 * (out - y) / 77, rtol=1e-6, atol=1e-7)
    a = torch.randn((9, 10)).requires_grad_(True)
    b = torch.randn((9, 10)).requires_grad_(True)
    ref = (a - b).pow(2).sum(-1).mean()
    ref.backward()
    ad, bd = (t.detach().to(DEV).requires_grad_(True) for t in (a, b))
    t = ops.transform_loss(ad, bd)
    t.backward()
    torch.testing.assert_close(t.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ad.grad.cpu(), a.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('sizes', [[1], [7, 8193, 3], [16384, 5, 100000], list(range(1, 20))])
def test_fused_adam_matches_oracle(sizes):
    from reviews4rec_amd.optim import Adam
    g = torch.Generator().manual_seed(sum(sizes))
    P = {str(i): torch.randn(n, generator=g) for i, n in enumerate(sizes)}
    dev = [torch.nn.Parameter(v.clone().to(DEV)) for v in P.values()]
    opt = Adam(dev, lr=0.002, weight_decay=1e-6)
    state = oracle.AdamState()
    for step in range(3):
        grads = {k: torch.randn(v.shape, generator=g) for k, v in P.items()}
        if step == 1:
            grads['0'] = None                               # a skipped parameter keeps its own step count
        oracle.adam_step(P, grads, state, 0.002, 1e-6)
        for p, gr in zip(dev, grads.values()):
            p.grad = None if gr is None else gr.to(DEV)
        opt.step()
    for p, ref in zip(dev, P.values()):
        torch.testing.assert_close(p.detach().cpu(), ref, rtol=1e-5, atol=1e-6)
    for i, p in enumerate(dev):
        torch.testing.assert_close(opt.state[id(p)]['exp_avg'].cpu(), state.m[str(i)], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(opt.state[id(p)]['exp_avg_sq'].cpu(), state.v[str(i)], rtol=1e-5, atol=1e-9)


def test_fused_adam_unaligned_views_and_untouched_rows():
    """Weight decay moves rows that received a zero gradient."""
    from reviews4rec_amd.optim import Adam
    base = torch.randn(1000 + 3, device=DEV)
    before = base[3:].cpu().clone()
    p = torch.nn.Parameter(base[3:])                        # 12-byte offset: the scalar path
    assert p.data_ptr() % 16 != 0
    ref = {'p': p.detach().cpu().clone()}
    opt = Adam([p], lr=0.002, weight_decay=1e-6)
    grad = torch.zeros(1000)
    grad[:10] = 1.0
    p.grad = grad.to(DEV)
    opt.step()
    st = oracle.AdamState()
    oracle.adam_step(ref, {'p': grad}, st, 0.002, 1e-6)
    torch.testing.assert_close(p.detach().cpu(), ref['p'], rtol=1e-5, atol=1e-6)
    assert (p.detach().cpu()[10:] != before[10:]).all()


@pytest.mark.parametrize('V', [336, 340, 1000, 3000, 8200, 9000, 16000, 16390, 17300, 20300, 21000, 24100, 25000, 28672, 29500, 30100, 30300, 30700, 30720, 30730,
                               36000, 41000, 45000, 70000, 100000])
def test_projection_gemm_balanced_form_is_bit_identical_to_the_tile_form(V):
    """The projection GEMM has two decompositions (csrc/project.hip): 128-row tiles, and the balanced form --
    7 private row tiles per workgroup + a row tile shared column-wise by >= 3 workgroups -- chosen on the
    device from the distinct-token count.  Counts on both sides of every edge of that plan (exactly 7 row
    tiles per workgroup, a shared tile split 3 / 4 / 5 ways, the 256-workgroup cap, counts where the plan
    does not apply): same bits either way, and equal to ATen.  The tile form cuts the tiles of its last, partial
    round into column parts when that round fills at most half of the grid (36,000 rows: 26 tiles in 4 parts;
    41,000: 65 tiles in 2; 70,000: two full rounds + 35 tiles in 4): r4r_gemm_form(2) -- whole tiles only -- must
    give the same bits too.  Form 3 (A-resident) takes 4 .. 7 private row tiles per workgroup -- 8,200 .. 17,300 rows:
    4; 20,300 / 21,000: 5; 24,100 / 25,000: 6; 28,672 .. 30,720: 7, each with and without shared row tiles, from
    30,100 on with row tiles shared by only two workgroups (up to 10 column units per sharer: 30,720 rows = 7 1/2
    row tiles on each of the 256 workgroups is the form's capacity) -- and falls back to the tile form elsewhere."""
    from reviews4rec_amd import _lib
    ops = _ops()
    E, T = 128, 100
    N = -(-V // T) + 3
    g = torch.Generator().manual_seed(V)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    idx = torch.cat([torch.randperm(V, generator=g), torch.randint(0, V, (N * T - V,), generator=g)]).view(N, T)
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))          # every one of the V rows is distinct-used
    lib = _lib.lib()
    try:
        lib.r4r_gemm_form(0)
        p0, a0 = ops.textcnn_fwd_raw(*args)
        p0, a0 = p0.clone(), a0.clone()
        lib.r4r_gemm_form(1)
        p1, a1 = ops.textcnn_fwd_raw(*args)
        p1, a1 = p1.clone(), a1.clone()
        lib.r4r_gemm_form(2)
        p2, a2 = ops.textcnn_fwd_raw(*args)
        p2, a2 = p2.clone(), a2.clone()
        lib.r4r_gemm_form(3)                                # the A-resident form of the balanced plan (E = 128: 8 resident chunks)
        p3, a3 = ops.textcnn_fwd_raw(*args)
        p3, a3 = p3.clone(), a3.clone()
        lib.r4r_gemm_form(4)                                # the weight-resident form (E = 128: its widest table)
        p4, a4 = ops.textcnn_fwd_raw(*args)
    finally:
        lib.r4r_gemm_form(-1)
    assert torch.equal(p0, p1) and torch.equal(a0, a1)
    assert torch.equal(p0, p2) and torch.equal(a0, a2)
    assert torch.equal(p0, p3) and torch.equal(a0, a3)
    assert torch.equal(p0, p4) and torch.equal(a0, a4)
    if V <= 3000:
        ref_pooled, ref_arg, y = conv_pool_reference(idx, table, w, b)
        torch.testing.assert_close(p1.cpu(), ref_pooled, rtol=1e-5, atol=1e-6)
    check_pool(*args, p1, a1)                                # every V: each (n, f) against float64, argmax exact


@pytest.mark.parametrize('E,V', [(4, 40), (16, 500), (20, 3000), (48, 7000), (64, 19744), (64, 19750), (64, 50000), (64, 77000),
                                 (100, 9000), (128, 20000)])
def test_projection_gemm_weight_resident_form_is_bit_identical_to_the_tile_form(E, V):
    """Form 4 of the projection GEMM (csrc/project.hip 2d: the tower's weights resident in LDS, units of 16 rows x 4
    column tiles round-robin over the waves; the default for E <= 64, i.e. NARRE's and TransNet's tables) against the
    128-row tile form: every K-chunk count 1 .. 8 incl. ragged K tails (E = 20, 100), cfg4's row count (19,744 =
    1,234 row tiles exactly; 19,750: a partial last tile) and cfg5's (77,000), one unit per wave and many."""
    from reviews4rec_amd import _lib
    ops = _ops()
    T = 100
    N = max(-(-V // T) + 3, 660)                             # >= 65,536 positions: the static rule runs project-then-gather
    g = torch.Generator().manual_seed(V + E)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    idx = torch.cat([torch.randperm(V, generator=g), torch.randint(0, V, (N * T - V,), generator=g)]).view(N, T)
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    lib = _lib.lib()
    try:
        lib.r4r_gemm_form(0)
        p0, a0 = ops.textcnn_fwd_raw(*args)
        p0, a0 = p0.clone(), a0.clone()
        lib.r4r_gemm_form(4)
        p4, a4 = ops.textcnn_fwd_raw(*args)
    finally:
        lib.r4r_gemm_form(-1)
    assert torch.equal(p0, p4) and torch.equal(a0, a4)
    if V <= 3000:
        ref_pooled, ref_arg, y = conv_pool_reference(idx, table, w, b)
        torch.testing.assert_close(p4.cpu(), ref_pooled, rtol=1e-5, atol=1e-6)
    check_pool(*args, p4, a4)


@pytest.mark.parametrize('N,T,E,V,tscale', [(36, 1000, 300, 1500, 0.011), (700, 100, 64, 2000, 1.0), (64, 1000, 300, 20000, 3.0)])
def test_fp16_split_gemm_is_as_accurate_as_the_fp32_gemm(N, T, E, V, tscale):
    """The opt-in arithmetic of the projection GEMM (csrc/project_f16.hip: hi + lo fp16 operands, three f16-MFMA
    products per fp32 product, fp32 accumulation, exact power-of-two scaling) against a float64 convolution: its
    error must be of the fp32 GEMM's order (measured: at or below it), the argmax identical, a table row four
    orders of magnitude below the maximum included."""
    if os.environ.get('R4R_CONV_ALGO') == 'direct':
        pytest.skip('R4R_CONV_ALGO=direct: no projection GEMM runs')
    from reviews4rec_amd import _lib
    ops = _ops()
    lib = _lib.lib()
    g = torch.Generator().manual_seed(N + T)
    table = (torch.rand((V, E), generator=g) * 2 - 1) * tscale
    table[5] *= 1e-4
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    zipf = torch.distributions.Categorical(probs=1.0 / torch.arange(1, V + 1).float())
    idx = zipf.sample((N, T))
    idx[0, :7] = 5
    x = F.embedding(idx, table.double()).unsqueeze(1)
    ref = F.relu(F.conv2d(x, w.double(), b.double(), padding=(2, 0))).squeeze(-1).max(dim=2).values
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    try:
        lib.r4r_gemm_math(0, 0.0, 0.0)
        p32, a32 = ops.textcnn_fwd_raw(*args)
        p32, a32 = p32.cpu().double(), a32.cpu()
        lib.r4r_gemm_math(2, float(table.abs().max()), float(w.abs().max()))
        p16, a16 = ops.textcnn_fwd_raw(*args)
        p16, a16 = p16.cpu().double(), a16.cpu()
    finally:
        lib.r4r_gemm_math(0, 0.0, 0.0)
    scale = float(ref.abs().max())
    e32, e16 = float((p32 - ref).abs().max()) / scale, float((p16 - ref).abs().max()) / scale
    assert e16 <= 2.0 * e32 + 1e-7, (e32, e16)
    assert not torch.equal(p16, p32)                         # (it really ran the other arithmetic)
    assert float((a16 == a32).float().mean()) > 0.9999
    torch.testing.assert_close(p16.float(), ref.float(), rtol=1e-5, atol=1e-6)
    check_pool(*args, p32, a32)                              # each (n, f) to its own bound, argmax exact
    check_pool(*args, p16, a16, coef=fp32_coef(E) + F16X2_EXTRA)


@pytest.mark.parametrize('world,n,B_pad', [(1, 5, 5), (2, 3, 7), (3, 0, 4), (2, 128, 128)])
def test_dp_pack_and_unpack_move_every_field_of_every_rank(world, n, B_pad):
    """csrc/dp_pack.hip: a rank's entry fields -> one padded block; the ranks' blocks -> rank-major field arrays
    (ids padded with -1, values with 0): bit-exact against plain indexing."""
    import ctypes
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    g = torch.Generator().manual_seed(world * 1000 + n)
    spec = [(1, torch.int64), (1, torch.int64), (1, torch.float32), (5, torch.float32), (16, torch.float32)]
    units = (ctypes.c_int * len(spec))(*[w * (2 if dt == torch.int64 else 1) for w, dt in spec])
    ones = (ctypes.c_int * len(spec))(*[1 if dt == torch.int64 else 0 for _, dt in spec])
    nbytes = lib.r4r_dp_block_bytes(len(spec), units, B_pad)
    assert nbytes % 256 == 0 and nbytes >= sum(B_pad * w * (8 if dt == torch.int64 else 4) for w, dt in spec)
    blocks = torch.zeros(world * nbytes, dtype=torch.uint8, device=DEV)
    fields = []
    for r in range(world):
        nr = max(n - r, 0)                                   # ragged shards
        mine = [(torch.randint(0, 1 << 40, (nr,), generator=g) if dt == torch.int64 else torch.randn(nr, w, generator=g)).to(DEV)
                for w, dt in spec]
        fields.append((nr, mine))
        src = (ctypes.c_uint64 * len(spec))(*[(t.data_ptr() if nr else 0) for t in mine])
        block = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=DEV)      # (every byte the layout names is written)
        _lib.check(lib.r4r_dp_pack(len(spec), src, units, ones, nr, B_pad, ptr(block), _lib.current_stream()), 'r4r_dp_pack')
        blocks[r * nbytes:(r + 1) * nbytes] = block
    outs = [torch.empty((world * B_pad,) + ((w,) if w > 1 else ()), dtype=dt, device=DEV) for w, dt in spec]
    dst = (ctypes.c_uint64 * len(spec))(*[o.data_ptr() for o in outs])
    _lib.check(lib.r4r_dp_unpack(len(spec), dst, units, ptr(blocks), world, B_pad, _lib.current_stream()), 'r4r_dp_unpack')
    torch.cuda.synchronize()
    for f, (w, dt) in enumerate(spec):
        want = torch.full_like(outs[f], -1) if dt == torch.int64 else torch.zeros_like(outs[f])
        for r, (nr, mine) in enumerate(fields):
            if nr:
                want[r * B_pad:r * B_pad + nr] = mine[f].reshape(want[r * B_pad:r * B_pad + nr].shape)
        assert torch.equal(outs[f], want), f


@pytest.mark.parametrize('N,T,E,V', [(32, 200, 300, 500), (40, 120, 128, 300), (17, 60, 702, 90)])
def test_wide_wgrad_buffer_batches_equal_the_per_row_loads(N, T, E, V, monkeypatch):
    """The wide weight gradient reads a round's rows through a buffer resource, eight requested together, skipped slots
    answered with zeros by the range check; tables of 4 GB and more keep one load per contributing row.  Same
    additions in the same order: the same bits (R4R_WGRAD_ROWS=loop selects the per-row form of the stand-alone op)."""
    ops = _ops()
    g = torch.Generator().manual_seed(N * 7 + E)
    table = ((torch.rand((V, E), generator=g) - 0.5) * 0.2).to(DEV)
    w = ((torch.rand((100, 1, 3, E), generator=g) - 0.5) * 0.2).to(DEV)
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    b[::5] = -10.0                                                       # every fifth filter dead: argmax -1, skipped slots
    b = b.to(DEV)
    idx = torch.randint(0, V, (N, T), generator=g).to(DEV)
    gp = torch.randn((N, 100), generator=g).to(DEV)
    pooled, arg = ops.textcnn_fwd_raw(idx, table, w, b)
    assert (arg < 0).any() and (arg >= 0).any()
    d_w, d_b = ops.textcnn_wgrad_raw(idx, table, gp, arg, w.shape)
    monkeypatch.setenv('R4R_WGRAD_ROWS', 'loop')
    l_w, l_b = ops.textcnn_wgrad_raw(idx, table, gp, arg, w.shape)
    assert torch.equal(d_w, l_w) and torch.equal(d_b, l_b)
