"""Both TextCNN conv algorithms -- the direct gather-fused MFMA conv (csrc/textcnn.hip) and project-then-gather in
every projection-GEMM form and under the f16x2 arithmetic (csrc/project.hip, project_f16.hip) -- against the float64
reference of tests/conv_ref.py, at the edges of the gather's slicing (short last segments, uniform slices, the
segment-pair rotation, the merge of slices in position order), of the direct conv's tile height (128 -> 256 rows at
T + 2 > 160) and of the GEMM forms' 2 GB guard.  Every (document, filter) is checked exactly: pooled value within its
rounding bound, argmax the FIRST of identical windows.  Runs on a real MI355X only (-m gpu)."""
import contextlib
import math

import pytest
import torch

from conv_ref import F16X2_EXTRA, check_pool, check_wgrad, fp32_coef

pytestmark = pytest.mark.gpu

DEV = 'cuda'
AUTO, DIRECT, PROJECT = 0, 1, 2
SEG = 128                                                   # positions per gather segment (csrc/project.hip)


def _lib():
    from reviews4rec_amd import _lib
    return _lib.lib()


def _ops():
    from reviews4rec_amd import ops
    return ops


@contextlib.contextmanager
def conv_algo(algo, form=-1, math_mode=0, scales=(0.0, 0.0)):
    """r4r_textcnn_fwd runs `algo` (GEMM form / arithmetic on the project path) inside the block; restored after."""
    lib = _lib()
    try:
        assert lib.r4r_textcnn_algo(algo) >= 0
        lib.r4r_gemm_form(form)
        assert lib.r4r_gemm_math(math_mode, *scales) == 0
        yield
    finally:
        lib.r4r_textcnn_algo(AUTO)
        lib.r4r_gemm_form(-1)
        lib.r4r_gemm_math(0, 0.0, 0.0)


def runs(algo, N, T, E):
    """Whether a request for `algo` really runs it (an R4R_CONV_ALGO pin overrides the hook)."""
    return _lib().r4r_conv_algo(algo, N, T, E, 100) == algo


def fwd(args, algo, **kw):
    with conv_algo(algo, **kw):
        p, a = _ops().textcnn_fwd_raw(*args)
        torch.cuda.synchronize()
    return p.clone(), a.clone()


def make_weights(E, g, F=100):
    w = (torch.rand((F, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(F, generator=g) - 0.5) * 0.1
    return w, b


def make_indices(N, T, V, g):
    """Every one of the V rows used when V <= N * T (a permutation, then random fill), in random order."""
    if V <= N * T:
        flat = torch.cat([torch.randperm(V, generator=g), torch.randint(0, V, (N * T - V,), generator=g)])
        flat = flat[torch.randperm(N * T, generator=g)]
    else:
        flat = torch.randint(0, V, (N * T,), generator=g)
    return flat.view(N, T)


def gather_boundaries(T):
    """Every position where a gather slice or segment starts (csrc/project.hip: full segments in slices of 32, a
    shorter last one in slices of ceil(len / 4))."""
    P = T + 2
    out = set()
    for s0 in range(0, P, SEG):
        ln = min(SEG, P - s0)
        sl = 32 if ln == SEG else -(-ln // 4)
        out.update(range(s0, s0 + ln, sl))
    return sorted(out)


def both_algorithms(args, N, T, E, forms=(0, 1, 2, 3, 4), f16=False, coef=None):
    """Direct conv, project-then-gather in every form (bit-identical to each other and to the default form), f16x2:
    every output through check_pool.  Returns {algo: (pooled, argmax)}."""
    idx, table, w, b = args
    coef = fp32_coef(E) if coef is None else coef
    out = {}
    if runs(DIRECT, N, T, E):
        out[DIRECT] = fwd(args, DIRECT)
        check_pool(idx, table, w, b, *out[DIRECT], coef=coef)
    if runs(PROJECT, N, T, E):
        p, a = out[PROJECT] = fwd(args, PROJECT)
        check_pool(idx, table, w, b, p, a, coef=coef)
        for form in forms:
            pf, af = fwd(args, PROJECT, form=form)
            assert torch.equal(pf, p) and torch.equal(af, a), 'GEMM form %d differs from the default form' % form
        if f16:
            scales = (float(table.abs().max()), float(w.abs().max()))
            p16, a16 = fwd(args, PROJECT, math_mode=2, scales=scales)
            check_pool(idx, table, w, b, p16, a16, coef=coef + F16X2_EXTRA)
    assert out, 'neither algorithm ran'
    return out


# ------------------------------------------------------------------------------------------- forward matrix
# (N, T, E, V, f16): V = 0 -> N * T // 2 (below N * T, every row used); V = -1 -> far above N * T; V = 1.
# f16: also under the f16x2 arithmetic.  E: K tails, the E % 4 padding inside ops, form 4's width limit (64 by default,
# 128 pinned) and form 3's (320).
FWD_CASES = [
    (5, 1, 4, 0, 0), (5, 1, 6, 1, 0), (7, 2, 20, -1, 0), (7, 3, 4, 0, 0), (3, 3, 300, 1, 0),       # P = 3 / 4 / 5: slices 1,1,1,0 ...
    (3, 126, 16, 0, 0), (3, 127, 64, -1, 0), (3, 128, 68, 0, 0), (2, 129, 6, 0, 0), (3, 131, 50, 0, 0),   # P = 128; last segment 1 / 2 / 3 / 5
    (9, 100, 64, 0, 1), (3, 1000, 300, 0, 1),                                            # slices 26,26,26,24; 27,27,27,25
    (3, 158, 320, 0, 0), (2, 159, 324, -1, 1), (3, 254, 64, 0, 0), (2, 255, 20, 1, 0),   # 128 -> 256-row direct tiles; P = 256 / 257
    (5, 300, 20, 0, 1), (35, 510, 64, 0, 1), (2, 1022, 4, 0, 0), (3, 1023, 128, -1, 0),  # odd tiles x odd N; rotation; 8 / 9 segments
]


@pytest.mark.parametrize('N,T,E,V,f16', FWD_CASES)
def test_forward_matrix_both_algorithms_every_form(N, T, E, V, f16):
    g = torch.Generator().manual_seed(N * 7919 + T * 31 + E)
    V = max(1, N * T // 2) if V == 0 else (50 * N * T + 7 if V == -1 else V)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w, b = make_weights(E, g)
    idx = make_indices(N, T, V, g)
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    both_algorithms(args, N, T, E, f16=bool(f16))


# ----------------------------------------------------------------------------------------- ties and padding
@pytest.mark.parametrize('T', [100, 300, 1023])
@pytest.mark.parametrize('zero_pad', [True, False])
def test_ties_and_padding_at_every_slice_and_segment_boundary(T, zero_pad):
    """A hot token in runs of 3+ and zero-padded tails starting two positions either side of every slice / segment
    start; an all-padding document, one without padding.  Half the filters have a bias above every real window of
    theirs, so that in padded documents the first all-padding window must win (row 0 zero) -- identical windows
    everywhere, the expected argmax exact under both algorithms.  One filter with bias 0 over the all-padding
    document: pooled 0, argmax -1."""
    E, F = 20, 100
    g = torch.Generator().manual_seed(T * 2 + zero_pad)
    V = 60
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    if zero_pad:
        table[0] = 0.0
    u = torch.randn(E, generator=g)
    table[1] = 10 * u / u.norm()                              # the hot token
    w, b = make_weights(E, g, F)
    b[::2] = 0.3                                             # above every real window of these filters
    b[1] = 0.0
    starts = sorted({o for p in gather_boundaries(T) for o in range(p - 4, p + 3) if 0 <= o <= T - 3})
    docs = []
    for o in starts:
        d = torch.randint(2, V, (T,), generator=g)
        ln = 3 + (o % 3) * 7                                 # runs of 3, 10, 17
        d[o:o + ln] = 1
        docs.append(d)
        d = torch.randint(2, V, (T,), generator=g)
        d[o:] = 0                                            # zero-padded tail from o
        docs.append(d)
    docs.append(torch.zeros(T, dtype=torch.int64))           # all padding
    docs.append(torch.randint(2, V, (T,), generator=g))     # no padding
    idx = torch.stack(docs)
    N = idx.shape[0]
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    out = both_algorithms(args, N, T, E, forms=(0, 4))
    for algo, (p, a) in out.items():
        p, a = p.cpu(), a.cpu()
        if zero_pad:                                         # the all-padding document: bias only, first window
            assert torch.equal(a[-2], torch.where(b > 0, 0, -1).int()), algo
            assert p[-2, 1] == 0 and a[-2, 1] == -1
        assert (a[:, ::2] >= 0).all()


# ---------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize('N', [1, 15, 16, 17, 31, 33, 128])
@pytest.mark.parametrize('E', [6, 20, 300])
def test_wgrad_at_the_kernels_argmax_edge_positions(N, E):
    """Filters dominated by one tap along a direction u, a hot token 10 u at the first word (even documents) or the
    last (odd): argmaxes at positions 0, 1, T, T + 1 -- the windows with taps outside the document.  The weight
    gradient is checked against float64 at the kernel's own argmax, across the 16-document wgrad splits."""
    T, V, F = 40, 50, 100
    g = torch.Generator().manual_seed(N * 3 + E)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    u = torch.randn(E, generator=g)
    u /= u.norm()
    table[1] = 10 * u
    w = (torch.rand((F, 1, 3, E), generator=g) - 0.5) * 0.02
    for f in range(F):
        w[f, 0, f % 3] += (0.5 + f / F) * u
    b = (torch.rand(F, generator=g) - 0.5) * 0.1
    b[::7] = -50.0                                           # dead filters: argmax -1, no gradient
    idx = torch.randint(2, V, (N, T), generator=g)
    idx[0::2, 0] = 1
    idx[1::2, T - 1] = 1
    gp = torch.randn((N, F), generator=g)
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    seen = set()
    for algo in (DIRECT, PROJECT):
        if not runs(algo, N, T, E):
            continue
        p, a = fwd(args, algo)
        check_pool(*args, p, a)
        d_w, d_b = _ops().textcnn_wgrad_raw(args[0], args[1], gp.to(DEV), a, w.shape)
        check_wgrad(args[0], args[1], gp, a, d_w, d_b)
        seen |= set(a.unique().tolist())
    want = {-1, 0, 1, 2} | ({T - 1, T, T + 1} if N > 1 else set())
    assert want <= seen, sorted(want - seen)


# ------------------------------------------------------------------------------------------------ 2 GB guard
@pytest.mark.parametrize('V', [1766022, 1766023])
def test_projected_row_table_2gb_guard(V):
    """Forms 3 and 4 address the projected-row table (1,216 bytes a row) with 32-bit byte offsets; the launcher falls
    back to form 1 once cap * 1216 >= 2^31.  1,766,022 distinct rows: the largest table form 4 runs; one more: the
    fallback.  The default form must give the tile form's bits, and every document must pass check_pool (rows are
    placed by an atomic at run time: only all documents cover the table's top rows)."""
    N, T, E = 1767, 1000, 4
    assert N * T >= V
    if not runs(PROJECT, N, T, E):
        pytest.skip('R4R_CONV_ALGO pins the direct conv: no projection GEMM runs')
    g = torch.Generator().manual_seed(V)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    w, b = make_weights(E, g)
    idx = make_indices(N, T, V, g)
    args = (idx.to(DEV), table.to(DEV), w.to(DEV), b.to(DEV))
    p, a = fwd(args, PROJECT)
    p0, a0 = fwd(args, PROJECT, form=0)
    assert torch.equal(p, p0) and torch.equal(a, a0)
    check_pool(*args, p, a, chunk_docs=128)


# --------------------------------------------------------------------------------------------- engine level
ENGINE_T = {
    'deepconn': [1, 127, 159, 1022, 1023, 2047], 'deepconn++': [1, 127, 159, 1022, 1023, 2047],
    'transnet': [1, 127, 159, 1022, 1023, 2047], 'transnet++': [1, 127, 159, 1022, 1023, 2047],
    'NARRE': [1, 126, 127, 158, 159, 254, 255],              # review length W (159: one direct tile, two segments)
}


def engine_for(mt, hp, P, algo):
    import reviews4rec_amd
    from reviews4rec_amd import engine as E
    key = 'target.word2vec.weight' if mt.startswith('transnet') else 'word2vec.weight'
    model = reviews4rec_amd.get_model_class(mt)(dict(hp, word_vectors=P[key].numpy()))
    model.load_state_dict(P)
    model = model.to(DEV).eval()
    cls = {'deepconn': E.DeepCoNNEngine, 'deepconn++': E.DeepCoNNPPEngine, 'NARRE': E.NarreEngine}.get(mt, E.TransNetEngine)
    return cls(model, lr=hp['lr'], weight_decay=hp['weight_decay'], conv_algo=algo)


@pytest.mark.parametrize('mt,T,algo', [(mt, T, algo) for mt, Ts in ENGINE_T.items() for T in Ts for algo in (DIRECT, PROJECT)
                                        if not (T == 2047 and algo == PROJECT)])   # (2047: the direct conv's case)
def test_engine_predict_at_tile_edges_matches_float64_oracle(mt, T, algo):
    """predict() of every text engine at the documents' tile / segment edges (the heads' pool-finish past 8 tiles at
    T = 1023 under project-then-gather and T = 2047 under the direct conv's 256-row tiles) against the oracle in float64.
    Pooled values do not depend on how ties break, so the predictions must agree to the fp32 rounding of the tower."""
    import oracle
    from helpers import synthetic_review_batch
    B, E, V, U, I = 6, 20, 300, 30, 20
    narre = mt == 'NARRE'
    hp = dict(model_type=mt, latent_size=10, word_embed_size=E, input_length=T, dropout=0.0, total_users=U,
              total_items=I, lr=0.002, weight_decay=1e-6, narre_num_reviews=10, narre_num_words=T, batch_size=B)
    P = oracle.init_params(hp, vocab_size=V, seed=T + 3)
    data, y = synthetic_review_batch(B, T, V, U, I, seed=T, R=10 if narre else None, W=T if narre else None)
    eng = engine_for(mt, hp, P, algo)
    pred, _ = eng.predict([d.to(DEV) for d in data])
    ref = oracle.model_forward({k: v.double() for k, v in P.items()}, data, hp)
    ref = ref[0] if isinstance(ref, list) else ref
    torch.testing.assert_close(pred.cpu().double(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('algo', [DIRECT, PROJECT])
@pytest.mark.parametrize('T', [1, 127, 1023])
def test_deepconn_gradient_with_unique_argmax_at_the_document_edges(T, algo):
    """One gradient-only DeepCoNN launch against float64 autograd of the oracle, on data whose every (n, f) argmax is
    unique by a float64 margin far above the rounding bound: filters W[f, j] = a_fj u + small noise, a hot token 10 u
    at the first word (even documents) or the last (odd), so the argmax falls on positions 0, 1, 2, T - 1, T, T + 1."""
    import oracle
    from helpers import synthetic_review_batch
    from conv_ref import conv64
    B, E, V, U, I = 8, 20, 300, 30, 20
    hp = dict(model_type='deepconn', latent_size=10, word_embed_size=E, input_length=T, dropout=0.0, total_users=U,
              total_items=I, lr=0.002, weight_decay=1e-6, batch_size=B)
    P = oracle.init_params(hp, vocab_size=V, seed=T)
    g = torch.Generator().manual_seed(T)
    u = torch.randn(E, generator=g)
    u /= u.norm()
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.02
    table[1] = 10 * u
    P['word2vec.weight'] = table
    data, y = synthetic_review_batch(B, T, V, U, I, seed=T)
    for k, tower in ((3, 'user_conv'), (4, 'item_conv')):
        a = 0.2 + 0.3 * torch.argsort(torch.rand((100, 3), generator=g), dim=1).float()   # taps 0.3 apart, random order
        w = a[:, None, :, None] * u + (torch.rand((100, 1, 3, E), generator=g) - 0.5) * 0.002
        P[tower + '.convs.0.weight'] = w
        P[tower + '.convs.0.bias'] = (torch.rand(100, generator=g) - 0.5) * 0.1
        docs = torch.randint(2, V, (B, T), generator=g)
        docs[0::2, 0] = 1
        docs[1::2, T - 1] = 1
        data[k] = docs
        y64, S = conv64(docs, table, w, P[tower + '.convs.0.bias'])
        top2 = y64.topk(2, dim=2).values
        margin = top2[..., 0] - top2[..., 1]
        assert float(margin.min()) > 1e3 * fp32_coef(E) * float(S.max()), 'argmax not unique by a wide margin'
    eng = engine_for('deepconn', hp, P, algo)
    dd = [d.to(DEV) for d in data]
    eng._launch(dd, y.to(DEV), grad=True, training=True, inv_denom=1.0 / B)
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().double() for k, v in eng.grads().items()}
    P64 = {k: v.double().requires_grad_(k != 'word2vec.weight') for k, v in P.items()}
    pred = oracle.model_forward(P64, data, hp, train=True)
    oracle.mse_loss(pred, y.double(), return_mean=True).backward()
    for k, gk in got.items():
        ref = P64[k].grad
        torch.testing.assert_close(gk, ref, rtol=1e-4, atol=1e-6 * (1 + float(ref.abs().max())), msg=lambda m: k + ': ' + m)
