"""The TransNets' catalogue, the parts that need no GPU: the algebra of recommend.fold_transnet_head against the oracle's
TransNet forward in float64, recommend.transnet_catalogue_limits and the class's refusals, main's hooks (which still
refuse the TransNets) and the C ABI's refusals (r4r_topk_rfm / r4r_pair_rfm / r4r_rank_rfm, include/r4r.h)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


# ---------------------------------------------------------------- the fold
def tiny_weights(mt):
    """The weights of tests/golden/tiny/transnet++_eval.npz; for plain transnet source_fm.V / lin.weight cut to their
    last L rows and the id embeddings dropped."""
    from test_tiny_eval import _fixture, _weights
    W = _weights(_fixture('transnet++', 'eval')[1])
    if mt == 'transnet':
        L = W['source.project.2.weight'].shape[0]
        W = {k: v for k, v in W.items() if k not in ('user_embedding.weight', 'item_embedding.weight')}
        W['source_fm.V'] = W['source_fm.V'][-L:].clone()
        W['source_fm.lin.weight'] = W['source_fm.lin.weight'][:, -L:].clone()
    return W


def all_pairs(hp, reader):
    """Every user x item pair as a batch of ratings outside the training split: nothing removed from either document."""
    U, I = hp['total_users'], hp['total_items']
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    none = np.full(len(u), -1, np.int64)
    data = [torch.from_numpy(np.ascontiguousarray(f)) for f in reader._review_fields_host(u, i, none, none, none)]
    return u, i, data + [torch.from_numpy(u), torch.from_numpy(i)]


def folded_scores(q, qb, c, cb, head, H):
    """The ReLU-FM form in float64 -> (scores [n_q, n_c], Mag [n_q, n_c]: the sum of the terms' magnitudes)."""
    W, b, s, l = (np.asarray(t, np.float64) for t in head)
    q, qb, c, cb = (np.asarray(t, np.float64) for t in (q, qb, c, cb))
    x = q[:, None, :] + c[None, :, :]
    x[..., :H] = np.maximum(x[..., :H], 0.0)
    y = x @ W.T + b
    Y = np.abs(x) @ np.abs(W).T + np.abs(b)
    score = (y * (s * y + l)).sum(-1) + cb[None, :] + qb[:, None]
    mag = (np.abs(s) * Y * Y + np.abs(l) * Y).sum(-1) + np.abs(cb)[None, :] + np.abs(qb)[:, None]
    return score, mag


@pytest.mark.parametrize('mt', ['transnet++', 'transnet'])
def test_the_fold_is_the_test_time_score(mt, tmp_path):
    """Algebra, not rounding: the folded form in float64 == the oracle's TransNet forward [0] in float64 over all user x
    item pairs, to 1e-12 relative to the sum of the terms' magnitudes."""
    import oracle
    import oracle.models
    from reviews4rec_amd import fold_transnet_head
    from reviews4rec_amd.data import load_data
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(dict(tiny_hp('transnet++', root), model_type=mt), device='cpu')
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in tiny_weights(mt).items()}
    U, I, L = hp['total_users'], hp['total_items'], hp['latent_size']
    assert L == 6
    u, i, data = all_pairs(hp, test)
    with torch.no_grad():
        want = oracle.models.transnet_forward(P64, data, mt)[0].numpy().reshape(U, I)
        # the towers' latents: one document per owner (the pairs (u, 0) and (0, i) hold them)
        table = P64['target.word2vec.weight']
        emb = torch.nn.functional.embedding
        zu = oracle.models.textcnn_forward(P64, 'source.user_conv', emb(data[3].reshape(U, I, -1)[:, 0], table), 0.0, False, None)
        zi = oracle.models.textcnn_forward(P64, 'source.item_conv', emb(data[4].reshape(U, I, -1)[0], table), 0.0, False, None)
    pp = mt == 'transnet++'
    ue = P64['user_embedding.weight'][:U] if pp else None
    ie = P64['item_embedding.weight'][:I] if pp else None
    q, qb, head = fold_transnet_head(P64, hp, 'user', zu, emb=ue, dtype=torch.float64)
    c, cb = fold_transnet_head(P64, hp, 'item', zi, emb=ie, dtype=torch.float64)
    Pw, M = (8 if pp else 0), 8 + L + 1
    assert q.shape == (U, L + Pw) and c.shape == (I, L + Pw) and qb.shape == (U,) and cb.shape == (I,)
    assert [tuple(t.shape) for t in head] == [(M, L + Pw), (M,), (M,), (M,)]
    assert head[2].tolist() == [0.5] * 8 + [-0.5] * L + [0.0] and head[3].tolist() == [0.0] * (8 + L) + [1.0]
    got, mag = folded_scores(q.numpy(), qb.numpy(), c.numpy(), cb.numpy(), [t.numpy() for t in head], L)
    worst = float((np.abs(got - want) / mag).max())
    print('%s: fold against the oracle in float64, worst |difference| / Mag = %.3g' % (mt, worst))
    assert worst < 1e-12
    assert float(np.abs(want).max()) > 0.1                     # (not a comparison of zeros)
    # the default is one rounding of the same numbers to fp32
    q32, qb32, head32 = fold_transnet_head(P64, hp, 'user', zu, emb=ue)
    assert q32.dtype == qb32.dtype == head32[0].dtype == torch.float32
    assert torch.equal(q32, q.float()) and torch.equal(qb32, qb.float()) and torch.equal(head32[0], head[0].float())
    with pytest.raises(ValueError):
        fold_transnet_head(P64, hp, 'both', zu, emb=ue)
    with pytest.raises(ValueError):
        fold_transnet_head(P64, hp, 'user', zu, emb=None if pp else zu[:, :5])
    with pytest.raises(ValueError):
        fold_transnet_head(P64, dict(hp, model_type='NARRE'), 'user', zu)


def test_the_head_alone_at_a_latent_size_below_the_embedding_width():
    """TransNetCatalogue.refresh() takes the head from a fold of ZERO user rows: at latent_size 3 < 5 (the id embeddings'
    width) that is z [0, 3] with emb [0, 5]; head=False skips building it (the per-call query side)."""
    from reviews4rec_amd import fold_transnet_head
    gen = torch.Generator().manual_seed(3)
    L = 3
    f = lambda *sh: torch.randn(sh, generator=gen)
    P = {'source.project.0.weight': f(L, 2 * L), 'source.project.0.bias': f(L), 'source.project.2.weight': f(L, L),
         'source.project.2.bias': f(L), 'source_fm.V': f(10 + L, 8), 'source_fm.lin.weight': f(1, 10 + L),
         'source_fm.lin.bias': f(1)}
    hp = dict(model_type='transnet++', latent_size=L)
    rows, qb, head = fold_transnet_head(P, hp, 'user', torch.zeros(0, L), emb=torch.zeros(0, 5))
    assert rows.shape == (0, L + 8) and qb.shape == (0,)
    assert [tuple(t.shape) for t in head] == [(8 + L + 1, L + 8), (8 + L + 1,), (8 + L + 1,), (8 + L + 1,)]
    z, e = f(4, L), f(4, 5)
    full, lean = fold_transnet_head(P, hp, 'user', z, emb=e), fold_transnet_head(P, hp, 'user', z, emb=e, head=False)
    assert lean[2] is None and torch.equal(lean[0], full[0]) and torch.equal(lean[1], full[1])
    assert all(torch.equal(a, b) for a, b in zip(full[2], head))          # the head does not depend on the rows
    with pytest.raises(ValueError):
        fold_transnet_head(P, hp, 'user', torch.zeros(0, L), emb=torch.zeros(0, L))


# ---------------------------------------------------------------- limits, refusals, export
def test_transnet_catalogue_limits_and_export():
    import reviews4rec_amd
    from reviews4rec_amd import transnet_catalogue_limits
    assert reviews4rec_amd.TransNetCatalogue is reviews4rec_amd.recommend.TransNetCatalogue
    assert reviews4rec_amd.fold_transnet_head is reviews4rec_amd.recommend.fold_transnet_head
    assert reviews4rec_amd.TransNetCatalogue._form == 'rfm'
    assert issubclass(reviews4rec_amd.TransNetCatalogue, reviews4rec_amd.Catalogue)
    for name in ('recommend', 'score_pairs', 'rank'):         # Catalogue's own calls, unchanged
        assert getattr(reviews4rec_amd.TransNetCatalogue, name) is getattr(reviews4rec_amd.Catalogue, name)
    for mt in ('transnet', 'transnet++'):
        assert transnet_catalogue_limits(dict(model_type=mt)) is None
        assert transnet_catalogue_limits(dict(model_type=mt, latent_size=64)) is None
        assert 'latent_size 65 > 64' in transnet_catalogue_limits(dict(model_type=mt, latent_size=65))
    serves = {'bias_only': 'Catalogue', 'MF_dot': 'Catalogue', 'deepconn': 'Catalogue', 'deepconn++': 'ReluCatalogue',
              'NeuMF': 'ReluCatalogue', 'NARRE': 'NarreCatalogue'}
    for mt, cls in serves.items():
        why = transnet_catalogue_limits(dict(model_type=mt, latent_size=8))
        assert repr(mt) in why and (cls + ' serves it') in why, (mt, why)
    why = transnet_catalogue_limits(dict(model_type='MF', latent_size=8))
    assert repr('MF') in why and 'no class serves it' in why
    with pytest.raises(RuntimeError, match='NarreCatalogue serves it'):
        reviews4rec_amd.TransNetCatalogue(None, dict(model_type='NARRE'), None)
    with pytest.raises(RuntimeError, match='latent_size 65 > 64'):
        reviews4rec_amd.TransNetCatalogue(None, dict(model_type='transnet', latent_size=65), None)
    model = reviews4rec_amd.get_model_class('MF_dot')(dict(model_type='MF_dot', latent_size=4, total_users=3, total_items=3,
                                                           dropout=0.0))
    with pytest.raises(RuntimeError, match='ROCm device'):     # no CPU fallback
        reviews4rec_amd.TransNetCatalogue(model, dict(model_type='transnet', latent_size=6), None)


@pytest.mark.parametrize('mt', ['transnet', 'transnet++'])
def test_the_hooks_still_refuse_the_transnets(mt):
    from reviews4rec_amd import catalogue_limits
    from reviews4rec_amd import main as M
    from reviews4rec_amd.recommend import (check_catalogue_metrics_request, check_recommend_request, hook_limits,
                                           narre_catalogue_limits, relu_catalogue_limits)
    hp = dict(model_type=mt, latent_size=6)
    for limits in (catalogue_limits, hook_limits):
        assert 'no catalogue form' in limits(hp)
    assert 'no ReLU-sum form' in relu_catalogue_limits(hp) and 'no product-MLP form' in narre_catalogue_limits(hp)
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_recommend_request(dict(hp, recommend_k=3, recommend_path='lists.npz'))
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_catalogue_metrics_request(dict(hp, catalogue_metrics_k=[1, 5]))
    with pytest.raises(RuntimeError, match='no catalogue form'):
        M.main(dict(hp, recommend_k=3, recommend_path='lists.npz', data_dir='/nonexistent/'))


# ---------------------------------------------------------------- the C ABI without a device
def _args(**kw):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=80, c_bias=p, W=p, b=p, s=p, l=p, H=64, P=16, M=80,
             excl_off=None, excl_ids=None, K=10, chunk=100, ws=p, ws_bytes=1 << 40, out_ids=p, out_scores=p,
             q_idx=p, c_idx=p, n=5, out=p, out_rank=p, out_score=p)
    a.update(kw)
    head = [a[k] for k in ('q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'W', 'b', 's', 'l', 'H', 'P', 'M')]
    return a, head, buf


def _topk(lib, **kw):
    """r4r_topk_rfm with well-formed defaults (host addresses: every refusal precedes the first dereference)."""
    a, head, buf = _args(**kw)
    rc = lib.r4r_topk_rfm(*head, a['excl_off'], a['excl_ids'], a['K'], a['chunk'], a['ws'], a['ws_bytes'], a['out_ids'],
                          a['out_scores'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _pair(lib, **kw):
    a, head, buf = _args(**kw)
    rc = lib.r4r_pair_rfm(*head, a['q_idx'], a['c_idx'], a['n'], a['out'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _rank(lib, **kw):
    a, head, buf = _args(**kw)
    rc = lib.r4r_rank_rfm(*head, a['q_idx'], a['c_idx'], a['n'], a['excl_off'], a['excl_ids'], a['chunk'], a['out_rank'],
                          a['out_score'], None)
    return rc, lib.r4r_last_error() or b'', buf


def test_symbols_are_declared_and_exported(lib):
    from reviews4rec_amd import _lib
    names = _lib.declared_symbols()
    for name in ('r4r_topk_rfm_ws_bytes', 'r4r_topk_rfm', 'r4r_pair_rfm', 'r4r_rank_rfm'):
        assert name in names and hasattr(lib, name)
    decl = _lib.parse_header()
    assert decl['r4r_topk_rfm'][2] == ['q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'W', 'b', 's', 'l', 'H', 'P',
                                       'M', 'excl_off', 'excl_ids', 'K', 'chunk', 'ws', 'ws_bytes', 'out_ids', 'out_scores',
                                       'stream']
    assert decl['r4r_pair_rfm'][2][7:14] == decl['r4r_rank_rfm'][2][7:14] == ['W', 'b', 's', 'l', 'H', 'P', 'M']
    assert decl['r4r_topk_rfm_ws_bytes'][0] is ctypes.c_size_t


@pytest.mark.parametrize('kw, word', [
    (dict(H=65, c_stride=100), b'H = 65'), (dict(H=-1), b'H = -1'), (dict(P=17, c_stride=100), b'P = 17'),
    (dict(P=-1), b'P = -1'), (dict(M=81), b'M = 81'), (dict(M=-1), b'M = -1'),
    (dict(W=None), b'null W'), (dict(s=None), b'null W, s or l'), (dict(l=None), b'null W, s or l'),
    (dict(c_stride=79), b'c_stride'), (dict(q=None), b'null'), (dict(c=None), b'null'),
])
def test_head_refusals_need_no_gpu(lib, kw, word):
    for call in (_topk, _pair, _rank):
        rc, msg, buf = call(lib, **kw)
        assert rc == -1 and word in msg, (call.__name__, rc, msg)
        assert buf.raw == b'\0' * 64


@pytest.mark.parametrize('kw, word', [
    (dict(K=0), b'K'), (dict(K=129), b'K'), (dict(out_ids=None), b'output'), (dict(out_scores=None), b'output'),
    (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'), (dict(chunk=-1), b'chunk'), (dict(chunk=(1 << 30) + 1), b'chunk'),
])
def test_topk_refusals_need_no_gpu(lib, kw, word):
    if kw.get('excl_off') == 1 or kw.get('excl_ids') == 1:
        keep = ctypes.create_string_buffer(16)
        kw = {k: ctypes.addressof(keep) for k in kw}
    rc, msg, _ = _topk(lib, **kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_short_workspace_is_minus_three(lib):
    need = lib.r4r_topk_rfm_ws_bytes(33, 4099, 10, 100)
    assert need == 33 * 41 * 10 * 12                          # 41 partial lists of 10 (score, id) per query
    rc, msg, _ = _topk(lib, ws_bytes=need - 1)
    assert rc == -3 and b'workspace' in msg
    rc, msg, _ = _topk(lib, ws=None, ws_bytes=need)
    assert rc == -3 and b'workspace' in msg


def test_zero_work_is_ok_and_enqueues_nothing(lib):
    for kw in (dict(n_q=0), dict(n_c=0), dict(n_q=0, n_c=0), dict(n_q=0, out_ids=None, out_scores=None),
               dict(n_c=0, W=None, s=None, l=None)):
        rc, msg, buf = _topk(lib, **kw)                       # (no GPU here: a launch would have failed)
        assert rc == 0, (kw, msg)
        assert buf.raw == b'\0' * 64
    for call in (_pair, _rank):
        rc, msg, buf = call(lib, n=0)
        assert rc == 0 and buf.raw == b'\0' * 64, (call.__name__, msg)
    rc, msg, buf = _rank(lib, n_c=0)
    assert rc == 0 and buf.raw == b'\0' * 64, msg
    ws = lib.r4r_topk_rfm_ws_bytes
    assert ws(0, 100, 10, 0) == 0 and ws(5, 0, 10, 0) == 0 and ws(5, 100, 0, 0) == 0 and ws(5, 100, 129, 0) == 0
    assert ws(5, 100, 10, 0) == 0                              # a single chunk needs none
