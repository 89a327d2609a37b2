"""MF's catalogue, the parts that need no GPU: the algebra of recommend.fold_mf_head against the oracle's MF forward in
float64, recommend.mf_catalogue_limits and the class's refusals, and the C ABI's refusals (r4r_topk_pfm / r4r_pair_pfm /
r4r_rank_pfm, include/r4r.h "Catalogue recommendation: product-FM heads")."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import Golden

EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


# ---------------------------------------------------------------- the fold
def folded_scores(q, qb, c, cb, head, H, split=False):
    """The product-FM form in float64 -> (scores [n_q, n_c], Mag [n_q, n_c]: the sum of the terms' magnitudes).
    split: Mag with |q| + |c| in place of |relu(q + c)| (what bounds the rounding of the TABLES, which the sum may
    cancel)."""
    W, b, s, g, e = (np.asarray(t, np.float64) for t in head)
    q, qb, c, cb = (np.asarray(t, np.float64) for t in (q, qb, c, cb))
    x = np.concatenate([np.maximum(q[:, None, :H] + c[None, :, :H], 0.0), q[:, None, H:] * c[None, :, H:]], -1)
    X = np.abs(x)
    if split:
        X = np.concatenate([np.abs(q)[:, None, :H] + np.abs(c)[None, :, :H], X[..., H:]], -1)
    y = x @ W.T + b
    Y = X @ np.abs(W).T + np.abs(b)
    score = (s * y * y).sum(-1) + (x * (g * x + e)).sum(-1) + cb[None, :] + qb[:, None]
    mag = (np.abs(s) * Y * Y).sum(-1) + (np.abs(g) * X * X + np.abs(e) * X).sum(-1) + np.abs(cb)[None, :] + np.abs(qb)[:, None]
    return score, mag


def golden_mf():
    """-> (hp, weights in float64, U, I, the oracle's eval-mode scores [U, I] over ALL rows of the two tables)."""
    import oracle.models
    g = Golden('mf_full')
    P64 = {k: v.double() for k, v in g.params().items()}
    U, I = P64['user_bias'].numel(), P64['item_bias'].numel()
    u, i = torch.arange(U).repeat_interleave(I), torch.arange(I).repeat(U)
    with torch.no_grad():
        want = oracle.models.mf_forward(P64, [None] * 5 + [u, i], 'MF').numpy().reshape(U, I)
    return g.hp, P64, U, I, want


def test_the_fold_is_the_eval_mode_score():
    """Algebra, not rounding: the folded form in float64 == the oracle's MF forward in float64 over all 31 x 21 id pairs,
    to 1e-12 relative to the sum of the terms' magnitudes."""
    from reviews4rec_amd import fold_mf_head
    hp, P64, U, I, want = golden_mf()
    L = hp['latent_size']
    assert (U, I, L) == (31, 21, 6)
    ue, ie = P64['user_embedding.weight'], P64['item_embedding.weight']
    q, qb, head = fold_mf_head(P64, hp, 'user', ue, bias=P64['user_bias'], dtype=torch.float64)
    c, cb = fold_mf_head(P64, hp, 'item', ie, bias=P64['item_bias'], dtype=torch.float64)
    assert q.shape == (U, 2 * L) and c.shape == (I, 2 * L) and qb.shape == (U,) and cb.shape == (I,)
    assert [tuple(t.shape) for t in head] == [(2 * L, 2 * L)] + [(2 * L,)] * 4
    W, b, s, g, e = head
    assert s.tolist() == [0.5] * L + [-0.5] * L
    assert (W[L:, L:] == 0).all() and (g[:L] == 0).all() and (g[L:] <= 0).all()
    assert torch.equal(q[:, L:], ue) and torch.equal(c[:, L:], ie) and torch.equal(cb, P64['item_bias'])
    got, mag = folded_scores(q.numpy(), qb.numpy(), c.numpy(), cb.numpy(), [t.numpy() for t in head], L)
    worst = float((np.abs(got - want) / mag).max())
    print('fold against the oracle in float64, worst |difference| / Mag = %.3g' % worst)
    assert worst < 1e-12
    assert float(np.abs(want).max()) > 0.1                     # (not a comparison of zeros)
    # the default is one rounding of the same numbers to fp32; head=False skips the head; bias=None counts as zeros
    q32, qb32, head32 = fold_mf_head(P64, hp, 'user', ue, bias=P64['user_bias'])
    assert q32.dtype == qb32.dtype == head32[0].dtype == torch.float32
    assert torch.equal(q32, q.float()) and torch.equal(qb32, qb.float())
    assert all(torch.equal(a, b_.float()) for a, b_ in zip(head32, head))
    lean = fold_mf_head(P64, hp, 'user', ue, bias=P64['user_bias'], head=False)
    assert lean[2] is None and torch.equal(lean[0], q32) and torch.equal(lean[1], qb32)
    bare = fold_mf_head(P64, hp, 'item', ie, dtype=torch.float64)
    assert torch.equal(bare[0], c) and (bare[1] == 0).all()
    # the head does not depend on the rows: the fold of zero rows yields it
    none = fold_mf_head(P64, hp, 'user', torch.zeros(0, L))
    assert none[0].shape == (0, 2 * L) and all(torch.equal(a, b_) for a, b_ in zip(none[2], head32))
    with pytest.raises(ValueError):
        fold_mf_head(P64, hp, 'both', ue)
    with pytest.raises(ValueError):
        fold_mf_head(P64, dict(hp, model_type='MF_dot'), 'user', ue)
    with pytest.raises(ValueError):
        fold_mf_head(P64, hp, 'user', ue[:, :5])
    with pytest.raises(ValueError):
        fold_mf_head(P64, hp, 'user', ue, bias=P64['item_bias'])


def test_the_rounded_tables_stay_within_eight_roundings():
    """The fp32-rounded tables, evaluated in float64, against the float64 oracle: within 8 x 2^-24 of Mag, with |q| + |c|
    for the magnitude of a ReLU'd column (the sum may cancel what was rounded).  Every table entry carries one relative
    rounding of at most 2^-24.  To first order: x_m carries 1 (a ReLU'd sum, relative to |q| + |c|) or 2 (a product); a
    term W_jm x_m 3 at most and b_j 1, so y_j carries 3 relative to Y_j and s_j y_j^2 6 (s = +-1/2 is exact); g_m x_m^2
    carries 1 + 2 * 2 = 5, e_m x_m 3, each bias 1.  6 at most, 8 with room for the second order."""
    from reviews4rec_amd import fold_mf_head
    hp, P64, U, I, want = golden_mf()
    L = hp['latent_size']
    q, qb, head = fold_mf_head(P64, hp, 'user', P64['user_embedding.weight'], bias=P64['user_bias'])
    c, cb = fold_mf_head(P64, hp, 'item', P64['item_embedding.weight'], bias=P64['item_bias'])
    got, mag = folded_scores(q.numpy(), qb.numpy(), c.numpy(), cb.numpy(), [t.numpy() for t in head], L, split=True)
    worst = float((np.abs(got - want) / (EPS * mag)).max())
    print('fp32 tables in float64 against the oracle, worst |difference| / (2^-24 Mag) = %.3f' % worst)
    assert 0 < worst <= 8


# ---------------------------------------------------------------- limits, refusals, export
def test_mf_catalogue_limits_and_export():
    import reviews4rec_amd
    from reviews4rec_amd import mf_catalogue_limits
    assert reviews4rec_amd.MFCatalogue is reviews4rec_amd.recommend.MFCatalogue
    assert reviews4rec_amd.fold_mf_head is reviews4rec_amd.recommend.fold_mf_head
    assert reviews4rec_amd.MFCatalogue._form == 'pfm'
    assert issubclass(reviews4rec_amd.MFCatalogue, reviews4rec_amd.Catalogue)
    for name in ('recommend', 'score_pairs', 'rank'):         # Catalogue's own calls, unchanged
        assert getattr(reviews4rec_amd.MFCatalogue, name) is getattr(reviews4rec_amd.Catalogue, name)
    assert mf_catalogue_limits(dict(model_type='MF')) is None
    assert mf_catalogue_limits(dict(model_type='MF', latent_size=64)) is None
    assert 'latent_size 65 > 64' in mf_catalogue_limits(dict(model_type='MF', latent_size=65))
    serves = {'bias_only': 'Catalogue', 'MF_dot': 'Catalogue', 'deepconn': 'Catalogue', 'deepconn++': 'ReluCatalogue',
              'NeuMF': 'ReluCatalogue', 'NARRE': 'NarreCatalogue', 'transnet': 'TransNetCatalogue',
              'transnet++': 'TransNetCatalogue'}
    for mt, cls in serves.items():
        why = mf_catalogue_limits(dict(model_type=mt, latent_size=8))
        assert repr(mt) in why and (cls + ' serves it') in why, (mt, why)
    why = mf_catalogue_limits(dict(model_type='svd', latent_size=8))
    assert repr('svd') in why and 'no product-FM form' in why
    with pytest.raises(RuntimeError, match='TransNetCatalogue serves it'):
        reviews4rec_amd.MFCatalogue(None, dict(model_type='transnet'), None)
    with pytest.raises(RuntimeError, match='latent_size 65 > 64'):
        reviews4rec_amd.MFCatalogue(None, dict(model_type='MF', latent_size=65), None)
    model = reviews4rec_amd.get_model_class('MF')(dict(model_type='MF', latent_size=4, total_users=3, total_items=3,
                                                       dropout=0.0))
    with pytest.raises(RuntimeError, match='ROCm device'):     # no CPU fallback
        reviews4rec_amd.MFCatalogue(model, dict(model_type='MF', latent_size=4, total_users=3, total_items=3), None)


def test_the_hooks_and_the_older_texts_still_refuse_mf():
    from reviews4rec_amd import catalogue_limits, transnet_catalogue_limits
    from reviews4rec_amd.recommend import check_catalogue_metrics_request, check_recommend_request, hook_limits
    hp = dict(model_type='MF', latent_size=6)
    for limits in (catalogue_limits, hook_limits):
        assert 'no catalogue form' in limits(hp)
    assert 'no class serves it' in transnet_catalogue_limits(hp)
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_recommend_request(dict(hp, recommend_k=3, recommend_path='lists.npz'))
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_catalogue_metrics_request(dict(hp, catalogue_metrics_k=[1, 5]))


# ---------------------------------------------------------------- the C ABI without a device
HEAD = ('q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'W', 'b', 's', 'g', 'e', 'H', 'G', 'M')


def _args(**kw):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=128, c_bias=p, W=p, b=p, s=p, g=p, e=p, H=64, G=64, M=128,
             excl_off=None, excl_ids=None, K=10, chunk=100, ws=p, ws_bytes=1 << 40, out_ids=p, out_scores=p,
             q_idx=p, c_idx=p, n=5, out=p, out_rank=p, out_score=p)
    a.update(kw)
    return a, [a[k] for k in HEAD], buf


def _topk(lib, **kw):
    """r4r_topk_pfm with well-formed defaults (host addresses: every refusal precedes the first dereference)."""
    a, head, buf = _args(**kw)
    rc = lib.r4r_topk_pfm(*head, a['excl_off'], a['excl_ids'], a['K'], a['chunk'], a['ws'], a['ws_bytes'], a['out_ids'],
                          a['out_scores'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _pair(lib, **kw):
    a, head, buf = _args(**kw)
    rc = lib.r4r_pair_pfm(*head, a['q_idx'], a['c_idx'], a['n'], a['out'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _rank(lib, **kw):
    a, head, buf = _args(**kw)
    rc = lib.r4r_rank_pfm(*head, a['q_idx'], a['c_idx'], a['n'], a['excl_off'], a['excl_ids'], a['chunk'], a['out_rank'],
                          a['out_score'], None)
    return rc, lib.r4r_last_error() or b'', buf


def test_symbols_are_declared_and_exported(lib):
    from reviews4rec_amd import _lib
    names = _lib.declared_symbols()
    for name in ('r4r_topk_pfm_ws_bytes', 'r4r_topk_pfm', 'r4r_pair_pfm', 'r4r_rank_pfm'):
        assert name in names and hasattr(lib, name)
    decl = _lib.parse_header()
    assert decl['r4r_topk_pfm'][2] == list(HEAD) + ['excl_off', 'excl_ids', 'K', 'chunk', 'ws', 'ws_bytes', 'out_ids',
                                                   'out_scores', 'stream']
    assert decl['r4r_pair_pfm'][2] == list(HEAD) + ['q_idx', 'c_idx', 'n', 'out', 'stream']
    assert decl['r4r_rank_pfm'][2] == list(HEAD) + ['q_idx', 't_idx', 'n_p', 'excl_off', 'excl_ids', 'chunk', 'out_rank',
                                                   'out_score', 'stream']
    # r4r_topk_rfm's list with (W, b, s, g, e, H, G, M) in place of (W, b, s, l, H, P, M)
    rfm = decl['r4r_topk_rfm'][2]
    assert decl['r4r_topk_pfm'][2][:7] == rfm[:7] and decl['r4r_topk_pfm'][2][15:] == rfm[14:]
    assert decl['r4r_topk_pfm_ws_bytes'][0] is ctypes.c_size_t


@pytest.mark.parametrize('kw, word', [
    (dict(H=65, c_stride=200), b'H = 65'), (dict(H=-1), b'H = -1'), (dict(G=65, c_stride=200), b'G = 65'),
    (dict(G=-1), b'G = -1'), (dict(M=129), b'M = 129'), (dict(M=-1), b'M = -1'),
    (dict(W=None), b'null W'), (dict(s=None), b'null W or s'),
    (dict(c_stride=127), b'c_stride'), (dict(q=None), b'null'), (dict(c=None), b'null'),
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
    need = lib.r4r_topk_pfm_ws_bytes(33, 4099, 10, 100)
    assert need == 33 * 41 * 10 * 12                          # 41 partial lists of 10 (score, id) per query
    rc, msg, _ = _topk(lib, ws_bytes=need - 1)
    assert rc == -3 and b'workspace' in msg
    rc, msg, _ = _topk(lib, ws=None, ws_bytes=need)
    assert rc == -3 and b'workspace' in msg


def test_zero_work_is_ok_and_enqueues_nothing(lib):
    for kw in (dict(n_q=0), dict(n_c=0), dict(n_q=0, n_c=0), dict(n_q=0, out_ids=None, out_scores=None),
               dict(n_c=0, W=None, s=None, g=None, e=None)):
        rc, msg, buf = _topk(lib, **kw)                       # (no GPU here: a launch would have failed)
        assert rc == 0, (kw, msg)
        assert buf.raw == b'\0' * 64
    for call in (_pair, _rank):
        rc, msg, buf = call(lib, n=0)
        assert rc == 0 and buf.raw == b'\0' * 64, (call.__name__, msg)
    rc, msg, buf = _rank(lib, n_c=0)
    assert rc == 0 and buf.raw == b'\0' * 64, msg
    ws = lib.r4r_topk_pfm_ws_bytes
    assert ws(0, 100, 10, 0) == 0 and ws(5, 0, 10, 0) == 0 and ws(5, 100, 0, 0) == 0 and ws(5, 100, 129, 0) == 0
    assert ws(5, 100, 10, 0) == 0                              # a single chunk needs none
