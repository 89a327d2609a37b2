"""ReLU-sum catalogue, the parts that need no GPU: the refusals of r4r_topk_relu / r4r_pair_relu / r4r_rank_relu
(include/r4r.h) with host addresses, recommend.relu_catalogue_limits, the algebra of recommend.fold_relu_head against the
oracle's forward in float64, and main's hooks."""
import ctypes

import pytest
import torch

from helpers import Golden


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def _defaults():
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    return buf, p


def _topk(lib, **kw):
    """r4r_topk_relu with well-formed defaults (host addresses: every refusal precedes the first dereference)."""
    buf, p = _defaults()
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, c_bias=p, w=p, H=5, P=3, excl_off=None, excl_ids=None,
             K=10, chunk=100, ws=p, ws_bytes=1 << 40, out_ids=p, out_scores=p)
    a.update(kw)
    rc = lib.r4r_topk_relu(a['q'], a['n_q'], a['q_bias'], a['c'], a['n_c'], a['c_stride'], a['c_bias'], a['w'], a['H'],
                           a['P'], a['excl_off'], a['excl_ids'], a['K'], a['chunk'], a['ws'], a['ws_bytes'],
                           a['out_ids'], a['out_scores'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _pair(lib, **kw):
    buf, p = _defaults()
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, c_bias=p, w=p, H=5, P=3, q_idx=p, c_idx=p, n=7, out=p)
    a.update(kw)
    rc = lib.r4r_pair_relu(a['q'], a['n_q'], a['q_bias'], a['c'], a['n_c'], a['c_stride'], a['c_bias'], a['w'], a['H'],
                           a['P'], a['q_idx'], a['c_idx'], a['n'], a['out'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _rank(lib, **kw):
    buf, p = _defaults()
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, c_bias=p, w=p, H=5, P=3, q_idx=p, t_idx=p, n_p=7,
             excl_off=None, excl_ids=None, chunk=100, out_rank=p, out_score=p)
    a.update(kw)
    rc = lib.r4r_rank_relu(a['q'], a['n_q'], a['q_bias'], a['c'], a['n_c'], a['c_stride'], a['c_bias'], a['w'], a['H'],
                           a['P'], a['q_idx'], a['t_idx'], a['n_p'], a['excl_off'], a['excl_ids'], a['chunk'],
                           a['out_rank'], a['out_score'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _with_addresses(kw):
    """A value of 1 stands for 'some valid host address'."""
    keep = ctypes.create_string_buffer(16)
    return {k: (ctypes.addressof(keep) if v == 1 and k.startswith('excl') else v) for k, v in kw.items()}, keep


def test_symbols_are_declared_and_exported(lib):
    from reviews4rec_amd import _lib
    names = _lib.declared_symbols()
    for name in ('r4r_topk_relu_ws_bytes', 'r4r_topk_relu', 'r4r_pair_relu', 'r4r_rank_relu'):
        assert name in names and hasattr(lib, name)
    decl = _lib.parse_header()
    assert decl['r4r_topk_relu'][2] == ['q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'w', 'H', 'P', 'excl_off',
                                        'excl_ids', 'K', 'chunk', 'ws', 'ws_bytes', 'out_ids', 'out_scores', 'stream']
    assert decl['r4r_pair_relu'][2] == ['q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'w', 'H', 'P', 'q_idx',
                                        'c_idx', 'n', 'out', 'stream']
    assert decl['r4r_rank_relu'][2] == ['q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'w', 'H', 'P', 'q_idx',
                                        't_idx', 'n_p', 'excl_off', 'excl_ids', 'chunk', 'out_rank', 'out_score', 'stream']
    assert decl['r4r_topk_relu_ws_bytes'][0] is ctypes.c_size_t


@pytest.mark.parametrize('kw, word', [
    (dict(K=0), b'K'), (dict(K=129), b'K'), (dict(H=-1), b'H'), (dict(H=129, c_stride=300), b'H'),
    (dict(P=-1), b'P'), (dict(P=129, c_stride=300), b'P'), (dict(n_q=-1), b'negative'), (dict(n_c=-1), b'negative'),
    (dict(chunk=-1), b'chunk'), (dict(chunk=(1 << 30) + 1), b'chunk'),
    (dict(out_ids=None), b'output'), (dict(out_scores=None), b'output'), (dict(c_stride=7), b'c_stride'),
    (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'), (dict(w=None), b'null w'),
    (dict(q=None), b'null q or c'), (dict(c=None), b'null q or c'), (dict(c=None, H=0), b'null q or c'),
])
def test_topk_refusals_need_no_gpu(lib, kw, word):
    kw, _keep = _with_addresses(kw)
    rc, msg, buf = _topk(lib, **kw)
    assert rc == -1 and word in msg and b'topk_relu' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64                              # (no GPU here: a launch would have failed, too)


@pytest.mark.parametrize('kw, word', [
    (dict(H=-1), b'H'), (dict(H=129, c_stride=300), b'H'), (dict(P=-1), b'P'), (dict(P=129, c_stride=300), b'P'),
    (dict(n=-1), b'negative'), (dict(n_q=0), b'empty'), (dict(n_c=0), b'empty'), (dict(c_stride=7), b'c_stride'),
    (dict(w=None), b'null w'), (dict(q_idx=None), b'null pointer'), (dict(c_idx=None), b'null pointer'),
    (dict(out=None), b'null pointer'), (dict(q=None), b'null pointer'), (dict(c=None, H=0), b'null pointer'),
])
def test_pair_refusals_need_no_gpu(lib, kw, word):
    rc, msg, buf = _pair(lib, **kw)
    assert rc == -1 and word in msg and b'pair_relu' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64


@pytest.mark.parametrize('kw, word', [
    (dict(H=-1), b'H'), (dict(H=129, c_stride=300), b'H'), (dict(P=-1), b'P'), (dict(P=129, c_stride=300), b'P'),
    (dict(n_p=-1), b'negative'), (dict(n_c=-1), b'negative'), (dict(chunk=-1), b'chunk'),
    (dict(chunk=(1 << 30) + 1), b'chunk'), (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'),
    (dict(c_stride=7), b'c_stride'), (dict(out_rank=None), b'output'), (dict(out_score=None), b'output'),
    (dict(n_q=0), b'empty'), (dict(w=None), b'null w'), (dict(q_idx=None), b'null pointer'),
    (dict(t_idx=None), b'null pointer'), (dict(q=None), b'null pointer'), (dict(c=None, H=0), b'null pointer'),
])
def test_rank_refusals_need_no_gpu(lib, kw, word):
    kw, _keep = _with_addresses(kw)
    rc, msg, buf = _rank(lib, **kw)
    assert rc == -1 and word in msg and b'rank_relu' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64


def test_short_workspace_is_minus_three(lib):
    need = lib.r4r_topk_relu_ws_bytes(33, 4099, 10, 100)
    assert need == 33 * 41 * 10 * 12                         # 41 partial lists of 10 (score, id) per query
    for kw in (dict(ws_bytes=need - 1), dict(ws=None, ws_bytes=need)):
        rc, msg, buf = _topk(lib, **kw)
        assert rc == -3 and b'workspace' in msg and buf.raw == b'\0' * 64


def test_zero_work_is_ok_and_enqueues_nothing(lib):
    for kw in (dict(n_q=0), dict(n_c=0), dict(n_q=0, n_c=0), dict(n_q=0, out_ids=None, out_scores=None),
               dict(n_c=0, q=None, c=None, w=None)):
        rc, msg, buf = _topk(lib, **kw)                      # (no GPU here: a launch would have failed)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    for kw in (dict(n=0), dict(n=0, n_q=0, n_c=0, out=None)):
        rc, msg, buf = _pair(lib, **kw)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    for kw in (dict(n_p=0), dict(n_c=0), dict(n_p=0, out_rank=None, out_score=None)):
        rc, msg, buf = _rank(lib, **kw)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    ws = lib.r4r_topk_relu_ws_bytes
    assert ws(0, 100, 10, 0) == 0 and ws(5, 0, 10, 0) == 0                 # empty inputs
    assert ws(5, 100, 10, 0) == 0 and ws(5, 100, 10, 100) == 0 and ws(5, 100, 10, 1 << 30) == 0      # a single chunk
    assert ws(5, 101, 10, 100) == 5 * 2 * 10 * 12


def test_relu_catalogue_limits():
    import reviews4rec_amd
    from reviews4rec_amd import catalogue_limits, relu_catalogue_limits
    assert reviews4rec_amd.ReluCatalogue is reviews4rec_amd.recommend.ReluCatalogue
    assert issubclass(reviews4rec_amd.ReluCatalogue, reviews4rec_amd.Catalogue)
    for L in (8, 128):
        assert relu_catalogue_limits(dict(model_type='deepconn++', latent_size=L)) is None
        assert relu_catalogue_limits(dict(model_type='NeuMF', latent_size=L)) is None
        for stage in ('GMF', 'MLP', 'NeuMF'):
            assert relu_catalogue_limits(dict(model_type='NeuMF', neumf_stage=stage, latent_size=L)) is None
    for mt in ('deepconn++', 'NeuMF'):
        assert 'latent_size 129 > 128' in relu_catalogue_limits(dict(model_type=mt, latent_size=129))
    assert 'neumf_stage' in relu_catalogue_limits(dict(model_type='NeuMF', neumf_stage='both', latent_size=8))
    for mt in ('bias_only', 'MF_dot', 'deepconn', 'MF', 'NARRE', 'transnet', 'transnet++'):
        why = relu_catalogue_limits(dict(model_type=mt, latent_size=8))
        assert isinstance(why, str) and repr(mt) in why, (mt, why)
        assert ('Catalogue' in why) == (mt in ('bias_only', 'MF_dot', 'deepconn')), why
    # Catalogue's own limits have not moved
    for mt in ('deepconn++', 'NeuMF'):
        assert 'no catalogue form' in catalogue_limits(dict(model_type=mt, latent_size=8))
        with pytest.raises(RuntimeError, match='no catalogue form'):
            reviews4rec_amd.Catalogue(None, dict(model_type=mt, latent_size=8), None)
    with pytest.raises(RuntimeError, match='no ReLU-sum form'):
        reviews4rec_amd.ReluCatalogue(None, dict(model_type='NARRE'), None)


def _relu_sum(q, qb, w, c, cb, H):
    h = (torch.relu(q[:, None, :H] + c[None, :, :H]) * w).sum(-1)
    return h + q[:, H:] @ c[:, H:].T + cb[None, :] + qb[:, None]


def _relu_scale(q, qb, w, c, cb, H):
    h = ((q[:, None, :H].abs() + c[None, :, :H].abs()) * w.abs()).sum(-1)
    return h + q[:, H:].abs() @ c[:, H:].abs().T + cb.abs()[None, :] + qb.abs()[:, None]


@pytest.mark.parametrize('case', ['deepconnpp_e20', 'neumf_gmf', 'neumf_mlp', 'neumf_full'])
def test_fold_relu_head_is_the_head_over_the_concatenation(case, monkeypatch):
    """Algebra, not rounding: the ReLU-sum of the folded sides (float64 intermediates) == the oracle's forward in
    float64 over random latents (deepconn++) / random table rows (NeuMF), 13 users x 11 items, to 1e-12 relative to
    sum_j |w_j| (|qa_j| + |ca_j|) + sum_j |qp_j cp_j| + |biases| (fold_fm's criterion)."""
    import oracle
    import oracle.models as OM
    from reviews4rec_amd import fold_relu_head
    g = Golden(case)
    hp, L = g.hp, g.hp['latent_size']
    P = {k: v.double() for k, v in g.params().items()}
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    nu, ni = 13, 11
    P['user_bias'], P['item_bias'] = rnd(*P['user_bias'].shape), rnd(*P['item_bias'].shape)
    uu, ii = torch.meshgrid(torch.arange(nu), torch.arange(ni), indexing='ij')
    data = [None] * 5 + [uu.reshape(-1), ii.reshape(-1)]
    ub, ib = P['user_bias'][:nu], P['item_bias'][:ni]
    P32 = {k: v for k, v in P.items()}
    if case == 'deepconnpp_e20':
        zu, zi = rnd(nu, L), rnd(ni, L)
        lat = {'user_conv': zu[uu.reshape(-1)], 'item_conv': zi[ii.reshape(-1)]}
        monkeypatch.setattr(OM, 'textcnn_forward', lambda params, prefix, x, *a, **k: lat[prefix])
        data[3] = data[4] = torch.zeros(nu * ni, 4, dtype=torch.int64)
        user, item = dict(x=zu, bias=ub), dict(x=zi, bias=ib)
        H, Pw = L, 0
    else:
        for k in list(P):
            if k.endswith('embedding.weight'):
                P[k] = rnd(*P[k].shape)
        stage = hp['neumf_stage']
        if stage == 'GMF':
            user = dict(gx=P['user_embedding.weight'][:nu], bias=ub)
            item = dict(gx=P['item_embedding.weight'][:ni], bias=ib)
        elif stage == 'MLP':
            user = dict(x=P['user_embedding.weight'][:nu], bias=ub)
            item = dict(x=P['item_embedding.weight'][:ni], bias=ib)
        else:
            user = dict(x=P['mlp_user_embedding.weight'][:nu], gx=P['gmf_user_embedding.weight'][:nu], bias=ub)
            item = dict(x=P['mlp_item_embedding.weight'][:ni], gx=P['gmf_item_embedding.weight'][:ni], bias=ib)
        H, Pw = {'GMF': (0, L), 'MLP': (L, 0), 'NeuMF': (L, L)}[stage]
    want = oracle.model_forward(P, data, hp).view(nu, ni)
    q, qb, w = fold_relu_head(P, hp, 'user', dtype=torch.float64, **user)
    c, cb = fold_relu_head(P, hp, 'item', dtype=torch.float64, **item)
    assert q.shape == (nu, H + Pw) and c.shape == (ni, H + Pw) and w.shape == (H,) and qb.shape == (nu,) and cb.shape == (ni,)
    got = _relu_sum(q, qb, w, c, cb, H)
    scale = _relu_scale(q, qb, w, c, cb, H)
    assert float(((got - want).abs() / scale).max()) < 1e-12
    # the default is one rounding of the same numbers to fp32
    q32, qb32, w32 = fold_relu_head(P, hp, 'user', **user)
    c32, cb32 = fold_relu_head(P, hp, 'item', **item)
    for a32, a64 in ((q32, q), (qb32, qb), (w32, w), (c32, c), (cb32, cb)):
        assert a32.dtype == torch.float32 and torch.equal(a32, a64.float())
    with pytest.raises(ValueError):
        fold_relu_head(P, hp, 'both', **user)
    with pytest.raises(ValueError):
        fold_relu_head(P, hp, 'user', **dict(user, bias=ub[:-1]))
    wide = {k: (torch.cat([v, v], 1) if k != 'bias' else v) for k, v in user.items()}
    with pytest.raises(ValueError):
        fold_relu_head(P, hp, 'user', **wide)
    with pytest.raises(ValueError):
        fold_relu_head(P, hp, 'user', bias=ub)               # the rows are missing


def test_hooks_accept_deepconnpp_and_still_refuse_the_rest():
    from reviews4rec_amd.recommend import check_catalogue_metrics_request, check_recommend_request
    hp = dict(model_type='deepconn++', latent_size=10, recommend_k=3, recommend_path='lists.npz', catalogue_metrics_k=[1, 5])
    check_recommend_request(hp)
    check_catalogue_metrics_request(hp)
    with pytest.raises(RuntimeError, match='latent_size 129 > 128'):
        check_recommend_request(dict(hp, latent_size=129))
    with pytest.raises(RuntimeError, match='recommend_path'):
        check_recommend_request(dict(model_type='deepconn++', latent_size=10, recommend_k=3))
    with pytest.raises(RuntimeError, match='catalogue_metrics_k'):
        check_catalogue_metrics_request(dict(hp, catalogue_metrics_k=[]))
    for mt in ('NARRE', 'NeuMF', 'MF', 'transnet', 'transnet++'):
        with pytest.raises(RuntimeError, match='no catalogue form'):
            check_recommend_request(dict(hp, model_type=mt))
        with pytest.raises(RuntimeError, match='no catalogue form'):
            check_catalogue_metrics_request(dict(hp, model_type=mt))
