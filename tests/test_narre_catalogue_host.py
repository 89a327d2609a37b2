"""NARRE's catalogue, the parts that need no GPU: the refusals of r4r_topk_hmlp / r4r_pair_hmlp / r4r_rank_hmlp
(include/r4r.h, "Catalogue recommendation: product-MLP heads") with host addresses, recommend.narre_catalogue_limits, the
fold -- NARRE's held-out score assembled from per-user and per-item vectors against the oracle's forward over every pair
of tests/golden/tiny in float64 -- and main's hooks, which still refuse NARRE."""
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


def _defaults():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.addressof(buf)


HEAD = ('q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'W', 'b', 'w', 'D', 'H')


def _head(p):
    return dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, c_bias=p, W=p, b=p, w=p, D=6, H=5)


def _topk(lib, **kw):
    """r4r_topk_hmlp with well-formed defaults (host addresses: every refusal precedes the first dereference)."""
    buf, p = _defaults()
    a = dict(_head(p), excl_off=None, excl_ids=None, K=10, chunk=100, ws=p, ws_bytes=1 << 40, out_ids=p, out_scores=p)
    a.update(kw)
    rc = lib.r4r_topk_hmlp(*[a[k] for k in HEAD], a['excl_off'], a['excl_ids'], a['K'], a['chunk'], a['ws'], a['ws_bytes'],
                           a['out_ids'], a['out_scores'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _pair(lib, **kw):
    buf, p = _defaults()
    a = dict(_head(p), q_idx=p, c_idx=p, n=7, out=p)
    a.update(kw)
    rc = lib.r4r_pair_hmlp(*[a[k] for k in HEAD], a['q_idx'], a['c_idx'], a['n'], a['out'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _rank(lib, **kw):
    buf, p = _defaults()
    a = dict(_head(p), q_idx=p, t_idx=p, n_p=7, excl_off=None, excl_ids=None, chunk=100, out_rank=p, out_score=p)
    a.update(kw)
    rc = lib.r4r_rank_hmlp(*[a[k] for k in HEAD], a['q_idx'], a['t_idx'], a['n_p'], a['excl_off'], a['excl_ids'], a['chunk'],
                           a['out_rank'], a['out_score'], None)
    return rc, lib.r4r_last_error() or b'', buf


def _with_addresses(kw):
    """A value of 1 stands for 'some valid host address'."""
    keep = ctypes.create_string_buffer(16)
    return {k: (ctypes.addressof(keep) if v == 1 and k.startswith('excl') else v) for k, v in kw.items()}, keep


def test_symbols_are_declared_and_exported(lib):
    from reviews4rec_amd import _lib
    names = _lib.declared_symbols()
    for name in ('r4r_topk_hmlp_ws_bytes', 'r4r_topk_hmlp', 'r4r_pair_hmlp', 'r4r_rank_hmlp'):
        assert name in names and hasattr(lib, name)
    decl = _lib.parse_header()
    head = list(HEAD)
    assert decl['r4r_topk_hmlp'][2] == head + ['excl_off', 'excl_ids', 'K', 'chunk', 'ws', 'ws_bytes', 'out_ids',
                                               'out_scores', 'stream']
    assert decl['r4r_pair_hmlp'][2] == head + ['q_idx', 'c_idx', 'n', 'out', 'stream']
    assert decl['r4r_rank_hmlp'][2] == head + ['q_idx', 't_idx', 'n_p', 'excl_off', 'excl_ids', 'chunk', 'out_rank',
                                               'out_score', 'stream']
    assert decl['r4r_topk_hmlp_ws_bytes'][0] is ctypes.c_size_t
    assert decl['r4r_topk_hmlp_ws_bytes'][2] == ['n_q', 'n_c', 'K', 'chunk']


@pytest.mark.parametrize('kw, word', [
    (dict(K=0), b'K'), (dict(K=129), b'K'), (dict(D=-1), b'D'), (dict(D=65, c_stride=300), b'D'),
    (dict(H=-1), b'H'), (dict(H=65), b'H'), (dict(n_q=-1), b'negative'), (dict(n_c=-1), b'negative'),
    (dict(chunk=-1), b'chunk'), (dict(chunk=(1 << 30) + 1), b'chunk'),
    (dict(out_ids=None), b'output'), (dict(out_scores=None), b'output'), (dict(c_stride=5), b'c_stride'),
    (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'), (dict(w=None), b'null w or W'), (dict(W=None), b'null w or W'),
    (dict(q=None), b'null q or c'), (dict(c=None), b'null q or c'), (dict(c=None, H=0), b'null q or c'),
])
def test_topk_refusals_need_no_gpu(lib, kw, word):
    kw, _keep = _with_addresses(kw)
    rc, msg, buf = _topk(lib, **kw)
    assert rc == -1 and word in msg and b'topk_hmlp' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64                              # (no GPU here: a launch would have failed, too)


@pytest.mark.parametrize('kw, word', [
    (dict(D=-1), b'D'), (dict(D=65, c_stride=300), b'D'), (dict(H=-1), b'H'), (dict(H=65), b'H'),
    (dict(n=-1), b'negative'), (dict(n_q=0), b'empty'), (dict(n_c=0), b'empty'), (dict(c_stride=5), b'c_stride'),
    (dict(w=None), b'null w or W'), (dict(W=None), b'null w or W'), (dict(q_idx=None), b'null pointer'),
    (dict(c_idx=None), b'null pointer'), (dict(out=None), b'null pointer'), (dict(q=None), b'null pointer'),
    (dict(c=None, H=0), b'null pointer'),
])
def test_pair_refusals_need_no_gpu(lib, kw, word):
    rc, msg, buf = _pair(lib, **kw)
    assert rc == -1 and word in msg and b'pair_hmlp' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64


@pytest.mark.parametrize('kw, word', [
    (dict(D=-1), b'D'), (dict(D=65, c_stride=300), b'D'), (dict(H=-1), b'H'), (dict(H=65), b'H'),
    (dict(n_p=-1), b'negative'), (dict(n_c=-1), b'negative'), (dict(chunk=-1), b'chunk'),
    (dict(chunk=(1 << 30) + 1), b'chunk'), (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'),
    (dict(c_stride=5), b'c_stride'), (dict(out_rank=None), b'output'), (dict(out_score=None), b'output'),
    (dict(n_q=0), b'empty'), (dict(w=None), b'null w or W'), (dict(W=None), b'null w or W'),
    (dict(q_idx=None), b'null pointer'), (dict(t_idx=None), b'null pointer'), (dict(q=None), b'null pointer'),
    (dict(c=None, H=0), b'null pointer'),
])
def test_rank_refusals_need_no_gpu(lib, kw, word):
    kw, _keep = _with_addresses(kw)
    rc, msg, buf = _rank(lib, **kw)
    assert rc == -1 and word in msg and b'rank_hmlp' in msg, (rc, msg)
    assert buf.raw == b'\0' * 64


def test_short_workspace_is_minus_three(lib):
    need = lib.r4r_topk_hmlp_ws_bytes(33, 4099, 10, 100)
    assert need == 33 * 41 * 10 * 12                         # 41 partial lists of 10 (score, id) per query
    for kw in (dict(ws_bytes=need - 1), dict(ws=None, ws_bytes=need)):
        rc, msg, buf = _topk(lib, **kw)
        assert rc == -3 and b'workspace' in msg and buf.raw == b'\0' * 64


def test_zero_work_is_ok_and_enqueues_nothing(lib):
    for kw in (dict(n_q=0), dict(n_c=0), dict(n_q=0, n_c=0), dict(n_q=0, out_ids=None, out_scores=None),
               dict(n_c=0, q=None, c=None, w=None, W=None, b=None)):
        rc, msg, buf = _topk(lib, **kw)                      # (no GPU here: a launch would have failed)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    for kw in (dict(n=0), dict(n=0, n_q=0, n_c=0, out=None)):
        rc, msg, buf = _pair(lib, **kw)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    for kw in (dict(n_p=0), dict(n_c=0), dict(n_p=0, out_rank=None, out_score=None)):
        rc, msg, buf = _rank(lib, **kw)
        assert rc == 0 and buf.raw == b'\0' * 64, (kw, msg)
    ws = lib.r4r_topk_hmlp_ws_bytes
    assert ws(0, 100, 10, 0) == 0 and ws(5, 0, 10, 0) == 0                 # empty inputs
    assert ws(5, 100, 10, 0) == 0 and ws(5, 100, 10, 100) == 0 and ws(5, 100, 10, 1 << 30) == 0      # a single chunk
    assert ws(5, 101, 10, 100) == 5 * 2 * 10 * 12


def test_narre_catalogue_limits():
    import reviews4rec_amd
    from reviews4rec_amd import narre_catalogue_limits
    assert reviews4rec_amd.NarreCatalogue is reviews4rec_amd.recommend.NarreCatalogue
    assert issubclass(reviews4rec_amd.NarreCatalogue, reviews4rec_amd.Catalogue)
    for L in (6, 32, 64):
        assert narre_catalogue_limits(dict(model_type='NARRE', latent_size=L, narre_num_reviews=10)) is None
    assert 'latent_size 65 > 64' in narre_catalogue_limits(dict(model_type='NARRE', latent_size=65, narre_num_reviews=10))
    for R in (1, 9, 11):
        why = narre_catalogue_limits(dict(model_type='NARRE', latent_size=8, narre_num_reviews=R))
        assert isinstance(why, str) and 'narre_num_reviews %d' % R in why, why
    serves = {'bias_only': 'Catalogue', 'MF_dot': 'Catalogue', 'deepconn': 'Catalogue', 'deepconn++': 'ReluCatalogue',
              'NeuMF': 'ReluCatalogue', 'MF': None, 'transnet': None, 'transnet++': None}
    for mt, cls in serves.items():
        why = narre_catalogue_limits(dict(model_type=mt, latent_size=8, narre_num_reviews=10))
        assert isinstance(why, str) and repr(mt) in why, (mt, why)
        if cls is None:
            assert 'Catalogue' not in why and 'no product-MLP form' in why, why
        else:
            assert (cls + ' serves it') in why and ('ReluCatalogue' in why) == (cls == 'ReluCatalogue'), why


def test_narre_catalogue_refuses_other_models_and_the_hooks_still_refuse_narre():
    import reviews4rec_amd
    from reviews4rec_amd.recommend import (_REFUSED, catalogue_limits, check_catalogue_metrics_request, check_recommend_request,
                                           hook_limits, relu_catalogue_limits)
    for mt in ('MF', 'deepconn', 'deepconn++', 'NeuMF', 'transnet'):
        with pytest.raises(RuntimeError, match='reviews4rec_amd.recommend'):
            reviews4rec_amd.NarreCatalogue(None, dict(model_type=mt, latent_size=8), None)
    with pytest.raises(RuntimeError, match='latent_size 65 > 64'):
        reviews4rec_amd.NarreCatalogue(None, dict(model_type='NARRE', latent_size=65, narre_num_reviews=10), None)
    hp = dict(model_type='NARRE', latent_size=8, narre_num_reviews=10, recommend_k=3, recommend_path='lists.npz',
              catalogue_metrics_k=[1, 5])
    for fn in (catalogue_limits, relu_catalogue_limits, hook_limits):
        assert isinstance(fn(hp), str)
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_recommend_request(hp)
    with pytest.raises(RuntimeError, match='no catalogue form'):
        check_catalogue_metrics_request(hp)
    # the reason given is the true one: the head, not the attention
    why = _REFUSED['NARRE']
    assert 'ReLU' in why and 'product' in why and 'NARRE.py' in why and 'Catalogue' not in why and len(why) > 40
    assert 'no per-item vector' not in why and len(set(_REFUSED.values())) == len(_REFUSED) - 1     # (the TransNets share one)


def test_the_held_out_score_factors_into_one_vector_per_user_and_one_per_item(tmp_path):
    """The fold, in float64 with the trained weights of tests/golden/tiny/NARRE_e2e.npz: oracle.models.narre_forward over
    all 48 x 24 pairs, on batches built the way ratings outside the training split are (data.py:240-246: nothing
    removed), against the same score assembled from 48 per-user and 24 per-item vectors.  Algebra, not rounding: the
    two run the same float64 operations on the same rows, so 1e-12 is generous (measured: 0.0)."""
    import oracle.models as OM
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp('NARRE', root), device='cpu')
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in _weights(_fixture('NARRE', 'e2e')[1], 'best/').items()}
    U, I = hp['total_users'], hp['total_items']
    assert (U, I) == (48, 24)
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    none = np.full(len(u), -1, np.int64)
    fields = [torch.from_numpy(np.ascontiguousarray(f)) for f in test._review_fields_host(u, i, none, none, none)]
    with torch.no_grad():
        want = OM.narre_forward(P, fields + [torch.from_numpy(u), torch.from_numpy(i)]).view(U, I)

        def attended(side, ids):
            none = np.full(len(ids), -1, np.int64)
            if side == 'user':
                _, _, what, docs, _ = test._review_fields_host(ids, np.zeros_like(ids), none, none, none)
                nb, own, other = what, 'user_embedding.weight', 'item_embedding.weight'
            else:
                _, who, _, _, docs = test._review_fields_host(np.zeros_like(ids), ids, none, none, none)
                nb, own, other = who, 'item_embedding.weight', 'user_embedding.weight'
            docs, nb = torch.from_numpy(np.ascontiguousarray(docs)), torch.from_numpy(np.ascontiguousarray(nb))
            n, R, W = docs.shape
            z = OM.textcnn_forward(P, side + '_conv', P['word2vec.weight'][docs.reshape(n * R, W)]).view(n, R, -1)
            att = OM._narre_attention(P, 'attention_scorer_' + side, z, P[other][nb], 0.0, False, None)
            return att + P[own][torch.from_numpy(ids)]

        au, ai = attended('user', np.arange(U, dtype=np.int64)), attended('item', np.arange(I, dtype=np.int64))
        assert au.shape == (U, hp['latent_size']) and ai.shape == (I, hp['latent_size'])
        x = au[:, None, :] * ai[None, :, :]                                                   # [U, I, L]
        y = x @ P['final.1.weight'].T + P['final.1.bias']
        got = torch.relu(y) @ P['final.3.weight'][0] + P['final.3.bias'][0]
        got = got + P['user_bias'][:U, None] + P['item_bias'][None, :I] + P['global_bias']
    active = float((y > 0).double().mean())
    print('max |factorised - oracle| = %.3g, active ReLUs: %.2f' % (float((got - want).abs().max()), active))
    assert 0.1 < active < 0.9                                 # the ReLU matters on this fixture
    assert float((got - want).abs().max()) <= 1e-12
