"""``what_if`` / ``leave_one_out`` / ``deletion_curve`` of the single-document catalogue classes on tests/golden/tiny
(recommend.py; include/r4r.h, "What-if documents"): deepconn, deepconn++ and transnet++ (the source network), at
input_length = 37, so that a removal slides later words in across the cut.

For a grid of pairs that includes the owner without a review and the owner with the most reviews on both sides, every
leave-one-out score must equal float64 copies of the model's own head modules over the float64 cast of
ops.textcnn_fwd_raw's pooled features of the HOST-built ``_np_docs(skip)`` documents -- the documents the loader gives a
training rating -- within pair_grad_ref's score bound widened by the fc's (F + 1) 2^-24, as
test_gpu_pair_explain_catalogue.py does; the three methods must agree with one another bit for bit, with hand-written
documents through the per-call ops, across towers='device' / 'host', pair_batch and the order of the pairs."""
import os

import numpy as np
import pytest
import torch

from head_ref import U32, compare, d64
from helpers import materialise_tiny, tiny_hp
from pair_grad_ref import pair_grad_ref
from phrases_ref import bits
from test_gpu_pair_explain_catalogue import KIND, _float64_model
from test_gpu_phrases_catalogue import _catalogues

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 3


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture
def direct_conv():
    """The conv request pinned for the test (bits are promised per algorithm; the automatic rule reads a round's row
    count, which differs between the passes compared here), restored afterwards."""
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    prev = lib.r4r_textcnn_algo(0)
    try:
        lib.r4r_textcnn_algo(1)
        yield
    finally:
        lib.r4r_textcnn_algo(prev)


def _grid(cat):
    """(users, items): a few owners of each side, the one with the most reviews and the one without any, every pair."""
    pu, pi = cat._phrase_side('user')[0], cat._phrase_side('item')[0]
    most = lambda p: int(np.diff(p.first).argmax())
    us = np.array(sorted({0, 3, most(pu), pu.owners - 1}), dtype=np.int64)
    its = np.array(sorted({1, 2, 5, most(pi), pi.owners - 1}), dtype=np.int64)
    assert pu.first[-1] == pu.first[-2] and pi.first[-1] == pi.first[-2]          # the last owners have no review
    return np.repeat(us, len(its)), np.tile(its, len(us))


def _side64(cat, side, ids):
    """The float64 latents of the side's documents with nothing removed and with each of the first 64 reviews removed,
    from HOST documents (``_np_docs`` with the loader's skip) -> (z64 [rows, L], pooled64, fc64, row owners [rows],
    {(owner, skip): row}); skip -1 is the whole document."""
    import copy
    from reviews4rec_amd import ops
    from reviews4rec_amd.data import _np_docs
    pool, tower, _ = cat._phrase_side(side)
    T = int(cat.hp['input_length'])
    keys = [(int(o), s) for o in sorted(set(ids.tolist())) for s in range(-1, min(int(pool.first[o + 1] - pool.first[o]), 64))]
    own, skip = np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)
    docs = _np_docs(pool.tok, pool.rev_off, pool.first[own], pool.first[own + 1], skip, T)
    conv = tower.convs[0]
    with torch.no_grad():
        pooled, _ = ops.textcnn_fwd_raw(torch.from_numpy(docs).to(DEV), cat._words(), conv.weight.detach(), conv.bias.detach())
    fc = copy.deepcopy(tower.fc).double().cpu()
    p64 = d64(pooled)
    with torch.no_grad():
        z = fc(p64)
    return z, p64, fc, own, {k: r for r, k in enumerate(keys)}, docs


def _hand_scores(cat, docs_u, docs_i, users, items):
    """The pairs' scores from hand-written documents [n, T] through the per-call ops and the class's own head."""
    from reviews4rec_amd import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    with torch.no_grad():
        zu = cat._tower(cat._phrase_side('user')[1], dev(docs_u))
        zi = cat._tower(cat._phrase_side('item')[1], dev(docs_i))
        idx = torch.arange(len(users), device=DEV)
        return ops.pair_grad(cat._pair_kind, zu, zi, idx, idx, want=('score',), **cat._pair_head(dev(users), dev(items)))['score']


def _whole(cat, side, ids):
    from reviews4rec_amd.data import _np_docs
    pool = cat._phrase_side(side)[0]
    return _np_docs(pool.tok, pool.rev_off, pool.first[ids], pool.first[ids + 1], np.full(len(ids), -1, np.int64),
                    int(cat.hp['input_length']))


@pytest.mark.parametrize('mt', ['deepconn', 'deepconn++', 'transnet++'])
def test_what_if_leave_one_out_and_deletion_curve_on_tiny(mt, tmp_path, monkeypatch, direct_conv):
    from reviews4rec_amd import DocDeletionCurve, DocLeaveOneOut, WhatIf
    host, dev, hp = _catalogues(mt, tmp_path, monkeypatch)
    T = int(hp['input_length'])
    assert T == 37
    users, items = _grid(host)
    n = len(users)
    pools = {s: host._phrase_side(s)[0] for s in ('user', 'item')}
    count = {'user': np.diff(pools['user'].first)[users], 'item': np.diff(pools['item'].first)[items]}

    # ---- leave_one_out against float64 over the loader's own documents
    loo = host.leave_one_out(users, items)
    assert isinstance(loo, DocLeaveOneOut)
    S_u, S_i = int(min(count['user'].max(), 64)), int(min(count['item'].max(), 64))
    assert tuple(loo.without_user.shape) == (n, S_u) and tuple(loo.without_item.shape) == (n, S_i) and S_u > 1 and S_i > 1
    for t in loo:
        assert t.is_cuda and t.shape[0] == n
    assert loo.live_user.tolist() == np.minimum(count['user'], 64).tolist()
    assert loo.live_item.tolist() == np.minimum(count['item'], 64).tolist()
    zu, pu, fc_u, own_u, row_u, _ = _side64(host, 'user', users)
    zi, pi, fc_i, own_i, row_i, _ = _side64(host, 'item', items)
    _, raw, qb, cb = _float64_model(host, mt, own_u, own_i)
    pairs = [(p, -1, -1) for p in range(n)]
    pairs += [(p, s, -1) for p in range(n) for s in range(int(loo.live_user[p]))]
    pairs += [(p, -1, s) for p in range(n) for s in range(int(loo.live_item[p]))]
    u_idx = torch.tensor([row_u[(int(users[p]), su)] for p, su, _ in pairs])
    i_idx = torch.tensor([row_i[(int(items[p]), si)] for p, _, si in pairs])
    F = pu.shape[1]
    dz = lambda p, fc: (F + 1) * U32 * (p.abs() @ fc.weight.detach().abs().T + fc.bias.detach().abs())
    ref = pair_grad_ref(KIND[mt], zu, zi, u_idx, i_idx, {k: v.detach() for k, v in raw.items()}, fc_u.weight.detach(),
                        fc_i.weight.detach(), qb.detach(), None if cb is None else cb.detach(), dzu=dz(pu, fc_u),
                        dzi=dz(pi, fc_i))
    val, bound = ref['score'][0], ref['score'][1] + U32 * qb.detach()[u_idx].abs()
    got = torch.stack([loo.base[p] if su < 0 and si < 0 else (loo.without_user[p, su] if su >= 0 else loo.without_item[p, si])
                       for p, su, si in pairs])
    worst = compare(mt + ' leave_one_out', got, val, bound)
    # ``pair_weights``' scores: the same float64 numbers by the same rule
    compare(mt + ' pair_weights', host.pair_weights(users, items)[2], val[:n], bound[:n])
    print('%s: leave_one_out worst error / bound %.3f over %d scores' % (mt, worst, len(pairs)))
    assert float((val[n:] - val[torch.tensor([p for p, _, _ in pairs[n:]])]).abs().max()) > 1e-4        # removals move scores
    # slots without a review, and reviews that cannot show in the document: the base's bits, a delta of exactly 0
    for wo, delta, live, reach, side, S in ((loo.without_user, loo.delta_user, loo.live_user, loo.reach_user, 'user', S_u),
                                            (loo.without_item, loo.delta_item, loo.live_item, loo.reach_item, 'item', S_i)):
        pool, ids = pools[side], users if side == 'user' else items
        start = [[int(pool.rev_off[pool.first[o] + s] - pool.rev_off[pool.first[o]]) for s in range(int(count[side][p]))]
                 for p, o in enumerate(ids)]
        assert reach.tolist() == [sum(1 for a in row if a < T) for row in start]
        slot = torch.arange(S, device=DEV)[None, :]
        idle = (slot >= live[:, None]) | (slot >= reach[:, None])
        assert bool(idle.any()) and same_bits(wo[idle], loo.base[:, None].expand(n, S)[idle])
        assert bool((delta[idle] == 0).all()) and same_bits(delta, loo.base[:, None] - wo)
        assert bool((reach < live).any())                    # T = 37 cuts the longest owners' lists short

    # ---- what_if: lists and masks; a single drop is leave_one_out's column
    lists = {s: [[[0] if c else [], list(range(min(int(c), 3)))] for c in count[s]] for s in ('user', 'item')}
    masks = {s: torch.tensor([[sum(1 << b for b in v) for v in row] for row in lists[s]], dtype=torch.int64) for s in lists}
    a = host.what_if(users, items, drop_user=lists['user'], drop_item=lists['item'])
    b = host.what_if(users, items, drop_user=masks['user'], drop_item=masks['item'].to(DEV))
    assert isinstance(a, WhatIf) and tuple(a.scores.shape) == (n, 2) and same_bits(a.scores, b.scores)
    assert same_bits(a.base, loo.base) and same_bits(b.base, loo.base)
    for s in (0, 1):
        one = host.what_if(users, items, drop_user=[[s] if c > s else [] for c in count['user']])
        assert same_bits(one.scores[:, 0], loo.without_user[:, s]) if s < S_u else True
        one = host.what_if(users, items, drop_item=torch.full((n, 1), 1 << s, dtype=torch.int64))     # (bits past a list: ignored)
        assert same_bits(one.scores[:, 0], loo.without_item[:, s])
    # both sides at once, against hand-written documents through the per-call ops
    from reviews4rec_amd.data import _np_docs
    skip0 = lambda side, ids: _np_docs(pools[side].tok, pools[side].rev_off, pools[side].first[ids], pools[side].first[ids + 1],
                                       np.zeros(len(ids), np.int64), T)
    hand = _hand_scores(host, skip0('user', users), skip0('item', items), users, items)
    both = host.what_if(users, items, drop_user=[[0] if c else [] for c in count['user']],
                        drop_item=[[0] if c else [] for c in count['item']])
    assert same_bits(both.scores[:, 0], hand)
    # occlusion, alone and on top of a removal: positions are the variant's own
    occ = [0, 5, 5, T - 1, 17]
    docs_u = skip0('user', users)
    docs_u[:, occ] = 0
    docs_i = _whole(host, 'item', items)
    docs_i[:, [3]] = 0
    got = host.what_if(users, items, drop_user=[[0] if c else [] for c in count['user']], occlude_user=[occ] * n,
                       occlude_item=torch.tensor([[[3, -1]]] * n))
    assert same_bits(got.scores[:, 0], _hand_scores(host, docs_u, docs_i, users, items))
    assert not same_bits(got.scores[:, 0], both.scores[:, 0])
    nothing = host.what_if(users, items, occlude_user=[[[], []]] * n, occlude_item=torch.full((n, 2, 3), -1))
    assert tuple(nothing.scores.shape) == (n, 2) and same_bits(nothing.scores, loo.base[:, None].expand(n, 2))

    # ---- deletion_curve: what_if over the occlusion sets written out by hand
    mine = torch.tensor([[4, 0, T + 1]] * n)
    mine[1] = torch.tensor([9, -1, -1])
    curves = {}
    for by, side, direction in (('pair', 'user', 'up'), ('pair', 'item', 'down'), ('mass', 'item', 'up'), (mine, 'user', 'up')):
        dc = host.deletion_curve(users, items, k=K, by=by, side=side, direction=direction)
        curves[(by if isinstance(by, str) else 'mine', side, direction)] = dc
        assert isinstance(dc, DocDeletionCurve) and tuple(dc.scores.shape) == (n, K + 1) and dc.positions.dtype == torch.int32
        pos = dc.positions.cpu().numpy()
        if isinstance(by, str) and by == 'pair':
            e = host.explain_pair(users, items, k=K, direction=direction)
            assert torch.equal(dc.positions, getattr(e, side).positions)
        elif isinstance(by, str):
            assert torch.equal(dc.positions, host.explain_words(users if side == 'user' else items, k=K, side=side).positions)
        else:
            assert np.array_equal(pos, mine.numpy())
        live = (pos >= 0).sum(1)
        assert dc.live.tolist() == live.tolist()
        sets = np.full((n, K, 3 * K), -1, np.int64)
        for p in range(n):
            words = []
            for j in range(K):
                if pos[p, j] >= 0:
                    words += [w for w in range(pos[p, j] - 2, pos[p, j] + 1) if 0 <= w < T]
                sets[p, j, :len(words)] = words
        wi = host.what_if(users, items, **{'occlude_' + side: torch.from_numpy(sets)})
        assert same_bits(dc.scores[:, 0], loo.base) and same_bits(dc.scores[:, 1:], wi.scores), (by, side)
        sc = dc.scores.cpu().double().numpy()
        for p in range(n):
            assert (bits(sc[p, live[p]:].astype(np.float32)) == bits(sc[p, live[p]].astype(np.float32))).all()
        aopc = np.array([np.mean(sc[p, 0] - sc[p, 1:live[p] + 1]) if live[p] else 0.0 for p in range(n)]).astype(np.float32)
        assert np.array_equal(bits(dc.aopc.cpu().numpy()), bits(aopc))
    assert curves[('mine', 'user', 'up')].live.tolist()[:2] == [3, 1]
    up = curves[('pair', 'user', 'up')]
    assert float((up.scores[:, 1:] - up.scores[:, :1]).abs().max()) > 0

    # ---- towers='device', another chunking, pair_batch, the order of the pairs, one pair, none
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    first = {}
    for cat in (host, dev):
        for pair_batch in (8192, 1, 3):
            cat.pair_batch = pair_batch
            l2 = cat.leave_one_out(users, items)
            for name, x, y in zip(loo._fields, loo, l2):
                assert (same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y)), (cat.towers, pair_batch, name)
            w2 = cat.what_if(users, items, drop_user=masks['user'], drop_item=lists['item'], occlude_user=[[occ, [1]]] * n)
            first.setdefault('w', w2)
            assert same_bits(w2.scores, first['w'].scores) and same_bits(w2.base, loo.base)
            d2 = cat.deletion_curve(users, items, k=K, by='pair', side='user')
            for x, y in zip(d2, up):
                assert (same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y)), (cat.towers, pair_batch)
        cat.pair_batch = 8192
        lp = cat.leave_one_out(torch.from_numpy(users)[perm].to(DEV), torch.from_numpy(items)[perm].to(DEV))
        for x, y in zip(lp, loo):
            assert (same_bits(x, y[perm.to(DEV)]) if x.dtype == torch.float32 else torch.equal(x, y[perm.to(DEV)]))
        p = int(np.argmax(count['user']))                    # a pair of the user with the most reviews
        alone = cat.leave_one_out(users[p:p + 1], items[p:p + 1])
        lu, li = int(alone.live_user[0]), int(alone.live_item[0])
        assert tuple(alone.without_user.shape) == (1, lu) and tuple(alone.without_item.shape) == (1, li)
        assert same_bits(alone.without_user, loo.without_user[p:p + 1, :lu]) and same_bits(alone.base, loo.base[p:p + 1])
        assert same_bits(alone.without_item, loo.without_item[p:p + 1, :li])
        none = cat.leave_one_out([], [])
        assert tuple(none.base.shape) == (0,) and tuple(none.without_user.shape) == (0, 0)
        assert tuple(cat.what_if([], [], drop_user=torch.zeros((0, 4), dtype=torch.int64)).scores.shape) == (0, 4)
        assert tuple(cat.deletion_curve([], [], k=K).scores.shape) == (0, K + 1)
        last = cat._phrase_side('user')[0].owners - 1           # two owners without a review: nothing to remove at all
        bare = cat.leave_one_out([last], [cat._phrase_side('item')[0].owners - 1])
        assert tuple(bare.without_user.shape) == (1, 0) and bool(torch.isfinite(bare.base).all())

    # ---- refusals, before anything is enqueued
    with pytest.raises(ValueError, match='2 users against 3 items'):
        host.what_if([0, 1], [0, 1, 2])
    with pytest.raises(KeyError):
        host.leave_one_out([0], [10 ** 6])
    with pytest.raises(KeyError):
        host.deletion_curve([-1], [0])
    with pytest.raises(ValueError, match='drop_user'):
        host.what_if(users, items, drop_user=[[int(c)] for c in count['user']])      # one past each owner's list
    with pytest.raises(ValueError, match='drop_item'):
        host.what_if(users, items, drop_item=[[64]] * n)
    with pytest.raises(ValueError, match='occlude_user'):
        host.what_if(users, items, occlude_user=[[T]] * n)
    with pytest.raises(ValueError, match='variants per pair'):
        host.what_if(users, items, drop_user=masks['user'], occlude_item=[[0]] * n)
    for kw in (dict(by='rev'), dict(side='both'), dict(direction='sideways'), dict(k=0), dict(k=101), dict(by=mine, k=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            host.deletion_curve(users, items, **kw)


def test_classes_without_a_tower_refuse_and_narre_keeps_its_own(tmp_path, monkeypatch):
    from reviews4rec_amd import Catalogue, DeletionCurve, LeaveOneOut, NarreCatalogue
    from test_gpu_narre_catalogue import _tiny as narre_tiny
    from test_gpu_recommend import _tiny_model
    hp, train, _, model, _ = _tiny_model('MF_dot', tmp_path)
    cat = Catalogue(model, hp, train)
    for call in (cat.what_if, cat.leave_one_out, cat.deletion_curve):
        with pytest.raises(RuntimeError, match="'MF_dot' has no TextCNN tower"):
            call([0], [0])
    for name in ('what_if', 'leave_one_out', 'deletion_curve', '_what_if'):
        assert getattr(NarreCatalogue, name) is not getattr(Catalogue, name), name
    hp, train, _, model, _ = narre_tiny(tmp_path)
    narre = NarreCatalogue(model, hp, train)
    U, I = int(hp['total_users']), int(hp['total_items'])
    users, items = np.repeat(np.arange(4), 3), np.tile(np.array([1, 2, 5]), 4)

    def tensors(x):
        if torch.is_tensor(x):
            return [x.clone()]
        return [t for part in x for t in tensors(part)] if isinstance(x, (tuple, list)) else []

    def answers():
        loo = narre.leave_one_out(users, items)
        dc = narre.deletion_curve(users, items)
        assert isinstance(loo, LeaveOneOut) and isinstance(dc, DeletionCurve)
        return tensors([loo, dc, narre.what_if(users, items, drop_user=[[0]] * len(users)),
                        narre.explain_pair_reviews(users, items, k=2), narre.score_pairs(users % U, items % I)])

    before = answers()
    (tmp_path / 'd').mkdir()
    _, dev, _ = _catalogues('deepconn', tmp_path / 'd', monkeypatch)       # the new passes run in between
    dev.leave_one_out([0, 3], [1, 2])
    dev.deletion_curve([0, 3], [1, 2], k=2)
    after = answers()
    assert len(before) == len(after) > 10
    for x, y in zip(before, after):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y)
    with pytest.raises(RuntimeError, match='softmax .*a gradient through it is not built'):
        narre.explain_pair([0], [0], k=3)


# ---------------------------------------------------------------- main.main
@pytest.mark.parametrize('mt', ['deepconn'])
def test_main_writes_the_reviews_behind_the_pairs_it_recommends(mt, tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from reviews4rec_amd.recommend import recommended_pairs
    from test_tiny_eval import _fixture, _weights
    meta, z = _fixture(mt, 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    hp = tiny_hp(mt, root, epochs=1, log_file=str(tmp_path / 'log'), model_path=str(tmp_path / 'model'),
                 recommend_k=3, recommend_path=str(tmp_path / 'lists.npz'), explain_reviews_k=2,
                 explain_reviews_path=str(tmp_path / 'reviews.npz'))
    M.main(hp)
    assert {'lists.npz', 'reviews.npz'} <= set(os.listdir(str(tmp_path)))
    state = torch.load(hp['model_path'], map_location='cpu')
    train, _, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(state)
    cat = Catalogue(model.cuda().eval(), hp, train)
    f, lists = np.load(str(tmp_path / 'reviews.npz')), np.load(str(tmp_path / 'lists.npz'))
    assert set(f.files) == {'users', 'items', 'side', 'pair_scores', 'reviews', 'deltas'}
    users, items = recommended_pairs(cat, 3)
    n = len(users)
    assert n > 3 and np.array_equal(items, lists['items'][lists['items'] >= 0])          # the pairs ARE the written lists
    assert np.array_equal(f['users'], np.tile(users, 2)) and np.array_equal(f['items'], np.tile(items, 2))
    assert np.array_equal(f['side'], np.repeat(np.array([0, 1], np.int8), n))
    loo = cat.leave_one_out(users, items)
    assert np.array_equal(bits(f['pair_scores']), bits(np.tile(loo.base.cpu().numpy(), 2)))
    assert f['reviews'].shape == (2 * n, 2) and f['reviews'].dtype == np.int64 and f['deltas'].dtype == np.float32
    for half, delta, live in ((0, loo.delta_user, loo.live_user), (1, loo.delta_item, loo.live_item)):
        delta, live = delta.cpu().numpy(), live.cpu().numpy()
        for p in range(n):
            order = sorted(range(int(live[p])), key=lambda s: (-float(delta[p, s]), s))[:2]
            want_r = order + [-1] * (2 - len(order))
            want_d = np.array([delta[p, s] for s in order] + [0.0] * (2 - len(order)), np.float32)
            assert f['reviews'][half * n + p].tolist() == want_r, (half, p)
            assert np.array_equal(bits(f['deltas'][half * n + p]), bits(want_d)), (half, p)
    assert (f['reviews'][:, 0] >= 0).all() and float(np.abs(f['deltas']).max()) > 0
