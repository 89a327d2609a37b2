"""``NarreCatalogue.pair_reviews`` / ``explain_pair_reviews`` on tests/golden/tiny (recommend.py; include/r4r.h, "NARRE
pair gradients").

For a 4 x 5 grid of (user, item) pairs that includes the owner without a review on both sides, the per-review weights,
``rev``, the logit gradients and the score must equal float64 autograd through a float64 COPY OF THE MODEL'S OWN modules
(tower.fc, the attention scorers, final, the embedding and bias tables) applied to the float64 cast of
ops.textcnn_fwd_raw's pooled features, within narre_pair_ref's bounds with the fp32 tower fc's roundings carried in --
that holds the class's parameter plumbing, not only the kernels; the attention must be ``explain``'s, bit for bit;
``explain_pair_reviews`` must be ``explain_words`` with the returned weights; and towers='device', ``pair_batch``, the
order of the pairs and a pair alone must not change a bit."""
import copy

import numpy as np
import pytest
import torch

from head_ref import U32, compare, d64
from narre_pair_ref import owner_ref, pair_ref, side_of
from test_gpu_narre_catalogue import _tiny
from test_gpu_narre_explain_catalogue import _with_an_empty_owner
from test_gpu_phrases_catalogue import same

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 3


def _side64(cat, side, ids):
    """-> (pooled float64 [n, R, F] from the kernels' own forward, the side's raw inputs for narre_pair_ref with the
    model's own parameters in float64, the float64 module copies)."""
    from reviews4rec_amd import ops
    from reviews4rec_amd.data import _np_neighbours, _np_reviews
    user, pool, tower, pad = cat._narre_side(side)
    m, hp = cat.model, cat.hp
    R, W = int(hp['narre_num_reviews']), int(hp['narre_num_words'])
    rb, re = pool.first[ids], pool.first[ids + 1]
    none = np.full(len(ids), -1, np.int64)
    docs = _np_reviews(pool.tok, pool.rev_off, rb, re, none, R, W).reshape(len(ids) * R, W)
    nb = torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, pad))
    conv = tower.convs[0]
    with torch.no_grad():
        pooled, _ = ops.textcnn_fwd_raw(torch.from_numpy(docs).to(DEV), cat._words(), conv.weight.detach(), conv.bias.detach())
    cp = lambda mod: copy.deepcopy(mod).double().cpu().eval()
    scorer = cp(m.attention_scorer_user if user else m.attention_scorer_item)
    own, other = (m.user_embedding, m.item_embedding) if user else (m.item_embedding, m.user_embedding)
    mods = dict(fc=cp(tower.fc), scorer=scorer, own=cp(own), other=cp(other))
    raw = dict(nb=nb, other_table=mods['other'].weight.detach(), own_table=mods['own'].weight.detach(),
               owner=torch.from_numpy(ids), W0=scorer[0].weight.detach(), b0=scorer[0].bias.detach(),
               w3=scorer[3].weight.detach().reshape(-1), b3=scorer[3].bias.detach(), fc=mods['fc'].weight.detach())
    return d64(pooled).reshape(len(ids), R, -1), raw, mods


def _attended64(pooled, raw, mods):
    """NARRE.py:103-119 through the module copies: pooled [n, R, F] -> (p [n, L], z [n, R, L], logits [n, R])."""
    z = mods['fc'](pooled)
    logits = mods['scorer'](torch.cat([z, mods['other'](raw['nb'])], dim=-1))[:, :, 0]
    a = torch.softmax(logits, dim=-1)
    return torch.sum(a.unsqueeze(-1) * z, dim=1) + mods['own'](raw['owner']), z, logits


def test_pair_reviews_and_explain_pair_reviews_on_tiny(tmp_path, monkeypatch):
    from reviews4rec_amd import NarreCatalogue, PairPhrases, PairReviews
    hp, train, test, model, W = _tiny(tmp_path)
    monkeypatch.setattr(train.store, 'items', _with_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_an_empty_owner(train.store.users))
    host = NarreCatalogue(model, hp, train)
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=7)
    assert host.pair_batch == 8192
    R, L = int(hp['narre_num_reviews']), int(hp['latent_size'])
    pu, pi = host._narre_side('user')[1], host._narre_side('item')[1]
    us = np.array([0, 3, 7, pu.owners - 1], dtype=np.int64)
    its = np.array([1, 2, 5, 11, pi.owners - 1], dtype=np.int64)
    users, items = np.repeat(us, len(its)), np.tile(its, len(us))
    n = len(users)
    pr = host.pair_reviews(users, items)
    assert isinstance(pr, PairReviews)
    F = pr.w_user.shape[2]
    assert F == 100
    for name in PairReviews._fields:
        t = getattr(pr, name)
        shape = (n, R, F) if name[:2] == 'w_' else (n,) if name in ('scores', 'live_user', 'live_item') else (n, R)
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == (torch.int64 if name[:4] == 'live' else torch.float32), name

    # ---- float64 autograd through the model's own modules
    pool_u, raw_u, mods_u = _side64(host, 'user', us)
    pool_i, raw_i, mods_i = _side64(host, 'item', its)
    pool_u.requires_grad_()
    pool_i.requires_grad_()
    p_u, z_u, lg_u = _attended64(pool_u, raw_u, mods_u)
    p_i, z_i, lg_i = _attended64(pool_i, raw_i, mods_i)
    final = copy.deepcopy(model.final).double().cpu().eval()
    u_row, i_row = torch.from_numpy(np.searchsorted(us, users)), torch.from_numpy(np.searchsorted(its, items))
    qb = d64(model.user_bias)[us] + d64(model.global_bias).reshape(()) + d64(final[3].bias).reshape(())
    cb = d64(model.item_bias)[its]
    # (final[3].bias is inside qb: the head below stops at final.3's weight)
    s64 = (torch.relu(final[1](p_u[u_row] * p_i[i_row])) @ final[3].weight.reshape(-1)) + qb[u_row] + cb[i_row]
    auto = {k: torch.zeros((n, R, F), dtype=torch.float64) for k in ('w_user', 'w_item')}
    auto.update({k: torch.zeros((n, R), dtype=torch.float64) for k in ('rev_user', 'rev_item', 'glogit_user', 'glogit_item')})
    for p in range(n):
        gu, gi, gzu, gzi, glu, gli = torch.autograd.grad(s64[p], [pool_u, pool_i, z_u, z_i, lg_u, lg_i], retain_graph=True)
        a, b = int(u_row[p]), int(i_row[p])
        auto['w_user'][p], auto['w_item'][p] = gu[a], gi[b]
        auto['rev_user'][p], auto['rev_item'][p] = (gzu[a] * z_u[a].detach()).sum(-1), (gzi[b] * z_i[b].detach()).sum(-1)
        auto['glogit_user'][p], auto['glogit_item'][p] = glu[a], gli[b]
    # the bounds: narre_pair_ref at the float64 latents, which the kernels' fp32 latents (ops.linear: an F-term dot and
    # the bias, c = F + 1) approach to within dx; the closed forms are autograd's values
    sides = []
    for pooled, raw, mods, z in ((pool_u, raw_u, mods_u, z_u), (pool_i, raw_i, mods_i, z_i)):
        fc = mods['fc']
        dx = (F + 1) * U32 * (pooled.detach().abs() @ fc.weight.detach().abs().T + fc.bias.detach().abs())
        sides.append(side_of(owner_ref(dict(raw, z=z.detach()), dx=dx), raw))
    ref = pair_ref(sides[0], sides[1], u_row, i_row, final[1].weight.detach(), final[1].bias.detach(),
                   final[3].weight.detach().reshape(-1), qb.detach(), cb.detach())
    worst = {}
    for name, want in auto.items():
        val, bound = ref[name]
        assert float((val - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
        worst[name] = compare('NARRE ' + name, getattr(pr, name), want, bound)
    # the class sums the score's scalars in float64 and rounds them once: one more rounding of |q_bias|
    assert float((ref['score'][0] - s64.detach()).abs().max()) <= 1e-12 * float(s64.detach().abs().max())
    score_bound = ref['score'][1] + U32 * qb.detach()[u_row].abs()
    worst['scores'] = compare('NARRE scores', pr.scores, s64.detach(), score_bound)
    print('NARRE pair_reviews: worst error / bound %s' % ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert float(pr.w_user.abs().max()) > 0 and float(pr.w_item.abs().max()) > 0
    assert float(pr.glogit_user.sum(1).abs().max()) <= float(ref['glogit_user'][1].sum(1).max())

    # ---- the same prediction as score_pairs', by another fp32 chain (test_gpu_pair_explain_catalogue's rule): eligible
    # items of real users only, the others are -inf
    real = (users < hp['total_users']) & (items < hp['total_items'])
    pairs = host.score_pairs(users[real], items[real]).cpu().double()
    held = torch.isfinite(pairs)
    assert int(held.sum()) >= 6
    sc = pr.scores.cpu().double()[torch.from_numpy(real)]
    tol = score_bound[torch.from_numpy(real)] + 1e-5 + 1e-5 * s64.detach().abs()[torch.from_numpy(real)]
    assert bool(((sc - pairs).abs()[held] <= tol[held]).all())

    # ---- the attention and the live counts are explain's, bit for bit
    for side, ids, attn, live in (('user', users, pr.attention_user, pr.live_user), ('item', items, pr.attention_item, pr.live_item)):
        e = host.explain(ids, k=K, side=side)
        assert torch.equal(attn.view(torch.int32), e.attention.view(torch.int32)) and torch.equal(live, e.live), side
    assert int(pr.live_user.min()) == 0 and int(pr.live_item.min()) == 0            # the owners without a review

    # ---- explain_pair_reviews is explain_words with those weights, bit for bit, in both directions
    for direction, sign in (('up', 1.0), ('down', -1.0)):
        e = host.explain_pair_reviews(users, items, k=K, direction=direction)
        assert isinstance(e, PairPhrases) and torch.equal(e.scores.view(torch.int32), pr.scores.view(torch.int32))
        same(e.user, host.explain_words(users, k=K, side='user', weights=sign * pr.w_user), (direction, 'user'))
        same(e.item, host.explain_words(items, k=K, side='item', weights=sign * pr.w_item), (direction, 'item'))
        assert tuple(e.user.positions.shape) == (n, R, K) and tuple(e.item.tokens.shape) == (n, R, K, 3)
        # reviews=2: the two live slots with the largest +-rev, ties by ascending slot
        c = host.explain_pair_reviews(users, items, k=K, reviews=2, direction=direction)
        for cut, whole, rev, live in ((c.user, e.user, pr.rev_user, pr.live_user), (c.item, e.item, pr.rev_item, pr.live_item)):
            rev_h, live_h = rev.cpu().numpy(), live.cpu().numpy()
            slots = np.full((n, 2), -1, np.int64)
            for p in range(n):
                order = sorted(range(int(live_h[p])), key=lambda r: (-sign * float(rev_h[p, r]), r))[:2]
                slots[p, :len(order)] = order
            assert np.array_equal(cut.slots.cpu().numpy(), slots)
            s = torch.from_numpy(slots).to(DEV)
            take, none = s.clamp(min=0), s < 0
            assert torch.equal(cut.weights.view(torch.int32), rev.gather(1, take).masked_fill(none, 0).view(torch.int32))
            assert tuple(cut.positions.shape) == (n, 2, K)
            want_pos = whole.positions.gather(1, take[:, :, None].expand(n, 2, K)).masked_fill(none[:, :, None], -1)
            want_sc = whole.scores.gather(1, take[:, :, None].expand(n, 2, K)).masked_fill(none[:, :, None], 0)
            assert torch.equal(cut.positions, want_pos) and torch.equal(cut.scores.view(torch.int32), want_sc.view(torch.int32))
            assert bool((cut.windows[none] == 0).all()) and bool((cut.reviews[none] == -1).all())
    # the lists depend on the pair: one user's weights differ from item to item
    assert not torch.equal(pr.w_user[0], pr.w_user[1])

    # ---- towers='device', another chunking, pair_batch: the same bits; permuted pairs, one pair alone, no pair
    def equal(a, b, sel=None):
        for name in PairReviews._fields:
            x, y = getattr(a, name), getattr(b, name)
            y = y if sel is None else y[sel]
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), name
    equal(dev.pair_reviews(users, items), pr)
    up = host.explain_pair_reviews(users, items, k=K, reviews=2)
    de = dev.explain_pair_reviews(users, items, k=K, reviews=2)
    same(de.user, up.user, 'device user')
    same(de.item, up.item, 'device item')
    for batch in (1, 3):
        for cat in (host, dev):
            cat.pair_batch = batch                              # an attribute, set after construction
            equal(cat.pair_reviews(users, items), pr)
    host.pair_batch = dev.pair_batch = 8192
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    for cat in (host, dev):
        equal(cat.pair_reviews(torch.from_numpy(users)[perm].to(DEV), torch.from_numpy(items)[perm].to(DEV)), pr, perm.to(DEV))
        equal(cat.pair_reviews(users[7:8], items[7:8]), pr, slice(7, 8))
        none = cat.pair_reviews([], [])
        assert tuple(none.w_user.shape) == (0, R, F) and tuple(none.scores.shape) == (0,)
        assert tuple(cat.explain_pair_reviews([], [], k=K).user.positions.shape) == (0, R, K)

    # ---- argument errors, before anything is enqueued
    with pytest.raises(ValueError, match='direction'):
        host.explain_pair_reviews(users, items, direction='sideways')
    for k in (0, 101, True, 2.0):
        with pytest.raises(ValueError, match='explain_pair_reviews k'):
            host.explain_pair_reviews(users, items, k=k)
    for r in (0, 11, True, 2.0):
        with pytest.raises(ValueError, match='explain_pair_reviews reviews'):
            host.explain_pair_reviews(users, items, k=K, reviews=r)
    with pytest.raises(ValueError, match='2 users against 3 items'):
        host.pair_reviews([0, 1], [0, 1, 2])
    with pytest.raises(KeyError):
        host.pair_reviews([0], [10 ** 6])
    with pytest.raises(KeyError):
        host.explain_pair_reviews([-1], [0])

    # ---- the per-owner calls keep refusing, with the old text
    for call in (lambda: host.pair_weights([0], [0]), lambda: host.explain_pair([0], [0], k=3)):
        with pytest.raises(RuntimeError, match='softmax .*a gradient through it is not built'):
            call()
