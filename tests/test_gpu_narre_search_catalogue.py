"""``NarreCatalogue.counterfactual`` on tests/golden/tiny (recommend.py; include/r4r.h, "NARRE counterfactual search").

For a grid of (user, item) pairs that includes the owner without a review and the owners with more than R reviews on
both sides, the search must equal, bit for bit, a host loop a caller could have written before: per step one ``what_if``
call over every candidate the rule allows (as lists of review indices), a host arg-best (narre_search_ref's float
compares, ties to the lowest c) and the update of the removed lists.  Budget 1 is the arg-best of ``leave_one_out``; ``k``
is a target written out by hand from ``recommend``; towers='device', ``pair_batch``, the order of the pairs, a pair
alone and no pair must not change a bit; and the calls that were there before answer as before."""
import numpy as np
import pytest
import torch

from narre_search_ref import ITEM, NAN, better, holds
from test_gpu_narre_catalogue import _tiny
from test_gpu_narre_explain_catalogue import _with_an_empty_owner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t


def host_loop(cat, users, items, target, direction, side, budget, slide, cu, ci):
    """The search as a loop of ``what_if`` calls -> (order, scores, steps, crossed, removed_user, removed_item) as numpy."""
    R = int(cat.hp['narre_num_reviews'])
    n, up = len(users), direction == 'up'
    S = min(64, R + budget) if slide else R
    gone_u, gone_i = [[] for _ in range(n)], [[] for _ in range(n)]
    base = cat.what_if(users, items).base.cpu().numpy()
    scores = np.repeat(base[:, None], budget + 1, 1)
    order = np.full((n, budget), -1, np.int64)
    steps, crossed = np.zeros(n, np.int64), np.zeros(n, bool)
    now = [base[p].item() for p in range(n)]
    done = [holds(now[p], float(target[p]), up) for p in range(n)]
    crossed[:] = done
    attended = lambda count, gone: [r for r in range(min(int(count), S)) if r not in gone][:R]
    for t in range(budget):
        cands = {}
        for p in range(n):
            if done[p]:
                continue
            cs = [(r, gone_u[p] + [r], gone_i[p]) for r in attended(cu[users[p]], gone_u[p])] if side != 'item' else []
            cs += [(ITEM + r, gone_u[p], gone_i[p] + [r]) for r in attended(ci[items[p]], gone_i[p])] if side != 'user' else []
            if cs:
                cands[p] = cs
            else:
                done[p] = True
        if not cands:
            break
        V = max(len(cs) for cs in cands.values())
        fill = lambda p, k: (cands[p] + [(None, gone_u[p], gone_i[p])] * V)[:V] if p in cands else [(None, gone_u[p], gone_i[p])] * V
        wi = cat.what_if(users, items, drop_user=[[list(v[1]) for v in fill(p, 0)] for p in range(n)],
                         drop_item=[[list(v[2]) for v in fill(p, 0)] for p in range(n)], slide=slide).scores.cpu().numpy()
        for p, cs in cands.items():
            best = best_k = None
            for k in range(len(cs)):
                if better(wi[p, k].item(), best, up):
                    best, best_k = wi[p, k].item(), k
            c, gone_u[p], gone_i[p] = cs[best_k]
            order[p, t], steps[p], now[p] = c, t + 1, best
            scores[p, t + 1:] = wi[p, best_k]
            if holds(best, float(target[p]), up):
                done[p] = crossed[p] = True
    pad = lambda rows: np.array([row + [-1] * (budget - len(row)) for row in rows], np.int64).reshape(n, budget)
    return order, scores, steps, crossed, pad(gone_u), pad(gone_i)


def check(cf, want, target):
    order, scores, steps, crossed, ru, ri = want
    assert np.array_equal(cf.order.cpu().numpy(), order)
    assert np.array_equal(cf.scores.cpu().numpy().view(np.int32), scores.astype(np.float32).view(np.int32))
    assert np.array_equal(cf.steps.cpu().numpy(), steps) and np.array_equal(cf.crossed.cpu().numpy(), crossed)
    assert np.array_equal(cf.removed_user.cpu().numpy(), ru) and np.array_equal(cf.removed_item.cpu().numpy(), ri)
    assert torch.equal(bits(cf.base), bits(cf.scores[:, 0]))
    assert np.array_equal(cf.target.cpu().numpy().view(np.int32), np.asarray(target, np.float32).view(np.int32))


def test_counterfactual_on_tiny(tmp_path, monkeypatch):
    from reviews4rec_amd import Counterfactual, NarreCatalogue
    hp, train, test, model, W = _tiny(tmp_path)
    monkeypatch.setattr(train.store, 'items', _with_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_an_empty_owner(train.store.users))
    host = NarreCatalogue(model, hp, train)
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=7)
    R = int(hp['narre_num_reviews'])
    pu, pi = host._narre_side('user')[1], host._narre_side('item')[1]
    cu, ci = pu.first[1:] - pu.first[:-1], pi.first[1:] - pi.first[:-1]
    assert int(cu.max()) > R and int(ci.max()) > R and cu[-1] == 0 and ci[-1] == 0
    us = np.unique(np.array([0, 3, int(cu.argmax()), int(cu[:-1].argmin()), pu.owners - 1], dtype=np.int64))
    its = np.unique(np.array([1, 2, int(ci.argmax()), int(ci[:-1].argmin()), pi.owners - 1], dtype=np.int64))
    users, items = np.repeat(us, len(its)), np.tile(its, len(us))
    n = len(users)
    real = (users < hp['total_users']) & (items < hp['total_items'])

    before = (host.what_if(users, items, drop_user=[[0][:int(cu[a])] for a in users]), host.leave_one_out(users, items),
              host.pair_reviews(users, items), host.explain(items, k=3, side='item'))
    pairs_before = host.score_pairs(users[real], items[real])
    loo = before[1]
    base = loo.base.cpu().numpy()

    # ---- the host loop of what_if calls: every side, both directions, slide on and off
    rng = np.random.default_rng(3)
    ran = {}
    for side in ('user', 'item', 'both'):
        for direction in ('down', 'up'):
            for slide in (True, False):
                shift = rng.choice(np.array([0.02, 0.1, 0.4, np.nan], np.float32), n)
                target = (base - shift if direction == 'down' else base + shift).astype(np.float32)
                B = 4 if side == 'both' else 3
                cf = host.counterfactual(users, items, target=torch.from_numpy(target), direction=direction, side=side,
                                         budget=B, slide=slide)
                assert isinstance(cf, Counterfactual) and all(t.is_cuda for t in cf)
                assert cf.order.dtype == torch.int64 and cf.steps.dtype == torch.int64 and cf.crossed.dtype == torch.bool
                assert tuple(cf.removed_user.shape) == (n, B) and tuple(cf.scores.shape) == (n, B + 1)
                check(cf, host_loop(host, users, items, target, direction, side, B, slide, cu, ci), target)
                assert torch.equal(bits(cf.base), bits(loo.base))
                ran[side, direction, slide] = (cf, target, B)
                steps = cf.steps.cpu().numpy()
                assert steps.max() == B and (steps[np.isnan(shift) & (cu[users] + ci[items] == 0)] == 0).all()
                if side == 'user':
                    assert (cf.removed_item == -1).all() and (cf.order < ITEM).all()
                if side == 'item':
                    assert (cf.removed_user == -1).all() and ((cf.order >= ITEM) | (cf.order < 0)).all()
    assert any(bool(c.crossed.any()) and not bool(c.crossed.all()) for c, _, _ in ran.values())
    # the slide-in matters: for owners with more than R reviews the two removals differ
    a, b = ran['both', 'down', True][0], ran['both', 'down', False][0]
    assert not torch.equal(bits(a.scores), bits(b.scores))

    # ---- budget 1 is the arg-best of leave_one_out; the default budget is the side's R (R_u + R_i for 'both')
    nan = torch.full((n,), NAN)
    for direction in ('down', 'up'):
        cf = host.counterfactual(users, items, target=nan, direction=direction, budget=1)
        wu, wi_ = loo.without_user.cpu().numpy(), loo.without_item.cpu().numpy()
        lu, li = loo.live_user.cpu().numpy(), loo.live_item.cpu().numpy()
        for p in range(n):
            cs = [(r, wu[p, r]) for r in range(lu[p])] + [(ITEM + r, wi_[p, r]) for r in range(li[p])]
            best = best_c = None
            for c, s in cs:
                if better(s.item(), best, direction == 'up'):
                    best, best_c = s.item(), c
            if best_c is None:
                assert int(cf.steps[p]) == 0 and int(cf.order[p, 0]) == -1
            else:
                assert int(cf.order[p, 0]) == best_c and float(cf.scores[p, 1]) == best and int(cf.steps[p]) == 1
    for side, B in (('user', R), ('item', R), ('both', min(64, 2 * R))):
        cf = host.counterfactual(users, items, target=nan, side=side)
        assert tuple(cf.order.shape) == (n, B)
        live = (np.minimum(cu[users], R + B) * (side != 'item') + np.minimum(ci[items], R + B) * (side != 'user'))
        assert np.array_equal(cf.steps.cpu().numpy(), np.minimum(live, B))       # every attended review goes, or the budget

    # ---- k: the threshold written out by hand from recommend
    ru, ri_ = users[real], items[real]
    for k in (1, 2, 100):
        rec_items, rec_scores = host.recommend(np.unique(ru), k + 1)
        rec_items, rec_scores = rec_items.cpu().numpy(), rec_scores.cpu().numpy()
        top = {int(u): rec_items[j, 0] for j, u in enumerate(np.unique(ru))}
        it_k = np.array([top[int(u)] if (j % 2 == 0 and top[int(u)] >= 0) else ri_[j] for j, u in enumerate(ru)], np.int64)
        want = np.full(len(ru), -np.inf, np.float32)
        for j, (u, i) in enumerate(zip(ru, it_k)):
            row = int(np.searchsorted(np.unique(ru), u))
            others = [(it, sc) for it, sc in zip(rec_items[row], rec_scores[row]) if it != i]
            if len(others) >= k and others[k - 1][0] >= 0:
                want[j] = others[k - 1][1]
        cf = host.counterfactual(ru, it_k, k=k, side='item')
        assert np.array_equal(cf.target.cpu().numpy().view(np.int32), want.view(np.int32))
        by_hand = host.counterfactual(ru, it_k, target=torch.from_numpy(want), side='item')
        for name in Counterfactual._fields:
            assert torch.equal(bits(getattr(cf, name)), bits(getattr(by_hand, name))), name
        if k == 100:
            assert bool(np.isneginf(want).all()) and not bool(cf.crossed.any())
        else:
            assert np.isfinite(want).any()
    for kw in (dict(side='both'), dict(side='user'), dict(side='item', direction='up')):
        with pytest.raises(ValueError, match='k goes with'):
            host.counterfactual(ru, ri_, k=2, **kw)
    with pytest.raises(KeyError):
        host.counterfactual([0], [10 ** 6], target=1.0)
    with pytest.raises(ValueError, match='2 users against 3 items'):
        host.counterfactual([0, 1], [0, 1, 2], target=1.0)

    # ---- towers='device', pair_batch, permuted pairs, a pair alone, no pair: the same bits
    def equal(a, b, sel=None):
        for name in a._fields:
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(bits(x), bits(y if sel is None else y[sel])), name
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    for key in (('both', 'down', True), ('item', 'up', False), ('user', 'down', True)):
        side, direction, slide = key
        cf, target, B = ran[key]
        how = dict(direction=direction, side=side, budget=B, slide=slide)
        tt = torch.from_numpy(target)
        for cat in (host, dev):
            for batch in (1, 3, 8192):
                cat.pair_batch = batch                          # an attribute, set after construction
                equal(cat.counterfactual(users, items, target=tt, **how), cf)
            equal(cat.counterfactual(torch.from_numpy(users)[perm].to(DEV), items[perm.numpy()], target=tt[perm], **how),
                  cf, perm.to(DEV))
            equal(cat.counterfactual(users[7:8], items[7:8], target=tt[7:8], **how), cf, slice(7, 8))
            empty = cat.counterfactual([], [], target=1.0, **how)
            assert tuple(empty.order.shape) == (0, B) and tuple(empty.scores.shape) == (0, B + 1)
            assert tuple(empty.steps.shape) == (0,) and empty.crossed.dtype == torch.bool

    # ---- what_if, leave_one_out, pair_reviews, explain and score_pairs answer as before
    after = (host.what_if(users, items, drop_user=[[0][:int(cu[a])] for a in users]), host.leave_one_out(users, items),
             host.pair_reviews(users, items), host.explain(items, k=3, side='item'))
    for a, b in zip(before, after):
        for name in a._fields:
            assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert torch.equal(bits(pairs_before), bits(host.score_pairs(users[real], items[real])))
