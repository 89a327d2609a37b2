"""``NarreCatalogue.what_if`` / ``leave_one_out`` / ``deletion_curve`` on tests/golden/tiny (recommend.py; include/r4r.h,
"NARRE what-if scores").

For a grid of (user, item) pairs that includes the owner without a review and an owner with more than R reviews on both
sides, every leave-one-out score must equal a float64 COPY OF THE MODEL'S OWN modules (tower.fc, the attention scorers,
final, the embedding and bias tables) fed the LOADER's ``skip``-built reviews and neighbour ids for that removal
(``data._np_reviews`` / ``_np_neighbours``: what a training rating sees of its own pair), within narre_whatif_ref's
bounds with the fp32 tower fc's roundings carried in -- that holds the class's plumbing, the slide-in of review R + 1 and
the padding slot, not only the kernels.  ``what_if`` takes lists and masks alike; ``slide=False`` is a pad substitution
written out by hand; ``deletion_curve`` is ``what_if`` over a host sort; and towers='device', ``pair_batch``, the order
of the pairs and a pair alone must not change a bit."""
import copy

import numpy as np
import pytest
import torch

from head_ref import U32, compare, d64
from narre_whatif_ref import logits_ref, whatif_ref
from test_gpu_narre_catalogue import _tiny
from test_gpu_narre_explain_catalogue import _with_an_empty_owner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t


class _Side64:
    """One side in float64 through copies of the model's own modules, over the kernels' own pooled features."""

    def __init__(self, cat, side, ids):
        self.cat, self.ids = cat, ids
        user, self.pool, self.tower, self.pad = cat._narre_side(side)
        m = cat.model
        cp = lambda mod: copy.deepcopy(mod).double().cpu().eval()
        self.scorer = cp(m.attention_scorer_user if user else m.attention_scorer_item)
        own, other = (m.user_embedding, m.item_embedding) if user else (m.item_embedding, m.user_embedding)
        self.fc, self.own, self.other = cp(self.tower.fc), cp(own), cp(other)
        self.R, self.W = int(cat.hp['narre_num_reviews']), int(cat.hp['narre_num_words'])
        self.count = self.pool.first[ids + 1] - self.pool.first[ids]
        # every document this side needs -- the loader's (owner, skip) reviews, the owners' first S_MAX reviews and the
        # all-padding review -- goes through the conv in ONE call: equal documents then have equal pooled features
        from reviews4rec_amd.data import _np_neighbours, _np_review_slots, _np_reviews
        R, pool, n = self.R, self.pool, len(ids)
        skips = np.tile(np.arange(-1, R, dtype=np.int64), n)
        rb, re = np.repeat(pool.first[ids], R + 1), np.repeat(pool.first[ids + 1], R + 1)
        fed = _np_reviews(pool.tok, pool.rev_off, rb, re, skips, R, self.W)
        self.fed_nb = torch.from_numpy(_np_neighbours(pool.nb, rb, re, skips, self.pad))
        slots, self.slot_nb = _np_review_slots(pool.tok, pool.rev_off, pool.nb, pool.first[ids], pool.first[ids + 1], 0,
                                               self.S_MAX, self.W, self.pad)
        every = self.pooled(np.concatenate([fed.reshape(-1, self.W), slots.reshape(-1, self.W), np.zeros((1, self.W), np.int64)]))
        self.fed_pooled = every[:fed.shape[0] * R].reshape(n * (R + 1), R, -1)
        self.slot_pooled = every[fed.shape[0] * R:-1].reshape(n, self.S_MAX, -1)
        self.pad_pooled = every[-1:]

    S_MAX = 16

    def pooled(self, docs):
        """docs int64 [..., W] -> the device conv's pooled features as float64 [..., F]."""
        from reviews4rec_amd import ops
        conv = self.tower.convs[0]
        flat = torch.from_numpy(np.ascontiguousarray(docs).reshape(-1, self.W)).to(DEV)
        with torch.no_grad():
            p, _ = ops.textcnn_fwd_raw(flat, self.cat._words(), conv.weight.detach(), conv.bias.detach())
        return d64(p).reshape(tuple(docs.shape[:-1]) + (-1,))

    def latents(self, pooled):
        """-> (z, dz): the float64 latents and what the fp32 fc (an F-term dot and the bias, c = F + 1) may be off by."""
        w, b = self.fc.weight.detach(), self.fc.bias.detach()
        F = w.shape[1]
        return pooled @ w.T + b, (F + 1) * U32 * (pooled.abs() @ w.abs().T + b.abs())

    def loader_fed(self):
        """p [n, R + 1, L]: NARRE.py:95-119 on what the loader builds with skip = -1 (index 0) and skip = r (index r + 1)."""
        R, n, nb = self.R, len(self.ids), self.fed_nb
        with torch.no_grad():
            z = self.fc(self.fed_pooled)
            logits = self.scorer(torch.cat([z, self.other(nb)], dim=-1))[:, :, 0]
            a = torch.softmax(logits, dim=-1)
            p = torch.sum(a.unsqueeze(-1) * z, dim=1) + self.own(torch.from_numpy(np.repeat(self.ids, R + 1)))
        return p.reshape(n, R + 1, -1)

    def ref_side(self, S):
        """``whatif_ref``'s side over S slots at the float64 latents, with the fc's and the logits' bounds."""
        assert S <= self.S_MAX
        nb = self.slot_nb[:, :S]
        z, dz = self.latents(self.slot_pooled[:, :S])
        z_pad, dz_pad = self.latents(self.pad_pooled)
        par = dict(other_table=self.other.weight.detach(), W0=self.scorer[0].weight.detach(), b0=self.scorer[0].bias.detach(),
                   w3=self.scorer[3].weight.detach().reshape(-1), b3=self.scorer[3].bias.detach())
        lg = logits_ref(dict(par, z=z, nb=torch.from_numpy(np.ascontiguousarray(nb))), dz=dz)['logit']
        lp = logits_ref(dict(par, z=z_pad.reshape(1, 1, -1), nb=torch.tensor([[self.pad]])), dz=dz_pad.reshape(1, 1, -1))['logit']
        return dict(z=z, dz=dz, logit=lg[0], dlogit=lg[1], z_pad=z_pad.reshape(-1), dz_pad=dz_pad.reshape(-1),
                    logit_pad=float(lp[0].reshape(())), dlogit_pad=lp[1].reshape(()), R=self.R,
                    own=self.own.weight.detach()[torch.from_numpy(self.ids)])


def _masks(lists):
    return torch.tensor([[sum(1 << r for r in variant) for variant in row] for row in lists], dtype=torch.int64)


def test_what_if_leave_one_out_and_deletion_curve_on_tiny(tmp_path, monkeypatch):
    from reviews4rec_amd import DeletionCurve, LeaveOneOut, NarreCatalogue, WhatIf, ops
    hp, train, test, model, W = _tiny(tmp_path)
    monkeypatch.setattr(train.store, 'items', _with_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_an_empty_owner(train.store.users))
    host = NarreCatalogue(model, hp, train)
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=7)
    R, L = int(hp['narre_num_reviews']), int(hp['latent_size'])
    pu, pi = host._narre_side('user')[1], host._narre_side('item')[1]
    cu, ci = pu.first[1:] - pu.first[:-1], pi.first[1:] - pi.first[:-1]
    # the owner without a review is the last of each side; the fixture HAS owners with more than R reviews
    assert int(cu.max()) > R and int(ci.max()) > R and cu[-1] == 0 and ci[-1] == 0
    us = np.unique(np.array([0, 3, int(cu.argmax()), int(cu[:-1].argmin()), pu.owners - 1], dtype=np.int64))
    its = np.unique(np.array([1, 2, int(ci.argmax()), int(ci[:-1].argmin()), pi.owners - 1], dtype=np.int64))
    users, items = np.repeat(us, len(its)), np.tile(its, len(us))
    n = len(users)
    u_row, i_row = torch.from_numpy(np.searchsorted(us, users)), torch.from_numpy(np.searchsorted(its, items))

    before = (host.pair_reviews(users, items), host.explain(items, k=3, side='item'))
    real = (users < hp['total_users']) & (items < hp['total_items'])
    pairs_before = host.score_pairs(users[real], items[real])

    # ---- the float64 side
    su, si = _Side64(host, 'user', us), _Side64(host, 'item', its)
    final = copy.deepcopy(model.final).double().cpu().eval()
    W1, b1, w = final[1].weight.detach(), final[1].bias.detach(), final[3].weight.detach().reshape(-1)
    qb = d64(model.user_bias).reshape(-1)[us] + d64(model.global_bias).reshape(()) + d64(final[3].bias).reshape(())
    cb = d64(model.item_bias).reshape(-1)[its]
    score64 = lambda a, b: torch.relu((a * b) @ W1.T + b1) @ w + qb[u_row] + cb[i_row]
    fed_u, fed_i = su.loader_fed(), si.loader_fed()
    base64 = score64(fed_u[u_row, 0], fed_i[i_row, 0])

    # ---- leave_one_out against the loader's own removals
    loo = host.leave_one_out(users, items)
    assert isinstance(loo, LeaveOneOut)
    for name in LeaveOneOut._fields:
        t = getattr(loo, name)
        shape = (n,) if name in ('base', 'live_user', 'live_item') else (n, R)
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == (torch.int64 if name[:4] == 'live' else torch.float32), name
    one = (torch.ones(R, dtype=torch.int64) << torch.arange(R))[None, :].expand(n, R)
    none = torch.zeros((n, R), dtype=torch.int64)
    ref = whatif_ref(su.ref_side(R + 1), si.ref_side(R + 1), u_row, i_row, torch.cat([none[:, :1], one, none], 1),
                     torch.cat([none[:, :1], none, one], 1), W1, b1, w, qb, cb)
    val, bound = ref['score']
    bound = bound + U32 * qb[u_row].abs()[:, None]              # the class rounds the summed scalars once
    want = torch.cat([base64[:, None]] + [score64(fed_u[u_row, r + 1], fed_i[i_row, 0])[:, None] for r in range(R)]
                     + [score64(fed_u[u_row, 0], fed_i[i_row, r + 1])[:, None] for r in range(R)], 1)
    assert float((val - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))    # the reference IS the loader's skip
    got = torch.cat([loo.base[:, None], loo.without_user, loo.without_item], 1)
    print('NARRE leave_one_out: worst error / bound %.3f' % compare('leave_one_out', got, want, bound))
    live_u = torch.from_numpy(np.minimum(cu[users], R)).to(DEV)
    live_i = torch.from_numpy(np.minimum(ci[items], R)).to(DEV)
    assert torch.equal(loo.live_user, live_u) and torch.equal(loo.live_item, live_i)
    assert int(live_u.min()) == 0 and int(live_i.min()) == 0 and int(live_u.max()) == R
    slot = torch.arange(R, device=DEV)[None, :]
    for without, delta, live in ((loo.without_user, loo.delta_user, live_u), (loo.without_item, loo.delta_item, live_i)):
        dead = slot >= live[:, None]
        assert torch.equal(bits(without[dead]), bits(loo.base[:, None].expand(n, R)[dead])) and bool((delta[dead] == 0).all())
        assert torch.equal(bits(delta), bits(loo.base[:, None] - without))
        assert float(delta[~dead].abs().max()) > 0
    # review R + 1 slides in: for an owner with more than R reviews, slide=False (padding at the tail) differs
    occl = host.leave_one_out(users, items, slide=False)
    many = torch.from_numpy(cu[users] > R).to(DEV)
    assert torch.equal(bits(occl.base), bits(loo.base))
    assert not torch.equal(occl.without_user[many], loo.without_user[many])

    # ---- base against score_pairs, by another fp32 chain (test_gpu_narre_pair_catalogue's rule)
    pairs = host.score_pairs(users[real], items[real]).cpu().double()
    held = torch.isfinite(pairs)
    assert int(held.sum()) >= 6
    sel = torch.from_numpy(real)
    tol = bound[:, 0][sel] + 1e-5 + 1e-5 * base64.abs()[sel]
    assert bool(((loo.base.cpu().double()[sel] - pairs).abs()[held] <= tol[held]).all())

    # ---- what_if: several drops per variant, as lists and as masks, against the float64 restatement
    def variants(c):
        v = [[], [0], [0, 1], [1, 3, 5], [c - 1], [r for r in range(12) if r % 2 == 0]]
        return [[r for r in row if 0 <= r < c] for row in v]
    drop_u = [variants(int(cu[a])) for a in users]
    drop_i = [variants(int(ci[b]))[::-1] for b in items]
    wi = host.what_if(users, items, drop_user=drop_u, drop_item=drop_i)
    assert isinstance(wi, WhatIf) and tuple(wi.scores.shape) == (n, 6) and tuple(wi.base.shape) == (n,)
    assert torch.equal(bits(wi.base), bits(loo.base))
    mu, mi = _masks(drop_u), _masks(drop_i)
    most = lambda rows: max(len(v) for row in rows for v in row)
    ref = whatif_ref(su.ref_side(R + most(drop_u)), si.ref_side(R + most(drop_i)), u_row, i_row, mu, mi, W1, b1, w, qb, cb)
    print('NARRE what_if: worst error / bound %.3f'
          % compare('what_if', wi.scores, ref['score'][0], ref['score'][1] + U32 * qb[u_row].abs()[:, None]))
    as_masks = host.what_if(users, items, drop_user=mu.to(DEV), drop_item=mi.numpy())
    assert torch.equal(bits(as_masks.scores), bits(wi.scores)) and torch.equal(bits(as_masks.base), bits(wi.base))
    only_u = host.what_if(users, items, drop_user=[row[1] for row in drop_u])            # one variant, one side
    assert tuple(only_u.scores.shape) == (n, 1)
    both = host.what_if(users, items, drop_user=mu[:, 1:2], drop_item=torch.zeros((n, 1), dtype=torch.int64))
    assert torch.equal(bits(only_u.scores), bits(both.scores))
    assert torch.equal(bits(only_u.scores[:, 0]), bits(torch.where(live_u > 0, loo.without_user[:, 0], loo.base)))
    nothing = host.what_if(users, items)
    assert tuple(nothing.scores.shape) == (n, 1) and torch.equal(bits(nothing.scores[:, 0]), bits(loo.base))

    # ---- slide=False is a pad substitution, written out by hand: the kept slots in order, then the pad slot
    uu = np.unique(users)
    side_u, side_i = host._whatif_side('user', uu, R), host._whatif_side('item', np.unique(items), R)
    r_drop = 2
    keep = [r for r in range(R) if r != r_drop]
    rows = torch.from_numpy(np.searchsorted(uu, users)).to(DEV)
    z_m = torch.cat([side_u['z'][rows][:, keep], side_u['z_pad'][None, None, :].expand(n, 1, L)], 1).contiguous()
    lg_m = torch.cat([side_u['logit'][rows][:, keep], torch.full((n, 1), side_u['logit_pad'], device=DEV)], 1).contiguous()
    manual_u = dict(side_u, z=z_m, logit=lg_m, own=side_u['own'][rows].contiguous())
    f64 = lambda t: t.detach().to(torch.float64)
    qb32 = (f64(model.user_bias).reshape(-1)[torch.from_numpy(users).to(DEV)] + f64(model.global_bias).reshape(())
            + f64(model.final[3].bias).reshape(())).to(torch.float32).contiguous()
    cb32 = model.item_bias.detach().reshape(-1)[torch.from_numpy(np.unique(items)).to(DEV)].contiguous()
    manual = ops.narre_whatif(manual_u, side_i, torch.arange(n, device=DEV), torch.from_numpy(np.searchsorted(np.unique(items), items)).to(DEV),
                              None, None, model.final[1].weight.detach(), model.final[1].bias.detach(),
                              model.final[3].weight.detach().reshape(-1), q_bias=qb32, c_bias=cb32)
    occluded = host.what_if(users, items, drop_user=torch.full((n, 1), 1 << r_drop, dtype=torch.int64), slide=False)
    assert torch.equal(bits(occluded.scores), bits(manual))
    alive = live_u > r_drop
    assert torch.equal(bits(occluded.scores[:, 0][alive]), bits(occl.without_user[:, r_drop][alive]))

    # ---- deletion_curve is what_if over a host sort of the key
    pr = host.pair_reviews(users, items)
    ex = {'user': host.explain(users, k=1, side='user').attention, 'item': host.explain(items, k=1, side='item').attention}
    own_key = torch.randn((n, R), generator=torch.Generator().manual_seed(5))
    own_key[:, 3] = own_key[:, 1]                               # a tie: the ascending slot goes first
    for by, side, direction in (('rev', 'user', 'up'), ('attention', 'item', 'up'), ('rev', 'item', 'down'), (own_key, 'user', 'up')):
        dc = host.deletion_curve(users, items, by=by, side=side, direction=direction)
        assert isinstance(dc, DeletionCurve) and tuple(dc.scores.shape) == (n, R + 1) and tuple(dc.aopc.shape) == (n,)
        key = (getattr(pr, 'rev_' + side) if isinstance(by, str) and by == 'rev' else ex[side] if isinstance(by, str) else by)
        key = key.cpu().numpy() * (1.0 if direction == 'up' else -1.0)
        live = (live_u if side == 'user' else live_i).cpu().numpy()
        masks, order = np.zeros((n, R), np.int64), np.full((n, R), -1, np.int64)
        for p in range(n):
            o = sorted(range(int(live[p])), key=lambda r: (-float(key[p, r]), r))
            order[p, :len(o)] = o
            for k in range(R):
                masks[p, k] = sum(1 << r for r in o[:k + 1])
        assert np.array_equal(dc.order.cpu().numpy(), order) and np.array_equal(dc.live.cpu().numpy(), live)
        m = torch.from_numpy(masks)
        wk = host.what_if(users, items, **{'drop_' + side: m})
        assert torch.equal(bits(dc.scores[:, 1:]), bits(wk.scores)) and torch.equal(bits(dc.scores[:, 0]), bits(wk.base))
        sc = dc.scores.cpu().double().numpy()
        aopc = np.array([np.mean(sc[p, 0] - sc[p, 1:int(live[p]) + 1]) if live[p] else 0.0 for p in range(n)])
        assert np.allclose(dc.aopc.cpu().numpy(), aopc, rtol=1e-6, atol=1e-7)
        # the curve ends where every live review is gone: one value per pair, whatever the key
        assert torch.equal(bits(dc.scores[:, R]), bits(host.deletion_curve(users, items, by=own_key, side=side).scores[:, R]))

    # ---- towers='device', another chunking, pair_batch, permuted pairs, a pair alone, no pair: the same bits
    def equal(a, b, sel=None):
        for name in a._fields:
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(bits(x), bits(y if sel is None else y[sel])), name
    dc = host.deletion_curve(users, items, by='rev', side='item')
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    for cat in (host, dev):
        for batch in (1, 3, 8192):
            cat.pair_batch = batch                              # an attribute, set after construction
            equal(cat.leave_one_out(users, items), loo)
            equal(cat.what_if(users, items, drop_user=drop_u, drop_item=drop_i), wi)
        equal(cat.deletion_curve(users, items, by='rev', side='item'), dc)
        pu_, pi_ = torch.from_numpy(users)[perm].to(DEV), torch.from_numpy(items)[perm].to(DEV)
        equal(cat.leave_one_out(pu_, pi_), loo, perm.to(DEV))
        equal(cat.what_if(pu_, pi_, drop_user=mu[perm], drop_item=mi[perm]), wi, perm.to(DEV))
        equal(cat.leave_one_out(users[7:8], items[7:8]), loo, slice(7, 8))
        empty = cat.what_if([], [])
        assert tuple(empty.scores.shape) == (0, 1) and tuple(empty.base.shape) == (0,)
        assert tuple(cat.leave_one_out([], []).without_user.shape) == (0, R)
        assert tuple(cat.deletion_curve([], []).scores.shape) == (0, R + 1)

    # ---- every refusal, before anything is enqueued
    with pytest.raises(ValueError, match='2 users against 3 items'):
        host.what_if([0, 1], [0, 1, 2])
    for call in (host.what_if, host.leave_one_out, host.deletion_curve):
        with pytest.raises(KeyError):
            call([0], [10 ** 6])
        with pytest.raises(KeyError):
            call([-1], [0])
    few = int(cu[0])
    for drop in ([[few]], [[-1]], [[64]], [[0], [0]], [0], torch.zeros((1, 1), dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64),
                 torch.zeros((1, 0), dtype=torch.int64)):
        with pytest.raises(ValueError, match='drop_user'):
            host.what_if([0], [1], drop_user=drop)
    with pytest.raises(ValueError, match='variants per pair'):
        host.what_if([0], [1], drop_user=[[[0], []]], drop_item=[[0]])
    for kw in (dict(by='gradient'), dict(side='pair'), dict(direction='sideways'), dict(by=torch.zeros(1, R - 1))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            host.deletion_curve([0], [1], **kw)

    # ---- pair_reviews, explain and score_pairs answer as before
    after = (host.pair_reviews(users, items), host.explain(items, k=3, side='item'))
    for a, b in zip(before, after):
        for name in a._fields:
            assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert torch.equal(bits(pairs_before), bits(host.score_pairs(users[real], items[real])))
