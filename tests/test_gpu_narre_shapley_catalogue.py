"""``NarreCatalogue.shapley`` on tests/golden/tiny (recommend.py; include/r4r.h, "NARRE Shapley values").

For a grid of (user, item) pairs that includes the owner without a review and the owners with more than R reviews on
both sides, every coalition's score must equal ``what_if`` of the same removals bit for bit (the removals of coalition c
as ``what_if``'s mask form: bit r = the owner's review r removed), the shares must lie within narre_shapley_ref's bound of
the float64 combination of those scores, a lone review's share is ``leave_one_out``'s delta, and towers='device',
``pair_batch``, the order of the pairs, a pair alone and no pair must not change a bit."""
import numpy as np
import pytest
import torch

from narre_shapley_ref import phi_bound, shapley_from_values
from test_gpu_narre_catalogue import _tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda'
bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t


def _with_a_lone_and_an_empty_owner(pool):
    """The pool with two more owners (the fixture has neither: every item has 6 .. 14 reviews, every user 2 .. 16): the
    last owner's last review goes to a new owner, who has that ONE review, and the owner after has none."""
    import copy
    p = copy.copy(pool)
    last = pool.first[-1]
    assert last - pool.first[-2] >= 2
    p.owners, p.first, p._dev = pool.owners + 2, np.concatenate([pool.first[:-1], [last - 1, last, last]]).astype(pool.first.dtype), None
    return p


def removal_masks(live_u, live_i, joint_side):
    """Per pair the masks of every coalition of a game -> (mask_u, mask_i) int64 [n, 2^P], n players per pair.
    ``joint_side``: 'user' / 'item' (that side's live reviews play) or 'joint' (the user's first, then the item's)."""
    nu = live_u if joint_side != 'item' else np.zeros_like(live_u)
    ni = live_i if joint_side != 'user' else np.zeros_like(live_i)
    P = max(int((nu + ni).max()), 1)
    c = np.arange(1 << P, dtype=np.int64)[None, :]
    absent_u = (~c) & ((np.int64(1) << nu[:, None]) - 1)                          # player t of the user: review t
    absent_i = ((~c) >> nu[:, None]) & ((np.int64(1) << ni[:, None]) - 1)
    return torch.from_numpy(absent_u), torch.from_numpy(absent_i), nu + ni, P


def check_game(cat, sh, users, items, live_u, live_i, game, slide):
    """One game of ``sh`` against what_if, float64 and the axioms."""
    mu, mi, n_of, P = removal_masks(live_u, live_i, game)
    wi = cat.what_if(users, items, drop_user=mu, drop_item=mi, slide=slide)
    table = sh.values[1 if game == 'item' else 0]
    assert tuple(table.shape) == (len(users), 1 << P) and torch.equal(bits(sh.base), bits(wi.base))
    table, want = table.cpu().numpy(), wi.scores.cpu().numpy()
    phi_u, phi_i = sh.phi_user.cpu().numpy(), sh.phi_item.cpu().numpy()
    empty = (sh.empty_item if game == 'item' else sh.empty_user).cpu().numpy()
    base = sh.base.cpu().numpy()
    worst = 0.0
    for p in range(len(users)):
        n = int(n_of[p])
        vals = table[p, :1 << n]
        assert np.array_equal(vals.view(np.int32), want[p, :1 << n].view(np.int32)), (game, p)
        assert vals[-1].view(np.int32) == base[p].view(np.int32) and vals[0].view(np.int32) == empty[p].view(np.int32)
        a = int(live_u[p]) if game != 'item' else 0
        phi = np.concatenate([phi_u[p, :a], phi_i[p, :n - a]]).astype(np.float64)
        ref = shapley_from_values(vals, n)
        bound, _ = phi_bound(vals, n)
        assert (np.abs(phi - ref) <= bound).all(), (game, p, phi, ref, bound)
        if n:
            worst = max(worst, float((np.abs(phi - ref) / bound).max()))
            assert abs(phi.sum() - (float(base[p]) - float(empty[p]))) <= bound.sum() + n * 2.0 ** -53 * np.abs(phi).sum()
        if game != 'item':
            assert (phi_u[p, a:].view(np.int32) == 0).all()
        if game != 'user':
            assert (phi_i[p, n - a:].view(np.int32) == 0).all()
    return worst


def test_shapley_on_tiny(tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue, Shapley
    hp, train, test, model, W = _tiny(tmp_path)
    monkeypatch.setattr(train.store, 'items', _with_a_lone_and_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_a_lone_and_an_empty_owner(train.store.users))
    host = NarreCatalogue(model, hp, train)
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=7)
    R = int(hp['narre_num_reviews'])
    pu, pi = host._narre_side('user')[1], host._narre_side('item')[1]
    cu, ci = pu.first[1:] - pu.first[:-1], pi.first[1:] - pi.first[:-1]
    assert int(cu.max()) > R and int(ci.max()) > R and cu[-1] == 0 and ci[-1] == 0 and cu[-2] == 1 and ci[-2] == 1
    us = np.unique(np.array([0, 3, int(cu.argmax()), int(cu[:-2].argmin()), pu.owners - 2, pu.owners - 1], dtype=np.int64))
    its = np.unique(np.array([1, 2, int(ci.argmax()), int(ci[:-2].argmin()), pi.owners - 2, pi.owners - 1], dtype=np.int64))
    users, items = np.repeat(us, len(its)), np.tile(its, len(us))
    n = len(users)
    live_u, live_i = np.minimum(cu[users], R).astype(np.int64), np.minimum(ci[items], R).astype(np.int64)
    loo = host.leave_one_out(users, items)
    before = (loo, host.what_if(users, items, drop_user=[[0][:int(cu[a])] for a in users]))

    # ---- the one-side games, slide on and off: values, shares, axioms
    runs = {}
    for slide in (True, False):
        both = host.shapley(users, items, values=True, slide=slide)
        assert isinstance(both, Shapley) and all(t.is_cuda for t in both[:7]) and len(both.values) == 2
        assert tuple(both.phi_user.shape) == tuple(both.phi_item.shape) == (n, R) and both.live_user.dtype == torch.int64
        assert np.array_equal(both.live_user.cpu().numpy(), live_u) and np.array_equal(both.live_item.cpu().numpy(), live_i)
        worst = max(check_game(host, both, users, items, live_u, live_i, 'user', slide),
                    check_game(host, both, users, items, live_u, live_i, 'item', slide))
        print('tiny, slide=%s: worst |phi - float64 of the own values| / bound %.3f' % (slide, worst))
        runs[slide] = both
        # side='both' is the two one-side calls, bit for bit
        for side, mine, other in (('user', 0, 1), ('item', 1, 0)):
            one = host.shapley(users, items, side=side, values=True, slide=slide)
            name = lambda f: f + '_' + side
            assert torch.equal(bits(getattr(one, name('phi'))), bits(getattr(both, name('phi'))))
            assert torch.equal(bits(getattr(one, name('empty'))), bits(getattr(both, name('empty'))))
            assert torch.equal(bits(one.base), bits(both.base)) and one.values[other] is None
            nw = one.values[mine].shape[1]
            live = torch.from_numpy(live_u if side == 'user' else live_i).to(DEV)
            written = torch.arange(nw, device=DEV)[None, :] < (1 << live)[:, None]
            assert torch.equal(bits(one.values[mine])[written], bits(both.values[mine])[written])
            off = 'item' if side == 'user' else 'user'         # the side that does not play: zeros, and empty = base
            assert not bool(getattr(one, 'phi_' + off).any()) and torch.equal(bits(getattr(one, 'empty_' + off)), bits(one.base))
            assert torch.equal(bits(getattr(one, 'phi_' + off)), torch.zeros((n, R), dtype=torch.int32, device=DEV))
    assert torch.equal(bits(runs[True].base), bits(loo.base))
    # the slide-in matters: for owners with more than R reviews the two removals differ
    assert not torch.equal(bits(runs[True].phi_user), bits(runs[False].phi_user))

    # ---- a pair with ONE live review on a side: its share is leave_one_out's delta (n = 1: phi = v(1) - v(0))
    both = runs[True]
    seen = 0
    for side, live, phi, delta, tab in (('user', live_u, both.phi_user, loo.delta_user, both.values[0]),
                                        ('item', live_i, both.phi_item, loo.delta_item, both.values[1])):
        for p in np.flatnonzero(live == 1):
            bound, _ = phi_bound(tab[p, :2].cpu().numpy(), 1)
            assert abs(float(phi[p, 0]) - float(delta[p, 0])) <= bound[0] + 2.0 ** -24 * abs(float(delta[p, 0]))
            seen += 1
    assert seen > 0

    # ---- one joint game over both sides, on the pairs within the limit; beyond, refused before anything runs
    few = np.flatnonzero(live_u + live_i <= 12)
    assert len(few) >= 4 and int((live_u + live_i)[few].max()) > R and (live_u + live_i).max() > 16
    with pytest.raises(ValueError, match='at most 16 players.*has %d' % int((live_u + live_i).max())):
        host.shapley(users, items, joint=True)
    ju, ji = users[few], items[few]
    joint = host.shapley(ju, ji, joint=True, values=True)
    assert joint.values[0] is joint.values[1] and torch.equal(bits(joint.empty_user), bits(joint.empty_item))
    check_game(host, joint, ju, ji, live_u[few], live_i[few], 'joint', True)
    total = joint.phi_user.double().sum(1) + joint.phi_item.double().sum(1)
    gap = (total - (joint.base.double() - joint.empty_user.double())).abs().cpu().numpy()
    for p in range(len(few)):
        nn = int(live_u[few][p] + live_i[few][p])
        bound, _ = phi_bound(joint.values[0][p].cpu().numpy(), nn)
        assert gap[p] <= bound.sum() + 2.0 ** -50 * float(total[p].abs()), p

    # ---- deletion_curve by='shapley' is deletion_curve by that tensor
    for side in ('user', 'item'):
        for direction in ('up', 'down'):
            a = host.deletion_curve(users, items, by='shapley', side=side, direction=direction)
            b = host.deletion_curve(users, items, by=getattr(both, 'phi_' + side), side=side, direction=direction)
            for name in a._fields:
                assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), (side, direction, name)

    # ---- towers='device', pair_batch, permuted pairs, a pair alone, no pair: the same bits
    def equal(a, b, sel=None):
        for name in Shapley._fields[:7]:
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(bits(x), bits(y if sel is None else y[sel])), name
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    for cat in (host, dev):
        for batch in (1, 3, 8192):
            cat.pair_batch = batch                              # an attribute, set after construction
            equal(cat.shapley(users, items), both)
        equal(cat.shapley(torch.from_numpy(users)[perm].to(DEV), items[perm.numpy()]), both, perm.to(DEV))
        equal(cat.shapley(users[7:8], items[7:8]), both, slice(7, 8))
        equal(cat.shapley(ju, ji, joint=True), joint)
        for kw in (dict(), dict(side='item', values=True), dict(joint=True, values=True)):
            empty = cat.shapley([], [], **kw)
            assert tuple(empty.phi_user.shape) == tuple(empty.phi_item.shape) == (0, R) and empty.phi_user.dtype == torch.float32
            assert tuple(empty.base.shape) == tuple(empty.empty_user.shape) == tuple(empty.empty_item.shape) == (0,)
            assert empty.live_user.dtype == empty.live_item.dtype == torch.int64 and tuple(empty.live_item.shape) == (0,)
            assert (empty.values is None) == ('values' not in kw)

    # ---- the other catalogue classes refuse, with the way out
    for cls in ('Catalogue', 'ReluCatalogue', 'TransNetCatalogue', 'MFCatalogue'):
        other = object.__new__(getattr(reviews4rec_amd, cls))
        other.hp = dict(model_type='deepconn')
        with pytest.raises(RuntimeError, match='leave_one_out'):
            other.shapley(users, items)
    with pytest.raises(KeyError):
        host.shapley([0], [10 ** 6])
    with pytest.raises(ValueError, match='2 users against 3 items'):
        host.shapley([0, 1], [0, 1, 2])

    # ---- what was there before answers as before
    after = (host.leave_one_out(users, items), host.what_if(users, items, drop_user=[[0][:int(cu[a])] for a in users]))
    for a, b in zip(before, after):
        for name in a._fields:
            assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
