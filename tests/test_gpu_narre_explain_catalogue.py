"""NarreCatalogue.explain and NarreCatalogue beyond latent_size 32 on tests/golden/tiny (recommend.py):
the explanations of every item and every user against a host recomputation, the class at latent sizes 33 and 64 against
the float64 oracle forward and the native engine, and main.main's explain_k hook."""
import os

import numpy as np
import pytest
import torch

import head_ref as hr
from helpers import materialise_tiny, tiny_hp
from test_gpu_narre_catalogue import _tiny
from test_gpu_recommend import check_lists
from test_narre_explain_host import explain_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _latents(cat, side, ids):
    """(z [n, R, L], nb [n, 10], the scorer's weights, the other side's table) as ``NarreCatalogue._attended`` builds
    them for the owners ``ids``, on the device."""
    from reviews4rec_amd.data import _np_neighbours, _np_reviews
    user, pool, conv, pad = cat._narre_side(side)
    R, Wd = int(cat.hp['narre_num_reviews']), int(cat.hp['narre_num_words'])
    rb, re = pool.first[ids], pool.first[ids + 1]
    none = np.full(len(ids), -1, np.int64)
    reviews = _np_reviews(pool.tok, pool.rev_off, rb, re, none, R, Wd)
    nb = torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, pad)).to(DEV)
    with torch.no_grad():
        z = cat._tower(conv, torch.from_numpy(reviews.reshape(len(ids) * R, Wd)).to(DEV)).view(len(ids), R, -1)
    m = cat.model
    scorer = m.attention_scorer_user if user else m.attention_scorer_item
    own, other = (m.user_embedding, m.item_embedding) if user else (m.item_embedding, m.user_embedding)
    weights = tuple(p.detach() for p in (scorer[0].weight, scorer[0].bias, scorer[3].weight, scorer[3].bias))
    return z, nb, weights, own.weight.detach(), other.weight.detach()


# ---------------------------------------------------------------- 1. latent_size 6, the fixture's weights
def _with_an_empty_owner(pool):
    """The pool with one more owner, who has no review (the fixture has none: every item has 6 .. 14, every user 2 .. 16)."""
    import copy
    p = copy.copy(pool)
    p.owners, p.first, p._dev = pool.owners + 1, np.append(pool.first, pool.first[-1]), None
    return p


def test_explanations_of_every_item_and_user_on_tiny(tmp_path, monkeypatch):
    from reviews4rec_amd import Explanation, NarreCatalogue, ops
    hp, train, test, model, W = _tiny(tmp_path)
    R, K = hp['narre_num_reviews'], 3
    assert (hp['latent_size'], R) == (6, 10)
    monkeypatch.setattr(train.store, 'items', _with_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_an_empty_owner(train.store.users))
    cat = NarreCatalogue(model, hp, train)
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=7)
    kinds = set()
    for side, total in (('item', hp['total_items']), ('user', hp['total_users'])):
        pool = cat._narre_side(side)[1]
        assert pool.owners == total + 1
        total = pool.owners                                   # every item / user, and the owner without a review
        ids = np.arange(total, dtype=np.int64)
        e = cat.explain(ids, k=K, side=side)
        assert isinstance(e, Explanation)
        for t, dt, shape in ((e.slots, torch.int64, (total, K)), (e.reviews, torch.int64, (total, K)),
                             (e.reviewers, torch.int64, (total, K)), (e.weights, torch.float32, (total, K)),
                             (e.attention, torch.float32, (total, R)), (e.live, torch.int64, (total,))):
            assert t.device.type == 'cuda' and t.dtype == dt and tuple(t.shape) == shape
        # live: owners with no review, with fewer than R, with more than R
        count = pool.first[ids + 1] - pool.first[ids]
        assert np.array_equal(e.live.cpu().numpy(), np.minimum(count, R))
        kinds |= {('none' if c == 0 else 'few' if c < R else 'exact' if c == R else 'many') for c in count.tolist()}
        # slots, reviews and reviewers: the list rules over the class's own attention, mapped back through the pool
        attn = e.attention.cpu().numpy()
        want_slot, want_w = explain_ref(attn, np.minimum(count, R), K)
        listed = want_slot >= 0
        want_rev = np.where(listed, pool.first[ids][:, None] + want_slot, -1)
        want_who = np.where(listed, pool.nb[np.where(listed, want_rev, 0)], -1)
        assert np.array_equal(e.slots.cpu().numpy(), want_slot)
        assert np.array_equal(e.weights.cpu().numpy().view(np.uint32), want_w.view(np.uint32))
        assert np.array_equal(e.reviews.cpu().numpy(), want_rev) and np.array_equal(e.reviewers.cpu().numpy(), want_who)
        assert (want_rev[listed] < pool.first[ids + 1][:, None].repeat(K, 1)[listed]).all()     # the owner's own reviews
        # the attention against float64 from the class's own review latents
        z, nb, weights, own, other = _latents(cat, side, ids)
        ref = hr.attention_ref(z, other[nb], *weights, None, torch.zeros((total, hp['latent_size'])))
        ratio = hr.compare('attention ' + side, e.attention, *ref['a_save'])
        print('tiny %s: attention against float64, worst error / bound %.3f' % (side, ratio))
        assert float((e.attention.double().sum(1) - 1).abs().max()) <= (R + 1) * hr.U32
        # the owner without a review: ten padded slots alike, none listed
        assert count[-1] == 0 and bool((e.attention[-1] == e.attention[-1, 0]).all()) and bool((e.slots[-1] == -1).all())
        assert bool((e.weights[-1] == 0).all()) and bool((e.reviews[-1] == -1).all()) and bool((e.reviewers[-1] == -1).all())
        # towers='device' and another chunking: the same bits
        e2 = dev.explain(ids, k=K, side=side)
        for a, b in zip(e, e2):
            assert torch.equal(a, b)
        assert hr.bits_equal(e.weights, e2.weights) and hr.bits_equal(e.attention, e2.attention)
        # ids as a device tensor, in another order and repeated
        pick = torch.tensor([total - 1, 0, 3, 0], device=DEV)
        e3 = cat.explain(pick, k=K, side=side)
        for a, b in zip(e, e3):
            assert torch.equal(a[pick], b)
        # the item side of the cache by the parent's path: r4r_narre_attn_fwd over the materialised neighbours + the id row
        if side == 'item':
            el = cat.eligible
            z, nb, weights, own, other = _latents(cat, side, el)
            with torch.no_grad():
                c = ops.narre_attention(z, other[nb].contiguous(), *weights, 0.0, False, None) + own[torch.from_numpy(el).to(DEV)]
            assert hr.bits_equal(cat.c[torch.from_numpy(el).to(DEV)], c) and hr.bits_equal(dev.c, cat.c)
    assert {'none', 'few', 'many'} <= kinds, kinds
    with pytest.raises(ValueError):
        cat.explain([0], k=R + 1)
    with pytest.raises(KeyError):
        cat.explain([10 ** 6])


# ---------------------------------------------------------------- 2. latent sizes beyond r4r_narre_attn_fwd's
def _seeded(tmp_path, L):
    """NARRE at latent_size L on tiny: the seeded model as a run starts from it (xavier_init), every matrix but the word
    table doubled so that the scores spread over the rating scale."""
    import reviews4rec_amd
    from reviews4rec_amd.data import load_data
    from reviews4rec_amd.utils import xavier_init
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp('NARRE', root, latent_size=L), device=DEV)
    torch.manual_seed(1000 + L)
    model = reviews4rec_amd.get_model_class('NARRE')(hp)
    xavier_init(model)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() > 1 and 'word2vec' not in name:
                p.mul_(2.0)
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return hp, train, test, model.cuda().eval(), W


# The widest NARRE the fused native step runs at R = 10 and 100 filters: its head keeps 2056 + 347 L + 5 L^2 floats in LDS
# (narre_head_lds_bytes, csrc/narre_engine.hip), 163,504 bytes at 60 and 167,312 at 61 against 160 KiB.
# main.native_step_limits says 64; the C entry point refuses 61 .. 64.
NATIVE_MAX_L = 60


@pytest.mark.parametrize('L', [33, NATIVE_MAX_L, 64])
def test_the_catalogue_at_latent_sizes_beyond_32(L, tmp_path):
    """score_pairs over all pairs within the project's eval tolerance 1e-5 + 1e-5 |s| of the float64 oracle forward and,
    where the native step runs the width (33 and 60; at 64 it refuses, which is asserted), of the native engine's
    predict; recommend and rank agree with each other.  On the parent commit the constructor raises from C:
    narre_attn_fwd refuses L > 32.

    The tolerance against the weights used: the fp32 oracle forward against the float64 one on the CPU, all 1152 pairs,
    worst |difference| / tolerance 0.012 at L = 33, 0.009 at L = 60 and 0.009 at L = 64 (scores 2.7 .. 6.1); with the
    matrices four times xavier_init's instead of twice, 1.7 at 33 and 0.64 at 64 -- hence twice."""
    import oracle
    from reviews4rec_amd import NarreCatalogue
    from reviews4rec_amd import main as M
    hp, train, test, model, W = _seeded(tmp_path, L)
    assert (hp['latent_size'], hp['narre_num_reviews']) == (L, 10)
    U, I, K = hp['total_users'], hp['total_items'], 5
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    none = np.full(len(u), -1, np.int64)
    data = [torch.from_numpy(np.ascontiguousarray(f)) for f in test._review_fields_host(u, i, none, none, none)]
    data = data + [torch.from_numpy(u), torch.from_numpy(i)]
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    assert s64.std() > 0.2                                    # the scores are not flat: the attention matters
    cat = NarreCatalogue(model, hp, train)
    eligible = sorted({int(r[1]) for r in train.data})
    assert cat.eligible.tolist() == eligible and cat.c.shape == (I, L) and cat.W.shape == (L, L)
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    tol = 1e-5 + 1e-5 * np.abs(s64)
    el = np.zeros(I, bool)
    el[eligible] = True
    worst = float((np.abs(got[:, el] - s64[:, el]) / tol[:, el]).max())
    print('NARRE L=%d: score_pairs against the float64 oracle, worst |difference| / tolerance = %.3f' % (L, worst))
    assert (np.abs(got[:, el] - s64[:, el]) <= tol[:, el]).all(), worst
    assert np.isneginf(got[:, ~el]).all()
    engine = M.make_engine(dict(hp, engine='native'), model)
    assert engine is not None and hasattr(engine, 'predict')
    dev_data = [d.to(DEV) for d in data]
    if L <= NATIVE_MAX_L:
        with torch.no_grad():
            pred = torch.cat([engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone() for a in range(0, U * I, 96)])
        mine = pred.reshape(U, I).cpu().numpy().astype(np.float64)
        worst = float((np.abs(got[:, el] - mine[:, el]) / tol[:, el]).max())
        print('NARRE L=%d: score_pairs against predict, worst |difference| / tolerance = %.3f' % (L, worst))
        assert (np.abs(got[:, el] - mine[:, el]) <= tol[:, el]).all(), worst
    else:
        with pytest.raises(RuntimeError, match='narre_step: R = 10, L = %d need [0-9]+ bytes of LDS' % L):
            engine.predict([d[:96] for d in dev_data], None)
    # towers='device' is the same cache
    dev = NarreCatalogue(model, hp, train, towers='device', tower_batch=5)
    assert torch.equal(dev.c, cat.c) and torch.equal(dev.score_pairs(u, i).cpu(), torch.from_numpy(got.reshape(-1)))
    # the lists and the ranks, as at latent_size 6
    seen = {}
    for r in train.data:
        seen.setdefault(int(r[0]), set()).add(int(r[1]))
    users = np.arange(U, dtype=np.int64)
    for exclude in (True, False):
        ids, sc = cat.recommend(users, k=K, exclude_seen=exclude)
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        masked = np.where(el[None, :], s64, -np.inf)
        if exclude:
            for uu, items in seen.items():
                masked[uu, sorted(items)] = -np.inf
        check_lists(ids, sc, masked, tol, K, 'NARRE L=%d exclude=%s' % (L, exclude))
        flat = ids.reshape(-1)
        again = cat.score_pairs(np.repeat(users, K)[flat >= 0], flat[flat >= 0]).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), sc.reshape(-1)[flat >= 0].view(np.uint32))
        full, _ = cat.recommend(users, k=128, exclude_seen=exclude)
        ranks, rsc = cat.rank(u, i, exclude_seen=exclude)
        full, ranks = full.cpu().numpy(), ranks.cpu().numpy().reshape(U, I)
        assert np.array_equal(rsc.cpu().numpy().view(np.uint32), got.reshape(-1).view(np.uint32))
        assert (ranks[:, ~el] == -1).all() and (ranks[:, el] >= 0).all()
        held = 0
        for uu in range(U):
            for pos, item in enumerate(full[uu]):
                if item >= 0:
                    assert ranks[uu, item] == pos, (uu, item, pos)
                    held += 1
        assert held >= U
    # ... and the explanations at this width sum to 1 and list live slots only
    e = cat.explain(np.arange(I), k=3)
    assert float((e.attention.double().sum(1) - 1).abs().max()) <= 11 * hr.U32
    assert bool(((e.slots >= 0).sum(1) == e.live.clamp(max=3)).all()) and bool((e.slots < e.live[:, None]).all())


# ---------------------------------------------------------------- 3. main.main
def test_main_writes_the_explanations_of_the_trained_model(tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    meta, z = _fixture('NARRE', 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    runs = {}
    for tag, extra in (('with', dict(explain_k=3, explain_path=str(tmp_path / 'why.npz'))), ('without', {})):
        hp = tiny_hp('NARRE', root, log_file=str(tmp_path / ('log_' + tag)), model_path=str(tmp_path / ('model_' + tag)),
                     **extra)
        before = set(os.listdir(str(tmp_path)))
        final = M.main(hp)
        runs[tag] = (final, torch.load(hp['model_path'], map_location='cpu'), set(os.listdir(str(tmp_path))) - before, hp)
    assert runs['with'][0] == runs['without'][0]                               # the metrics are what they were
    assert set(runs['with'][1]) == set(runs['without'][1])
    for k, v in runs['with'][1].items():
        assert torch.equal(v, runs['without'][1][k]), k                        # ... and so is the training state
    assert runs['without'][2] == {'log_without', 'model_without'}, runs['without'][2]
    assert 'why.npz' in runs['with'][2]
    # the file holds NarreCatalogue.explain of the trained (best-on-validation) model, every eligible item
    hp = runs['with'][3]
    train, _, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class('NARRE')(hp)
    model.load_state_dict(runs['with'][1])
    f = np.load(str(tmp_path / 'why.npz'))
    assert set(f.files) == {'items', 'slots', 'reviews', 'reviewers', 'weights'}
    cat = NarreCatalogue(model.cuda().eval(), hp, train)
    items = np.array(sorted({int(r[1]) for r in train.data}), np.int64)
    assert np.array_equal(f['items'], items)
    e = cat.explain(items, k=3)
    assert np.array_equal(f['slots'], e.slots.cpu().numpy()) and np.array_equal(f['reviews'], e.reviews.cpu().numpy())
    assert np.array_equal(f['reviewers'], e.reviewers.cpu().numpy())
    assert np.array_equal(f['weights'].view(np.uint32), e.weights.cpu().numpy().view(np.uint32))
    assert (f['slots'][:, 0] >= 0).all()                                       # an eligible item has a review
