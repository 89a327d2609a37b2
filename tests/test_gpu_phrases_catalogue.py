"""``explain_words`` of the four catalogue classes on tests/golden/tiny (recommend.py; include/r4r.h, "Phrase
explanations"): deepconn, deepconn++, transnet++ (the source towers) and NARRE (one row per review slot).

Every item's and every user's lists must equal a host recomputation -- pooled / argmax from ops.textcnn_fwd_raw over
numpy-built documents, the lists by phrases_ref, reviews / offsets / tokens read back from the pools with numpy loops --
towers='device' must give the bits of towers='host', weights='latent' those of the column norms passed explicitly, and
main.main's explain_words_k hook must write ``explain_words(cat.eligible)`` of the model it trained."""
import os

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from phrases_ref import bits, phrases_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 4
FIELDS = ('positions', 'scores', 'filters', 'tokens', 'reviews', 'offsets', 'windows')


def _catalogues(mt, tmp_path, monkeypatch, **kw):
    """(host catalogue, device catalogue, hp) over the fixture's weights; both pools get one more owner without a review."""
    from test_gpu_narre_explain_catalogue import _with_an_empty_owner
    from test_gpu_tower_span import _tiny
    cls, hp, train, _, model = _tiny(mt, tmp_path)
    monkeypatch.setattr(train.store, 'items', _with_an_empty_owner(train.store.items))
    monkeypatch.setattr(train.store, 'users', _with_an_empty_owner(train.store.users))
    return cls(model, hp, train, **kw), cls(model, hp, train, towers='device', tower_batch=7), hp


def same(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        if x is None or y is None:
            assert x is None and y is None, (what, name)
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), (what, name)


def recompute(cat, side, ids, k, wt=None):
    """The host recomputation, document layout -> dict of numpy arrays by ``Phrases`` field."""
    from reviews4rec_amd import ops
    from reviews4rec_amd.data import _np_docs
    pool, tower, _ = cat._phrase_side(side)
    T = int(cat.hp['input_length'])
    none = np.full(len(ids), -1, np.int64)
    docs = _np_docs(pool.tok, pool.rev_off, pool.first[ids], pool.first[ids + 1], none, T)
    conv = tower.convs[0]
    with torch.no_grad():
        pooled, argmax = ops.textcnn_fwd_raw(torch.from_numpy(docs).to(DEV), cat._words(), conv.weight.detach(),
                                             conv.bias.detach())
    pos, score, filt, win = phrases_ref(pooled.cpu().numpy(), argmax.cpu().numpy(), wt, T, k)
    n = len(ids)
    tok = np.full((n, k, 3), -1, np.int64)
    rev, off = np.full((n, k), -1, np.int64), np.full((n, k), -1, np.int64)
    for a, o in enumerate(ids):
        begin, end = pool.rev_off[pool.first[o]], pool.rev_off[pool.first[o + 1]]
        for b in range(k):
            p = int(pos[a, b])
            if p < 0:
                continue
            for j in range(3):
                t = p - 2 + j
                if 0 <= t < T:
                    tok[a, b, j] = pool.tok[begin + t] if begin + t < end else 0
            g = begin + max(p - 2, 0)
            if g < end:
                r = [r for r in range(pool.first[o], pool.first[o + 1]) if pool.rev_off[r] <= g < pool.rev_off[r + 1]]
                assert len(r) == 1
                rev[a, b], off[a, b] = r[0], g - pool.rev_off[r[0]]
    return dict(positions=pos, scores=score, filters=filt, tokens=tok, reviews=rev, offsets=off, windows=win)


def recompute_narre(cat, side, ids, k):
    """The host recomputation, NARRE's layout: one row per (owner, slot) -> arrays [n, R, ...]."""
    from reviews4rec_amd import ops
    from reviews4rec_amd.data import _np_reviews
    pool, tower, _ = cat._phrase_side(side)
    R, W = int(cat.hp['narre_num_reviews']), int(cat.hp['narre_num_words'])
    none = np.full(len(ids), -1, np.int64)
    docs = _np_reviews(pool.tok, pool.rev_off, pool.first[ids], pool.first[ids + 1], none, R, W).reshape(len(ids) * R, W)
    conv = tower.convs[0]
    with torch.no_grad():
        pooled, argmax = ops.textcnn_fwd_raw(torch.from_numpy(docs).to(DEV), cat._words(), conv.weight.detach(),
                                             conv.bias.detach())
    pos, score, filt, win = phrases_ref(pooled.cpu().numpy(), argmax.cpu().numpy(), None, W, k)
    n = len(ids)
    pos, score, filt, win = pos.reshape(n, R, k), score.reshape(n, R, k), filt.reshape(n, R, k), win.reshape(n, R)
    tok = np.full((n, R, k, 3), -1, np.int64)
    rev, off = np.full((n, R, k), -1, np.int64), np.full((n, R, k), -1, np.int64)
    for a, o in enumerate(ids):
        count = pool.first[o + 1] - pool.first[o]
        for s in range(R):
            r = pool.first[o] + s
            length = min(pool.rev_off[r + 1] - pool.rev_off[r], W) if s < count else 0
            for b in range(k):
                p = int(pos[a, s, b])
                if p < 0:
                    continue
                for j in range(3):
                    t = p - 2 + j
                    if 0 <= t < W:
                        tok[a, s, b, j] = pool.tok[pool.rev_off[r] + t] if t < length else 0
                if max(p - 2, 0) < length:
                    rev[a, s, b], off[a, s, b] = r, max(p - 2, 0)
    return dict(positions=pos, scores=score, filters=filt, tokens=tok, reviews=rev, offsets=off, windows=win)


def against(phr, want, what):
    for name in FIELDS:
        got, ref = getattr(phr, name).cpu().numpy(), want[name]
        if name == 'scores':
            got, ref = bits(got), bits(ref)
        assert got.dtype == ref.dtype and got.shape == ref.shape, (what, name, got.dtype, got.shape)
        assert np.array_equal(got, ref), (what, name)


# ---------------------------------------------------------------- the document families
@pytest.mark.parametrize('mt', ['deepconn', 'deepconn++', 'transnet++'])
def test_explain_words_of_every_item_and_user_on_tiny(mt, tmp_path, monkeypatch):
    from reviews4rec_amd import Phrases
    host, dev, hp = _catalogues(mt, tmp_path, monkeypatch)
    T = int(hp['input_length'])
    for side in ('item', 'user'):
        pool, tower, _ = host._phrase_side(side)
        if mt == 'transnet++':
            assert tower is getattr(host.model.source, side + '_conv')           # the towers that score at test time
        total = pool.owners
        ids = np.arange(total, dtype=np.int64)
        p = host.explain_words(ids, k=K, side=side)
        assert isinstance(p, Phrases) and p.slots is None and p.weights is None
        for t, dt, shape in ((p.positions, torch.int32, (total, K)), (p.scores, torch.float32, (total, K)),
                             (p.filters, torch.int32, (total, K)), (p.tokens, torch.int64, (total, K, 3)),
                             (p.reviews, torch.int64, (total, K)), (p.offsets, torch.int64, (total, K)),
                             (p.windows, torch.int32, (total,))):
            assert t.device.type == 'cuda' and t.dtype == dt and tuple(t.shape) == shape
        against(p, recompute(host, side, ids, K), (mt, side))
        # real phrases: words of the pool, inside the owner's own reviews
        pos, rev, tok = p.positions.cpu().numpy(), p.reviews.cpu().numpy(), p.tokens.cpu().numpy()
        assert (pos[:-1, 0] >= 0).all() and (rev[:-1] >= 0).any() and tok.max() > 0
        held = rev >= 0
        assert (rev[held] >= pool.first[ids][:, None].repeat(K, 1)[held]).all()
        assert (rev[held] < pool.first[ids + 1][:, None].repeat(K, 1)[held]).all()
        # the owner without a review: a document of pad words -- windows there may be (the conv's bias), reviews not
        assert (rev[-1] == -1).all() and (p.offsets[-1] == -1).all() and set(tok[-1].reshape(-1).tolist()) <= {0, -1}
        listed = pos[-1] >= 0
        for b in np.nonzero(listed)[0]:
            assert tok[-1, b].tolist() == [0 if 0 <= pos[-1, b] - 2 + j < T else -1 for j in range(3)]
        assert (tok[-1][~listed] == -1).all()
        # towers='device', another chunking: the same bits
        same(p, dev.explain_words(ids, k=K, side=side), (mt, side, 'device'))
        # ids as a device tensor, out of order and repeated; another k is the head of the list
        pick = torch.tensor([total - 1, 0, 3, 0], device=DEV)
        for cat in (host, dev):
            q = cat.explain_words(pick, k=2, side=side)
            for name in FIELDS[:6]:
                assert torch.equal(getattr(q, name), getattr(p, name)[pick][:, :2]), name
            assert torch.equal(q.windows, p.windows[pick])
        # weights: 'latent' is the column norms passed explicitly, for both paths; per-owner rows weigh their own owner
        norms = tower.fc.weight.detach().norm(dim=0)
        lat = host.explain_words(ids, k=K, side=side, weights='latent')
        same(lat, host.explain_words(ids, k=K, side=side, weights=norms), 'latent')
        same(lat, dev.explain_words(ids, k=K, side=side, weights='latent'), 'latent on the device')
        same(lat, dev.explain_words(ids, k=K, side=side, weights=norms[None, :].repeat(total, 1)), 'latent per owner')
        if side == 'item':                                    # ... and the exactly rounded fma chain on the host
            against(lat, recompute(host, side, ids, K, wt=norms.cpu().numpy()), (mt, 'latent'))
        rows = torch.randn((total, norms.numel()), generator=torch.Generator().manual_seed(4)).to(DEV)
        mine = host.explain_words(ids, k=K, side=side, weights=rows)
        same(mine, dev.explain_words(ids, k=K, side=side, weights=rows), 'per owner on the device')
        alone = host.explain_words(ids[5:6], k=K, side=side, weights=rows[5])
        assert torch.equal(alone.positions[0], mine.positions[5]) and torch.equal(alone.scores[0], mine.scores[5])
    with pytest.raises(ValueError):
        host.explain_words([0], k=101)
    with pytest.raises(KeyError):
        host.explain_words([10 ** 6])
    assert host.explain_words([], k=3).positions.shape == (0, 3) and dev.explain_words([], k=3).tokens.shape == (0, 3, 3)


# ---------------------------------------------------------------- NARRE: a list per review
def test_narre_explain_words_per_review_on_tiny(tmp_path, monkeypatch):
    host, dev, hp = _catalogues('NARRE', tmp_path, monkeypatch)
    R, W = int(hp['narre_num_reviews']), int(hp['narre_num_words'])
    for side in ('item', 'user'):
        pool, tower, _ = host._phrase_side(side)
        total = pool.owners
        ids = np.arange(total, dtype=np.int64)
        p = host.explain_words(ids, k=K, side=side)
        assert tuple(p.positions.shape) == (total, R, K) and tuple(p.tokens.shape) == (total, R, K, 3)
        assert tuple(p.windows.shape) == (total, R) and p.slots is None and p.weights is None
        against(p, recompute_narre(host, side, ids, K), side)
        rev = p.reviews.cpu().numpy()
        count = np.minimum(pool.first[ids + 1] - pool.first[ids], R)
        for a in range(total):
            assert (rev[a, count[a]:] == -1).all()                               # a padded slot holds no review
            held = rev[a, :count[a]]
            assert ((held == -1) | (held == (pool.first[a] + np.arange(count[a]))[:, None])).all()
        assert (rev >= 0).any() and (rev[-1] == -1).all() and set(p.tokens[-1].reshape(-1).tolist()) <= {0, -1}
        same(p, dev.explain_words(ids, k=K, side=side), (side, 'device'))
        norms = tower.fc.weight.detach().norm(dim=0)
        lat = host.explain_words(ids, k=K, side=side, weights='latent')
        same(lat, host.explain_words(ids, k=K, side=side, weights=norms), 'latent')
        same(lat, dev.explain_words(ids, k=K, side=side, weights=norms[None, :].repeat(total, 1)), 'latent per owner')
        # reviews=k_r: the rows of the slots explain lists, in its order, with its slots and weights alongside
        for cat in (host, dev):
            e = cat.explain(ids, k=3, side=side)
            q = cat.explain_words(ids, k=K, side=side, reviews=3)
            assert torch.equal(q.slots, e.slots) and torch.equal(q.weights.view(torch.int32), e.weights.view(torch.int32))
            assert tuple(q.positions.shape) == (total, 3, K) and tuple(q.tokens.shape) == (total, 3, K, 3)
            slots = e.slots.cpu().numpy()
            for name in FIELDS:
                got, full = getattr(q, name).cpu().numpy(), getattr(p, name).cpu().numpy()
                fill = {'positions': -1, 'tokens': -1, 'reviews': -1, 'offsets': -1}.get(name, 0)
                for a in range(total):
                    for s in range(3):
                        want = full[a, slots[a, s]] if slots[a, s] >= 0 else np.full_like(full[a, 0], fill)
                        assert np.array_equal(got[a, s].view(np.uint32) if got.dtype == np.float32 else got[a, s],
                                              want.view(np.uint32) if want.dtype == np.float32 else want), (name, a, s)
            assert (slots[-1] == -1).all() and (q.positions[-1] == -1).all()
    with pytest.raises(ValueError):
        host.explain_words([0], k=3, reviews=R + 1)


# ---------------------------------------------------------------- refusals
def test_families_without_a_tower_are_refused_with_the_reason(tmp_path):
    from reviews4rec_amd import Catalogue, ReluCatalogue
    from test_gpu_recommend import _tiny_model
    from test_gpu_relu_catalogue import _tiny as relu_tiny
    hp, train, _, model, _ = _tiny_model('MF_dot', tmp_path)
    with pytest.raises(RuntimeError, match="'MF_dot' has no TextCNN tower"):
        Catalogue(model, hp, train).explain_words([0], k=3)
    hp, train, _, model, _ = relu_tiny('NeuMF', 'NeuMF', tmp_path)
    with pytest.raises(RuntimeError, match="'NeuMF' has no TextCNN tower"):
        ReluCatalogue(model, hp, train).explain_words([0], k=3)


# ---------------------------------------------------------------- main.main
@pytest.mark.parametrize('towers', ['host', 'device'])
def test_main_writes_the_phrases_of_the_trained_model(towers, tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    meta, z = _fixture('deepconn', 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    hp = tiny_hp('deepconn', root, epochs=1, log_file=str(tmp_path / 'log'), model_path=str(tmp_path / 'model'),
                 explain_words_k=K, explain_words_path=str(tmp_path / 'words.npz'), catalogue_towers=towers)
    M.main(hp)
    assert 'words.npz' in os.listdir(str(tmp_path))
    state = torch.load(hp['model_path'], map_location='cpu')
    train, _, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class('deepconn')(hp)
    model.load_state_dict(state)
    f = np.load(str(tmp_path / 'words.npz'))
    assert set(f.files) == {'items', 'positions', 'scores', 'filters', 'tokens', 'reviews', 'offsets'}
    cat = Catalogue(model.cuda().eval(), hp, train)
    assert np.array_equal(f['items'], cat.eligible) and len(cat.eligible) > 3
    p = cat.explain_words(cat.eligible, k=K)
    for name in f.files[1:]:
        got, want = f[name], getattr(p, name).cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(bits(got) if name == 'scores' else got,
                                                          bits(want) if name == 'scores' else want), name
    assert (f['positions'][:, 0] >= 0).all() and (f['reviews'] >= 0).any()
