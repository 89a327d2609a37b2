"""Slates through the five catalogue classes: Catalogue.recommend_among / rank_among (one r4r_slate_topk_<form> /
r4r_slate_rank_<form> call each) and eval.eval_sampled, on the weights each class's own test file builds (tests/golden/tiny;
MF: tests/golden/mf_full.npz).  The reference is the host sort / count over score_pairs' bits (test_gpu_slate.py's), with
no tolerance; with every user's slate = the eligible ids the results must be recommend's and rank's own."""
import numpy as np
import pytest
import torch

import test_gpu_mf_catalogue as PFM
import test_gpu_narre_catalogue as HMLP
import test_gpu_relu_catalogue as RELU
import test_gpu_transnet_catalogue as RFM
from test_gpu_recommend import _tiny_model
from test_gpu_slate import bits, ref_lists, ref_ranks

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CLASSES = ['Catalogue', 'ReluCatalogue', 'NarreCatalogue', 'TransNetCatalogue', 'MFCatalogue']


def build(name, tmp_path):
    """-> (catalogue, hyper_params, train, test) of one model per class."""
    import reviews4rec_amd
    if name == 'MFCatalogue':                                  # test_gpu_mf_catalogue.py's golden model and ratings
        from helpers import Golden
        gold = Golden('mf_full')
        hp = dict(gold.hp)
        U, I = hp['total_users'], hp['total_items']
        rng = np.random.default_rng(8)
        eligible = sorted(rng.permutation(I)[:15].tolist())
        rows = sorted({(int(rng.integers(0, U)), int(rng.choice(eligible))) for _ in range(90)})
        rows += [(0, i) for i in eligible if i not in {r[1] for r in rows}]
        train = PFM.Ratings([(u, i, 3.0) for u, i in rows])
        test = PFM.Ratings([(int(rng.integers(0, U)), int(rng.integers(0, I)), 4.0) for _ in range(40)])
        model = reviews4rec_amd.get_model_class('MF')(hp)
        model.load_state_dict(gold.params(), strict=True)
        model = model.cuda().eval()
    elif name == 'Catalogue':
        hp, train, test, model, _ = _tiny_model('MF_dot', tmp_path)
    elif name == 'ReluCatalogue':
        hp, train, test, model, _ = RELU._tiny('NeuMF', None, tmp_path)
    elif name == 'NarreCatalogue':
        hp, train, test, model, _ = HMLP._tiny(tmp_path)
    else:
        hp, train, test, model, _ = RFM._tiny('transnet++', tmp_path)
    return getattr(reviews4rec_amd, name)(model, hp, train), hp, train, test


def same(got, want, what):
    assert np.array_equal(got[0].cpu().numpy(), want[0]), what
    assert np.array_equal(bits(got[1].cpu().numpy()), bits(want[1])), what


@pytest.mark.parametrize('name', CLASSES)
def test_slates_through_the_class(name, tmp_path):
    from reviews4rec_amd import eval_sampled, ranking_metrics, sample_negatives
    cat, hp, train, test = build(name, tmp_path)
    U, n_c = cat.n_users, cat.n_c
    assert len(cat.eligible) >= 8
    # score_pairs' bits of every (user, candidate row) pair
    S = cat.score_pairs(np.repeat(np.arange(U), n_c), np.tile(np.arange(n_c), U)).cpu().numpy().reshape(U, n_c)
    el = np.zeros(n_c, bool)
    el[cat.eligible] = True
    assert np.isneginf(S[:, ~el]).all() and np.isfinite(S[:, el]).all()
    rng = np.random.default_rng(len(name))

    # (a) random slates, two per user and one user more often: a padded block; a user's training items among them
    users = np.concatenate([np.arange(U), rng.permutation(U), np.full(3, U // 2)])
    n = len(users)
    width = n_c + 3
    block = np.full((n, width), -1, np.int64)
    lists = []
    for r in range(n):
        l = rng.permutation(n_c)[:rng.integers(0, n_c + 1)].astype(np.int64)
        block[r, rng.permutation(width)[:len(l)]] = l          # (the padding anywhere in the row)
        lists.append(block[r][block[r] >= 0])
    lists[0], block[0] = lists[0][:0], -1                      # an empty slate
    items = rng.choice(cat.eligible, n)
    items[1] = np.nonzero(~el)[0][0] if (~el).any() else items[1]
    seen = cat.seen
    assert any(len(np.intersect1d(lists[r], seen[1][seen[0][users[r]]:seen[0][users[r] + 1]])) for r in range(n))
    for exclude in (True, False):
        excl = seen if exclude else None
        for k in (5, 128):
            got = cat.recommend_among(users, block, k=k, exclude_seen=exclude)
            assert got[0].shape == (n, k) and got[0].dtype == torch.int64 and got[1].dtype == torch.float32
            same(got, ref_lists(S, users, lists, k, excl), (name, 'lists', exclude, k))
        ranks, sc = cat.rank_among(users, items, block, exclude_seen=exclude)
        want = ref_ranks(S, users, items, lists, excl)
        assert np.array_equal(ranks.cpu().numpy(), want), (name, 'ranks', exclude)
        assert np.array_equal(bits(sc.cpu().numpy()), bits(S[users, items]))
        assert want[0] == 0 and (el.all() or want[1] == -1) and (want > 0).any()
    # a CSR, lists and device tensors are taken as well
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    a = cat.recommend_among(users.tolist(), (off, np.concatenate(lists)), k=5)
    b = cat.recommend_among(torch.from_numpy(users).to(DEV), torch.from_numpy(block).to(DEV), k=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    empty = cat.recommend_among([], np.zeros((0, 4), np.int64), k=3)
    assert empty[0].shape == (0, 3) and cat.rank_among([], [], ([0], []))[0].shape == (0,)
    with pytest.raises(ValueError):
        cat.recommend_among([0], [[1, 1]])
    with pytest.raises(ValueError):
        cat.recommend_among([0], [[n_c]])
    with pytest.raises(ValueError):
        cat.recommend_among([0, 1], [[1, 2]])

    # (b) every user's slate = the eligible ids: recommend's and rank's own results
    every = np.arange(U)
    whole = np.tile(cat.eligible, (U, 1))
    for exclude in (True, False):
        for k in (5, 128):
            want = cat.recommend(every, k=k, exclude_seen=exclude)
            got = cat.recommend_among(every, whole, k=k, exclude_seen=exclude)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, exclude, k)
        tu, ti = np.repeat(every, len(cat.eligible) + 1)[:4 * U], np.tile(np.arange(n_c), U)[:4 * U]
        want = cat.rank(tu, ti, exclude_seen=exclude)
        got = cat.rank_among(tu, ti, np.tile(cat.eligible, (len(tu), 1)), exclude_seen=exclude)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, exclude)

    # (c) eval_sampled == ranking_metrics over host counts on the same sample_negatives output
    data = np.asarray(test.data)
    tu, ti = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64)
    off, ids = sample_negatives(tu, ti, cat.eligible, cat.seen, 3, 1)
    negs = [ids[off[p]:off[p + 1]] for p in range(len(tu))]
    m = ranking_metrics(ref_ranks(S, tu, ti, negs), (1, 5, 10))
    want = {'samp_' + k: round(100.0 * v, 2) for k, v in m.items() if k not in ('ranked', 'unranked')}
    want.update(samp_ranked=m['ranked'], samp_unranked=m['unranked'], samp_short=int((np.diff(off) < 3).sum()))
    res = eval_sampled(cat.model, train, test, hp, n_negatives=3, seed=1, catalogue=cat)
    assert res == want, (res, want)
    assert res['samp_ranked'] + res['samp_unranked'] == len(tu) and res['samp_ranked'] > 0
    assert res['samp_HR@5'] == res['samp_HR@10'] == 100.0                                      # four candidates a row
    if name == 'Catalogue':                                    # ... and builds its own Catalogue when given none
        assert eval_sampled(cat.model, train, test, hp, n_negatives=3, seed=1) == want

    # (d) the dataset's own negatives (tests/golden/tiny): one ranked row per ranking user with an eligible positive
    if name != 'MFCatalogue':
        res = eval_sampled(cat.model, train, test, hp, ks=(1,), catalogue=cat, negatives='dataset')
        positives = [int(v[0][0]) for v in test.negs.values()]
        assert len(positives) > 0 and res['samp_ranked'] == sum(bool(el[p]) for p in positives) > 0
        assert res['samp_ranked'] + res['samp_unranked'] == len(positives)
        rows = [(int(u), int(v[0][0]), np.setdiff1d(np.unique(v[1]), [v[0][0]]).astype(np.int64)) for u, v in test.negs.items()]
        m = ranking_metrics(ref_ranks(S, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]), (1,))
        assert res['samp_HR@1'] == round(100.0 * m['HR@1'], 2) and res['samp_MRR'] == round(100.0 * m['MRR'], 2)


def test_a_recommend_among_pass_leaves_the_deepconn_training_state():
    """Train, re-rank, continue == training never interrupted: weights, moments, offset, step_count, bit for bit."""
    from reviews4rec_amd import Catalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build as build_engine, same as same_state, tiny_corpus
    corpus = tiny_corpus(seed=52)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build_engine('deepconn', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = Catalogue(model, hp, reader, engine=engine, tower_batch=50)
            slates = np.tile(cat.eligible[:40], (300, 1))
            items, sc = cat.recommend_among(np.arange(300), slates, k=10, exclude_seen=False)
            ranks, _ = cat.rank_among(np.arange(300), cat.eligible[np.arange(300) % len(cat.eligible)], slates)
            assert (items >= 0).all() and torch.isfinite(sc).all() and (ranks >= 0).all() and model.training
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same_state(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K
