"""Scoring spans (include/r4r.h "Scoring spans": r4r_*_span_score, r4r_rank_top1; engine._Spans.score_split;
data.DataLoader.score_descriptor; eval.evaluate / eval.eval_ranking on top of them): a validation or ranking pass whose
launches are enqueued from C must give EXACTLY what the per-launch loop gives at the same launch size -- the same
kernels with the same arguments, so the same bits per score -- and must leave the engine's training state where that
loop leaves it.

The loops these replace: the reference's eval.py:24-40 and eval.py:64-78 over data.py:250-447.

Bits are promised per launch size n only: the conv rule may pick another algorithm for another n."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp
from test_gpu_span import FAMILIES, hyper, same, tiny_corpus

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REVIEW = ('deepconn', 'deepconn++', 'NARRE', 'transnet', 'transnet++')
B = 16
N = 1520                                                     # 95 launches of 16: more than SPAN_STEPS = 64 per pass


def ranking_rows(corpus, items=120, seed=7):
    """negs in the reference's schema (make_negative_sets.py:83): user -> [[positive, ...], five negatives]; the positive
    is one of the user's training items (data.py:217 looks its review indices up)."""
    rng = np.random.default_rng(seed)
    first = {}
    for u, i, _ in corpus['train']:
        first.setdefault(u, i)
    # (negatives other than the positive itself, as make_negative_sets.py draws them: the same item scores the same)
    return {u: [[i], ((i + rng.integers(1, items, 5)) % items).tolist()] for u, i in first.items()}


def build(mt, corpus, negs=None, **kw):
    import reviews4rec_amd
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.utils import xavier_init
    hp = hyper(mt, **dict(dict(batch_size=B), **kw))
    reader = DataLoader(hp, corpus['train'], corpus['user_reviews'], corpus['item_reviews'], negs,
                        this_index_user_item=corpus['this_index_user_item'], device=DEV)
    torch.manual_seed(5)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    xavier_init(model)
    model = model.cuda()
    return hp, reader, model, M.make_engine(hp, model)


def per_launch(engine, reader, n, negs=False, review=False):
    """What the loops of eval.py compute today: engine.predict over the reader's slices of n ratings (n / 6 rows)."""
    pred, se, aux = [], [], []
    batches = reader.iter_negs(review, batch=n // 6) if negs else reader.iter(eval=True, batch=n)
    for data, y in batches:
        p, s = engine.predict(data, None if negs else y)
        pred.append(p.reshape(-1).clone())
        if not negs:
            se.append(s.reshape(-1).clone())
            if hasattr(engine, 'aux'):
                aux.append(engine.aux(data)[:, 1:3])
    return torch.cat(pred), (torch.cat(se) if se else None), (torch.cat(aux) if aux else None)


def top1_counts(scores):
    from reviews4rec_amd import _lib
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    rows, C = (int(s) for s in scores.shape)
    _lib.check(_lib.lib().r4r_rank_top1(_lib.ptr(scores), rows, C, _lib.ptr(counts), _lib.current_stream()), 'r4r_rank_top1')
    return [int(c) for c in counts.cpu()]


# ---------------------------------------------------------------- 1. bits
# batch_size | 8 x batch_size (a ragged tail of 112) | a ragged tail of 20 | larger than the split | an exact divisor
LAUNCHES = [B, 8 * B, 100, 2000, 80]


@pytest.mark.parametrize('mt', FAMILIES)
def test_scores_keep_the_bits_of_the_per_launch_loop(mt, monkeypatch):
    """Every launch size: score_split's pred / se (TransNet: aux) == the concatenation of predict over the reader's
    slices of the same n.  Groups of 64 ratings (4 launches of 16: the first and last launch of 23 ring groups, both
    ring slots rebuilt many times), 95 launches cut at SPAN_STEPS = 64, and once more at 5 per call."""
    from reviews4rec_amd.data import DataLoader
    monkeypatch.setattr(DataLoader, 'SPAN_RATINGS', 64)
    corpus = tiny_corpus(ratings=N, seed=41)
    hp, reader, model, engine = build(mt, corpus, dropout=0.0)
    model.eval()
    for n, steps in [(n, 64) for n in LAUNCHES] + [(B, 5)]:
        engine.SPAN_STEPS = steps
        desc = reader.score_descriptor(n)
        assert (desc.n_ratings, desc.batch_size, desc.full_batches) == (N, n, N // n)
        want = per_launch(engine, reader, n)
        got = engine.score_split(reader, desc)
        assert got is not None, 'no scoring-span form'
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), (mt, n, 'pred')
        assert torch.equal(got[1], want[1]), (mt, n, 'se')
        if mt.startswith('transnet'):
            assert torch.equal(got[2], want[2]), (mt, n, 'aux')
        else:
            assert got[2] is None
        if desc.review and n == B:
            assert desc.built.value == -(-(N // B) // 4) - 1           # every ring group was built, in order


@pytest.mark.parametrize('mt', FAMILIES)
def test_ranking_scores_keep_the_bits_of_the_per_launch_loop(mt, monkeypatch):
    """The negatives: six candidates per row, the POSITIVE item's overlap indices and reviewer list for all six
    (nb_item), no ratings.  Launches of 6 x 16 candidates (ragged tail), 6 x 2 (more than 64 launches, groups of 5
    launches), one larger than the rows."""
    from reviews4rec_amd.data import DataLoader
    monkeypatch.setattr(DataLoader, 'SPAN_RATINGS', 64)
    corpus = tiny_corpus(ratings=N, seed=42)
    negs = ranking_rows(corpus)
    hp, reader, model, engine = build(mt, corpus, negs=negs, dropout=0.0)
    model.eval()
    review = mt in REVIEW
    rows = len(negs)
    assert rows > 130
    for n in (6 * 16, 6 * 2, 6 * 1000):
        desc = reader.score_descriptor(n, negs=True, review=review)
        assert (desc.n_ratings, desc.full_batches) == (6 * rows, 6 * rows // n)
        want = per_launch(engine, reader, n, negs=True, review=review)
        got = engine.score_split(reader, desc)
        assert got is not None and got[1] is None and got[2] is None
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), (mt, n)


# ---------------------------------------------------------------- 2. metrics
def _tiny(mt, tmp_path):
    import reviews4rec_amd
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _counts, _fixture, _weights
    meta, z = _fixture(mt, 'eval')
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp(mt, root), device='cuda')
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(_weights(z), strict=True)
    model = model.cuda()
    return hp, test, model, M.make_engine(dict(hp, engine='native'), model), lambda: _counts(root)


def _check_metrics(hp, reader, model, engine, counts, review, sizes):
    from reviews4rec_amd.eval import evaluate, eval_ranking, _launch_size, RANK_LAUNCH
    from reviews4rec_amd.loss import MSELoss
    for size in sizes:
        got = {}
        for spans in (True, False):
            h = dict(hp, eval_spans=spans)
            if size:
                h['eval_batch_size'] = size
            uc, ic = counts()
            calls = []
            inner = engine.score_split
            engine.score_split = lambda *a, _inner=inner, **k: (calls.append(1), _inner(*a, **k))[1]
            try:
                got[spans] = evaluate(model, MSELoss(hp), reader, h, uc, ic, review, engine=engine) + \
                    (eval_ranking(model, reader, h, review, engine=engine), uc, ic)
            finally:
                del engine.score_split
            assert len(calls) == (2 if spans else 0)         # the switch decides the path
        on, off = got[True], got[False]
        print(hp['model_type'], size, on[0], off[0], on[3], off[3])
        assert set(on[0]) == set(off[0])
        for k in on[0]:
            # one unit of the reference's fourth rounded decimal: the two paths sum in different precision and order
            assert abs(on[0][k] - off[0][k]) <= 1e-4 + 1e-12, k
        assert on[1] == off[1] and list(on[1]) == list(off[1])             # count -> [SE] maps, list order included
        assert on[2] == off[2] and list(on[2]) == list(off[2])
        assert on[4] == off[4] and on[5] == off[5]                         # ids the maps entered with count 0
        ses = np.concatenate([np.asarray(v, np.float64) for v in on[1].values()])
        assert on[0]['MSE'] == round(float(ses.sum()) / len(ses), 4)
        assert on[3] == off[3]
        # the DEVICE count decided HR@1: no undecided row among these scores
        n = _launch_size(reader, dict(hp, **({'eval_batch_size': size} if size else {})), engine, RANK_LAUNCH)
        scores = engine.score_split(reader, reader.score_descriptor(6 * n, negs=True, review=review))[0].view(-1, 6)
        hits, undecided = top1_counts(scores)
        assert undecided == 0
        assert on[3] == {'HR@1': round(100.0 * hits / scores.shape[0], 2)}


@pytest.mark.parametrize('mt', ['deepconn', 'NARRE', 'MF_dot', 'transnet++'])
def test_evaluate_and_ranking_with_spans_on_and_off_tiny(mt, tmp_path):
    hp, test, model, engine, counts = _tiny(mt, tmp_path)
    _check_metrics(hp, test, model, engine, counts, mt in REVIEW + ('transnet++',), [None, hp['batch_size'], 7])


@pytest.mark.parametrize('mt', FAMILIES)
def test_evaluate_and_ranking_with_spans_on_and_off_synthetic(mt):
    """1,527 ratings (a ragged reference slice: TransNet's means of per-slice means), 300 ranking rows; seed 43: the
    spans-off scores have no tied positive (asserted through the device count's undecided == 0)."""
    corpus = tiny_corpus(ratings=N + 7, seed=43)
    hp, reader, model, engine = build(mt, corpus, negs=ranking_rows(corpus), dropout=0.0)
    gen = torch.Generator().manual_seed(43)
    with torch.no_grad():                                    # (xavier_init leaves the biases zero: bias_only would score
        for k, p in model.named_parameters():                #  every candidate alike)
            if 'word2vec' not in k:
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).to(p.device))
    _check_metrics(hp, reader, model, engine, lambda: ({}, {}), mt in REVIEW, [None, B, 100])


# ---------------------------------------------------------------- 3. ties
def _top1_numpy(s):
    pos, rest = s[:, 0], s[:, 1:]
    nan = np.isnan(s).any(axis=1)
    with np.errstate(invalid='ignore'):
        best = np.fmax.reduce(rest, axis=1)
        hit = ~nan & (pos > best)
        und = nan | (pos == best)
    return [int(hit.sum()), int(und.sum())]


@pytest.mark.parametrize('C', [2, 6, 64])
@pytest.mark.parametrize('rows', [0, 1, 63, 64, 65, 100003])
def test_rank_top1_against_numpy(rows, C):
    rng = np.random.default_rng(rows * 131 + C)
    s = rng.integers(-3, 4, size=(rows, C)).astype(np.float32) + rng.random((rows, C), dtype=np.float32) * (rng.random((rows, 1)) < 0.5)
    if rows:
        k = rng.integers(0, rows, size=max(1, rows // 5))
        s[k, 0] = s[k, 1:].max(axis=1)                                  # planted ties: positive == best negative
        k = rng.integers(0, rows, size=max(1, rows // 7))
        s[k, 0] = s[k, 1:].max(axis=1) + 1.0                             # clear hits
        if C > 2:
            k = rng.integers(0, rows, size=max(1, rows // 6))
            s[k, 1] = s[k, 2] = np.abs(s[k]).max(axis=1) + 1.0            # the maximum duplicated among the negatives only: decided
        k = rng.integers(0, rows, size=rows // 9)
        s[k, rng.integers(0, C, size=len(k))] = np.nan
        if rows > 70:
            s[70, 0] = np.nan                                           # a NaN positive
            s[69] = np.inf                                              # every column +inf: a tie
    want = _top1_numpy(s)
    t = torch.from_numpy(s).to(DEV)
    assert top1_counts(t) == want
    if rows > 1 and (rows * C) % 2 == 0:                                # a base that is only 4-byte aligned
        flat = torch.empty(rows * C + 1, dtype=torch.float32, device=DEV)
        flat[1:].copy_(t.view(-1))
        assert top1_counts(flat[1:].view(rows, C)) == want
    counts = torch.tensor([5, 7], dtype=torch.int64, device=DEV)        # counts accumulate
    from reviews4rec_amd import _lib
    _lib.check(_lib.lib().r4r_rank_top1(_lib.ptr(t), rows, C, _lib.ptr(counts), _lib.current_stream()), 'r4r_rank_top1')
    assert [int(c) for c in counts.cpu()] == [5 + want[0], 7 + want[1]]


@pytest.mark.parametrize('mt', ['MF_dot', 'deepconn'])
def test_all_scores_coincide_every_row_goes_to_the_host(mt):
    """Every parameter zero: all six scores of a row coincide, every row is undecided, eval_ranking takes the host
    torch.topk and returns what the per-launch path returns."""
    from reviews4rec_amd.eval import eval_ranking
    corpus = tiny_corpus(ratings=N, seed=44)
    negs = ranking_rows(corpus)
    hp, reader, model, engine = build(mt, corpus, negs=negs, dropout=0.0)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if 'word2vec' not in k:
                p.zero_()
    review = mt in REVIEW
    scores = engine.score_split(reader, reader.score_descriptor(6 * 64, negs=True, review=review))[0].view(-1, 6)
    assert top1_counts(scores) == [0, len(negs)]
    on = eval_ranking(model, reader, dict(hp, eval_spans=True), review, engine=engine)
    off = eval_ranking(model, reader, dict(hp, eval_spans=False), review, engine=engine)
    assert on == off


def test_zero_ranking_rows_still_raise():
    from reviews4rec_amd.eval import eval_ranking
    corpus = tiny_corpus(ratings=200, seed=45)
    hp, reader, model, engine = build('MF_dot', corpus, negs={})
    with pytest.raises(ZeroDivisionError):
        eval_ranking(model, reader, hp, False, engine=engine)


# ---------------------------------------------------------------- 4. state
def _snapshot(model, engine):
    sd = copy.deepcopy(engine.state_dict())                  # (flushes pending sweeps: the tables as a reader sees them)
    torch.cuda.synchronize()
    return dict(weights={k: v.detach().clone() for k, v in model.state_dict().items()}, opt=sd,
                step=engine.step_count, offset=engine.offset, sse=engine.sse.clone())


def _sequence(mt, corpus, negs, scoring, eval_n, K=5):
    """K training steps (a span; the last one announces its successor), a scoring pass over both kinds of split, K more,
    then one whole epoch.  scoring: True (spans), False (the per-launch predict loop), None (no scoring at all)."""
    from reviews4rec_amd import main as M
    from reviews4rec_amd.eval import evaluate, eval_ranking
    from reviews4rec_amd.loss import MSELoss
    hp, reader, model, engine = build(mt, corpus, negs=negs, dropout=0.5)
    if mt in REVIEW:
        engine.conv_algo = 2                                 # the projection: the algorithm with token state, no probes
    model.train()
    desc = reader.span_descriptor()
    engine._span(desc, 0, K, True)
    scored = None
    if scoring is not None:
        h = dict(hp, eval_spans=scoring, eval_batch_size=eval_n)
        scored = (evaluate(model, MSELoss(hp), reader, h, {}, {}, mt in REVIEW, engine=engine),
                  eval_ranking(model, reader, h, mt in REVIEW, engine=engine))
        model.train()
    engine._span(desc, K, K, False)
    mid = _snapshot(model, engine)
    metric = M.train(model, MSELoss(hp), None, reader, hp, engine=engine)
    return mid, _snapshot(model, engine), metric, scored


@pytest.mark.parametrize('eval_n', [B, 8 * B])
@pytest.mark.parametrize('mt', FAMILIES)
def test_a_scoring_pass_leaves_the_training_state_of_the_predict_loop(mt, eval_n):
    """eval_n = batch_size: the scoring launches share the training workspace, and for the projecting families the
    fifth step's announced batch is pending when the pass starts; K = 5 leaves the temporally blocked sweeps (period 8)
    mid-period.  (a) against the per-launch loop: everything, the next epoch included; (b) against no scoring at all:
    every parameter and moment."""
    corpus = tiny_corpus(ratings=N, seed=46)
    negs = ranking_rows(corpus)
    on = _sequence(mt, corpus, negs, True, eval_n)
    off = _sequence(mt, corpus, negs, False, eval_n)
    none = _sequence(mt, corpus, negs, None, eval_n)
    same(on[0], off[0], 'after 2K steps')
    same(on[1], off[1], 'after the next epoch')
    assert on[2] == off[2]
    assert on[3][1] == off[3][1]
    same(on[0]['weights'], none[0]['weights'], 'weights against no scoring')
    same(on[0]['opt'], none[0]['opt'], 'optimiser state against no scoring')
    assert on[0]['step'] == none[0]['step'] == 10 and on[0]['offset'] == none[0]['offset']
