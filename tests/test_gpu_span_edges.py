"""Spans (csrc/span.hip, engine._Spans) at the loader's edges.  tests/test_gpu_span.py holds the span path to the
per-step loop at one configuration per family (B = 32, G = 32: the ring's two slots are each built once per epoch);
here the same contract -- an epoch through spans leaves the bits of main.train's per-step loop: weights, Adam moments,
step count, epoch metric -- is asserted where the span path differs from that configuration:

- ring geometry: groups of G = 1, 2, 3 batches, so spans start, end and announce across group boundaries and every
  slot of the two-group ring is rebuilt many times per epoch (the ordering argument in the header of csrc/span.hip);
- shapes through the loader (word sizes, latent sizes, NARRE's review geometry, a vocabulary past 262,144), batches
  past the ID steps' 2,048-rating scan and NARRE's 4,096-entry fused launch, and the cases that must fall back;
- NARRE with R != 10 (the ring holds NEIGHBOURS = 10 ids per rating): refused the same way with spans on or off;
- the fp16-split GEMM (no spans: main.train's loop with next_data), an epoch interrupted with a batch announced;
- and, since bit-equality with the per-step loop cannot see a fault both paths share, one short epoch per family
  through main.train with spans on against the float64 CPU oracle replaying the loader's batches.

The loop the spans replace: the reference's main.py:23-60 over data.py:250-372."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_span import build, run_epochs, same, tiny_corpus

pytestmark = pytest.mark.gpu


def zipf_corpus(ratings, users, items, vocab=400, seed=21, words=(3, 40)):
    """tiny_corpus's schema with room for tens of thousands of distinct (user, item) pairs: half the ids from a zipf
    head (a few rows named by a large share of every batch), half uniform."""
    rng = np.random.default_rng(seed)

    def ids(n, count):
        return np.where(rng.random(n) < 0.5, rng.zipf(1.3, n) % count, rng.integers(0, count, n))

    pairs = np.empty((0, 2), np.int64)
    while len(pairs) < ratings:
        cand = np.concatenate([pairs, np.stack([ids(2 * ratings, users), ids(2 * ratings, items)], 1)])
        _, first = np.unique(cand[:, 0] * items + cand[:, 1], return_index=True)
        pairs = cand[np.sort(first)]
    user_reviews = {u: [] for u in range(users)}
    item_reviews = {i: [] for i in range(items)}
    tiui, train = {}, []
    for u, i in pairs[:ratings].tolist():
        rev = rng.integers(1, vocab, size=int(rng.integers(*words))).tolist()
        tiui.setdefault(u, {})[i] = [len(user_reviews[u]), len(item_reviews[i])]
        user_reviews[u].append(rev)
        item_reviews[i].append(rev)
        train.append([u, i, float(rng.integers(1, 6))])
    return dict(train=train, user_reviews=user_reviews, item_reviews=item_reviews, this_index_user_item=tiui)


def model_kw(mt):
    kw = {}
    if '/' in mt:
        mt, kw['neumf_stage'] = mt.split('/')
    return mt, kw


def conv(algo):
    def setup(engine):
        engine.conv_algo = algo                              # (R4R_CONV_ALGO is read once per process)
    return setup


def check_same(mt, corpus, span_steps, spanned, setup=None, epochs=2, **kw):
    """Spans on against spans off; `spanned`: the epoch must (True) or must not (False) go through the span entry."""
    want_m, want_w, want_o, _, want_e = run_epochs(mt, corpus, spans=False, epochs=epochs, setup=setup, **kw)
    got_m, got_w, got_o, calls, got_e = run_epochs(mt, corpus, spans=True, epochs=epochs, span_steps=span_steps,
                                                   setup=setup, **kw)
    if spanned:
        assert calls['span'] > 0, calls
    else:
        assert calls['span'] == 0, calls
    assert got_m == want_m
    same(got_w, want_w, 'weights')
    same(got_o, want_o, 'optimiser state')
    n, B = len(corpus['train']), int(kw.get('batch_size', 32))
    assert got_e.step_count == want_e.step_count == epochs * -(-n // B)
    return calls


# ---------------------------------------------------------------- ring geometry
RING = [(mt, G, algo) for mt in ('deepconn', 'NARRE', 'transnet++') for G in (1, 2, 3) for algo in (1, 2)]
RING += [('deepconn++', 2, 2), ('transnet', 2, 1)]


@pytest.mark.parametrize('mt,G,algo', RING)
def test_ring_slots_are_rebuilt_in_order(mt, G, algo, monkeypatch):
    """G = 1 .. 3 batches per group (1,500 ratings, B = 32: 16 .. 46 groups an epoch), spans of 5 steps: a span starts,
    ends and announces its successor inside a group and across every kind of boundary, and group g is built into slot
    g & 1 while the previous group's last steps are still enqueued before it.  Dropout 0.5: the masks advance per step."""
    from reviews4rec_amd.data import DataLoader
    monkeypatch.setattr(DataLoader, 'SPAN_RATINGS', G * 32)
    calls = check_same(mt, tiny_corpus(seed=20 + G), 5, True, setup=conv(algo))
    assert calls['built'] >= 2, calls                        # group 2 went into group 0's slot
    assert calls['span'] >= 2 * (46 // 5), calls


# ---------------------------------------------------------------- shapes through the loader
SHAPES = [
    ('deepconn', dict(word_embed_size=50, latent_size=24), True, 0),
    ('deepconn', dict(word_embed_size=50, latent_size=32), True, 0),
    ('deepconn', dict(word_embed_size=768, input_length=200), True, 0),                # the multi-pass weight gradient
    ('deepconn', dict(vocab=262200, total_words=262200), True, 2),                      # the large-vocabulary compaction
    ('NARRE', dict(latent_size=32), True, 0),
    ('NARRE', dict(narre_num_words=1), True, 0),
    ('NARRE', dict(narre_num_words=33), True, 0),
    ('NARRE', dict(latent_size=33), False, 0),                                         # train_step's split form
    ('deepconn++', dict(latent_size=64, word_embed_size=50), True, 0),
    ('transnet', dict(latent_size=64, word_embed_size=50), True, 0),
]


@pytest.mark.parametrize('mt,kw,spanned,algo', SHAPES, ids=lambda v: str(v) if not isinstance(v, dict) else
                         '-'.join('%s%s' % (k[:5], x) for k, x in v.items()))
def test_shapes_through_the_loader(mt, kw, spanned, algo):
    corpus = tiny_corpus(seed=30, vocab=int(kw.get('vocab', 400)))
    check_same(mt, corpus, 9, spanned, setup=conv(algo) if algo else None, **kw)


# ---------------------------------------------------------------- batches
BATCHES = [('MF_dot', B) for B in (2048, 2049, 5000)] + [('bias_only', B) for B in (2048, 2049, 5000)]
BATCHES += [('MF', 2500), ('NeuMF/NeuMF', 2500), ('transnet++', 2500)]


@pytest.mark.parametrize('mt,B', BATCHES)
def test_large_batches_through_spans(mt, B):
    """Past the ID steps' 2,048-rating scan, with popular rows (a zipf head: one row is named by hundreds of ratings of
    every batch); transnet++: its temporally blocked sweep's schedule crosses the span boundaries.  Three full batches
    and a ragged tail, spans of two steps."""
    mt, kw = model_kw(mt)
    users, items = 4000, 1500
    corpus = zipf_corpus(3 * B + B // 3, users, items, seed=B, words=(3, 40) if mt == 'transnet++' else (3, 4))
    check_same(mt, corpus, 2, True, batch_size=B, total_users=users, total_items=items, **kw)


@pytest.mark.parametrize('B,spanned', [(372, True), (373, False)])
def test_narre_batch_at_the_fused_entry_limit(B, spanned):
    """B (1 + R) ID entries: 4,092 fit the fused launch's 4,096 (spans); 4,103 do not (train_step's split form)."""
    check_same('NARRE', tiny_corpus(ratings=3 * B + 50, seed=33), 2, spanned, batch_size=B)


# ---------------------------------------------------------------- NARRE with R != 10
@pytest.mark.parametrize('R', [5, 12, 32])
def test_narre_with_r_other_than_ten_is_refused_with_spans_on_or_off(R):
    """The loader's neighbour lists are 10 wide (data.py NEIGHBOURS; NARRE.py concatenates R review vectors with those
    10 embeddings, so the reference cannot train R != 10 either): main.train raises train_step's error either way and
    leaves the model, the optimiser state and the step count as they were."""
    from reviews4rec_amd import main as M
    from reviews4rec_amd.loss import MSELoss
    corpus = tiny_corpus(seed=34)
    errors = {}
    for spans in (False, True):
        hp, reader, model, engine = build('NARRE', corpus, narre_num_reviews=R, spans=spans)
        desc = reader.span_descriptor()
        assert desc.doc_shape[0] == R and not engine._span_ok(desc)
        weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
        opt = copy.deepcopy(engine.state_dict())
        with pytest.raises(RuntimeError) as err:
            M.train(model, MSELoss(hp), None, reader, hp, engine=engine)
        torch.cuda.synchronize()
        errors[spans] = str(err.value)
        same({k: v.detach() for k, v in model.state_dict().items()}, weights, 'weights')
        same(engine.state_dict(), opt, 'optimiser state')
        assert engine.step_count == 0
    assert errors[True] == errors[False] and '10 neighbour ids for %d reviews' % R in errors[True], errors


# ---------------------------------------------------------------- the fp16-split GEMM
@pytest.fixture
def f16x2(monkeypatch):
    from reviews4rec_amd import engine as E
    monkeypatch.setenv('R4R_GEMM_MATH', 'f16x2')
    yield
    monkeypatch.setenv('R4R_GEMM_MATH', 'f32')
    E.apply_gemm_math(None)                                  # the process-wide math back to fp32
    E._MATH_OWNER[0] = None


@pytest.mark.parametrize('mt', ['deepconn', 'NARRE'])
def test_fp16_split_gemm_keeps_the_announcing_loop(mt, f16x2):
    """R4R_GEMM_MATH=f16x2 refreshes its scales between steps, so no span may carry its steps: main.train's own loop
    runs, and every step but an epoch's last is told the next batch (its token marks ride on that step)."""
    kw = dict(word_embed_size=64)
    calls = check_same(mt, tiny_corpus(seed=35), 7, False, setup=conv(2), **kw)
    assert calls['next'] == ([True] * 46 + [False]) * 2, calls['next']


# ---------------------------------------------------------------- an interrupted epoch
class _Interrupt(Exception):
    pass


@pytest.mark.parametrize('mt', ['deepconn', 'NARRE'])
def test_an_interrupted_epoch_leaves_the_bits_of_the_interrupted_loop(mt):
    """An exception after the third span (batches 10 .. 14, batch 15 announced: its token state is prepared from ring
    addresses, engine._RawPtr) against the per-step loop interrupted after batch 14 (batch 15 announced from the loader's
    tensors); then one complete epoch each.  The pending state is dropped (_discard_prepared) the same way in both."""
    from reviews4rec_amd import main as M
    from reviews4rec_amd.engine import _RawPtr
    from reviews4rec_amd.loss import MSELoss
    corpus = tiny_corpus(seed=36)
    got = {}
    for spans in (False, True):
        hp, reader, model, engine = build(mt, corpus, spans=spans)
        engine.conv_algo = 2                                 # the projection: the only algorithm with token state
        engine.SPAN_STEPS = 5
        name = '_span' if spans else 'train_step'
        inner, seen = getattr(engine, name), [0]

        def interrupting(*a, _inner=inner, _stop=3 if spans else 15, **k):
            out = _inner(*a, **k)
            seen[0] += 1
            if seen[0] == _stop:
                raise _Interrupt()
            return out
        setattr(engine, name, interrupting)
        with pytest.raises(_Interrupt):
            M.train(model, MSELoss(hp), None, reader, hp, engine=engine)
        assert engine.step_count == 15 and engine._prepared is not None
        if spans:
            assert all(isinstance(t, _RawPtr) for t in engine._prepared[-1])
        setattr(engine, name, inner)
        metric = M.train(model, MSELoss(hp), None, reader, hp, engine=engine)
        torch.cuda.synchronize()
        got[spans] = (metric, {k: v.detach().clone() for k, v in model.state_dict().items()}, engine.state_dict(),
                      engine.step_count)
    assert got[True][0] == got[False][0]
    same(got[True][1], got[False][1], 'weights')
    same(got[True][2], got[False][2], 'optimiser state')
    assert got[True][3] == got[False][3] == 15 + 47


# ---------------------------------------------------------------- the float64 oracle through the loader
ORACLE = [('deepconn', 1, 32), ('deepconn++', 2, 32), ('NARRE', 1, 32), ('transnet++', 2, 32), ('MF_dot', 1, 2049),
          ('NeuMF/NeuMF', 2, 64)]
WORDS = ('deepconn', 'deepconn++', 'NARRE', 'transnet++')


@pytest.mark.parametrize('mt,G,B', ORACLE)
def test_an_epoch_through_spans_follows_the_float64_oracle(mt, G, B, monkeypatch):
    """main.train, spans on, one epoch of 6 full batches and a ragged tail, against oracle.train_step (TransNet:
    oracle.transnet_train_step) in float64 on the CPU, replaying the batches reader.iter() yields: the final parameters
    at test_gpu_full_size's tolerances, the epoch metric (rounded by main.train to 4 decimals) to 1e-4."""
    import oracle
    from reviews4rec_amd.data import DataLoader
    from test_oracle_golden import ill_conditioned
    monkeypatch.setattr(DataLoader, 'SPAN_RATINGS', G * B)
    mt, kw = model_kw(mt)
    kw.update(batch_size=B, dropout=0.0)
    if mt in WORDS:
        kw.update(latent_size=24, word_embed_size=50)
    n = 6 * B + B // 2 + 1
    if B > 300:
        kw.update(total_users=3000, total_items=1000)
        corpus = zipf_corpus(n, 3000, 1000, seed=37, words=(3, 4))
    else:
        corpus = tiny_corpus(ratings=n, seed=37)
    hp, reader, model, _ = build(mt, corpus, **kw)           # (build is deterministic: run_epochs builds the same)
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batches = [([None if d is None else d.cpu() for d in data], y.cpu()) for data, y in reader.iter()]
    assert len(batches) == 7 and batches[-1][1].numel() < B
    metrics, got, _, calls, engine = run_epochs(mt, corpus, spans=True, epochs=1, span_steps=4, **kw)
    assert calls['span'] >= 2 and engine.step_count == 7, calls

    def replay(dtype):
        P = {k: v.to(dtype).clone() for k, v in init.items()}
        if mt.startswith('transnet'):
            states = dict(source=oracle.AdamState(), source_fm=oracle.AdamState(), target=oracle.AdamState())
            sse = sum(float(oracle.transnet_train_step(P, data, y.to(dtype), hp, states)[0].sum()) for data, y in batches)
        else:
            state = oracle.AdamState()
            sse = sum(oracle.train_step(P, data, y.to(dtype), hp, state)[0] for data, y in batches)
        return P, sse

    P, sse = replay(torch.float64)
    # (the same replay in float32 gives the entries whose trajectory fp32 rounding alone moves past the tolerance: a
    # gradient that is nearly zero -- a hidden unit of NARRE's scorer that is off for most reviews -- is normalised by
    # Adam into steps of up to lr, so its rounding noise is not small.  Two correct float32 implementations need not
    # agree there; they are left to the max-difference bound, and there must be few of them)
    P32, _ = replay(torch.float32)
    for k, v in P.items():
        if ill_conditioned(k):
            continue
        tol = 2e-5 + 1e-4 * v.abs()
        diff, noisy = (got[k].cpu().double() - v).abs(), (P32[k].double() - v).abs() > tol
        assert float(noisy.float().mean()) < 0.05, k
        assert float((diff[~noisy] > tol[~noisy]).float().mean()) < 2e-3, k
        assert float(diff.max()) < 2.5e-3, k
    torch.testing.assert_close(metrics[0]['MSE'], sse / n, rtol=1e-4, atol=5e-5)      # (atol: the rounding)
