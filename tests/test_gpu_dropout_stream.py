"""WHICH mask the device draws.  include/r4r.h gives every dropout draw a formula -- the native steps draw at
Philox4x32-10(seed, offset + b * ND + k), the stand-alone op r4r_dropout_fwd one 128-bit draw per four consecutive
elements at counter offset + i / 4, advancing by ceil(n / 4) -- and the train-mode parity tests (test_gpu_engine.py,
test_gpu_models.py, test_gpu_full_size.py, test_gpu_span.py) read the device's masks back and inject them into the CPU
oracle: they prove a mask is applied correctly, whatever it is.  Here every multiplier of every stream is compared with
tests/philox_ref.py (plain numpy from the algorithm's definition, held to the published known-answer vectors by
tests/test_philox_ref.py): the keep / drop pattern bit-equal over EVERY element, the kept value one and the same,
the host-side stream position after every step -- ragged batches, eval forwards in between, counters that carry into
the high word, seeds with a high word, spans, and the module path's consecutive sites."""
import functools
import math

import numpy as np
import pytest
import torch

import philox_ref as P
from helpers import multipliers

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def check_multipliers(mult, keep, p, what=''):
    """mult: the device's multipliers; keep: the reference's bool pattern, element for element.  Non-zero multipliers:
    one value, exactly 2.0 at p = 0.5, else within one float32 ulp of float32(1) / (float32(1) - float32(p)) (the
    slack is the device's divide)."""
    m = mult.detach().cpu().numpy().reshape(-1)
    assert m.dtype == np.float32 and m.shape == keep.shape, (what, m.dtype, m.shape, keep.shape)
    bad = np.flatnonzero((m != 0) != keep)
    assert bad.size == 0, '%s: %d of %d draws differ from the reference, first at %s' % (what, bad.size, m.size, bad[:8])
    kept = np.unique(m[keep])
    assert kept.size <= 1, (what, kept[:8])
    assert kept.size == 1 or not keep.any(), what
    if kept.size:
        want = P.scale(p)
        if p == 0.5:
            assert float(want) == 2.0 and float(kept[0]) == 2.0, (what, kept)
        else:
            assert abs(float(kept[0]) - float(want)) <= float(np.spacing(want)), (what, kept, want)


# ------------------------------------------------------------------ a. the stand-alone op
OP_SEED = 0xA5A5F00D12345678                                 # (a non-zero high word: k1)
OP_OFFSETS = [0, 2 ** 32 - 2, 2 ** 40 + 12345]


def _two_draws(ops, x1, x2, p):
    out = []
    for x in (x1, x2):
        ops.DropoutState.record = {}
        y = ops.dropout(x, p, True, 'site')
        out.append((y, ops.DropoutState.record['site']))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('offset', OP_OFFSETS)
@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 4097])
def test_op_stream(n, p, offset):
    """Two consecutive calls, position on the host and then in the device counter: element i of a call that starts at
    position `at` takes word i % 4 of counter at + i / 4; the call advances the position by ceil(n / 4)."""
    from reviews4rec_amd import ops
    S = ops.DropoutState
    saved = (S.seed, S.offset, S.record, S.device_counter)
    g = torch.Generator().manual_seed(n)
    x1, x2 = (torch.randn(n, generator=g).to(DEV) for _ in range(2))
    adv = (n + 3) // 4
    assert adv == math.ceil(n / 4)
    try:
        for mode in ('host', 'device'):
            S.seed, S.record = OP_SEED, None
            if mode == 'host':
                S.device_counter, S.offset = None, offset
            else:                                            # the position lives on the device; the host's is passed as 0
                S.device_counter, S.offset = torch.tensor([offset], dtype=torch.int64, device=DEV), 0
            draws = _two_draws(ops, x1, x2, p)
            for call, (x, (y, mult)) in enumerate(zip((x1, x2), draws)):
                what = '%s position, call %d' % (mode, call)
                check_multipliers(mult, P.op_keep(OP_SEED, offset + call * adv, n, p), p, what)
                assert torch.equal(y.view(torch.int32), (x * mult).view(torch.int32)), what      # bit for bit
            if mode == 'host':
                assert S.offset == offset + 2 * adv
            else:
                assert S.offset == 0
                assert int(S.device_counter.item()) == offset + 2 * adv
    finally:
        S.seed, S.offset, S.record, S.device_counter = saved


# ------------------------------------------------------------------ b. every native family, per-batch steps
B, RATINGS, L, R = 32, 1500, 8, 10                           # test_gpu_span.hyper's batch_size, latent_size, narre_num_reviews
D = L


def draws_per_rating(mt):
    """ND of include/r4r.h, written out: DeepCoNN 2L (the two towers' FC outputs), MF_dot 2D (user row, item row),
    NARRE 4RL + 3L, DeepCoNN++ 3L, TransNet(++) 5L + 10, and the ID-only networks (r4r_idnet_step; the engine's
    draws()): the gathered rows, 2L per table pair -- one pair, NeuMF two -- then the projection's 2L inputs where
    the variant has a projection (MF, MLP, NeuMF; GMF has none).  bias_only has no dropout site."""
    return {'deepconn': 2 * L, 'MF_dot': 2 * D, 'NARRE': 4 * R * L + 3 * L, 'deepconn++': 3 * L,
            'transnet': 5 * L + 10, 'transnet++': 5 * L + 10,
            'MF': 2 * L + 2 * L, 'NeuMF/GMF': 2 * L, 'NeuMF/MLP': 2 * L + 2 * L, 'NeuMF/NeuMF': 2 * (2 * L) + 2 * L,
            'bias_only': 0}[mt]


@functools.lru_cache(maxsize=None)
def corpus():
    """test_gpu_span's corpus: 1,500 ratings = 46 batches of 32 and a last one of 28.  Built once, never changed."""
    from test_gpu_span import tiny_corpus
    return tiny_corpus(ratings=RATINGS)


def build(mt, p):
    from test_gpu_span import build as span_build
    kw = {}
    name = mt
    if '/' in mt:
        name, kw['neumf_stage'] = mt.split('/')
    hp, reader, model, engine = span_build(name, corpus(), dropout=p, **kw)
    assert (hp['batch_size'], hp['latent_size'], hp['narre_num_reviews']) == (B, L, R)
    model.train()
    return hp, reader, model, engine


def run_sequence(mt, p, start=None):
    """Two training steps on full batches, an eval forward, a training step on the 28-rating batch, one more full
    batch.  Before each training step the position is `at`: draw k of rating b is the first word of counter
    at + b * ND + k, and the step leaves the position at at + n * ND."""
    hp, reader, model, engine = build(mt, p)
    ND = draws_per_rating(mt)
    if start is not None:
        engine.offset, engine.seed = start
    seed, at = engine.seed, engine.offset
    assert seed >> 32, 'the default seed exercises the high key word'
    last = (RATINGS - 1) // B
    for b in (0, 1, 'eval', last, 2):
        if b == 'eval':
            data, y = reader.batch(3)
            engine.predict(data, y)
            assert engine.offset == at, 'an eval forward moved the stream'
            continue
        data, y = reader.batch(b)
        n = int(y.numel())
        assert n == (RATINGS - last * B if b == last else B)
        engine.train_step(data, y)
        got = multipliers(engine, data)
        what = '%s p=%s batch %s (n=%d) at %d' % (mt, p, b, n, at)
        assert got.numel() == n * ND, what
        check_multipliers(got, P.engine_keep(seed, at, n * ND, p), p, what)
        at += n * ND
        assert engine.offset == at, what
    assert engine.seed == seed
    return engine


FAMILIES = ['deepconn', 'deepconn++', 'NARRE', 'transnet', 'transnet++', 'MF_dot', 'MF', 'NeuMF/GMF', 'NeuMF/MLP',
            'NeuMF/NeuMF']


@pytest.mark.parametrize('mt,p', [(mt, 0.5) for mt in FAMILIES] + [('deepconn', 0.2), ('NARRE', 0.2)])
def test_native_step_stream(mt, p):
    assert 28 == RATINGS - 46 * B
    run_sequence(mt, p)


# one per engine class (DeepCoNNEngine, MFEngine, the NarreEngine base, IdNetEngine): the carry into the counter's
# high word falls inside the first rating's draws (ND >= 12 > 7 for each), and the key's high word is not the default's
@pytest.mark.parametrize('mt', ['deepconn', 'MF_dot', 'NARRE', 'NeuMF/NeuMF'])
def test_native_step_stream_carries_into_the_high_word(mt):
    assert draws_per_rating(mt) > 7
    run_sequence(mt, 0.5, start=(2 ** 32 - 7, 0xFEDCBA9800000001))


def test_bias_only_draws_nothing():
    hp, reader, model, engine = build('bias_only', 0.5)
    for b in (0, 1):
        data, y = reader.batch(b)
        engine.train_step(data, y)
        assert engine.offset == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ c. through spans
@pytest.mark.parametrize('mt', ['deepconn', 'NARRE', 'MF_dot'])
def test_span_epoch_stream_position(mt):
    """test_gpu_span.py proves a span epoch leaves the bits of the per-step loop; this is the absolute position: after
    one epoch of 1,500 ratings the stream stands at 1500 ND, and the epoch's last step -- the 28-rating tail, which
    goes through train_step -- drew at (1500 - 28) ND."""
    from test_gpu_span import run_epochs
    ND = draws_per_rating(mt)
    seen = {}

    def setup(engine):
        inner = engine.train_step

        def keeping(data, y, *a, **k):
            seen['last'] = (data, engine.offset)
            return inner(data, y, *a, **k)
        engine.train_step = keeping
        assert engine.offset == 0

    _, _, _, calls, engine = run_epochs(mt, corpus(), spans=True, epochs=1, span_steps=7, setup=setup)
    assert calls['span'] >= 1, calls                         # the epoch really went through the span entry
    assert engine.offset == RATINGS * ND
    data, at = seen['last']
    assert int(data[5].numel()) == 28 and at == (RATINGS - 28) * ND
    got = multipliers(engine, data)
    assert got.numel() == 28 * ND
    check_multipliers(got, P.engine_keep(engine.seed, at, 28 * ND, 0.5), 0.5, mt + ' tail')


# ------------------------------------------------------------------ d. the module path's sites
@pytest.mark.parametrize('case', ['deepconnpp_e20', 'narre_e16'])
def test_module_path_sites_take_consecutive_counters(case):
    """One train-mode forward of the op-by-op path: site j (in the order the forward reached them) starts where site
    j - 1 stopped, sum_{i<j} ceil(n_i / 4) -- no two sites share a counter and none is skipped."""
    from helpers import Golden
    from reviews4rec_amd import ops
    from test_gpu_models import build_model
    S = ops.DropoutState
    saved = (S.seed, S.offset, S.record, S.device_counter)
    try:
        g = Golden(case)
        model, hp = build_model(g, dropout=0.5)
        model.train()
        S.device_counter = None
        S.manual_seed(3)
        seed = S.seed
        assert seed == (3 * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF and S.offset == 0
        S.record = {}
        data, _ = g.batch(0, DEV)
        model(data)
        torch.cuda.synchronize()
        sites = list(S.record.items())
        S.record = None
        assert len(sites) >= 3, [k for k, _ in sites]
        at = 0
        for name, mult in sites:
            n = mult.numel()
            check_multipliers(mult, P.op_keep(seed, at, n, 0.5), 0.5, '%s: site %s at %d' % (case, name, at))
            at += (n + 3) // 4
        assert S.offset == at                                # ... and no unrecorded draw in between
    finally:
        S.seed, S.offset, S.record, S.device_counter = saved
