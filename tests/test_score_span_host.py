"""Host side of the scoring spans (include/r4r.h "Scoring spans", csrc/span.hip, data.DataLoader.score_descriptor,
eval.evaluate's spanned path) where no GPU is needed: the descriptor arithmetic of both forms, every refusal (nothing
enqueued, launches_done = 0, a message), the host reductions of evaluate() from per-rating values against the
reference-generated Tiny fixtures, and the off switches.  The loops these replace: the reference's eval.py:24-40,
eval.py:64-78 over data.py:375-447."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import OracleModule, materialise_tiny, tiny_hp
from reviews4rec_amd import _lib
from test_span_host import FAKE, _desc, _ring, _span_call
from test_tiny_eval import EVAL_MODELS, MSE_TOL, _check_eval, _counts, _fixture, _weights

FAMILIES = ['deepconn', 'deepconnpp', 'narre', 'transnet', 'mf', 'idnet']


# ---------------------------------------------------------------- descriptors
def _loaders(mt, tmp_path):
    from reviews4rec_amd.data import load_data
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp(mt, root), device='cpu')
    return root, train, test, hp


@pytest.mark.parametrize('mt', ['deepconn', 'NARRE', 'MF_dot'])
def test_descriptor_arithmetic_of_both_forms(mt, tmp_path):
    """Built over host tensors here (nothing dereferences the words): N, n, group, stride, the y word; the negatives'
    six-fold expansion against iter_negs' own arrays."""
    from reviews4rec_amd.data import NEIGHBOURS, SpanDescriptor
    root, train, test, hp = _loaders(mt, tmp_path)
    review = mt != 'MF_dot'
    doc = (hp['narre_num_reviews'] * hp['narre_num_words']) if mt == 'NARRE' else hp['input_length']
    N = len(test.data)
    for n in (hp['batch_size'], 7, 8 * hp['batch_size'], 5000):
        d = SpanDescriptor(test, launch=n)
        assert (d.n_ratings, d.batch_size, d.full_batches, d.rated, d.nb_item) == (N, n, N // n, True, None)
        assert list(d.words[24:27]) == [N, d.group, n] and d.words[15] != 0 and d.words[27] == 0
        if review:
            assert d.group == max(1, test.SPAN_RATINGS // n)
            assert d.words[23] == d.group * n * (3 * doc + 2 * NEIGHBOURS) and d.ring.numel() == 2 * d.words[23]
            # the memory bound behind eval.EVAL_LAUNCH_CAP: a group is one launch, or SPAN_RATINGS ratings at most
            assert d.group * n <= max(n, test.SPAN_RATINGS)
        else:
            assert d.group == 1 and d.ring is None and d.words[22] == 0
    # the training descriptor is what it was
    t = SpanDescriptor(train)
    assert t.batch_size == hp['batch_size'] and t.full_batches == len(train.data) // hp['batch_size'] and t.words[15] != 0
    # negatives: the flattened candidates, each of iter_negs' per-row values six times, the positive as nb_item
    flat = test._device_negs(review)
    rows = len(test.negs)
    d = SpanDescriptor(test, launch=12, negs=flat, review=review)
    assert (d.n_ratings, d.batch_size, d.full_batches, d.rated) == (6 * rows, 12, 6 * rows // 12, False)
    assert d.words[15] == 0 and d.words[24] == 6 * rows and d.review == review
    us, cs, fields = [], [], []
    for data, y in test.iter_negs(review, batch=3):
        us.append(data[5].reshape(-1))
        cs.append(data[6].reshape(-1))
        fields.append(data[:5])
    assert torch.equal(flat['u'], torch.cat(us)) and torch.equal(flat['i'], torch.cat(cs))
    if review:
        assert d.nb_item is flat['nb_item']
        a = test._negs_arrays(True)
        for k in ('ku', 'ki', 'held'):
            assert np.array_equal(flat[k].numpy(), np.repeat(a[k], 6))
        assert np.array_equal(flat['nb_item'].numpy(), np.repeat(a['cand'][:, 0], 6))
        # ... and what the group build is handed reproduces iter_negs' documents and neighbour lists
        f = test._review_fields_host(flat['u'].numpy(), flat['i'].numpy(), flat['ku'].numpy(), flat['ki'].numpy(),
                                     flat['held'].numpy(), own_user_pos=flat['nb_item'].numpy())
        for s in range(5):
            want = torch.cat([x[s].reshape((-1,) + tuple(x[s].shape[2:])) for x in fields])
            assert np.array_equal(f[s], want.numpy()), s
    else:
        assert d.nb_item is None and set(flat) == {'u', 'i'}
    assert test.score_descriptor(12) is None                 # on the host there is nothing to enqueue


# ---------------------------------------------------------------- refusals
def _score_call(name, words, **over):
    """r4r_<name>_span_score with fake device pointers and real host out-parameters -> (rc, launches_done, error)."""
    lib, decl = _lib.lib(), _lib.parse_header()
    built, done = ctypes.c_int64(-1), ctypes.c_int64(7)
    rows = (ctypes.c_uint64 * 6)(*([FAKE] * 6))
    host = dict(loader=words, nb_item=None, built_group=ctypes.byref(built), launches_done=ctypes.byref(done),
                rows_p=rows, p=rows, stream=None)
    scalars = dict(first_launch=0, launches=2, V=400, n_users=300, n_items=120, ws_bytes=1 << 20, E=16, L=8, D=8,
                   T=64, R=10, dropout_p=0.0, seed=1, offset=0, conv_algo=1)
    fn = 'r4r_%s_span_score' % name
    args = []
    for a, t in zip(decl[fn][2], decl[fn][1]):
        if a in over:
            args.append(over[a])
        elif a in host:
            args.append(host[a])
        elif a in scalars:
            args.append(scalars[a])
        elif t is ctypes.c_void_p:
            args.append(FAKE)
        else:
            args.append(0)
    rc = getattr(lib, fn)(*args)
    return rc, done.value, lib.r4r_last_error()


def _words(name, **kw):
    if name in ('mf', 'idnet'):
        w = dict(w10=FAKE, w11=FAKE, w15=FAKE, w24=8 * 11 + 5, w26=8)
        w.update(kw)
        return _desc(**w)
    ring = _ring(R=10, W=64) if name == 'narre' else _ring(T=64)
    for k, v in kw.items():
        ring[int(k[1:])] = v
    return ring


def test_every_scoring_symbol_is_declared_and_exported():
    lib, decl = _lib.lib(), _lib.parse_header()
    for name in FAMILIES:
        fn = 'r4r_%s_span_score' % name
        assert getattr(lib, fn) is not None
        assert decl[fn][2][:6] == ['loader', 'nb_item', 'first_launch', 'launches', 'built_group', 'launches_done']
        assert decl[fn][2][-4:] == ['pred_out', 'se_out', 'aux_out', 'stream']
    assert decl['r4r_rank_top1'][2] == ['scores', 'rows', 'C', 'counts', 'stream']


@pytest.mark.parametrize('name', FAMILIES)
def test_refusals_enqueue_nothing(name):
    def refused(what, words=None, **over):
        rc, done, err = _score_call(name, _words(name) if words is None else words, **over)
        assert rc != 0 and done == 0 and err, (name, what, rc, done, err)
        return err

    # a launch range beyond N / n (11 full launches of 8)
    assert b'11 full' in refused('range', first_launch=10, launches=2)
    assert b'full' in refused('range', first_launch=-1)
    # se_out NULL while the descriptor has ratings
    assert b'se_out' in refused('se_out', se_out=None)
    # a resident table together with nb_item
    table = (ctypes.c_uint64 * 8)(*([FAKE] * 8))
    resident = _desc(w24=1 << 40, w25=1, w26=8, w27=ctypes.addressof(table))
    assert b'resident' in refused('resident + nb_item', words=resident, nb_item=FAKE)
    assert b'needs u, i' in refused('an empty descriptor', words=_desc())
    if name == 'transnet':
        assert b'aux_out' in refused('aux_out', aux_out=None)
    if name == 'narre':
        for R in (5, 12, 32):
            assert b'neighbour' in refused('R', words=_ring(R=R, W=64), R=R)
        assert b'descriptor builds' in refused('shape', T=63)
    if name in ('deepconn', 'deepconnpp', 'transnet'):
        assert b'T = 63' in refused('shape', T=63)
        assert b'R x W' in refused('shape', words=_ring(R=10, W=12), T=120)
        assert b'ids-only' in refused('ids-only', words=_desc(w10=FAKE, w11=FAKE, w15=FAKE, w24=64, w26=8))
    if name in ('deepconn', 'deepconnpp', 'narre', 'transnet'):
        assert b'built_group' in refused('built_group', built_group=None)


@pytest.mark.parametrize('name', ['deepconn', 'deepconnpp', 'narre', 'transnet', 'mf', 'idnet'])
def test_training_spans_still_refuse_a_descriptor_without_ratings(name):
    """Word 15 = 0 is a scoring descriptor; the training entries say what they said before."""
    over = dict(R=10, T=64) if name == 'narre' else dict(T=64)
    rc, done, err = _span_call(name, _words(name, w15=0), **over)
    assert rc != 0 and b'the descriptor needs u, i, y and a batch size' in err, err
    assert done == 0 or name in ('mf', 'idnet')              # (the ids-only entries leave steps_done alone, as before)


def test_rank_top1_checks_its_arguments():
    lib = _lib.lib()
    counts = (ctypes.c_int64 * 2)(3, 4)
    for rows, C, c in ((4, 1, counts), (4, 65, counts), (-1, 6, counts), (4, 6, None)):
        assert lib.r4r_rank_top1(FAKE, rows, C, c, None) != 0 and b'rank_top1' in lib.r4r_last_error()
    assert lib.r4r_rank_top1(None, 4, 6, counts, None) != 0
    assert lib.r4r_rank_top1(None, 0, 6, counts, None) == 0 and list(counts) == [3, 4]     # no rows: nothing to add


# ---------------------------------------------------------------- evaluate()'s host reductions
class RecordedEngine:
    """The engine's duck type over per-rating values computed by the float oracle, one rating per forward (TransNet's
    transform loss of a one-rating batch is that rating's distance): score_split hands evaluate() the whole split at
    once, predict / aux serve the per-launch loop."""

    def __init__(self, model, hp):
        self.model, self.tn, self.calls = model, hp['model_type'] in ('transnet', 'transnet++'), 0

    def _values(self, data, y):
        rows = []
        with torch.no_grad():
            for r in range(int(data[5].shape[0])):
                one = [None if d is None else d[r:r + 1] for d in data]
                out = self.model(one)
                if self.tn:
                    rows.append([float(out[0][0]), float(out[1][0]), float(out[2])])
                else:
                    rows.append([float(out.reshape(-1)[0]), 0.0, 0.0])
        v = torch.tensor(rows, dtype=torch.float32).reshape(-1, 3)
        yy = y.float().reshape(-1)
        return v[:, 0], (v[:, 0] - yy) ** 2, torch.stack([v[:, 1], (v[:, 1] - yy) ** 2, v[:, 2]], dim=1)

    def predict(self, data, y=None):
        pred, se, self._aux = self._values(data, y)
        return pred, se

    def aux(self, data):
        return self._aux

    def score_split(self, reader, desc):
        self.calls += 1
        parts = [self._values(data, y) for data, y in reader.iter(eval=True)]
        aux = torch.cat([p[2][:, 1:3] for p in parts])
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), (aux if self.tn else None)


class DeviceFaced:
    """A host loader that answers like a device loader where evaluate() decides its path (its iterators stay the
    host's: the recorded engine computes on the CPU)."""

    def __init__(self, loader):
        self._loader = loader

    def __getattr__(self, name):
        return getattr(self._loader, name)

    def _on_device(self):
        return True

    def score_descriptor(self, n, **kw):
        return ('descriptor', n)


def _recorded(mt, tmp_path, monkeypatch):
    from reviews4rec_amd.loss import MSELoss
    meta, z = _fixture(mt, 'eval')
    root, train, test, hp = _loaders(mt, tmp_path)
    model = OracleModule(hp, params=_weights(z))
    model.eval()
    return meta, root, DeviceFaced(test), hp, model, RecordedEngine(model, hp), MSELoss(hp)


@pytest.mark.parametrize('mt', EVAL_MODELS)
def test_host_reductions_against_the_reference_fixtures(mt, tmp_path, monkeypatch):
    """evaluate() through the spanned path on recorded per-rating values: MSE, TransNet's means of per-slice means over
    the REFERENCE's slices of batch_size (the last one ragged), the two count -> [SE] maps and the ids they enter --
    what the reference's own evaluate() returned on the Tiny dataset."""
    from reviews4rec_amd.eval import evaluate
    meta, root, test, hp, model, engine, crit = _recorded(mt, tmp_path, monkeypatch)
    assert len(test.data) % hp['batch_size'] != 0            # a ragged last slice
    review = mt != 'MF_dot'
    uc, ic = _counts(root)
    metrics, ucm, icm = evaluate(model, crit, test, hp, uc, ic, review, engine=engine)
    assert engine.calls == 1
    _check_eval(meta, metrics, ucm, icm, uc, ic, meta['ranking'], rtol=1e-4)
    assert all(isinstance(v, float) for v in metrics.values()) and all(isinstance(k, int) for k in ucm)
    # the launch size does not enter: the slices are the reference's
    m2, _, _ = evaluate(model, crit, test, dict(hp, eval_batch_size=3 * hp['batch_size']), *_counts(root), review,
                        engine=engine)
    assert m2 == metrics


def test_slice_means_and_rounding():
    from reviews4rec_amd.eval import metrics_from_se, slice_means
    v = np.arange(22, dtype=np.float64).reshape(11, 2)
    total, slices = slice_means(v, 4)                        # slices of 4, 4 and a ragged 3
    assert slices == 3
    assert np.allclose(total, v[:4].mean(0) + v[4:8].mean(0) + v[8:].mean(0))
    assert slice_means(v, 11)[1] == 1 and slice_means(v, 50)[1] == 1 and slice_means(v, 1)[1] == 11
    ses = np.array([0.12344, 0.12346, 1.0, 2.0], np.float32)
    m = metrics_from_se(ses, None, 2)
    assert m == {'MSE': round(float(ses.astype(np.float64).sum()) / 4, 4)}
    m = metrics_from_se(ses, np.stack([ses, 2 * ses], 1), 3)
    a = ses.astype(np.float64)
    assert m['MSE_right'] == round((a[:3].mean() + a[3:].mean()) / 2, 4)
    assert m['MSE_transform'] == round(2 * (a[:3].mean() + a[3:].mean()) / 2, 4)
    with pytest.raises(ZeroDivisionError):
        metrics_from_se(np.zeros(0, np.float32), None, 4)


@pytest.mark.parametrize('how', ['env', 'hyper_params', 'no score_split', 'host loader'])
def test_the_off_switches(how, tmp_path, monkeypatch):
    """R4R_SPANS=0, hyper_params['eval_spans'] = False, an engine without score_split, a loader on the host: the
    per-launch loop runs, with the same results."""
    from reviews4rec_amd.eval import evaluate
    mt = 'transnet++'
    meta, root, test, hp, model, engine, crit = _recorded(mt, tmp_path, monkeypatch)
    if how == 'env':
        monkeypatch.setenv('R4R_SPANS', '0')
    elif how == 'hyper_params':
        hp = dict(hp, eval_spans=False)
    elif how == 'no score_split':
        monkeypatch.delattr(RecordedEngine, 'score_split')
    else:
        test = test._loader
    uc, ic = _counts(root)
    metrics, ucm, icm = evaluate(model, crit, test, hp, uc, ic, True, engine=engine)
    assert engine.calls == 0
    _check_eval(meta, metrics, ucm, icm, uc, ic, meta['ranking'], rtol=1e-4)
