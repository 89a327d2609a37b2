"""Phrase explanations (include/r4r.h, "Phrase explanations"), the parts that need no GPU: the refusals of
r4r_textcnn_phrases and r4r_tower_span_phrases (host addresses that are never dereferenced), the argument errors of
``explain_words``, the refusals of main's explain_words_k hook, and phrases_ref -- the sequential statement of the
contract that tests/test_gpu_phrases*.py hold the kernel to -- against a brute-force dictionary version."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from phrases_ref import bits, fma32, phrases_ref, round_f32, tokens_ref

OK, ERR_ARG, ERR_WS = 0, -1, -3
P = 4096                                                    # a non-null "pointer": never dereferenced by a refusal
NAME, SPAN = b'r4r_textcnn_phrases', b'r4r_tower_span_phrases'


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def call(lib, name, args):
    from reviews4rec_amd import _lib
    names = _lib.parse_header()[name][2]
    assert list(args) == names, (list(args), names)         # the dict IS the header's argument list
    return getattr(lib, name)(*args.values())


def phrase_args(**kw):
    a = dict(pooled=P, argmax=P, wt=P, wt_stride=100, idx=P, N=7, T=64, F=100, K=5, top_pos=P, top_score=P,
             top_filters=P, top_tok=P, n_windows=P, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def span_args(**kw):
    a = dict(tok=P, rev_off=P, first=P, nb=P, owners=100, ids=P, n=70, group=32, T=64, R=0, W=0, pad=0, table=P, V=400,
             conv_w=P, conv_b=P, E=20, F=100, wt=None, wt_stride=0, K=5, top_pos=P, top_score=P, top_filters=P,
             top_tok=P, n_windows=P, neigh=None, ws=P, ws_bytes=1 << 40, groups_done=None, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


# ---------------------------------------------------------------- the header and the library
def test_the_library_exports_both_symbols_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    for name in ('r4r_textcnn_phrases', 'r4r_tower_span_phrases'):
        assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int, name
    assert decls['r4r_textcnn_phrases'][2] == list(phrase_args())
    assert decls['r4r_tower_span_phrases'][2] == list(span_args())
    ints = dict(wt_stride=ctypes.c_int64, N=ctypes.c_int64, T=ctypes.c_int, F=ctypes.c_int, K=ctypes.c_int)
    for name, t in zip(decls['r4r_textcnn_phrases'][2], decls['r4r_textcnn_phrases'][1]):
        assert t is ints.get(name, ctypes.c_void_p), name
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * Phrase explanations:'):]
    for cite in ('common_pytorch_models.py:29-31', 'DeepCoNN.py:53-54', 'NARRE.py:95-96', 'TransNet.py:100-102'):
        assert cite in section, cite
    # the span's leading arguments are r4r_tower_span_fwd's
    fwd = decls['r4r_tower_span_fwd'][2]
    assert decls['r4r_tower_span_phrases'][2][:16] == fwd[:16] and 'latent' not in span_args() and 'L' not in span_args()


# ---------------------------------------------------------------- r4r_textcnn_phrases
@pytest.mark.parametrize('over, word', [
    (dict(pooled=None), b'null'), (dict(argmax=None), b'null'),
    (dict(F=0, wt_stride=0), b'F='), (dict(F=113, wt_stride=113), b'F='), (dict(F=-4, wt_stride=0), b'F='),
    (dict(K=0), b'K='), (dict(K=101), b'K='), (dict(K=-1), b'K='), (dict(K=113, F=112, wt_stride=112), b'K='),
    (dict(T=0), b'T='), (dict(T=-5), b'T='),
    (dict(N=-1), b'N='), (dict(N=1 << 31), b'N='),
    (dict(wt_stride=1), b'wt_stride'), (dict(wt_stride=99), b'wt_stride'), (dict(wt_stride=-100), b'wt_stride'),
    (dict(wt_stride=200), b'wt_stride'),
    (dict(idx=None), b'top_tok'),
])
def test_phrases_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = call(lib, 'r4r_textcnn_phrases', phrase_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(NAME) and word in msg, (over, got, msg)


def test_no_rows_is_ok_and_enqueues_nothing(lib):
    assert call(lib, 'r4r_textcnn_phrases', phrase_args(N=0)) == OK
    nul = dict(top_pos=None, top_score=None, top_filters=None, top_tok=None, n_windows=None, idx=None, wt=None)
    assert call(lib, 'r4r_textcnn_phrases', phrase_args(N=0, **nul)) == OK
    assert call(lib, 'r4r_textcnn_phrases', phrase_args(N=0, wt_stride=0)) == OK
    # ... but the shape is still checked
    assert call(lib, 'r4r_textcnn_phrases', phrase_args(N=0, K=101)) == ERR_ARG
    assert (lib.r4r_last_error() or b'').startswith(NAME)


# ---------------------------------------------------------------- r4r_tower_span_phrases
@pytest.mark.parametrize('what, over, rc, msg', [
    ('null pool', dict(tok=None), ERR_ARG, b'null pointer'),
    ('null ids', dict(ids=None), ERR_ARG, b'null pointer'),
    ('null table', dict(table=None), ERR_ARG, b'null pointer'),
    ('null conv bias', dict(conv_b=None), ERR_ARG, b'null pointer'),
    ('null workspace', dict(ws=None), ERR_ARG, b'null pointer'),
    ('NARRE without neigh', dict(R=10, W=16, neigh=None), ERR_ARG, b'null pointer'),
    ('group 0', dict(group=0), ERR_ARG, b'group'),
    ('group -3', dict(group=-3), ERR_ARG, b'group'),
    ('E % 4', dict(E=50), ERR_ARG, b'multiple of 4'),
    ('E 0', dict(E=0), ERR_ARG, b'multiple of 4'),
    ('F 113', dict(F=113), ERR_ARG, b'112'),
    ('T 0', dict(T=0), ERR_ARG, b'bad shape'),
    ('R without W', dict(R=10, W=0, neigh=P), ERR_ARG, b'bad shape'),
    ('R negative', dict(R=-1), ERR_ARG, b'bad shape'),
    ('n negative', dict(n=-1), ERR_ARG, b'bad shape'),
    ('n 2^31', dict(n=1 << 31), ERR_ARG, b'bad shape'),
    ('owners negative', dict(owners=-1), ERR_ARG, b'bad shape'),
    ('K 0', dict(K=0), ERR_ARG, b'K='),
    ('K above F', dict(K=101), ERR_ARG, b'K='),
    ('a stride that is neither 0 nor F', dict(wt=P, wt_stride=8), ERR_ARG, b'wt_stride'),
    ('2^31 rows', dict(n=(1 << 31) - 1, R=10, W=16, neigh=P), ERR_ARG, b'rows'),
    ('no workspace bytes', dict(ws_bytes=0), ERR_WS, b'workspace'),
])
def test_span_refusals_need_no_gpu(lib, what, over, rc, msg):
    done = ctypes.c_int64(-7)
    got = call(lib, 'r4r_tower_span_phrases', span_args(groups_done=ctypes.byref(done), **over))
    err = lib.r4r_last_error() or b''
    assert got == rc and err.startswith(SPAN) and msg in err, (what, got, err)
    assert done.value == 0, what                            # no round was enqueued


@pytest.mark.parametrize('shape', [dict(T=64), dict(R=10, W=16, neigh=P), dict(T=300, E=52, n=5, group=256)])
def test_a_workspace_one_byte_short_is_refused(lib, shape):
    """The workspace is r4r_tower_span_fwd's: r4r_tower_span_ws_bytes of the largest round, whatever latent size it is told."""
    a = span_args(**shape)
    G = min(a['group'], a['n'])
    need = lib.r4r_tower_span_ws_bytes(G, a['T'], a['R'], a['W'], a['E'], a['F'], 8, a['V'])
    assert need > 0 and need == lib.r4r_tower_span_ws_bytes(G, a['T'], a['R'], a['W'], a['E'], a['F'], 64, a['V'])
    done = ctypes.c_int64(-7)
    got = call(lib, 'r4r_tower_span_phrases', span_args(ws_bytes=need - 1, groups_done=ctypes.byref(done), **shape))
    assert got == ERR_WS and b'workspace' in lib.r4r_last_error() and done.value == 0


def test_an_empty_span_is_a_no_op(lib):
    done = ctypes.c_int64(-7)
    assert call(lib, 'r4r_tower_span_phrases', span_args(n=0, groups_done=ctypes.byref(done))) == OK and done.value == 0
    assert call(lib, 'r4r_tower_span_phrases', span_args(n=0, tok=None, ws=None, K=0)) == OK


# ---------------------------------------------------------------- the reference
def test_round_f32_rounds_once_to_nearest_even():
    one, eps = Fraction(1), Fraction(1, 1 << 23)
    assert round_f32(one + eps / 2) == np.float32(1.0)                       # a tie: to the even neighbour
    assert round_f32(one + eps + eps / 2) == np.float32(1.0) + np.float32(2.0 ** -22)
    assert round_f32(one + eps / 2 + Fraction(1, 1 << 80)) == np.float32(1.0 + 2.0 ** -23)   # just above the tie
    assert round_f32(Fraction(0)) == 0 and round_f32(-one - eps) == np.float32(-1.0 - 2.0 ** -23)
    assert round_f32(Fraction(1, 1 << 149)) == np.float32(2.0 ** -149) and round_f32(Fraction(1, 1 << 151)) == 0
    rng = np.random.default_rng(0)
    for a, b in rng.standard_normal((200, 2)).astype(np.float32):
        assert bits(fma32(a, b, 0.0)) == bits(np.float32(a) * np.float32(b))  # one rounding: the fp32 product
        assert bits(fma32(1.0, a, b)) == bits(np.float32(a) + np.float32(b))  # ... and the fp32 sum
    # where a float64 detour would round twice: 1 + 2^-24 + 2^-60 is above the tie, float64 drops the 2^-60
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1 + 2.0 ** -11)          # rounded twice: down
    assert fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)                         # rounded once: up


def _brute(pooled, argmax, wt, T, K):
    """The contract by dictionary: group the live filters by position, sum each group in ascending f, then pick the
    best window left, K times."""
    N, F = pooled.shape
    out = []
    for n in range(N):
        groups = {}
        for f in range(F):
            p = int(argmax[n, f])
            if p < 0 or p >= T + 2:
                continue
            groups.setdefault(p, []).append(f)
        sums = {}
        for p, fs in groups.items():
            acc = np.float32(0.0)
            for f in sorted(fs):
                if wt is None:
                    acc = np.float32(acc + pooled[n, f])
                else:
                    w = wt[f] if wt.ndim == 1 else wt[n, f]
                    acc = fma32(w, pooled[n, f], acc)
            sums[p] = acc
        left, row = set(sums), []
        while left and len(row) < K:
            best = None
            for p in left:
                if best is None or sums[p] > sums[best] or (sums[p] == sums[best] and p < best):
                    best = p
            row.append((best, sums[best], len(groups[best])))
            left.remove(best)
        out.append((row, len(sums)))
    return out


@pytest.mark.parametrize('weights', [None, 'shared', 'per row'])
def test_phrases_ref_against_a_brute_force_dictionary(weights):
    rng = np.random.default_rng(11)
    for F, T in ((1, 1), (7, 3), (20, 5), (64, 40), (100, 9)):
        N = 12
        pooled = rng.random((N, F)).astype(np.float32)
        pooled[1] = 0.25                                      # equal contributions: ties between windows of equal size
        argmax = rng.integers(-2, T + 4, size=(N, F)).astype(np.int32)     # dead ones on both sides
        argmax[2] = -1                                        # a row of dead filters
        argmax[3] = T + 1                                     # one window
        argmax[4] = np.arange(F) % (T + 2)                    # every position
        wt = None
        if weights == 'shared':
            wt = rng.standard_normal(F).astype(np.float32)
        elif weights == 'per row':
            wt = rng.standard_normal((N, F)).astype(np.float32)
        for K in sorted({1, min(3, F), F}):
            pos, score, filt, win = phrases_ref(pooled, argmax, wt, T, K)
            assert pos.dtype == np.int32 and score.dtype == np.float32 and filt.dtype == np.int32 and win.dtype == np.int32
            assert pos.shape == score.shape == filt.shape == (N, K) and win.shape == (N,)
            for n, (row, count) in enumerate(_brute(pooled, argmax, wt, T, K)):
                assert win[n] == count and len(row) == min(K, count)
                assert pos[n, :len(row)].tolist() == [r[0] for r in row], (F, T, K, n)
                assert bits(score[n, :len(row)]).tolist() == [int(bits(r[1]).ravel()[0]) for r in row]
                assert filt[n, :len(row)].tolist() == [r[2] for r in row]
                assert (pos[n, len(row):] == -1).all() and (bits(score[n, len(row):]) == 0).all()
                assert (filt[n, len(row):] == 0).all()
            assert win[2] == 0 and (pos[2] == -1).all()
            assert win[3] == 1 and pos[3, 0] == T + 1 and filt[3, 0] == F
            assert win[4] == min(F, T + 2)
            # a list at K is the head of the list at F
            full = phrases_ref(pooled, argmax, wt, T, F)
            assert np.array_equal(pos, full[0][:, :K]) and np.array_equal(bits(score), bits(full[1][:, :K]))


def test_tokens_ref_marks_the_conv_padding():
    idx = np.array([[11, 12, 13, 0]], np.int64)               # T = 4, the last word is the pad word 0
    pos = np.array([[0, 1, 2, 4, 5, -1]], np.int32)           # T + 1 = 5 is the last conv position
    tok = tokens_ref(pos, idx, 4)
    assert tok[0].tolist() == [[-1, -1, 11], [-1, 11, 12], [11, 12, 13], [13, 0, -1], [0, -1, -1], [-1, -1, -1]]


# ---------------------------------------------------------------- explain_words' arguments
class _Pool:
    owners = 5
    first = np.arange(6, dtype=np.int64)


class _Store:
    users = items = _Pool()


class _Reader:
    store = _Store()


class _Loud:
    def flush(self):
        raise AssertionError('flushed before the arguments were checked')


def _tower(F=100):
    import types
    import torch
    return types.SimpleNamespace(convs=[types.SimpleNamespace(bias=torch.zeros(F))],
                                 fc=types.SimpleNamespace(weight=torch.ones(8, F)))


def _bare(cls, mt):
    """A catalogue without a device: ``explain_words``' checks come before the first use of one."""
    import types
    cat = object.__new__(cls)
    cat.hp = dict(model_type=mt, narre_num_reviews=10, narre_num_words=16, input_length=64)
    cat.mt, cat.reader, cat.engine, cat.n_users, cat.n_items = mt, _Reader(), _Loud(), 5, 5
    t = _tower()
    cat.model = types.SimpleNamespace(user_conv=t, item_conv=t, source=types.SimpleNamespace(user_conv=t, item_conv=t))
    return cat


@pytest.mark.parametrize('cls, mt', [('Catalogue', 'deepconn'), ('ReluCatalogue', 'deepconn++'),
                                     ('TransNetCatalogue', 'transnet++'), ('NarreCatalogue', 'NARRE')])
def test_explain_words_argument_errors_are_raised_before_anything_runs(cls, mt):
    import torch
    import reviews4rec_amd
    from reviews4rec_amd import Phrases
    assert Phrases._fields[:7] == ('positions', 'scores', 'filters', 'tokens', 'reviews', 'offsets', 'windows')
    assert reviews4rec_amd.recommend.Phrases is Phrases
    cat = _bare(getattr(reviews4rec_amd, cls), mt)
    for side in ('items', 'pair', None, 0):
        with pytest.raises(ValueError, match='side'):
            cat.explain_words([0], side=side)
    for k in (0, -1, 101, 2.0, True, None):
        with pytest.raises(ValueError, match='explain_words k'):
            cat.explain_words([0], k=k)
    for w in ('mass', 3, torch.zeros(99), torch.zeros(2, 100), torch.zeros(100, dtype=torch.float64), [1.0] * 100):
        with pytest.raises(ValueError, match='weights'):
            cat.explain_words([0], k=3, weights=w)
    for side in ('item', 'user'):
        for ids in ([5], [-1], [0, 7]):
            with pytest.raises(KeyError):
                cat.explain_words(ids, k=3, side=side)
    if mt == 'NARRE':
        for r in (0, 11, 2.5, True):
            with pytest.raises(ValueError, match='reviews'):
                cat.explain_words([0], k=3, reviews=r)


@pytest.mark.parametrize('cls, mt', [('Catalogue', 'bias_only'), ('Catalogue', 'MF_dot'), ('ReluCatalogue', 'NeuMF'),
                                     ('MFCatalogue', 'MF')])
def test_a_configuration_without_a_tower_is_refused_with_the_reason(cls, mt):
    import reviews4rec_amd
    cat = _bare(getattr(reviews4rec_amd, cls), mt)
    with pytest.raises(RuntimeError, match='has no TextCNN tower'):
        cat.explain_words([0], k=3)
    assert mt in reviews4rec_amd.phrase_limits(dict(model_type=mt))


# ---------------------------------------------------------------- main's hook
@pytest.mark.parametrize('entry', ['main', 'main_pytorch', 'main_NeuMF'])
def test_explain_words_k_is_refused_before_anything_is_loaded(entry):
    from reviews4rec_amd import main as M
    from reviews4rec_amd.recommend import check_explain_words_request, phrase_limits
    fn = getattr(M, entry)
    ask = dict(latent_size=8, explain_words_k=3, explain_words_path='words.npz', data_dir='/nonexistent/')
    for other in ('NeuMF',) if entry == 'main_NeuMF' else ('MF_dot', 'bias_only', 'MF'):
        hp = dict(ask, model_type=other)
        why = phrase_limits(hp)
        assert isinstance(why, str) and 'no TextCNN tower' in why
        with pytest.raises(RuntimeError) as e:
            fn(hp)
        assert str(e.value) == "hyper_params['explain_words_k']: " + why
    if entry != 'main_NeuMF':
        for mt in ('deepconn', 'deepconn++', 'transnet', 'transnet++', 'NARRE'):
            hp = dict(ask, model_type=mt, narre_num_reviews=10)
            for k in (101, -1, 2.5, True):
                with pytest.raises(RuntimeError, match='explain_words_k'):
                    fn(dict(hp, explain_words_k=k))
            with pytest.raises(RuntimeError, match='explain_words_path'):
                fn({k: v for k, v in hp.items() if k != 'explain_words_path'})
            with pytest.raises(RuntimeError, match='catalogue_towers'):
                fn(dict(hp, catalogue_towers='x'))
            assert check_explain_words_request(dict(hp, catalogue_towers='device')) is None
            assert check_explain_words_request(hp) is None
        with pytest.raises(RuntimeError, match='latent_size 65 > 64'):   # a shape the serving class refuses
            fn(dict(ask, model_type='NARRE', narre_num_reviews=10, latent_size=65))
    # no request, no check
    assert check_explain_words_request(dict(model_type='MF_dot')) is None
    assert check_explain_words_request(dict(model_type='MF_dot', explain_words_k=0)) is None
