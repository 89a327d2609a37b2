"""The document fold without a GPU (include/r4r.h, "Document fold"): tower_fold_ref's fold against its brute force over
every window, bit for bit; the search reference against the true minimum; the entry points' refusals, which come before
any launch; ``review_counterfactual``'s argument checks on a catalogue whose engine raises when flushed."""
import ctypes

import numpy as np
import pytest
import torch

import tower_fold_ref as R
from tower_variants_ref import COUNTS, synthetic_pool, variant_doc

OK, ERR_ARG = 0, -1
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
ALL = (1 << 64) - 1
NAN = float('nan')


# ---------------------------------------------------------------- the fold is the brute force
def test_the_fold_equals_every_window_over_random_pools():
    """T 1 .. 13, reviews of 0 .. 5 words, 0 .. 8 of them, a slot limit of 1 .. 6 with a tail behind it, cached maxima
    for some slots only, word 0 a zero row in a third of the pools."""
    rng = np.random.default_rng(0)
    V, F = 7, 5
    saved = 0
    for trial in range(4000):
        P = rng.standard_normal((V, 3, F)).astype(np.float32)
        b = rng.standard_normal(F).astype(np.float32)
        if trial % 3 == 0:
            P[0] = 0
        cnt, SL = int(rng.integers(0, 9)), int(rng.integers(1, 7))
        lens = [int(rng.integers(0, 6)) for _ in range(cnt)]
        rev_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        first = np.array([0, cnt], np.int64)
        tok = rng.integers(0, V, int(rev_off[-1])).astype(np.int32)
        T, mask = int(rng.integers(1, 14)), int(rng.integers(0, 1 << SL))
        S = SL if trial % 2 else int(rng.integers(0, SL + 1))
        revs = R.reviews_of(tok, rev_off, first, 0)
        runs, cached = R.pool_runs(tok, rev_off, first, 0, mask, S=S, slots=SL)
        got, n = R.fold(P, b, runs, [None if s is None else R.seg(P, b, revs[s]) for s in cached], T)
        kept = [revs[s] for s in range(min(cnt, SL)) if not (mask >> s) & 1]
        doc = ([t for r in kept for t in r] + [t for r in revs[SL:] for t in r])[:T]
        doc += [0] * (T - len(doc))
        want = R.brute(P, b, doc)
        assert got.tobytes() == want.tobytes(), trial
        assert R.brute_docs(P, b, [doc])[0].tobytes() == want.tobytes(), trial
        assert not np.signbit(got).any()
        saved += (T + 2) - n
    assert saved > 0                                        # cached maxima stand in for windows


@pytest.mark.parametrize('T', (1, 5, 37, 300))
def test_the_fold_equals_every_window_over_the_synthetic_pool(T):
    tok, rev_off, first, counts = synthetic_pool()
    assert tuple(counts) == COUNTS == (0, 1, 2, 63, 64, 65, 70)
    rng = np.random.default_rng(T)
    F = 6
    P, b = rng.standard_normal((1000, 3, F)).astype(np.float32), rng.standard_normal(F).astype(np.float32)
    P[0] = 0
    for o, c in enumerate(int(c) for c in counts):
        segs = R.seg_table(P, b, tok, rev_off, first, [o], 64)[0]
        live = min(c, 64)
        masks = [0, ALL, (1 << live) - 1, ALL >> c << c if c < 64 else 0, 0x5555555555555555]
        masks += [1 << s for s in range(0, 64, 7)] + [ALL & ~(1 << s) for s in (0, live // 2, 63)]
        for m in masks:
            got = R.fold_pool(P, b, tok, rev_off, first, o, m, T, segs=segs)
            assert got.tobytes() == R.brute(P, b, variant_doc(tok, rev_off, first, o, m, (), T)).tobytes(), (o, hex(m))
        for S in (0, 1, 64):                                # fewer cached slots than reviews: the same bits
            assert R.fold_pool(P, b, tok, rev_off, first, o, 5, T, S=S).tobytes() == \
                R.brute_pool(P, b, tok, rev_off, first, o, 5, T).tobytes()


# ---------------------------------------------------------------- the search reference
def test_the_greedy_steps_are_never_below_the_true_minimum():
    """A toy scorer over S <= 6 slots a side: every mask is scanned for the fewest removals that cross."""
    rng = np.random.default_rng(3)
    found = 0
    for trial in range(300):
        S_u, S_i, T = int(rng.integers(1, 7)), int(rng.integers(0, 7)), int(rng.integers(3, 12))
        lens_u, lens_i = [int(x) for x in rng.integers(0, 4, S_u)], [int(x) for x in rng.integers(0, 4, S_i)]
        w = rng.standard_normal((2, 6)).astype(np.float32)
        pair = rng.standard_normal((6, 6)).astype(np.float32) * 0.5

        def score(mu, mi):                                  # removals interact: the greedy choice can be wrong
            x = np.array([(mu >> s) & 1 for s in range(6)], np.float32)
            y = np.array([(mi >> s) & 1 for s in range(6)], np.float32)
            return np.float32(w[0] @ x + w[1] @ y + x @ pair @ y)
        direction = trial % 2
        target = np.float32(rng.standard_normal() * 1.5)
        cand_u, cand_i = int(rng.integers(0, 64)), (int(rng.integers(0, 64)) if S_i else None)
        order, scores, steps, hit = R.search(score, lens_u, lens_i, S_u, S_i, T, 0, 0, cand_u, cand_i, target, direction, 12)
        assert scores[0] == score(0, 0) and len(order) == 12 and len(scores) == 13
        assert all(c == -1 for c in order[steps:]) and all(s == scores[steps] for s in scores[steps:])
        assert hit == R.crossed(scores[steps], target, direction)
        if not hit:
            continue
        least = min(bin(mu).count('1') + bin(mi).count('1') for mu in range(1 << S_u) for mi in range(1 << max(S_i, 0))
                    if R.crossed(score(mu, mi), target, direction))
        assert steps >= least, trial
        found += 1
        mu = sum(1 << c for c in order[:steps] if c < R.ITEM)
        mi = sum(1 << (c - R.ITEM) for c in order[:steps] if c >= R.ITEM)
        assert scores[steps] == score(mu, mi)
    assert found >= 50


def test_the_search_rule_at_its_edges():
    score = lambda mu, mi: np.float32(10 - bin(mu).count('1') - 2 * bin(mi).count('1'))
    run = lambda **kw: R.search(score, [2, 0, 2, 2], [1, 1], 4, 2, kw.pop('T', 5), kw.pop('start_u', 0), 0,
                                kw.pop('cand_u', ALL), kw.pop('cand_i', ALL), kw.pop('target', NAN), kw.pop('direction', 0), 4)
    assert run()[0] == [R.ITEM, R.ITEM + 1, 0, 2]           # the lowest score first; slot 1 is empty, never a step
    assert run(T=4)[0][2:] == [0, 2]                        # slot 3 starts at 4 = T until a removal slides it in ...
    assert run(T=4, cand_i=None)[0] == [0, 2, 3, -1]        # ... (ties go to the lowest c)
    assert run(T=2, cand_i=None, cand_u=0b1100)[0] == [-1] * 4           # candidates that do not show
    assert run(direction=1, cand_i=None)[0] == [0, 2, 3, -1]             # 'up': the best is still taken, the wrong way
    assert run(target=np.float32(8))[2:] == (2, True)       # strict: the first step's 8 < 8 does not hold, the second's 6 does
    assert run(target=np.float32(6))[2:] == (3, True)
    assert run(target=np.float32(10))[2:] == (1, True)      # ... nor does 10 < 10 at the start
    assert run(target=np.float32(11))[2:] == (0, True) and run(target=NAN)[3] is False
    assert run(start_u=0b0101, cand_i=None)[0] == [3, -1, -1, -1]


# ---------------------------------------------------------------- the entry points' refusals
@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(lib, name, args):
    from reviews4rec_amd import _lib
    names = _lib.parse_header()[name][2]
    assert list(args) == names, (list(args), names)         # the dict IS the header's argument list
    return getattr(lib, name)(*args.values())


def _args(base, kw):
    assert not set(kw) - set(base)
    base.update(kw)
    return base


ARGS = {
    'r4r_fold_project': lambda **kw: _args(dict(table=PTR, V=50, conv_w=PTR, ptab=PTR, E=8, F=100, stream=None), kw),
    'r4r_fold_segments': lambda **kw: _args(dict(ptab=PTR, conv_b=PTR, tok=PTR, rev_off=PTR, first=PTR, ids=PTR, n=5, S=12,
                                                 F=100, seg=PTR, stream=None), kw),
    'r4r_fold_compose': lambda **kw: _args(dict(ptab=PTR, conv_b=PTR, seg=PTR, S=12, tok=PTR, rev_off=PTR, first=PTR,
                                                row_owner=PTR, ids=PTR, drop=PTR, M=9, T=37, F=100, pooled=PTR,
                                                stream=None), kw),
    'r4r_fold_search_begin': lambda **kw: _args(dict(score0=PTR, target=PTR, direction=0, budget=5, n_p=7, out_order=PTR,
                                                     out_scores=PTR, out_steps=PTR, out_crossed=PTR, done=PTR,
                                                     stream=None), kw),
    'r4r_fold_search_rows': lambda **kw: _args(dict(rev_off_u=PTR, first_u=PTR, ids_u=PTR, own_u=PTR, mask_u=PTR, cand_u=PTR,
                                                    S_u=12, rev_off_i=PTR, first_i=PTR, ids_i=PTR, own_i=PTR, mask_i=PTR,
                                                    cand_i=PTR, S_i=5, done=PTR, n_p=7, T=37, row_owner_u=PTR, drop_u=PTR,
                                                    row_owner_i=PTR, drop_i=PTR, stream=None), kw),
    'r4r_fold_search_pick': lambda **kw: _args(dict(cand_score=PTR, row_owner_u=PTR, row_owner_i=PTR, S_u=12, S_i=5,
                                                    target=PTR, direction=1, budget=5, n_p=7, mask_u=PTR, mask_i=PTR,
                                                    z_u=PTR, z_i=PTR, L=32, out_order=PTR, out_scores=PTR, out_steps=PTR,
                                                    out_crossed=PTR, done=PTR, stream=None), kw),
}
EMPTY = {'r4r_fold_project': 'V', 'r4r_fold_segments': 'n', 'r4r_fold_compose': 'M', 'r4r_fold_search_begin': 'n_p',
         'r4r_fold_search_rows': 'n_p', 'r4r_fold_search_pick': 'n_p'}


def test_the_library_exports_the_symbols_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    ints = dict(V=ctypes.c_int64, n=ctypes.c_int64, M=ctypes.c_int64, n_p=ctypes.c_int64)
    for name, make in ARGS.items():
        assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
        assert decls[name][2] == list(make())
        for arg, t in zip(decls[name][2], decls[name][1]):
            want = ctypes.c_void_p if make()[arg] in (PTR, None) else ints.get(arg, ctypes.c_int)
            assert t is want, (name, arg)
    assert decls['r4r_fold_ptab_stride'] == (ctypes.c_int, [ctypes.c_int], ['F'])
    for F in (1, 5, 100, 112):
        assert lib.r4r_fold_ptab_stride(F) >= 3 * F
    assert lib.r4r_fold_ptab_stride(0) == 0 and lib.r4r_fold_ptab_stride(113) == 0
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * Document fold:'):]
    for cite in ('common_pytorch_models.py:29-31', 'data.py:223-235', 'DeepCoNN.py:53-54', '((r0 + r1) + r2) + conv_b',
                 'ties (float ==) to the lowest column', 'CURRENT document'):
        assert cite in section, cite


@pytest.mark.parametrize('name, over, word', [
    ('r4r_fold_project', dict(F=0), b'F='), ('r4r_fold_project', dict(F=113), b'F='),
    ('r4r_fold_project', dict(E=0), b'word_embed_size'), ('r4r_fold_project', dict(E=6), b'word_embed_size'),
    ('r4r_fold_project', dict(V=-1), b'V='), ('r4r_fold_project', dict(V=1 << 31), b'V='),
    ('r4r_fold_project', dict(table=None), b'null'), ('r4r_fold_project', dict(conv_w=None), b'null'),
    ('r4r_fold_project', dict(ptab=None), b'null'),
    ('r4r_fold_segments', dict(F=0), b'F='), ('r4r_fold_segments', dict(F=113), b'F='),
    ('r4r_fold_segments', dict(S=0), b'S='), ('r4r_fold_segments', dict(S=65), b'S='),
    ('r4r_fold_segments', dict(n=-1), b'n='), ('r4r_fold_segments', dict(n=1 << 31), b'n='),
    ('r4r_fold_segments', dict(ptab=None), b'null'), ('r4r_fold_segments', dict(conv_b=None), b'null'),
    ('r4r_fold_segments', dict(tok=None), b'null'), ('r4r_fold_segments', dict(rev_off=None), b'null'),
    ('r4r_fold_segments', dict(first=None), b'null'), ('r4r_fold_segments', dict(ids=None), b'null'),
    ('r4r_fold_segments', dict(seg=None), b'null'),
    ('r4r_fold_compose', dict(F=0), b'F='), ('r4r_fold_compose', dict(F=113), b'F='),
    ('r4r_fold_compose', dict(S=0), b'S='), ('r4r_fold_compose', dict(S=65), b'S='),
    ('r4r_fold_compose', dict(T=0), b'T='), ('r4r_fold_compose', dict(T=65537), b'T='),
    ('r4r_fold_compose', dict(M=-1), b'M='), ('r4r_fold_compose', dict(M=1 << 31), b'M='),
    ('r4r_fold_compose', dict(ptab=None), b'null'), ('r4r_fold_compose', dict(seg=None), b'null'),
    ('r4r_fold_compose', dict(tok=None), b'null'), ('r4r_fold_compose', dict(row_owner=None), b'null'),
    ('r4r_fold_compose', dict(ids=None), b'null'), ('r4r_fold_compose', dict(pooled=None), b'null'),
    ('r4r_fold_search_begin', dict(direction=2), b'direction'), ('r4r_fold_search_begin', dict(budget=0), b'budget='),
    ('r4r_fold_search_begin', dict(budget=65), b'budget='), ('r4r_fold_search_begin', dict(n_p=-1), b'n_p='),
    ('r4r_fold_search_begin', dict(n_p=(1 << 31) // 6 + 1), b'n_p='), ('r4r_fold_search_begin', dict(score0=None), b'null'),
    ('r4r_fold_search_begin', dict(target=None), b'null'), ('r4r_fold_search_begin', dict(done=None), b'null'),
    ('r4r_fold_search_rows', dict(S_u=-1), b'S_u='), ('r4r_fold_search_rows', dict(S_u=65), b'S_u='),
    ('r4r_fold_search_rows', dict(S_i=65), b'S_i='), ('r4r_fold_search_rows', dict(S_u=0, S_i=0), b'S_u='),
    ('r4r_fold_search_rows', dict(T=0), b'T='), ('r4r_fold_search_rows', dict(T=65537), b'T='),
    ('r4r_fold_search_rows', dict(n_p=-1), b'n_p='), ('r4r_fold_search_rows', dict(done=None), b'done'),
    ('r4r_fold_search_rows', dict(own_u=None), b'user side'), ('r4r_fold_search_rows', dict(drop_i=None), b'item side'),
    ('r4r_fold_search_pick', dict(S_u=65), b'S_u='), ('r4r_fold_search_pick', dict(S_u=0, S_i=0), b'S_u='),
    ('r4r_fold_search_pick', dict(direction=-1), b'direction'), ('r4r_fold_search_pick', dict(budget=65), b'budget='),
    ('r4r_fold_search_pick', dict(L=0), b'L='), ('r4r_fold_search_pick', dict(n_p=-1), b'n_p='),
    ('r4r_fold_search_pick', dict(cand_score=None), b'null'), ('r4r_fold_search_pick', dict(z_u=None), b'user side'),
    ('r4r_fold_search_pick', dict(mask_i=None), b'item side'),
])
def test_refusals_precede_the_launch_and_name_the_entry_point(lib, name, over, word):
    got = _call(lib, name, ARGS[name](**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(name.encode()) and word in msg, (name, over, got, msg)


@pytest.mark.parametrize('name', sorted(ARGS))
def test_nothing_to_do_is_ok_and_enqueues_nothing(lib, name):
    nul = {k: None for k, v in ARGS[name]().items() if v == PTR}
    assert _call(lib, name, ARGS[name](**{EMPTY[name]: 0})) == OK
    assert _call(lib, name, ARGS[name](**dict(nul, **{EMPTY[name]: 0}))) == OK
    bad = dict(F=113) if 'F' in ARGS[name]() else (dict(budget=65) if 'budget' in ARGS[name]() else dict(T=0))
    assert _call(lib, name, ARGS[name](**dict(bad, **{EMPTY[name]: 0}))) == ERR_ARG      # the shape is still checked
    assert (lib.r4r_last_error() or b'').startswith(name.encode())


def test_an_unsearched_side_takes_null_pointers(lib):
    """S = 0 with NULL pointers: the side is not searched.  (The call itself would launch: only the refusal that a
    searched side with the same NULLs gets is shown here.)"""
    side_i = dict(rev_off_i=None, first_i=None, ids_i=None, own_i=None, mask_i=None, cand_i=None, row_owner_i=None, drop_i=None)
    assert _call(lib, 'r4r_fold_search_rows', ARGS['r4r_fold_search_rows'](**side_i)) == ERR_ARG
    assert b'item side' in (lib.r4r_last_error() or b'')


# ---------------------------------------------------------------- the catalogue's argument checks
def test_review_counterfactual_checks_its_arguments_before_anything_runs():
    import reviews4rec_amd
    from test_phrases_host import _bare
    assert reviews4rec_amd.Counterfactual._fields == ('removed_user', 'removed_item', 'order', 'scores', 'steps',
                                                      'crossed', 'base', 'target')
    reached = pytest.raises(AssertionError, match='flushed before')      # every check passed: the pass would start
    for cls, mt in (('Catalogue', 'deepconn'), ('ReluCatalogue', 'deepconn++'), ('TransNetCatalogue', 'transnet++')):
        klass = getattr(reviews4rec_amd, cls)
        assert klass.fold is False and 'fold' not in klass.__init__.__code__.co_varnames
        assert klass.review_counterfactual is reviews4rec_amd.Catalogue.review_counterfactual
        assert klass._leave_topk_targets is reviews4rec_amd.Catalogue._leave_topk_targets
        cat = _bare(klass, mt)
        cat.dev = torch.device('cpu')
        with pytest.raises(ValueError, match='2 users against 1 items'):
            cat.review_counterfactual([0, 1], [0], target=3.0)
        for users, items in (([0], [5]), ([-1], [0]), ([7], [0])):
            with pytest.raises(KeyError):
                cat.review_counterfactual(users, items, target=3.0)
        for kw, word in ((dict(), 'exactly one of target and k'), (dict(target=3.0, k=2), 'exactly one of target and k'),
                         (dict(k=0, side='item'), 'k = 0'), (dict(k=128, side='item'), 'k = 128'),
                         (dict(k=True, side='item'), 'k = True'), (dict(k=2.0, side='item'), 'k = 2.0'),
                         (dict(k=3), 'every item'), (dict(k=3, side='user'), 'every item'),
                         (dict(k=3, side='item', direction='up'), "direction='down' only"),
                         (dict(target=3.0, side='items'), 'side'), (dict(target=3.0, side=None), 'side'),
                         (dict(target=3.0, direction='sideways'), 'direction'),
                         (dict(target=3.0, budget=0), 'budget'), (dict(target=3.0, budget=65), 'budget'),
                         (dict(target=3.0, budget=2.0), 'budget'), (dict(target=3.0, budget=True), 'budget'),
                         (dict(target=3.0, budget=None), 'budget'),
                         (dict(target=torch.zeros(3)), 'target holds 3 values for 2 pairs'),
                         (dict(target='high'), 'target must be'), (dict(target=True), 'target must be')):
            with pytest.raises(ValueError, match=word):
                cat.review_counterfactual([0, 1], [2, 3], **kw)
        for kw in (dict(target=3.0), dict(target=torch.tensor([1.0, 2.0]), direction='up', side='user', budget=64),
                   dict(target=np.array([1.0, NAN]), budget=1), dict(target=[1.0, 2.0], side='item'),
                   dict(k=1, side='item'), dict(k=127, side='item', budget=3)):
            with reached:
                cat.review_counterfactual([0, 1], [2, 3], **kw)


def test_narre_and_towerless_classes_refuse_review_counterfactual():
    import reviews4rec_amd
    from reviews4rec_amd.recommend import phrase_limits
    from test_phrases_host import _bare
    cat = _bare(reviews4rec_amd.NarreCatalogue, 'NARRE')
    with pytest.raises(RuntimeError, match='NarreCatalogue.counterfactual'):
        cat.review_counterfactual([0], [0], target=3.0)
    assert hasattr(reviews4rec_amd.NarreCatalogue, 'counterfactual')
    for cls, mt in (('Catalogue', 'MF_dot'), ('Catalogue', 'bias_only'), ('ReluCatalogue', 'NeuMF'), ('MFCatalogue', 'MF')):
        cat = _bare(getattr(reviews4rec_amd, cls), mt)
        why = phrase_limits(cat.hp)
        assert why
        with pytest.raises(RuntimeError) as e:
            cat.review_counterfactual([0], [0], target=3.0)
        assert why in str(e.value)
