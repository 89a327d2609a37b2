"""What-if documents without a GPU (include/r4r.h, "What-if documents"): the rule as a plain loop
(tower_variants_ref.py) and its numpy twin ``data._np_docs_masked`` against the loader's own ``_np_docs``; the entry
points' refusals, which come before any launch; the argument checks of ``Catalogue.what_if`` / ``leave_one_out`` /
``deletion_curve`` on a catalogue whose engine raises when flushed; ``check_explain_reviews_request``."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tower_variants_ref import as_signed, remaining_doc, synthetic_pool, variant_docs

OK, ERR_ARG, ERR_WS = 0, -1, -3
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
TS = (1, 5, 37, 300)


@pytest.fixture(scope='module')
def pool():
    return synthetic_pool()


def _masked(pool, ids, drop, occ, T):
    from reviews4rec_amd.data import _np_docs_masked
    tok, rev_off, first, _ = pool
    ids = np.asarray(ids, np.int64)
    occ_m = None
    if occ is not None:
        P = max([len(o) for o in occ] + [1])
        occ_m = np.full((len(ids), P), -1, np.int64)
        for r, o in enumerate(occ):
            occ_m[r, :len(o)] = o
    d = None if drop is None else np.array([as_signed(int(m)) for m in drop], np.int64)
    return _np_docs_masked(tok, rev_off, first[ids], first[ids + 1], d, occ_m, T)


@pytest.mark.parametrize('T', TS)
def test_one_bit_is_the_loaders_skip_and_no_bit_its_whole_document(pool, T):
    from reviews4rec_amd.data import _np_docs
    tok, rev_off, first, counts = pool
    owners = np.arange(len(counts), dtype=np.int64)
    rb, re = first[owners], first[owners + 1]
    whole = _np_docs(tok, rev_off, rb, re, np.full(len(owners), -1, np.int64), T)
    assert np.array_equal(variant_docs(tok, rev_off, first, owners, None, None, T), whole)
    assert np.array_equal(_masked(pool, owners, None, None, T), whole)
    assert np.array_equal(_masked(pool, owners, [0] * len(owners), [[]] * len(owners), T), whole)
    for skip in range(64):                                   # a skip past an owner's list removes nothing
        want = _np_docs(tok, rev_off, rb, re, np.full(len(owners), skip, np.int64), T)
        drop = [1 << skip] * len(owners)
        assert np.array_equal(variant_docs(tok, rev_off, first, owners, drop, None, T), want), skip
        assert np.array_equal(_masked(pool, owners, drop, None, T), want), skip


@pytest.mark.parametrize('T', TS)
def test_several_bits_are_the_remaining_list_and_the_tail_is_kept(pool, T):
    tok, rev_off, first, counts = pool
    rng = np.random.RandomState(T)
    ids, drop, want = [], [], []
    for o, c in enumerate(int(c) for c in counts):
        sets = [set(), set(range(min(c, 64))), set(range(1, min(c, 64))), {0, min(c, 64) - 1} if c else set()]
        sets += [set(rng.choice(min(c, 64), size=rng.randint(1, min(c, 64) + 1), replace=False).tolist()) for _ in range(4)
                 if c]
        for s in sets:
            ids.append(o)
            drop.append(sum(1 << b for b in s) | (((1 << 64) - 1) >> c << c if c < 64 else 0))   # + bits beyond count
            want.append(remaining_doc(tok, rev_off, first, o, s, T))
        ids.append(o)
        drop.append((1 << 64) - 1)                          # all ones: only the reviews from the 65th on remain
        want.append(remaining_doc(tok, rev_off, first, o, set(range(64)), T))
    want = np.array(want, np.int64)
    assert np.array_equal(variant_docs(tok, rev_off, first, ids, drop, None, T), want)
    assert np.array_equal(_masked(pool, ids, drop, None, T), want)
    if T >= 5:
        assert want[-1].any()                               # the 70-review owner's tail really shows


@pytest.mark.parametrize('T', TS)
def test_occlusion_zeroes_in_place_and_ignores_what_lies_outside(pool, T):
    tok, rev_off, first, counts = pool
    ids = [6, 6, 6, 6, 6, 6, 3, 0]
    drop = [0, 0, 0, 0, 0, 5, (1 << 64) - 2, 0]
    occ = [[], [0], [T - 1], [-1, T, T + 7, -5], [T // 2, T // 2, T // 2], list(range(T)), [0, T - 1], [0]]
    ref = variant_docs(tok, rev_off, first, ids, drop, occ, T)
    assert np.array_equal(_masked(pool, ids, drop, occ, T), ref)
    plain = variant_docs(tok, rev_off, first, ids, drop, None, T)
    assert np.array_equal(ref[0], plain[0]) and np.array_equal(ref[3], plain[3]) and not ref[5].any()
    assert ref[1][0] == 0 and np.array_equal(ref[1][1:], plain[1][1:])
    assert not variant_docs(tok, rev_off, first, [-1, len(counts)], [3, 3], None, T).any()      # ids outside the pool


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


def build_args(**kw):
    a = dict(tok=PTR, rev_off=PTR, first=PTR, owners=7, ids=PTR, drop=PTR, occ_off=PTR, occ_pos=PTR, n=5, T=37, docs=PTR,
             stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def span_args(**kw):
    a = dict(tok=PTR, rev_off=PTR, first=PTR, owners=7, ids=PTR, drop=PTR, occ_off=PTR, occ_pos=PTR, n=5, group=3, T=37,
             table=PTR, V=50, conv_w=PTR, conv_b=PTR, fc_w=PTR, fc_b=PTR, E=8, F=100, L=32, latent=PTR, pooled=PTR,
             argmax=PTR, ws=PTR, ws_bytes=1 << 40, groups_done=None, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def test_the_library_exports_the_symbols_and_the_header_cites_the_loader(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    for name, args in (('r4r_tower_build_variants', build_args()), ('r4r_tower_span_variants', span_args())):
        assert name in decls and hasattr(lib, name) and decls[name][0] is ctypes.c_int
        assert decls[name][2] == list(args)
    assert decls['r4r_tower_span_variants_ws_bytes'][0] is ctypes.c_size_t
    assert decls['r4r_tower_span_variants_ws_bytes'][2] == ['group', 'T', 'E', 'F', 'L', 'V']
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * What-if documents:'):]
    for cite in ('data.py:223-235', 'data.py:181-210', 'data.py:240-246', '65536'):
        assert cite in section, cite


BUILD_REFUSALS = [
    (dict(tok=None), b'null'), (dict(rev_off=None), b'null'), (dict(first=None), b'null'), (dict(ids=None), b'null'),
    (dict(docs=None), b'null'), (dict(n=-1), b'n='), (dict(n=1 << 31), b'n='), (dict(owners=-1), b'owners='),
    (dict(T=0), b'T='), (dict(T=-4), b'T='), (dict(T=65537), b'T='), (dict(occ_pos=None), b'occ_off without occ_pos'),
]


@pytest.mark.parametrize('over, word', BUILD_REFUSALS)
def test_builder_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = _call(lib, 'r4r_tower_build_variants', build_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_tower_build_variants') and word in msg, (over, got, msg)


@pytest.mark.parametrize('over, word', BUILD_REFUSALS[:4] + BUILD_REFUSALS[5:] + [
    (dict(table=None), b'null'), (dict(conv_w=None), b'null'), (dict(conv_b=None), b'null'), (dict(fc_w=None), b'null'),
    (dict(fc_b=None), b'null'), (dict(latent=None), b'null'), (dict(ws=None), b'null'), (dict(group=0), b'group'),
    (dict(E=6), b'multiple of 4'), (dict(E=0), b'multiple of 4'), (dict(F=113), b'filters'), (dict(F=0), b'filters'),
    (dict(L=0), b'L='), (dict(V=0), b'V='),
])
def test_span_refusals_precede_the_first_launch_and_name_the_entry_point(lib, over, word):
    done = ctypes.c_int64(-7)
    got = _call(lib, 'r4r_tower_span_variants', span_args(groups_done=ctypes.addressof(done), **over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(b'r4r_tower_span_variants') and word in msg, (over, got, msg)
    assert done.value == 0


def test_a_short_workspace_is_refused_and_nothing_to_do_is_ok(lib):
    want = lib.r4r_tower_span_variants_ws_bytes(3, 37, 8, 100, 32, 50)
    assert want > 0 and want == lib.r4r_tower_span_ws_bytes(3, 37, 0, 0, 8, 100, 32, 50)     # r4r_tower_span_fwd's layout
    assert _call(lib, 'r4r_tower_span_variants', span_args(ws_bytes=want - 1)) == ERR_WS
    assert (lib.r4r_last_error() or b'').startswith(b'r4r_tower_span_variants')
    for bad in (dict(group=0), dict(T=0), dict(T=65537), dict(E=0), dict(F=0), dict(L=0), dict(V=0)):
        a = dict(group=3, T=37, E=8, F=100, L=32, V=50)
        a.update(bad)
        assert lib.r4r_tower_span_variants_ws_bytes(*a.values()) == 0, bad
    assert lib.r4r_tower_span_variants_ws_bytes(3, 65536, 8, 100, 32, 50) > 0
    nul = lambda args: {k: None for k, v in args.items() if v == PTR}
    assert _call(lib, 'r4r_tower_build_variants', build_args(n=0)) == OK
    assert _call(lib, 'r4r_tower_build_variants', build_args(n=0, **nul(build_args()))) == OK
    done = ctypes.c_int64(-7)
    assert _call(lib, 'r4r_tower_span_variants', span_args(n=0, groups_done=ctypes.addressof(done))) == OK
    assert done.value == 0
    assert _call(lib, 'r4r_tower_span_variants', span_args(n=0, ws_bytes=0, **nul(span_args()))) == OK


# ---------------------------------------------------------------- the catalogue's argument checks
@pytest.mark.parametrize('cls, mt', [('Catalogue', 'deepconn'), ('ReluCatalogue', 'deepconn++'),
                                     ('TransNetCatalogue', 'transnet++')])
def test_the_three_methods_check_their_arguments_before_anything_runs(cls, mt):
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(getattr(reviews4rec_amd, cls), mt)             # five owners a side, one review each; a flush raises
    side = types.SimpleNamespace(owners=5, first=np.arange(6, dtype=np.int64), rev_off=3 * np.arange(6, dtype=np.int64),
                                 tok=np.arange(1, 16, dtype=np.int32))
    cat.reader = types.SimpleNamespace(store=types.SimpleNamespace(users=side, items=side))
    cat.dev = torch.device('cpu')
    T = cat.hp['input_length']
    assert reviews4rec_amd.DocLeaveOneOut._fields == reviews4rec_amd.LeaveOneOut._fields + ('reach_user', 'reach_item')
    assert reviews4rec_amd.DocDeletionCurve._fields == ('scores', 'aopc', 'positions', 'live')
    reached = pytest.raises(AssertionError, match='flushed before')      # every check passed: the pass would start
    for call in (cat.what_if, cat.leave_one_out, cat.deletion_curve):
        with pytest.raises(ValueError, match='2 users against 1 items'):
            call([0, 1], [0])
        for users, items in (([0], [5]), ([-1], [0]), ([7], [0])):
            with pytest.raises(KeyError):
                call(users, items)
        with reached:
            call([0, 1], [2, 3])
    ok = torch.tensor([[1, 0], [0, 1]], dtype=torch.int64)
    bad_drops = ([[0]], [[0], [1]], [[0], [-1]], [[0], [64]], [[0], [True]], [[0], [0.0]], [[0], 0], 'mask', 3,
                 [[[0]], [[0], []]], ok.to(torch.int32), ok.to(torch.float32), ok[0], ok[:1],
                 torch.zeros((2, 0), dtype=torch.int64))
    for side in ('drop_user', 'drop_item'):
        for drop in bad_drops:
            with pytest.raises(ValueError, match=side):
                cat.what_if([0, 1], [2, 3], **{side: drop})
        for drop in ([[0], []], [[[0], []], [[], [0]]], ok, ok.numpy(), ([0], [0])):
            with reached:
                cat.what_if([0, 1], [2, 3], **{side: drop})
    pos = torch.tensor([[[0, -1], [T - 1, 3]], [[-1, -1], [5, 5]]])
    bad_occ = ([[0]], [[0], [T]], [[0], [-2]], [[0], [1.5]], [[0], [True]], [[0], 0], 'all', 3, [[[0]], [[0], []]],
               pos.to(torch.float32), pos[0], pos[:1], pos.clone().fill_(T), torch.zeros((2, 0, 1), dtype=torch.int64))
    for side in ('occlude_user', 'occlude_item'):
        for occ in bad_occ:
            with pytest.raises(ValueError, match=side):
                cat.what_if([0, 1], [2, 3], **{side: occ})
        for occ in ([[0], []], [[[0], []], [[], [T - 1]]], pos, pos.numpy(), pos.to(torch.int32), ([0, 0], [-1])):
            with reached:
                cat.what_if([0, 1], [2, 3], **{side: occ})
    with pytest.raises(ValueError, match=r'\[1, 2\] variants per pair'):
        cat.what_if([0, 1], [2, 3], drop_user=ok, occlude_item=pos[:, :1])
    with reached:
        cat.what_if([0, 1], [2, 3], drop_user=ok, drop_item=ok, occlude_user=pos, occlude_item=pos)
    for kw in (dict(side='items'), dict(side=None), dict(direction='sideways'), dict(by='gradient'), dict(by=None),
               dict(by=torch.zeros(2, 5)), dict(by=torch.zeros(2, 4, dtype=torch.int64)),
               dict(by=torch.zeros(3, 5, dtype=torch.int64)), dict(by=torch.full((2, 5), T + 2)),
               dict(by=torch.full((2, 5), -2)), dict(by=torch.tensor([[0, -1, 4, -1, -1]] * 2)),
               dict(k=0), dict(k=101), dict(k=2.0), dict(k=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cat.deletion_curve([0, 1], [2, 3], **kw)
    for kw in (dict(by='pair'), dict(by='mass', side='item', direction='down'), dict(by=torch.zeros(2, 5, dtype=torch.int64)),
               dict(by=torch.tensor([[T + 1, 0, -1]] * 2), k=3), dict(by=np.zeros((2, 1), np.int32), k=1)):
        with reached:
            cat.deletion_curve([0, 1], [2, 3], **kw)


@pytest.mark.parametrize('cls, mt', [('Catalogue', 'bias_only'), ('Catalogue', 'MF_dot'), ('ReluCatalogue', 'NeuMF'),
                                     ('MFCatalogue', 'MF')])
def test_a_configuration_without_a_tower_is_refused_with_the_reason(cls, mt):
    import reviews4rec_amd
    from test_phrases_host import _bare
    cat = _bare(getattr(reviews4rec_amd, cls), mt)
    for call in (cat.what_if, cat.leave_one_out, cat.deletion_curve):
        with pytest.raises(RuntimeError, match='no TextCNN tower'):
            call([0], [0])


def test_distinct_rows_fold_what_cannot_change_the_document():
    """``_whatif_rows``: bits beyond the list, reviews that are empty or start beyond the cut, repeated positions."""
    import reviews4rec_amd
    tok, rev_off, first, counts = synthetic_pool()
    pool = types.SimpleNamespace(tok=tok, rev_off=rev_off, first=first, owners=len(counts))
    cat = object.__new__(reviews4rec_amd.Catalogue)
    cat.hp = dict(input_length=5)
    ids = np.array([2, 2, 6, 1, 0], np.int64)               # the 2-review owner's first review is empty
    start = rev_off[first[6]:first[6] + 64] - rev_off[first[6]]
    far = int(np.nonzero(start >= 5)[0][0])                  # a review of the 70-review owner beyond the cut
    masks = np.array([[1, 2, 4], [3, 1, 0], [1 << far, 1 | (1 << far), 1 << 5], [2, 1, 0], [1, -1, 0]], np.int64)
    row_ids, row_drop, row_occ, index, nb = cat._whatif_rows(pool, ids, masks, None)
    assert nb == 4 and row_occ is None and row_ids[:nb].tolist() == [0, 1, 2, 6]
    base = index[:, 0].tolist()
    assert base == [2, 2, 3, 1, 0]
    assert index[0].tolist()[1:] == [2, index[0, 2], 2] and index[0, 2] >= nb      # empty review / beyond the list
    assert index[1, 2] == 2 and index[1, 3] == 2 and index[1, 1] >= nb
    assert index[2, 1] == 3 and index[2, 3] == 3 and index[2, 2] >= nb              # beyond the cut; empty
    assert index[3].tolist()[1:] == [1, index[3, 2], 1] and index[4].tolist() == [0, 0, 0, 0]
    rows = list(zip(row_ids[nb:].tolist(), row_drop[nb:].tolist()))
    assert len(set(rows)) == len(rows) and (2, 2) in rows and (2, 3) in rows
    occ = np.array([[[3, 3, -1], [-1, -1, -1]], [[-1, 3, 3], [4, 0, 4]]], np.int64)
    row_ids, row_drop, row_occ, index, nb = cat._whatif_rows(pool, np.array([2, 2], np.int64), None, occ)
    assert nb == 1 and index.tolist() == [[0, 1, 0], [0, 1, 2]]
    assert row_occ.tolist() == [[-1, -1, -1], [3, -1, -1], [4, 0, -1]] and not row_drop.any()


def test_check_explain_reviews_request_refuses_before_any_training():
    from reviews4rec_amd import check_explain_reviews_request as check
    ok = dict(model_type='deepconn', explain_reviews_k=2, explain_reviews_path='p.npz', recommend_k=3, recommend_path='r.npz')
    check(ok)
    check(dict(ok, model_type='deepconn++', catalogue_towers='device', explain_reviews_k=64))
    check(dict(model_type='NARRE'))                          # not asked for: nothing to refuse
    check(dict(ok, explain_reviews_k=0, model_type='MF'))
    for mt, word in (('MF_dot', 'no TextCNN tower'), ('MF', 'no TextCNN tower'), ('NeuMF', 'no TextCNN tower'),
                     ('bias_only', 'no TextCNN tower'), ('NARRE', 'no catalogue form'), ('transnet', 'no catalogue form'),
                     ('transnet++', 'no catalogue form')):
        with pytest.raises(RuntimeError, match=r"explain_reviews_k'\]: .*" + word):
            check(dict(ok, model_type=mt))
    for k in (65, -1, 2.0, True, '3'):
        with pytest.raises(RuntimeError, match='must be an int in 1 .. 64'):
            check(dict(ok, explain_reviews_k=k))
    for path in (None, ''):
        with pytest.raises(RuntimeError, match='explain_reviews_path'):
            check(dict(ok, explain_reviews_path=path))
    no_list = dict(ok)
    del no_list['recommend_k']
    with pytest.raises(RuntimeError, match="needs hyper_params\\['recommend_k'\\]"):
        check(no_list)
    with pytest.raises(RuntimeError, match='catalogue_towers'):
        check(dict(ok, catalogue_towers='gpu'))
