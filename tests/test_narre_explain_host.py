"""NARRE explanations (include/r4r.h, "NARRE explanations"), the parts that need no GPU: r4r_narre_explain's refusals,
NarreCatalogue.explain's argument errors, the refusals of main's explain_k hook, and explain_ref -- the numpy statement
of the list rules that tests/test_gpu_narre_explain*.py hold the kernel to -- against a brute-force ordering."""
import ctypes
import itertools

import numpy as np
import pytest

NAME = b'narre_explain'
ARGS = ('z', 'nb', 'other_table', 'other_rows', 'own_table', 'owner', 'live', 'W0', 'b0', 'w3', 'b3', 'out', 'attn',
        'top_slot', 'top_w', 'K', 'N', 'R', 'L')


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


# ---------------------------------------------------------------- the reference of the lists
def explain_ref(attn, live, k):
    """The list rules of include/r4r.h over given weights ``attn`` [n, R] (float32) and ``live`` [n] (None: every slot):
    slot r is listed only if r < live[n]; weight descending, ties by ascending slot; places beyond min(k, live[n]) hold
    (-1, 0.0) -> (slots int32 [n, k], weights float32 [n, k], the bits of attn[n, slot])."""
    attn = np.asarray(attn, dtype=np.float32)
    n, R = attn.shape
    live = np.full(n, R, np.int64) if live is None else np.clip(np.asarray(live, dtype=np.int64), 0, R)
    slots = np.full((n, k), -1, np.int32)
    w = np.zeros((n, k), np.float32)
    for i in range(n):
        lv = int(live[i])
        order = np.lexsort((np.arange(lv), -attn[i, :lv].astype(np.float64)))[:k]
        slots[i, :len(order)] = order
        w[i, :len(order)] = attn[i, order]
    return slots, w


def _brute(attn_row, lv, k):
    """A place is the count of live slots ahead; the list by trying every permutation's sortedness is too slow, so:
    place by place, the slot no live slot beats."""
    left = list(range(lv))
    out = []
    while left and len(out) < k:
        best = left[0]
        for r in left[1:]:
            if attn_row[r] > attn_row[best] or (attn_row[r] == attn_row[best] and r < best):
                best = r
        out.append(best)
        left.remove(best)
    return out


def test_explain_ref_against_a_brute_force_ordering():
    rng = np.random.default_rng(3)
    for R in (1, 2, 5, 10, 64):
        attn = rng.random((40, R)).astype(np.float32)
        attn[3] = 0.25                                        # every weight equal: the slots ascend
        attn[4, ::2] = attn[4, 0]                             # ties among the even slots
        if R > 2:
            attn[5, R - 1] = attn[5, 0] = 2.0                 # the largest weight twice: slot 0 before slot R - 1
        live = rng.integers(0, R + 1, 40)
        live[0], live[1], live[3] = 0, R, R
        for k in sorted({1, min(3, R), R}):
            for lv in (live, None):
                slots, w = explain_ref(attn, lv, k)
                assert slots.dtype == np.int32 and w.dtype == np.float32 and slots.shape == w.shape == (40, k)
                for i in range(40):
                    n_live = R if lv is None else int(lv[i])
                    want = _brute(attn[i], n_live, k)
                    assert slots[i, :len(want)].tolist() == want, (R, k, i)
                    assert (slots[i, len(want):] == -1).all() and (w[i, len(want):] == 0).all()
                    assert np.array_equal(w[i, :len(want)].view(np.uint32), attn[i, want].view(np.uint32))
                    assert len(want) == min(k, n_live)
                if lv is not None:
                    assert (slots[0] == -1).all()              # live = 0: nothing listed
                assert slots[3].tolist() == list(range(k))     # all equal: ascending slots
        if R > 2:
            assert explain_ref(attn, None, 2)[0][5].tolist() == [0, R - 1]
    # k > live: the tail is the fill; a live count outside 0..R is clamped
    s, w = explain_ref(np.array([[0.1, 0.7, 0.2]], np.float32), [2], 3)
    assert s.tolist() == [[1, 0, -1]] and w.tolist() == [[np.float32(0.7), np.float32(0.1), 0.0]]
    assert explain_ref(np.array([[0.1, 0.7, 0.2]], np.float32), [9], 3)[0].tolist() == [[1, 2, 0]]
    assert explain_ref(np.array([[0.1, 0.7, 0.2]], np.float32), [-4], 3)[0].tolist() == [[-1, -1, -1]]
    # every permutation of three distinct weights
    for perm in itertools.permutations([0.5, 0.3, 0.2]):
        s, _ = explain_ref(np.array([perm], np.float32), None, 3)
        assert [perm[j] for j in s[0]] == [0.5, 0.3, 0.2]


# ---------------------------------------------------------------- the entry point
def _call(lib, **kw):
    """r4r_narre_explain with well-formed defaults (host addresses: every refusal precedes the first dereference)
    -> (rc, message, the buffer every pointer points at)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(z=p, nb=p, other_table=p, other_rows=100, own_table=p, owner=p, live=p, W0=p, b0=p, w3=p, b3=p, out=p, attn=p,
             top_slot=p, top_w=p, K=3, N=7, R=10, L=6)
    a.update(kw)
    rc = lib.r4r_narre_explain(*[a[k] for k in ARGS], None)
    return rc, lib.r4r_last_error() or b'', buf


def test_the_symbol_is_declared_exported_and_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decl = _lib.parse_header()['r4r_narre_explain']
    assert decl[0] is ctypes.c_int and decl[2] == list(ARGS) + ['stream']
    ints = {'other_rows': ctypes.c_int64, 'K': ctypes.c_int, 'N': ctypes.c_int64, 'R': ctypes.c_int, 'L': ctypes.c_int}
    for name, t in zip(decl[2], decl[1]):
        assert t is ints.get(name, ctypes.c_void_p), name
    assert hasattr(lib, 'r4r_narre_explain')
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * NARRE explanations:'):]
    assert 'NARRE.py:53-64' in section and 'not renormalised' in section


def test_refusals_precede_the_launch_and_name_the_entry_point(lib):
    cases = [(dict(N=-1), b'negative'), (dict(other_rows=-1), b'negative'),
             (dict(R=0), b'R='), (dict(R=65), b'R='), (dict(R=-3), b'R='), (dict(L=0), b'L='), (dict(L=65), b'L='),
             (dict(K=-1), b'K='), (dict(K=11), b'K='), (dict(K=65, R=64), b'K='),
             (dict(own_table=None), b'own_table'), (dict(owner=None), b'own_table'),
             (dict(top_slot=None), b'top_slot'), (dict(top_w=None), b'top_slot'),
             (dict(top_slot=None, top_w=None), b'top_slot'),                       # K = 3 with no list to write
             (dict(out=None, attn=None, top_slot=None, top_w=None, K=0), b'no output'),
             (dict(other_table=None), b'other_table')]
    cases += [({k: None}, b'null') for k in ('z', 'nb', 'W0', 'b0', 'w3', 'b3')]
    for kw, word in cases:
        rc, msg, buf = _call(lib, **kw)
        assert rc == -1 and word in msg and msg.startswith(NAME), (kw, rc, msg)
        assert buf.raw == b'\0' * 64                         # (no GPU here: a launch would have failed otherwise)


def test_nothing_to_do_is_ok(lib):
    nul = {k: None for k in ARGS if k not in ('other_rows', 'K', 'N', 'R', 'L')}
    for kw in (dict(N=0), dict(N=0, **nul), dict(N=0, K=0, **nul), dict(N=0, other_rows=0)):
        rc, msg, buf = _call(lib, **kw)
        assert rc == 0, (kw, msg)
        assert buf.raw == b'\0' * 64
    # ... but the shape is still checked
    rc, msg, _ = _call(lib, N=0, L=65)
    assert rc == -1 and msg.startswith(NAME)


# ---------------------------------------------------------------- NarreCatalogue.explain's arguments
class _Pool:
    owners = 5
    first = np.arange(6, dtype=np.int64)


class _Store:
    users = items = _Pool()


class _Reader:
    store = _Store()


def test_explains_argument_errors_are_raised_before_anything_runs():
    import reviews4rec_amd
    from reviews4rec_amd import Explanation, NarreCatalogue
    assert Explanation._fields == ('slots', 'reviews', 'reviewers', 'weights', 'attention', 'live')
    assert reviews4rec_amd.recommend.Explanation is Explanation
    cat = object.__new__(NarreCatalogue)                      # no device: the checks come before the first use of one
    cat.hp, cat.reader, cat.model = dict(narre_num_reviews=10), _Reader(), None
    cat.n_users = cat.n_items = 5

    class Loud:
        def flush(self):
            raise AssertionError('flushed before the arguments were checked')

    cat.engine = Loud()
    for side in ('items', 'pair', None, 0):
        with pytest.raises(ValueError, match='side'):
            cat.explain([0], side=side)
    for k in (0, -1, 11, 2.0, True, None):
        with pytest.raises(ValueError, match='explain k'):
            cat.explain([0], k=k)
    for side in ('item', 'user'):
        for ids in ([5], [-1], [0, 7]):
            with pytest.raises(KeyError):
                cat.explain(ids, k=3, side=side)
    assert 'nothing is renormalised over the live slots' in ' '.join(NarreCatalogue.explain.__doc__.split())


# ---------------------------------------------------------------- main's hook
@pytest.mark.parametrize('entry', ['main', 'main_pytorch', 'main_NeuMF'])
def test_explain_k_is_refused_before_anything_is_loaded(entry):
    """Every entry of main.py says so at once: a model type other than NARRE (narre_catalogue_limits' reason), a NARRE
    shape the class cannot serve, a request without a file."""
    from reviews4rec_amd import main as M
    from reviews4rec_amd.recommend import check_explain_request, narre_catalogue_limits
    fn = getattr(M, entry)
    other = 'NeuMF' if entry == 'main_NeuMF' else 'deepconn'
    hp = dict(model_type=other, latent_size=8, explain_k=3, explain_path='why.npz', data_dir='/nonexistent/')
    why = narre_catalogue_limits(hp)
    assert isinstance(why, str) and 'serves it' in why
    with pytest.raises(RuntimeError) as e:
        fn(hp)
    assert str(e.value) == "hyper_params['explain_k']: " + why
    if entry != 'main_NeuMF':
        with pytest.raises(RuntimeError, match='latent_size 65 > 64'):
            fn(dict(model_type='NARRE', latent_size=65, narre_num_reviews=10, explain_k=3, explain_path='why.npz',
                    data_dir='/nonexistent/'))
        with pytest.raises(RuntimeError, match='explain_path'):
            fn(dict(model_type='NARRE', latent_size=8, narre_num_reviews=10, explain_k=3, data_dir='/nonexistent/'))
        for k in (11, -1, 2.5, True):
            with pytest.raises(RuntimeError, match='explain_k'):
                fn(dict(model_type='NARRE', latent_size=8, narre_num_reviews=10, explain_k=k, explain_path='why.npz',
                        data_dir='/nonexistent/'))
    # no request, no check; and the existing hooks still refuse NARRE
    assert check_explain_request(dict(model_type='deepconn')) is None
    assert check_explain_request(dict(model_type='NARRE', latent_size=64, narre_num_reviews=10, explain_k=3,
                                      explain_path='why.npz')) is None
    with pytest.raises(RuntimeError, match='no catalogue form'):
        M.main(dict(model_type='NARRE', latent_size=8, narre_num_reviews=10, recommend_k=3, recommend_path='lists.npz',
                    data_dir='/nonexistent/'))
