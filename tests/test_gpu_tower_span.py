"""Tower spans on the device (include/r4r.h "Tower spans": r4r_tower_build, r4r_tower_span_fwd, csrc/tower_span.hip;
recommend.Catalogue(towers='device') on top of them).

The builder must write, integer for integer, what the host evaluates with data._np_docs / _np_reviews / _np_neighbours
and nothing removed; a span over `group` owners per round must leave the bits of the per-chunk
``_tower(_documents(...))`` loop with tower_batch == group (the same kernels with the same arguments, and the conv's
algorithm resolved from the same N); and a catalogue built with towers='device' must hold, list and rank exactly what
the one built with towers='host' does, and leave the training state where it found it."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NB = 10


# ---------------------------------------------------------------- synthetic pools
def make_pool(review_lens, vocab=400, others=50, seed=0):
    """A data._Pool whose owner o holds reviews of ``review_lens[o]`` tokens; nb holds random ids of the other side."""
    from reviews4rec_amd.data import _Pool
    rng = np.random.default_rng(seed)
    reviews = {o: [rng.integers(1, vocab, size=n).tolist() for n in lens] for o, lens in enumerate(review_lens) if lens}
    pool = _Pool(reviews, len(review_lens))
    pool.nb[:] = rng.integers(0, others, size=len(pool.nb))
    return pool


# owner: 0 none | 1 one short review | 2 three reviews, 24 tokens | 3 fifteen reviews of 30 (450 tokens > 300) |
# 4 exactly ten reviews, some longer than W = 16 | 5 eleven one-token reviews | 6 none | 7 (the last) twelve mixed
LENS = [[], [5], [3, 17, 4], [30] * 15, [1, 16, 17, 40, 2, 15, 33, 16, 9, 64], [1] * 11, [], [20, 2, 41, 16, 1, 7, 39, 3, 18, 5, 50, 6]]
IDS = {'every owner': list(range(8)), 'unordered with repeats': [7, 3, 3, 0, 5, 7, 1, 6, 4, 2, 7], 'one': [3],
       'the last owner': [7], 'an owner without reviews': [6]}


def device_build(pool, ids, T=0, R=0, W=0, pad=0, owners=None):
    """r4r_tower_build over ``ids`` -> (docs, neigh or None) on the host; the outputs start as -7 everywhere."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    tok, rev_off, first, nb = pool.device(torch.device(DEV, torch.cuda.current_device()))
    n = len(ids)
    dev_ids = torch.tensor(list(ids), dtype=torch.int64, device=DEV)
    docs = torch.full((n, R, W) if R else (n, T), -7, dtype=torch.int64, device=DEV)
    neigh = torch.full((n, NB), -7, dtype=torch.int64, device=DEV) if R else None
    _lib.call('r4r_tower_build', ptr(tok), ptr(rev_off), ptr(first), ptr(nb), pool.owners if owners is None else owners,
              ptr(dev_ids), n, T, R, W, pad, ptr(docs), ptr(neigh))
    torch.cuda.synchronize()
    return docs.cpu(), (None if neigh is None else neigh.cpu())


def host_build(pool, ids, T=0, R=0, W=0, pad=0):
    from reviews4rec_amd.data import _np_docs, _np_neighbours, _np_reviews
    ids = np.asarray(ids, dtype=np.int64)
    rb, re, none = pool.first[ids], pool.first[ids + 1], np.full(len(ids), -1, np.int64)
    if R:
        return (torch.from_numpy(_np_reviews(pool.tok, pool.rev_off, rb, re, none, R, W)),
                torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, pad)))
    return torch.from_numpy(_np_docs(pool.tok, pool.rev_off, rb, re, none, T)), None


@pytest.mark.parametrize('which', sorted(IDS))
@pytest.mark.parametrize('T', [37, 300])
def test_the_builder_writes_the_host_s_documents(T, which):
    pool, ids = make_pool(LENS), IDS[which]
    got, _ = device_build(pool, ids, T=T)
    want, _ = host_build(pool, ids, T=T)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    if which == 'every owner':                               # the cases are what they say
        lens = (want != 0).sum(1).tolist()
        assert lens[0] == 0 and lens[1] == 5 and lens[2] == 24 and lens[3] == min(T, 450) and lens[7] > 0


@pytest.mark.parametrize('which', sorted(IDS))
@pytest.mark.parametrize('R, W', [(10, 16), (3, 5)])
def test_the_builder_writes_the_host_s_reviews_and_neighbours(R, W, which):
    pool, ids, pad = make_pool(LENS), IDS[which], 51
    got, got_nb = device_build(pool, ids, R=R, W=W, pad=pad)
    want, want_nb = host_build(pool, ids, R=R, W=W, pad=pad)
    assert torch.equal(got, want) and torch.equal(got_nb, want_nb)
    if which == 'every owner' and R == 10:
        assert (want_nb[0] == pad).all() and (want_nb[2] == pad).sum() == 7 and (want_nb[3] != pad).all()
        assert (want_nb[4] != pad).all() and (want_nb[7] != pad).all()          # ten and twelve reviews: no pad
        assert (want[4, 3] != 0).all() and (want[1, 1:] == 0).all()             # a review cut at W, missing slots


def test_the_builder_on_an_empty_pool():
    """No review anywhere: len(rev_off) < 2, every document is zero and every neighbour the pad id."""
    pool = make_pool([[], [], [], [], []])
    assert len(pool.rev_off) < 2
    for ids in ([0, 4, 2, 2], [4]):
        got, _ = device_build(pool, ids, T=37)
        assert torch.equal(got, host_build(pool, ids, T=37)[0]) and (got == 0).all()
        got, got_nb = device_build(pool, ids, R=10, W=16, pad=9)
        want, want_nb = host_build(pool, ids, R=10, W=16, pad=9)
        assert torch.equal(got, want) and torch.equal(got_nb, want_nb) and (got_nb == 9).all()


def test_an_id_outside_the_pool_is_an_owner_without_reviews():
    pool = make_pool(LENS)
    ids = [3, -1, 8, 7, 13, 1 << 40, -(1 << 40), 2]          # owners = 8: 8 is the first id past the pool
    known = [k for k, o in enumerate(ids) if 0 <= o < 8]
    got, _ = device_build(pool, ids, T=37)
    got_r, got_nb = device_build(pool, ids, R=10, W=16, pad=77)
    for k in range(len(ids)):
        if k in known:
            assert torch.equal(got[k], host_build(pool, [ids[k]], T=37)[0][0])
            want, want_nb = host_build(pool, [ids[k]], R=10, W=16, pad=77)
            assert torch.equal(got_r[k], want[0]) and torch.equal(got_nb[k], want_nb[0])
        else:
            assert (got[k] == 0).all() and (got_r[k] == 0).all() and (got_nb[k] == 77).all(), ids[k]
    # `owners` is the argument's: the same pool seen as three owners has nothing for owner 3
    got, _ = device_build(pool, [2, 3], T=37, owners=3)
    assert torch.equal(got[0], host_build(pool, [2], T=37)[0][0]) and (got[1] == 0).all()


def test_an_empty_build_is_a_no_op():
    pool = make_pool(LENS)
    for kw in (dict(T=37), dict(R=10, W=16, pad=3)):
        docs, neigh = device_build(pool, [], **kw)
        assert docs.shape[0] == 0 and (neigh is None or neigh.shape[0] == 0)
    from reviews4rec_amd import _lib
    out = torch.full((4, 37), -7, dtype=torch.int64, device=DEV)
    _lib.call('r4r_tower_build', None, None, None, None, 8, None, 0, 37, 0, 0, 0, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert (out == -7).all()


# ---------------------------------------------------------------- the span against the per-chunk loop
N_SPAN, T_SPAN, L_SPAN, F_SPAN, V_SPAN = 70, 64, 8, 100, 400


def span_lens(n, seed):
    """n owners: none, short, and longer than T = 64 / more than R = 10 reviews, reviews around W = 16."""
    rng = np.random.default_rng(seed)
    return [[] if o % 9 == 4 else rng.integers(1, 40, size=int(rng.integers(1, 15))).tolist() for o in range(n)]


def bare_catalogue(E, group, seed=0):
    """A Catalogue with nothing but what ``_tower`` / ``_documents`` / ``_span_latents`` read: a word table, one tower."""
    from reviews4rec_amd.recommend import Catalogue
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: ((torch.rand(shape, generator=g) - 0.5) * 0.4).to(DEV)
    tower = types.SimpleNamespace(convs=[types.SimpleNamespace(weight=rnd(F_SPAN, 1, 3, E), bias=rnd(F_SPAN))],
                                  fc=types.SimpleNamespace(weight=rnd(L_SPAN, F_SPAN), bias=rnd(L_SPAN)))
    cat = object.__new__(Catalogue)
    cat.hp = dict(input_length=T_SPAN, narre_num_reviews=10, narre_num_words=16)
    cat.dev, cat.tower_batch, cat.towers = torch.device(DEV, torch.cuda.current_device()), group, 'device'
    cat.model = types.SimpleNamespace(word2vec=types.SimpleNamespace(weight=rnd(V_SPAN, E)))
    return cat, tower


def host_loop(cat, tower, pool, ids, narre_pad=None):
    """The loop the span replaces: per tower_batch chunk, documents from numpy, one ``_tower`` call."""
    from reviews4rec_amd.data import _np_neighbours, _np_reviews
    z, nbs = [], []
    for _, chunk in cat._batches(ids):
        if narre_pad is None:
            z.append(cat._tower(tower, cat._documents(pool, chunk)))
            continue
        rb, re, none = pool.first[chunk], pool.first[chunk + 1], np.full(len(chunk), -1, np.int64)
        rev = _np_reviews(pool.tok, pool.rev_off, rb, re, none, 10, 16)
        z.append(cat._tower(tower, torch.from_numpy(rev.reshape(len(chunk) * 10, 16)).to(DEV)))
        nbs.append(torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, narre_pad)).to(DEV))
    return torch.cat(z), (torch.cat(nbs) if nbs else None)


@pytest.fixture
def pinned():
    """r4r_textcnn_algo pinned by the test, restored afterwards."""
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    prev = lib.r4r_textcnn_algo(0)
    yield lambda algo: lib.r4r_textcnn_algo(algo)
    lib.r4r_textcnn_algo(prev)


@pytest.mark.parametrize('algo', [0, 1, 2])                  # auto, direct, project-then-gather
@pytest.mark.parametrize('E', [20, 50])                      # 50: the zero-padded table and conv weight
def test_a_span_leaves_the_bits_of_the_per_chunk_loop(E, algo, pinned):
    pool = make_pool(span_lens(N_SPAN, 5), vocab=V_SPAN, seed=6)
    ids = np.random.default_rng(7).permutation(N_SPAN).astype(np.int64)
    ids[3] = ids[40]                                         # a repeat
    pinned(algo)
    for group in (32, 100, 1):                               # rounds of 32, 32, 6; one round; one owner per round
        cat, tower = bare_catalogue(E, group)
        want, _ = host_loop(cat, tower, pool, ids)
        got = cat._span_latents(tower, pool, ids)
        torch.cuda.synchronize()
        assert got.shape == (N_SPAN, L_SPAN) and torch.equal(got, want), (group, float((got - want).abs().max()))
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize('algo', [1, 2])
@pytest.mark.parametrize('E', [20, 50])
def test_a_narre_span_leaves_the_bits_of_the_per_chunk_loop(E, algo, pinned):
    pool = make_pool(span_lens(N_SPAN, 8), vocab=V_SPAN, seed=9)
    ids = np.random.default_rng(10).permutation(N_SPAN).astype(np.int64)
    pinned(algo)
    for group in (32, 100, 1):
        cat, tower = bare_catalogue(E, group)
        want, want_nb = host_loop(cat, tower, pool, ids, narre_pad=51)
        got, got_nb = cat._span_latents(tower, pool, ids, narre_pad=51)
        torch.cuda.synchronize()
        assert got.shape == (N_SPAN * 10, L_SPAN) and torch.equal(got, want), group
        assert got_nb.shape == (N_SPAN, NB) and torch.equal(got_nb, want_nb), group


def test_the_span_counts_its_rounds_and_refuses_a_short_workspace_on_the_device():
    """The C entry as a binder calls it: groups_done, and a refusal that leaves latent untouched."""
    import ctypes
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    pool = make_pool(span_lens(N_SPAN, 5), vocab=V_SPAN, seed=6)
    cat, tower = bare_catalogue(20, 32)
    tok, rev_off, first, nb = pool.device(cat.dev)
    ids = torch.arange(N_SPAN, dtype=torch.int64, device=DEV)
    latent = torch.full((N_SPAN, L_SPAN), -7.0, device=DEV)
    need = lib.r4r_tower_span_ws_bytes(32, T_SPAN, 0, 0, 20, F_SPAN, L_SPAN, V_SPAN)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    done = ctypes.c_int64(-1)
    conv = tower.convs[0]
    args = lambda nbytes: (ptr(tok), ptr(rev_off), ptr(first), ptr(nb), pool.owners, ptr(ids), N_SPAN, 32, T_SPAN, 0, 0, 0,
                           ptr(cat._words()), V_SPAN, ptr(conv.weight), ptr(conv.bias), ptr(tower.fc.weight),
                           ptr(tower.fc.bias), 20, F_SPAN, L_SPAN, ptr(latent), None, ptr(ws), nbytes, ctypes.byref(done),
                           _lib.current_stream())
    assert lib.r4r_tower_span_fwd(*args(need - 1)) == -3 and done.value == 0
    torch.cuda.synchronize()
    assert (latent == -7.0).all()
    assert lib.r4r_tower_span_fwd(*args(need)) == 0 and done.value == 3
    torch.cuda.synchronize()
    assert torch.equal(latent, host_loop(cat, tower, pool, np.arange(N_SPAN, dtype=np.int64))[0])


def test_an_id_outside_the_pools_is_a_key_error_before_anything_is_enqueued():
    pool = make_pool(span_lens(N_SPAN, 5), vocab=V_SPAN, seed=6)
    cat, tower = bare_catalogue(20, 32)
    for bad in ([0, N_SPAN], [-1, 3]):
        with pytest.raises(KeyError, match='outside the review pools'):
            cat._span_latents(tower, pool, np.array(bad, dtype=np.int64))
    assert cat._span_latents(tower, pool, np.zeros(0, np.int64)).shape == (0, L_SPAN)


# ---------------------------------------------------------------- the classes on tests/golden/tiny
def _tiny(mt, tmp_path):
    """(class, hp, train, test, model) with the fixtures' trained weights, through the catalogue tests' own helpers."""
    from reviews4rec_amd import Catalogue, NarreCatalogue, ReluCatalogue, TransNetCatalogue
    if mt == 'deepconn':
        from test_gpu_recommend import _tiny_model
        return (Catalogue,) + _tiny_model(mt, tmp_path)[:4]
    if mt == 'deepconn++':
        from test_gpu_relu_catalogue import _tiny as relu_tiny
        return (ReluCatalogue,) + relu_tiny(mt, None, tmp_path)[:4]
    if mt == 'NARRE':
        from test_gpu_narre_catalogue import _tiny as narre_tiny
        return (NarreCatalogue,) + narre_tiny(tmp_path)[:4]
    from test_gpu_transnet_catalogue import _tiny as transnet_tiny
    return (TransNetCatalogue,) + transnet_tiny(mt, tmp_path)[:4]


HEADS = {'deepconn': (), 'deepconn++': ('w',), 'NARRE': ('W', 'b', 'w'), 'transnet': ('W', 'b', 's', 'l'),
         'transnet++': ('W', 'b', 's', 'l')}


def same_catalogue(dev, host, head, users, pairs, candidates=None):
    """Everything a catalogue holds and answers, bit for bit (NaN-free: torch.equal)."""
    assert dev.towers == 'device' and host.towers == 'host'
    assert torch.equal(dev.c, host.c) and torch.equal(dev.c_bias, host.c_bias)
    assert torch.isfinite(dev.c).all() and torch.isfinite(dev.c_bias[torch.from_numpy(dev.eligible).to(DEV)]).all()
    for name in head:
        assert torch.equal(getattr(dev, name), getattr(host, name)), name
    for exclude in (True, False):
        for k in (1, 5):
            a, b = dev.recommend(users, k=k, exclude_seen=exclude), host.recommend(users, k=k, exclude_seen=exclude)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (exclude, k)
    assert (a[0][:, 0] >= 0).all()
    pu, pi = pairs
    assert torch.equal(dev.score_pairs(pu, pi), host.score_pairs(pu, pi))
    for exclude in (True, False):
        a, b = dev.rank(pu, pi, exclude_seen=exclude), host.rank(pu, pi, exclude_seen=exclude)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), exclude


@pytest.mark.parametrize('mt', ['deepconn', 'deepconn++', 'transnet', 'transnet++', 'NARRE'])
def test_device_towers_give_the_host_catalogue_on_tiny(mt, tmp_path):
    from reviews4rec_amd import eval_catalogue
    cls, hp, train, test, model = _tiny(mt, tmp_path)
    U, I = int(hp['total_users']), int(hp['total_items'])
    assert U > 6 and I > 6                                   # tower_batch = 3: several rounds and a ragged last one
    dev, host = (cls(model, hp, train, tower_batch=3, towers=t) for t in ('device', 'host'))
    users = np.array([U - 1, 0, 3, 0, 2, U - 1, 1, 3, 3, 5], dtype=np.int64)     # duplicates, out of order
    assert len(dev.eligible) > 3 and len(users) % 3 == 1     # rounds of 3, 3, 3 and 1
    pu, pi = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    same_catalogue(dev, host, HEADS[mt], users, (pu, pi))
    same_catalogue(dev, host, HEADS[mt], np.arange(U, dtype=np.int64), (pu[::-1].copy(), pi[::-1].copy()))
    # a candidates= subset
    few = dev.eligible[::2]
    dev2, host2 = (cls(model, hp, train, tower_batch=3, towers=t, candidates=few) for t in ('device', 'host'))
    assert dev2.eligible.tolist() == few.tolist()
    same_catalogue(dev2, host2, HEADS[mt], users, (pu, pi))
    # the metrics of a whole split
    a, b = (eval_catalogue(model, train, test, hp, ks=(1, 5), catalogue=c) for c in (dev, host))
    assert a == b and a['cat_ranked'] > 0
    # refresh() again: the same cache
    c0 = dev.c.clone()
    dev.refresh()
    assert torch.equal(dev.c, c0)


@pytest.mark.parametrize('mt', ['deepconn', 'NARRE'])
def test_device_towers_over_many_rounds(mt):
    """300 users / 120 items at tower_batch = 16: a refresh of eight rounds, queries of nineteen, ragged last ones."""
    from reviews4rec_amd import Catalogue, NarreCatalogue
    from test_gpu_span import build, tiny_corpus
    hp, reader, model, _ = build(mt, tiny_corpus(seed=61))
    model.eval()
    cls = NarreCatalogue if mt == 'NARRE' else Catalogue
    dev, host = (cls(model, hp, reader, tower_batch=16, towers=t) for t in ('device', 'host'))
    assert len(dev.eligible) > 48 and 300 % 16             # more than three rounds of items; the users' last round is ragged
    rng = np.random.default_rng(62)
    pu, pi = rng.integers(0, 300, 500), rng.integers(0, 120, 500)
    same_catalogue(dev, host, HEADS[mt], np.arange(300, dtype=np.int64)[::-1].copy(), (pu, pi))


def test_catalogues_without_a_tower_take_either_value(tmp_path):
    from reviews4rec_amd import Catalogue
    from test_gpu_recommend import _tiny_model
    hp, train, test, model, _ = _tiny_model('MF_dot', tmp_path)
    dev, host = (Catalogue(model, hp, train, towers=t) for t in ('device', 'host'))
    U = int(hp['total_users'])
    users = np.arange(U, dtype=np.int64)
    same_catalogue(dev, host, (), users, (users, np.zeros(U, np.int64)))


# ---------------------------------------------------------------- the training state
def test_a_device_tower_pass_leaves_the_deepconn_training_state():
    """Train, refresh() + recommend with towers='device', continue == training never interrupted: weights, moments,
    offset, step_count, bit for bit (the fifth step's announced token batch is pending when the pass starts; dropout
    0.5: a moved stream would show)."""
    from reviews4rec_amd import Catalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=52)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('deepconn', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = Catalogue(model, hp, reader, engine=engine, tower_batch=50, towers='device')
            cat.refresh()
            ids, sc = cat.recommend(np.arange(300), k=5)
            assert (ids[:, 0] >= 0).all() and torch.isfinite(sc[:, 0]).all() and model.training
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K
