"""r4r_tower_span_phrases on the device (include/r4r.h, "Phrase explanations"; csrc/tower_span.hip), in the form of
tests/test_gpu_tower_span.py: over the pools of tests/golden/tiny, for the document layout and for NARRE's [R, W] review
layout, a span over `group` owners per round must leave, bit for bit, what the per-chunk host path leaves --
data._np_docs / _np_reviews -> ops.textcnn_fwd_raw -> ops.textcnn_phrases, one call each per chunk of `group` owners."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 5
NAMES = ('pos', 'score', 'filt', 'tok', 'win')


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    """(hp, item pool with one more owner who has no review, tower, word table) of the deepconn fixture."""
    from test_gpu_narre_explain_catalogue import _with_an_empty_owner
    from test_gpu_tower_span import _tiny
    _, hp, train, _, model = _tiny('deepconn', tmp_path_factory.mktemp('tiny'))
    pool = _with_an_empty_owner(train.store.items)
    assert pool.first[-1] == pool.first[-2] and pool.owners == hp['total_items'] + 1
    return hp, pool, model.item_conv, model.word2vec.weight.detach()


def the_ids(pool):
    """Out of order, with repeats, the owner without reviews (the last), ids outside the pool on both sides."""
    o = pool.owners
    return np.array([3, o - 1, 0, 3, o, 7, -1, o - 2, 3, 1, 0, 1 << 40, 5], dtype=np.int64)


def host_path(hp, pool, tower, table, ids, group, narre, wt):
    """The per-chunk loop: numpy documents (an id outside the pool: an owner without reviews), one textcnn_fwd_raw and
    one textcnn_phrases call per chunk."""
    from reviews4rec_amd import ops
    from reviews4rec_amd.data import _np_docs, _np_reviews
    conv = tower.convs[0]
    R, W, T = int(hp['narre_num_reviews']), int(hp['narre_num_words']), int(hp['input_length'])
    per = R if narre else 1
    out = [[] for _ in NAMES]
    for s in range(0, len(ids), group):
        chunk = ids[s:s + group]
        known = (chunk >= 0) & (chunk < pool.owners)
        safe = np.where(known, chunk, 0)
        rb, re = np.where(known, pool.first[safe], 0), np.where(known, pool.first[safe + 1], 0)
        none = np.full(len(chunk), -1, np.int64)
        if narre:
            docs = _np_reviews(pool.tok, pool.rev_off, rb, re, none, R, W).reshape(len(chunk) * R, W)
        else:
            docs = _np_docs(pool.tok, pool.rev_off, rb, re, none, T)
        docs = torch.from_numpy(docs).to(DEV)
        pooled, argmax = ops.textcnn_fwd_raw(docs, table, conv.weight.detach(), conv.bias.detach())
        w = wt if wt is None or wt.dim() == 1 else wt[s * per:(s + len(chunk)) * per]
        for acc, t in zip(out, ops.textcnn_phrases(pooled, argmax, K, W if narre else T, weights=w, idx=docs)):
            acc.append(t)
    torch.cuda.synchronize()
    return {k: torch.cat(v).cpu() for k, v in zip(NAMES, out)}


def span(hp, pool, tower, table, ids, group, narre, wt, ws_bytes=None, want=NAMES):
    """One r4r_tower_span_phrases call, the outputs pre-filled with -7 -> (rc, rounds enqueued, dict of host tensors)."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    conv = tower.convs[0]
    R, W, T = (int(hp['narre_num_reviews']), int(hp['narre_num_words']), 0) if narre else (0, 0, int(hp['input_length']))
    n, rows = len(ids), len(ids) * max(R, 1)
    V, E = table.shape
    F = conv.bias.numel()
    dev = torch.device(DEV, torch.cuda.current_device())
    tok, rev_off, first, nb = pool.device(dev)
    dev_ids = torch.from_numpy(ids).to(DEV)
    shapes = dict(pos=((rows, K), torch.int32), score=((rows, K), torch.float32), filt=((rows, K), torch.int32),
                  tok=((rows, K, 3), torch.int64), win=((rows,), torch.int32))
    out = {k: torch.full(s, -7, dtype=t, device=DEV) for k, (s, t) in shapes.items() if k in want}
    neigh = torch.empty((n, 10), dtype=torch.int64, device=DEV) if narre else None
    need = lib.r4r_tower_span_ws_bytes(min(group, n), T, R, W, E, F, int(tower.fc.weight.shape[0]), V)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    done = ctypes.c_int64(-1)
    cw, cb = conv.weight.detach().contiguous(), conv.bias.detach().contiguous()
    rc = lib.r4r_tower_span_phrases(ptr(tok), ptr(rev_off), ptr(first), ptr(nb), pool.owners, ptr(dev_ids), n, group, T, R, W,
                                    77, ptr(table), V, ptr(cw), ptr(cb), E, F, ptr(wt),
                                    0 if wt is None or wt.dim() == 1 else F, K, *[ptr(out.get(k)) for k in NAMES],
                                    ptr(neigh), ptr(ws), need if ws_bytes is None else ws_bytes, ctypes.byref(done),
                                    _lib.current_stream())
    torch.cuda.synchronize()
    return rc, done.value, {k: v.cpu() for k, v in out.items()}


def weights_of(form, rows, F):
    g = torch.Generator().manual_seed(3)
    if form == 'none':
        return None
    return (torch.randn((F,) if form == 'shared' else (rows, F), generator=g)).to(DEV)


@pytest.mark.parametrize('form', ['none', 'shared', 'per_row'])
@pytest.mark.parametrize('narre', [False, True], ids=['documents', 'reviews'])
def test_a_span_leaves_the_bits_of_the_per_chunk_host_path(tiny, narre, form):
    hp, pool, tower, table = tiny
    ids = the_ids(pool)
    n = len(ids)
    per = int(hp['narre_num_reviews']) if narre else 1
    wt = weights_of(form, n * per, 100)
    seen = None
    for group in (1, 3, n, n + 5):
        want = host_path(hp, pool, tower, table, ids, group, narre, wt)
        rc, done, got = span(hp, pool, tower, table, ids, group, narre, wt)
        assert rc == 0 and done == -(-n // group), (group, done)
        for k in NAMES:
            a, b = got[k], want[k]
            assert a.dtype == b.dtype and a.shape == b.shape, (group, k)
            assert torch.equal(a.view(torch.int32) if k == 'score' else a, b.view(torch.int32) if k == 'score' else b), (group, k)
        if seen is None:
            seen = got
    # the cases are what they say: real windows and real words; nothing for the owner without reviews but the document
    # of pad words (the conv still pools its bias); the ids outside the pool read as that owner
    pos, tok, win = seen['pos'].view(n, per, K), seen['tok'].view(n, per, K, 3), seen['win'].view(n, per)
    assert int(win[0].max()) > 1 and int(tok[0].max()) > 0 and (seen['pos'] != -7).all() and (seen['win'] != -7).all()
    empty = 1                                                 # ids[1] = owners - 1
    assert int(tok[empty].max()) <= 0
    for outside in (4, 6, 11):
        assert torch.equal(win[outside], win[empty]) and int(tok[outside].max()) <= 0
    assert torch.equal(win[0], win[3]) and torch.equal(win[0], win[8]) and torch.equal(win[2], win[10])   # the repeats
    if form != 'per_row':                                     # (rows with weights of their own rank the same windows apart)
        for outside in (4, 6, 11):
            assert torch.equal(pos[outside], pos[empty]) and torch.equal(tok[outside], tok[empty])
        assert torch.equal(pos[0], pos[3]) and torch.equal(pos[0], pos[8]) and torch.equal(tok[2], tok[10])


def test_the_span_counts_its_rounds_refuses_a_short_workspace_and_takes_null_outputs(tiny):
    from reviews4rec_amd import _lib
    hp, pool, tower, table = tiny
    ids = the_ids(pool)
    lib = _lib.lib()
    need = lib.r4r_tower_span_ws_bytes(3, int(hp['input_length']), 0, 0, table.shape[1], 100, 6, table.shape[0])
    rc, done, got = span(hp, pool, tower, table, ids, 3, False, None, ws_bytes=need - 1)
    assert rc == -3 and done == 0 and b'r4r_tower_span_phrases' in lib.r4r_last_error()
    assert all((t == -7).all() for t in got.values())       # nothing was enqueued
    whole = span(hp, pool, tower, table, ids, 3, False, None)[2]
    rc, done, got = span(hp, pool, tower, table, ids, 3, False, None, want=('pos', 'win'))
    assert rc == 0 and done == 5 and torch.equal(got['pos'], whole['pos']) and torch.equal(got['win'], whole['win'])
