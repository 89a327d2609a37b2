"""r4r_tower_span_variants (include/r4r.h, "What-if documents") on tests/golden/tiny's user pool plus an owner without
reviews: a span over `group` rows per round leaves the bits of one r4r_tower_build_variants + r4r_textcnn_fwd +
r4r_linear_fwd call per chunk of `group` rows -- latent, pooled and argmax; with nothing removed it is
r4r_tower_span_fwd; and asking for pooled / argmax changes no bit of the latents."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T, E, F, L = 37, 20, 100, 8


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from reviews4rec_amd.data import load_data
    from test_gpu_recommend import materialise_tiny, tiny_hp
    root = materialise_tiny(tmp_path_factory.mktemp('tiny'))
    train = load_data(tiny_hp('deepconn', root), device=DEV)[0]
    p = train.store.users
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    first = np.concatenate([p.first, p.first[-1:]])          # one more owner, without a review
    owners = p.owners + 1
    pool = (t(np.concatenate([p.tok, np.zeros(1, np.int32)])), t(p.rev_off), t(first), None)
    V = int(p.tok.max()) + 1
    g = torch.Generator().manual_seed(3)
    rnd = lambda *shape: ((torch.rand(shape, generator=g) - 0.5) * 0.4).to(DEV)
    w = dict(table=rnd(V, E), conv_w=rnd(F, 1, 3, E), conv_b=rnd(F), fc_w=rnd(L, F), fc_b=rnd(L))
    rng = np.random.RandomState(4)
    count = np.diff(first)
    ids, drop, occ = [], [], []
    for o in list(range(owners)) + [owners - 1, int(count.argmax()), 0]:
        c = int(count[o])
        for mask in [0, 1, (1 << c) - 1 if c else 0] + [int(rng.randint(0, 1 << min(c, 30))) if c else 7 for _ in range(2)]:
            ids.append(o)
            drop.append(mask)
            occ.append(sorted(rng.choice(T, size=rng.randint(0, 6), replace=False).tolist()))
    order = rng.permutation(len(ids))
    pick = lambda v: [v[k] for k in order]
    lens = [len(o) for o in pick(occ)]
    rows = dict(ids=t(np.array(pick(ids), np.int64)), drop=t(np.array(pick(drop), np.int64)),
                occ_off=t(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)),
                occ_pos=t(np.array([p_ for o in pick(occ) for p_ in o] + [0], np.int32)))
    assert count[-1] == 0 and count.max() > 1 and len(ids) > 20
    return dict(pool=pool, owners=owners, w=w, rows=rows, n=len(ids), V=V)


def per_chunk(world, group, plain=False):
    """The calls the span stands for: per chunk of ``group`` rows the builder, the conv and the fc, one call each."""
    from reviews4rec_amd import ops
    r, w, n = world['rows'], world['w'], world['n']
    z, pooled, argmax = [], [], []
    for a in range(0, n, group):
        b = min(n, a + group)
        kw = {} if plain else dict(drop=r['drop'][a:b], occ_off=r['occ_off'][a:b + 1], occ_pos=r['occ_pos'])
        docs = ops.tower_build_variants(world['pool'], r['ids'][a:b], T, **kw)
        p, am = ops.textcnn_fwd_raw(docs, w['table'], w['conv_w'], w['conv_b'])
        z.append(ops.linear(p, w['fc_w'], w['fc_b']))
        pooled.append(p)
        argmax.append(am)
    return torch.cat(z), torch.cat(pooled), torch.cat(argmax)


@pytest.fixture
def pinned():
    """r4r_textcnn_algo pinned by the test, restored afterwards."""
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    prev = lib.r4r_textcnn_algo(0)
    try:
        yield lambda algo: lib.r4r_textcnn_algo(algo)
    finally:
        lib.r4r_textcnn_algo(prev)


@pytest.mark.parametrize('algo', [0, 1, 2])                  # auto, direct, project-then-gather
def test_a_span_leaves_the_bits_of_the_per_chunk_calls(world, algo, pinned):
    from reviews4rec_amd import ops
    pinned(algo)
    r, w, n = world['rows'], world['w'], world['n']
    for group in (1, 3, n, n + 5):
        want = per_chunk(world, group)
        got = ops.tower_span_variants(world['pool'], r['ids'], T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'], w['fc_b'],
                                      group, drop=r['drop'], occ_off=r['occ_off'], occ_pos=r['occ_pos'],
                                      want=('latent', 'pooled', 'argmax'))
        for name, ref in zip(('latent', 'pooled', 'argmax'), want):
            assert got[name].shape == ref.shape and torch.equal(got[name], ref), (group, name)
        alone = ops.tower_span_variants(world['pool'], r['ids'], T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'],
                                        w['fc_b'], group, drop=r['drop'], occ_off=r['occ_off'], occ_pos=r['occ_pos'])
        assert torch.equal(alone, got['latent']), group       # NULL pooled / argmax: the same latents
        for one in ('pooled', 'argmax'):
            part = ops.tower_span_variants(world['pool'], r['ids'], T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'],
                                           w['fc_b'], group, drop=r['drop'], occ_off=r['occ_off'], occ_pos=r['occ_pos'],
                                           want=('latent', one))
            assert torch.equal(part['latent'], alone) and torch.equal(part[one], got[one]), (group, one)
    assert float(want[0].abs().max()) > 0 and not torch.equal(want[0], per_chunk(world, n, plain=True)[0])


@pytest.mark.parametrize('algo', [0, 1, 2])
def test_with_nothing_removed_the_span_is_r4r_tower_span_fwd(world, algo, pinned):
    from reviews4rec_amd import _lib, ops
    from reviews4rec_amd._lib import ptr
    pinned(algo)
    lib = _lib.lib()
    r, w, n, V = world['rows'], world['w'], world['n'], world['V']
    tok, rev_off, first, _ = world['pool']
    for group in (1, 3, n, n + 5):
        want = torch.full((n, L), -7.0, device=DEV)
        ws = torch.empty(lib.r4r_tower_span_ws_bytes(min(group, n), T, 0, 0, E, F, L, V), dtype=torch.uint8, device=DEV)
        done = ctypes.c_int64(-1)
        _lib.call('r4r_tower_span_fwd', ptr(tok), ptr(rev_off), ptr(first), None, world['owners'], ptr(r['ids']), n, group,
                  T, 0, 0, 0, ptr(w['table']), V, ptr(w['conv_w']), ptr(w['conv_b']), ptr(w['fc_w']), ptr(w['fc_b']), E, F,
                  L, ptr(want), None, ptr(ws), ws.numel(), ctypes.addressof(done))
        got = ops.tower_span_variants(world['pool'], r['ids'], T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'], w['fc_b'],
                                      group)
        assert torch.equal(got, want), group
        zero = torch.zeros_like(r['drop'])
        none = torch.zeros_like(r['occ_off'])
        got = ops.tower_span_variants(world['pool'], r['ids'], T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'], w['fc_b'],
                                      group, drop=zero, occ_off=none, occ_pos=r['occ_pos'])
        assert torch.equal(got, want), group
        assert done.value == -(-n // group)


def test_the_span_counts_its_rounds_and_an_empty_span_is_a_no_op(world):
    from reviews4rec_amd import _lib, ops
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    r, w, n, V = world['rows'], world['w'], world['n'], world['V']
    tok, rev_off, first, _ = world['pool']
    latent = torch.full((n, L), -7.0, device=DEV)
    need = lib.r4r_tower_span_variants_ws_bytes(3, T, E, F, L, V)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    done = ctypes.c_int64(-1)
    args = lambda nbytes, rows: (ptr(tok), ptr(rev_off), ptr(first), world['owners'], ptr(r['ids']), ptr(r['drop']),
                                 ptr(r['occ_off']), ptr(r['occ_pos']), rows, 3, T, ptr(w['table']), V, ptr(w['conv_w']),
                                 ptr(w['conv_b']), ptr(w['fc_w']), ptr(w['fc_b']), E, F, L, ptr(latent), None, None, ptr(ws),
                                 nbytes, ctypes.addressof(done), _lib.current_stream())
    assert lib.r4r_tower_span_variants(*args(need - 1, n)) == -3 and done.value == 0
    assert lib.r4r_tower_span_variants(*args(need, 0)) == 0 and done.value == 0
    torch.cuda.synchronize()
    assert (latent == -7.0).all()
    assert lib.r4r_tower_span_variants(*args(need, n)) == 0 and done.value == -(-n // 3)
    torch.cuda.synchronize()
    assert torch.equal(latent, per_chunk(world, 3)[0])
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    assert ops.tower_span_variants(world['pool'], none, T, w['table'], w['conv_w'], w['conv_b'], w['fc_w'], w['fc_b'],
                                   3).shape == (0, L)
