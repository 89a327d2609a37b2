"""The document fold on the device (include/r4r.h, "Document fold"; csrc/tower_fold.hip): r4r_fold_project against a
float64 product element by element, r4r_fold_segments and r4r_fold_compose bit for bit against tower_fold_ref.py
evaluated in numpy fp32 from the device's own ptab -- the brute force over every window of
``tower_variants_ref.variant_doc``'s document --, a row's independence of its call, and both the fold and the tower
(``ops.textcnn_fwd_raw``) against the float64 conv of conv_ref.py."""
import numpy as np
import pytest
import torch

import tower_fold_ref as R
from conv_ref import check_pool, conv64, fp32_coef
from tower_variants_ref import COUNTS, as_signed, synthetic_pool, variant_docs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL = (1 << 64) - 1
V, E, F = 1000, 8, 100
TS = (1, 2, 3, 5, 37, 300)

# owners appended to the synthetic pool's seven (0, 1, 2, 63, 64, 65 and 70 reviews): their review lengths
EDGE = ([0, 1, 2, 3, 0, 3, 2, 1, 0, 4, 5],                 # 0 .. 3 words next to each other
        [3, 3, 3],                                          # T = 3: on a boundary; 5 and 4: two words and one word in
        [1, 1, 1, 1, 1],                                    # one-word reviews: the token two back is another review's
        [2, 1, 2],
        [2, 2, 1],                                          # kept lengths T - 1, T - 2, T - 3 and 0 at T = 5
        [1] * 66,                                           # a tail of two one-word reviews
        [0] * 64 + [7],                                     # nothing but the tail
        [130, 61, 62, 63, 64, 65, 3],                       # around the 60 windows one read of 64 tokens serves
        [300],                                              # cut by every T
        [35, 2])                                            # T = 37: the second review ends on it


def _pool():
    tok, rev_off, first, counts = synthetic_pool()
    rng = np.random.RandomState(11)
    lens = np.concatenate([np.diff(rev_off)] + [np.array(l, np.int64) for l in EDGE])
    counts = list(int(c) for c in counts) + [len(l) for l in EDGE]
    extra = rng.randint(0, V, size=int(sum(sum(l) for l in EDGE))).astype(np.int32)        # word 0 among them
    tok = np.concatenate([tok, extra])
    rev_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return tok, rev_off, first, counts


def _rows(counts):
    """[(owner, mask)]: nothing removed, every single bit, bits beyond the list, all bits, all but one, every subset of
    a short list."""
    rows = []
    for o, c in enumerate(counts):
        live = min(c, 64)
        rows += [(o, 0)] + [(o, 1 << s) for s in range(64)]
        rows += [(o, ALL >> c << c if c < 64 else 0), (o, ALL), (o, (1 << live) - 1)]
        rows += [(o, ALL & ~(1 << s)) for s in sorted({0, 1, live // 2, max(live - 1, 0), 63})]
        if c <= 5:
            rows += [(o, m) for m in range(1 << c)]
        rows += [(o, 0x5555555555555555), (o, 0xF0F0F0F0F0F0F0F0 | 5)]
    return rows


@pytest.fixture(scope='module')
def setup():
    from reviews4rec_amd import ops
    tok, rev_off, first, counts = _pool()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    g = torch.Generator().manual_seed(5)
    table = torch.randn(V, E, generator=g)
    table[0] = 0                                            # the padding word
    conv_w = torch.randn(F, 1, 3, E, generator=g) * 0.3
    conv_b = torch.randn(F, generator=g) * 0.1
    dev = (t(np.concatenate([tok, np.zeros(1, np.int32)])), t(rev_off), t(first), None)
    ptab = ops.fold_project(table.to(DEV), conv_w.to(DEV))
    P, b = R.ptab3(ptab.cpu().numpy(), F), conv_b.numpy()
    ids = np.arange(len(counts), dtype=np.int64)
    S = max(min(c, 64) for c in counts)
    seg = ops.fold_segments(ptab, conv_b.to(DEV), dev, t(ids), S)
    rows = _rows(counts)
    return dict(host=(tok, rev_off, first), dev=dev, counts=counts, table=table, conv_w=conv_w, conv_b=conv_b, ptab=ptab,
                P=P, b=b, ids=ids, S=S, seg=seg, rows=rows, t=t, ref={})


def _reference(s, T):
    """The brute force over the rows' documents, computed once per T and left unchanged."""
    if T not in s['ref']:
        tok, rev_off, first = s['host']
        docs = variant_docs(tok, rev_off, first, [r[0] for r in s['rows']], [r[1] for r in s['rows']], None, T)
        want = R.brute_docs(s['P'], s['b'], docs)
        want.setflags(write=False)
        s['ref'][T] = (docs, want)
    return s['ref'][T]


def _compose(s, rows, T, seg=None, ids=None, drop_null=False, owner_of=None):
    from reviews4rec_amd import ops
    t = s['t']
    owner = np.array([r[0] for r in rows], np.int64) if owner_of is None else owner_of
    drop = None if drop_null else t(np.array([as_signed(r[1]) for r in rows], np.int64))
    return ops.fold_compose(s['ptab'], s['conv_b'].to(DEV), s['seg'] if seg is None else seg, s['dev'], t(owner),
                            t(s['ids'] if ids is None else ids), T, drop=drop).cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('Vp', (1, 5, 1000))
@pytest.mark.parametrize('Fp', (1, 100, 112))
@pytest.mark.parametrize('Ep', (4, 52, 300))
def test_ptab_is_within_the_dot_product_bound_of_float64(Ep, Fp, Vp):
    from reviews4rec_amd import _lib, ops
    g = torch.Generator().manual_seed(Ep * 1000 + Fp * 7 + Vp)
    table, w = torch.randn(Vp, Ep, generator=g), torch.randn(Fp, 1, 3, Ep, generator=g)
    ptab = ops.fold_project(table.to(DEV), w.to(DEV)).cpu()
    PS = _lib.lib().r4r_fold_ptab_stride(Fp)
    assert PS >= 3 * Fp and tuple(ptab.shape) == (Vp, PS)
    w3 = w.reshape(Fp, 3, Ep).to(torch.float64)
    want = torch.einsum('vk,fjk->vjf', table.to(torch.float64), w3)
    mag = torch.einsum('vk,fjk->vjf', table.to(torch.float64).abs(), w3.abs())
    got = ptab[:, :3 * Fp].reshape(Vp, 3, Fp).to(torch.float64)
    err, bound = (got - want).abs(), (Ep + 1) * 2.0 ** -24 * mag
    print('E=%d F=%d V=%d worst |err| / bound = %.3f' % (Ep, Fp, Vp, float((err / bound.clamp(min=1e-300)).max())))
    assert (err <= bound).all()


def test_segments_equal_the_reference_bit_for_bit(setup):
    s = setup
    tok, rev_off, first = s['host']
    want = R.seg_table(s['P'], s['b'], tok, rev_off, first, s['ids'], s['S'])
    got = s['seg'].cpu().numpy()
    assert np.isneginf(want).any() and np.isfinite(want).any()
    assert _same(got, want)


@pytest.mark.parametrize('T', TS)
def test_pooled_equals_the_brute_force_bit_for_bit(setup, T):
    s = setup
    docs, want = _reference(s, T)
    got = _compose(s, s['rows'], T)
    assert (got >= 0).all() and not np.signbit(got).any()  # no -0
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert len(bad) == 0, [(s['rows'][r][0], hex(s['rows'][r][1])) for r in bad[:8]]
    if T >= 5:
        tail_row = [r for r, (o, m) in enumerate(s['rows']) if o == 6 and m == ALL][0]
        assert docs[tail_row].any()                         # the 70-review owner's tail really slides in


@pytest.mark.parametrize('T', (5, 37))
def test_null_masks_negative_owners_and_an_id_outside(setup, T):
    s = setup
    _, want = _reference(s, T)
    plain = [r for r, (o, m) in enumerate(s['rows']) if m == 0]
    rows = [s['rows'][r] for r in plain]
    assert _same(_compose(s, rows, T, drop_null=True), want[plain])
    owner = np.array([r[0] for r in rows], np.int64)
    owner[::3] = -1 - np.arange(len(owner[::3]))            # rows that are not computed: +0 everywhere
    got = _compose(s, rows, T, owner_of=owner)
    assert not got[::3].any() and not np.signbit(got[::3]).any()
    keep = owner >= 0
    assert _same(got[keep], want[plain][keep])
    ids = s['ids'].copy()
    ids[2] = -1                                             # an owner without reviews: the all-padding document
    two = _compose(s, [(2, 0), (0, 0)], T, ids=ids)
    assert _same(two[0], two[1])                            # (owner 0 has no reviews either)


@pytest.mark.parametrize('T', (3, 37))
def test_a_rows_bits_do_not_depend_on_its_call(setup, T):
    from reviews4rec_amd import ops
    s = setup
    _, want = _reference(s, T)
    rows = s['rows']
    for M in (1, 5, 257):
        assert _same(_compose(s, rows[:M], T), want[:M]), M
    for cut in (1, 64, 65):
        assert _same(_compose(s, rows[cut:cut + 300], T), want[cut:cut + 300]), cut
        assert _same(_compose(s, rows[:cut], T), want[:cut]), cut
    perm = np.random.RandomState(T).permutation(len(rows))
    assert _same(_compose(s, [rows[r] for r in perm], T), want[perm])
    # the owners in another order, one of them twice; S smaller than the lists (uncached reviews are walked) and at 64
    ids = np.concatenate([s['ids'][::-1], s['ids'][3:4]])
    where = {int(o): j for j, o in enumerate(ids)}
    owner_of = np.array([where[r[0]] for r in rows], np.int64)
    for S in (1, 3, 64):
        seg = ops.fold_segments(s['ptab'], s['conv_b'].to(DEV), s['dev'], s['t'](ids), S)
        assert _same(_compose(s, rows, T, seg=seg, ids=ids, owner_of=owner_of), want), S


def test_fewer_filters_than_a_wave(setup):
    from reviews4rec_amd import ops
    s, T, Fs = setup, 37, 37
    ptab = ops.fold_project(s['table'].to(DEV), s['conv_w'][:Fs].to(DEV))
    conv_b = s['conv_b'][:Fs].contiguous()
    seg = ops.fold_segments(ptab, conv_b.to(DEV), s['dev'], s['t'](s['ids']), s['S'])
    docs, _ = _reference(s, T)
    rows = s['rows']
    got = ops.fold_compose(ptab, conv_b.to(DEV), seg, s['dev'], s['t'](np.array([r[0] for r in rows], np.int64)),
                           s['t'](s['ids']), T, drop=s['t'](np.array([as_signed(r[1]) for r in rows], np.int64)))
    assert _same(got.cpu().numpy(), R.brute_docs(R.ptab3(ptab.cpu().numpy(), Fs), conv_b.numpy(), docs))


@pytest.mark.parametrize('T', (5, 37))
def test_the_fold_and_the_tower_lie_within_the_float64_bound(setup, T):
    from reviews4rec_amd import ops
    s = setup
    docs, _ = _reference(s, T)
    pick = np.arange(0, len(docs), 7)
    idx = torch.from_numpy(docs[pick]).to(DEV)
    table, w, b = s['table'].to(DEV), s['conv_w'].to(DEV), s['conv_b'].to(DEV)
    pooled, arg = ops.textcnn_fwd_raw(idx, table, w, b)
    check_pool(idx, table, w, b, pooled, arg)              # the tower, by conv_ref's own rule
    # the fold has no argmax: relu(max (y64 - beta)) <= pooled <= relu(max (y64 + beta)), beta = fp32_coef(E) S per
    # window -- three E-term dots, two adds and a bias
    y, S = conv64(idx, table, w, b)
    beta = fp32_coef(E) * S
    got = torch.from_numpy(_compose(s, [s['rows'][r] for r in pick], T)).to(DEV, torch.float64)
    lo, hi = (y - beta).max(2).values.clamp(min=0), (y + beta).max(2).values.clamp(min=0)
    assert ((got >= lo) & (got <= hi)).all()
    assert ((pooled.to(torch.float64) >= lo) & (pooled.to(torch.float64) <= hi)).all()
