"""r4r_tower_build_variants on the device (include/r4r.h, "What-if documents"; csrc/tower_variants.hip) against the
plain loop of tower_variants_ref.py, integer for integer: every single removed review, sets of them, bits that mean
nothing, the tail beyond the 64th review, occluded positions, ids outside the pool -- at document lengths below, at and
above one position per thread and at one row, a few and more rows than fit a round of anything."""
import numpy as np
import pytest
import torch

from tower_variants_ref import COUNTS, as_signed, synthetic_pool, variant_docs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL = (1 << 64) - 1
OWNERS = len(COUNTS)


@pytest.fixture(scope='module')
def pool():
    tok, rev_off, first, counts = synthetic_pool()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dev = (t(np.concatenate([tok, np.zeros(1, np.int32)])), t(rev_off), t(first), None)
    return dict(host=(tok, rev_off, first), dev=dev, counts=counts)


def rows_of(T):
    """[(id, mask, positions or None)]: the issue's list, spelt out."""
    rows = [(o, 0, None) for o in range(OWNERS)]
    rows += [(o, 1 << s, None) for o in range(OWNERS) for s in range(64)]             # every single bit (63 included)
    for o, c in enumerate(COUNTS):
        live = min(c, 64)
        rows += [(o, ALL >> c << c if c < 64 else 0, None),                            # only bits at or beyond count
                 (o, ALL, None),                                                       # all bits: the tail alone is kept
                 (o, (1 << live) - 1, None)]
        rows += [(o, ALL & ~(1 << s), None) for s in sorted({0, 1, live // 2, max(live - 1, 0), 63})]   # all but one
        rows += [(o, 0, []), (o, 0, [0]), (o, 0, [T - 1]), (o, 0, [-1, T, T + 1, -(1 << 31), (1 << 31) - 1]),
                 (o, 0, [T // 2] * 3), (o, 0, list(range(T))), (o, 0, list(range(T))[::-1] + [0, 0]),
                 (o, 5, [0, 2, T - 1]), (o, ALL, [0]), (o, 1 << 1, [1, 1, T // 3])]    # occlusion with removal
    rows += [(-1, 3, [0]), (OWNERS, ALL, None), (1 << 40, 1, [0]), (-(1 << 40), 0, None)]   # ids outside the pool
    return rows


def device_docs(pool, rows, T, drop_null=False, occ_null=False, owners=OWNERS):
    """One r4r_tower_build_variants call over ``rows`` -> docs on the host; the output starts as -7 everywhere."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    tok, rev_off, first, _ = pool['dev']
    n = len(rows)
    ids = torch.tensor([r[0] for r in rows], dtype=torch.int64, device=DEV)
    drop = None if drop_null else torch.tensor([as_signed(r[1]) for r in rows], dtype=torch.int64, device=DEV)
    occ_off = occ_pos = None
    if not occ_null:
        lens = [len(r[2] or ()) for r in rows]
        lead = 3                                             # the table need not start at 0: entries are absolute
        occ_off = torch.tensor(np.concatenate([[lead], lead + np.cumsum(lens)]), dtype=torch.int64, device=DEV)
        occ_pos = torch.tensor([0] * lead + [p for r in rows for p in (r[2] or ())] + [0], dtype=torch.int32, device=DEV)
    docs = torch.full((n, T), -7, dtype=torch.int64, device=DEV)
    _lib.call('r4r_tower_build_variants', ptr(tok), ptr(rev_off), ptr(first), owners, ptr(ids), ptr(drop), ptr(occ_off),
              ptr(occ_pos), n, T, ptr(docs))
    return docs


_REF = {}


def reference(pool, T):
    if T not in _REF:
        rows = rows_of(T)
        tok, rev_off, first = pool['host']
        _REF[T] = (rows, variant_docs(tok, rev_off, first, [r[0] for r in rows], [r[1] for r in rows],
                                      [r[2] or () for r in rows], T))
    return _REF[T]


@pytest.mark.parametrize('n', [1, 5, 257])
@pytest.mark.parametrize('T', [1, 5, 37, 300])
def test_documents_equal_the_rule_integer_for_integer(pool, T, n):
    rows, want = reference(pool, T)
    pick = list(range(0, len(rows), 9)) if n == 1 else list(range(len(rows)))        # one row per call: every ninth
    got = torch.cat([device_docs(pool, [rows[k] for k in pick[a:a + n]], T) for a in range(0, len(pick), n)])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.nonzero((got != want[pick]).any(1))[0]
    assert not len(bad), [(rows[pick[k]][:2], got[k].tolist(), want[pick[k]].tolist()) for k in bad[:3]]
    if n == 257 and T >= 37:                                 # the cases are what they say
        full = {r[:2]: want[k] for k, r in enumerate(rows) if r[2] is None}
        assert full[(6, ALL)].any() and not full[(5, ALL)][6:].any() and not full[(4, ALL)].any()
        assert not np.array_equal(full[(6, 1)], full[(6, 0)]) and np.array_equal(full[(2, 1)], full[(2, 0)])


@pytest.mark.parametrize('T', [5, 300])
def test_permuted_rows_and_split_calls_change_nothing(pool, T):
    rows, want = reference(pool, T)
    order = np.random.RandomState(T).permutation(len(rows))
    got = device_docs(pool, [rows[k] for k in order], T).cpu().numpy()
    assert np.array_equal(got, want[order])
    some = [rows[k] for k in order[:130]]
    for cut in (1, 64, 65):
        parts = torch.cat([device_docs(pool, some[:cut], T), device_docs(pool, some[cut:], T)]).cpu().numpy()
        assert np.array_equal(parts, got[:130]), cut


@pytest.mark.parametrize('T', [1, 37, 300])
def test_null_masks_and_null_positions_are_r4r_tower_build(pool, T):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    tok, rev_off, first, _ = pool['dev']
    ids = list(range(OWNERS)) + [6, -1, OWNERS, 3, 3, 1 << 40]
    dev_ids = torch.tensor(ids, dtype=torch.int64, device=DEV)
    want = torch.full((len(ids), T), -7, dtype=torch.int64, device=DEV)
    _lib.call('r4r_tower_build', ptr(tok), ptr(rev_off), ptr(first), None, OWNERS, ptr(dev_ids), len(ids), T, 0, 0, 0,
              ptr(want), None)
    rows = [(o, ALL, [0]) for o in ids]                      # (what the NULLs keep from being read)
    for drop_null, occ_null in ((True, True), (True, False), (False, True)):
        plain = [(o, 0 if not drop_null else m, None if not occ_null else p) for o, m, p in rows]
        got = device_docs(pool, plain, T, drop_null=drop_null, occ_null=occ_null)
        assert torch.equal(got, want), (drop_null, occ_null)
    # `owners` is the argument's: the same pool seen as three owners has nothing for owner 3
    got = device_docs(pool, [(2, 0, None), (3, 0, None)], T, owners=3)
    assert torch.equal(got[0], want[2]) and (got[1] == 0).all()


def test_an_empty_call_enqueues_nothing(pool):
    from reviews4rec_amd import _lib, ops
    out = torch.full((4, 37), -7, dtype=torch.int64, device=DEV)
    _lib.call('r4r_tower_build_variants', None, None, None, OWNERS, None, None, None, None, 0, 37, out.data_ptr())
    torch.cuda.synchronize()
    assert (out == -7).all()
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    assert ops.tower_build_variants(pool['dev'], none, 37).shape == (0, 37)


def test_the_wrapper_passes_what_it_is_given(pool):
    from reviews4rec_amd import ops
    rows, want = reference(pool, 37)
    t = lambda v, dt=torch.int64: torch.tensor(v, dtype=dt, device=DEV)
    lens = [len(r[2] or ()) for r in rows]
    got = ops.tower_build_variants(pool['dev'], t([r[0] for r in rows]), 37, drop=t([as_signed(r[1]) for r in rows]),
                                   occ_off=t(np.concatenate([[0], np.cumsum(lens)])),
                                   occ_pos=t([p for r in rows for p in (r[2] or ())], torch.int32))
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match='come together'):
        ops.tower_build_variants(pool['dev'], t([0]), 37, occ_off=t([0, 0]))
    with pytest.raises(RuntimeError, match=r'drop must be \[n\]'):
        ops.tower_build_variants(pool['dev'], t([0]), 37, drop=t([0, 0]))
    with pytest.raises(RuntimeError, match='T=65537'):
        ops.tower_build_variants(pool['dev'], t([0]), 65537)
