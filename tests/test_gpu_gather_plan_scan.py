"""The gather's segment plan at the sizes where its scan spans threads and waves (csrc/tokens_device.h,
segment_plan_block<256>: thread i owns units 16 i .. 16 i + 15, a __shfl_up prefix inside each wave of 1,024 units, a
four-entry LDS table of wave totals, the tail mask `unit < units`, plan_ready = an eighth of the units uniform).
tests/test_gpu_gather_plan.py holds the helpers and the cases at 8 .. 32 units, which stay inside threads 0 and 1; the
cases here run 1,024 .. 4,096 units per tower (4,096 is the limit; 4,104 gets no plan), with live patterns that put the
uniform units behind whole waves of live ones, the ready threshold on both of its sides with the deciding document in
the last wave, a flag set by hand behind a tower's last unit (the tail mask), a mispredicted announcement under a
raised plan, a span, and the planned gather's partials against the float64 convolution (conv_ref.check_pool, its own
per-element fp32 bound).

Every case keeps E = 20, L = 4, V = 60, conv_algo = 2 and three steps per run: the kernels take milliseconds at these
sizes, and the host-side restatement of the rule is linear in the units.

Document lengths decide the flags.  A document's first and last segment are live; segment s in between is uniform
exactly when the document is at most 128 s - 2 words long (`uniform_by_length`; every case that builds a count from
lengths first holds it against host_live)."""
import numpy as np
import pytest
import torch

import conv_ref
from test_gpu_gather_plan import (E, L, LIVE, MIXED_ITEM, MIXED_USER, NP, PERM, READY, V, Run, check_perm, host_live,
                                  make_batches, on_and_off, same_bits, tiles_of)

pytestmark = pytest.mark.gpu
F_CONV = 100
SHORT_USER, SHORT_ITEM = [0, 1, 100, 130], [0, 50, 449, 450]     # the mixed layout of the 4-tile cases (T = 450)


def uniform_by_length(lengths, T):
    """How many uniform segments documents of these lengths have (the rule of the module docstring)."""
    lengths = np.minimum(np.asarray(lengths), T)
    return int(sum(int((lengths <= 128 * s - 2).sum()) for s in range(1, tiles_of(T) - 1)))


def assert_uniform(batches, T, count):
    """The construction itself: every batch has `count` uniform segments in both towers, by the host-side rule."""
    for data, _ in batches:
        for t in range(2):
            assert int((~host_live(data[3 + t].cpu().numpy(), T)).sum()) == count, 'the test built the wrong batch'


def mixed(B, T):
    """The file's mixed layout for T, resized to B documents: (user lengths, item lengths, is the plan ready)."""
    ul, il = (MIXED_USER, MIXED_ITEM) if tiles_of(T) == 8 else (SHORT_USER, SHORT_ITEM)
    units = B * tiles_of(T)
    ready = [uniform_by_length(np.resize(l, B), T) * 8 >= units for l in (ul, il)]
    assert ready[0] == ready[1]
    return ul, il, ready[0]


# ---- 1. the size matrix: wave 0 exactly full; thread 64 half filled; two waves and a bit; the tail mask inside the last
# thread; the limit; a tail inside thread 1; the limit over 4 tiles with the short last segment
SIZES = [(128, 1000), (129, 1000), (258, 1000), (511, 1000), (512, 1000), (5, 450), (1024, 450)]


@pytest.mark.parametrize('B,T', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_size_matrix(B, T):
    ul, il, ready = mixed(B, T)
    batches = make_batches(B, T, ul, il)
    on, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=ready)
    # no word of `perm` behind the tower's last unit was ever written (the workspace starts zero-filled)
    units = B * tiles_of(T)
    assert not any(on.words(PERM, t, bf, 4096)[units:].any() for t in range(2) for bf in range(2))


TAILS = [(129, 1000), (511, 1000), (5, 450)]                 # the tower ends inside thread 64, thread 255, thread 1


@pytest.mark.parametrize('B,T', TAILS, ids=['%dx%d' % s for s in TAILS])
def test_a_flag_behind_the_last_unit_is_cut_off(B, T):
    """The scan's tail mask, `unit < units`, in a thread that also owns real units: live[units], the word behind the
    tower's last flag, is set by hand before the step that scans the flags of batch 2.  (The flag role never writes it,
    so without this the mask could be off by one unseen.)  `perm` must be the partition of the tower's own flags all the
    same, and the thread -- it counted live units of its own -- clears the word with the rest."""
    from reviews4rec_amd import _lib
    ul, il, ready = mixed(B, T)
    units = B * tiles_of(T)
    batches = make_batches(B, T, ul, il)
    try:
        r = Run(B, T, 1)
        r.step(batches, 0)
        scanned = r.eng._last_buf                            # the next step announces into the buffer it does not use
        for t in range(2):
            at = r.lib.r4r_deepconn_ws_plan_offset(B, T, E, L, V, t, scanned, LIVE) + 4 * units
            r.eng._ws[at:at + 4].view(torch.int32).fill_(1)
            assert r.words(LIVE, t, scanned, units + 1).tolist() == [0] * units + [1]
        r.step(batches, 1)
        assert r.eng._last_buf == scanned ^ 1
        plan = {'ready_all': r.ready(), 'ready': [int(r.words(READY, t, scanned, 1)[0]) for t in range(2)],
                'perm': [r.words(PERM, t, scanned, units) for t in range(2)]}
        check_perm([plan], batches[1:] + batches[:1], B, T, expect_ready=ready)      # (held against batch 2's flags)
        for t in range(2):
            assert not r.words(LIVE, t, scanned, 4096).any()
            assert not r.words(PERM, t, scanned, 4096)[units:].any()
    finally:
        _lib.lib().r4r_gather_plan(1)


def test_one_document_over_the_limit_writes_no_plan_word():
    B, T = 513, 1000                                         # 4,104 segments per tower
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM, n=2)
    _, plans = on_and_off(B, T, batches)
    for p in plans:
        assert p['ready_all'] == [0, 0, 0, 0] and not any(q.any() for q in p['perm'])


# ---- 2. live patterns that load the prefix unevenly, at the limit
def layout(name, B, T):
    half = B // 2
    if name == 'full_then_empty':                            # waves 0 and 1 all live: every uniform unit behind 2,048 live
        return [T] * half + [0] * (B - half)
    if name == 'empty_then_full':
        return [0] * half + [T] * (B - half)
    if name == 'alternating':
        return [T, 0] * half
    if name == 'all_full_but_the_last':                      # 6 uniform units: not ready, and still the partition
        return [T] * (B - 1) + [0]
    assert name == 'random'
    return np.random.default_rng(5).integers(0, T + 1, size=B).tolist()


LAYOUTS = ['full_then_empty', 'empty_then_full', 'alternating', 'all_full_but_the_last', 'random']


@pytest.mark.parametrize('name', LAYOUTS)
def test_live_patterns_at_the_limit(name):
    B, T = 512, 1000
    lengths = layout(name, B, T)
    count = uniform_by_length(lengths, T)
    if name != 'random':
        assert count == {'all_full_but_the_last': 6}.get(name, 6 * (B // 2))
    batches = make_batches(B, T, lengths, lengths)
    assert_uniform(batches, T, count)
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=count * 8 >= B * tiles_of(T))


# ---- 3. the ready threshold, both sides, at the limit: 512 uniform units of 4,096 raise the plan, 511 do not
def threshold_lengths(B, T, empty, special):
    """`empty` empty documents scattered evenly over the batch, one document of length `special` (None: none) four from
    its end -- in the scan's last wave, also after make_batches has rotated the batch by up to three documents -- and
    every other document full."""
    lengths = np.full(B, T)
    at = (np.arange(empty) * (B - 8)) // empty
    assert len(set(at.tolist())) == empty and at[-1] < B - 8
    lengths[at] = 0
    if special is not None:
        lengths[B - 4] = special
    return lengths.tolist()


THRESHOLDS = [
    # B, T, empty documents, the special document's length, uniform units, ready
    (512, 1000, 85, 600, 512, True),        # 85 * 6 + 2 (a 600-word document: segments 5 and 6)
    (512, 1000, 85, 700, 511, False),       # 85 * 6 + 1 (639 .. 766 words: segment 6 alone)
    (1024, 450, 256, None, 512, True),      # an empty 4-tile document has 2 uniform segments
    (1024, 450, 255, 200, 511, False),      # 255 * 2 + 1 (127 .. 254 words: segment 2 alone)
]


@pytest.mark.parametrize('B,T,empty,special,count,ready', THRESHOLDS,
                         ids=['%dx%d-%d' % (c[0], c[1], c[4]) for c in THRESHOLDS])
def test_ready_threshold_both_sides(B, T, empty, special, count, ready):
    units = B * tiles_of(T)
    assert units == 4096 and (count * 8 >= units) == ready
    lengths = threshold_lengths(B, T, empty, special)
    assert uniform_by_length(lengths, T) == count
    batches = make_batches(B, T, lengths, lengths)
    assert_uniform(batches, T, count)
    on, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=ready)
    assert on.followed() == [int(ready)] * 2                 # the last step's gather, on the plan raised before it
    assert all(p['ready'] == [int(ready)] * 2 for p in plans)


# ---- 4. a mispredicted announcement under a raised plan
def test_mispredicted_announcement_drops_the_raised_plan():
    """Batch 2 is announced and its plan raised, then the engine is given batch 3: that step compacts its own tokens
    and follows no plan, batch 2's plan word is withdrawn, and the bits of it and of the step after it are those of an
    engine without plans that was given the same calls."""
    from reviews4rec_amd import _lib
    B, T = 128, 1000
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM)
    calls = [(0, 1), (1, 2), (3, 0), (0, 1)]                 # (train on, announce); the third call is the wrong guess
    try:
        snaps = {}
        for plan in (1, 0):
            r = Run(B, T, plan)
            snaps[plan] = []
            for n, (k, ann) in enumerate(calls):
                r.eng.train_step(*batches[k], next_data=batches[ann][0])
                snaps[plan].append(r.snapshot())
                if not plan:
                    assert r.ready() == [0, 0, 0, 0] and r.followed() == [0, 0]
                    continue
                ob = r.eng._last_buf ^ 1                     # the buffer of the batch this call announced
                assert [int(r.words(READY, t, ob, 1)[0]) for t in range(2)] == [1, 1], 'call %d raised no plan' % n
                assert not any(r.words(LIVE, t, bf, 4096).any() for t in range(2) for bf in range(2))
                if n == 1:
                    a_buf = ob                               # batch 2's token state and plan
                    assert r.followed() == [1, 1]
                if n == 2:
                    assert r.eng._last_buf == a_buf          # the step took over the buffer of the dropped batch
                    # (it was handed no plan pointers at all -- tokens_ready = 0 -- so the word is the buffer's last one;
                    # the withdrawn plan_ready and the equal bits below are what hold this step)
                    assert r.followed() == [0, 0]
                    assert [int(r.words(READY, t, a_buf, 1)[0]) for t in range(2)] == [0, 0]
                    assert sum(r.ready()) == 2               # only the plan of the batch announced now is up
                if n == 3:
                    assert r.followed() == [1, 1]
        for n in range(len(calls)):
            same_bits(snaps[1][n], snaps[0][n], 'call %d' % n)
    finally:
        _lib.lib().r4r_gather_plan(1)


# ---- 5. a span at a size that uses more than one wave of the scan
def test_span_of_three_steps_at_a_multi_wave_size():
    from reviews4rec_amd import _lib
    from reviews4rec_amd.data import SpanDescriptor
    B, T = 258, 1000
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM)
    try:
        single = Run(B, T, 1)
        for k in range(3):
            last = single.step(batches, k)
        span = Run(B, T, 1)
        span.eng._span(SpanDescriptor.resident(batches), 0, 3, True)
        assert span.eng.step_count == single.eng.step_count == 3
        same_bits(last, span.snapshot(), 'span')
        assert span.ready() == single.ready() and sum(span.ready()) == 2
        assert span.followed() == single.followed() == [1, 1]
    finally:
        _lib.lib().r4r_gather_plan(1)


# ---- 6. the planned gather against the float64 convolution
def pool_of_partials(run, snap, tower):
    """The head kernel's reduction of a tower's partials [B, tiles, 112] (csrc/engine.hip, "pool finish"): the first
    tile with the largest value wins (strict >), relu, and the argmax -- `parg` holds the position 0 .. T + 1 inside the
    document -- is -1 where nothing is above zero.  -> pooled [B, 100] float32, argmax [B, 100] int32."""
    tiles = tiles_of(run.T)
    pmax = snap['pmax%d' % tower].view(np.float32).reshape(run.B, tiles, NP)[:, :, :F_CONV]
    parg = snap['parg%d' % tower].reshape(run.B, tiles, NP)[:, :, :F_CONV]
    win = pmax.argmax(axis=1)                                # (the first of equal maxima)
    best = np.take_along_axis(pmax, win[:, None, :], 1)[:, 0]
    pos = np.take_along_axis(parg, win[:, None, :], 1)[:, 0]
    above = best > 0
    return torch.from_numpy(np.where(above, best, np.float32(0))), torch.from_numpy(np.where(above, pos, -1))


def test_planned_gather_against_float64():
    from reviews4rec_amd import _lib
    B, T = 512, 1000
    lengths = layout('full_then_empty', B, T)
    batches = make_batches(B, T, lengths, lengths)
    try:
        r = Run(B, T, 1)
        r.step(batches, 0)
        weights = r.eng.flat_p.clone()                       # what the next step's projection multiplies by
        snap = r.step(batches, 1)
        assert r.followed() == [1, 1]
        off, size = r.eng.offsets, r.eng.sizes
        assert r.eng.E == E and size[0] == size[4] == F_CONV * 3 * E and size[1] == size[5] == F_CONV
        for t in range(2):
            w = weights[off[4 * t]:off[4 * t] + size[4 * t]].view(F_CONV, 1, 3, E)
            b = weights[off[4 * t + 1]:off[4 * t + 1] + size[4 * t + 1]]
            pooled, arg = pool_of_partials(r, snap, t)
            worst = conv_ref.check_pool(batches[1][0][3 + t], r.eng.table, w, b, pooled, arg)
            print('tower %d: worst |pooled - y64[arg]| / bound = %.4f' % (t, worst))
            assert 0 < worst <= 1
    finally:
        _lib.lib().r4r_gather_plan(1)
