"""The gather-add-max's segment plan (r4r_gather_plan; csrc/tokens_device.h): a plan may only reorder which workgroup
walks which segment.  Every case runs the fused DeepCoNN engine for 3 steps with the next batch announced, once with
the plan on and once with it off, from the same seed, and requires the same BITS in pred, se, every parameter and Adam
moment and in the conv partials (pmax / parg, read back from the workspace) after each step.

The plan words are read back as well: `perm` must be the stable partition "live segments first" of the host-side
flags of the announced batch, and plan_ready must be 0 wherever the plan does not apply.  Equal bits cannot tell a plan
that was followed from one that was ignored, so the gather leaves a word next to the token counter saying which mapping
a launch that was given a plan took: it must be 1 exactly in the steps whose batch had a plan raised for it.  (A
document's first and last segment hold tokens outside the document and are live by the rule, so the two-tile case never
gets a plan: an eighth of its segments would have to be uniform.  The short last segment UNDER a plan has a case of its
own, T = 450.)

The cases of this file run at B = 4 -- 8 to 32 segments per tower, inside the first two threads of the plan's scan --
and once over the limit of 4,096.  tests/test_gpu_gather_plan_scan.py runs the same checks, with the helpers of this
file, at 1,024 .. 4,096 segments, where the scan's prefix crosses lanes and waves."""
import numpy as np
import pytest
import torch

import oracle
from helpers import synthetic_review_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E, L, V, U, I = 20, 4, 60, 12, 9
NP = 112
PMAX, PARG = 0, 1               # r4r_deepconn_ws_partials_offset
PERM, READY, LIVE = 0, 1, 2      # r4r_deepconn_ws_plan_offset


def tiles_of(T):
    return (T + 2 + 127) // 128


def documents(lengths, T, rng):
    """[len(lengths), T]: random words 1 .. V - 1 up to each length, zero padding behind (data.py:198-199)."""
    tok = rng.integers(1, V, size=(len(lengths), T))
    return np.where(np.arange(T)[None, :] < np.asarray(lengths)[:, None], tok, 0).astype(np.int64)


def make_batches(B, T, user_lengths, item_lengths, n=4, seed=11):
    """n batches in the 7-slot layout whose documents have the given lengths, rotated by one document per batch."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        data, y = synthetic_review_batch(B, T, V, U, I, seed=seed + k, device=DEV)
        ul, il = np.roll(np.resize(user_lengths, B), k), np.roll(np.resize(item_lengths, B), k)
        data[3] = torch.from_numpy(documents(ul, T, rng)).to(DEV)
        data[4] = torch.from_numpy(documents(il, T, rng)).to(DEV)
        out.append((data, y))
    return out


def host_live(idx, T):
    """The rule of csrc/tokens_device.h on the host: segment u = doc * tiles + seg is live unless every token of its
    window 128 seg - 2 .. p_hi - 1 is the same row, tokens outside the document being a row of their own."""
    tiles = tiles_of(T)
    ext = np.full((idx.shape[0], T + 4), -1, dtype=np.int64)      # token t at column t + 2
    ext[:, 2:T + 2] = idx
    live = np.zeros(idx.shape[0] * tiles, dtype=bool)
    for doc in range(idx.shape[0]):
        for seg in range(tiles):
            w = ext[doc, 128 * seg:min(T + 2, 128 * (seg + 1)) + 2]
            live[doc * tiles + seg] = bool((w != w[0]).any())
    return live


class Run:
    """One engine; `step` trains on batch k announcing batch k + 1 and snapshots everything the plan must not change."""

    def __init__(self, B, T, plan, dropout=0.3):
        import reviews4rec_amd
        from reviews4rec_amd import _lib
        from reviews4rec_amd.engine import DeepCoNNEngine
        self.lib, self.B, self.T = _lib.lib(), B, T
        self.lib.r4r_gather_plan(plan)
        hp = dict(model_type='deepconn', latent_size=L, word_embed_size=E, input_length=T, dropout=dropout,
                  total_users=U, total_items=I, lr=0.002, weight_decay=1e-6)
        P = oracle.init_params(hp, vocab_size=V, seed=3)
        model = reviews4rec_amd.get_model_class('deepconn')(dict(hp, word_vectors=P['word2vec.weight'].numpy()))
        model.load_state_dict(P)
        self.eng = DeepCoNNEngine(model.to(DEV).train(), lr=hp['lr'], weight_decay=hp['weight_decay'], seed=99,
                                  conv_algo=2)              # project-then-gather at every size

    def at(self, off, n):
        return self.eng._ws[off:off + 4 * n].view(torch.int32).cpu().numpy().copy()

    def words(self, which, tower, buf, n):
        return self.at(self.lib.r4r_deepconn_ws_plan_offset(self.B, self.T, E, L, V, tower, buf, which), n)

    def partials(self, which, tower, n):
        return self.at(self.lib.r4r_deepconn_ws_partials_offset(self.B, self.T, E, L, V, tower, which), n)

    def followed(self):
        """Per tower: did the gather of the last step follow a plan (the int after the two token counters)."""
        buf = self.eng._last_buf
        return [int(self.at(self.lib.r4r_deepconn_ws_count_offset(self.B, self.T, E, L, V, t, buf), 3)[2]) for t in range(2)]

    def ready(self):
        return [int(self.words(READY, t, bf, 1)[0]) for bf in range(2) for t in range(2)]

    def snapshot(self):
        torch.cuda.synchronize()
        n = self.B * tiles_of(self.T) * NP
        snap = {'pred': self.eng._outputs(self.B)[0], 'se': self.eng._outputs(self.B)[1], 'p': self.eng.flat_p,
                'm': self.eng.flat_m, 'v': self.eng.flat_v, 'sse': self.eng.sse}
        snap = {k: v.cpu().numpy().copy() for k, v in snap.items()}
        for t in range(2):
            snap['pmax%d' % t] = self.partials(PMAX, t, n)          # (bit patterns)
            snap['parg%d' % t] = self.partials(PARG, t, n)
        return snap

    def step(self, batches, k):
        data, y = batches[k % len(batches)]
        self.eng.train_step(data, y, next_data=batches[(k + 1) % len(batches)][0])
        return self.snapshot()


def same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), '%s: %s differs between the schedules' % (what, k)


def on_and_off(B, T, batches, steps=3):
    """-> (the run with the plan on, the plan words it left after each step); asserts the bits of the two schedules."""
    from reviews4rec_amd import _lib
    try:
        on, off = Run(B, T, 1), None
        snaps, plans = [], []
        for k in range(steps):
            snaps.append(on.step(batches, k))
            ob = on.eng._last_buf ^ 1                        # the buffer that holds the announced batch's state
            units = B * tiles_of(T)
            # the gather followed a plan exactly where the step before raised one for this batch (never in the first step)
            assert on.followed() == (plans[-1]['ready'] if k else [0, 0]), 'step %d' % k
            plans.append({'ready_all': on.ready(), 'ready': [int(on.words(READY, t, ob, 1)[0]) for t in range(2)],
                          'perm': [on.words(PERM, t, ob, min(units, 4096)) for t in range(2)],
                          'live': [on.words(LIVE, t, bf, 4096) for t in range(2) for bf in range(2)]})
        off = Run(B, T, 0)
        for k in range(steps):
            same_bits(snaps[k], off.step(batches, k), 'step %d' % k)
            assert off.ready() == [0, 0, 0, 0] and off.followed() == [0, 0]
        for p in plans:
            assert all(not l.any() for l in p['live'])      # the scan leaves the flags all-zero
        return on, plans
    finally:
        _lib.lib().r4r_gather_plan(1)


def check_perm(plans, batches, B, T, expect_ready):
    units = B * tiles_of(T)
    for k, p in enumerate(plans):
        nxt = batches[(k + 1) % len(batches)][0]
        for t in range(2):
            live = host_live(nxt[3 + t].cpu().numpy(), T)
            perm = p['perm'][t]
            assert np.array_equal(np.sort(perm), np.arange(units)), 'perm is not a permutation'
            want = np.concatenate([np.flatnonzero(live), np.flatnonzero(~live)])
            assert np.array_equal(perm, want), 'perm is not the stable partition "live first"'
            uniform = int((~live).sum())
            assert (uniform * 8 >= units) == expect_ready
            assert p['ready'][t] == int(expect_ready)
        # the plan the step's own gather consumed was withdrawn behind it: only the announced batch's may be up
        assert sum(p['ready_all']) == sum(p['ready'])


MIXED_USER, MIXED_ITEM = [0, 1, 127, 128], [129, 500, 998, 1000]


def test_mixed_lengths_and_the_plan_is_the_stable_partition():
    """T = 1000 (8 tiles), lengths 0, 1, 127, 128, 129, 500, 998, 1000 over the 8 documents: live and uniform segments,
    boundary segments, an all-pad and a full document -- and `perm` as read back is a permutation with the live first."""
    B, T = 4, 1000
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM)
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=True)


def test_every_document_padded_from_position_zero():
    B, T = 4, 1000
    batches = make_batches(B, T, [0], [0])
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=True)     # 6 of 8 segments per document uniform


def test_all_live_refuses_the_plan():
    B, T = 4, 1000
    batches = make_batches(B, T, [T], [T])
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=False)
    assert all(p['ready_all'] == [0, 0, 0, 0] for p in plans)


def test_short_last_segment():
    """T = 254 (2 tiles): the last segment is shorter than 128 -- the equal-slices rule."""
    B, T = 4, 254
    batches = make_batches(B, T, [0, 1, 126, 127], [128, 200, 253, 254])
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=False)    # (both segments of a document are live by the rule)


def test_short_last_segment_under_a_plan():
    """T = 450 (4 tiles, the last one 68 positions): the equal-slices rule in workgroups that pair the short segment
    with one of another document."""
    B, T = 4, 450
    batches = make_batches(B, T, [0, 1, 100, 130], [0, 50, 449, 450])
    _, plans = on_and_off(B, T, batches)
    check_perm(plans, batches, B, T, expect_ready=True)


def test_odd_tile_count_falls_back():
    B, T = 4, 300
    batches = make_batches(B, T, [0, 1, 127, 128], [129, 200, 299, 300])
    on, plans = on_and_off(B, T, batches)
    for p in plans:
        assert p['ready_all'] == [0, 0, 0, 0] and not any(q.any() for q in p['perm'])     # no plan was written


def test_over_the_limit_no_plan():
    B, T = 600, 1000                                         # 4,800 segments per tower
    batches = make_batches(B, T, [0, 1, 127, 128, 129, 500], [998, 1000, 3, 700], n=2)
    on, plans = on_and_off(B, T, batches)
    for p in plans:
        assert p['ready_all'] == [0, 0, 0, 0] and not any(q.any() for q in p['perm'])


def test_span_of_three_steps_leaves_the_bits_of_three_single_steps():
    from reviews4rec_amd.data import SpanDescriptor
    B, T = 4, 1000
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM)
    single = Run(B, T, 1)
    for k in range(3):
        last = single.step(batches, k)
    span = Run(B, T, 1)
    span.eng._span(SpanDescriptor.resident(batches), 0, 3, True)
    assert span.eng.step_count == single.eng.step_count == 3
    same_bits(last, span.snapshot(), 'span')
    assert span.ready() == single.ready() and sum(span.ready()) == 2       # both left batch 3's plan up
    assert span.followed() == single.followed() == [1, 1]


def test_first_step_and_forward_only_have_no_plan():
    """The first step of an engine compacts its own tokens (tokens_ready = 0) and a forward-only call announces
    nothing: neither has a plan, with the switch on or off."""
    from reviews4rec_amd import _lib
    B, T = 4, 1000
    batches = make_batches(B, T, MIXED_USER, MIXED_ITEM)
    try:
        got = []
        for plan in (1, 0):
            r = Run(B, T, plan)
            r.eng.model.eval()
            pred, se = r.eng.predict(*batches[0])
            fwd = r.snapshot()
            fwd['pred_fwd'], fwd['se_fwd'] = pred.cpu().numpy().copy(), se.cpu().numpy().copy()
            assert r.ready() == [0, 0, 0, 0]
            r.eng.model.train()
            got.append((fwd, r.step(batches, 0)))
        same_bits(got[0][0], got[1][0], 'forward only')
        same_bits(got[0][1], got[1][1], 'first step')
    finally:
        _lib.lib().r4r_gather_plan(1)
