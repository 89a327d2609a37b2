"""The DeepCoNN training step in four launches (r4r_deepconn_tail_fold; csrc/engine.hip: deepconn_backward_fold_kernel,
csrc/wgrad_device.h: wgrad_row_block) against the five-launch step in one build.

Every case drives r4r_deepconn_step through the C ABI for a chain of six training steps, each announcing the next batch,
from identical state: once with the old tail forced, once with the switch on.  After EVERY step the two runs must agree
bit for bit in pred, se, sse_accum, the whole flat gradient and flat P / M / V (pads included, and the pads must be +0),
and the token state the step prepared for the next batch in the OTHER buffer must be what it is today: the same count,
the same set of tokens in `list` (the order in which workgroups reserve rows varies run to run by design), `slot` the
inverse of `list`, flags and `live` all zero, `perm` and plan_ready equal.

Equal bits cannot tell a folded step from an unfolded one, so every case also asks r4r_deepconn_tail which tail its
shape resolves to, against the rule worked out here: B <= 256, ceil(B / 16) * E / 4 <= 1,024, latent_size <= 64.

The inputs hold what the conv gradient's row role can get wrong: dead filters (conv bias -1e4: argmax -1 for every
document), an argmax at the first and at the last conv position (taps outside the document), a document of one repeated
token -- each asserted from the argmax the step left in its workspace."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
V, F = 500, 100
TOK_A, TOK_C, TOK_REP = V - 1, V - 2, 7          # rows that pin an argmax to the first / last position; the repeated token
F_FIRST, F_LAST, DEAD = 0, 1, (3, 50, 99)
STEPS = 6
FLAGS, SLOT, LIST, ARGMAX = 0, 1, 2, 3           # r4r_deepconn_ws_state_offset
PERM, READY, LIVE = 0, 1, 2                      # r4r_deepconn_ws_plan_offset
PROJECT, DIRECT = 2, 1


def expect_fold(B, E, L):
    nsplit = min(16, -(-B // 16))
    return int(B <= 256 and -(-B // nsplit) <= 16 and nsplit * (E // 4) <= 1024 and L <= 64)


def make_inputs(B, T, E, L, lib, seed=5):
    """Table, flat parameters and STEPS + 1 batches, on the host (both runs start from copies of them)."""
    rng = np.random.default_rng(seed)
    table = (0.1 * rng.standard_normal((V, E))).astype(np.float32)
    table[0] = 0.0
    table[TOK_A] = 1.0
    table[TOK_C] = np.where(np.arange(E) % 2 == 0, 1.0, -1.0)     # orthogonal to TOK_A's row
    n = lib.r4r_deepconn_nparam()
    off, size, total = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(1, np.int64))
    assert lib.r4r_deepconn_layout(E, L, off.ctypes.data, size.ctypes.data, total.ctypes.data) == 0
    flat = np.zeros(int(total[0]), np.float32)
    pad = np.ones(int(total[0]), bool)
    for o, s in zip(off, size):
        flat[o:o + s] = (0.05 * rng.standard_normal(int(s))).astype(np.float32)
        pad[o:o + s] = False
    for tower in range(2):                       # slots 0 / 4: conv weight [100, 3, E], 1 / 5: conv bias
        w = flat[off[4 * tower]:off[4 * tower] + F * 3 * E].reshape(F, 3, E)
        b = flat[off[4 * tower + 1]:off[4 * tower + 1] + F]
        b[list(DEAD)] = -1.0e4
        w[F_FIRST] = 0.0
        w[F_FIRST, 2] = 0.25 * table[TOK_A]      # position 0 sees token 0 at tap 2
        w[F_LAST] = 0.0
        w[F_LAST, 0] = 0.25 * table[TOK_C]       # position T + 1 sees token T - 1 at tap 0
    batches = []
    for k in range(STEPS + 1):
        def docs():
            tok = rng.integers(1, V - 2, size=(B, T))
            fill = rng.integers(1, T + 1, size=(B,))
            return np.where(np.arange(T)[None, :] < fill[:, None], tok, 0).astype(np.int64)
        u, i = docs(), docs()
        u[0] = rng.integers(1, V - 2, size=T)
        u[0, 0], u[0, T - 1] = TOK_A, TOK_C
        i[0] = TOK_REP
        if B > 1:                                # the item tower's edges, beside its repeated-token document
            i[1] = rng.integers(1, V - 2, size=T)
            i[1, 0], i[1, T - 1] = TOK_A, TOK_C
        y = rng.integers(1, 6, size=(B,)).astype(np.float32)
        batches.append((u, i, y))
    return table, flat, pad, batches


class Chain:
    def __init__(self, lib, shape, inputs, fold):
        self.lib, self.shape = lib, shape
        self.B, self.E, self.T, self.L, self.opt, self.announce, self.algo = shape
        table, flat, self.pad, batches = inputs
        t = lambda a: torch.from_numpy(a.copy()).to(DEV)
        self.table, self.p = t(table), t(flat)
        self.g, self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.batches = [(t(u), t(i), t(y)) for u, i, y in batches]
        B = self.B
        self.pred, self.se = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        self.sse = torch.zeros(1, device=DEV)
        self.ws = torch.zeros(lib.r4r_deepconn_ws_bytes(B, self.T, self.E, self.L, V), dtype=torch.uint8, device=DEV)
        self.fold = fold

    def ints(self, off, n):
        return self.ws[off:off + 4 * n].view(torch.int32).cpu().numpy().copy()

    def state(self, which, tower, buf, n):
        return self.ints(self.lib.r4r_deepconn_ws_state_offset(self.B, self.T, self.E, self.L, V, tower, buf, which), n)

    def plan(self, which, tower, buf, n):
        return self.ints(self.lib.r4r_deepconn_ws_plan_offset(self.B, self.T, self.E, self.L, V, tower, buf, which), n)

    def step(self, k):
        lib, B, T, E, L = self.lib, self.B, self.T, self.E, self.L
        u, i, y = self.batches[k]
        nu, ni, _ = self.batches[k + 1]
        projecting = self.algo == PROJECT
        lib.r4r_deepconn_tail_fold(self.fold)
        rc = lib.r4r_deepconn_step(
            self.table.data_ptr(), V, u.data_ptr(), i.data_ptr(), y.data_ptr(), self.p.data_ptr(), self.g.data_ptr(),
            self.pred.data_ptr(), self.se.data_ptr(), self.sse.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            B, T, E, L, 0.3, 1, 99, k * B * 2 * L, 1.0 / B, self.algo, k & 1,
            int(k > 0 and self.announce and projecting),
            nu.data_ptr() if self.announce else None, ni.data_ptr() if self.announce else None,
            self.m.data_ptr() if self.opt else None, self.v.data_ptr() if self.opt else None,
            0.002, 0.9, 0.999, 1e-8, 1e-6, k + 1 if self.opt else 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.r4r_last_error()
        torch.cuda.synchronize()
        snap = {name: x.cpu().numpy().copy() for name, x in
                dict(pred=self.pred, se=self.se, sse=self.sse, g=self.g, p=self.p, m=self.m, v=self.v).items()}
        ob, tok = (k & 1) ^ 1, []
        units = B * ((T + 2 + 127) // 128)
        for t in range(2):
            count = int(self.ints(lib.r4r_deepconn_ws_count_offset(B, T, E, L, V, t, ob), 1)[0])
            tok.append(dict(count=count, list=self.state(LIST, t, ob, count) if count else np.zeros(0, np.int32),
                            slot=self.state(SLOT, t, ob, V), flags=self.state(FLAGS, t, ob, V + 4),
                            live=self.plan(LIVE, t, ob, 4096), perm=self.plan(PERM, t, ob, min(units, 4096)),
                            ready=self.plan(READY, t, ob, 1)))
        argmax = [self.state(ARGMAX, t, 0, B * F).reshape(B, F) for t in range(2)]
        return snap, tok, argmax


def check_step(what, shape, new, old, nxt, conv_w_off):
    B, E, T, L, opt, announce, algo = shape
    (snap, tok, argmax), (snap_old, tok_old, _) = new, old
    for name in snap:
        assert np.array_equal(snap[name].view(np.uint8), snap_old[name].view(np.uint8)), '%s: %s differs' % (what, name)
    for t in range(2):
        a, b = tok[t], tok_old[t]
        assert a['count'] == b['count'], what
        assert np.array_equal(np.sort(a['list']), np.sort(b['list'])), what
        if announce and algo == PROJECT:
            assert np.array_equal(np.sort(a['list']), np.unique(nxt[t])), '%s: not the announced batch\'s tokens' % what
            assert a['count'] > 0
        for s in (a, b):
            assert np.array_equal(s['slot'][s['list']], np.arange(s['count'])), '%s: slot is not the inverse of list' % what
            if s['count']:
                assert int((s['slot'] >= 0).sum()) == s['count'], what
            assert not s['flags'].any() and not s['live'].any(), '%s: flags / live not left zero' % what
        assert np.array_equal(a['perm'], b['perm']) and np.array_equal(a['ready'], b['ready']), what
    # what the inputs were built to contain
    assert (argmax[0][:, list(DEAD)] == -1).all() and (argmax[1][:, list(DEAD)] == -1).all(), '%s: dead filters' % what
    assert argmax[0][0, F_FIRST] == 0 and argmax[0][0, F_LAST] == T + 1, '%s: argmax at the edges' % what
    if B > 1:
        assert argmax[1][1, F_FIRST] == 0 and argmax[1][1, F_LAST] == T + 1, '%s: argmax at the edges, item tower' % what
    # the document of one repeated token (item tower, document 0): every interior window is the same three rows, so a
    # live filter's first maximum is a window that overlaps the document's edge or the first whole one -- the row role
    # reads ONE row three times, or fewer taps
    rep_arg = argmax[1][0]
    assert np.isin(rep_arg, [-1, 0, 1, 2, T, T + 1]).all() and (rep_arg >= 0).any(), '%s: repeated-token document' % what
    assert (argmax[0] >= 0).any()
    live = [f for f in range(F) if f not in DEAD]
    gw = [snap['g'][o:o + F * 3 * E].reshape(F, 3, E) for o in conv_w_off]
    for t in range(2):                           # a dead filter's gradient row is exactly zero, the live ones' are not
        assert not gw[t][list(DEAD)].any() and gw[t][live].any(), '%s: dead filters\' gradient' % what


#         B    E    T    L  Adam  next  conv
CASES = [(1, 8, 200, 10, 1, 1, PROJECT),          # one split, one document, two float4 columns
         (5, 52, 200, 10, 1, 1, PROJECT),
         (16, 304, 200, 10, 1, 1, PROJECT),        # one full split
         (17, 304, 30, 40, 1, 1, PROJECT),         # two splits of 9 and 8; one segment: the plan is refused
         (37, 52, 200, 40, 0, 1, PROJECT),         # three splits, ragged; gradients only
         (37, 304, 200, 10, 1, 0, PROJECT),        # without a next batch
         (128, 304, 200, 10, 1, 1, PROJECT),       # the full eight splits x 76 columns
         (128, 512, 30, 10, 1, 1, PROJECT),        # nsplit x E / 4 = 1,024 exactly
         (128, 768, 30, 10, 1, 1, PROJECT),        # over: the query says old tail, the step still matches
         (128, 8, 200, 10, 0, 0, PROJECT),         # sixteen threads of row work in 256; gradients only, no next batch
         (17, 512, 200, 10, 0, 1, PROJECT),
         (5, 52, 30, 10, 1, 1, DIRECT),            # the direct conv: no token state, the same tail
         (5, 52, 200, 80, 1, 1, PROJECT),          # latent_size 65 .. 128 keeps the old tail
         (129, 52, 200, 10, 1, 1, PROJECT),        # nine splits of 15 + 9
         (241, 64, 200, 10, 1, 1, PROJECT),        # sixteen splits, a last split of one document
         (255, 52, 30, 10, 1, 1, PROJECT),
         (256, 256, 30, 10, 1, 1, PROJECT),        # 1,024 threads, 256 documents: both limits at once
         (256, 260, 30, 10, 1, 1, PROJECT),        # over: the query says old tail, the step still matches
         (257, 32, 30, 10, 1, 1, PROJECT),         # over by B
         (256, 64, 200, 64, 0, 0, PROJECT),        # the widest folded head; gradients only, no next batch
         (256, 52, 30, 10, 1, 1, DIRECT)]


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'B%d-E%d-T%d-L%d-adam%d-next%d-conv%d' % s)
def test_four_launch_step_leaves_the_bits_of_the_five_launch_step(shape):
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    B, E, T, L, opt, announce, algo = shape
    try:
        lib.r4r_deepconn_tail_fold(1)
        assert lib.r4r_deepconn_tail(B, E, L) == expect_fold(B, E, L)
        lib.r4r_deepconn_tail_fold(0)
        assert lib.r4r_deepconn_tail(B, E, L) == 0
        inputs = make_inputs(B, T, E, L, lib)
        n = lib.r4r_deepconn_nparam()
        off, size, total = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(1, np.int64)
        assert lib.r4r_deepconn_layout(E, L, off.ctypes.data, size.ctypes.data, total.ctypes.data) == 0
        conv_w_off = [int(off[0]), int(off[4])]
        assert (inputs[3][0][1][0] == TOK_REP).all()             # the document of one repeated token
        old, new = Chain(lib, shape, inputs, 0), Chain(lib, shape, inputs, 1)
        for k in range(STEPS):
            a, b = new.step(k), old.step(k)
            check_step('step %d' % k, shape, a, b, inputs[3][k + 1][:2], conv_w_off)
            pad = inputs[2]
            for name in ('g', 'p', 'm', 'v'):                    # the pads between the slots: +0, never stepped
                assert not a[0][name].view(np.uint32)[pad].any(), (name, k)
            assert np.isfinite(a[0]['p']).all() and np.isfinite(a[0]['pred']).all()
    finally:
        lib.r4r_deepconn_tail_fold(1)


# ---- the span case drives the engine class (what main.train and bench.py use)
SE, SL, SV, SU, SI = 20, 4, 60, 12, 9


def span_batches(B, T, n=4, seed=11):
    """n batches in the 7-slot layout: documents of mixed lengths, zero padding behind (data.py:198-199)."""
    from helpers import synthetic_review_batch
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        data, y = synthetic_review_batch(B, T, SV, SU, SI, seed=seed + k, device=DEV)
        for slot, lengths in ((3, [0, 1, 127, 128, T]), (4, [129, 150, T - 1, T])):
            ln = np.roll(np.resize(lengths, B), k)
            tok = rng.integers(1, SV, size=(B, T))
            data[slot] = torch.from_numpy(np.where(np.arange(T)[None, :] < ln[:, None], tok, 0).astype(np.int64)).to(DEV)
        out.append((data, y))
    return out


class SpanRun:
    def __init__(self, B, T):
        import oracle
        import reviews4rec_amd
        from reviews4rec_amd.engine import DeepCoNNEngine
        hp = dict(model_type='deepconn', latent_size=SL, word_embed_size=SE, input_length=T, dropout=0.3,
                  total_users=SU, total_items=SI, lr=0.002, weight_decay=1e-6)
        P = oracle.init_params(hp, vocab_size=SV, seed=3)
        model = reviews4rec_amd.get_model_class('deepconn')(dict(hp, word_vectors=P['word2vec.weight'].numpy()))
        model.load_state_dict(P)
        self.B = B
        self.eng = DeepCoNNEngine(model.to(DEV).train(), lr=hp['lr'], weight_decay=hp['weight_decay'], seed=99,
                                  conv_algo=PROJECT)

    def snapshot(self):
        torch.cuda.synchronize()
        e = self.eng
        snap = {'pred': e._outputs(self.B)[0], 'se': e._outputs(self.B)[1], 'p': e.flat_p, 'm': e.flat_m, 'v': e.flat_v,
                'sse': e.sse}
        return {k: v.cpu().numpy().copy() for k, v in snap.items()}


def same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), '%s: %s differs' % (what, k)


def test_span_of_eight_steps_leaves_the_bits_of_eight_single_steps():
    """r4r_deepconn_span, eight steps in one call, against the same steps one at a time -- both in four launches -- and
    against the span with the old tail forced."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd.data import SpanDescriptor
    lib = _lib.lib()
    B, T = 37, 200
    batches = span_batches(B, T)
    try:
        lib.r4r_deepconn_tail_fold(1)
        assert lib.r4r_deepconn_tail(B, SE, SL) == 1
        single = SpanRun(B, T)
        for k in range(8):
            single.eng.train_step(*batches[k % 4], next_data=batches[(k + 1) % 4][0])
        last = single.snapshot()
        span = SpanRun(B, T)
        span.eng._span(SpanDescriptor.resident(batches), 0, 8, True)
        assert span.eng.step_count == single.eng.step_count == 8
        got = span.snapshot()
        same_bits(last, got, 'span')
        lib.r4r_deepconn_tail_fold(0)
        old = SpanRun(B, T)
        old.eng._span(SpanDescriptor.resident(batches), 0, 8, True)
        same_bits(got, old.snapshot(), 'span, old tail')
    finally:
        lib.r4r_deepconn_tail_fold(1)
