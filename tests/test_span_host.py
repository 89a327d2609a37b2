"""Host side of the span entry points (include/r4r.h "Spans", csrc/span.hip, engine._Spans) where no GPU is needed:
the descriptor's batch arithmetic (r4r_span_batch is pure host code), its argument checks, the resident-table form,
and the conv rule's span planning against its per-step twin.  The loop these replace: /root/reference/main.py:23-60
over data_fast.py:99-109 / data.py:250-372 (contiguous slices of batch_size ratings, ragged tail)."""
import ctypes

import pytest

from reviews4rec_amd import _lib

WORDS = 28


def _desc(**kw):
    w = [0] * WORDS
    for k, v in kw.items():
        w[int(k[1:])] = v
    return (ctypes.c_uint64 * WORDS)(*w)


def _slots(words, b):
    out = (ctypes.c_uint64 * 8)()
    rc = _lib.lib().r4r_span_batch(words, b, out)
    return rc, list(out)


def test_batch_pointers_follow_the_group_layout():
    """Batch b lives in group b // G, ring slot (b // G) & 1, as rows [j B, (j + 1) B) of the group's five fields
    [n, doc] [n, 10] [n, 10] [n, doc] [n, doc] (r4r_batch_build's block for the group's n ratings)."""
    B, G, T, N = 8, 4, 16, 8 * 11 + 5                       # 11 full batches: groups of 4, 4, 3; a ragged tail of 5
    ring, stride = 0x100000, 4 * 8 * (3 * 16 + 20) + 64
    u, i, y = 0x2000000, 0x3000000, 0x4000000
    words = _desc(w10=u, w11=i, w12=1, w13=1, w14=1, w15=y, w17=T, w22=ring, w23=stride, w24=N, w25=G, w26=B)
    for b in range(11):
        g, j = divmod(b, G)
        n = min(G * B, 11 * B - g * G * B)
        base = ring + (g & 1) * stride * 8
        rc, s = _slots(words, b)
        assert rc == 0
        assert s[0] == base + 8 * (j * B * T)
        assert s[1] == base + 8 * (n * T + j * B * 10)
        assert s[2] == base + 8 * (n * T + n * 10 + j * B * 10)
        assert s[3] == base + 8 * (n * T + 2 * n * 10 + j * B * T)
        assert s[4] == base + 8 * (2 * n * T + 2 * n * 10 + j * B * T)
        assert s[5:] == [u + 8 * b * B, i + 8 * b * B, y + 4 * b * B]
    assert _slots(words, 11)[0] != 0                        # the ragged tail is not a span batch
    assert _slots(words, -1)[0] != 0
    # NARRE: documents are R x W
    words = _desc(w10=u, w11=i, w12=1, w13=1, w14=1, w15=y, w17=100, w18=10, w19=12, w22=ring, w23=10 ** 6, w24=64, w25=2, w26=8)
    rc, s = _slots(words, 3)
    assert rc == 0 and s[3] - s[0] == 8 * (16 * 120 + 2 * 16 * 10)


def test_descriptor_checks():
    lib = _lib.lib()
    assert lib.r4r_span_batch(None, 0, (ctypes.c_uint64 * 8)()) != 0 and b'span' in lib.r4r_last_error()
    small = _desc(w10=1, w11=1, w12=1, w13=1, w14=1, w15=1, w17=16, w22=0x1000, w23=10, w24=64, w25=4, w26=8)
    assert _slots(small, 0)[0] != 0 and b'stride' in lib.r4r_last_error()       # the ring cannot hold a group
    no_ids = _desc(w17=16, w24=64, w26=8)
    assert _slots(no_ids, 0)[0] != 0
    built = ctypes.c_int64(-1)
    ids_only = _desc(w10=1, w11=1, w15=1, w24=64, w26=8)
    assert lib.r4r_span_build(ids_only, 0, ctypes.byref(built), None) != 0       # nothing to build for an ids-only loader
    rc, s = _slots(ids_only, 7)
    assert rc == 0 and s[:5] == [0] * 5 and s[5] == 1 + 8 * 56


def test_resident_table_cycles():
    """Word 27: a host table of G built batches; batch b is entry b % G, nothing is constructed."""
    G = 3
    table = (ctypes.c_uint64 * (8 * G))(*range(100, 100 + 8 * G))
    words = _desc(w24=1 << 40, w25=G, w26=128, w27=ctypes.addressof(table))
    for b in (0, 1, 2, 3, 7, 3000001):
        rc, s = _slots(words, b)
        assert rc == 0 and s == list(range(100 + 8 * (b % G), 108 + 8 * (b % G)))


def test_every_declared_span_symbol_is_exported():
    lib, decl = _lib.lib(), _lib.parse_header()
    names = [n for n in decl if n.endswith('_span') or n.startswith('r4r_span_')]
    assert sorted(names) == sorted(['r4r_span_build', 'r4r_span_batch', 'r4r_deepconn_span', 'r4r_deepconnpp_span',
                                    'r4r_narre_span', 'r4r_transnet_span', 'r4r_mf_span', 'r4r_idnet_span'])
    for n in names:
        assert getattr(lib, n) is not None
        # a span's arguments are its family's step arguments: the per-step pointers give way to the descriptor
        assert decl[n][2][0] == 'loader'


@pytest.mark.parametrize('E,V,T,docs', [(304, 50002, 1000, 128), (64, 50002, 100, 1280), (64, 1000000, 1000, 128)])
def test_span_planning_agrees_with_the_per_step_rule(E, V, T, docs):
    """engine._ConvRule: _rule_peek (what a span may cover) against _rule_request (what every single step asks for):
    a span never contains a probing step, carries the request its steps would have made, and advances the rule's count
    like they would."""
    from reviews4rec_amd.engine import _ConvRule

    class Rule(_ConvRule):
        def __init__(self):
            self.E, self.V, self.conv_algo, self.gemm_math = E, V, 0, 'f32'
            self._rule_reset()

    a, b = Rule(), Rule()
    step = 0
    while step < 2200:
        limit, req, algo, counted = b._rule_peek(docs, T)
        if limit <= 0:                                      # the next step is its own: it must be a probing one
            r, al, probe = a._rule_request(docs, T, True)
            assert probe
            b._rule_request(docs, T, True)
            a._rule_choice = b._rule_choice = 2             # (what a probe would have decided)
            step += 1
            continue
        k = min(limit, 64)
        for _ in range(k):
            r, al, probe = a._rule_request(docs, T, True)
            assert not probe and (r, al) == (req, algo)
        b._rule_advance(k, counted)
        assert a._rule_n == b._rule_n
        # `ahead`: the planner's look past the span it is about to issue
        assert (b._rule_peek(docs, T)[0] > 0) == (Rule._rule_peek(a, docs, T)[0] > 0)
        step += k


# ---- the shape a span's step reads against the documents the descriptor's ring holds (csrc/span.hip, check_doc_shape).
# The step indexes the ring's blocks by its own (R, T): NARRE's neighbour ids as b*R + r of a list NEIGHBOURS = 10 wide
# (data.py:275-279), the documents as B x doc.  A mismatch must be refused before anything is enqueued -- every call
# below would otherwise launch on these fake device pointers.
FAKE = 0x7f0000000000                                       # never dereferenced: the checks run on the host first


def _span_call(name, words, **over):
    """Call r4r_<name>_span with fake device pointers and real host out-parameters -> (rc, steps_done, last error)."""
    lib, decl = _lib.lib(), _lib.parse_header()
    built, done = ctypes.c_int64(-1), ctypes.c_int64(7)
    sweep_base, sweep_out = ctypes.c_int64(0), ctypes.c_int(-5)
    rows = (ctypes.c_uint64 * 4)(FAKE, FAKE, FAKE, FAKE)
    host = dict(loader=words, built_group=ctypes.byref(built), steps_done=ctypes.byref(done), rows_p=rows, rows_m=rows,
                rows_v=rows, sweep_base=ctypes.byref(sweep_base), sweep_period_out=ctypes.byref(sweep_out), stream=None)
    scalars = dict(first_batch=0, steps=2, announce=0, V=400, n_users=300, n_items=120, ws_bytes=1 << 20, E=16, L=8,
                   dropout_p=0.0, training=1, seed=1, offset=0, draws_per_step=0, inv_denom=1.0 / 8, lr=1e-3, beta1=0.9,
                   beta2=0.999, eps=1e-8, weight_decay=0.0, adam_step=1, sweep_period=1, sweep_want=1)
    args = []
    for a, t in zip(decl['r4r_%s_span' % name][2], decl['r4r_%s_span' % name][1]):
        if a in over:
            args.append(over[a])
        elif a in host:
            args.append(host[a])
        elif a in scalars:
            args.append(scalars[a])
        elif t is ctypes.c_void_p:
            args.append(FAKE)
        else:
            args.append(0)
    rc = getattr(lib, 'r4r_%s_span' % name)(*args)
    if name == 'transnet':
        assert sweep_out.value == 1 and sweep_base.value == 0   # (refused: the schedule is the one passed in)
    return rc, done.value, lib.r4r_last_error()


def _ring(T=64, R=0, W=0, B=8, G=4, N=8 * 11 + 5):
    doc = R * W if R else T
    return _desc(w0=FAKE, w1=FAKE, w2=FAKE, w3=FAKE, w4=FAKE, w5=FAKE, w6=FAKE, w7=FAKE, w8=FAKE, w9=FAKE,
                 w10=FAKE, w11=FAKE, w12=FAKE, w13=FAKE, w14=FAKE, w15=FAKE, w16=1, w17=T, w18=R, w19=W, w20=301,
                 w21=121, w22=FAKE, w23=G * B * (3 * doc + 20), w24=N, w25=G, w26=B)


@pytest.mark.parametrize('R', [5, 12, 32])
def test_narre_span_refuses_r_other_than_the_ring_s_neighbour_width(R):
    """R != 10: the ring holds 10 neighbour ids per rating, the step would read R (R < 10: the wrong neighbours;
    R > 10: document tokens as ids, then row tags written out of bounds) -- also when the descriptor agrees."""
    rc, done, err = _span_call('narre', _ring(R=R, W=12), R=R, T=12)
    assert rc != 0 and done == 0
    assert b'narre_span' in err and b'neighbour' in err, err


def test_narre_span_refuses_a_shape_the_descriptor_does_not_build():
    ring = _ring(R=10, W=12)
    for R, T in ((10, 11), (10, 13), (12, 12), (9, 12)):
        rc, done, err = _span_call('narre', ring, R=R, T=T)
        assert rc != 0 and done == 0, (R, T)
        assert b'narre_span' in err and (b'12' in err or b'neighbour' in err), (R, T, err)
    # a descriptor built for another R or W (the step's R, T are NARRE's 10 x 12)
    for R, W in ((12, 12), (5, 12), (10, 11), (10, 33)):
        rc, done, err = _span_call('narre', _ring(R=R, W=W), R=10, T=12)
        assert rc != 0 and done == 0, (R, W)
        assert b'descriptor builds %d x %d' % (R, W) in err, err
    # ... a DeepCoNN-shaped ring (one T-token document per rating), an ids-only loader
    rc, done, err = _span_call('narre', _ring(T=120), R=10, T=12)
    assert rc != 0 and done == 0 and b'0 x 0' in err, err
    ids_only = _desc(w10=FAKE, w11=FAKE, w15=FAKE, w24=64, w26=8)
    rc, done, err = _span_call('narre', ids_only, R=10, T=12)
    assert rc != 0 and done == 0 and b'ids-only' in err, err


@pytest.mark.parametrize('name', ['deepconn', 'deepconnpp', 'transnet'])
def test_document_span_refuses_a_t_the_descriptor_does_not_build(name):
    for T in (63, 65, 32, 128):
        rc, done, err = _span_call(name, _ring(T=64), T=T)
        assert rc != 0 and done == 0, T
        assert (b'%s_span' % name.encode()) in err and b'T = %d' % T in err and b'T = 64' in err, err
    rc, done, err = _span_call(name, _ring(R=10, W=12), T=120)       # NARRE's ring: R x W reviews, not a T document
    assert rc != 0 and done == 0 and b'R x W = 120' in err, err
    ids_only = _desc(w10=FAKE, w11=FAKE, w15=FAKE, w24=64, w26=8)
    rc, done, err = _span_call(name, ids_only, T=64)
    assert rc != 0 and done == 0 and b'ids-only' in err, err


def test_resident_descriptor_narre_needs_the_neighbour_width():
    """Word 27 (bench.py's pool): no shape in the descriptor; NARRE's R must still be the lists' width."""
    table = (ctypes.c_uint64 * 8)(*([FAKE] * 8))
    words = _desc(w24=1 << 40, w25=1, w26=8, w27=ctypes.addressof(table))
    for R in (5, 12, 32):
        rc, done, err = _span_call('narre', words, R=R, T=12)
        assert rc != 0 and done == 0 and b'neighbour' in err, (R, err)


class _Desc:
    def __init__(self, doc_shape, batch_size=32, review=True):
        self.doc_shape, self.batch_size, self.review = doc_shape, batch_size, review


def _stub(cls, **kw):
    e = cls.__new__(cls)
    e.L, e.gemm_math = 8, 'f32'
    e.__dict__.update(kw)
    return e


@pytest.mark.parametrize('R', [5, 10, 12, 32])
def test_narre_span_doc_only_for_the_ring_s_neighbour_width(R):
    from reviews4rec_amd.data import NEIGHBOURS
    from reviews4rec_amd.engine import NarreEngine
    e = _stub(NarreEngine)
    for W in (1, 12, 33):
        got = e._span_doc(_Desc((R, W)))
        if R == NEIGHBOURS:
            assert got == (R, W) and e._span_ok(_Desc((R, W)))
        else:
            assert got is None and not e._span_ok(_Desc((R, W)))     # train_step raises its own error instead


def test_no_spans_under_the_fp16_split_gemm():
    """R4R_GEMM_MATH=f16x2 refreshes its scales between steps (_rule_peek: no span may carry a step): main.train must
    keep its own loop, which announces every next batch (next_data), rather than a span-less train_epoch."""
    from reviews4rec_amd.engine import DeepCoNNEngine, DeepCoNNPPEngine, NarreEngine, TransNetEngine
    for cls, shape in ((DeepCoNNEngine, (64,)), (NarreEngine, (10, 12)), (DeepCoNNPPEngine, (64,)),
                       (TransNetEngine, (64,))):
        assert _stub(cls, gemm_math='f32')._span_ok(_Desc(shape)), cls
        assert not _stub(cls, gemm_math='f16x2')._span_ok(_Desc(shape)), cls
