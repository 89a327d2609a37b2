"""Host side of the data-parallel spans of the native families other than DeepCoNN (include/r4r.h "Spans",
csrc/span.hip: r4r_narre_span_dp, r4r_deepconnpp_span_dp, r4r_transnet_span_dp, r4r_idnet_span_dp, r4r_mf_span_dp).
No GPU is needed: the entry points are declared, exported and bound, and every argument is checked before anything is
enqueued -- a refusal names the entry point and leaves *steps_done at 0.  The loop they replace is the reference's
main.py:23-60 on every rank, plus the gradient exchange of reviews4rec_amd/engine.py _train_step_dp."""
import ctypes

import pytest

from reviews4rec_amd import _lib

NAMES = ['r4r_narre_span_dp', 'r4r_deepconnpp_span_dp', 'r4r_transnet_span_dp', 'r4r_idnet_span_dp', 'r4r_mf_span_dp']
WORDS = 28
FAKE = 0x7f0000001000              # a device address no refused call ever reads


def test_declared_exported_and_bound():
    lib, decl = _lib.lib(), _lib.parse_header()
    for n in NAMES:
        assert n in decl, n
        restype, argtypes, argnames = decl[n]
        assert argnames[0] == 'loader', n
        fn = getattr(lib, n)
        assert fn.argtypes == argtypes and fn.restype is ctypes.c_int, n
        # the exchange: RCCL's entry points passed in, never linked
        assert {'allgather', 'comm', 'world', 'B_pad', 'block', 'blocks'} <= set(argnames), n
        assert ('allreduce' in argnames) == (n != 'r4r_mf_span_dp'), n


class _Host:
    """Host memory a call may read before it refuses: the resident descriptor, the state cells, the pointer arrays."""

    def __init__(self):
        self.table = (ctypes.c_uint64 * 8)(*([FAKE] * 8))
        w = [0] * WORDS
        w[24], w[25], w[26], w[27] = 1 << 20, 1, 32, ctypes.addressof(self.table)   # N, G, B, a resident table
        self.loader = (ctypes.c_uint64 * WORDS)(*w)
        self.built = ctypes.c_int64(-1)
        self.done = ctypes.c_int64(7)
        self.base = ctypes.c_int64(0)
        self.period = ctypes.c_int(1)
        self.ptrs = [(ctypes.c_uint64 * 8)(*([FAKE] * 8)) for _ in range(4)]


def _args(name, h, **over):
    """Every argument of `name` by its header name: a call that would pass every check, with `over` applied."""
    _, _, argnames = _lib.parse_header()[name]
    ints = dict(first_batch=0, steps=2, announce=0, V=400, n_users=300, n_items=120, ws_bytes=1 << 20, R=10, T=12, E=16,
                L=8, D=8, training=1, seed=1, offset=0, draws_per_step=0, conv_algo=0, token_buffer=0, tokens_ready=0,
                total=64, adam_step=1, world=1, B_pad=32, variant=0, plus=0, sweep_period=1, sweep_want=1)
    floats = dict(dropout_p=0.5, inv_denom=1.0 / 32, lr=0.002, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-6)
    host = dict(loader=h.loader, built_group=ctypes.byref(h.built), steps_done=ctypes.byref(h.done),
                sweep_base=ctypes.byref(h.base), sweep_period_out=ctypes.byref(h.period), rows_p=h.ptrs[0],
                rows_m=h.ptrs[1], rows_v=h.ptrs[2], p=h.ptrs[0], m=h.ptrs[1], v=h.ptrs[2], gathered=h.ptrs[3])
    out = []
    for a in argnames:
        if a in over:
            out.append(over[a])
        elif a in host:
            out.append(host[a])
        elif a in ints:
            out.append(ints[a])
        elif a in floats:
            out.append(floats[a])
        elif a == 'stream':
            out.append(None)
        else:
            out.append(FAKE)                                 # device buffers and the collectives' addresses
    return out


def _refused(name, **over):
    h = _Host()
    lib = _lib.lib()
    rc = getattr(lib, name)(*_args(name, h, **over))
    return rc, h.done.value, lib.r4r_last_error().decode()


MOMENTS = {'r4r_narre_span_dp': 'flat_m', 'r4r_deepconnpp_span_dp': 'flat_v', 'r4r_transnet_span_dp': 'flat_m',
           'r4r_idnet_span_dp': 'flat_v', 'r4r_mf_span_dp': 'm'}


@pytest.mark.parametrize('name,what', [(n, w) for n in NAMES for w in ('allreduce', 'allgather', 'comm', 'world',
                                                                         'adam_step', 'moments')
                                        if not (w == 'allreduce' and n == 'r4r_mf_span_dp')])   # (MF_dot: all-gather only)
def test_every_refusal_names_the_entry_point_before_anything_is_enqueued(name, what):
    over = {'world': {'world': 0}, 'adam_step': {'adam_step': 0}, 'moments': {MOMENTS[name]: None}}.get(what, {what: None})
    rc, done, err = _refused(name, **over)
    assert rc != 0 and done == 0, (name, what, rc, done)
    assert name[len('r4r_'):] in err, err


@pytest.mark.parametrize('R', [0, 9, 12])
def test_narre_refuses_r_other_than_the_ring_s_neighbour_width(R):
    rc, done, err = _refused('r4r_narre_span_dp', R=R)
    assert rc != 0 and done == 0 and 'narre_span_dp' in err and 'R = %d' % R in err, err


@pytest.mark.parametrize('name,over', [
    ('r4r_narre_span_dp', dict(world=2, B_pad=1024)),          # 2 x 1024 x 11 entries > 16384: not the block form
    ('r4r_narre_span_dp', dict(L=40)),                         # rows wider than the block form keeps
    ('r4r_transnet_span_dp', dict(plus=1, world=2, B_pad=1025)),  # TransNet++: world x B_pad > 2048
    ('r4r_deepconnpp_span_dp', dict(world=2, B_pad=8193)),
    ('r4r_idnet_span_dp', dict(world=4, B_pad=4097)),
    ('r4r_mf_span_dp', dict(world=8, B_pad=2049)),
    ('r4r_mf_span_dp', dict(B_pad=16)),                        # the loader's B = 32 does not fit the padded shard
    ('r4r_idnet_span_dp', dict(B_pad=31)),
    ('r4r_deepconnpp_span_dp', dict(gathered=None)),
    ('r4r_transnet_span_dp', dict(plus=1, blocks=None)),
    ('r4r_mf_span_dp', dict(block=None)),
])
def test_forms_outside_the_packed_blocks_are_refused(name, over):
    rc, done, err = _refused(name, **over)
    assert rc != 0 and done == 0 and name[len('r4r_'):] in err, (over, err)


def test_transnet_refusal_keeps_the_schedule_passed_in():
    h = _Host()
    h.period.value = 0
    rc = _lib.lib().r4r_transnet_span_dp(*_args('r4r_transnet_span_dp', h, sweep_period=4, comm=None))
    assert rc != 0 and h.period.value == 4 and h.base.value == 0 and h.done.value == 0


def test_the_engines_take_the_dp_span_only_over_the_on_stream_communicator():
    """engine._Spans._span_dp_ok / _span_dp_form on stand-ins (no device): RCCL's communicator on the stream, MF_dot's
    all-gather form only, every family's packed-block limits; outside them train_step carries the step."""
    from types import SimpleNamespace as NS
    from reviews4rec_amd.engine import IdNetEngine, MFEngine, NarreEngine, TransNetEngine

    def dp(world=1, comm=True, rccl=True):
        return NS(on=True, world=world, stream_rccl=NS(comm=FAKE if comm else None) if rccl else None)

    desc = NS(batch_size=32, review=True, doc_shape=(10, 12))
    mf = MFEngine.__new__(MFEngine)
    mf.dp, mf.hp, mf.exchange = dp(), {'batch_size': 32}, ''
    assert mf._span_dp_ok() and mf._span_limit(desc) == mf.SPAN_STEPS
    mf.exchange = 'peer'
    assert not mf._span_dp_ok()
    mf.exchange, mf.dp = '', dp(rccl=False)                    # a gloo job: torch.distributed's collectives
    assert not mf._span_dp_ok()
    mf.dp = dp(comm=False)
    assert not mf._span_dp_ok()
    mf.dp, mf.hp = dp(world=8), {'batch_size': 4096}           # 32,768 gathered ratings: beyond the block form
    assert mf._span_limit(desc) == 0
    mf.dp, mf.hp = dp(), {'batch_size': 16}                    # a shard beyond hyper_params['batch_size']
    assert mf._span_limit(desc) == 0

    idn = IdNetEngine.__new__(IdNetEngine)
    idn.dp, idn.hp = dp(), {'batch_size': 32}
    assert idn._span_dp_ok() and idn._span_limit(desc) == idn.SPAN_STEPS

    narre = NarreEngine.__new__(NarreEngine)
    narre.dp, narre.hp, narre.L = dp(), {'batch_size': 32}, 8
    assert narre._span_dp_ok() and narre._span_dp_form(desc)
    narre.dp, narre.hp = dp(world=2), {'batch_size': 1024}
    assert not narre._span_dp_form(NS(batch_size=1024, review=True, doc_shape=(10, 12)))

    tn = TransNetEngine.__new__(TransNetEngine)
    d1 = NS(batch_size=1024, review=True, doc_shape=(64,))
    tn.dp, tn.hp, tn.plus, tn.L = dp(world=4), {'batch_size': 1024}, 0, 8
    assert tn._span_dp_form(d1)                                # plain TransNet exchanges no rows
    tn.plus = 1
    assert not tn._span_dp_form(d1)                            # TransNet++: 4,096 > 2,048 gathered ratings
