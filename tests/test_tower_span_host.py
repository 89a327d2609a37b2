"""Tower spans without a GPU (include/r4r.h "Tower spans", csrc/tower_span.hip; recommend.Catalogue(towers=...)): the
header declares the entry points, every refusal of r4r_tower_build / r4r_tower_span_fwd happens on the host before anything
is launched or dereferenced (the pointers passed here are not addresses of anything), and the Python surface refuses an
unknown ``towers`` / hyper_params['catalogue_towers'] and leaves requests without the key as they were."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_WS = 0, -1, -3
P = 4096                                                    # a non-null "pointer": never dereferenced by a refusal


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def span_args(**kw):
    """r4r_tower_span_fwd's arguments by name (the header's order), a valid DeepCoNN-shaped call unless overridden."""
    a = dict(tok=P, rev_off=P, first=P, nb=P, owners=100, ids=P, n=70, group=32, T=64, R=0, W=0, pad=0, table=P, V=400,
             conv_w=P, conv_b=P, fc_w=P, fc_b=P, E=20, F=100, L=8, latent=P, neigh=None, ws=P, ws_bytes=1 << 40,
             groups_done=None, stream=None)
    unknown = set(kw) - set(a)
    assert not unknown, unknown
    a.update(kw)
    return a


def call(lib, name, args):
    from reviews4rec_amd import _lib
    names = _lib.parse_header()[name][2]
    assert list(args) == names, (list(args), names)         # the dict above IS the header's argument list
    return getattr(lib, name)(*args.values())


def test_the_header_declares_the_tower_span_entry_points(lib):
    from reviews4rec_amd import _lib
    names = _lib.declared_symbols()
    for must in ('r4r_tower_build', 'r4r_tower_span_ws_bytes', 'r4r_tower_span_fwd'):
        assert must in names and hasattr(lib, must), must
    decls = _lib.parse_header()
    assert decls['r4r_tower_span_ws_bytes'][0] is ctypes.c_size_t
    assert decls['r4r_tower_build'][2] == ['tok', 'rev_off', 'first', 'nb', 'owners', 'ids', 'n', 'T', 'R', 'W', 'pad',
                                          'docs', 'neigh', 'stream']


def test_the_group_cites_what_it_replaces():
    src = open(os.path.join(ROOT, 'include', 'r4r.h')).read()
    group = src[src.index('Tower spans: one side'):src.index('int r4r_tower_build(')]
    for cite in ('data.py:240-246', 'data.py:181-210', 'data.py:144-172', 'data.py:275-279'):
        assert cite in group, cite
    for site in ('_documents', '_tower', '_attended'):
        assert re.search(r'\b%s\b' % site, group), site


@pytest.mark.parametrize('what, over, rc, msg', [
    ('null pool', dict(tok=None), ERR_ARG, b'null pointer'),
    ('null ids', dict(ids=None), ERR_ARG, b'null pointer'),
    ('null table', dict(table=None), ERR_ARG, b'null pointer'),
    ('null fc bias', dict(fc_b=None), ERR_ARG, b'null pointer'),
    ('null latent', dict(latent=None), ERR_ARG, b'null pointer'),
    ('null workspace', dict(ws=None), ERR_ARG, b'null pointer'),
    ('NARRE without neigh', dict(R=10, W=16, neigh=None), ERR_ARG, b'null pointer'),
    ('group 0', dict(group=0), ERR_ARG, b'group'),
    ('group -3', dict(group=-3), ERR_ARG, b'group'),
    ('E % 4', dict(E=50), ERR_ARG, b'multiple of 4'),
    ('E 0', dict(E=0), ERR_ARG, b'multiple of 4'),
    ('F 113', dict(F=113), ERR_ARG, b'112'),
    ('T 0', dict(T=0), ERR_ARG, b'bad shape'),
    ('R without W', dict(R=10, W=0, neigh=P), ERR_ARG, b'bad shape'),
    ('R negative', dict(R=-1), ERR_ARG, b'bad shape'),
    ('n negative', dict(n=-1), ERR_ARG, b'bad shape'),
    ('n 2^31', dict(n=1 << 31), ERR_ARG, b'bad shape'),
    ('owners negative', dict(owners=-1), ERR_ARG, b'bad shape'),
    ('no workspace bytes', dict(ws_bytes=0), ERR_WS, b'workspace'),
])
def test_span_refusals_need_no_gpu(lib, what, over, rc, msg):
    done = ctypes.c_int64(-7)
    got = call(lib, 'r4r_tower_span_fwd', span_args(groups_done=ctypes.byref(done), **over))
    assert got == rc, (what, got, lib.r4r_last_error())
    assert msg in lib.r4r_last_error(), (what, lib.r4r_last_error())
    assert done.value == 0, what                            # no round was enqueued


@pytest.mark.parametrize('shape', [dict(T=64), dict(R=10, W=16, neigh=P), dict(T=300, E=52, n=5, group=256)])
def test_a_workspace_one_byte_short_is_refused(lib, shape):
    """r4r_tower_span_ws_bytes is what the span asks for: one byte less than a full group's is R4R_ERR_WORKSPACE."""
    a = span_args(**shape)
    G = min(a['group'], a['n'])                             # (the span lays its workspace out for its largest round)
    need = lib.r4r_tower_span_ws_bytes(G, a['T'], a['R'], a['W'], a['E'], a['F'], a['L'], a['V'])
    rows, width = G * max(a['R'], 1), a['W'] if a['R'] else a['T']
    assert need >= rows * width * 8 + 2 * rows * a['F'] * 4 + lib.r4r_textcnn_ws_bytes(rows, width, a['E'], a['F'], a['V'])
    assert lib.r4r_tower_span_ws_bytes(a['group'], a['T'], a['R'], a['W'], a['E'], a['F'], a['L'], a['V']) >= need
    done = ctypes.c_int64(-7)
    assert call(lib, 'r4r_tower_span_fwd', span_args(ws_bytes=need - 1, groups_done=ctypes.byref(done), **shape)) == ERR_WS
    assert b'workspace' in lib.r4r_last_error() and done.value == 0


def test_ws_bytes_of_a_bad_shape_is_zero(lib):
    assert lib.r4r_tower_span_ws_bytes(32, 64, 0, 0, 20, 100, 8, 400) > 0
    for bad in ((0, 64, 0, 0, 20, 100, 8, 400), (32, 0, 0, 0, 20, 100, 8, 400), (32, 64, 10, 0, 20, 100, 8, 400),
                (32, 64, 0, 0, 0, 100, 8, 400), (32, 64, 0, 0, 20, 0, 8, 400), (32, 64, 0, 0, 20, 100, 8, 0)):
        assert lib.r4r_tower_span_ws_bytes(*bad) == 0, bad


def test_an_empty_span_is_a_no_op(lib):
    done = ctypes.c_int64(-7)
    assert call(lib, 'r4r_tower_span_fwd', span_args(n=0, groups_done=ctypes.byref(done))) == OK and done.value == 0
    assert call(lib, 'r4r_tower_span_fwd', span_args(n=0, groups_done=None)) == OK


def test_build_refusals_need_no_gpu(lib):
    def build(**kw):
        a = dict(tok=P, rev_off=P, first=P, nb=P, owners=100, ids=P, n=5, T=64, R=0, W=0, pad=0, docs=P, neigh=None,
                 stream=None)
        a.update(kw)
        return call(lib, 'r4r_tower_build', a)
    assert build(n=0) == OK and build(n=0, tok=None, docs=None) == OK          # nothing to do: nothing is looked at
    for over in (dict(tok=None), dict(rev_off=None), dict(first=None), dict(ids=None), dict(docs=None),
                 dict(R=10, W=16)):                                              # (NARRE needs neigh)
        assert build(**over) == ERR_ARG and b'null pointer' in lib.r4r_last_error(), over
    for over in (dict(T=0), dict(R=10, W=0, neigh=P), dict(R=-1), dict(n=-1), dict(n=1 << 31), dict(owners=-1)):
        assert build(**over) == ERR_ARG and b'bad shape' in lib.r4r_last_error(), over


# ---------------------------------------------------------------- the Python surface
@pytest.mark.parametrize('cls', ['Catalogue', 'ReluCatalogue', 'NarreCatalogue', 'TransNetCatalogue'])
def test_an_unknown_towers_value_is_a_value_error(cls):
    """Before anything else is looked at: the model, the limits, the device."""
    from reviews4rec_amd import recommend
    for bad in ('x', 'Device', None, 1):
        with pytest.raises(ValueError, match='towers'):
            getattr(recommend, cls)(None, {'model_type': 'deepconn'}, None, towers=bad)
    assert recommend.TOWERS == ('host', 'device')


def test_the_default_is_the_host_path():
    import inspect
    from reviews4rec_amd import recommend
    assert inspect.signature(recommend.Catalogue.__init__).parameters['towers'].default == 'host'
    assert 'towers' not in inspect.signature(recommend.MFCatalogue.__init__).parameters


@pytest.mark.parametrize('mt', ['deepconn', 'deepconn++', 'MF_dot', 'bias_only'])
def test_request_checks_refuse_an_unknown_catalogue_towers(mt):
    from reviews4rec_amd.recommend import check_catalogue_metrics_request, check_recommend_request
    hp = dict(model_type=mt, latent_size=8)
    rec, met = dict(hp, recommend_k=3, recommend_path='lists.npz'), dict(hp, catalogue_metrics_k=[1, 5])
    for bad in ('x', 'gpu', '', None, 0):
        with pytest.raises(RuntimeError, match='catalogue_towers'):
            check_recommend_request(dict(rec, catalogue_towers=bad))
        with pytest.raises(RuntimeError, match='catalogue_towers'):
            check_catalogue_metrics_request(dict(met, catalogue_towers=bad))
    for good in ('host', 'device'):
        check_recommend_request(dict(rec, catalogue_towers=good))
        check_catalogue_metrics_request(dict(met, catalogue_towers=good))
    # without the key: accepted as before; without a request: nothing is looked at
    check_recommend_request(rec)
    check_catalogue_metrics_request(met)
    check_recommend_request(dict(hp, catalogue_towers='x'))
    check_catalogue_metrics_request(dict(hp, catalogue_towers='x'))


def test_main_refuses_an_unknown_catalogue_towers_before_anything_is_loaded():
    from reviews4rec_amd import main as M
    hp = dict(model_type='deepconn', latent_size=8, data_dir='/nonexistent/', catalogue_towers='x')
    with pytest.raises(RuntimeError, match='catalogue_towers'):
        M.main(dict(hp, recommend_k=3, recommend_path='lists.npz'))
    with pytest.raises(RuntimeError, match='catalogue_towers'):
        M.main(dict(hp, catalogue_metrics_k=[1, 5]))


def test_make_catalogue_passes_the_key_on(monkeypatch):
    from reviews4rec_amd import recommend
    seen = []

    class Stub:
        def __init__(self, model, hp, reader, engine=None, towers='host'):
            seen.append(towers)
    monkeypatch.setattr(recommend, 'Catalogue', Stub)
    monkeypatch.setattr(recommend, 'ReluCatalogue', Stub)
    for mt in ('deepconn', 'deepconn++'):
        recommend.make_catalogue(None, dict(model_type=mt, latent_size=8), None)
        recommend.make_catalogue(None, dict(model_type=mt, latent_size=8, catalogue_towers='device'), None)
    assert seen == ['host', 'device', 'host', 'device']
