"""Full-catalogue ranking metrics, the parts that need no GPU: r4r_rank_dot's refusals (include/r4r.h, "Catalogue
recommendation"), recommend.ranking_metrics against hand-computed values, eval.eval_catalogue's bookkeeping over a
stand-in catalogue, and main's refusal of hyper_params['catalogue_metrics_k'] before anything is loaded."""
import ctypes
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def _rank(lib, **kw):
    """r4r_rank_dot with well-formed defaults (host addresses: every refusal precedes the first dereference)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(q=p, n_q=33, q_bias=p, c=p, n_c=4099, c_stride=8, c_bias=p, D=8, q_idx=p, t_idx=p, n_p=200, excl_off=None,
             excl_ids=None, chunk=100, out_rank=p, out_score=p)
    a.update(kw)
    rc = lib.r4r_rank_dot(a['q'], a['n_q'], a['q_bias'], a['c'], a['n_c'], a['c_stride'], a['c_bias'], a['D'], a['q_idx'],
                          a['t_idx'], a['n_p'], a['excl_off'], a['excl_ids'], a['chunk'], a['out_rank'], a['out_score'],
                          None)
    return rc, lib.r4r_last_error() or b'', buf


def test_symbol_is_declared_and_exported(lib):
    from reviews4rec_amd import _lib
    assert 'r4r_rank_dot' in _lib.declared_symbols() and hasattr(lib, 'r4r_rank_dot')
    restype, argtypes, names = _lib.parse_header()['r4r_rank_dot']
    assert restype is ctypes.c_int
    assert names == ['q', 'n_q', 'q_bias', 'c', 'n_c', 'c_stride', 'c_bias', 'D', 'q_idx', 't_idx', 'n_p', 'excl_off',
                     'excl_ids', 'chunk', 'out_rank', 'out_score', 'stream']
    text = open(_lib.HEADER_PATH).read()
    assert 'eval.py:64-92' in text[text.index('r4r_rank_dot:'):]          # the call site this generalises


@pytest.mark.parametrize('kw, word', [
    (dict(D=-1), b'D'), (dict(D=257, c_stride=300), b'D'), (dict(c_stride=7), b'c_stride'),
    (dict(n_p=-1), b'negative'), (dict(n_q=-1), b'negative'), (dict(n_c=-1), b'negative'),
    (dict(chunk=-1), b'chunk'), (dict(chunk=(1 << 30) + 1), b'chunk'),
    (dict(n_p=1 << 40, chunk=1), b'grid'), (dict(n_c=1 << 40, n_p=1 << 20, chunk=1), b'grid'),
    (dict(out_rank=None), b'output'), (dict(out_score=None), b'output'),
    (dict(q_idx=None), b'null'), (dict(t_idx=None), b'null'), (dict(q=None), b'null'), (dict(c=None), b'null'),
    (dict(excl_off=1), b'excl'), (dict(excl_ids=1), b'excl'),
    (dict(n_q=0), b'empty'),
])
def test_refusals_need_no_gpu(lib, kw, word):
    if kw.get('excl_off') == 1 or kw.get('excl_ids') == 1:
        keep = ctypes.create_string_buffer(16)
        kw = {k: ctypes.addressof(keep) for k in kw}
    rc, msg, buf = _rank(lib, **kw)
    assert rc == -1 and word in msg, (rc, msg)
    assert buf.raw == b'\0' * 64                             # (no GPU here: a launch would have failed otherwise)


def test_zero_work_is_ok_and_leaves_the_outputs_untouched(lib):
    for kw in (dict(n_p=0), dict(n_c=0), dict(n_p=0, n_c=0), dict(n_p=0, out_rank=None, out_score=None),
               dict(n_p=0, n_q=0, q_idx=None, t_idx=None)):
        rc, msg, buf = _rank(lib, **kw)
        assert rc == 0, (kw, msg)
        assert buf.raw == b'\0' * 64
    # D = 0 needs neither q nor c: accepted up to the launch (there is no device here to take it)
    rc, msg, _ = _rank(lib, D=0, q=None, c=None, n_p=0)
    assert rc == 0, msg


def test_ranking_metrics_by_hand():
    import reviews4rec_amd
    from reviews4rec_amd.recommend import ranking_metrics
    assert reviews4rec_amd.ranking_metrics is ranking_metrics
    want_ndcg10 = (1 + 1 / math.log2(3) + 1 / math.log2(6) + 1 / math.log2(11)) / 5
    want_mrr = (1 + 1 / 2 + 1 / 5 + 1 / 10 + 1 / 11) / 5
    for ranks in ([0, 1, 4, 9, 10, -1], np.array([0, 1, 4, 9, 10, -1]), torch.tensor([0, 1, 4, 9, 10, -1])):
        m = ranking_metrics(ranks, (1, 5, 10))
        assert set(m) == {'HR@1', 'HR@5', 'HR@10', 'NDCG@1', 'NDCG@5', 'NDCG@10', 'MRR', 'ranked', 'unranked'}
        assert (m['HR@1'], m['HR@5'], m['HR@10']) == (1 / 5, 3 / 5, 4 / 5)
        assert abs(m['NDCG@10'] - want_ndcg10) <= 4 * np.finfo(np.float64).eps       # float64, nothing rounded
        assert abs(m['NDCG@5'] - (1 + 1 / math.log2(3) + 1 / math.log2(6)) / 5) <= 4 * np.finfo(np.float64).eps
        assert m['NDCG@1'] == 1 / 5
        assert abs(m['MRR'] - want_mrr) <= 4 * np.finfo(np.float64).eps
        assert m['ranked'] == 5 and m['unranked'] == 1 and isinstance(m['ranked'], int)
    with pytest.raises(ZeroDivisionError):
        ranking_metrics([-1, -1, -1], (1, 5, 10))
    with pytest.raises(ZeroDivisionError):
        ranking_metrics([], (1,))
    with pytest.raises(ValueError):
        ranking_metrics([0, 1], (0,))


class _Reader:
    def __init__(self, data):
        self.data = data


class _FixedCatalogue:
    """Catalogue.rank's surface with the ranks given: what eval_catalogue does around the device call."""

    def __init__(self, ranks):
        self.ranks, self.calls = ranks, []

    def rank(self, users, items, exclude_seen=True):
        self.calls.append((np.asarray(users).tolist(), np.asarray(items).tolist(), exclude_seen))
        return torch.tensor(self.ranks, dtype=torch.int64), torch.zeros(len(self.ranks))


def test_eval_catalogue_over_given_ranks():
    import reviews4rec_amd
    from reviews4rec_amd.eval import eval_catalogue
    assert reviews4rec_amd.eval_catalogue is eval_catalogue
    test = _Reader(np.array([[3, 7, 5.0], [3, 8, 1.0], [0, 2, 4.0], [1, 2, 4.0], [5, 5, 2.0], [6, 1, 3.0]]))
    cat = _FixedCatalogue([0, 1, 4, 9, 10, -1])
    m = eval_catalogue(None, None, test, {}, catalogue=cat)
    assert cat.calls == [([3, 3, 0, 1, 5, 6], [7, 8, 2, 2, 5, 1], True)]          # every row, training items excluded
    assert set(m) == {'cat_HR@1', 'cat_HR@5', 'cat_HR@10', 'cat_NDCG@1', 'cat_NDCG@5', 'cat_NDCG@10', 'cat_MRR',
                      'cat_ranked', 'cat_unranked'}
    assert (m['cat_HR@1'], m['cat_HR@5'], m['cat_HR@10']) == (20.0, 60.0, 80.0)
    assert m['cat_NDCG@10'] == 46.14 and m['cat_MRR'] == 37.82                    # percent, two places, like HR@1
    assert m['cat_ranked'] == 5 and m['cat_unranked'] == 1
    assert set(eval_catalogue(None, None, test, {}, ks=[3], catalogue=cat)) == {
        'cat_HR@3', 'cat_NDCG@3', 'cat_MRR', 'cat_ranked', 'cat_unranked'}
    with pytest.raises(ZeroDivisionError):                                        # like eval.py:90
        eval_catalogue(None, None, _Reader(test.data[:2]), {}, catalogue=_FixedCatalogue([-1, -1]))


@pytest.mark.parametrize('entry', ['main', 'main_pytorch', 'main_NeuMF'])
def test_catalogue_metrics_k_is_refused_before_anything_is_loaded(entry):
    from reviews4rec_amd import main as M
    from reviews4rec_amd.recommend import check_catalogue_metrics_request
    fn = getattr(M, entry)
    for mt in ('NARRE', 'NeuMF'):
        with pytest.raises(RuntimeError, match='catalogue_metrics_k.*no catalogue form'):
            fn(dict(model_type=mt, catalogue_metrics_k=[1, 5], data_dir='/nonexistent/'))
    for bad in ([], [0], '10', [1, -2], [1.5], 10, [True]):
        with pytest.raises(RuntimeError, match='catalogue_metrics_k.*non-empty list of positive ints'):
            fn(dict(model_type='MF_dot', latent_size=8, catalogue_metrics_k=bad, data_dir='/nonexistent/'))
    # a well-formed request for a model with a catalogue form passes the check; absent, nothing is asked
    for mt in ('bias_only', 'MF_dot', 'deepconn'):
        check_catalogue_metrics_request(dict(model_type=mt, latent_size=8, catalogue_metrics_k=[1, 5, 10]))
    check_catalogue_metrics_request(dict(model_type='NARRE'))
