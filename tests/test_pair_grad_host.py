"""Pair gradients (include/r4r.h, "Pair gradients"), the parts that need no GPU: pair_grad_ref's closed forms against
torch.autograd in float64, its bounds against a float32 evaluation in another summation order (the seeds and shapes
tests/test_gpu_pair_grad.py uses: the bounds can be met, and the ReLU margins hold), the mutants the bounds must catch,
every refusal of r4r_pair_grad (host addresses that are never dereferenced), and main's explain_pairs_k hook."""
import ctypes

import pytest
import torch

from head_ref import compare_all
from pair_grad_ref import (KINDS, MUTANTS, N_I, N_U, OUTPUTS, f32_of, pair_inputs, ref_of, shapes, with_zero_rows,
                           with_zero_unit)

OK, ERR_ARG = 0, -1
PTR = 4096                                                  # a non-null "pointer": never dereferenced by a refusal
NAME = b'r4r_pair_grad'
FM, MLP, PFM = 0, 1, 2
ALL = N_U * N_I                                             # every pair once


# ---------------------------------------------------------------- the closed forms are the gradients
def _torch_fm(x, V, lw):
    """TorchFM.forward without lin.bias (common_pytorch_models.py:49-57)."""
    out_1 = torch.matmul(x, V).pow(2).sum(1, keepdim=True)
    out_2 = torch.matmul(x.pow(2), V.pow(2)).sum(1, keepdim=True)
    return (0.5 * (out_1 - out_2) + torch.matmul(x, lw.reshape(-1, 1)))[:, 0]


def _torch_score(kind, zu, zi, p, eu, ei):
    """The three reference heads over the towers' outputs, in plain torch (DeepCoNN.py:61-72, TransNet.py:25-35, 105-114)."""
    cat = torch.cat([zu, zi], -1)
    if kind == 'fm':
        return _torch_fm(cat, p['V'], p['lw'])
    hidden = torch.relu(cat @ p['W0'].T + p['b0'])
    if kind == 'mlp':
        return hidden @ p['w3']
    ir = hidden @ p['W2'].T + p['b2']
    return _torch_fm(torch.cat([eu, ei, ir], -1) if eu is not None else ir, p['V'], p['lw'])


@pytest.mark.parametrize('kind, L, F, P', [('fm', 7, 9, 0), ('fm', 65, 100, 0), ('mlp', 7, 9, 0), ('mlp', 33, 100, 0),
                                           ('pfm', 7, 9, 0), ('pfm', 7, 9, 5), ('pfm', 33, 100, 5)])
def test_the_closed_forms_equal_autograd_in_float64(kind, L, F, P):
    d = pair_inputs(kind, L, F, P, n_p=ALL)
    f64 = lambda t: t.to(torch.float64)
    g = torch.Generator().manual_seed(5)
    pooled_u = torch.randn((N_U, F), generator=g, dtype=torch.float64).requires_grad_()
    pooled_i = torch.randn((N_I, F), generator=g, dtype=torch.float64).requires_grad_()
    bu, bi = torch.randn(L, generator=g, dtype=torch.float64), torch.randn(L, generator=g, dtype=torch.float64)
    zu, zi = pooled_u @ f64(d['fc_u']).T + bu, pooled_i @ f64(d['fc_i']).T + bi      # z = fc.weight pooled + fc.bias
    p = {k: f64(v) for k, v in d['params'].items()}
    u, i = d['u_idx'], d['i_idx']
    eu, ei = (p['xu'][u], p['xi'][i]) if P else (None, None)
    # one pair at a time: the gradient of ONE score with respect to the towers' outputs and the pooled features
    ref = pair_grad_ref_f64(kind, d, zu.detach(), zi.detach())
    for n in range(ALL):
        un, in_ = u[n:n + 1], i[n:n + 1]
        score = _torch_score(kind, zu[un], zi[in_], p, None if eu is None else eu[n:n + 1],
                             None if ei is None else ei[n:n + 1])[0] + f64(d['q_bias'])[un[0]] + f64(d['c_bias'])[in_[0]]
        g_zu, g_zi, g_pu, g_pi = torch.autograd.grad(score, [zu, zi, pooled_u, pooled_i], retain_graph=True)
        for name, want in (('score', score.detach()), ('g_user', g_zu[un[0]]), ('g_item', g_zi[in_[0]]),
                           ('w_user', g_pu[un[0]]), ('w_item', g_pi[in_[0]])):
            got = ref[name][0][n]
            scale = max(1.0, float(want.abs().max()))
            assert float((got - want).abs().max()) <= 1e-12 * scale, (kind, name, n)
        # every other row of the four gradients is zero: a pair's score depends on that pair's owners only
        others = torch.arange(N_U) != un[0]
        assert float(g_pu[others].abs().max()) == 0.0 and float(g_zu[others].abs().max()) == 0.0


def pair_grad_ref_f64(kind, d, zu, zi):
    from pair_grad_ref import pair_grad_ref
    return pair_grad_ref(kind, zu, zi, d['u_idx'], d['i_idx'], d['params'], d['fc_u'], d['fc_i'], d['q_bias'], d['c_bias'])


# ---------------------------------------------------------------- the bounds can be met, and the margins hold
@pytest.mark.parametrize('kind', KINDS)
def test_float32_in_another_order_stays_inside_the_bounds_at_every_gpu_shape(kind):
    """The inputs of a case do not depend on n_p and the indices past the first twelve repeat the twelve pairs, so the
    twelve pairs are every pair the GPU test sees; ``ref_of`` asserts the ReLU margins."""
    worst = 0.0
    for L, F, P in shapes(kind):
        for biases in (True, False):
            d = pair_inputs(kind, L, F, P, n_p=ALL, biases=biases)
            worst = max(worst, compare_all('%s L=%d F=%d P=%d' % (kind, L, F, P), f32_of(kind, d), ref_of(kind, d)))
    assert 0.0 < worst <= 1.0
    print('%s: worst float32 (numpy, descending order) error / bound %.3f' % (kind, worst))


@pytest.mark.parametrize('kind', ['mlp', 'pfm'])
def test_exact_zero_pre_activations_are_off_and_inside_the_bounds(kind):
    for L, F, P in ((33, 65, 0), (64, 100, 5 if kind == 'pfm' else 0)):
        d = with_zero_rows(pair_inputs(kind, L, F, P, n_p=ALL))
        ref = ref_of(kind, d)
        assert not bool(ref.aux['on'][0].any()) and bool(ref.aux['on'][1:].any())        # the pair (0, 0) is p = 0
        got = f32_of(kind, d)
        compare_all(kind + ' zero rows', got, ref)
        for name in OUTPUTS[1:]:
            assert float(ref[name][1][0].abs().max()) == 0.0 and float(got[name][0].abs().max()) == 0.0, name
        d = with_zero_unit(pair_inputs(kind, L, F, P, n_p=ALL), L // 2)
        ref = ref_of(kind, d)
        assert not bool(ref.aux['on'][:, L // 2].any()) and float(ref.aux['a'][:, L // 2].abs().max()) == 0.0
        compare_all(kind + ' zero unit', f32_of(kind, d), ref)


# ---------------------------------------------------------------- the bounds catch wrong formulas
def _outside(kind, d, mutant, names):
    ref = ref_of(kind, d)
    got = f32_of(kind, d, mutant=mutant)
    for name in names:
        with pytest.raises(AssertionError, match='beyond their bound'):
            compare_all('%s %s' % (kind, mutant), got, ref, names=[name])


@pytest.mark.parametrize('kind, L, F, P', [('fm', 1, 1, 0), ('fm', 33, 65, 0), ('fm', 128, 112, 0), ('pfm', 1, 1, 0),
                                           ('pfm', 33, 65, 5), ('pfm', 64, 100, 5)])
def test_mutant_without_the_square_term_falls_outside(kind, L, F, P):
    assert 'drop_x_v2' in MUTANTS
    _outside(kind, pair_inputs(kind, L, F, P, n_p=ALL), 'drop_x_v2', ('g_user', 'g_item', 'w_user', 'w_item'))


@pytest.mark.parametrize('kind, L, F, P', [('mlp', 1, 1, 0), ('mlp', 33, 65, 0), ('mlp', 64, 100, 0), ('pfm', 33, 65, 5)])
def test_mutant_with_a_mask_of_greater_or_equal_falls_outside(kind, L, F, P):
    _outside(kind, with_zero_rows(pair_inputs(kind, L, F, P, n_p=ALL)), 'mask_ge', ('g_user', 'g_item', 'w_user', 'w_item'))
    # (a unit made zero through its own W0 row and bias -- with_zero_unit -- cannot show this mutant: whatever passes
    # its mask is multiplied by that zero row on the way back; only an exact-zero INPUT row can)


@pytest.mark.parametrize('L, F, P', [(31, 64, 0), (33, 65, 5), (64, 100, 5)])
def test_mutant_with_w2_not_transposed_falls_outside(L, F, P):
    _outside('pfm', pair_inputs('pfm', L, F, P, n_p=ALL), 'w2_not_transposed', ('g_user', 'g_item', 'w_user', 'w_item'))


@pytest.mark.parametrize('kind, L, F, P', [('fm', 33, 65, 0), ('mlp', 64, 100, 0), ('pfm', 31, 1, 5)])
def test_mutant_with_the_fc_matrices_swapped_falls_outside(kind, L, F, P):
    d = pair_inputs(kind, L, F, P, n_p=ALL)
    _outside(kind, d, 'fc_swapped', ('w_user', 'w_item'))
    ref = ref_of(kind, d)                                    # ... and only those: the latents' gradients do not read fc
    compare_all('fc swapped', f32_of(kind, d, mutant='fc_swapped'), ref, names=['score', 'g_user', 'g_item'])


# ---------------------------------------------------------------- the entry point's refusals
@pytest.fixture(scope='module')
def lib():
    from reviews4rec_amd import _lib
    _lib.build()
    return _lib.lib()


def call(lib, args):
    from reviews4rec_amd import _lib
    names = _lib.parse_header()['r4r_pair_grad'][2]
    assert list(args) == names, (list(args), names)         # the dict IS the header's argument list
    return lib.r4r_pair_grad(*args.values())


def grad_args(**kw):
    a = dict(kind=PFM, zu=PTR, n_u=3, zi=PTR, n_i=4, u_idx=PTR, i_idx=PTR, n_p=7, q_bias=PTR, c_bias=PTR, W0=PTR, b0=PTR,
             W2=PTR, b2=PTR, w3=PTR, V=PTR, lw=PTR, xu=PTR, xi=PTR, P=5, fc_u=PTR, fc_i=PTR, L=32, F=100, out_score=PTR,
             g_user=PTR, g_item=PTR, w_user=PTR, w_item=PTR, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def test_the_library_exports_the_symbol_and_the_header_cites_the_reference(lib):
    from reviews4rec_amd import _lib
    decls = _lib.parse_header()
    assert 'r4r_pair_grad' in decls and hasattr(lib, 'r4r_pair_grad') and decls['r4r_pair_grad'][0] is ctypes.c_int
    assert decls['r4r_pair_grad'][2] == list(grad_args())
    ints = dict(kind=ctypes.c_int, n_u=ctypes.c_int64, n_i=ctypes.c_int64, n_p=ctypes.c_int64, P=ctypes.c_int,
                L=ctypes.c_int, F=ctypes.c_int)
    for name, t in zip(decls['r4r_pair_grad'][2], decls['r4r_pair_grad'][1]):
        assert t is ints.get(name, ctypes.c_void_p), name
    text = open(_lib.HEADER_PATH).read()
    section = text[text.index(' * Pair gradients:'):]
    for cite in ('DeepCoNN.py:61-66', 'common_pytorch_models.py:49-57', 'common_pytorch_models.py:37', 'DeepCoNN.py:68-72',
                 'TransNet.py:25-35, 105-114', 'TransNet.py:75-76, 108-110', 'Fixed fp32 order'):
        assert cite in section, cite
    for k, v in (('R4R_PAIR_GRAD_FM', FM), ('R4R_PAIR_GRAD_MLP', MLP), ('R4R_PAIR_GRAD_PFM', PFM)):
        assert '#define %s %d' % (k, v) in text


@pytest.mark.parametrize('over, word', [
    (dict(kind=3), b'kind='), (dict(kind=-1), b'kind='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(kind=MLP, P=0, L=65), b'L='), (dict(kind=FM, P=0, L=129), b'L='),
    (dict(kind=FM, P=0, L=-3), b'L='),
    (dict(F=0), b'F='), (dict(F=113), b'F='), (dict(F=-1), b'F='),
    (dict(P=9), b'P='), (dict(P=-1), b'P='), (dict(kind=FM, P=5), b'P='), (dict(kind=MLP, P=1), b'P='),
    (dict(n_u=-1), b'n_u='), (dict(n_i=-1), b'n_i='), (dict(n_p=-1), b'n_p='), (dict(n_p=1 << 31), b'n_p='),
    (dict(kind=FM, P=0, V=None), b'null'), (dict(kind=FM, P=0, lw=None), b'null'),
    (dict(kind=MLP, P=0, W0=None), b'null'), (dict(kind=MLP, P=0, b0=None), b'null'), (dict(kind=MLP, P=0, w3=None), b'null'),
    (dict(W0=None), b'null'), (dict(b0=None), b'null'), (dict(W2=None), b'null'), (dict(b2=None), b'null'),
    (dict(V=None), b'null'), (dict(lw=None), b'null'), (dict(xu=None), b'null'), (dict(xi=None), b'null'),
    (dict(fc_u=None), b'fc_u'), (dict(fc_i=None), b'fc_i'),
    (dict(zu=None), b'null'), (dict(zi=None), b'null'), (dict(u_idx=None), b'null'), (dict(i_idx=None), b'null'),
    (dict(n_u=0), b'n_u='), (dict(n_i=0), b'n_i='),
])
def test_refusals_precede_the_launch_and_name_the_entry_point(lib, over, word):
    got = call(lib, grad_args(**over))
    msg = lib.r4r_last_error() or b''
    assert got == ERR_ARG and msg.startswith(NAME) and word in msg, (over, got, msg)


def test_no_pairs_is_ok_and_enqueues_nothing(lib):
    nul = dict(zu=None, zi=None, u_idx=None, i_idx=None, q_bias=None, c_bias=None, out_score=None, g_user=None, g_item=None,
               w_user=None, w_item=None, fc_u=None, fc_i=None)
    assert call(lib, grad_args(n_p=0)) == OK
    assert call(lib, grad_args(n_p=0, n_u=0, n_i=0, **nul)) == OK
    assert call(lib, grad_args(n_p=0, kind=FM, P=0, L=128, W0=None, b0=None, W2=None, b2=None, w3=None, xu=None, xi=None)) == OK
    assert call(lib, grad_args(n_p=0, P=0, xu=None, xi=None)) == OK               # transnet: no id embeddings, no tables
    # ... but the shape is still checked
    assert call(lib, grad_args(n_p=0, L=65)) == ERR_ARG and (lib.r4r_last_error() or b'').startswith(NAME)
    assert call(lib, grad_args(n_p=0, w_user=PTR, fc_u=None)) == ERR_ARG


# ---------------------------------------------------------------- main's hook
def test_check_explain_pairs_request_refuses_before_any_training():
    from reviews4rec_amd import check_explain_pairs_request as check
    ok = dict(model_type='deepconn', explain_pairs_k=2, explain_pairs_path='p.npz', recommend_k=3, recommend_path='r.npz')
    check(ok)
    check(dict(ok, model_type='deepconn++', catalogue_towers='device'))
    check(dict(model_type='NARRE'))                          # not asked for: nothing to refuse
    check(dict(ok, explain_pairs_k=0, model_type='MF'))
    for mt, word in (('MF_dot', 'no TextCNN tower'), ('MF', 'no TextCNN tower'), ('NeuMF', 'no TextCNN tower'),
                     ('bias_only', 'no TextCNN tower'), ('NARRE', 'no catalogue form'), ('transnet', 'no catalogue form'),
                     ('transnet++', 'no catalogue form')):
        with pytest.raises(RuntimeError, match=r"explain_pairs_k'\]: .*" + word):
            check(dict(ok, model_type=mt))
    for k in (101, -1, 2.0, True, '3'):
        with pytest.raises(RuntimeError, match='must be an int in 1 .. 100'):
            check(dict(ok, explain_pairs_k=k))
    for path in (None, ''):
        with pytest.raises(RuntimeError, match='explain_pairs_path'):
            check(dict(ok, explain_pairs_path=path))
    no_list = dict(ok)
    del no_list['recommend_k']
    with pytest.raises(RuntimeError, match="needs hyper_params\\['recommend_k'\\]"):
        check(no_list)
    with pytest.raises(RuntimeError, match='catalogue_towers'):
        check(dict(ok, catalogue_towers='gpu'))
    with pytest.raises(RuntimeError, match='latent_size 129'):
        check(dict(ok, model_type='deepconn++', latent_size=129))


def test_main_refuses_the_request_before_it_loads_anything():
    from reviews4rec_amd import main as M
    with pytest.raises(RuntimeError, match="explain_pairs_k'\\]: .*no TextCNN tower"):
        M.main(dict(model_type='MF_dot', explain_pairs_k=2, explain_pairs_path='p.npz', recommend_k=3,
                    recommend_path='r.npz', data_dir='/nonexistent'))
