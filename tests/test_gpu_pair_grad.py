"""r4r_pair_grad on the GPU (include/r4r.h, "Pair gradients"; csrc/pair_grad.hip) through ops.pair_grad: every element
of every output within pair_grad_ref's float64 bounds at the shapes where the kernel's lanes, rows and slots change,
the exact-zero edges, and the bits -- the same pair gives the same bits alone, inside a batch, in a permuted batch, in
a split call, repeated within a call and whatever the other outputs are.

Worst error / bound seen on MI355X per kind: see DESIGN 4.24 (every run prints them with -s)."""
import itertools

import pytest
import torch

from head_ref import bits_equal, compare_all
from pair_grad_ref import (FM_LS, FS, HEAD_LS, KINDS, NPS, N_I, N_U, OUTPUTS, PS, pair_inputs, ref_of, with_zero_rows,
                           with_zero_unit)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def run(kind, d, want=OUTPUTS, rows=None):
    """ops.pair_grad over a case's inputs (``rows``: a selection of its pairs) -> dict name -> tensor."""
    from reviews4rec_amd import ops
    dev = lambda t: None if t is None else t.to(DEV)
    sel = slice(None) if rows is None else rows
    return ops.pair_grad(kind, dev(d['zu']), dev(d['zi']), dev(d['u_idx'][sel]), dev(d['i_idx'][sel]),
                         q_bias=dev(d['q_bias']), c_bias=dev(d['c_bias']), fc_u=dev(d['fc_u']), fc_i=dev(d['fc_i']),
                         want=want, **{k: dev(v) for k, v in d['params'].items()})


def same_bits(a, b, what, names=OUTPUTS):
    for name in names:
        assert bits_equal(a[name], b[name]), (what, name)


# ---------------------------------------------------------------- every element within its bound
@pytest.mark.parametrize('kind, L', [(k, L) for k in KINDS for L in (FM_LS if k == 'fm' else HEAD_LS)])
def test_every_output_element_is_within_its_bound(kind, L):
    worst = {}
    for F, P, n_p in itertools.product(FS, PS if kind == 'pfm' else (0,), NPS):
        d = pair_inputs(kind, L, F, P, n_p=n_p)
        got = run(kind, d)
        for name, shape in (('score', (n_p,)), ('g_user', (n_p, L)), ('g_item', (n_p, L)), ('w_user', (n_p, F)),
                            ('w_item', (n_p, F))):
            assert got[name].dtype == torch.float32 and tuple(got[name].shape) == shape and got[name].is_cuda, name
        each = {}
        compare_all('%s L=%d F=%d P=%d n_p=%d' % (kind, L, F, P, n_p), got, ref_of(kind, d), each=each)
        for name, ratio in each.items():
            worst[name] = max(worst.get(name, 0.0), ratio)
    assert 0.0 < max(worst.values()) <= 1.0
    print('%s L=%d: worst error / bound %s' % (kind, L, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------- edge rows
@pytest.mark.parametrize('kind, L, F, P', [('mlp', 33, 65, 0), ('mlp', 64, 100, 0), ('pfm', 33, 65, 0), ('pfm', 64, 100, 5)])
def test_exact_zero_pre_activations_have_their_masks_off(kind, L, F, P):
    d = with_zero_rows(pair_inputs(kind, L, F, P, n_p=N_U * N_I))
    ref = ref_of(kind, d)
    assert not bool(ref.aux['on'][0].any())                  # the pair (0, 0) is p = 0: all-zero latents, zero b0
    got = run(kind, d)
    compare_all(kind + ' zero rows', got, ref)
    for name in OUTPUTS[1:]:                                 # g and w of that pair: exactly 0 (for pfm too: every unit is off)
        assert float(got[name][0].abs().max()) == 0.0, name
    assert float(got['g_user'][1:].abs().max()) > 0.0
    # a unit whose a is an exact 0 for every pair, among live units
    d = with_zero_unit(pair_inputs(kind, L, F, P, n_p=N_U * N_I), L // 2)
    ref = ref_of(kind, d)
    assert float(ref.aux['a'][:, L // 2].abs().max()) == 0.0 and bool(ref.aux['on'].any())
    compare_all(kind + ' zero unit', run(kind, d), ref)


@pytest.mark.parametrize('kind, L, F, P', [('fm', 33, 65, 0), ('mlp', 31, 64, 0), ('pfm', 32, 100, 0), ('pfm', 64, 112, 5)])
def test_null_biases_count_as_zero_and_p_zero_reads_no_embedding(kind, L, F, P):
    d = pair_inputs(kind, L, F, P, n_p=5, biases=False)
    assert d['q_bias'] is None and d['c_bias'] is None and (P > 0) == ('xu' in d['params'])
    got = run(kind, d)
    compare_all(kind + ' no biases', got, ref_of(kind, d))
    one = dict(d, q_bias=None, c_bias=torch.zeros(N_I))
    same_bits(run(kind, one), got, 'c_bias of zeros', names=OUTPUTS[1:])
    with_b = pair_inputs(kind, L, F, P, n_p=5)              # the gradients do not read the biases at all
    same_bits(run(kind, with_b), got, 'biases', names=OUTPUTS[1:])


# ---------------------------------------------------------------- bits
@pytest.mark.parametrize('kind, L, F, P', [('fm', 33, 65, 0), ('fm', 128, 112, 0), ('mlp', 64, 100, 0), ('pfm', 31, 1, 0),
                                           ('pfm', 64, 100, 5)])
def test_a_pair_has_the_same_bits_wherever_it_is_computed(kind, L, F, P):
    n_p = 257
    d = pair_inputs(kind, L, F, P, n_p=n_p)
    full = run(kind, d)
    # permuted
    perm = torch.randperm(n_p, generator=torch.Generator().manual_seed(3))
    shuffled = run(kind, d, rows=perm)
    for name in OUTPUTS:
        assert bits_equal(shuffled[name], full[name][perm.to(DEV)]), ('permuted', name)
    # split at 1 / 64 / 65 pairs
    for cut in (1, 64, 65):
        a, b = run(kind, d, rows=slice(0, cut)), run(kind, d, rows=slice(cut, n_p))
        for name in OUTPUTS:
            assert bits_equal(torch.cat([a[name], b[name]]), full[name]), ('split', cut, name)
    # a pair repeated within one call (the indices past the first twelve repeat them), and alone
    u, i = d['u_idx'], d['i_idx']
    for p in (12, 100, 256):
        first = int(((u == u[p]) & (i == i[p])).nonzero()[0])
        assert first < 12
        alone = run(kind, d, rows=slice(p, p + 1))
        for name in OUTPUTS:
            here = full[name][p:p + 1]
            assert bits_equal(here, full[name][first:first + 1]) and bits_equal(alone[name], here), (p, name)
    # every subset of the outputs (the others NULL)
    few = run(kind, d, rows=slice(0, 70))
    for r in range(1, len(OUTPUTS)):
        for names in itertools.combinations(OUTPUTS, r):
            got = run(kind, d, want=names, rows=slice(0, 70))
            assert set(got) == set(names)
            same_bits(got, few, names, names=names)


def test_the_wrapper_refuses_what_the_kernel_cannot_take():
    from reviews4rec_amd import ops
    d = pair_inputs('mlp', 8, 9, n_p=5)
    with pytest.raises(RuntimeError, match='kind'):
        run('dot', d)
    with pytest.raises(RuntimeError, match='needs V'):
        run('fm', d)
    with pytest.raises(RuntimeError, match='want'):
        run('mlp', d, want=('scores',))
    with pytest.raises(RuntimeError, match='L=65'):
        run('mlp', pair_inputs('mlp', 65, 9, n_p=5))
    with pytest.raises(RuntimeError, match='ROCm device'):
        ops.pair_grad('mlp', d['zu'], d['zi'], d['u_idx'], d['i_idx'], **d['params'])
    none = run('mlp', d, rows=slice(0, 0))
    assert tuple(none['w_user'].shape) == (0, 9) and tuple(none['score'].shape) == (0,)
