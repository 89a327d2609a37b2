"""What the native training steps leave in Adam's moments, against the oracle in float64.

Every native step sums the gradient rows of all ratings that name the same ID row inside its launches (the entry
waves, narre_rows_block, rl_apply_kernel).  The engines' gradient introspection rebuilds those sums in torch, and two
Adam steps hide the size of a gradient from the weights, so the summation shows only in exp_avg / exp_avg_sq: after
step 1, exp_avg = 0.1 (g + wd p) is the gradient as the kernel summed it.  Per engine the smallest shapes that reach
each summation path (tests/step_state_cases.py); every element of every moment, gradient and weight after step 1 and
after step 2 (helpers.assert_step_state; tests/test_step_state_checker.py tests that checker), and a second run from
the same state leaves the same bits.

The text families' cases have twins with dropout on (`-p0.5` / `-p0.3`).  The forward of a dropout site multiplies by
0 or 1 / (1 - p), its backward has to multiply by the same; a backward that multiplies by the 0 / 1 keep pattern
instead puts the factor 1 - p on the gradient of every parameter upstream of the site, which two Adam steps hide from
the weights and the SE and exp_avg shows.  Each twin's device masks equal the Philox stand-in the CPU checker ran on
(tests/test_step_state_checker.py), element for element, and are injected into the float64 reference.

DeepCoNN's dense gradients are sums over the ratings, dealt to splits, rounds and passes by the batch size: its
batch-axis cases (deepconn_batch_cases: 1 to 1,000 ratings) hold the step to the same reference on either side of every
batch size at which that dealing or the tail of the step changes, with the four-launch and the five-launch tail.

Every rating's SE is compared on its own (rtol 1e-4, atol 1e-5), on every case.

No absolute tolerance is widened: every tensor is held to rtol 1e-4, atol 1e-7 (exp_avg_sq: 1e-10)."""
import os

import pytest
import torch

from helpers import (StateStandIn, assert_per_rating_se, assert_step_state, float64_step_reference, multipliers,
                     state_distances)
from step_state_cases import (deepconn_batch_cases, deepconn_cases, deepconnpp_cases, idnet_cases, mf_cases, narre_cases,
                              stream_keep, transnet_cases)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def build(case):
    import reviews4rec_amd
    from reviews4rec_amd import main as M
    P0 = case.params()
    hp = dict(case.hp)
    assert M.native_step_limits(hp) is None
    key = 'target.word2vec.weight' if hp['model_type'].startswith('transnet') else 'word2vec.weight'
    if key in P0:
        hp['word_vectors'] = P0[key].numpy()
    model = reviews4rec_amd.get_model_class(hp['model_type'])(hp)
    model.load_state_dict(P0)
    model = model.to(DEV).train()
    eng = M.make_engine(dict(case.hp, engine='native', log_file=None), model)
    assert type(eng).__name__ == case.engine
    return P0, model, eng


def worst(d):
    return ', '.join('%s %.3g (%s)' % ((kind,) + max((v, k) for k, v in per.items())) for kind, per in d.items() if per)


def run(case, check):
    """Two steps of the case's engine; with `check` each against the float64 step from the same weights.  Returns the
    bits it left after each step: per-example SE, weights, moments."""
    P0, model, eng = build(case)
    ref = float64_step_reference(P0, case.hp)
    o32 = float64_step_reference(P0, case.hp, dtype=torch.float32)
    bits, before = [], None
    for step, (data, y) in enumerate(case.batches()):
        dev = [None if d is None else d.to(DEV) for d in data]
        se = eng.train_step(dev, y.to(DEV)).cpu().clone()
        masks = None
        if case.draws:
            mult = multipliers(eng, dev).cpu().reshape(y.numel(), case.draws)
            if case.stream:                                  # the CPU pre-check saw these very masks
                off = torch.nonzero((mult != 0) != stream_keep(case, step))
                assert off.numel() == 0, ('%s step %d: %d draws differ from the Philox stand-in, first at %s'
                                          % (case.id, step + 1, off.shape[0], off[0].tolist()))
            masks = case.sites(mult)
        m, v = eng.moments()
        sd = {k: t.detach().cpu().clone() for k, t in model.state_dict().items()}
        bits.append((se, sd, {k: t.cpu().clone() for k, t in m.items()}, {k: t.cpu().clone() for k, t in v.items()}))
        if check:
            r = ref.step(data, y, masks, start=before)
            r32 = o32.step(data, y, masks, start=before)
            print('STEP-STATE %s %s step %d | engine: %s | float32 oracle: %s'
                  % (case.engine, case.id, r.step, worst(state_distances(eng, r, dev)),
                     worst(state_distances(StateStandIn(r32), r))))
            torch.testing.assert_close(se.double().sum(), torch.tensor(r.sse, dtype=torch.float64), rtol=1e-4, atol=1e-3)
            assert_per_rating_se(se, r, what=case.id)
            assert_step_state(eng, model, r, data=dev, weights=case.weights, what=case.id)
        before = sd
    return bits


def same_bits(first, again, between='two runs'):
    assert len(first) == len(again)
    for step, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a[0], b[0]), 'per-example SE of step %d differs between %s' % (step + 1, between)
        for what, x, z in (('weight', a[1], b[1]), ('exp_avg', a[2], b[2]), ('exp_avg_sq', a[3], b[3])):
            assert set(x) == set(z)
            for k in x:
                assert torch.equal(x[k], z[k]), '%s %s of step %d differs between %s' % (what, k, step + 1, between)


def check_case(case):
    first = run(case, check=True)
    same_bits(first, run(case, check=False))
    return first


@pytest.mark.parametrize('case', mf_cases(), ids=repr)
def test_mf_step_state(case):
    """r4r_mf_step: D 4 / 10 (generic entry waves), 64 (wide), 100, 256; B = 1,000 (inside the 2,048-rating scan), 2,100
    (just past it), 16,384; bias_only; one case with dropout 0.5, the device's multipliers injected."""
    check_case(case)


@pytest.mark.parametrize('case', idnet_cases(), ids=repr)
def test_idnet_step_state(case):
    """r4r_idnet_step: MF, GMF, NeuMF, MLP; the last row of each table named."""
    check_case(case)


@pytest.mark.parametrize('case', narre_cases(), ids=repr)
def test_narre_step_state(case):
    """r4r_narre_step's fused ID role with rows that hundreds of entries hit, its <= 32 instantiation, the split form
    (L or R beyond 32 -> r4r_narre_rows_apply_large), B = 372 / 373 on either side of the fused 4,096-entry limit,
    B = 512 (the stand-alone rows-apply launch) and B = 2,048 (22,528 entries -> r4r_narre_rows_apply_large).
    The twins draw at all seven sites (the towers' outputs, the two scorers' hidden layers, the two ID rows, the
    product): the fused form, both instantiations, the split form and the first split batch size, at p 0.5 / 0.3."""
    check_case(case)


@pytest.mark.parametrize('case', deepconnpp_cases(), ids=repr)
def test_deepconnpp_step_state(case):
    """r4r_deepconnpp_step at L 16 / 17 / 32 / 33 / 64, and B = 300 with users drawn from 12 ids, items from 8.
    Every case has a twin that draws at its three sites (the towers' outputs and the head's hidden layer)."""
    check_case(case)


@pytest.mark.parametrize('case', transnet_cases(), ids=repr)
def test_transnet_step_state(case):
    """r4r_transnet_step, `transnet` and `transnet++`, L 24 / 48 / 64: the moments of its three optimisers' groups;
    transnet++ also at B = 300 with users drawn from 12 ids.  Every case has a twin that draws at its five (transnet)
    or seven (transnet++: the two ID rows) sites; a scale lost at a source site shows in the `source` group's moments,
    at a target site in the `target` group's."""
    check_case(case)


@pytest.mark.parametrize('case', deepconn_cases(), ids=repr)
def test_deepconn_step_state(case):
    """r4r_deepconn_step at L 16 / 17 / 64 / 65 / 128 (the 65 .. 128 head instantiation keeps the old tail).  Every
    case has a twin that draws at the two towers' outputs."""
    check_case(case)


def expect_fold(B, E, L):
    nsplit = min(16, -(-B // 16))
    return int(B <= 256 and -(-B // nsplit) <= 16 and nsplit * (E // 4) <= 1024 and L <= 64)


@pytest.mark.parametrize('case', deepconn_batch_cases(), ids=repr)
def test_deepconn_batch_step_state(case):
    """r4r_deepconn_step along its batch axis, B = 1 .. 1,000: one to sixteen splits, a last split of one document,
    head_grad_block's passes on either side of 128 ratings, the four-launch tail up to its limits (256 documents,
    1,024 threads, L = 64) and the five-launch tail just past each of them and at several rounds per split.  Equal
    numbers cannot tell the tails apart, so the tail the shape resolves to is asked for (r4r_deepconn_tail) and held to
    the rule worked out here; every shape the four-launch tail takes is run with the five-launch tail too: each is
    held to float64 on its own, and the two leave the same bits."""
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    hp = case.hp
    B, E, L = int(hp['batch_size']), int(hp['word_embed_size']), int(hp['latent_size'])
    folds = lib.r4r_deepconn_tail(B, E, L)
    if not any(k in os.environ for k in ('R4R_TAIL', 'R4R_WGRAD_DOCS', 'R4R_WGRAD_MAX_SPLITS')):
        assert folds == expect_fold(B, E, L)
    print('STEP-STATE %s %s takes the %s-launch tail' % (case.engine, case.id, 'four' if folds else 'five'))
    first = check_case(case)
    if not folds:
        return
    before = lib.r4r_deepconn_tail_fold(0)
    try:
        assert lib.r4r_deepconn_tail(B, E, L) == 0
        print('STEP-STATE %s %s again, the five-launch tail forced' % (case.engine, case.id))
        same_bits(first, run(case, check=True), 'the four-launch and the five-launch tail')
    finally:
        lib.r4r_deepconn_tail_fold(before)
