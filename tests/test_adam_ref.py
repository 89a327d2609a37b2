"""The Adam reference and its bounds (tests/adam_ref.py) tested on their own, without a GPU.

On the inputs of every case of tests/test_gpu_adam_steps.py:
  - the float32 emulation of each written form (uncontracted and with the two contractions a compiler may make) stays
    inside that form's bound on every element -- the bounds are attainable, and the worst fraction is printed;
  - each mutation of MUTATIONS -- the ways a kernel could be subtly wrong -- is rejected on at least one case;
  - the reference agrees with oracle.adam_step within the IEEE bound;
  - the step counts at which two correct double pows may round a scalar differently are (almost) none."""
import numpy as np
import pytest
import torch

import adam_ref as ar
import oracle


def run_forms(what, p, g, m, v, t, hp, forms=(False, True)):
    worst = {}
    for fast in forms:
        ref = ar.adam_ref(p, g, m, v, t, fast=fast, **hp)
        for contract in (False, True):
            got = ar.emulate(p, g, m, v, t, fast=fast, contract=contract, **hp)
            frac = ar.check('%s %s%s' % (what, 'fast' if fast else 'ieee', ' contracted' if contract else ''), got, ref)
            for k, x in frac.items():
                worst[k] = max(worst.get(k, 0.0), x)
    return worst


def test_the_state_holds_every_regime_and_ends_on_ordinary_elements():
    p, g, m, v = ar.adam_state(ar.STATE_N, 0)
    r = np.arange(ar.STATE_N) % ar.REGIMES
    assert all(x.dtype == np.float32 and x.shape == (ar.STATE_N,) for x in (p, g, m, v))
    assert bool((v >= 0).all()) and bool(np.isfinite(np.stack([p, g, m, v])).all())
    body = np.arange(ar.STATE_N) < ar.STATE_N - 3
    assert bool((g[(r == 8) & body] == 0).all()) and bool((v[(r == 8) & body] > 0).all())
    assert not m[(r == 9) & body].any() and not v[(r == 9) & body].any() and bool((g[(r == 9) & body] != 0).all())
    sel = (r == 11) & body
    assert bool(((v[sel] > 0) & (v[sel] < ar.TINY)).all()) and not p[sel].any()
    assert not p[(r == 12) & body].any()
    assert float(np.abs(g[r == 13]).max()) > 1e17 and float(np.abs(g[(r == 14) & body]).min()) < 1e-19
    assert bool((np.abs(g[-3:]) > 0).all()) and bool((p[-3:] != 0).all()) and bool((v[-3:] > 0).all())
    sq = np.sqrt(v[(r == 15) & body].astype(np.float64))
    assert 1e-9 < float(np.median(sq)) < 1e-6                 # comparable to eps = 1e-8


@pytest.mark.parametrize('case', ar.STEP_CASES + [ar.PLACEMENT_CASE], ids=ar.case_id)
def test_emulation_of_both_forms_is_inside_the_bound(case):
    p, g, m, v = ar.case_inputs(case)
    worst = run_forms(case['name'], p, g, m, v, case['t'], case['hp'])
    msg = '%s: worst error / bound %s' % (case['name'], ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    print(msg)
    assert max(worst.values()) <= 1.0, msg


@pytest.mark.parametrize('numel', ar.GATHERED_NUMELS)
@pytest.mark.parametrize('world', ar.GATHERED_WORLDS)
def test_emulation_of_the_gathered_form_is_inside_the_bound(world, numel):
    worst = 0.0
    for t in ar.GATHERED_STEPS:
        p, gathered, m, v = ar.gathered_inputs(world, numel, t)
        g = ar.sequential_sum(gathered)
        if world == 1:
            assert ar.bits_equal(g, gathered[0])
        elif world >= 3 and numel >= 1020:
            assert not ar.bits_equal(g, ar.sequential_sum(gathered[::-1]))     # the order shows: the bits pin it
        w = run_forms('gathered world %d numel %d t %d' % (world, numel, t), p, g, m, v, t, ar.DEFAULTS, forms=(False,))
        worst = max([worst] + list(w.values()))
    assert worst <= 1.0, 'worst error / bound %.3f' % worst


@pytest.mark.parametrize('W', ar.ROWS_WIDTHS)
def test_emulation_of_the_row_update_is_inside_the_fast_bound(W):
    worst = 0.0
    for t in ar.ROWS_STEPS:
        d = ar.rows_inputs(W, t)
        named = d['named']
        assert named.size == ar.ROWS_NAMED == np.unique(d['ids'][d['ids'] >= 0]).size
        assert int((d['ids'] < 0).sum()) == ar.ROWS_PAD
        for p, g, m, v in ((d['p'], d['g_rows'], d['m'], d['v']), (d['bp'], d['g_bias'], d['bm'], d['bv'])):
            w = run_forms('rows W %d t %d' % (W, t), p[named], g[named], m[named], v[named], t, ar.DEFAULTS, forms=(True,))
            worst = max([worst] + list(w.values()))
    assert worst <= 1.0, 'worst error / bound %.3f' % worst


def test_emulation_of_the_class_trajectory_is_inside_the_bound_at_every_step():
    worst, steps = 0.0, {}
    state = {i: (ar.class_param(i, n), np.zeros(n, np.float32), np.zeros(n, np.float32))
             for i, n in enumerate(ar.CLASS_SIZES)}
    for step in range(ar.CLASS_STEPS):
        for i, n in enumerate(ar.CLASS_SIZES):
            if not ar.class_has_grad(i, step):
                continue
            steps[i] = steps.get(i, 0) + 1
            p, m, v = state[i]
            g = ar.class_grad(i, step, n)
            w = run_forms('class %d step %d' % (i, step), p, g, m, v, steps[i], ar.DEFAULTS, forms=(False,))
            worst = max([worst] + list(w.values()))
            out = ar.emulate(p, g, m, v, steps[i], **ar.DEFAULTS)
            state[i] = (out['p'], out['m'], out['v'])
    assert sorted(set(steps.values())) == [7, 10, 12] and len(steps) == 40
    assert worst <= 1.0, 'worst error / bound %.3f' % worst


@pytest.mark.parametrize('fast', [False, True], ids=['ieee', 'fast'])
@pytest.mark.parametrize('mutation', ar.MUTATIONS)
def test_the_bounds_reject_a_wrong_kernel(mutation, fast):
    """Each mutation must fall outside the bound on at least one listed case (and the unmutated emulation inside, on the
    same case, so that it is the mutation that is rejected)."""
    rejected = []
    for case in ar.STEP_CASES:
        p, g, m, v = ar.case_inputs(case)
        ref = ar.adam_ref(p, g, m, v, case['t'], fast=fast, **case['hp'])
        ar.check(case['name'], ar.emulate(p, g, m, v, case['t'], fast=fast, **case['hp']), ref)
        try:
            ar.check(case['name'], ar.emulate(p, g, m, v, case['t'], fast=fast, mutate=mutation, **case['hp']), ref)
        except AssertionError as e:
            assert 'beyond their bound' in str(e)
            rejected.append(case['name'])
    print('%s rejected on %d of %d cases: %s' % (mutation, len(rejected), len(ar.STEP_CASES), ' '.join(rejected)))
    assert rejected, '%s passes every case' % mutation
    if mutation == 'drop_wd_null':
        assert all(name.startswith('gnull') for name in rejected)
    if mutation in ('beta2_for_m', 'eps_in_sqrt', 'tail_unwritten'):
        assert len(rejected) == len(ar.STEP_CASES)            # wrong at every step count and setting


def test_a_mutation_that_changes_nothing_is_not_rejected():
    """t - 1 for t beyond both corrections' fade and float32 pow at t = 1 give the same two scalars: the bounds answer
    what was computed, not how."""
    case = [c for c in ar.STEP_CASES if c['name'] == 't%d' % (2 ** 31 + 1)][0]
    p, g, m, v = ar.case_inputs(case)
    ref = ar.adam_ref(p, g, m, v, case['t'], **case['hp'])
    ar.check('t - 1', ar.emulate(p, g, m, v, case['t'], mutate='t_minus_1', **case['hp']), ref)


@pytest.mark.parametrize('t', [1, 2, 3, 1000])
def test_reference_agrees_with_the_oracle(t):
    case = ar.STEP_CASES[0]
    p, g, m, v = ar.case_inputs(case)
    hp = case['hp']
    ref = ar.adam_ref(p, g, m, v, t, **hp)
    params = {'x': torch.from_numpy(p.copy())}
    state = oracle.AdamState()
    state.m['x'], state.v['x'], state.t['x'] = torch.from_numpy(m.copy()), torch.from_numpy(v.copy()), t - 1
    oracle.adam_step(params, {'x': torch.from_numpy(g.copy())}, state, hp['lr'], hp['wd'],
                     betas=(hp['beta1'], hp['beta2']), eps=hp['eps'])
    frac = ar.check('oracle t %d' % t, dict(p=params['x'], m=state.m['x'], v=state.v['x']), ref)
    print('oracle.adam_step t=%d: worst error / IEEE bound %s' % (t, frac))


def test_reference_scalars():
    lrb, isb = ar.ref_scalars(1, 0.002, 0.9, 0.999)
    assert abs(lrb / (ar.f32(0.002) / 0.1) - 1) < 1e-15 and abs(isb / (1 / np.sqrt(0.001)) - 1) < 1e-13
    for t in (7100, 745000, 10 ** 7, 2 ** 31 + 1):            # beta1^t underflows in double near 7,100, beta2^t near 745,000
        lrb, isb = ar.ref_scalars(t, 0.002, 0.9, 0.999)
        assert lrb == ar.f32(0.002) and (isb == 1.0) == (t >= 745000)
    assert 0.9 ** 7100 == 0.0 and 0.9 ** 7000 > 0.0 and 0.999 ** 745000 == 0.0 and 0.999 ** 740000 > 0.0
    for t in ar.STEP_COUNTS:                                   # the host's double pow agrees with expm1 to a float32 ulp
        for b1, b2 in ar.BETA_PAIRS:
            ref = ar.ref_scalars(t, 0.002, b1, b2)
            host = ar.host_scalars(t, 0.002, b1, b2)
            for x, h in zip(ref, host):
                assert abs(float(h) - x) <= ar.U32 * x * (1 + 1e-6), (t, b1, b2, x, h)


@pytest.mark.parametrize('betas', ar.BETA_PAIRS, ids=str)
def test_few_step_counts_sit_on_a_rounding_boundary(betas):
    """The condition under which tests/test_gpu_adam_steps.py may leave a t out of its host-step / step_dev bit
    comparison holds for at most 1 % of t = 1 .. 2,048."""
    out = [t for t in range(1, ar.CONSEC_STEPS + 1) if ar.fragile(t, 0.002, *betas)]
    print('betas %s: left out %s' % (betas, out))
    assert len(out) <= ar.CONSEC_STEPS // 100


def test_the_list_layouts_are_the_ones_meant():
    assert len(ar.LIST_LAYOUTS) == 14
    for pos, n in ar.LIST_LAYOUTS:
        numel, g_null = ar.list_layout(pos, n)
        assert len(numel) == n and numel[pos - 1] == ar.STATE_N and not g_null[pos - 1]
        assert set(numel) - {ar.STATE_N} <= set(ar.NEIGHBOUR_NUMELS)
        for k in (0, n // 2, n - 1):
            assert numel[k] == 0 or k == pos - 1
    numel, g_null = ar.list_layout(17, 33)
    assert set(numel) == set(ar.NEIGHBOUR_NUMELS) | {ar.STATE_N} and any(g_null)
    assert sum(ar.BIG_LIST) >= ar.FOUR_MI and sum(ar.UNDER_LIST) == ar.FOUR_MI - 1
