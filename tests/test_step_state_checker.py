"""The step-state checker (helpers.assert_step_state) tested on its own, without a GPU: the float32 oracle stands in for
an engine.  On the inputs of every case of tests/test_gpu_step_state.py the oracle as it is must pass -- the reference
alone stays inside the tolerance -- and every seeded mistake in the summation of duplicate rows must raise, from the
Adam moments alone.  The weights-only criteria the edge-shape tests used so far pass the first two mistakes: two Adam
steps hide a positive factor on a gradient (step 1 is lr g / (|g| + eps), step 2 is homogeneous of degree 0), which is
why the moments are compared at all.

The same holds for dropout: the text families' dropout-on cases run on the masks the device will draw (the Philox
stream, step_state_cases.stream_multipliers), and a dropout site whose backward loses the factor 1 / (1 - p), or hands
dropped elements a gradient, must raise at every site -- while the weights-only criteria pass the lost factor."""
import pytest
import torch

import oracle
from helpers import (StateStandIn, assert_per_rating_se, assert_step_state, float64_step_reference, ill_conditioned,
                     is_row_tensor, oracle_atol, state_distances, weights_failures, weights_outliers)
from step_state_cases import all_cases, stand_in_multipliers

CASES = all_cases()
BY_ID = {c.id: c for c in CASES}


def masks_of(case, step):
    if not case.draws:
        return None
    return case.sites(stand_in_multipliers(case, step))


_UNSEEDED = {}


def run(case, mistake=None, at_site=None):
    """The two steps of a case by the float32 oracle, each next to the float64 step from the same weights: a list of
    (float32 StepState, float64 StepState).  mistake(step, data, y, masks, grads, params) edits the gradients the float32
    oracle's Adam sees; at_site(masks) edits the dropout multipliers the float32 oracle sees (the float64 step keeps
    the true ones).  The unseeded run of a case is computed once and shared; nothing changes it."""
    if mistake is None and at_site is None and case.id in _UNSEEDED:
        return _UNSEEDED[case.id]
    o32 = float64_step_reference(case.params(), case.hp, dtype=torch.float32)
    ref = float64_step_reference(case.params(), case.hp)
    out, before = [], None
    for step, (data, y) in enumerate(case.batches()):
        masks = masks_of(case, step)
        perturb = None
        if mistake is not None:
            perturb = lambda grads, params, a=(step, data, y, masks): mistake(*a, grads, params)   # noqa: E731
        s32 = o32.step(data, y, masks if at_site is None else at_site(masks), perturb=perturb)
        out.append((s32, ref.step(data, y, masks, start=before)))
        before = s32.params
    if mistake is None and at_site is None:
        _UNSEEDED[case.id] = out
    return out


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_the_float32_oracle_stays_inside_the_tolerance_on_every_case(case):
    """Gradients, exp_avg, exp_avg_sq and weights of the float32 oracle against float64 after step 1 and step 2, element
    by element, at the tolerances the engines are held to (no widened atol)."""
    steps = run(case)
    for s32, s64 in steps:
        assert_step_state(StateStandIn(s32), StateStandIn(s32), s64, data=None, weights=case.weights, what=case.id)
        d = state_distances(StateStandIn(s32), s64)
        print('%s step %d float32 oracle vs float64: ' % (case.id, s64.step)
              + ', '.join('%s %.3g' % (kind, max(v.values())) for kind, v in d.items() if v))
    if case.table is not None:                               # the case has what the seeded mistakes need
        zero = steps[-1][1].zero_so_far[case.table[0]]
        assert bool((zero.all(dim=-1) if zero.dim() > 1 else zero).any()), 'no row without a gradient'


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_the_float32_oracle_s_per_rating_se_stays_inside_the_tolerance_on_every_case(case):
    """Each rating's squared error of the float32 oracle against float64, on both steps, at the tolerance
    tests/test_gpu_step_state.py holds the engines to (rtol 1e-4, atol 1e-5)."""
    for s32, s64 in run(case):
        assert s32.se.numel() == s64.se.numel() == case.batches()[s64.step - 1][1].numel()
        assert_per_rating_se(s32.se, s64, what=case.id)


@pytest.mark.parametrize('case', [c for c in CASES if c.stream], ids=repr)
def test_a_dropout_case_draws_at_every_site_on_both_steps(case):
    """The stand-in masks of a dropout-on case: every site named by the oracle's forward, each with dropped and kept
    elements, kept ones at 1 / (1 - p); the two steps draw different masks (step 2 starts where step 1 stopped)."""
    p = float(case.hp['dropout'])
    both = [masks_of(case, step) for step in range(2)]
    for masks in both:
        assert len(masks) == SITES[case.hp['model_type']]
        for site, m in masks.items():
            kept = m[m != 0]
            assert 0 < kept.numel() < m.numel(), site
            assert bool((kept == kept[0]).all()) and abs(float(kept[0]) - 1 / (1 - p)) < 1e-6, site
    assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(both[0].values(), both[1].values()))


# ------------------------------------------------------------------------------------------------ seeded mistakes
def counts(case, step):
    """How often each row of the case's table is named by the batch of `step`."""
    name, slots = case.table
    data = case.batches()[step][0]
    n = case.params()[name].shape[0]
    return sum(torch.bincount(data[s].reshape(-1), minlength=n) for s in slots)


def without_one_hit(case, data, y, masks, params, row, last):
    """The gradients of one step with one hit of `row` of the case's table left out of the duplicate summation: the hit
    (the first, or the last, in the last slot that names the table: for NARRE a rating's own row) reads a copy of the row appended to the table, so the
    forward pass is unchanged and that hit's gradient row lands in the copy, which is then dropped."""
    name, slots = case.table
    slot = [s for s in slots if bool((data[s] == row).any())][-1]
    at = torch.nonzero(data[slot].reshape(-1) == row).reshape(-1)
    at = int(at[-1] if last else at[0])
    side = 'user' if 'user' in name else 'item'
    extended = [name] if slot in (1, 2) else [k for k in params if is_row_tensor(k) and side in k]
    leaves = {}
    for k in oracle.trainable_names(params):
        t = params[k].detach().clone()
        if k in extended:
            t = torch.cat([t, t[row:row + 1]], 0)
        leaves[k] = t.requires_grad_(True)
    moved = [d if d is None else d.clone() for d in data]
    flat = moved[slot].reshape(-1)
    flat[at] = params[name].shape[0]
    moved[slot] = flat.reshape(data[slot].shape)
    full = dict(params)
    full.update(leaves)
    out = oracle.model_forward(full, moved, case.hp, train=True, masks=masks)
    oracle.mse_loss(out, y.to(out.dtype), return_mean=False).mean().backward()
    return {k: leaves[k].grad[:params[k].shape[0]] for k in extended}


def doubled(case):
    def mistake(step, data, y, masks, grads, params):
        name = case.table[0]
        if name in grads:                                    # (TransNet: the optimiser that steps the table)
            g = grads[name].clone()
            g[int(counts(case, step).argmax())] *= 2
            grads[name] = g
    return mistake


def hot_hit_dropped_on_step_2(case):
    def mistake(step, data, y, masks, grads, params):
        if step == 1:
            grads.update(without_one_hit(case, data, y, masks, params, int(counts(case, step).argmax()), last=False))
    return mistake


def last_of_two_hits_dropped(case):
    def mistake(step, data, y, masks, grads, params):
        n = counts(case, step)
        fewest = int(n[n >= 2].min())                        # 2 wherever the batch names a row twice (the ID-only cases do)
        grads.update(without_one_hit(case, data, y, masks, params, int(torch.nonzero(n == fewest)[0]), last=True))
    return mistake


def dense_halved(case):
    def mistake(step, data, y, masks, grads, params):
        name = [k for k, g in grads.items() if g is not None and not is_row_tensor(k) and not ill_conditioned(k)][0]
        grads[name] = grads[name] * 0.5
    return mistake


def untouched_row_given_a_gradient(case):
    def mistake(step, data, y, masks, grads, params):
        name = case.table[0]
        if step == 0 and name in grads:
            never = torch.nonzero((counts(case, 0) + counts(case, 1)) == 0).reshape(-1)
            g = grads[name].clone()
            g[int(never[0])] = 1e-3
            grads[name] = g
    return mistake


# ------------------------------------------------------------------------------------------------ dropout sites
SITES = {'deepconn': 2, 'deepconn++': 3, 'NARRE': 7, 'transnet': 5, 'transnet++': 7}


class SiteMistake:
    """In place of a site's multipliers: the forward is x * mult to the bit, the gradient flows through x * through."""

    def __init__(self, mult, through):
        self.mult, self.through = mult, through

    def to(self, dtype):
        return SiteMistake(self.mult.to(dtype), self.through.to(dtype))

    def __rmul__(self, x):
        back = x * self.through
        return (x * self.mult).detach() + (back - back.detach())


def scale_lost_in_backward(site):
    """The backward of `site` multiplies by the 0 / 1 keep pattern where the forward multiplied by 0 or 1 / (1 - p)."""
    def at_site(masks):
        return dict(masks, **{site: SiteMistake(masks[site], (masks[site] != 0).to(masks[site].dtype))})
    return at_site


def dropped_elements_keep_their_gradient(site):
    """The backward of `site` multiplies every element by 1 / (1 - p), the dropped ones too."""
    def at_site(masks):
        return dict(masks, **{site: SiteMistake(masks[site], torch.full_like(masks[site], float(masks[site].max())))})
    return at_site


def caught_at_site(case, at_site):
    """caught(), for a mistake seeded through the masks."""
    steps = run(case, at_site=at_site)
    raised = []
    for s32, s64 in steps:
        try:
            assert_step_state(StateStandIn(s32, with_grads=False), StateStandIn(s32), s64, what=case.id)
            raised.append(False)
        except AssertionError:
            raised.append(True)
    return raised, steps


# one dropout-on case per family, every site of it
SITE_CASES = ['deepconn-L17-p0.5', 'deepconnpp-L33-B12-p0.5', 'narre-L24-R20-p0.5', 'transnet-L48-B12-p0.5',
              'transnet++-L64-B12-p0.5']
EVERY_SITE = [(id, site) for id in SITE_CASES for site in masks_of(BY_ID[id], 0)]
assert [sum(1 for i, _ in EVERY_SITE if i == id) for id in SITE_CASES] == [2, 3, 7, 5, 7]


@pytest.mark.parametrize('mistake', [scale_lost_in_backward, dropped_elements_keep_their_gradient],
                         ids=lambda f: f.__name__)
@pytest.mark.parametrize('case,site', EVERY_SITE)
def test_a_seeded_mistake_at_a_dropout_site_raises(case, site, mistake):
    """At every dropout site of one case per text family, from the moments alone, on step 1 and on step 2.  The seeded
    forward is the true one to the bit: the SE does not move."""
    case = BY_ID[case]
    raised, steps = caught_at_site(case, mistake(site))
    assert raised == [True, True]
    assert torch.equal(steps[0][0].se, run(case)[0][0].se)


@pytest.mark.parametrize('case,site', [
    ('deepconn-L17-p0.5', 'user_conv.dropout'), ('deepconnpp-L33-B12-p0.5', 'final.2'),
    ('deepconnpp-L33-B12-p0.5', 'user_conv.dropout'), ('transnet-L48-B12-p0.5', 'source.dropout'),
    ('transnet-L48-B12-p0.5', 'target.dropout'), ('transnet-L48-B12-p0.5', 'target.conv.dropout'),
    ('transnet++-L64-B12-p0.5', 'dropout.user')])
def test_the_weights_only_criteria_pass_a_scale_lost_in_the_backward_of_a_dropout_site(case, site):
    """Why the dropout-on cases exist: with the factor 1 / (1 - p) lost in the backward of one site -- the gradient of
    every parameter upstream of it halved -- the weights after each of two Adam steps stay inside the case's own
    weights criterion and every rating's SE inside its tolerance, which is all the dropout-on engine tests compared;
    the moments raise on both steps."""
    case = BY_ID[case]
    raised, steps = caught_at_site(case, scale_lost_in_backward(site))
    assert raised == [True, True]
    for s32, s64 in steps:
        assert weights_failures(s32.params, s64.params, case.weights) == []
        assert_per_rating_se(s32.se, s64, what=case.id)


# one case per engine that sums ID rows (TransNet++, whose oracle step is its own, below)
SEEDED = ['mf_dot-D10-B2100', 'idnet-GMF-L5-B2100', 'narre-fused-B96', 'deepconnpp-L16-B300']
MISTAKES = [doubled, hot_hit_dropped_on_step_2, last_of_two_hits_dropped, dense_halved, untouched_row_given_a_gradient]


def caught(case, mistake):
    """The checker's verdict on the float32 oracle with a mistake seeded, from the Adam moments alone (the stand-in
    reports no gradients), step by step; and the states, for the weights-only criteria."""
    steps = run(case, mistake(case))
    raised = []
    for s32, s64 in steps:
        try:
            assert_step_state(StateStandIn(s32, with_grads=False), StateStandIn(s32), s64, what=case.id)
            raised.append(False)
        except AssertionError:
            raised.append(True)
    return raised, steps


@pytest.mark.parametrize('mistake', MISTAKES, ids=lambda f: f.__name__)
@pytest.mark.parametrize('case', SEEDED)
def test_a_seeded_mistake_in_the_row_sums_raises(case, mistake):
    case = BY_ID[case]
    raised, _ = caught(case, mistake)
    if mistake is hot_hit_dropped_on_step_2:
        assert raised == [False, True]                       # step 1 is untouched: the checker must not cry wolf there
    else:
        assert raised[0] and raised[1]                       # (step 2 too: exp_avg remembers)


@pytest.mark.parametrize('mistake', [doubled, dense_halved, untouched_row_given_a_gradient], ids=lambda f: f.__name__)
def test_a_seeded_mistake_in_transnetpp_s_three_optimisers_raises(mistake):
    raised, _ = caught(BY_ID['transnet++-L24-B300'], mistake)
    assert raised[0] and raised[1]


@pytest.mark.parametrize('case,mistake', [
    ('mf_dot-D10-B2100', doubled), ('mf_dot-D10-B2100', hot_hit_dropped_on_step_2), ('idnet-GMF-L5-B2100', doubled),
    ('idnet-GMF-L5-B2100', hot_hit_dropped_on_step_2), ('narre-fused-B96', doubled)],   # (NARRE's popular user is rated 8
    ids=lambda v: v if isinstance(v, str) else v.__name__)   # times: one of those hits is an eighth of the row, no rounding)
def test_the_weights_only_criteria_pass_the_first_two_mistakes(case, mistake):
    """Why this file exists: the popular row's gradient doubled on both steps, or one of its hits lost on step 2, leaves
    the weights after two Adam steps inside the criteria of the tests named after popular rows: the doubled row inside
    each engine's own, MF_dot's rtol 1e-5 / atol 5e-6 included; the lost hit inside every fraction + max criterion (of
    MF_dot's 30,010 item elements, five leave the rtol / atol one)."""
    case = BY_ID[case]
    raised, steps = caught(case, mistake)
    assert raised[1]
    old = case.weights if (mistake is doubled or 'frac' in case.weights) else weights_outliers()
    for s32, s64 in steps:
        assert weights_failures(s32.params, s64.params, old) == []


# ------------------------------------------------------------------------------------------------ dense sums over B
def one_rating_s_gradient(case, data, y, masks, params, n):
    """The gradients of rating n's term of the loss, (pred_n - y_n)^2 / B, by the float32 oracle's autograd on that
    rating alone."""
    leaves = {k: params[k].detach().clone().requires_grad_(True) for k in oracle.trainable_names(params)}
    full = dict(params)
    full.update(leaves)
    one = [d if d is None else d[n:n + 1] for d in data]
    if masks is not None:
        masks = {site: m[n:n + 1] for site, m in masks.items()}
    out = oracle.model_forward(full, one, case.hp, train=True, masks=masks)
    (oracle.mse_loss(out, y[n:n + 1].to(out.dtype), return_mean=False).sum() / y.numel()).backward()
    return {k: t.grad for k, t in leaves.items()}


def one_rating_missing_from_a_dense_sum(case, name, n):
    def mistake(step, data, y, masks, grads, params):
        grads[name] = grads[name] - one_rating_s_gradient(case, data, y, masks, params, n)[name]
    return mistake


def one_rating_counted_twice(case, name, n):
    def mistake(step, data, y, masks, grads, params):
        grads[name] = grads[name] + one_rating_s_gradient(case, data, y, masks, params, n)[name]
    return mistake


def split_boundaries(B):
    """The last rating of split 0, the first of the last split and rating B - 1 (min(16, ceil(B / 16)) splits of
    ceil(B / nsplit) documents: csrc/textcnn.hip, textcnn_wgrad_splits)."""
    nsplit = min(16, -(-B // 16))
    per = -(-B // nsplit)
    return sorted({min(per, B) - 1, (nsplit - 1) * per, B - 1})


assert split_boundaries(17) == [8, 9, 16] and split_boundaries(241) == [15, 240]
assert split_boundaries(256) == [15, 240, 255] and split_boundaries(257) == [16, 255, 256]
assert split_boundaries(1000) == [62, 945, 999]

# two splits; a last split of one document; the last folded batch size; the first unfolded one, and with dropout on;
# several rounds per split
DENSE_SEEDED = ['deepconn-B17', 'deepconn-B241', 'deepconn-B256', 'deepconn-B257', 'deepconn-B257-p0.3', 'deepconn-B1000']
DENSE_TENSORS = ['user_conv.convs.0.weight', 'item_conv.convs.0.bias', 'user_conv.fc.weight', 'fm.V']
EVERY_BOUNDARY = [(id, n) for id in DENSE_SEEDED for n in split_boundaries(int(BY_ID[id].hp['batch_size']))]


@pytest.mark.parametrize('mistake', [one_rating_missing_from_a_dense_sum, one_rating_counted_twice],
                         ids=lambda f: f.__name__)
@pytest.mark.parametrize('name', DENSE_TENSORS)
@pytest.mark.parametrize('case,n', EVERY_BOUNDARY)
def test_one_rating_lost_or_doubled_in_a_dense_sum_raises(case, n, name, mistake):
    """DeepCoNN's dense gradients are sums over the B ratings, dealt to splits and rounds by B: with the term of ONE
    rating at a split boundary left out of (or added twice to) one tensor's gradient, the moments alone raise on both
    steps -- at B = 1,000 as at B = 17."""
    case = BY_ID[case]
    steps = run(case, mistake(case, name, n))
    clean = run(case)
    assert not torch.equal(steps[0][0].grads[name], clean[0][0].grads[name])
    for s32, s64 in steps:
        with pytest.raises(AssertionError, match='exp_avg(_sq)? ' + name.replace('.', r'\.')):
            assert_step_state(StateStandIn(s32, with_grads=False), StateStandIn(s32), s64, what=case.id)


def test_a_widened_atol_is_eight_oracle_distances_and_holds_for_its_tensor_alone():
    """The rule for a kernel whose summation order needs more than atol 1e-7 on one tensor: 8 x the float32 oracle's own
    largest distance from float64 on it, for that tensor and that quantity only."""
    case = BY_ID['mf_dot-D10-B2100']
    s32, s64 = run(case)[0]
    for kind in ('grad', 'exp_avg', 'exp_avg_sq'):
        assert oracle_atol(s64, s32, kind, 'global_bias') == 8 * state_distances(StateStandIn(s32), s64)[kind]['global_bias']
    off, _ = run(case, lambda step, data, y, masks, grads, params: grads.update(global_bias=grads['global_bias'] + 1e-2))[0]
    stand_in = StateStandIn(off)
    wide = {(kind, 'global_bias'): 1e-1 for kind in ('grad', 'exp_avg', 'exp_avg_sq')}
    assert_step_state(stand_in, stand_in, s64, atol=wide)
    with pytest.raises(AssertionError, match='exp_avg global_bias'):
        assert_step_state(stand_in, stand_in, s64, atol={(kind, 'item_bias'): 1e-1 for kind, _ in wide})
