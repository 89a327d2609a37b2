"""The Adam kernels (csrc/adam.hip, csrc/adam_device.h, and the fast form through csrc/rows_large.hip), one step at a
time against the float64 reference and the per-rounding bounds of tests/adam_ref.py: step counts from 1 to beyond the
underflow of both beta^t, every regime a table element can be in, the host-step and device-counter forms, every
placement of a tensor in a list (alignment, position, chunk size), the data-parallel form and its guard, and the
Python Adam class step by step.  tests/test_adam_ref.py shows on the CPU that a float32 emulation of the written
operations passes these bounds at these very inputs and that subtly wrong kernels do not.  Every device buffer lies
inside a larger allocation between 64-float sentinel runs that must keep their bits.  Each test prints the worst
error / bound it saw (`ADAM_RATIO <what> <form> p m v`).  Runs on a real MI355X only (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as ar

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 64
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload: compared as int32


def _lib():
    from reviews4rec_amd import _lib
    return _lib


class Arena:
    """Float32 buffers inside ONE device allocation, each at a 16-byte boundary plus `shift` floats, with at least
    GUARD sentinel floats before and after it."""

    def __init__(self, specs):
        self.spans, cur = [], 0
        for numel, shift in specs:
            cur = (cur + GUARD + 3) // 4 * 4 + shift
            self.spans.append((cur, numel))
            cur += numel
        self.size = cur + GUARD
        self.bits = torch.full((self.size,), SENTINEL, dtype=torch.int32, device=DEV)
        self.f = self.bits.view(torch.float32)
        assert self.bits.data_ptr() % 16 == 0
        self.outside = torch.ones(self.size, dtype=torch.bool, device=DEV)
        for off, numel in self.spans:
            self.outside[off:off + numel] = False

    def view(self, k):
        off, numel = self.spans[k]
        return self.f[off:off + numel]

    def put(self, k, x):
        self.view(k).copy_(torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1)))

    def ptr(self, k):
        return self.bits.data_ptr() + 4 * self.spans[k][0]

    def guards_intact(self):
        return bool((self.bits[self.outside] == SENTINEL).all())


class Launch:
    """The four arenas of one r4r_adam_multi call: .before / .after views per tensor."""

    def __init__(self, tensors):
        self.tensors = tensors
        self.n = len(tensors)
        self.numel = [int(np.asarray(t['p']).size) for t in tensors]
        self.arena = {}
        for name in 'pgmv':
            self.arena[name] = Arena([(n, t.get('shift', {}).get(name, 0)) for n, t in zip(self.numel, tensors)])
            for k, t in enumerate(tensors):
                if t[name] is not None:
                    self.arena[name].put(k, t[name])
        self.before = {name: a.bits.clone() for name, a in self.arena.items()}

    def old(self, name, k):
        off, numel = self.arena[name].spans[k]
        return self.before[name].view(torch.float32)[off:off + numel]

    def new(self, name, k):
        return self.arena[name].view(k)

    def run(self, t, hp, step_dev=None):
        L = _lib()
        arr = ctypes.c_uint64 * self.n
        ptrs = {name: arr(*[0 if (name == 'g' and x[name] is None) else self.arena[name].ptr(k)
                            for k, x in enumerate(self.tensors)]) for name in 'pgmv'}
        rc = L.lib().r4r_adam_multi(self.n, ptrs['p'], ptrs['g'], ptrs['m'], ptrs['v'],
                                    (ctypes.c_int64 * self.n)(*self.numel), hp['lr'], hp['beta1'], hp['beta2'],
                                    hp['eps'], hp['wd'], 0 if step_dev is not None else t, L.ptr(step_dev),
                                    L.current_stream())
        L.check(rc, 'r4r_adam_multi')
        torch.cuda.synchronize()
        for name in 'pmv':
            assert self.arena[name].guards_intact(), 'sentinels around %s were written' % name
        assert torch.equal(self.arena['g'].bits, self.before['g']), 'the gradient buffers (or their sentinels) changed'
        return self

    def check(self, what, t, hp, ks=None):
        """Every listed tensor (default: all) against the IEEE bound of the reference run on the device; a zero-length
        tensor has nothing to check.  -> worst error / bound by name."""
        worst = dict(p=0.0, m=0.0, v=0.0)
        for k in (range(self.n) if ks is None else ks):
            if self.numel[k] == 0:
                continue
            g = None if self.tensors[k]['g'] is None else self.old('g', k)
            ref = ar.adam_ref(self.old('p', k), g, self.old('m', k), self.old('v', k), t, **hp)
            frac = ar.check('%s tensor %d' % (what, k), {name: self.new(name, k) for name in 'pmv'}, ref)
            worst = {name: max(worst[name], frac[name]) for name in worst}
        return worst

    def result_bits(self, k):
        return {name: ar.bits(self.new(name, k)) for name in 'pmv'}


def tensor(p, g, m, v, shift=None):
    return dict(p=p, g=g, m=m, v=v, shift=dict(shift or {}))


def report(what, form, worst):
    print('ADAM_RATIO %s %s p %.4f m %.4f v %.4f' % (what, form, worst['p'], worst['m'], worst['v']))


def counter(t):
    return torch.tensor([t - 1], dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------------------------- (a), (b): one step from any state
@pytest.mark.parametrize('case', ar.STEP_CASES, ids=ar.case_id)
def test_one_step_with_a_host_step(case):
    t, hp = case['t'], case['hp']
    run = Launch([tensor(*ar.case_inputs(case))]).run(t, hp)
    report(case['name'], 'ieee', run.check(case['name'], t, hp))


@pytest.mark.parametrize('case', ar.STEP_CASES, ids=ar.case_id)
def test_one_step_with_a_device_counter(case):
    """step_dev holds t - 1: the kernel derives both corrections with a device pow in double.  Same bound, the counter
    is left alone, and -- unless t sits on a rounding boundary of a scalar -- the host-step launch's bits."""
    t, hp = case['t'], case['hp']
    ctr = counter(t)
    run = Launch([tensor(*ar.case_inputs(case))]).run(t, hp, step_dev=ctr)
    report(case['name'], 'ieee-step_dev', run.check(case['name'], t, hp))
    assert int(ctr.item()) == t - 1
    if not ar.fragile(t, hp['lr'], hp['beta1'], hp['beta2']):
        host = Launch([tensor(*ar.case_inputs(case))]).run(t, hp)
        for name in 'pmv':
            assert ar.bits_equal(run.new(name, 0), host.new(name, 0)), '%s differs from the host-step launch' % name


@pytest.mark.parametrize('betas', ar.BETA_PAIRS, ids=str)
def test_device_counter_and_host_step_give_the_same_bits_over_2048_consecutive_steps(betas):
    """One 1,028-element tensor, t = 1 .. 2,048 with a fresh gradient each step: both forms from the same state.  A t is
    left out only where adam_ref.fragile says two correct pows may round a scalar differently (at most 1 %;
    tests/test_adam_ref.py shows the condition leaves out no more)."""
    L = _lib()
    hp = dict(ar.DEFAULTS, beta1=betas[0], beta2=betas[1])
    n = ar.CONSEC_N
    p0, _, _, _ = ar.adam_state(n, 60)
    arenas = {name: Arena([(n, 0), (n, 0)]) for name in 'pgmv'}       # tensor 0: host step; tensor 1: device counter
    for k in (0, 1):
        arenas['p'].put(k, p0)
        arenas['m'].put(k, np.zeros(n, np.float32))
        arenas['v'].put(k, np.zeros(n, np.float32))
    gen = torch.Generator(device=DEV).manual_seed(61)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    differs = torch.zeros(ar.CONSEC_STEPS + 1, dtype=torch.bool, device=DEV)
    one = ctypes.c_uint64 * 1
    for t in range(1, ar.CONSEC_STEPS + 1):
        g = torch.randn(n, generator=gen, device=DEV) * 0.3
        if t % 7 == 0:
            g[::3] = 0.0
        for k in (0, 1):
            arenas['g'].view(k).copy_(g)
            rc = L.lib().r4r_adam_multi(1, *[one(arenas[name].ptr(k)) for name in 'pgmv'], (ctypes.c_int64 * 1)(n),
                                        hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], hp['wd'], t if k == 0 else 0,
                                        L.ptr(ctr) if k == 1 else None, L.current_stream())
            L.check(rc, 'r4r_adam_multi')
        same = torch.ones((), dtype=torch.bool, device=DEV)
        for name in 'pmv':
            a = arenas[name]
            same &= (a.view(0).view(torch.int32) == a.view(1).view(torch.int32)).all()
        differs[t] = ~same
        for name in 'pmv':                                    # the next step starts from the host-step state on both
            arenas[name].view(1).copy_(arenas[name].view(0))
        ctr += 1
    torch.cuda.synchronize()
    assert int(ctr.item()) == ar.CONSEC_STEPS
    for name in 'pgmv':
        assert arenas[name].guards_intact()
    left_out = [t for t in range(1, ar.CONSEC_STEPS + 1) if ar.fragile(t, hp['lr'], *betas)]
    assert len(left_out) <= ar.CONSEC_STEPS // 100
    bad = [t for t in differs.nonzero().flatten().tolist() if t not in left_out]
    lines = ['t %d: host scalars %r, float64 %r' % (t, tuple(float(x) for x in ar.host_scalars(t, hp['lr'], *betas)),
                                                    ar.ref_scalars(t, hp['lr'], *betas)) for t in bad[:8]]
    assert not bad, '%d step counts differ: %s' % (len(bad), '; '.join(lines))


# ------------------------------------------------------------------------------ (c): placement does not change a bit
@pytest.fixture(scope='module')
def placement():
    """The 4,099-element tensor alone and 16-byte aligned: the bits every other layout must give."""
    case = ar.PLACEMENT_CASE
    p, g, m, v = ar.case_inputs(case)
    run = Launch([tensor(p, g, m, v)]).run(case['t'], case['hp'])
    report('placement alone', 'ieee', run.check('alone', case['t'], case['hp']))
    return dict(p=p, g=g, m=m, v=v, bits=run.result_bits(0))


def neighbour(k, numel, g_null):
    p, g, m, v = ar.adam_state(numel, 700 + k)
    return tensor(p, None if g_null else g, m, v)


def assert_same_bits(what, run, k, want):
    got = run.result_bits(k)
    for name in 'pmv':
        assert np.array_equal(got[name], want[name]), '%s: %s of the 4,099-element tensor differs from the lone, aligned launch' % (what, name)


@pytest.mark.parametrize('shift', [dict(p=1, g=1, m=1, v=1), dict(p=3, g=3, m=3, v=3), dict(g=1), dict(g=2), dict(m=1),
                                   dict(p=2, m=2, v=2)],
                         ids=['all+4B', 'all+12B', 'g+4B', 'g+8B', 'm+4B', 'pmv+8B'])
def test_alignment_does_not_change_a_bit(placement, shift):
    """Everything 4 (12) bytes off a 16-byte boundary, and ONE operand off (the gradient at 4 and 8 bytes, a moment, or
    everything but the gradient): the scalar path for that tensor."""
    case = ar.PLACEMENT_CASE
    run = Launch([tensor(placement['p'], placement['g'], placement['m'], placement['v'], shift=shift)])
    for name in 'pgmv':
        assert run.arena[name].ptr(0) % 16 == 4 * shift.get(name, 0)
    run.run(case['t'], case['hp'])
    assert_same_bits(str(shift), run, 0, placement['bits'])


@pytest.mark.parametrize('pos,n', ar.LIST_LAYOUTS)
def test_position_in_a_list_does_not_change_a_bit(placement, pos, n):
    """The pos-th of n tensors (16 per launch: the 16th ends a launch, the 17th and 33rd begin one), among neighbours of
    0 .. 2,049 elements, zero-length ones first, in the middle and last, some with a null gradient, and with the
    gradient of the nearest neighbour of 1,023 elements or more misaligned: only THAT tensor takes the scalar path."""
    case = ar.PLACEMENT_CASE
    numel, g_null = ar.list_layout(pos, n)
    tensors = [neighbour(k, numel[k], g_null[k]) for k in range(n)]
    tensors[pos - 1] = tensor(placement['p'], placement['g'], placement['m'], placement['v'])
    for k in sorted(range(n), key=lambda k: abs(k - (pos - 1))):
        if k != pos - 1 and numel[k] >= 1023 and not g_null[k]:
            tensors[k]['shift'] = dict(g=1)
            break
    run = Launch(tensors).run(case['t'], case['hp'])
    assert_same_bits('tensor %d of %d' % (pos, n), run, pos - 1, placement['bits'])
    report('list %d/%d' % (pos, n), 'ieee', run.check('list %d/%d' % (pos, n), case['t'], case['hp']))


@pytest.mark.parametrize('which', ['chunk8192', 'chunk1024'])
def test_chunk_size_does_not_change_a_bit(placement, which):
    """A list of 4 Mi elements or more runs at 8,192 elements per workgroup, one of 4 Mi - 1 at 1,024: the 4,099-element
    tensor comes last, behind tensors of 511 chunks, one chunk less / more than a chunk by one element, 1, 0 and 7
    elements.  Same bits, and EVERY element of the list inside the bound of the float64 reference (run on the device)."""
    case = ar.PLACEMENT_CASE
    numel = ar.BIG_LIST if which == 'chunk8192' else ar.UNDER_LIST
    assert (sum(numel) >= ar.FOUR_MI) == (which == 'chunk8192') and _lib().lib().r4r_adam_chunk_elems() == 8192
    tensors = [neighbour(k, numel[k], k == 2) for k in range(len(numel) - 1)]
    tensors.append(tensor(placement['p'], placement['g'], placement['m'], placement['v']))
    run = Launch(tensors).run(case['t'], case['hp'])
    assert_same_bits(which, run, len(numel) - 1, placement['bits'])
    report(which, 'ieee', run.check(which, case['t'], case['hp']))


# -------------------------------------------------------------------------------------- (d): the data-parallel form
def gathered_call(a, world, numel, t, hp, g_sum, abort=None, guarded=False):
    L = _lib()
    args = [a['p'].ptr(0), a['gathered'].ptr(0), world, a['g_sum'].ptr(0) if g_sum else None, a['m'].ptr(0),
            a['v'].ptr(0), numel, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], hp['wd'], t]
    if guarded:
        rc = L.lib().r4r_adam_gathered_guarded(*args, L.ptr(abort), L.current_stream())
    else:
        rc = L.lib().r4r_adam_gathered(*args, L.current_stream())
    torch.cuda.synchronize()
    return rc


def gathered_arenas(world, numel, t, shift=0):
    p, gathered, m, v = ar.gathered_inputs(world, numel, t)
    a = dict(p=Arena([(numel, shift)]), gathered=Arena([(world * numel, 0)]), m=Arena([(numel, 0)]),
             v=Arena([(numel, 0)]), g_sum=Arena([(numel, 0)]))
    for name, x in (('p', p), ('gathered', gathered), ('m', m), ('v', v)):
        a[name].put(0, x)
    return a, (p, gathered, m, v)


def snapshot(a):
    return {name: x.bits.clone() for name, x in a.items()}


def unchanged(a, snap, names=None):
    return all(torch.equal(a[name].bits, snap[name]) for name in (names or a))


@pytest.mark.parametrize('numel', ar.GATHERED_NUMELS)
@pytest.mark.parametrize('world', ar.GATHERED_WORLDS)
def test_gathered_sums_in_rank_order_and_steps_within_the_bound(world, numel):
    hp = ar.DEFAULTS
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in ar.GATHERED_STEPS:
        results = {}
        for g_sum in (True, False):
            a, (p, gathered, m, v) = gathered_arenas(world, numel, t)
            snap = snapshot(a)
            rc = gathered_call(a, world, numel, t, hp, g_sum)
            _lib().check(rc, 'r4r_adam_gathered')
            for name in a:
                assert a[name].guards_intact(), name
            assert unchanged(a, snap, ['gathered'] if g_sum else ['gathered', 'g_sum'])
            gs = ar.sequential_sum(gathered)
            if g_sum:
                assert ar.bits_equal(a['g_sum'].view(0), gs), 'g_sum is not the sequential float32 sum in rank order'
            if numel:
                ref = ar.adam_ref(p, gs, m, v, t, **hp)
                frac = ar.check('gathered world %d numel %d t %d' % (world, numel, t),
                                {name: a[name].view(0) for name in 'pmv'}, ref)
                worst = {name: max(worst[name], frac[name]) for name in worst}
            results[g_sum] = {name: ar.bits(a[name].view(0)) for name in 'pmv'}
        for name in 'pmv':
            assert np.array_equal(results[True][name], results[False][name])
        # the guard: a non-zero word leaves everything as it was, a zero word gives the unguarded call's bits
        for word in (1, 0x80000000, 0):
            a, _ = gathered_arenas(world, numel, t)
            snap = snapshot(a)
            abort = torch.tensor([word], dtype=torch.int64, device=DEV).view(torch.int32)[:1]
            rc = gathered_call(a, world, numel, t, hp, True, abort=abort, guarded=True)
            _lib().check(rc, 'r4r_adam_gathered_guarded')
            assert int(abort.view(torch.int32)[0].item()) & 0xFFFFFFFF == word
            if word:
                assert unchanged(a, snap), 'abort word %#x: the launch wrote' % word
            else:
                for name in 'pmv':
                    assert np.array_equal(ar.bits(a[name].view(0)), results[True][name])
                assert a['g_sum'].guards_intact() and (numel == 0 or not unchanged(a, snap, ['g_sum']))
    report('gathered world %d numel %d' % (world, numel), 'ieee', worst)


@pytest.mark.parametrize('numel,shift,message', [(1022, 0, 'multiple of 4'), (1023, 0, 'multiple of 4'),
                                                 (1024, 1, '16-byte aligned'), (1024, 2, '16-byte aligned')])
def test_gathered_refuses_what_its_float4_accesses_cannot_take(numel, shift, message):
    hp = ar.DEFAULTS
    for guarded in (False, True):
        a, _ = gathered_arenas(2, numel, 3, shift=shift)
        snap = snapshot(a)
        rc = gathered_call(a, 2, numel, 3, hp, True, guarded=guarded)
        assert rc != 0 and message in _lib().lib().r4r_last_error().decode()
        assert unchanged(a, snap), 'a refused call wrote'


# ------------------------------------------------------------------- (e): the fast form through r4r_rows_apply_large
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('W', ar.ROWS_WIDTHS)
def test_rows_apply_large_is_the_fast_adam_of_each_named_row(W, bias):
    """Every named row is named once, so its gradient is one entry and the launch is adam_elem_fast of that row (and of
    its bias element); rows nobody names and everything outside the tables keep their bits."""
    L = _lib()
    hp = ar.DEFAULTS
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in ar.ROWS_STEPS:
        d = ar.rows_inputs(W, t)
        named = torch.from_numpy(d['named'])
        rest = torch.ones(ar.ROWS_TOTAL, dtype=torch.bool)
        rest[named] = False
        a = {name: Arena([(ar.ROWS_TOTAL * W, 0)]) for name in 'pmv'}
        a.update({name: Arena([(ar.ROWS_TOTAL, 0)]) for name in ('bp', 'bm', 'bv')})
        a.update(grads=Arena([(d['grads'].size, 0)]), gbias=Arena([(d['gbias'].size, 0)]))
        for name in a:
            a[name].put(0, d[name])
        snap = snapshot(a)
        ids = torch.from_numpy(d['ids']).to(DEV)
        scratch = torch.empty(L.lib().r4r_rows_large_ws_bytes(ids.numel()), dtype=torch.uint8, device=DEV)
        rc = L.lib().r4r_rows_apply_large(L.ptr(ids), a['grads'].ptr(0), a['gbias'].ptr(0) if bias else None, ids.numel(),
                                          W, a['p'].ptr(0), a['m'].ptr(0), a['v'].ptr(0),
                                          *[a[name].ptr(0) if bias else None for name in ('bp', 'bm', 'bv')],
                                          ar.ROWS_TOTAL, L.ptr(scratch), scratch.numel(), hp['lr'], hp['beta1'],
                                          hp['beta2'], hp['eps'], hp['wd'], t, L.current_stream())
        L.check(rc, 'r4r_rows_apply_large')
        torch.cuda.synchronize()
        for name in a:
            assert a[name].guards_intact(), name
        assert unchanged(a, snap, ['grads', 'gbias'] + ([] if bias else ['bp', 'bm', 'bv']))
        assert torch.equal(ids.cpu(), torch.from_numpy(d['ids']))
        groups = [(('p', 'm', 'v'), d['g_rows'], W)] + ([(('bp', 'bm', 'bv'), d['g_bias'], 1)] if bias else [])
        for (np_, nm, nv), g, width in groups:
            lo = a[np_].spans[0][0]
            old = {x: snap[x].view(torch.float32)[lo:lo + ar.ROWS_TOTAL * width].reshape(ar.ROWS_TOTAL, width).cpu()
                   for x in (np_, nm, nv)}
            new = {x: a[x].view(0).reshape(ar.ROWS_TOTAL, width).cpu() for x in (np_, nm, nv)}
            for x in (np_, nm, nv):
                assert ar.bits_equal(new[x][rest], old[x][rest]), '%s: a row nobody names changed' % x
            gr = torch.from_numpy(np.ascontiguousarray(g.reshape(ar.ROWS_TOTAL, width)))[named]
            ref = ar.adam_ref(old[np_][named], gr, old[nm][named], old[nv][named], t, fast=True, **hp)
            frac = ar.check('rows W %d t %d %s' % (W, t, np_), dict(p=new[np_][named].contiguous(),
                                                                    m=new[nm][named].contiguous(),
                                                                    v=new[nv][named].contiguous()), ref)
            worst = {name: max(worst[name], frac[name]) for name in worst}
    report('rows W %d %s' % (W, 'bias' if bias else 'nobias'), 'fast', worst)


# -------------------------------------------------------------------------------------- (f): the Python Adam class
def test_adam_class_step_by_step_against_the_reference():
    """40 parameters of 1 .. 2,049 elements in three groups that skip different steps (grad = None), so that every
    step() launches up to three lists at three step counts; 12 steps, each checked against the reference applied to the
    device's own previous state (a per-step bound, not a drifting trajectory); a skipped parameter keeps its bits."""
    from reviews4rec_amd.optim import Adam
    hp = ar.DEFAULTS
    params = [torch.nn.Parameter(torch.from_numpy(ar.class_param(i, n)).to(DEV)) for i, n in enumerate(ar.CLASS_SIZES)]
    opt = Adam(params, lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'], weight_decay=hp['wd'])
    taken = [0] * len(params)
    worst = dict(p=0.0, m=0.0, v=0.0)
    lists = 0
    for step in range(ar.CLASS_STEPS):
        before = []
        for i, p in enumerate(params):
            st = opt.state.get(id(p))
            before.append((p.detach().clone(),
                           torch.zeros_like(p) if st is None else st['exp_avg'].clone(),
                           torch.zeros_like(p) if st is None else st['exp_avg_sq'].clone()))
            p.grad = (torch.from_numpy(ar.class_grad(i, step, p.numel())).to(DEV)
                      if ar.class_has_grad(i, step) else None)
        lists = max(lists, len({taken[i] + 1 for i in range(len(params)) if ar.class_has_grad(i, step)}))
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            p0, m0, v0 = before[i]
            st = opt.state.get(id(p))
            if not ar.class_has_grad(i, step):
                assert ar.bits_equal(p.detach(), p0)
                if st is not None:
                    assert ar.bits_equal(st['exp_avg'], m0) and ar.bits_equal(st['exp_avg_sq'], v0)
                continue
            taken[i] += 1
            ref = ar.adam_ref(p0, p.grad, m0, v0, taken[i], **hp)
            frac = ar.check('parameter %d step %d' % (i, step), dict(p=p.detach(), m=st['exp_avg'], v=st['exp_avg_sq']), ref)
            worst = {name: max(worst[name], frac[name]) for name in worst}
    assert sorted(set(taken)) == [7, 10, 12] and lists == 3
    sd = opt.state_dict()['state']
    assert [sd[i]['step'] for i in range(len(params))] == taken
    report('Adam class', 'ieee', worst)
