"""Shared test helpers: golden-fixture loading, synthetic batches and the float64 step-state checker."""
import contextlib
import inspect
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

GOLDEN_CASES = ['mf_bias_only', 'mf_dot', 'mf_full', 'deepconn_e20', 'deepconn_e64',
                'deepconnpp_e20', 'narre_e16', 'transnet_e16', 'transnetpp_e16',
                'neumf_gmf', 'neumf_mlp', 'neumf_full']
TRAINABLE_CASES = [c for c in GOLDEN_CASES if not c.startswith('transnet')]

_INT_KEYS = ('latent_size', 'word_embed_size', 'input_length', 'total_users', 'total_items',
             'narre_num_reviews', 'narre_num_words', 'batch_size')
_FLOAT_KEYS = ('dropout', 'lr', 'weight_decay')


class Golden:
    """One npz fixture written by tests/golden/make_golden.py."""

    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
        self.z = {k: z[k] for k in z.files}
        hp = dict(zip(self.z['hp_keys'].tolist(), self.z['hp_vals'].tolist()))
        for k in _INT_KEYS:
            hp[k] = int(hp[k])
        for k in _FLOAT_KEYS:
            hp[k] = float(hp[k])
        self.hp = hp
        self.vocab = int(self.z['vocab'])

    def group(self, prefix, device='cpu'):
        pre = prefix + '/'
        return {k[len(pre):]: torch.from_numpy(v.copy()).to(device)
                for k, v in self.z.items() if k.startswith(pre)}

    def params(self, tag='w', device='cpu'):
        return self.group(tag, device)

    def batch(self, k, device='cpu'):
        d = self.group('b%d' % k, device)
        data = [d[str(s)] for s in range(7)]
        return data, torch.from_numpy(self.z['y%d' % k].copy()).to(device)

    def neg_batch(self, device='cpu'):
        d = self.group('neg', device)
        return [d[str(s)] for s in range(7)]

    def arr(self, key):
        return torch.from_numpy(self.z[key].copy())

    def has(self, key):
        return key in self.z


def synthetic_review_batch(B, T, V, U, I, seed=0, R=None, W=None, device='cpu'):
    """Amazon-shaped random batch in the 7-slot layout of data_fast.py:101-109."""
    rng = np.random.default_rng(seed)

    def docs(shape):
        tok = rng.integers(1, V, size=shape)
        fill = rng.integers(1, shape[-1] + 1, size=shape[:-1])
        return np.where(np.arange(shape[-1]) < fill[..., None], tok, 0)

    if R is None:
        ur, ir = docs((B, T)), docs((B, T))
    else:
        ur, ir = docs((B, R, W)), docs((B, R, W))
    data = [docs((B, T)), rng.integers(0, U + 2, size=(B, 10)), rng.integers(0, I + 2, size=(B, 10)),
            ur, ir, rng.integers(0, U, size=(B,)), rng.integers(0, I, size=(B,))]
    y = rng.integers(1, 6, size=(B,)).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(d.astype(np.int64))).to(device) for d in data], \
        torch.from_numpy(y).to(device)


class OracleModule(torch.nn.Module):
    """CPU stand-in with the drop-in models' duck type (Model(hp) -> forward(data)),
    computing with the oracle.  Lets the host loop / batcher / data-parallel logic be
    tested where no GPU exists.  TEST ONLY."""

    def __init__(self, hyper_params, params=None, vocab=50, seed=0):
        super().__init__()
        import oracle
        self.hyper_params = hyper_params
        P = params if params is not None else oracle.init_params(hyper_params, vocab_size=vocab, seed=seed)
        self.names = list(P)
        self.plist = torch.nn.ParameterList([
            torch.nn.Parameter(v.clone(), requires_grad=not k.endswith('word2vec.weight')) for k, v in P.items()])

    def as_dict(self):
        return dict(zip(self.names, self.plist))

    def forward(self, data):
        import oracle
        return oracle.model_forward(self.as_dict(), data, self.hyper_params, train=self.training)


TINY_DIR = os.path.join(GOLDEN_DIR, 'tiny')
TINY_FILES = ('train', 'test', 'val', 'user_reviews', 'item_reviews', 'test_reviews', 'this_index_user_item',
              'num_users_items', 'word2vec', 'user_count', 'item_count', 'negs')


def materialise_tiny(root):
    """Write tests/golden/tiny/dataset.json back into the .pkl files of a reference dataset directory
    (preprocess_random_split.py:296-316, make_negative_sets.py:83) -> the data_dir string."""
    import json
    import pickle
    ds = json.load(open(os.path.join(TINY_DIR, 'dataset.json')))

    def ints(d, depth):
        if depth == 0 or not isinstance(d, dict):
            return d
        return {int(k): ints(v, depth - 1) for k, v in d.items()}

    ds['user_reviews'], ds['item_reviews'] = ints(ds['user_reviews'], 1), ints(ds['item_reviews'], 1)
    ds['test_reviews'], ds['this_index_user_item'] = ints(ds['test_reviews'], 2), ints(ds['this_index_user_item'], 2)
    ds['user_count'], ds['item_count'] = ints(ds['user_count'], 1), ints(ds['item_count'], 1)
    ds['negs'] = ints(ds['negs'], 1)
    root = os.path.join(str(root), 'data', 'Tiny', '5_core')
    os.makedirs(root, exist_ok=True)
    for name in TINY_FILES:
        with open(os.path.join(root, name + '.pkl'), 'wb') as f:
            pickle.dump(ds[name], f, 2)
    return root + '/'


def tiny_hp(model_type, data_dir, **kw):
    """hyper_params of a tests/golden/tiny fixture (the generator's tiny_hp) + the data directory."""
    import json
    name = model_type + ('_eval' if model_type in ('deepconn', 'NARRE', 'MF_dot', 'transnet++') else '_e2e')
    hp = dict(json.load(open(os.path.join(TINY_DIR, name + '.json')))['hp'])
    for k in ('total_users', 'total_items', 'total_words'):
        hp.pop(k, None)                                   # load_data sets them (data.py:469-471)
    hp['data_dir'] = data_dir
    hp.update(kw)
    return hp


# ----------------------------------------------------------------------------------------------------------------------
# The float64 step-state checker: what a native training step leaves in Adam's moments, against the oracle in float64.
#
# Two Adam steps hide the size of a gradient from the weights (step 1 is lr g / (|g| + eps), step 2 is homogeneous of
# degree 0 in (g1, g2)); exp_avg after step 1 is 0.1 (g + wd p): the gradient as the kernel summed it.
# ----------------------------------------------------------------------------------------------------------------------
STATE_RTOL = 1e-4                   # the golden trajectory tests' tolerances (test_gpu_engine.py, NARRE trajectory)
GRAD_ATOL = 1e-7                    # ... gradients and exp_avg
EXP_AVG_SQ_ATOL = 1e-10             # ... exp_avg_sq
# An element whose gradient has been exactly 0 so far (a row no rating names, a column whose dropout multiplier is 0)
# holds the pure weight-decay moments 0.1 wd p and 0.001 (wd p)^2: ~1e-8 and ~1e-17, far below the absolute tolerances
# above, so those elements are compared on their own with STATE_RTOL and absolute tolerances below any such value
# (fp32 evaluates them with a handful of roundings, 1 - 0.999f alone is off by 1.3e-5: STATE_RTOL covers it).
PURE_WD_ATOL = {'exp_avg': 1e-20, 'exp_avg_sq': 1e-32}
TRANSNET_GROUPS = ('target', 'source', 'source_fm')

WEIGHTS_CLOSE = dict(rtol=1e-5, atol=5e-6)                                   # the MF engine tests' weight criterion


def weights_outliers(frac=2e-3, max_diff=5e-4):
    """The text engines' weight criterion: share of elements off by more than 2e-5 + 1e-4 |w| below `frac`, and no
    element off by `max_diff` or more."""
    return dict(frac=frac, max_diff=max_diff)


def ill_conditioned(name):
    """NARRE's scorer output bias feeds a softmax over reviews, which is shift
    invariant: its true gradient is exactly 0, what autograd returns is rounding
    noise (~1e-9), and Adam normalises that noise to +-lr steps.  Its trajectory is
    not comparable between two correct implementations."""
    return name.startswith('attention_scorer_') and name.endswith('.3.bias')


def is_row_tensor(name):
    """ID tables and per-ID bias vectors: the tensors whose gradient rows the steps sum over duplicate ids."""
    return name.endswith('embedding.weight') or name in ('user_bias', 'item_bias')


@contextlib.contextmanager
def _adam_tap(seen, perturb=None):
    """While active, oracle.adam_step records the gradients each optimiser consumes (TransNet's three included) and,
    for the checker's own tests, lets `perturb(grads, params)` seed a mistake into them first."""
    import oracle.optim as O
    real = O.adam_step

    def tapped(params, grads, state, *args, **kw):
        grads = dict(grads)
        if perturb is not None:
            perturb(grads, params)
        for k, g in grads.items():
            assert k not in seen, 'parameter %s stepped twice in one step' % k
            seen[k] = None if g is None else g.detach().clone()
        return real(params, grads, state, *args, **kw)

    O.adam_step = tapped
    try:
        yield
    finally:
        O.adam_step = real


SE_RTOL, SE_ATOL = 1e-4, 1e-5       # per-rating SE: the golden SE comparisons' tolerances (test_gpu_engine.py)


class StepState:
    """What one reference step left: the sum of the squared errors and each rating's (in the reference's dtype),
    gradients, Adam moments and weights by parameter name."""

    def __init__(self, step, sse, se, grads, m, v, params, zero_so_far):
        self.step, self.sse, self.se, self.grads, self.m, self.v, self.params = step, sse, se, grads, m, v, params
        self.zero_so_far = zero_so_far          # row tensors: elements whose gradient was exactly 0 in every step so far


class _StepReference:
    def __init__(self, params, hyper_params, dtype):
        self.hp, self.dtype = dict(hyper_params), dtype
        self.params = {k: v.detach().clone().to(dtype) for k, v in params.items()}
        self.transnet = self.hp['model_type'] in ('transnet', 'transnet++')
        import oracle
        self.states = {g: oracle.AdamState() for g in TRANSNET_GROUPS} if self.transnet else oracle.AdamState()
        self.steps = 0
        self._zero = {}

    def step(self, data, y, masks=None, start=None, perturb=None):
        """One training step on (data, y) with the injected dropout multipliers; returns its StepState.
        start: the weights the engine under test holds before this step (its model's state_dict).  The reference takes
        them over (cast up; its moments stay its own), so that this step is the float64 step FROM THE SAME WEIGHTS.
        Without it, step 2 would compare two trajectories: Adam turns a 1e-9 rounding difference on a gradient of ~1e-8
        into a 1e-4 difference of one weight, and a max-pool or ReLU near a tie then picks another branch -- a
        difference of a whole document's gradient that says nothing about either implementation.  The weights after
        step 1 are compared before they are taken over."""
        import oracle
        if start is not None:
            for k in oracle.trainable_names(self.params):
                self.params[k] = start[k].detach().cpu().to(self.dtype).clone()
        y = y.to(self.dtype)
        if masks is not None:
            masks = {k: v.to(self.dtype) for k, v in masks.items()}
        seen = {}
        with _adam_tap(seen, perturb):
            if self.transnet:
                se, _, _ = oracle.transnet_train_step(self.params, data, y, self.hp, self.states, masks=masks)
                sse = float(se.sum())
            else:
                with torch.no_grad():                        # (train_step returns the sum alone)
                    out = oracle.model_forward(self.params, data, self.hp, train=True, masks=masks)
                    se = oracle.mse_loss(out, y, return_mean=False).reshape(-1).clone()
                sse, _ = oracle.train_step(self.params, data, y, self.hp, self.states, masks=masks)
        self.steps += 1
        states = list(self.states.values()) if self.transnet else [self.states]
        m, v = {}, {}
        for st in states:
            assert not (set(st.m) & set(m))
            m.update({k: t.clone() for k, t in st.m.items()})
            v.update({k: t.clone() for k, t in st.v.items()})
        for k, g in seen.items():
            if g is not None and is_row_tensor(k):
                z = g == 0
                self._zero[k] = z if k not in self._zero else (self._zero[k] & z)
        return StepState(self.steps, sse, se, seen, m, v, {k: t.detach().clone() for k, t in self.params.items()},
                         {k: z.clone() for k, z in self._zero.items()})


def float64_step_reference(params, hyper_params, dtype=torch.float64):
    """The oracle's training step (oracle.train_step; TransNet: oracle.transnet_train_step, its three optimisers as three
    AdamStates keyed by group) on a float64 copy of `params`; ratings and injected dropout multipliers are cast with
    them.  `.step(data, y, masks)` advances it by one step and returns that step's StepState.  dtype=torch.float32 gives
    the oracle as it is: an independent implementation at the kernels' precision, the yardstick of a widened atol."""
    return _StepReference(params, hyper_params, dtype)


class StateStandIn:
    """A StepState behind the engines' duck type -- moments() and, unless told otherwise, grads(data): the float32
    oracle in an engine's place."""

    def __init__(self, state, with_grads=True):
        self.state = state
        if with_grads:
            self.grads = lambda data: {k: g for k, g in state.grads.items() if g is not None}

    def moments(self):
        return self.state.m, self.state.v

    def state_dict(self):
        return self.state.params


def _engine_grads(engine, data):
    fn = getattr(engine, 'dense_grads', None) or getattr(engine, 'grads', None)
    if fn is None:
        return None
    return fn(data) if len(inspect.signature(fn).parameters) else fn()


def state_distances(engine, ref, data=None):
    """{'grad' | 'exp_avg' | 'exp_avg_sq': {name: largest |engine - ref|}} over the parameters the reference steps."""
    m, v = engine.moments()
    out = {'exp_avg': {}, 'exp_avg_sq': {}, 'grad': {}}
    got_g = _engine_grads(engine, data) or {}
    for kind, got, want in (('exp_avg', m, ref.m), ('exp_avg_sq', v, ref.v), ('grad', got_g, ref.grads)):
        for k, w in want.items():
            if w is not None and k in got and not ill_conditioned(k):
                out[kind][k] = float((got[k].detach().cpu().double() - w.double()).abs().max())
    return out


def oracle_atol(ref64, ref32, kind, name, factor=8.0):
    """The widened absolute tolerance of one tensor: `factor` x the float32 oracle's own largest distance from float64 on
    it at the same inputs (8 covers a different association order over a few hundred terms).  kind: 'grad', 'exp_avg' or
    'exp_avg_sq'; never computed from an engine's output."""
    pick = {'grad': lambda r: r.grads, 'exp_avg': lambda r: r.m, 'exp_avg_sq': lambda r: r.v}[kind]
    return factor * float((pick(ref32)[name].double() - pick(ref64)[name].double()).abs().max())


def weights_failures(state_dict, ref_params, weights, skip=ill_conditioned):
    """The weight criteria the engine tests have used all along (WEIGHTS_CLOSE or weights_outliers(...)) as a list of
    failure lines: empty when the weights pass."""
    bad = []
    for k, w in ref_params.items():
        if skip(k) or k not in state_dict:
            continue
        got, w = state_dict[k].detach().cpu().double(), w.double()
        diff = (got - w).abs()
        if 'frac' in weights:
            share = float((diff > 2e-5 + 1e-4 * w.abs()).double().mean())
            if not (share < weights['frac'] and float(diff.max()) < weights['max_diff']):
                bad.append('weight %s: share outside 2e-5 + 1e-4|w| %.3g (limit %.3g), max diff %.3g (limit %.3g)'
                           % (k, share, weights['frac'], float(diff.max()), weights['max_diff']))
        else:
            out = diff > weights['atol'] + weights['rtol'] * w.abs()
            if bool(out.any()):
                bad.append('weight %s: %d of %d elements outside rtol %g atol %g, max diff %.3g'
                           % (k, int(out.sum()), out.numel(), weights['rtol'], weights['atol'], float(diff.max())))
    return bad


def _outside(kind, name, got, want, rtol, atol, where=None):
    """One failure line if any element of `got` (restricted to the mask `where`) is outside rtol / atol of `want`."""
    if tuple(got.shape) != tuple(want.shape):
        return '%s %s: shape %s, the reference has %s' % (kind, name, tuple(got.shape), tuple(want.shape))
    got, want = got.detach().cpu().double(), want.double()
    diff = (got - want).abs()
    out = ~(diff <= atol + rtol * want.abs())                # (a NaN is outside)
    if where is not None:
        out &= where
    if not bool(out.any()):
        return None
    worst = int(torch.where(out, diff, torch.zeros_like(diff)).argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(diff.shape))) if diff.dim() else ()
    return ('%s %s: %d of %d elements outside rtol %g atol %g; worst at %s: %.9g, the reference has %.9g'
            % (kind, name, int(out.sum()), out.numel(), rtol, atol, idx, float(got.reshape(-1)[worst]),
               float(want.reshape(-1)[worst])))


def assert_step_state(engine, model, ref, data=None, weights=None, atol=None, what='', skip=ill_conditioned):
    """After a training step of `engine` on `data`: every element of exp_avg and exp_avg_sq of every parameter the
    reference stepped (every row of every ID table and bias vector; elements whose gradient has been exactly 0 show the
    pure weight-decay moments), of the engine's gradients where it exposes them (grads / dense_grads), and the weights
    under `weights` (WEIGHTS_CLOSE or weights_outliers(...); None: not compared) against the StepState `ref` of
    float64_step_reference.  Only attention_scorer_*.3.bias is left out (ill_conditioned).  Engines with blocked sweeps
    are read through moments(), which flushes.  atol: {(kind, name): value} widens the absolute tolerance of single
    tensors (oracle_atol); skip: the names left out, for the one test that has to leave out more than the ill-conditioned
    bias.  Every failing tensor is reported, then AssertionError."""
    atol = atol or {}
    m, v = engine.moments()
    bad = []
    stepped = [k for k, g in ref.grads.items() if g is not None]
    assert set(stepped) == set(ref.m) == set(ref.v), 'the reference stepped what it has no moments for'
    for kind, got, want, base in (('exp_avg', m, ref.m, GRAD_ATOL), ('exp_avg_sq', v, ref.v, EXP_AVG_SQ_ATOL)):
        for k in got:
            if k not in want and bool((got[k] != 0).any()):
                bad.append('%s %s: non-zero, but the reference never steps this parameter' % (kind, k))
        for k, w in want.items():
            if skip(k):
                continue
            if k not in got:
                bad.append('%s %s: the engine has no such moment' % (kind, k))
                continue
            bad.append(_outside(kind, k, got[k], w, STATE_RTOL, atol.get((kind, k), base)))
            if k in ref.zero_so_far and tuple(got[k].shape) == tuple(w.shape):
                bad.append(_outside(kind + ' (gradient 0 so far: pure weight decay)', k, got[k], w, STATE_RTOL,
                                    PURE_WD_ATOL[kind], where=ref.zero_so_far[k]))
    got_g = _engine_grads(engine, data)
    if got_g is not None:
        for k in stepped:
            if skip(k):
                continue
            if k not in got_g:
                bad.append('grad %s: the engine reports no such gradient' % k)
                continue
            bad.append(_outside('grad', k, got_g[k], ref.grads[k], STATE_RTOL, atol.get(('grad', k), GRAD_ATOL)))
    if weights is not None:
        sd = model.state_dict()
        missing = [k for k in stepped if k not in sd]
        assert not missing, missing
        bad += weights_failures(sd, ref.params, weights, skip)
    bad = [b for b in bad if b]
    assert not bad, '%s after step %d:\n  ' % (what or type(engine).__name__, ref.step) + '\n  '.join(bad)


def assert_per_rating_se(se, ref, what=''):
    """Each rating's squared error of a training step against the StepState `ref`, at SE_RTOL / SE_ATOL."""
    torch.testing.assert_close(se.detach().cpu().double().reshape(-1), ref.se.double().reshape(-1), rtol=SE_RTOL,
                               atol=SE_ATOL, msg=lambda m: '%s per-rating SE of step %d: %s' % (what, ref.step, m))


def multipliers(engine, data):
    """The multipliers the last training step of a native engine drew, flattened: the [n, ND] block is one contiguous
    counter range.  Each engine class has its own call."""
    from reviews4rec_amd import engine as E
    n = data[5].numel()
    if isinstance(engine, E.DeepCoNNEngine):
        m = engine.dropout_multipliers(n, data[3].reshape(n, -1).shape[1])
    elif isinstance(engine, (E.MFEngine, E.IdNetEngine)):
        m = engine.dropout_multipliers(n)
    else:
        m = engine.dropout_multipliers(data)
    torch.cuda.synchronize()
    return m.reshape(-1)


class StepStateProbe:
    """assert_step_state next to an engine test's own oracle steps: built from the initial parameters (copied, before
    the test's oracle moves them), then `after_step` once per training step.  Each step's reference is the float64 step
    from the weights the engine held before it (float64_step_reference, `start`)."""

    def __init__(self, engine, model, params, hyper_params, what=''):
        self.engine, self.model, self.what = engine, model, what
        self.ref = float64_step_reference(params, hyper_params)
        self.before = None

    def after_step(self, data, y, masks=None, weights=None, atol=None, skip=ill_conditioned):
        """data, y: the step's batch (on any device); masks: the dropout multipliers it drew, by oracle site."""
        cpu = [None if d is None else d.cpu() for d in data]
        dev = self.engine.dev
        state = self.ref.step(cpu, y.cpu(), masks, start=self.before)
        assert_step_state(self.engine, self.model, state, data=[None if d is None else d.to(dev) for d in data],
                          weights=weights, atol=atol, what=self.what, skip=skip)
        self.before = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        return state
