"""Float64 restatement of ONE Adam step as csrc/adam_device.h writes it, a per-element a-priori bound for what the two
written forms may return, a float32 emulation of both forms, and the seeded cases of tests/test_adam_ref.py (CPU) and
tests/test_gpu_adam_steps.py (the kernels).  No kernel of the project and no GPU code lives here.

The update (torch.optim.Adam: L2 weight decay added to the gradient, bias-corrected, no amsgrad), exact:
    G = g + wd p        M' = b1 m + (1 - b1) G        V' = b2 v + (1 - b2) G^2
    P' = p - lrb M' / (sqrt(V') isb + eps),   lrb = lr / (1 - b1^t),   isb = 1 / sqrt(1 - b2^t)
p, g, m, v are float32; lr, eps and wd are what the C ABI takes, floats (rounded to float32 on entry here, exact from
then on); b1 and b2 stay doubles.  1 - b^t is -expm1(t log b): no cancellation at small t, exactly 1 once b^t underflows.

The bound.  u = 2^-24 (a correctly rounded operation: half an ulp), U = 2^-23 (one ulp: each scalar that the kernel
holds rounded to float32 -- b1, b2, 1 - b1, 1 - b2, lrb, isb -- and each of v_sqrt_f32 / v_rcp_f32), d = 2^-149 (one
denormal spacing, absolute, per operation: a result below 2^-126 is rounded to a multiple of it).  Every line is
    E(result) = e + k (|exact result| + e) + d,     e = the operands' errors carried through the exact operation
written rnd(exact, e, k) below, k = u unless noted; nothing is first order only, and absolute values are of the exact
intermediates, so a cancelling m' = b1 m + (1 - b1) G keeps the errors of its terms.  One line per operation of
adam_elem_form, in its order:
    g1 = fmaf(wd, p, g)          Eg  = rnd(G, 0)                                  (wd, p, g exact: one rounding)
    a  = omb1 * g1               Ea  = rnd(A, (1 + U) (1 - b1) Eg + U |A|)        A = (1 - b1) G; omb1 rounded: U
    m' = fmaf(beta1, m, a)       Em  = rnd(M', U |b1 m| + Ea)                     beta1 rounded: U
    b  = omb2 * g1               Eb  = rnd(B, (1 + U) (1 - b2) Eg + U |B|)        B = (1 - b2) G
    c  = b * g1                  Ec  = rnd(C, |B| Eg + |G| Eb + Eb Eg)            C = B G
    v' = fmaf(beta2, v, c)       Ev  = rnd(V', U |b2 v| + Ec)
    s  = sqrt(v')                Es  = rnd(S, max(sqrt(V' + Ev) - S, S - sqrt(max(V' - Ev, 0))))         IEEE: k = u
                                 fast: k = U, + 2^-63 where V' - Ev < 2^-126 (v_sqrt_f32 may read a denormal as zero)
    d1 = s * isb                 Ed1 = rnd(S isb, (1 + U) isb Es + U S isb)       isb rounded: U
    dn = d1 + eps                Ed  = rnd(D, Ed1)                                eps exact; D - Ed > 0 is asserted
    q  = m' / dn         IEEE    Eq  = rnd(Q, (Em + |Q| Ed) / (D - Ed))
    r  = rcp(dn)         fast    Er  = Ed / (D (D - Ed)) + U / (D - Ed) + d       v_rcp_f32: one ulp of the result
    q  = m' * r          fast    Eq  = rnd(Q, Em (1 / D + Er) + |M'| Er)
    w  = lrb * q                 Ew  = rnd(W, (1 + U) lrb Eq + U |W|)             lrb rounded: U
    p' = p - w                   Ep  = rnd(P', Ew)
A compiler that contracts d1 + eps or p - w into an fma drops a rounding and stays inside.  The bounds of m', v', p'
are Em, Ev, Ep.  No rtol / atol and no fraction of elements left out; NaN and inf fail."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24                 # half an ulp, relative: a correctly rounded fp32 operation
ULP = 2.0 ** -23                 # one ulp: a float32-rounded scalar, v_sqrt_f32, v_rcp_f32
DEN = 2.0 ** -149                # the denormal spacing of fp32
TINY = 2.0 ** -126               # smallest normal fp32
SQRT_TINY = 2.0 ** -63

DEFAULTS = dict(lr=0.002, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-6)


def f32(x):
    return float(np.float32(x))


def ref_scalars(t, lr, beta1, beta2):
    """(lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) as adam_make_scalars defines them, in float64; lr as the float the
    ABI takes."""
    bc1 = -math.expm1(t * math.log(beta1))
    bc2 = -math.expm1(t * math.log(beta2))
    return f32(lr) / bc1, 1.0 / math.sqrt(bc2)


class AdamRef:
    """val[name], bound[name] for name in 'p', 'm', 'v' (float64 tensors on the inputs' device) and the two scalars."""

    def __init__(self, val, bound, lr_over_bc1, inv_sqrt_bc2):
        self.val, self.bound, self.lr_over_bc1, self.inv_sqrt_bc2 = val, bound, lr_over_bc1, inv_sqrt_bc2


def _t64(x, like=None):
    if x is None:
        return torch.zeros_like(like)
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    assert x.dtype == torch.float32, x.dtype
    return x.detach().to(torch.float64)


def adam_ref(p, g, m, v, t, lr, beta1, beta2, eps, wd, fast=False):
    """One exact step from float32 p, g (None: zero), m, v (numpy arrays or tensors, on any device) and its bounds for
    the IEEE form (adam_elem) or the fast form (adam_elem_fast / adam_pair_fast)."""
    p, m, v = _t64(p), _t64(m), _t64(v)
    g = _t64(g, like=p)
    lrb, isb = ref_scalars(t, lr, beta1, beta2)
    eps, wd = f32(eps), f32(wd)
    k_hw = ULP if fast else U32

    def rnd(exact, e, k=U32):
        return e + k * (exact.abs() + e) + DEN

    G = g + wd * p
    A = (1.0 - beta1) * G
    M = beta1 * m + A
    B = (1.0 - beta2) * G
    C = B * G
    V = beta2 * v + C
    S = V.sqrt()
    D = S * isb + eps
    Q = M / D
    W = lrb * Q
    P = p - W
    Eg = rnd(G, torch.zeros_like(G))
    Ea = rnd(A, (1 + ULP) * (1.0 - beta1) * Eg + ULP * A.abs())
    Em = rnd(M, ULP * (beta1 * m).abs() + Ea)
    Eb = rnd(B, (1 + ULP) * (1.0 - beta2) * Eg + ULP * B.abs())
    Ec = rnd(C, B.abs() * Eg + G.abs() * Eb + Eb * Eg)
    Ev = rnd(V, ULP * (beta2 * v).abs() + Ec)
    Es = rnd(S, torch.maximum((V + Ev).sqrt() - S, S - (V - Ev).clamp(min=0.0).sqrt()), k_hw)
    if fast:
        Es = Es + torch.where(V - Ev < TINY, torch.full_like(S, SQRT_TINY), torch.zeros_like(S))
    Ed1 = rnd(S * isb, (1 + ULP) * isb * Es + ULP * S * isb)
    Ed = rnd(D, Ed1)
    lo = D - Ed
    assert bool((lo > 0).all()), 'the denominator is not bounded away from zero'
    if fast:
        Er = Ed / (D * lo) + ULP / lo + DEN
        Eq = rnd(Q, Em * (1.0 / D + Er) + M.abs() * Er)
    else:
        Eq = rnd(Q, (Em + Q.abs() * Ed) / lo)
    Ew = rnd(W, (1 + ULP) * lrb * Eq + ULP * W.abs())
    Ep = rnd(P, Ew)
    for x in (P, M, V, Ep, Em, Ev):
        assert bool(torch.isfinite(x).all()), 'the reference itself is not finite: the case is out of range'
    return AdamRef(dict(p=P, m=M, v=V), dict(p=Ep, m=Em, v=Ev), lrb, isb)


def check(what, got, ref, names=('p', 'm', 'v')):
    """Asserts |got - float64| <= bound for EVERY element of every name (NaN fails); -> {name: worst error / bound}."""
    out = {}
    for name in names:
        val, bound = ref.val[name], ref.bound[name]
        x = got[name]
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x))
        assert x.dtype == torch.float32 and x.numel() == val.numel(), (what, name, x.dtype, x.numel(), val.numel())
        x = x.detach().to(val.device, torch.float64).reshape(val.shape)
        err = (x - val).abs()
        ok = err <= bound
        if not bool(ok.all()):
            bad = (~ok).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError("%s %s': %d of %d elements beyond their bound, e.g. at %s got %.9g, float64 %.9g, "
                                 'error %.3g, bound %.3g' % (what, name, bad.shape[0], val.numel(), i, float(x[i]),
                                                             float(val[i]), float(err[i]), float(bound[i])))
        out[name] = float((err / bound).max()) if err.numel() else 0.0
    return out


def bits(x):
    """The int32 bit pattern of a float32 array / tensor, as a numpy array (distinguishes -0 from +0, compares NaNs)."""
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return np.ascontiguousarray(x).view(np.int32)


def bits_equal(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


# ------------------------------------------------------------------------------------------------------------ emulation
# The two written forms in float32 numpy: test infrastructure that shows, without a GPU, that the bounds are attainable
# (tests/test_adam_ref.py) and what they reject (MUTATIONS).  fmaf goes through float64 (the product of two float32 is
# exact there); rcp and sqrt are modelled as correctly rounded, v_sqrt_f32 reading a denormal as zero.
MUTATIONS = ('pow32',            # bias corrections computed with float32 pow
             't_minus_1',        # t - 1 in place of t
             'drop_wd_null',     # weight decay dropped when g is null
             'eps_in_sqrt',      # eps added inside the square root
             'beta2_for_m',      # beta2 used for m
             'tail_unwritten')   # the last numel % 4 elements left unwritten


def host_scalars(t, lr, beta1, beta2, mutate=None):
    """adam_make_scalars: the two float32 scalars from a double pow."""
    F = np.float32
    with np.errstate(all='ignore'):
        if mutate == 't_minus_1':
            t = t - 1
        if mutate == 'pow32':
            bc1 = F(1) - np.power(F(beta1), F(t))
            bc2 = F(1) - np.power(F(beta2), F(t))
            return F(F(lr) / bc1), F(F(1) / np.sqrt(bc2))
        bc1 = np.float64(1.0) - np.power(np.float64(beta1), np.float64(t))
        bc2 = np.float64(1.0) - np.power(np.float64(beta2), np.float64(t))
        return F(np.float64(F(lr)) / bc1), F(np.float64(1.0) / np.sqrt(bc2))


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate(p, g, m, v, t, lr, beta1, beta2, eps, wd, fast=False, mutate=None, contract=False):
    """adam_elem_form<fast> over float32 arrays -> dict(p, m, v).  contract: d1 + eps and p - w as one fma each, what a
    compiler may make of the written expressions."""
    assert mutate is None or mutate in MUTATIONS, mutate
    F = np.float32
    p0, m0, v0 = (np.asarray(x, F) for x in (p, m, v))
    lrb, isb = host_scalars(t, lr, beta1, beta2, mutate)
    b1, b2, omb1, omb2, eps, wd = F(beta1), F(beta2), F(1.0 - beta1), F(1.0 - beta2), F(eps), F(wd)
    with np.errstate(all='ignore'):
        if g is None:
            g1 = np.zeros_like(p0) if mutate == 'drop_wd_null' else _fma(wd, p0, np.zeros_like(p0))
        else:
            g1 = _fma(wd, p0, np.asarray(g, F))
        m1 = _fma(b2 if mutate == 'beta2_for_m' else b1, m0, omb1 * g1)
        v1 = _fma(b2, v0, (omb2 * g1) * g1)
        root = v1 + eps if mutate == 'eps_in_sqrt' else v1
        s = np.sqrt(root)
        if fast:
            s = np.where(root < F(TINY), F(0), s)
        if mutate == 'eps_in_sqrt':
            dn = s * isb
        else:
            dn = _fma(s, isb, eps) if contract else s * isb + eps
        q = m1 * (F(1) / dn) if fast else m1 / dn
        p1 = _fma(-lrb, q, p0) if contract else p0 - lrb * q
    out = dict(p=p1.astype(F), m=m1.astype(F), v=v1.astype(F))
    if mutate == 'tail_unwritten':
        tail = p0.size % 4
        if tail:
            for name, old in (('p', p0), ('m', m0), ('v', v0)):
                out[name][-tail:] = old[-tail:]
    return out


def sequential_sum(gathered):
    """[world, numel] float32 -> the float32 sum in rank order, as adam_gathered_kernel adds the ranks' buffers."""
    acc = np.array(gathered[0], np.float32)
    for w in range(1, gathered.shape[0]):
        acc = (acc + gathered[w]).astype(np.float32)
    return acc


def fragile(t, lr, beta1, beta2):
    """True where the float32 rounding of either scalar changes when its float64 value moves by a relative 2^-48: two
    correct double pows may then legitimately round to different floats."""
    for x in ref_scalars(t, lr, beta1, beta2):
        if np.float32(x * (1.0 + 2.0 ** -48)) != np.float32(x * (1.0 - 2.0 ** -48)):
            return True
    return False


# ===================================================================================================== cases and inputs
REGIMES = 16


def adam_state(n, seed, wd=DEFAULTS['wd']):
    """(p, g, m, v): n float32 elements mixing, by index mod 16, the regimes a table element can be in.
      0-7  ordinary: p ~ 0.1, m ~ 0.05, v ~ g^2 (the last n % 4 elements are ordinary too, whatever their index)
      8    a row no rating ever named, long into training: g = 0, m ~ wd p, sqrt(v) between 0.1 and 3 eps
      9    first step: m = v = 0, an ordinary gradient          10   first step of a never-named row: g = m = v = 0
      11   v (and v') in the denormal range: p = 0, |g| ~ 1e-20, v < 2^-126, m ~ 1e-21
      12   p = 0, the rest ordinary
      13   |g| from 1e12 to 1e18, m and v to scale (every fourth one: v = 0)
      14   |g| from 1e-20 to 1e-12, m and v to scale (v = g^2 reaches the denormals)
      15   a never-named row in its steady state: g = 0, m = wd p, v = (wd p)^2, so that sqrt(v) ~ eps"""
    rng = np.random.default_rng(seed)
    F = np.float64
    p = 0.1 * rng.standard_normal(n)
    g = 0.3 * rng.standard_normal(n)
    m = 0.05 * rng.standard_normal(n)
    v = g * g * (0.5 + rng.random(n))
    r = np.arange(n) % REGIMES
    r[n - (n % 4):] = 0
    u1, u2, z = rng.random(n), rng.random(n), rng.standard_normal(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    wdp = (wd if wd else 1e-6) * p

    def put(k, **kw):
        sel = r == k
        for name, val in kw.items():
            arr = dict(p=p, g=g, m=m, v=v)[name]
            arr[sel] = (val[sel] if isinstance(val, np.ndarray) else val)

    put(8, g=0.0, m=wdp * (0.5 + u1), v=(1e-8 * (0.1 + 2.9 * u2)) ** 2)
    put(9, m=0.0, v=0.0)
    put(10, g=0.0, m=0.0, v=0.0)
    put(11, p=0.0, g=sign * 1e-20 * (1.0 + u1), v=u2 * 2.0 ** -128, m=1e-21 * z)
    put(12, p=0.0)
    big = sign * 10.0 ** (12.0 + 6.0 * u1)
    put(13, g=big, m=0.05 * big * z, v=np.where(np.arange(n) % (4 * REGIMES) == 13, 0.0, big * big * (0.5 + u2)))
    small = sign * 10.0 ** (-20.0 + 8.0 * u1)
    put(14, g=small, m=0.05 * small * z, v=small * small * (0.5 + u2))
    put(15, g=0.0, m=wdp, v=wdp * wdp)
    return tuple(np.ascontiguousarray(x.astype(F).astype(np.float32)) for x in (p, g, m, v))


STEP_COUNTS = [1, 2, 3, 7, 8, 9, 10, 100, 693, 1000, 6931, 7100, 100000, 745000, 10 ** 7, 2 ** 31 + 1]
BETAS_ALT = dict(DEFAULTS, beta1=0.8, beta2=0.99, eps=1e-6)
STATE_N = 4099


def _case(name, t, hp, g_null=False, n=STATE_N, seed=0):
    return dict(name=name, t=t, hp=dict(hp), g_null=g_null, n=n, seed=seed)


# (a) / (b): one step from an arbitrary state -- the defaults at every step count; wd = 0, the second beta pair and a
# null gradient at step counts before, at and beyond the corrections' fade
STEP_CASES = ([_case('t%d' % t, t, DEFAULTS, seed=i) for i, t in enumerate(STEP_COUNTS)]
              + [_case('wd0-t%d' % t, t, dict(DEFAULTS, wd=0.0), seed=20 + i) for i, t in enumerate((1, 1000, 10 ** 7))]
              + [_case('betas-t%d' % t, t, BETAS_ALT, seed=30 + i) for i, t in enumerate((1, 8, 693, 1000, 10 ** 7))]
              + [_case('gnull-t%d' % t, t, DEFAULTS, g_null=True, seed=40 + i) for i, t in enumerate((1, 9, 7100))])


def case_inputs(case):
    """(p, g or None, m, v) of a case."""
    p, g, m, v = adam_state(case['n'], case['seed'], case['hp']['wd'])
    return p, (None if case['g_null'] else g), m, v


def case_id(case):
    return case['name']


# (b) consecutive steps
CONSEC_N, CONSEC_STEPS = 1028, 2048
BETA_PAIRS = [(0.9, 0.999), (0.8, 0.99)]

# (c) placement
NEIGHBOUR_NUMELS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2047, 2049]
LIST_LAYOUTS = [(pos, n) for n in (1, 15, 16, 17, 32, 33) for pos in (1, 16, 17, 33) if pos <= n]
PLACEMENT_CASE = _case('placement', 1000, DEFAULTS, seed=50)
FOUR_MI = 4 << 20
BIG_LIST = [511 * 8192, 8191, 8193, 1, 0, 7, STATE_N]                 # 4,206,603 elements: the 8,192-element chunk
UNDER_LIST = [FOUR_MI - 1 - (8191 + 8193 + 1 + 0 + 7 + STATE_N), 8191, 8193, 1, 0, 7, STATE_N]   # 4 Mi - 1: the 1,024 one


def list_layout(pos, n):
    """numel of each tensor of an n-tensor list whose pos-th (1-based) tensor is the 4,099-element one, and which of them
    have a null gradient: neighbours cycle through NEIGHBOUR_NUMELS, with zero-length tensors first, in the middle and
    last wherever the 4,099-element tensor is not."""
    numel = [NEIGHBOUR_NUMELS[(3 + 7 * k) % len(NEIGHBOUR_NUMELS)] for k in range(n)]
    for k in (0, n // 2, n - 1):
        numel[k] = 0
    numel[pos - 1] = STATE_N
    g_null = [k % 5 == 2 and k != pos - 1 for k in range(n)]
    return numel, g_null


# (d) the data-parallel form
GATHERED_WORLDS = [1, 2, 3, 16]
GATHERED_NUMELS = [0, 4, 1020, 1024, 1028]
GATHERED_STEPS = [1, 1000, 10 ** 7]


def gathered_inputs(world, numel, t):
    """(p, gathered [world, numel], m, v): the state of adam_state with its gradient dealt over `world` ranks in unequal
    shares (the ranks' sum is not exact in float32: the order shows)."""
    p, g, m, v = adam_state(numel, 1000 * world + numel + t % 97)
    rng = np.random.default_rng(7 * world + numel)
    share = rng.random((world, numel)) + 0.1
    share /= share.sum(0, keepdims=True)
    return p, np.ascontiguousarray((share * g[None, :].astype(np.float64)).astype(np.float32)), m, v


# (e) the fast form through r4r_rows_apply_large
ROWS_NAMED, ROWS_TOTAL, ROWS_PAD = 1500, 1600, 77
ROWS_WIDTHS = [1, 5, 33, 64]
ROWS_STEPS = [1, 8, 1000, 7100, 10 ** 7]


def rows_inputs(W, t):
    """A [1600, W] table and a 1600-element bias vector in the states of adam_state, and 1,577 entries: a permutation
    of 1,500 of the rows, each named once, with 77 padding entries (-1) among them.  -> dict."""
    seed = 100 * W + t % 89
    p, g, m, v = (x.reshape(ROWS_TOTAL, W) for x in adam_state(ROWS_TOTAL * W, seed))
    bp, bg, bm, bv = adam_state(ROWS_TOTAL, seed + 1)
    rng = np.random.default_rng(seed + 2)
    named = rng.permutation(ROWS_TOTAL)[:ROWS_NAMED]
    ids = np.full(ROWS_NAMED + ROWS_PAD, -1, np.int64)
    slots = np.sort(rng.permutation(ids.size)[:ROWS_NAMED])
    ids[slots] = named
    grads = rng.standard_normal((ids.size, W)).astype(np.float32)       # padding entries carry garbage that must not land
    gbias = rng.standard_normal(ids.size).astype(np.float32)
    grads[slots] = g[named]
    gbias[slots] = bg[named]
    return dict(p=p, m=m, v=v, bp=bp, bm=bm, bv=bv, ids=ids, grads=grads, gbias=gbias, named=np.sort(named),
                g_rows=g, g_bias=bg)


# (f) the Python Adam class
CLASS_SIZES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1000, 1023, 1024,
               1025, 1027, 1028, 1029, 1500, 2000, 2044, 2045, 2046, 2047, 2048, 2049, 6, 9, 100]
CLASS_STEPS = 12


def class_has_grad(i, step):
    """Whether parameter i has a gradient at step 0 .. 11: three groups that end at three different step counts."""
    if i % 3 == 1:
        return step not in (3, 7)
    if i % 3 == 2:
        return step >= 5
    return True


def class_grad(i, step, n):
    return (0.3 * np.random.default_rng(10000 + 100 * i + step).standard_normal(n)).astype(np.float32)


def class_param(i, n):
    return (0.1 * np.random.default_rng(500 + i).standard_normal(n)).astype(np.float32)
