"""Float64 restatements of the op-by-op head ops (csrc/smallops.hip, csrc/narre.hip, reviews4rec_amd/ops.py) and
per-element checkers of what the kernels return for them.  No kernel of the project and no GPU code lives here.

The rule, for every output element:   |kernel - float64| <= c * 2^-24 * M
  M  the same expression evaluated in float64 with every term replaced by its absolute value;
  c  the number of fp32 roundings on the longest path to that element, counted for an ARBITRARY summation order, so
     that the checker does not encode the kernel's: a product is 1, an n-term sum of products (a dot) is n (one product
     and n - 1 additions), every further +, -, * is 1.  Each c is written next to its derivation below.
Quantities that feed a non-linearity or a second product carry their own bound forward to first order (`d...` names):
a gradient through a recomputed s_k inherits s_k's bound times |V_ik|, softmax weights inherit 2 max d(score) plus the
expf and division roundings.  No fixed rtol / atol, no fraction of elements left out: NaN and inf fail, and an element
whose M is 0 (an untouched row, a masked unit) must be exactly 0.

ReLU: a mask is only comparable where fp32 and float64 must agree on the sign, so every reference asserts, before
anything is compared, that each pre-activation lies outside its own bound of zero or is zero by construction (M == 0:
every term is an exact zero, e.g. an all-zero row with a zero bias; the mask is then off on both sides)."""
import numpy as np
import torch

U32 = 2.0 ** -24                 # unit roundoff of fp32
TINY = 2.0 ** -126               # smallest normal fp32: what a flushed (or subnormal) expf result can be off by
C_EXPF = 4                       # expf: within 2 ulp = 4 units of 2^-24 (the device's and the host's libm both claim <= 2 ulp)


def d64(t):
    return t.detach().to('cpu', torch.float64)


class Ref(dict):
    """name -> (float64 value, float64 per-element bound); .aux holds intermediates the host tests build mutants from."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.aux = {}


def compare(what, got, val, bound):
    """Asserts |got - val| <= bound for EVERY element (NaN fails) and returns the worst error / bound (0 / 0 = 0)."""
    got = d64(got)
    val, bound = torch.as_tensor(val, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    assert got.numel() == val.numel(), '%s: %d elements, expected %d' % (what, got.numel(), val.numel())
    got, bound = got.reshape(val.shape), bound.expand(val.shape)
    err = (got - val).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError('%s: %d of %d elements beyond their bound, e.g. at %s got %.9g, float64 %.9g, error %.3g, '
                             'bound %.3g' % (what, bad.shape[0], val.numel(), i, float(got[i]), float(val[i]),
                                             float(err[i]), float(bound[i])))
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def compare_all(what, got, ref, names=None, each=None):
    """got: name -> tensor.  Checks every name of `names` (default: every name of ref) and returns the worst ratio;
    `each` (a dict) receives the ratio of every name."""
    worst = 0.0
    for name in (names or list(ref)):
        val, bound = ref[name]
        ratio = compare('%s %s' % (what, name), got[name], val, bound)
        if each is not None:
            each[name] = ratio
        worst = max(worst, ratio)
    return worst


def assert_relu_margin(what, pre, dpre, M):
    """Every pre-activation is outside its bound of zero, or an exact zero by construction (M == 0)."""
    bad = ~((pre.abs() > dpre) | (M == 0))
    assert not bool(bad.any()), ('%s: %d pre-activations within their rounding bound of zero (smallest |pre| / bound '
                                 '%.3g): the ReLU mask is not comparable; change the seed' %
                                 (what, int(bad.sum()), float((pre.abs() / dpre.clamp(min=1e-300))[bad].min())))


def bits_equal(a, b):
    """Bit equality of two fp32 arrays / tensors (distinguishes -0 from +0)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, (a.dtype, b.dtype)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


# ------------------------------------------------------------------------------------------------------------ linear
def linear_ref(x, w, b, gy, relu):
    """y = act(x w^T + b) over the last dimension of x, and the gradients of <gy, y>.
      y    c = n_in + 1          n_in-term dot, + bias                        M = |x| |w|^T + |b|
      g_x  c = n_out             n_out-term dot of geff (exact: gy or 0) and w M = |geff| |w|
      g_w  c = N + 1             N-term dot over the rows, + 1 for the add of split partials counted apart
      g_b  c = N + 1             N-term sum (the kernel's g * 1), same allowance M = sum |geff|"""
    x, w, b, gy = d64(x), d64(w), d64(b), d64(gy)
    n_in, n_out = w.shape[1], w.shape[0]
    x2, gy = x.reshape(-1, n_in), gy.reshape(-1, n_out)
    N = x2.shape[0]
    pre = x2 @ w.T + b
    M = x2.abs() @ w.abs().T + b.abs()
    dpre = (n_in + 1) * U32 * M
    on = torch.ones_like(pre, dtype=torch.bool)
    if relu:
        assert_relu_margin('linear', pre, dpre, M)
        on = pre > 0
    zero = torch.zeros_like(pre)
    geff = torch.where(on, gy, zero)
    ref = Ref(y=(torch.where(on, pre, zero).reshape(*x.shape[:-1], n_out), torch.where(on, dpre, zero).reshape(*x.shape[:-1], n_out)),
              g_x=((geff @ w).reshape(x.shape), (n_out * U32 * (geff.abs() @ w.abs())).reshape(x.shape)),
              g_w=(geff.T @ x2, (N + 1) * U32 * (geff.abs().T @ x2.abs())),
              g_b=(geff.sum(0), (N + 1) * U32 * geff.abs().sum(0)))
    ref.aux = dict(geff=geff, x2=x2, on=on)
    return ref


def linear_splits(N):
    """(number of splits, rows per split) of linear_bwd_w_kernel: clamp(N / 64, 1, 32), cdiv(N, ns)."""
    ns = min(max(N // 64, 1), 32)
    return ns, -(-max(N, 1) // ns)


# ---------------------------------------------------------------------------------------------------------------- FM
def fm_ref(x, V, lw, lb, go):
    """out_b = 0.5 sum_k (s_bk^2 - s2_bk) + x_b . lw + lb,  s = x V, s2 = x^2 V^2; with A = |x| |V|, Q = x^2 V^2:
      out      c = 2n + k + 4   s_k: n; s_k^2: 2n + 1; - s2: + 1; k-term sum: + k; + lin, + lb: + 2 (the 0.5 is exact)
                                M = 0.5 sum_k (A_k^2 + Q_k) + |x| . |lw| + |lb|
      g_x      c = n + k + 4    s_k V_ik: n + 1 (s_k's bound times |V_ik|); - x V^2: + 1; k-term sum: + k; + lw: 1; * g: 1
                                M = |g| (sum_k (A_k |V_ik| + |x_i| V_ik^2) + |lw_i|)
      g_V      c = n + N + 3    s_bk x_bi: n + 1; - x^2 V: + 1; * g: + 1; N-term sum over the examples: + N
                                M = sum_b |g_b| (A_bk |x_bi| + x_bi^2 |V_ik|)
      g_lin_w  c = N            N-term dot                                  M = sum_b |g_b| |x_bi|
      g_lin_b  c = N            N-term sum                                  M = sum_b |g_b|"""
    x, V, lw_, lb, go = d64(x), d64(V), d64(lw), d64(lb).reshape(()), d64(go)
    lwv = lw_.reshape(-1)
    N, n = x.shape
    k = V.shape[1]
    s, A = x @ V, x.abs() @ V.abs()
    Q = (x * x) @ (V * V)
    v2 = (V * V).sum(1)
    g1, ga = go[:, None], go.abs()[:, None]
    out = 0.5 * (s * s - Q).sum(1) + x @ lwv + lb
    Mout = 0.5 * (A * A + Q).sum(1) + x.abs() @ lwv.abs() + lb.abs()
    gx = g1 * (s @ V.T - x * v2 + lwv)
    Mgx = ga * (A @ V.abs().T + x.abs() * v2 + lwv.abs())
    gV = x.T @ (g1 * s) - (g1 * x * x).sum(0)[:, None] * V
    MgV = x.abs().T @ (ga * A) + (ga * x * x).sum(0)[:, None] * V.abs()
    ref = Ref(out=(out, (2 * n + k + 4) * U32 * Mout),
              g_x=(gx, (n + k + 4) * U32 * Mgx),
              g_V=(gV, (n + N + 3) * U32 * MgV),
              g_lin_w=((go @ x).reshape(lw_.shape), (N * U32 * (go.abs() @ x.abs())).reshape(lw_.shape)),
              g_lin_b=(go.sum().reshape(1), (N * U32 * go.abs().sum()).reshape(1)))
    ref.aux = dict(x=x, V=V, lw=lwv, lb=lb, go=go)
    return ref


# ------------------------------------------------------------------------------------------- rowdot, bias head, embed
def rowdot_ref(a, c, go):
    """out_b = a_b . c_b: c = D (D-term dot), M = |a| . |c|;  g_a = g c, g_c = g a: c = 1 (one product)."""
    a, c, go = d64(a), d64(c), d64(go)
    D = a.shape[1]
    g1 = go[:, None]
    return Ref(out=((a * c).sum(1), D * U32 * (a.abs() * c.abs()).sum(1)),
               g_a=(g1 * c, U32 * (g1 * c).abs()), g_c=(g1 * a, U32 * (g1 * a).abs()))


def multiplicity_sum(idx, g, R):
    """Dense [R, D] sum of the rows g[e] at idx[e] >= 0 and its bound: c = the row's multiplicity m (an m-term sum in
    any order -- the atomic scatter's -- counts m), M = sum |g|.  Rows nobody names have M = 0: exact zeros."""
    idx = idx.detach().cpu().reshape(-1)
    g = d64(g).reshape(idx.numel(), -1)
    keep = idx >= 0
    D = g.shape[1]
    val = torch.zeros((R, D), dtype=torch.float64).index_add_(0, idx[keep], g[keep])
    M = torch.zeros((R, D), dtype=torch.float64).index_add_(0, idx[keep], g[keep].abs())
    m = torch.bincount(idx[keep], minlength=R).to(torch.float64)[:, None]
    return val, m * U32 * M


def bias_head_ref(r, ub, ib, gb, uid, iid, go):
    """out = ((r + ub[uid]) + ib[iid]) + gb, any of r / (ub, ib) may be None:
      out       c = number of additions (3, 2 with ids only, 1 with r only)   M = |r| + |ub| + |ib| + |gb|
      g_global  c = N (N-term sum)                                            M = sum |g|
      g_user_bias / g_item_bias: multiplicity_sum;  g_r is the incoming gradient itself (checked bit for bit)."""
    go = d64(go)
    N = go.numel()
    out = torch.zeros(N, dtype=torch.float64)
    M = torch.zeros(N, dtype=torch.float64)
    c = 0
    for t, i in ((r, None), (ub, uid), (ib, iid)):
        if t is not None:
            v = d64(t).reshape(-1)
            v = v if i is None else v[i.cpu().reshape(-1)]
            out, M, c = out + v, M + v.abs(), c + 1
    out, M = out + d64(gb).reshape(()), M + d64(gb).abs().reshape(())
    ref = Ref(out=(out, c * U32 * M), g_global=(go.sum().reshape(1), (N * U32 * go.abs().sum()).reshape(1)))
    if ub is not None:
        for name, t, i in (('g_user_bias', ub, uid), ('g_item_bias', ib, iid)):
            val, bound = multiplicity_sum(i, go.reshape(-1, 1), t.numel())
            ref[name] = (val.reshape(-1), bound.reshape(-1))
    return ref


def ordered_scatter_np(idx, g, R, descending=False):
    """The ordered scatter's contract as a numpy float32 loop: row idx[e] gets g[e] for its first entry, then each
    later duplicate added in ascending entry order; idx < 0 is padding.  descending=True is the wrong order (a mutant)."""
    idx = np.asarray(idx).reshape(-1)
    g = np.asarray(g, dtype=np.float32).reshape(idx.size, -1)
    out = np.zeros((R, g.shape[1]), dtype=np.float32)
    seen = set()
    for e in (range(idx.size - 1, -1, -1) if descending else range(idx.size)):
        row = int(idx[e])
        if row < 0:
            continue
        out[row] = g[e] if row not in seen else (out[row] + g[e]).astype(np.float32)
        seen.add(row)
    return out


# ------------------------------------------------------------------------------------------------------------ losses
def transform_loss_ref(a, b, gup):
    """out = (1/N) sum_{n,l} (a - b)^2:
      out        c = N L + 5   a - b: 1; squared: 2 + 1; (N L)-term sum: + N L; 1/N rounded: 1; the product with it: 1
                               M = (1/N) sum (|a| + |b|)^2
      g_a, g_b   c = 4         1/N: 1; gup * 2 * (1/N): 1 (the 2 is exact); a - b: 1; the product: 1
                               M = |gup| (2/N) (|a| + |b|);   g_b = -g_a exactly (checked by bits)."""
    a, b = d64(a), d64(b)
    gup = float(gup)
    N, L = a.shape
    S = a.abs() + b.abs()
    ga = gup * 2.0 / N * (a - b)
    bound = 4 * U32 * abs(gup) * 2.0 / N * S
    return Ref(out=(((a - b) ** 2).sum() / N, (N * L + 5) * U32 * (S * S).sum() / N), g_a=(ga, bound), g_b=(-ga, bound))


def mse_ref(out, y, denom):
    """se = (out - y)^2: c = 3 (the difference: 1, squared: 2 + 1), M = (|out| + |y|)^2;
    g = 2 (out - y) / denom: c = 3 (1 / denom: 1, the difference: 1, the product: 1), M = 2 (|out| + |y|) / denom."""
    out, y = d64(out).reshape(-1), d64(y).reshape(-1)
    S = out.abs() + y.abs()
    return Ref(se=((out - y) ** 2, 3 * U32 * S * S), g=(2 * (out - y) / denom, 3 * U32 * 2 * S / denom))


# --------------------------------------------------------------------------------------------------- NARRE attention
def attn_splits(rows):
    """(number of splits, rows per split) of narre_attn_bwd_p_kernel: clamp(rows / 128, 1, 64), cdiv(rows, ns)."""
    ns = min(max(rows // 128, 1), 64)
    return ns, -(-max(rows, 1) // ns)


def attention_ref(x, other, W0, b0, w3, b3, mult, go):
    """NARRE's review attention, forward and backward, with the scorer's dropout multiplier `mult` ([N, R, L] or None)
    applied in both.  cat = [x, other]; rows = N R.  Every d... below is a bound carried forward to first order.
      pre   = cat W0^T + b0              c = 2L + 1   (2L-term dot, + bias)                M = |cat| |W0|^T + |b0|
      h     = relu(pre) mult             c = 2L + 2   (+ the product)                      (h_save; exactly 0 where off)
      sc    = h . w3 + b3                dsc = dh . |w3| + (L + 1) 2^-24 (|h| . |w3| + |b3|)
      a     = softmax_r(sc)              relative: expm1(2 rho + (R + 1) 2^-24), rho = max_r dsc + 2^-24 spread(sc)
                                         + C_EXPF 2^-24 (sc - max rounded, then expf), the R-term denominator R and the
                                         division 1; + 2 TINY absolute for an exp that underflows      (a_save)
      out   = sum_r a_r x_r              dout = da . |x| + R 2^-24 a . |x|
      ga_r  = g_out . x_r                c = L
      dot   = sum_r a_r ga_r             ddot = da . |ga| + a . dga + R 2^-24 a . Mga
      g_sc  = a (ga - dot)               dg_sc = da |ga - dot| + a (dga + ddot) + 2 2^-24 a (|ga| + |dot|)
      g_pre = g_sc w3 mult [pre > 0]     dg_pre = (dg_sc + 2 2^-24 |g_sc|) |w3| mult
      g_cat = g_pre W0                   dg_cat = dg_pre |W0| + L 2^-24 |g_pre| |W0|
      g_x   = g_cat[:L] + a g_out        + da |g_out| + 2 2^-24 (|g_pre| |W0| + a |g_out|);    g_other = g_cat[L:]
      g_W0  = g_pre^T cat, g_b0 = sum g_pre, g_w3 = g_sc^T h, g_b3 = sum g_sc (true value 0, M = sum |g_sc|):
              rows-term sums in any order, + 1 for the add of split partials: c = rows + 1, plus the inherited
              dg_pre |cat|, dg_pre, dg_sc |h| + |g_sc| dh, dg_sc."""
    x, other, W0, b0, b3, go = d64(x), d64(other), d64(W0), d64(b0), d64(b3).reshape(()), d64(go)
    w3v = d64(w3).reshape(-1)
    N, R, L = x.shape
    rows = N * R
    m = torch.ones_like(x) if mult is None else d64(mult)
    zero = torch.zeros_like(x)
    cat = torch.cat([x, other], -1)
    pre = cat @ W0.T + b0
    Mpre = cat.abs() @ W0.abs().T + b0.abs()
    assert_relu_margin('attention scorer', pre, (2 * L + 1) * U32 * Mpre, Mpre)
    on = pre > 0
    h = torch.where(on, pre, zero) * m
    dh = torch.where(on, (2 * L + 2) * U32 * Mpre, zero) * m
    sc = h @ w3v + b3
    dsc = dh @ w3v.abs() + (L + 1) * U32 * (h.abs() @ w3v.abs() + b3.abs())
    a = torch.softmax(sc, dim=1)
    spread = sc.max(1).values - sc.min(1).values + 2 * dsc.max(1).values
    rho = dsc.max(1).values + U32 * spread + C_EXPF * U32
    da = a * torch.expm1(2 * rho + (R + 1) * U32)[:, None] + 2 * TINY
    out = torch.einsum('nr,nrl->nl', a, x)
    dout = torch.einsum('nr,nrl->nl', da, x.abs()) + R * U32 * torch.einsum('nr,nrl->nl', a, x.abs())
    # backward
    ga = torch.einsum('nl,nrl->nr', go, x)
    Mga = torch.einsum('nl,nrl->nr', go.abs(), x.abs())
    dga = L * U32 * Mga
    dot = (a * ga).sum(1, keepdim=True)
    ddot = (da * ga.abs() + a * dga).sum(1, keepdim=True) + R * U32 * (a * Mga).sum(1, keepdim=True)
    gsc = a * (ga - dot)
    dgsc = da * (ga - dot).abs() + a * (dga + ddot) + 2 * U32 * a * (ga.abs() + dot.abs())
    gpre = torch.where(on, gsc[..., None] * w3v * m, zero)
    dgpre = torch.where(on, (dgsc + 2 * U32 * gsc.abs())[..., None] * w3v.abs() * m, zero)
    Mgcat = gpre.abs() @ W0.abs()
    gcat = gpre @ W0
    dgcat = dgpre @ W0.abs() + L * U32 * Mgcat
    ago = a[..., None] * go[:, None, :]
    g_x = gcat[..., :L] + ago
    dg_x = dgcat[..., :L] + da[..., None] * go.abs()[:, None, :] + 2 * U32 * (Mgcat[..., :L] + ago.abs())
    G, dG, C = gpre.reshape(rows, L), dgpre.reshape(rows, L), cat.reshape(rows, 2 * L)
    H, dH, S, dS = h.reshape(rows, L), dh.reshape(rows, L), gsc.reshape(rows), dgsc.reshape(rows)
    cs = (rows + 1) * U32
    ref = Ref(out=(out, dout), h_save=(h, dh), a_save=(a, da), g_x=(g_x, dg_x), g_other=(gcat[..., L:], dgcat[..., L:]),
              g_W0=(G.T @ C, dG.T @ C.abs() + cs * (G.abs().T @ C.abs())),
              g_b0=(G.sum(0), dG.sum(0) + cs * G.abs().sum(0)),
              g_w3=((S @ H).reshape(w3.shape), (dS @ H.abs() + S.abs() @ dH + cs * (S.abs() @ H.abs())).reshape(w3.shape)),
              g_b3=(S.sum().reshape(1), (dS.sum() + cs * S.abs().sum()).reshape(1)))
    ref.aux = dict(G=G, C=C, H=H, S=S, sc=sc, a=a, on=on, pre=pre)
    return ref


# ===================================================================================================== cases and inputs
# Seeded inputs of every case, shared by tests/test_head_ref.py (CPU: the fp32 reference alone, the mutants, the ReLU
# margins) and tests/test_gpu_head_ops.py (the kernels).  Gaussian scale as in tests/test_gpu_kernels.py.
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# (N, n_in, n_out) or (lead shape, n_in, n_out).  What each one is aimed at:
LINEAR_CASES = [
    (1, 1, 1),                  # one thread of one wave does everything; red[] holds LB_ROWS x 2 floats
    (3, 63, 2),                 # n_in + 1 = 64: the bias column is the last lane of the only wave, tx = 64
    (3, 64, 2),                 # n_in + 1 = 65: a second wave holds the bias column alone, tx = 128
    (5, 255, 3),                # the widest layer: tx = 256, a 1024-thread workgroup
    (51, 7, 5), (64, 7, 4), (257, 7, 1),   # N n_out = 255 / 256 / 257: `if (i >= N * n_out) return` of linear_fwd_kernel
    (127, 20, 10),              # N / 64 = 1: one split, `part == NULL`, the direct store
    (128, 20, 10),              # two even splits of 64
    (129, 20, 10),              # two splits of cdiv = 65: the last one is ragged (64 rows), r1 = min(N, ...)
    (191, 20, 10),              # two splits of 96 and 95; 95 is no multiple of LB_ROWS
    (2047, 20, 10),             # 31 splits of 67, the last 37 rows
    (2048, 20, 10),             # 32 even splits: the cap reached exactly
    (2049, 20, 10),             # 32 splits of 65, the last 34 rows
    (2111, 20, 10),             # N / 64 = 32.98: 32 splits of 66, the last 65
    (4100, 20, 10),             # N / 64 = 64 clamped to 32: 129 rows per split, the last 101
    ((13, 10), 20, 10),         # leading dimensions [N, R, n_in], N R = 130: ops.Linear's reshape / view, two splits
]
FM_CASES = [
    (1, 1, 1),                  # k = 1, one live lane
    (3, 63, 2), (4, 64, 3),     # the last lane idle / live: still one slot per lane (`64 * t < n` false for t = 1)
    (5, 65, 3),                 # slot 1 holds exactly one input (lane 0); fm_bwd_p's second block of 64 has one live lane
    (2, 128, 5), (3, 129, 4),   # two full slots / a third with one input
    (6, 448, 2), (2, 449, 3),   # seven full slots / the eighth (FM_MAX_SLOTS) with one input
    (3, 512, 70),               # all eight slots full, k > 64
    (2, 8, 300),                # many kk columns on few inputs: fm_bwd_p's grid.x = k + 1
    (1, 65, 3), (3, 65, 3), (4, 65, 3), (9, 65, 3),   # with (5, 65, 3): fm_bwd_p's 4 row groups -- one used, three, all, ragged
]
ROWDOT_CASES = [(1, 1), (4, 63), (5, 64), (3, 65), (7, 200)]      # the `d += 64` loop of rowdot_fwd_kernel: 0, 1, 1, 2, 4 trips
BIAS_NS = [1, 255, 256, 257, 1000]      # sum_kernel strides by 256: the loop runs once, once (last thread idle), once, twice, four times
EMBED_CASES = [(1, 1), (12, 64), (64, 65), (65, 3), (130, 600)]   # (D, n): n D around the 256-thread blocks of the gather
ORDERED_DS = [1, 64, 65, 130]           # `d0 += 64`: one trip with one lane, one full trip, two, three
ORDERED_NS = [1, 64, 65, 600]           # the 64-strided duplicate search `k += 64` runs 0 / 1 / 2 / 10 times
TLOSS_CASES = [(1, 1), (5, 51), (16, 16), (257, 1), (70, 100)]    # N L = 1, 255, 256, 257, 7000: sqdist_mean_fwd's 256 stride
MSE_NS = [1, 256, 257]
ELEMENTWISE_NS = [255, 256, 257]

# name -> (N, R, L, kind).  rows = N R against attn_splits: clamp(rows / 128, 1, 64) splits of cdiv rows each.
ATTN_CASES = {
    'one':        (1, 1, 1, 'plain'),       # a single thread; softmax over one review is exactly 1
    'one_review': (2, 1, 7, 'plain'),       # R = 1: the r loops run once
    'one_unit':   (3, 32, 1, 'plain'),      # L = 1: blockDim = (1, 32), hs[r][0] only
    'full':       (2, 32, 32, 'plain'),     # MAXR x MAXL: a 1024-thread workgroup
    'rows130':    (13, 10, 10, 'plain'),    # one split of 130 rows
    'rows260':    (26, 10, 10, 'plain'),    # two even splits of 130
    'rows8200':   (820, 10, 10, 'ragged'),  # 64 splits of 129, the last one ragged (73 rows)
    'rows9000':   (900, 10, 10, 'ragged'),  # rows / 128 = 70 clamped to 64: 141 rows per split, the last 117
    'big_scores': (4, 10, 10, 'big'),       # scores up to about +-96: expf(sc - m) with m subtracted, exp underflow
    'identical':  (5, 10, 10, 'identical'),  # every review of an example the same: weights 1 / R
    'padded':     (6, 10, 10, 'padded'),    # trailing all-zero reviews: not masked, they still receive weight
}
# name -> seed where seed 0 will not do: its last review has an attention weight of 3e-4 (rows8200 under dropout), so a
# lost last row would vanish inside the rows + 1 bound; at these seeds the ReLU margin holds and the last row's own
# contribution to g_W0 and g_w3 is above 5 times their bounds, with and without dropout
ATTN_SEEDS = {'rows8200': 2, 'rows9000': 4}


def linear_inputs(case, seed=None):
    shape, n_in, n_out = case
    lead = shape if isinstance(shape, tuple) else (shape,)
    seed = LINEAR_SEEDS.get(case, 0) if seed is None else seed
    g = _gen(1, *lead, n_in, n_out, seed)
    x = torch.randn(lead + (n_in,), generator=g)
    w = torch.randn((n_out, n_in), generator=g) * 0.1
    b = torch.randn(n_out, generator=g)
    gy = torch.randn(lead + (n_out,), generator=g)
    return x, w, b, gy


# case -> seed where seed 0 will not do: its bias of the single output of (257, 7, 1) is so negative that the ReLU is off
# for every row, and no defect of the weight gradient could show
LINEAR_SEEDS = {(257, 7, 1): 1}


def linear_zero_inputs():
    """Exact-zero pre-activations: zero bias, rows 1 and 4 all +0, row 2 all -0 (every product is a signed zero and
    the sum is 0: M == 0); the other rows are Gaussian.  The mask must be off for rows 1, 2, 4 forward and backward."""
    x, w, b, gy = linear_inputs((6, 20, 10), seed=1)
    x[1] = 0.0
    x[4] = 0.0
    x[2] = -0.0
    return x, w, torch.zeros_like(b), gy


def fm_inputs(case):
    N, n, k = case
    g = _gen(2, N, n, k)
    V = torch.randn((n, k), generator=g) * 0.3
    lw = torch.randn((1, n), generator=g) * 0.3
    lb = torch.randn(1, generator=g)
    x = torch.randn((N, n), generator=g)
    go = torch.randn(N, generator=g)
    return x, V, lw, lb, go


def rowdot_inputs(case):
    N, D = case
    g = _gen(3, N, D)
    return torch.randn((N, D), generator=g), torch.randn((N, D), generator=g), torch.randn(N, generator=g)


def bias_head_inputs(N, U):
    """U = I = 3: every row is named about N / 3 times (the atomic scatter's duplicates); U = I = 1: all N on one row."""
    g = _gen(4, N, U)
    r, ub, ib, gb = (torch.randn(s, generator=g) for s in (N, U, U, 1))
    uid, iid = torch.randint(0, U, (N,), generator=g), torch.randint(0, U, (N,), generator=g)
    return r, ub, ib, gb, uid, iid, torch.randn(N, generator=g)


EMBED_ROWS = 9


def embed_inputs(case):
    """Indices over rows 0..6 of a 9-row table (heavy duplication once n > 7), row 8 named last; row 7 is never named."""
    D, n = case
    g = _gen(5, D, n)
    table = torch.randn((EMBED_ROWS, D), generator=g)
    idx = torch.randint(0, 7, (n,), generator=g)
    idx[-1] = EMBED_ROWS - 1
    return table, idx, torch.randn((n, D), generator=g)


def ordered_inputs(D, n, layout):
    """A compact (row id, gradient row) list over a 9-row table.  'dups': rows 0..6 at random (about n / 7 duplicates
    each) and row R - 1 = 8 at entries 0, 63, 64, 65 and n - 1 (those that exist): its leader is entry 0, and its later
    duplicates sit at the end of the first 64-lane search stride, at the start of the second, one further and at the
    very end.  'lead' / 'trail': the same with the first / last five entries and every ninth one -1 (padding);
    'all': nothing but padding."""
    g = _gen(6, D, n)
    idx = torch.randint(0, 7, (n,), generator=g)
    for e in (0, 63, 64, 65, n - 1):
        if e < n:
            idx[e] = EMBED_ROWS - 1
    rows = torch.randn((n, D), generator=g)
    if layout == 'lead':
        idx[:5] = -1
        idx[7::9] = -1
    elif layout == 'trail':
        idx[-5:] = -1
        idx[7::9] = -1
    elif layout == 'all':
        idx[:] = -1
    else:
        assert layout == 'dups'
    return idx, rows


ORDERED_CASES = ([(D, n, 'dups') for D in ORDERED_DS for n in ORDERED_NS]
                 + [(65, 600, 'lead'), (65, 600, 'trail'), (130, 64, 'lead'), (1, 65, 'trail'),
                    (1, 1, 'all'), (65, 600, 'all')])


def tloss_inputs(case):
    N, L = case
    g = _gen(7, N, L)
    return torch.randn((N, L), generator=g), torch.randn((N, L), generator=g), 1.75      # (exact in fp32)


def vector_inputs(n, tag):
    g = _gen(8, n, tag)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def attention_inputs(name, dropout):
    """(x, other, W0, b0, w3, b3, mult, g_out) of a case; dropout=True adds a p = 0.5 multiplier (0 or 2)."""
    N, R, L, kind = ATTN_CASES[name]
    g = _gen(9, N, R, L, ATTN_SEEDS.get(name, 0), *[ord(ch) for ch in kind[:3]])
    W0 = torch.randn((L, 2 * L), generator=g) * 0.4
    b0 = torch.randn(L, generator=g) * 0.1
    w3 = torch.randn((1, L), generator=g) * 0.4
    b3 = torch.randn(1, generator=g)
    x = torch.randn((N, R, L), generator=g)
    o = torch.randn((N, R, L), generator=g)
    go = torch.randn((N, L), generator=g)
    mult = (torch.rand((N, R, L), generator=g) >= 0.5).float() * 2.0 if dropout else None
    if kind == 'identical':
        x, o = x[:, :1].expand(N, R, L).contiguous(), o[:, :1].expand(N, R, L).contiguous()
    elif kind == 'ragged':
        # the last example's upstream gradient is 16 times the others': with c = rows + 1 and M a sum over all rows the
        # bound of a parameter gradient is about 4 average terms at rows = 8200, so a lost AVERAGE last row would pass
        go[-1] *= 16.0
    elif kind == 'padded':
        for n in range(N):                                   # example n keeps n + 2 reviews, the rest is padding
            x[n, n + 2:] = 0.0
            o[n, n + 2:] = 0.0
    elif kind == 'big':
        # w3 rescaled (and its sign chosen) so that the largest score is about +96: above fp32 expf's overflow at 88.7,
        # so a softmax that forgets to subtract the maximum gives inf / inf
        W0 = W0 * 4.0
        h = torch.relu(torch.cat([x, o], -1).double() @ W0.double().T + b0.double())
        if mult is not None:
            h = h * mult.double()
        s = h @ w3.double().reshape(-1)
        top = s.flatten()[s.abs().argmax()]
        w3 = (w3.double() * (96.0 / top)).float()
    return x, o, W0, b0, w3, b3, mult, go
