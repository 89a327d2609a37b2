"""Float64 restatements of r4r_pair_grad's three head kinds (include/r4r.h, "Pair gradients"; csrc/pair_grad.hip) with
per-element bounds, a float32 numpy evaluation of the same closed forms in ANOTHER summation order (and its mutants),
and the seeded inputs the host and the GPU tests share.  No kernel of the project and no GPU code lives here.

The rule is tests/head_ref.py's, for every output element:   |kernel - float64| <= c * 2^-24 * M
  M  the same expression evaluated in float64 with every term replaced by its absolute value;
  c  the number of fp32 roundings on the longest path to that element, counted for an ARBITRARY summation order: a
     product is 1, an n-term sum of products (a dot) is n, every further +, -, * is 1 (an fmaf is counted as the product
     and the addition it replaces: the bound does not encode the kernel's fusing either).
A recomputed quantity that feeds a later product (s_k, a, ir, gy, the masked upstream, g) carries its own bound forward
to first order (`d...` names) through the absolute values of what multiplies it.  An element whose M is 0 (a masked-off
unit's whole column, an all-zero latent) must be exactly 0; NaN and inf fail.

ReLU: ``assert_relu_margin`` (head_ref) before anything is compared -- every a_m lies outside its own bound of zero, or
is zero by construction (M == 0: the mask is then off on both sides, the derivative at 0 being 0 as in torch)."""
import numpy as np
import torch

from head_ref import U32, Ref, _gen, assert_relu_margin, d64

RANK = 8                         # TorchFM's k (common_pytorch_models.py:41-47 as DeepCoNN.py:32 / TransNet.py:77-79 build it)
KINDS = ('fm', 'mlp', 'pfm')
OUTPUTS = ('score', 'g_user', 'g_item', 'w_user', 'w_item')
N_U, N_I = 3, 4                  # so that indices repeat


# ------------------------------------------------------------------------------------------------------ the float64 side
def _fm(y, dy, V, lw):
    """TorchFM over y [N, n] (without lin.bias) and its gradient, y known to within dy (>= 0, first order):
      s_k    c = n               n-term dot                                        A_k = |y| |V|_k
             ds_k = dy . |V|_k + n 2^-24 A_k
      head   c = 2n + k + 3      s_k: n; s_k^2: 2n + 1; k-term sum: + k; - q2: + 1; + lin: + 1   (the 1/2 is exact;
                                 q2 = sum_j y_j^2 v2_j is n + k + 2 and lin n roundings deep: both below 2n + k + 1)
                                 M = 1/2 sum_k (A_k^2 + Q_k) + |y| . |lw|,   Q_k = y^2 (V^2)_k
             + the inputs' part  sum_j dy_j (|lw_j| + sum_k |s_k| |V_jk| + |y_j| v2_j)
      gy_j   c = n + k + 3       s_k: n; s_k V_jk: + 1; k-term sum: + k; + lw_j: + 1; - y_j v2_j: + 1  (y_j v2_j itself is
                                 k + 1 roundings deep: below n + k + 1)
                                 M = sum_k A_k |V_jk| + |y_j| v2_j + |lw_j|
             + the inputs' part  sum_k |V_jk| (dy . |V|_k) + dy_j v2_j
    -> (head, dhead, gy, dgy)."""
    n, k = V.shape
    Va, v2 = V.abs(), (V * V).sum(1)
    s, A = y @ V, y.abs() @ Va
    Q = (y * y) @ (V * V)
    ds_in = dy @ Va
    head = 0.5 * ((s * s).sum(1) - Q.sum(1)) + y @ lw
    Mhead = 0.5 * (A * A + Q).sum(1) + y.abs() @ lw.abs()
    dhead = (2 * n + k + 3) * U32 * Mhead + (dy * (lw.abs() + s.abs() @ Va.T + y.abs() * v2)).sum(1)
    gy = lw + s @ V.T - y * v2
    Mgy = A @ Va.T + y.abs() * v2 + lw.abs()
    dgy = (n + k + 3) * U32 * Mgy + ds_in @ Va.T + dy * v2
    return head, dhead, gy, dgy


def pair_grad_ref(kind, zu, zi, u_idx, i_idx, params, fc_u, fc_i, q_bias=None, c_bias=None, dzu=None, dzi=None):
    """Float64 values and per-element bounds of every output of r4r_pair_grad -> Ref (head_ref) by OUTPUTS' names.
    ``params``: V, lw (fm); W0, b0, w3 (mlp); W0, b0, W2, b2, V, lw and xu / xi or neither (pfm).  Per kind:

      fm     score = (head + q_bias) + c_bias: head's bound + 2 2^-24 (|head| + |q_bias| + |c_bias|); g = gy over x.
      mlp    a_m    c = 2L + 1    2L-term dot, + b0                                Ma = |W0| |x| + |b0|
             score  c = L + 2     L-term dot of w3 and relu(a), + q_bias, + c_bias  M = |w3| . relu(a) + |q_bias| + |c_bias|
                    + the carried part |w3| . da over the units that are on
             g_j    c = L         L-term dot of [a > 0] w3 (exact) and W0[:, j]     M = sum_m [a_m > 0] |w3_m| |W0_mj|
      pfm    a as mlp;  ir_k  c = L + 1  (L-term dot, + b2)   d ir = |W2| dh + (L + 1) 2^-24 (|W2| h + |b2|),  dh = da where on
             y = [eu ; ei ; ir], dy = [0 ; 0 ; d ir];  the fm over y with those dy;  score as fm
             t_m = sum_k W2[k, m] gy[2P + k]   c = L   dt = |W2|^T dgy + L 2^-24 |W2|^T |gy|
             up = [a > 0] t (dup = dt where on);  g_j = sum_m up_m W0[m, j]   c = L   dg = |W0|^T dup + L 2^-24 |W0|^T |up|
      w_user[f] = sum_l g_user[l] fc_u[l, f]   c = L   dw = dg |fc| + L 2^-24 |g| |fc|;  w_item likewise.
    ``dzu`` / ``dzi`` (>= 0, the shapes of zu / zi; default 0): how far the latents the kernel is given may lie from
    ``zu`` / ``zi`` -- e.g. the roundings of the fp32 tower fc against a float64 one.  dx = [dzu ; dzi] enters to first
    order where x does: da += dx |W0|^T, and the fm over x takes dy = dx."""
    assert kind in KINDS, kind
    zu, zi, fc_u, fc_i = d64(zu), d64(zi), d64(fc_u), d64(fc_i)
    u, i = u_idx.detach().cpu().reshape(-1), i_idx.detach().cpu().reshape(-1)
    P_ = {k: d64(v) for k, v in params.items() if v is not None}
    L = zu.shape[1]
    x = torch.cat([zu[u], zi[i]], 1)
    N = x.shape[0]
    qb = d64(q_bias)[u] if q_bias is not None else torch.zeros(N, dtype=torch.float64)
    cb = d64(c_bias)[i] if c_bias is not None else torch.zeros(N, dtype=torch.float64)
    dx = torch.cat([d64(dzu)[u] if dzu is not None else torch.zeros_like(zu[u]),
                    d64(dzi)[i] if dzi is not None else torch.zeros_like(zi[i])], 1)
    aux = {}
    if kind == 'fm':
        head, dhead, g, dg = _fm(x, dx, P_['V'], P_['lw'].reshape(-1))
    else:
        W0, b0 = P_['W0'], P_['b0'].reshape(-1)
        a = x @ W0.T + b0
        Ma = x.abs() @ W0.abs().T + b0.abs()
        da = (2 * L + 1) * U32 * Ma + dx @ W0.abs().T
        assert_relu_margin('pair_grad ' + kind, a, da, Ma)
        on = a > 0
        off = torch.zeros_like(a)
        h, dh = torch.where(on, a, off), torch.where(on, da, off)
        aux.update(a=a, on=on)
        if kind == 'mlp':
            w3 = P_['w3'].reshape(-1)
            head = h @ w3
            dhead = dh @ w3.abs() + L * U32 * (h @ w3.abs())
            up, dup = torch.where(on, w3.expand_as(a), off), off
        else:
            W2, b2 = P_['W2'], P_['b2'].reshape(-1)
            ir = h @ W2.T + b2
            dir_ = dh @ W2.abs().T + (L + 1) * U32 * (h @ W2.abs().T + b2.abs())
            emb = [P_['xu'][u], P_['xi'][i]] if 'xu' in P_ else []
            P2 = sum(e.shape[1] for e in emb)
            y = torch.cat(emb + [ir], 1)
            dy = torch.cat([torch.zeros((N, P2), dtype=torch.float64), dir_], 1)
            head, dhead, gy, dgy = _fm(y, dy, P_['V'], P_['lw'].reshape(-1))
            gir, dgir = gy[:, P2:], dgy[:, P2:]
            t = gir @ W2
            dt = dgir @ W2.abs() + L * U32 * (gir.abs() @ W2.abs())
            up, dup = torch.where(on, t, off), torch.where(on, dt, off)
            aux.update(y=y, gy=gy, t=t)
        g = up @ W0
        dg = dup @ W0.abs() + L * U32 * (up.abs() @ W0.abs())
    score = head + qb + cb
    dscore = dhead + 2 * U32 * (head.abs() + qb.abs() + cb.abs())
    gu, gi, dgu, dgi = g[:, :L], g[:, L:], dg[:, :L], dg[:, L:]
    ref = Ref(score=(score, dscore), g_user=(gu, dgu), g_item=(gi, dgi),
              w_user=(gu @ fc_u, dgu @ fc_u.abs() + L * U32 * (gu.abs() @ fc_u.abs())),
              w_item=(gi @ fc_i, dgi @ fc_i.abs() + L * U32 * (gi.abs() @ fc_i.abs())))
    ref.aux = aux
    return ref


# --------------------------------------------------------------------------------- float32, in another summation order
MUTANTS = ('drop_x_v2', 'mask_ge', 'w2_not_transposed', 'fc_swapped')


def pair_grad_f32(kind, zu, zi, u_idx, i_idx, params, fc_u, fc_i, q_bias=None, c_bias=None, mutant=None):
    """The closed forms in numpy float32, every dot in DESCENDING index order through numpy's own (pairwise / BLAS)
    summation -- not the kernel's chains -- -> dict by OUTPUTS' names.  ``mutant``: one of MUTANTS, a wrong formula:
    the FM gradient without - x_j sum_k V_jk^2; the ReLU mask as a >= 0; W2 in the place of W2^T (pfm); fc_u and fc_i
    swapped."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = lambda t: None if t is None else np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    zu, zi, fc_u, fc_i = f(zu), f(zi), f(fc_u), f(fc_i)
    p = {k: f(v) for k, v in params.items() if v is not None}
    u, i = u_idx.detach().cpu().numpy().reshape(-1), i_idx.detach().cpu().numpy().reshape(-1)
    L = zu.shape[1]

    def dot(a, b):                                           # a [N, n] @ b [n, m], n walked downwards
        return np.matmul(a[:, ::-1], b[::-1]).astype(np.float32)

    def fm(y, V, lw):
        s = dot(y, V)
        v2 = (V * V)[:, ::-1].sum(1, dtype=np.float32)
        head = np.float32(0.5) * ((s * s).sum(1, dtype=np.float32) - dot(y * y, v2[:, None])[:, 0]) + dot(y, lw[:, None])[:, 0]
        gy = lw + dot(s, np.ascontiguousarray(V.T))
        if mutant != 'drop_x_v2':
            gy = gy - y * v2
        return head.astype(np.float32), gy.astype(np.float32)

    x = np.concatenate([zu[u], zi[i]], 1)
    if kind == 'fm':
        head, g = fm(x, p['V'], p['lw'].reshape(-1))
    else:
        W0 = p['W0']
        a = dot(x, np.ascontiguousarray(W0.T)) + p['b0'].reshape(-1)
        on = (a >= 0) if mutant == 'mask_ge' else (a > 0)
        h = np.where(a > 0, a, np.float32(0))
        if kind == 'mlp':
            w3 = p['w3'].reshape(-1)
            head = dot(h, w3[:, None])[:, 0]
            up = np.where(on, w3[None, :], np.float32(0)).astype(np.float32)
        else:
            W2 = p['W2']
            ir = dot(h, np.ascontiguousarray(W2.T)) + p['b2'].reshape(-1)
            emb = [p['xu'][u], p['xi'][i]] if 'xu' in p else []
            P2 = sum(e.shape[1] for e in emb)
            head, gy = fm(np.concatenate(emb + [ir], 1), p['V'], p['lw'].reshape(-1))
            t = dot(gy[:, P2:], np.ascontiguousarray(W2.T) if mutant == 'w2_not_transposed' else W2)
            up = np.where(on, t, np.float32(0)).astype(np.float32)
        g = dot(up, W0)
    qb = f(q_bias)[u] if q_bias is not None else np.zeros(len(u), np.float32)
    cb = f(c_bias)[i] if c_bias is not None else np.zeros(len(u), np.float32)
    if mutant == 'fc_swapped':
        fc_u, fc_i = fc_i, fc_u
    out = dict(score=cb + (qb + head), g_user=g[:, :L], g_item=g[:, L:], w_user=dot(g[:, :L], fc_u), w_item=dot(g[:, L:], fc_i))
    assert all(v.dtype == np.float32 for v in out.values())
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# ===================================================================================================== cases and inputs
FM_LS = (1, 31, 32, 33, 64, 65, 128)        # around the 64-lane slots of x = [zu ; zi] (2L = 2, 62, 64, 66, 128, 130, 256)
HEAD_LS = (1, 31, 32, 33, 64)               # mlp, pfm: around the 16-lane rows and the 64-lane columns; 64 is the limit
FS = (1, 64, 65, 100, 112)                  # one filter; one per lane; the first lane holds two; the towers' 100; the limit
PS = (0, 5)                                 # transnet / transnet++
NPS = (1, 5, 257)                           # one wave; two workgroups, the second with one live wave; 65 workgroups
# (kind, L, F, P) -> seed where seed 0 leaves a pre-activation inside its ReLU margin (as it is, with ``with_zero_rows`` or
# with ``with_zero_unit(L // 2)``); tests/test_pair_grad_host.py asserts the margins of every case with these seeds
SEEDS = {('mlp', 64, 100, 0): 1, ('pfm', 64, 65, 5): 1}


def shapes(kind):
    """Every (L, F, P) of a kind."""
    return [(L, F, P) for L in (FM_LS if kind == 'fm' else HEAD_LS) for F in FS for P in (PS if kind == 'pfm' else (0,))]


def pair_inputs(kind, L, F, P=0, n_p=5, seed=None, biases=True):
    """Seeded Gaussian inputs of a case -> dict(zu, zi, u_idx, i_idx, params, fc_u, fc_i, q_bias, c_bias), float32 / int64
    on the CPU.  Everything but the indices depends on (kind, L, F, P) alone, so the same pair has the same inputs at
    every n_p; the indices walk all N_U x N_I pairs first, then repeat at random."""
    seed = SEEDS.get((kind, L, F, P), 0) if seed is None else seed
    g = _gen(11, KINDS.index(kind), L, F, P, seed)
    r = lambda *s: torch.randn(s, generator=g)
    n = 2 * L if kind == 'fm' else 2 * P + L
    params = {}
    if kind != 'fm':
        params.update(W0=r(L, 2 * L) * 0.4, b0=r(L) * 0.1)
    if kind == 'mlp':
        params.update(w3=r(L) * 0.4)
    if kind == 'pfm':
        params.update(W2=r(L, L) * 0.4, b2=r(L) * 0.1)
        if P:
            params.update(xu=r(N_U, P), xi=r(N_I, P))
    if kind != 'mlp':
        params.update(V=r(n, RANK) * 0.3, lw=r(n) * 0.3)
    d = dict(zu=r(N_U, L), zi=r(N_I, L), params=params, fc_u=r(L, F) * 0.3, fc_i=r(L, F) * 0.3,
             q_bias=r(N_U) if biases else None, c_bias=r(N_I) if biases else None)
    gi = _gen(12, n_p)
    every = torch.arange(N_U * N_I)
    more = torch.randint(0, N_U * N_I, (max(n_p - N_U * N_I, 0),), generator=gi)
    pairs = torch.cat([every, more])[:n_p]
    d.update(u_idx=(pairs // N_I).to(torch.int64), i_idx=(pairs % N_I).to(torch.int64))
    return d


def ref_of(kind, d):
    return pair_grad_ref(kind, d['zu'], d['zi'], d['u_idx'], d['i_idx'], d['params'], d['fc_u'], d['fc_i'], d['q_bias'],
                         d['c_bias'])


def f32_of(kind, d, mutant=None):
    return pair_grad_f32(kind, d['zu'], d['zi'], d['u_idx'], d['i_idx'], d['params'], d['fc_u'], d['fc_i'], d['q_bias'],
                         d['c_bias'], mutant=mutant)


def with_zero_rows(d):
    """User 0 and item 0 all-zero, b0 zero: the pair (0, 0) has a == 0 exactly in every unit (M == 0): the masks are off."""
    d = dict(d, zu=d['zu'].clone(), zi=d['zi'].clone(), params=dict(d['params']))
    d['zu'][0] = 0.0
    d['zi'][0] = 0.0
    d['params']['b0'] = torch.zeros_like(d['params']['b0'])
    return d


def with_zero_unit(d, m):
    """Unit m with an all-zero W0 row and a zero bias: a_m is an exact 0 for every pair while the other units are live."""
    d = dict(d, params=dict(d['params']))
    d['params']['W0'], d['params']['b0'] = d['params']['W0'].clone(), d['params']['b0'].clone()
    d['params']['W0'][m] = 0.0
    d['params']['b0'][m] = 0.0
    return d
