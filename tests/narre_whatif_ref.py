"""Float64 restatements of the two passes of NARRE's what-if scores (include/r4r.h, "NARRE what-if scores";
csrc/narre_whatif.hip) with per-element bounds, a float32 numpy evaluation of the same closed forms in ANOTHER summation
order (and its mutants), and the seeded inputs the host and the GPU tests share.  No kernel of the project and no GPU
code lives here.

The rule is tests/head_ref.py's, for every output element:   |kernel - float64| <= c * 2^-24 * M
  M  the same expression evaluated in float64 with every term replaced by its absolute value;
  c  the number of fp32 roundings on the longest path to that element, counted for an ARBITRARY summation order: a
     product is 1, an n-term sum of products (a dot) is n, every further +, -, * is 1 (an fmaf counts as the product and
     the addition it replaces).
A recomputed quantity that feeds a later product carries its own bound forward to first order (`d...` names) through
the absolute values of what multiplies it.  NaN and inf fail.

Owner pass (``logits_ref``), cat = [z ; other], z known to within dz >= 0 (default 0):
  pre = cat W0^T + b0      c = 2L + 1                    dpre = (2L + 1) 2^-24 M + dz |W0[:, :L]|^T
  h = relu(pre)            the same roundings            (exactly 0 where off, once the ReLU margin holds)
  logit = h . w3 + b3      c = L + 1                     dlogit = dh . |w3| + (L + 1) 2^-24 (|h| . |w3| + |b3|)
Variant pass (``whatif_ref``), per (pair, variant, side); the side's z, logit, z_pad, logit_pad known to within dz,
dlogit, dz_pad, dlogit_pad (default 0):
  list   ``select``: the first R clear slots of 0 .. S - 1 ascending, the tail the pad slot (index S)
  a' = softmax_R(logit')   head_ref.attention_ref's rule: relative expm1(2 rho + (R + 1) 2^-24), rho = max dlogit'
                           + 2^-24 spread(logit') + C_EXPF 2^-24, + 2 TINY absolute: the logit's bound goes through the
                           softmax to first order
  o' = sum_k a'_k z'_k     do = da . |z'| + a . dz' + R 2^-24 a . |z'|
  p' = o' + own            c = 1     dp = do + 2^-24 (|o'| + |own|)       (no own: p' = o', dp = do)
  x = p'_u p'_i            c = 1     dx = dp_u |p_i| + |p_u| dp_i + 2^-24 |x|
  t = W1 x + b1            c = L + 1 dt = |W1| dx + (L + 1) 2^-24 (|W1| |x| + |b1|)
  head = w . relu(t)       c = L     dhead = |w| . dt (where on) + L 2^-24 |w| . relu(t)
  score = (head + q_bias) + c_bias   + 2 2^-24 (|head| + |q_bias| + |c_bias|)
ReLU: ``assert_relu_margin`` (head_ref) for the scorer's pre and, for EVERY variant, for t, before anything is compared."""
import numpy as np
import torch

from head_ref import C_EXPF, TINY, U32, Ref, _gen, assert_relu_margin, d64
from narre_pair_ref import gather_other

N_U, N_I = 3, 4
OTHER_ROWS = 7
ALL_BITS = -1                       # int64 with every bit set
BIT63 = -(1 << 63)                  # int64 with bit 63 alone


# ------------------------------------------------------------------------------------------------------ the float64 side
def logits_ref(s, dz=None):
    """``s``: dict(z [N, S, L], nb [N, S], other_table, W0, b0, w3, b3) -> Ref(logit=(value, bound))."""
    x, W0, b0, b3 = d64(s['z']), d64(s['W0']), d64(s['b0']).reshape(-1), d64(s['b3']).reshape(())
    w3 = d64(s['w3']).reshape(-1)
    L = x.shape[-1]
    dz = torch.zeros_like(x) if dz is None else d64(dz)
    cat = torch.cat([x, gather_other(s['other_table'], s['nb'])], -1)
    pre = cat @ W0.T + b0
    Mpre = cat.abs() @ W0.abs().T + b0.abs()
    dpre_in = dz @ W0[:, :L].abs().T
    assert_relu_margin('narre what-if scorer', pre, (2 * L + 1) * U32 * Mpre + dpre_in, Mpre + dpre_in)
    on = pre > 0
    zero = torch.zeros_like(pre)
    h = torch.where(on, pre, zero)
    dh = torch.where(on, (2 * L + 1) * U32 * Mpre + dpre_in, zero)
    sc = h @ w3 + b3
    dsc = dh @ w3.abs() + (L + 1) * U32 * (h.abs() @ w3.abs() + b3.abs())
    ref = Ref(logit=(sc, dsc))
    ref.aux = dict(pre=pre, on=on)
    return ref


def select(mask, S, R):
    """``mask``: int64 array of any shape -> int64 [..., R]: the first R slots of 0 .. S - 1 whose bit is clear, in
    ascending order; S (the pad slot) where fewer than R are left.  Bits at positions >= S are ignored."""
    m = np.ascontiguousarray(np.asarray(mask, dtype=np.int64)).view(np.uint64)
    keep = ((m[..., None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)) == 0
    order = np.argsort(~keep, axis=-1, kind='stable')[..., :R]
    left = keep.sum(-1)
    return np.where(np.arange(R) < left[..., None], order, S).astype(np.int64)


def _side64(s):
    z, lg = d64(s['z']), d64(s['logit'])
    n, S, L = z.shape
    zp, lp = d64(torch.as_tensor(s['z_pad'])).reshape(1, 1, L), torch.full((1, 1), float(s['logit_pad']), dtype=torch.float64)
    opt = lambda k, like: d64(torch.as_tensor(s[k])).reshape(like.shape).expand(like.shape) if s.get(k) is not None else torch.zeros_like(like)
    full = dict(z=torch.cat([z, zp.expand(n, 1, L)], 1), lg=torch.cat([lg, lp.expand(n, 1)], 1),
                dz=torch.cat([opt('dz', z), opt('dz_pad', zp).expand(n, 1, L)], 1),
                dlg=torch.cat([opt('dlogit', lg), opt('dlogit_pad', lp).expand(n, 1)], 1))
    full['own'] = None if s.get('own') is None else d64(s['own'])
    full['S'], full['R'] = S, int(s['R'])
    return full


def _pooled64(f, idx, drop):
    """One side of a chunk of pairs: owners ``idx`` [c], masks ``drop`` [c, V] -> (p', dp') [c, V, L]."""
    S, R = f['S'], f['R']
    sel = torch.from_numpy(select(drop.numpy(), S, R))                          # [c, V, R]
    c, V = drop.shape
    rows = idx[:, None, None].expand(c, V, R)
    lg, dlg = f['lg'][rows, sel], f['dlg'][rows, sel]
    z, dz = f['z'][rows, sel], f['dz'][rows, sel]                               # [c, V, R, L]
    a = torch.softmax(lg, dim=-1)
    spread = lg.max(-1).values - lg.min(-1).values + 2 * dlg.max(-1).values
    rho = dlg.max(-1).values + U32 * spread + C_EXPF * U32
    da = a * torch.expm1(2 * rho + (R + 1) * U32)[..., None] + 2 * TINY
    o = torch.einsum('cvr,cvrl->cvl', a, z)
    do = (torch.einsum('cvr,cvrl->cvl', da, z.abs()) + torch.einsum('cvr,cvrl->cvl', a, dz)
          + R * U32 * torch.einsum('cvr,cvrl->cvl', a, z.abs()))
    if f['own'] is None:
        return o, do
    own = f['own'][idx][:, None, :]
    return o + own, do + U32 * (o.abs() + own.abs())


def whatif_ref(user, item, u_idx, i_idx, drop_u, drop_i, W1, b1, w, q_bias=None, c_bias=None, chunk=16):
    """``user`` / ``item``: dicts with z [n, S, L], logit [n, S], z_pad [L], logit_pad, R, optionally own [n, L] and the
    bounds dz, dlogit, dz_pad, dlogit_pad.  ``drop_*``: int64 [n_p, V] or None -> Ref(score=(value, bound)) [n_p, V];
    aux['t'] holds the head's pre-activations of every variant."""
    W1, b1, w = d64(W1), d64(b1).reshape(-1), d64(w).reshape(-1)
    L = W1.shape[0]
    u_idx, i_idx = u_idx.detach().cpu().reshape(-1), i_idx.detach().cpu().reshape(-1)
    n_p = u_idx.numel()
    V = next((int(d.shape[1]) for d in (drop_u, drop_i) if d is not None), 1)
    zeros = torch.zeros((n_p, V), dtype=torch.int64)
    drop_u = zeros if drop_u is None else drop_u.detach().cpu()
    drop_i = zeros if drop_i is None else drop_i.detach().cpu()
    fu, fi = _side64(user), _side64(item)
    score, dscore, ts = [], [], []
    for c0 in range(0, n_p, chunk):
        sl = slice(c0, c0 + chunk)
        pu, dpu = _pooled64(fu, u_idx[sl], drop_u[sl])
        pi, dpi = _pooled64(fi, i_idx[sl], drop_i[sl])
        x = pu * pi
        dx = dpu * pi.abs() + pu.abs() * dpi + U32 * x.abs()
        t = x @ W1.T + b1
        Mt = x.abs() @ W1.abs().T + b1.abs()
        dt_in = dx @ W1.abs().T
        dt = (L + 1) * U32 * Mt + dt_in
        assert_relu_margin('narre what-if head', t, dt, Mt + dt_in)
        on = t > 0
        zero = torch.zeros_like(t)
        h = torch.where(on, t, zero)
        head = h @ w
        dhead = torch.where(on, dt, zero) @ w.abs() + L * U32 * (h @ w.abs())
        n = x.shape[0]
        qb = d64(q_bias)[u_idx[sl]] if q_bias is not None else torch.zeros(n, dtype=torch.float64)
        cb = d64(c_bias)[i_idx[sl]] if c_bias is not None else torch.zeros(n, dtype=torch.float64)
        score.append(head + qb[:, None] + cb[:, None])
        dscore.append(dhead + 2 * U32 * (head.abs() + qb.abs()[:, None] + cb.abs()[:, None]))
        ts.append(t)
    cat = lambda parts, tail: torch.cat(parts) if parts else torch.zeros((0, V) + tail, dtype=torch.float64)
    ref = Ref(score=(cat(score, ()), cat(dscore, ())))
    ref.aux = dict(t=cat(ts, (L,)))
    return ref


# --------------------------------------------------------------------------------- float32, in another summation order
MUTANTS = ('no_renorm', 'pad_without_logit', 'no_slide', 'sides_swapped', 'bits_reversed', 'no_own')


def _np32(t):
    return None if t is None else np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=np.float32)


def _dot(a, b):
    """a [..., n] @ b [n, m] with n walked downwards through numpy's own summation -- not the kernels' chains."""
    return np.matmul(a[..., ::-1], b[::-1]).astype(np.float32)


def logits_f32(s):
    """The owner pass in numpy float32, descending order -> float32 [N, S]."""
    x, W0, b0, w3, b3 = (_np32(s[k]) for k in ('z', 'W0', 'b0', 'w3', 'b3'))
    other = gather_other(s['other_table'], s['nb']).numpy().astype(np.float32)
    cat = np.concatenate([x, other], -1)
    pre = _dot(cat, np.ascontiguousarray(W0.T)) + b0.reshape(-1)
    h = np.where(pre > 0, pre, np.float32(0)).astype(np.float32)
    sc = (_dot(h, w3.reshape(-1, 1))[..., 0] + b3.reshape(())).astype(np.float32)
    assert sc.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(sc))


def _reverse_bits(mask, S):
    m = np.ascontiguousarray(np.asarray(mask, dtype=np.int64)).view(np.uint64)
    out = np.zeros_like(m)
    for s in range(S):
        out |= ((m >> np.uint64(s)) & np.uint64(1)) << np.uint64(S - 1 - s)
    return out.view(np.int64)


def _pooled32(s, idx, drop, mutant):
    z, lg, zp = _np32(s['z']), _np32(s['logit']), _np32(s['z_pad']).reshape(-1)
    n, S, L = z.shape
    R = int(s['R'])
    lp = np.float32(0.0 if mutant == 'pad_without_logit' else s['logit_pad'])
    zf = np.concatenate([z, np.broadcast_to(zp, (n, 1, L))], 1)
    lf = np.concatenate([lg, np.full((n, 1), lp, np.float32)], 1)
    drop = np.asarray(drop, dtype=np.int64)
    if mutant == 'bits_reversed':
        drop = _reverse_bits(drop, S)
    c, V = drop.shape
    rows = np.broadcast_to(idx[:, None, None], (c, V, R))
    if mutant == 'no_slide':                                    # the slots beyond R never move up
        sel = select(drop, R, R)
        sel = np.where(sel == R, S, sel)
    else:
        sel = select(drop, S, R)
    if mutant == 'no_renorm':                                   # the weights of the list with nothing removed
        base = select(np.zeros_like(drop), S, R)
        lgb = lf[rows, base]
        e = np.exp((lgb - lgb.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
        ab = (e / e[..., ::-1].sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
        gone = ((np.ascontiguousarray(drop).view(np.uint64)[..., None] >> base.clip(max=63).astype(np.uint64)) & np.uint64(1)) == 1
        a = np.where(gone & (base < S), np.float32(0), ab).astype(np.float32)
        sel = base
    else:
        lgs = lf[rows, sel]
        e = np.exp((lgs - lgs.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
        a = (e / e[..., ::-1].sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    zs = zf[rows, sel]
    o = np.einsum('cvr,cvrl->cvl', a[..., ::-1], zs[:, :, ::-1]).astype(np.float32)
    if s.get('own') is not None and mutant != 'no_own':
        o = (_np32(s['own'])[idx][:, None, :] + o).astype(np.float32)
    return o


def whatif_f32(user, item, u_idx, i_idx, drop_u, drop_i, W1, b1, w, q_bias=None, c_bias=None, mutant=None, chunk=16):
    """The variant pass in numpy float32, descending order -> float32 [n_p, V].  Mutants: 'no_renorm' (the softmax of the
    list with nothing removed, the removed slots' weights dropped), 'pad_without_logit' (z_pad with a logit of 0),
    'no_slide' (nothing beyond slot R moves up), 'sides_swapped' (the two masks), 'bits_reversed' (bit s read as slot
    S - 1 - s), 'no_own'."""
    assert mutant is None or mutant in MUTANTS, mutant
    W1, b1, w = _np32(W1), _np32(b1).reshape(-1), _np32(w).reshape(-1)
    u, i = u_idx.detach().cpu().numpy().reshape(-1), i_idx.detach().cpu().numpy().reshape(-1)
    V = next((int(d.shape[1]) for d in (drop_u, drop_i) if d is not None), 1)
    zeros = np.zeros((len(u), V), np.int64)
    du = zeros if drop_u is None else drop_u.detach().cpu().numpy()
    di = zeros if drop_i is None else drop_i.detach().cpu().numpy()
    if mutant == 'sides_swapped':
        du, di = di, du
    out = []
    for c0 in range(0, len(u), chunk):
        sl = slice(c0, c0 + chunk)
        x = _pooled32(user, u[sl], du[sl], mutant) * _pooled32(item, i[sl], di[sl], mutant)
        t = _dot(x, np.ascontiguousarray(W1.T)) + b1
        head = _dot(np.where(t > 0, t, np.float32(0)).astype(np.float32), w[:, None])[..., 0]
        qb = _np32(q_bias)[u[sl]] if q_bias is not None else np.zeros(x.shape[0], np.float32)
        cb = _np32(c_bias)[i[sl]] if c_bias is not None else np.zeros(x.shape[0], np.float32)
        out.append((cb[:, None] + (qb[:, None] + head)).astype(np.float32))
    got = np.concatenate(out) if out else np.zeros((0, V), np.float32)
    assert got.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(got))


# ===================================================================================================== cases and inputs
RSS = ((1, 1), (1, 3), (5, 5), (10, 10), (10, 12), (10, 64), (33, 40), (64, 64))   # (R, S): one slot; slide-in at R = 1;
#   one staged group; the catalogue's R as occlusion, with two and with 54 spare slots; ragged groups; the limit
LS = (1, 31, 32, 33, 64)         # around the 16-row MFMA tiles (LT = 1 / 2 / 3 / 4), the owner pass's LMAX classes, the limit
VS = (1, 15, 16, 17, 21, 33)     # one column; a ragged tile; a full tile; a second tile of one; the benchmark's; three tiles
NPS = (1, 5, 257)                # one wave; two workgroups; many
# pairwise covering: every ((R, S), L), ((R, S), V) and (L, V) value pair occurs
SHAPES = ([(RSS[a], LS[b], VS[(a + b) % 6]) for a in range(8) for b in range(5)]
          + [(RSS[a], LS[a % 5], VS[(a + 5) % 6]) for a in range(8)])
# (R_u, S_u, R_i, S_i, L, V, n_p): every shape with both sides alike, and one pair of sides that differ in R and S
CASES = ([(rs[0], rs[1], rs[0], rs[1], L, V, NPS[k % 3]) for k, (rs, L, V) in enumerate(SHAPES)]
         + [(5, 7, 10, 12, 32, 21, 5)])
LOGIT_CASES = [(NS, S, L) for k, (NS, (S, L)) in enumerate(
    zip((1, 5, 9) * 9, [(S, L) for S in (1, 3, 5, 10, 12, 40, 64) for L in LS][::2]))]
# case -> seed where seed 0 leaves a pre-activation inside its ReLU margin (``find_seed`` below is how they are found;
# tests/test_narre_whatif_host.py asserts the margins of every case with these seeds)
SEEDS = {(1, 3, 1, 3, 64, 33, 1): 1, (10, 64, 10, 64, 64, 17, 257): 9, (64, 64, 64, 64, 64, 33, 1): 18,
         (5, 5, 5, 5, 32, 15, 1): 1}
LOGIT_SEEDS = {(5, 64, 32): 2, (9, 64, 64): 2}
# the cases that are also run without own rows and without biases (their margins hold there too, with the same seeds)
BARE_CASES = CASES[::7] + [CASES[-1]]


def owner_inputs(tag, N, S, L, seed=0):
    """Seeded Gaussian inputs of one side's owner pass -> dict, float32 / int64 on the CPU.  An owner's inputs do not
    depend on N: every tensor is drawn owner by owner.  nb holds ids of a 7-row table; slot S - 1 of owner 0 names a row
    OUTSIDE it (-1; owner 1: OTHER_ROWS), which reads as zeros."""
    g = _gen(31, tag, S, L, seed)
    r = lambda *s: torch.randn(s, generator=g)
    d = dict(W0=r(L, 2 * L) * 0.4, b0=r(L) * 0.1, w3=r(L) * 0.4, b3=r(1), other_table=r(OTHER_ROWS, L), z_pad=r(L) * 0.5,
             own_all=r(11, L))
    z, nb = [], []
    for n in range(N):
        gn = _gen(32, tag, S, L, seed, n)
        z.append(torch.randn((S, L), generator=gn))
        nb.append(torch.randint(0, OTHER_ROWS, (S,), generator=gn))
    d['z'], d['nb'] = torch.stack(z), torch.stack(nb).to(torch.int64)
    d['nb'][0, S - 1] = -1
    if N > 1:
        d['nb'][1, S - 1] = OTHER_ROWS
    d['own'] = d['own_all'][(torch.arange(N) * 3 + 1) % 11].contiguous()
    d['pad_id'] = OTHER_ROWS - 1
    return d


def pad_inputs(raw):
    """The owner-pass call of a side's padding slot: N = 1, S = 1 on z_pad and the pad id."""
    return dict(raw, z=raw['z_pad'].reshape(1, 1, -1), nb=torch.tensor([[raw['pad_id']]], dtype=torch.int64))


def edge_masks(S, R):
    """The masks every what-if test must see, as int64: nothing; every single bit; bit S - 1; bit 63; a bit >= S (where
    S < 64); all bits (every slot is the pad: uniform weights); drops that leave fewer than R slots; two spellings of
    one list (a bit on a slot that would not have been selected)."""
    i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    m = [0] + [i64(1 << s) for s in range(S)] + [i64(1 << (S - 1)), BIT63, ALL_BITS]
    if S < 64:
        m += [i64(1 << S), i64((1 << S) | 1)]
    m += [i64(((1 << S) - 1) & ~1), i64(((1 << S) - 1) & ~(1 << (S - 1)))]      # one slot left: R - 1 pads
    if S > R:
        m += [i64(1 | (1 << (S - 1))), i64(3)]
    return m


def variant_masks(S, R, V, stride, n_p=N_U * N_I):
    """[n_p, V] int64: the edge masks walked with ``stride``, interleaved with seeded random masks of up to three drops."""
    edge = edge_masks(S, R)
    g = _gen(35, S, R, V, stride)
    rnd = torch.zeros(n_p * V, dtype=torch.int64)
    for _ in range(3):
        bit = torch.randint(0, S, (n_p * V,), generator=g)
        on = torch.randint(0, 2, (n_p * V,), generator=g)
        rnd |= torch.where(on == 1, torch.ones_like(bit) << bit.clamp(max=62), torch.zeros_like(bit))
    at = (torch.arange(n_p * V) * stride) % (2 * len(edge))
    m = torch.where(at < len(edge), torch.tensor(edge, dtype=torch.int64)[at.clamp(max=len(edge) - 1)], rnd)
    return m.reshape(n_p, V).contiguous()


def whatif_inputs(R_u, S_u, R_i, S_i, L, V, n_p=5, seed=0, biases=True, own=True):
    """Seeded inputs of a variant-pass case -> dict(user, item, u_idx, i_idx, drop_u, drop_i, W1, b1, w, q_bias, c_bias,
    raw_user, raw_item): per side z, the float64 owner pass's logits rounded to float32 (of the slots and of the pad
    slot), z_pad, own; 3 users and 4 items; the indices walk all twelve pairs first, then repeat at random."""
    raws = owner_inputs(1, N_U, S_u, L, seed), owner_inputs(2, N_I, S_i, L, seed)
    sides = []
    for raw, R in zip(raws, (R_u, R_i)):
        lg = logits_ref(raw)['logit'][0].to(torch.float32)
        lp = float(logits_ref(pad_inputs(raw))['logit'][0].to(torch.float32).reshape(()))
        sides.append(dict(z=raw['z'], logit=lg, z_pad=raw['z_pad'], logit_pad=lp, R=R, own=raw['own'] if own else None))
    g = _gen(33, R_u, S_u, R_i, S_i, L, seed)
    r = lambda *s: torch.randn(s, generator=g)
    d = dict(user=sides[0], item=sides[1], W1=r(L, L) * 0.4, b1=r(L) * 0.1, w=r(L) * 0.4, raw_user=raws[0], raw_item=raws[1])
    qb, cb = r(N_U), r(N_I)
    d.update(q_bias=qb if biases else None, c_bias=cb if biases else None)
    gi = _gen(34, n_p)
    every = torch.arange(N_U * N_I)
    more = torch.randint(0, N_U * N_I, (max(n_p - N_U * N_I, 0),), generator=gi)
    pairs = torch.cat([every, more])[:n_p]
    d.update(u_idx=(pairs // N_I).to(torch.int64), i_idx=(pairs % N_I).to(torch.int64))
    # a pair's masks go with the PAIR, not with its place in the call: a repeated pair repeats its variants, so the
    # twelve pairs are every (pair, variant) a case holds, whatever n_p
    d.update(drop_u=variant_masks(S_u, R_u, V, 1)[pairs].contiguous(), drop_i=variant_masks(S_i, R_i, V, 3)[pairs].contiguous())
    return d


ARGS = ('user', 'item', 'u_idx', 'i_idx', 'drop_u', 'drop_i', 'W1', 'b1', 'w', 'q_bias', 'c_bias')


def whatif_ref_of(d):
    return whatif_ref(*(d[k] for k in ARGS))


def whatif_f32_of(d, mutant=None):
    return whatif_f32(*(d[k] for k in ARGS), mutant=mutant)


def whatif_case(case, n_p=None, **how):
    R_u, S_u, R_i, S_i, L, V, n = case
    return whatif_inputs(R_u, S_u, R_i, S_i, L, V, n if n_p is None else n_p, SEEDS.get(case, 0), **how)


def logit_case(case):
    N, S, L = case
    return owner_inputs(0, N, S, L, LOGIT_SEEDS.get(case, 0))


def find_seed(make, tries=64):
    """The lowest seed at which ``make(seed)`` (which builds the references, hence asserts the ReLU margins) passes."""
    for seed in range(tries):
        try:
            make(seed)
            return seed
        except AssertionError as e:
            if 'ReLU mask' not in str(e):
                raise
    raise AssertionError('no seed in %d' % tries)


# the edge masks, one variant each: (R, S, L) with both sides alike, twelve pairs
EDGE_SHAPES = [(1, 3, 32), (5, 5, 33), (10, 12, 64), (10, 64, 31), (64, 64, 64)]
EDGE_SEEDS = {(10, 64, 31): 1, (64, 64, 64): 18}


def edge_case(R, S, L):
    """Every edge mask of (S, R) as one variant on the user side, against a walk of the same masks (rotated by the pair's
    number + 1) on the item side, for the twelve pairs."""
    edge = edge_masks(S, R)
    n_p, V = N_U * N_I, len(edge)
    d = whatif_inputs(R, S, R, S, L, V, n_p, EDGE_SEEDS.get((R, S, L), 0))
    m = torch.tensor(edge, dtype=torch.int64)
    d['drop_u'] = m[None, :].expand(n_p, V).contiguous()
    d['drop_i'] = torch.stack([m.roll(p + 1) for p in range(n_p)]).contiguous()
    return d


# the two passes chained: (R_u, S_u, R_i, S_i, L, V), twelve pairs -- the small shapes a catalogue on tests/golden/tiny meets
CHAIN_CASES = [(10, 12, 10, 12, 8, 21), (5, 7, 10, 12, 7, 5), (1, 3, 3, 3, 16, 4)]
CHAIN_SEEDS = {}


def chain_case(case):
    """-> (d, ref_sides): a case's inputs and its sides with the float64 logits and their bounds (dlogit, dlogit_pad) in
    the place of the rounded ones: what ``whatif_ref`` takes to bound the composition of the two passes."""
    d = whatif_inputs(*case, n_p=N_U * N_I, seed=CHAIN_SEEDS.get(case, 0))
    ref_sides = {}
    for name in ('user', 'item'):
        raw = d['raw_' + name]
        r, rp = logits_ref(raw)['logit'], logits_ref(pad_inputs(raw))['logit']
        ref_sides[name] = dict(d[name], logit=r[0], dlogit=r[1], logit_pad=float(rp[0].reshape(())), dlogit_pad=rp[1].reshape(()))
    return d, ref_sides
