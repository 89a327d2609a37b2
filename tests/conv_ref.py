"""Float64 restatement of the TextCNN tower -- word gather -> conv(3 x E, pad 2) -> relu -> global max-pool -- and
exact per-element checkers of what the kernels return for it: pooled values, argmaxes, weight gradients.

No fraction-agreeing thresholds: every (document, filter) is held to a rounding bound derived from its own window.
  y64[n, f, p] = b[f] + sum_j table[idx[n, p - 2 + j]] . w[f, j]          (a tap outside the document adds 0)
  S[n, f, p]   = |b[f]| + sum_j |table[idx[n, p - 2 + j]]| . |w[f, j]|
  beta         = coef * S,  coef = (3E + 2) 2^-24 for the fp32 GEMMs (fp32_coef), + 2^-20 under the f16x2 arithmetic
The reference is computed project-then-gather, per chunk of documents over the chunk's distinct rows, on the device
the indices live on (plain ATen float64 ops; no kernel of the project is involved)."""
import torch

U32 = 2.0 ** -24                 # unit roundoff of fp32
F16X2_EXTRA = 2.0 ** -20         # the f16x2 GEMM's extra relative error: ~2^-21 per product (include/r4r.h), doubled


def fp32_coef(E):
    """Relative bound of one conv output in fp32: a 3E-term dot product plus the bias (either algorithm's order)."""
    return (3 * E + 2) * U32


def _w3(w):
    F = w.shape[0]
    return w.reshape(F, 3, w.shape[-1])


def _tap_tokens(T, dev):
    """[P, 3] token index of tap j at position p (p - 2 + j) and whether it lies inside the document."""
    P = T + 2
    t = torch.arange(P, device=dev)[:, None] - 2 + torch.arange(3, device=dev)[None, :]
    return t.clamp(0, T - 1), (t >= 0) & (t < T)


def conv64_chunks(idx, table, w, b, chunk_docs=64):
    """Yields (n0, y64 [n, F, P], S [n, F, P]) for consecutive chunks of documents, in float64."""
    dev = idx.device
    N, T = idx.shape
    W = _w3(w).to(dev, torch.float64)                       # [F, 3, E]
    Wa = W.abs()
    b64 = b.to(dev, torch.float64)
    tok, inside = _tap_tokens(T, dev)
    for n0 in range(0, N, chunk_docs):
        ids = idx[n0:n0 + chunk_docs]
        n = ids.shape[0]
        uniq, inv = torch.unique(ids, return_inverse=True)
        X = table[uniq.to(table.device)].to(dev, torch.float64)          # [u, E]
        u = X.shape[0]
        y = b64.expand(n, T + 2, -1).clone()                             # [n, P, F]
        S = b64.abs().expand(n, T + 2, -1).clone()
        for j in range(3):
            pj = torch.cat([X @ W[:, j, :].T, X.new_zeros(1, W.shape[0])])          # row u: a tap outside the document
            aj = torch.cat([X.abs() @ Wa[:, j, :].T, X.new_zeros(1, W.shape[0])])
            r = torch.where(inside[:, j][None, :], inv[:, tok[:, j]], u)     # [n, P]
            y += pj[r]
            S += aj[r]
        yield n0, y.permute(0, 2, 1), S.permute(0, 2, 1)


def conv64(idx, table, w, b):
    """Whole y64 [N, F, P] and S (small shapes only)."""
    ys, Ss = zip(*[(y, S) for _, y, S in conv64_chunks(idx, table, w, b, chunk_docs=1 << 30)])
    return torch.cat(ys), torch.cat(Ss)


def first_identical_window(idx, table):
    """first[n, p]: the first position p' <= p of document n whose window reads the same rows tap by tap as p's.
    A tap outside the document and a tap on an all-zero table row both add an exact zero, so they count as equal."""
    dev = idx.device
    N, T = idx.shape
    P = T + 2
    V = table.shape[0]
    assert V + 1 < (1 << 21), 'window keys pack three row ids into 63 bits'
    zero_row = (table == 0).all(dim=1).to(dev)
    tok, inside = _tap_tokens(T, dev)
    key = torch.zeros((N, P), dtype=torch.int64, device=dev)
    for j in range(3):
        r = idx[:, tok[:, j]]                                            # [N, P]
        r = torch.where(inside[:, j][None, :] & ~zero_row[r], r, torch.full_like(r, -1))
        key = key * (V + 1) + (r + 1)
    sk, order = torch.sort(key, dim=1, stable=True)
    start = torch.ones_like(sk, dtype=torch.bool)
    start[:, 1:] = sk[:, 1:] != sk[:, :-1]
    pos = torch.arange(P, device=dev).expand(N, P)
    grp = torch.where(start, pos, torch.zeros_like(pos)).cummax(dim=1).values   # sorted index of the group's head
    first = torch.empty_like(order)
    first.scatter_(1, order, order.gather(1, grp))                       # (stable sort: the head is the first position)
    return first


def check_pool(idx, table, w, b, pooled, arg, coef=None, chunk_docs=64):
    """Asserts, for every (n, f), with beta = coef * S (coef defaults to fp32_coef(E)):
      - pooled >= 0, |pooled - relu(max_p y64)| <= max(beta at arg, beta at the float64 max);
      - arg == -1 exactly where pooled == 0; arg >= 0 where max y64 - beta > 0; arg == -1 where every y64 + beta <= 0;
      - |pooled - y64[arg]| <= beta[arg]  and  y64[arg] >= max y64 - (beta[arg] + beta at the max);
      - first-max rule: no earlier position than arg has an identical window (so ties resolve to the first position).
    idx [N, T] (its device runs the float64 reference), table [V, E], w [F, 1, 3, E], b [F], pooled [N, F],
    arg [N, F] (any int dtype).  Returns the largest |pooled - y64[arg]| / beta[arg] seen."""
    dev = idx.device
    N, T = idx.shape
    P = T + 2
    E = table.shape[1]
    coef = fp32_coef(E) if coef is None else coef
    pooled = pooled.to(dev, torch.float64)
    arg = arg.to(dev).long()
    assert pooled.shape == arg.shape == (N, w.shape[0]), (pooled.shape, arg.shape)
    assert ((arg >= -1) & (arg < P)).all(), 'argmax outside [-1, T + 2)'
    assert (pooled >= 0).all(), 'negative pooled value'
    assert torch.equal(arg < 0, pooled == 0), _where('arg == -1 exactly where pooled == 0', (arg < 0) != (pooled == 0),
                                                     pooled, arg)
    first = first_identical_window(idx, table)
    worst = 0.0
    for n0, y, S in conv64_chunks(idx, table, w, b, chunk_docs):
        n1 = n0 + y.shape[0]
        pc, a = pooled[n0:n1], arg[n0:n1]
        ac = a.clamp(min=0).unsqueeze(-1)
        beta = coef * S
        ymax, pm = y.max(dim=2)
        beta_m = beta.gather(2, pm.unsqueeze(-1)).squeeze(-1)
        y_a = y.gather(2, ac).squeeze(-1)
        beta_a = torch.where(a >= 0, beta.gather(2, ac).squeeze(-1), torch.zeros_like(beta_m))
        hi = (y + beta).max(dim=2).values
        live = a >= 0

        def fail(what, bad):
            return _where(what, bad, pc, a, n0, ymax=ymax, y_a=y_a, beta_a=beta_a, beta_m=beta_m)
        bad = (pc - ymax.clamp(min=0)).abs() > torch.maximum(beta_a, beta_m)
        assert not bad.any(), fail('|pooled - relu(max y64)| <= beta', bad)
        bad = (ymax - beta_m > 0) & ~live
        assert not bad.any(), fail('max y64 - beta > 0 but arg == -1', bad)
        bad = (hi <= 0) & live
        assert not bad.any(), fail('every y64 + beta <= 0 but arg >= 0', bad)
        bad = live & ((pc - y_a).abs() > beta_a)
        assert not bad.any(), fail('|pooled - y64[arg]| <= beta[arg]', bad)
        bad = live & (y_a < ymax - (beta_a + beta_m))
        assert not bad.any(), fail('y64[arg] within beta[arg] + beta[max] of max y64', bad)
        fa = first[n0:n1].gather(1, a.clamp(min=0))
        bad = live & (fa != a)
        assert not bad.any(), fail('first-max rule: an earlier position has an identical window (first = %s)'
                                   % fa[bad][:8].tolist(), bad)
        if live.any():
            r = ((pc - y_a).abs() / beta_a.clamp(min=1e-300))[live]
            worst = max(worst, float(r.max()))
    return worst


def _where(what, bad, pooled, arg, n0=0, **more):
    nz = bad.nonzero()[:6]
    rows = []
    for n, f in nz.tolist():
        extra = ' '.join('%s=%.9g' % (k, float(v[n, f])) for k, v in more.items())
        rows.append('(n=%d f=%d) pooled=%.9g arg=%d %s' % (n0 + n, f, float(pooled[n, f]), int(arg[n, f]), extra))
    return '%s: %d (n, f) fail, e.g. %s' % (what, int(bad.sum()), '; '.join(rows))


def wgrad64(idx, table, g, arg):
    """Float64 weight gradient GIVEN the kernel's argmax: dW[f, j, :] = sum_n g[n, f] x(n, arg[n, f] - 2 + j) (a zero
    row outside the document), db[f] = sum over arg >= 0 of g[n, f]; and their bounds (N + 2) 2^-24 sum |g x|.
    -> dW [F, 3, E], db [F], bound_w, bound_b (float64, on idx's device)."""
    dev = idx.device
    N, T = idx.shape
    g = g.to(dev, torch.float64)
    a = arg.to(dev).long()
    live = a >= 0
    F = g.shape[1]
    E = table.shape[1]
    dW = torch.zeros((F, 3, E), dtype=torch.float64, device=dev)
    aW = torch.zeros_like(dW)
    for j in range(3):
        t = a - 2 + j
        ok = live & (t >= 0) & (t < T)
        rows = idx.gather(1, t.clamp(0, T - 1))                          # [N, F]
        X = table[rows.to(table.device)].to(dev, torch.float64) * ok.unsqueeze(-1)   # [N, F, E]
        dW[:, j, :] = torch.einsum('nf,nfe->fe', g, X)
        aW[:, j, :] = torch.einsum('nf,nfe->fe', g.abs(), X.abs())
    gl = g * live
    db = gl.sum(0)
    k = (N + 2) * U32
    return dW, db, k * aW, k * gl.abs().sum(0)


def check_wgrad(idx, table, g, arg, d_w, d_b):
    """The kernel's (d_w [F, 1, 3, E], d_b [F]) against wgrad64 at the kernel's own argmax, element by element."""
    dW, db, bw, bb = wgrad64(idx, table, g, arg)
    dev = dW.device
    d_w = _w3(d_w).to(dev, torch.float64)
    d_b = d_b.to(dev, torch.float64)
    ew, eb = (d_w - dW).abs(), (d_b - db).abs()
    assert (ew <= bw).all(), 'd_w: %d elements beyond (N + 2) 2^-24 sum|g x|, worst excess %.3g' % (
        int((ew > bw).sum()), float((ew - bw).max()))
    assert (eb <= bb).all(), 'd_b: %d elements beyond the bound, worst excess %.3g' % (int((eb > bb).sum()), float((eb - bb).max()))
