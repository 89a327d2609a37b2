"""torch.autograd glue over the C ABI (include/r4r.h).

Every Function here is a thin shim: it allocates outputs with torch (device
memory is torch's job), passes raw device pointers to libr4r_hip.so on torch's
current stream, and wires forward/backward together.  No arithmetic on the hot
path is done by PyTorch ops and there is no CPU fallback: tensors must be
fp32/int64, contiguous and on a ROCm device, and a missing library raises.
"""
import torch
from torch.autograd import Function

from . import _lib
from ._lib import call, ptr

NUM_FILTERS_MAX = 112


def _f32(t, name):
    if not t.is_cuda:
        raise RuntimeError('reviews4rec_amd.ops: %s must live on a ROCm device (got %s); the HIP path '
                           'has no CPU fallback' % (name, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError('reviews4rec_amd.ops: %s must be float32, got %s' % (name, t.dtype))
    return t.contiguous()


def _i64(t, name):
    if not t.is_cuda:
        raise RuntimeError('reviews4rec_amd.ops: %s must live on a ROCm device (got %s)' % (name, t.device))
    if t.dtype != torch.int64:
        raise RuntimeError('reviews4rec_amd.ops: %s must be int64 (LongTensor), got %s' % (name, t.dtype))
    return t.contiguous()


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ TextCNN
_PADDED_TABLES = {}     # (data_ptr, shape, _version) of a frozen table -> (weakref to it, its zero-padded device copy)


def _padded_table(table):
    """word_embed_size % 4 != 0 (the reference takes any width, hyper_params.py:64, common_pytorch_models.py:15):
    the kernels read 16-byte aligned rows, so the frozen table gets a cached zero-padded copy; the conv weight is
    padded per call (100 x 3 x E floats) and the pad columns of its gradient -- exactly 0: g * 0 -- are dropped.
    The entry holds a weak reference to the tensor it was made from: a later table of the same shape that the
    allocator places at the same address (a second model built in one process) must not get this one's copy."""
    import weakref
    E = table.shape[1]
    E4 = (E + 3) // 4 * 4
    if E4 == E:
        return table
    key = (table.data_ptr(), tuple(table.shape), table._version)
    hit = _PADDED_TABLES.get(key)
    if hit is not None and hit[0]() is table:
        return hit[1]
    _PADDED_TABLES.clear()                                  # one table per model: no unbounded growth
    pt = torch.zeros((table.shape[0], E4), dtype=table.dtype, device=table.device)
    pt[:, :E].copy_(table.detach())
    _PADDED_TABLES[key] = (weakref.ref(table), pt)
    return pt


def textcnn_fwd_raw(idx, table, conv_w, conv_b):
    """idx [N,T] -> (pooled [N,F] fp32, argmax [N,F] int32).  No autograd."""
    idx, table = _i64(idx, 'idx'), _f32(table, 'table')
    conv_w, conv_b = _f32(conv_w, 'conv_w'), _f32(conv_b, 'conv_b')
    if table.shape[1] % 4:
        E0 = table.shape[1]
        table = _padded_table(table)
        pw = torch.zeros(tuple(conv_w.shape[:-1]) + (table.shape[1],), dtype=conv_w.dtype, device=conv_w.device)
        pw[..., :E0].copy_(conv_w)
        conv_w = pw
    N, T = idx.shape
    V, E = table.shape
    F = conv_b.numel()
    pooled = torch.empty((N, F), dtype=torch.float32, device=idx.device)
    argmax = torch.empty((N, F), dtype=torch.int32, device=idx.device)
    nb = _lib.lib().r4r_textcnn_ws_bytes(N, T, E, F, V)
    ws = _workspace(nb, idx.device)
    call('r4r_textcnn_fwd', ptr(table), V, ptr(idx), ptr(conv_w), ptr(conv_b), ptr(pooled), ptr(argmax),
         ptr(ws), ws.numel(), N, T, E, F)
    return pooled, argmax


def _phrase_weights(weights, N, F):
    """``weights`` of a phrase call as (tensor or None, wt_stride): None, one [F] vector or [N, F]."""
    if weights is None:
        return None, 0
    weights = _f32(weights, 'weights')
    if tuple(weights.shape) == (F,):
        return weights, 0
    if tuple(weights.shape) == (N, F):
        return weights, F
    raise RuntimeError('reviews4rec_amd.ops: weights must be [F] or [N, F] with N = %d, F = %d, got %s'
                       % (N, F, tuple(weights.shape)))


def textcnn_phrases(pooled, argmax, k, T, weights=None, idx=None):
    """r4r_textcnn_phrases (include/r4r.h, "Phrase explanations"): the ``k`` heaviest word windows of every row of
    ``pooled`` [N, F] fp32 / ``argmax`` [N, F] int32 as ``textcnn_fwd_raw`` returns them for documents of ``T`` words.
    ``weights``: None (activation mass), [F] or [N, F] fp32; ``idx`` [N, T] int64: the documents, for the tokens.
    No autograd -> (positions int32 [N, k], scores fp32 [N, k], filters int32 [N, k], tokens int64 [N, k, 3] or None
    without ``idx``, windows int32 [N])."""
    pooled = _f32(pooled, 'pooled')
    if not argmax.is_cuda or argmax.dtype != torch.int32:
        raise RuntimeError('reviews4rec_amd.ops: argmax must be int32 on a ROCm device, got %s on %s'
                           % (argmax.dtype, argmax.device))
    argmax = argmax.contiguous()
    if pooled.dim() != 2 or tuple(argmax.shape) != tuple(pooled.shape):
        raise RuntimeError('reviews4rec_amd.ops: textcnn_phrases takes pooled [N, F] and argmax [N, F], got %s and %s'
                           % (tuple(pooled.shape), tuple(argmax.shape)))
    N, F = (int(d) for d in pooled.shape)
    k, T = int(k), int(T)
    weights, stride = _phrase_weights(weights, N, F)
    if idx is not None:
        idx = _i64(idx, 'idx')
        if tuple(idx.shape) != (N, T):
            raise RuntimeError('reviews4rec_amd.ops: idx must be [N, T] = [%d, %d], got %s' % (N, T, tuple(idx.shape)))
    dev = pooled.device
    rows = max(k, 0)
    pos = torch.empty((N, rows), dtype=torch.int32, device=dev)
    score = torch.empty((N, rows), dtype=torch.float32, device=dev)
    filters = torch.empty((N, rows), dtype=torch.int32, device=dev)
    tokens = torch.empty((N, rows, 3), dtype=torch.int64, device=dev) if idx is not None else None
    windows = torch.empty((N,), dtype=torch.int32, device=dev)
    if N:                                                       # (an empty tensor has no address to pass)
        call('r4r_textcnn_phrases', ptr(pooled), ptr(argmax), ptr(weights), stride, ptr(idx), N, T, F, k, ptr(pos),
             ptr(score), ptr(filters), ptr(tokens), ptr(windows))
    return pos, score, filters, tokens, windows


VARIANT_SLOTS = 64            # r4r_tower_build_variants: a mask removes reviews 0 .. 63 of an owner
VARIANT_MAX_T = 65536         # ... and a document has at most this many words


def _variant_args(pool, ids, drop, occ_off, occ_pos):
    """The pool (tok, rev_off, first, nb -- ``data._Pool.device``'s tuple) and the per-row arguments of the two variant
    entry points, checked: ids int64 [n]; drop int64 [n] or None; occ_off int64 [n + 1] with occ_pos int32, or both
    None."""
    tok, rev_off, first = pool[0], _i64(pool[1], 'rev_off'), _i64(pool[2], 'first')
    if not tok.is_cuda or tok.dtype != torch.int32:
        raise RuntimeError('reviews4rec_amd.ops: tok must be int32 on a ROCm device, got %s on %s' % (tok.dtype, tok.device))
    ids = _i64(ids, 'ids').reshape(-1)
    n = int(ids.numel())
    if drop is not None:
        drop = _i64(drop, 'drop').reshape(-1)
        if drop.numel() != n:
            raise RuntimeError('reviews4rec_amd.ops: drop must be [n] = [%d], got %d masks' % (n, drop.numel()))
    if (occ_off is None) != (occ_pos is None):
        raise RuntimeError('reviews4rec_amd.ops: occ_off and occ_pos come together')
    if occ_off is not None:
        occ_off = _i64(occ_off, 'occ_off').reshape(-1)
        if occ_off.numel() != n + 1:
            raise RuntimeError('reviews4rec_amd.ops: occ_off must be [n + 1] = [%d], got %d' % (n + 1, occ_off.numel()))
        if not occ_pos.is_cuda or occ_pos.dtype != torch.int32:
            raise RuntimeError('reviews4rec_amd.ops: occ_pos must be int32 on a ROCm device, got %s on %s'
                               % (occ_pos.dtype, occ_pos.device))
        occ_pos = occ_pos.contiguous().reshape(-1)
        if occ_pos.numel() == 0:                                # (an empty tensor has no address to pass)
            occ_pos = torch.zeros(1, dtype=torch.int32, device=occ_pos.device)
    return tok.contiguous(), rev_off, first, int(first.numel()) - 1, ids, drop, occ_off, occ_pos, n


def tower_build_variants(pool, ids, T, drop=None, occ_off=None, occ_pos=None):
    """r4r_tower_build_variants (include/r4r.h, "What-if documents"): docs int64 [n, T], row r = the document of owner
    ``ids[r]`` of ``pool`` (the device tuple of ``data._Pool.device``) without the reviews whose bit is set in
    ``drop[r]`` and with word 0 at the positions ``occ_pos[occ_off[r] : occ_off[r + 1]]``.  One launch."""
    tok, rev_off, first, owners, ids, drop, occ_off, occ_pos, n = _variant_args(pool, ids, drop, occ_off, occ_pos)
    docs = torch.empty((n, int(T)), dtype=torch.int64, device=ids.device)
    call('r4r_tower_build_variants', ptr(tok), ptr(rev_off), ptr(first), owners, ptr(ids), ptr(drop), ptr(occ_off),
         ptr(occ_pos), n, int(T), ptr(docs))
    return docs


def tower_span_variants(pool, ids, T, table, conv_w, conv_b, fc_w, fc_b, group, drop=None, occ_off=None, occ_pos=None,
                        want=('latent',)):
    """r4r_tower_span_variants: the tower over the variant documents of ``tower_build_variants``, ``group`` rows per
    round, every launch enqueued from C -> latent [n, L], or with ``want`` naming 'pooled' / 'argmax' as well a dict
    name -> tensor (pooled fp32 [n, F], argmax int32 [n, F]: the rounds' own)."""
    tok, rev_off, first, owners, ids, drop, occ_off, occ_pos, n = _variant_args(pool, ids, drop, occ_off, occ_pos)
    want = tuple(want)
    if 'latent' not in want or set(want) - {'latent', 'pooled', 'argmax'}:
        raise RuntimeError("reviews4rec_amd.ops: tower_span_variants want names 'latent' and any of 'pooled', 'argmax', "
                           'got %r' % (want,))
    table, conv_w, conv_b = _f32(table, 'table'), _f32(conv_w, 'conv_w'), _f32(conv_b, 'conv_b')
    fc_w, fc_b = _f32(fc_w, 'fc_w'), _f32(fc_b, 'fc_b')
    if table.shape[1] % 4:                                      # (textcnn_fwd_raw's padding)
        E0 = table.shape[1]
        table = _padded_table(table)
        pw = torch.zeros(tuple(conv_w.shape[:-1]) + (table.shape[1],), dtype=conv_w.dtype, device=conv_w.device)
        pw[..., :E0].copy_(conv_w)
        conv_w = pw
    V, E = (int(d) for d in table.shape)
    F, L, T, group = int(conv_b.numel()), int(fc_w.shape[0]), int(T), int(group)
    dev = ids.device
    out = {'latent': torch.empty((n, L), dtype=torch.float32, device=dev)}
    if 'pooled' in want:
        out['pooled'] = torch.empty((n, F), dtype=torch.float32, device=dev)
    if 'argmax' in want:
        out['argmax'] = torch.empty((n, F), dtype=torch.int32, device=dev)
    ws = _workspace(_lib.lib().r4r_tower_span_variants_ws_bytes(max(1, min(group, n)), T, E, F, L, V), dev)
    call('r4r_tower_span_variants', ptr(tok), ptr(rev_off), ptr(first), owners, ptr(ids), ptr(drop), ptr(occ_off),
         ptr(occ_pos), n, group, T, ptr(table), V, ptr(conv_w), ptr(conv_b), ptr(fc_w), ptr(fc_b), E, F, L,
         ptr(out['latent']), ptr(out.get('pooled')), ptr(out.get('argmax')), ptr(ws), ws.numel(), None)
    return out['latent'] if want == ('latent',) else out


FOLD_SEARCH_ITEM = 64         # r4r_fold_search_pick: an item review's step number is 64 + its slot
FOLD_SEARCH_MAX_BUDGET = 64


def _fold_pool(pool):
    """The pool's device tuple (``data._Pool.device``) as the fold's three arrays, checked."""
    tok, rev_off, first = pool[0], _i64(pool[1], 'rev_off'), _i64(pool[2], 'first')
    if not tok.is_cuda or tok.dtype != torch.int32:
        raise RuntimeError('reviews4rec_amd.ops: tok must be int32 on a ROCm device, got %s on %s' % (tok.dtype, tok.device))
    return tok.contiguous(), rev_off, first


def _fold_ptab(ptab, conv_b):
    ptab, conv_b = _f32(ptab, 'ptab'), _f32(conv_b, 'conv_b').reshape(-1)
    F = int(conv_b.numel())
    if ptab.dim() != 2 or ptab.shape[1] != _lib.lib().r4r_fold_ptab_stride(F):
        raise RuntimeError('reviews4rec_amd.ops: ptab must be [V, r4r_fold_ptab_stride(%d)], got %s' % (F, tuple(ptab.shape)))
    return ptab, conv_b, F


def fold_project(table, conv_w):
    """r4r_fold_project (include/r4r.h, "Document fold"): ptab [V, PS] fp32, element (v, j, f) at [v, j F + f] =
    sum_k table[v, k] conv_w[f, j, k], for the whole vocabulary of one tower.  One launch; no autograd."""
    table, conv_w = _f32(table, 'table'), _f32(conv_w, 'conv_w')
    if table.shape[1] % 4:                                      # (textcnn_fwd_raw's padding)
        E0 = table.shape[1]
        table = _padded_table(table)
        pw = torch.zeros(tuple(conv_w.shape[:-1]) + (table.shape[1],), dtype=conv_w.dtype, device=conv_w.device)
        pw[..., :E0].copy_(conv_w)
        conv_w = pw
    V, E = (int(d) for d in table.shape)
    F = int(conv_w.shape[0])
    if conv_w.numel() != F * 3 * E:
        raise RuntimeError('reviews4rec_amd.ops: conv_w must hold [F, 3, E] = [%d, 3, %d], got %s' % (F, E, tuple(conv_w.shape)))
    PS = _lib.lib().r4r_fold_ptab_stride(F)
    ptab = torch.zeros((V, max(PS, 1)), dtype=torch.float32, device=table.device)
    call('r4r_fold_project', ptr(table), V, ptr(conv_w), ptr(ptab), E, F)
    return ptab


def fold_segments(ptab, conv_b, pool, ids, S):
    """r4r_fold_segments: seg fp32 [n, S, F], per owner ``ids[i]`` of ``pool`` and review slot s < S the maximum over
    the windows that lie inside the review (-inf: fewer than three words, or no such review).  One launch."""
    ptab, conv_b, F = _fold_ptab(ptab, conv_b)
    tok, rev_off, first = _fold_pool(pool)
    ids = _i64(ids, 'ids').reshape(-1)
    n, S = int(ids.numel()), int(S)
    seg = torch.empty((n, max(S, 0), F), dtype=torch.float32, device=ids.device)
    call('r4r_fold_segments', ptr(ptab), ptr(conv_b), ptr(tok), ptr(rev_off), ptr(first), ptr(ids) if n else None, n, S, F,
         ptr(seg) if n else None)
    return seg


def fold_compose(ptab, conv_b, seg, pool, row_owner, ids, T, drop=None):
    """r4r_fold_compose: pooled fp32 [M, F], row m = the tower's pooled features of the document of owner
    ``ids[row_owner[m]]`` without the reviews of ``drop[m]`` (int64 [M] or None), from ``seg`` [n, S, F] of the same
    ``ids``; a negative ``row_owner[m]`` gives a row of zeros.  One launch."""
    ptab, conv_b, F = _fold_ptab(ptab, conv_b)
    tok, rev_off, first = _fold_pool(pool)
    ids, row_owner, seg = _i64(ids, 'ids').reshape(-1), _i64(row_owner, 'row_owner').reshape(-1), _f32(seg, 'seg')
    n, M = int(ids.numel()), int(row_owner.numel())
    if seg.dim() != 3 or seg.shape[0] != n or seg.shape[2] != F:
        raise RuntimeError('reviews4rec_amd.ops: seg must be [n, S, F] = [%d, S, %d], got %s' % (n, F, tuple(seg.shape)))
    if drop is not None:
        drop = _i64(drop, 'drop').reshape(-1)
        if drop.numel() != M:
            raise RuntimeError('reviews4rec_amd.ops: drop must be [M] = [%d], got %d masks' % (M, drop.numel()))
    pooled = torch.empty((M, F), dtype=torch.float32, device=row_owner.device)
    if M:                                                       # (an empty tensor has no address to pass)
        call('r4r_fold_compose', ptr(ptab), ptr(conv_b), ptr(seg), int(seg.shape[1]), ptr(tok), ptr(rev_off), ptr(first),
             ptr(row_owner), ptr(ids), ptr(drop), M, int(T), F, ptr(pooled))
    return pooled


def fold_latents(side, row_owner, T, drop=None, out=None):
    """compose + the tower's fc for one side -> latent [M, L] (into ``out`` when given).  ``side``: a dict with ptab,
    conv_b, seg, pool, ids, fc_w, fc_b."""
    pooled = fold_compose(side['ptab'], side['conv_b'], side['seg'], side['pool'], row_owner, side['ids'], T, drop=drop)
    fc_w, fc_b = _f32(side['fc_w'], 'fc_w'), _f32(side['fc_b'], 'fc_b')
    M, (L, F) = int(pooled.shape[0]), (int(d) for d in fc_w.shape)
    if out is None:
        out = torch.empty((M, L), dtype=torch.float32, device=pooled.device)
    if M:
        call('r4r_linear_fwd', ptr(pooled), ptr(fc_w), ptr(fc_b), ptr(out), M, F, L, 0)
    return out


def fold_search(kind, head, side_u, side_i, own_u, own_i, target, direction, budget, T, start_u=None, start_i=None,
                cand_u=None, cand_i=None):
    """The fewest-review greedy search of include/r4r.h, "Document fold", over the pairs p = (own_u[p], own_i[p]) --
    indices into the sides' ``ids`` -> (order int32 [n_p, B], scores fp32 [n_p, B + 1], steps int32 [n_p], crossed
    int32 [n_p]).

    ``side_u`` / ``side_i``: dicts with ptab, conv_b, seg [n, S, F], pool, ids, fc_w, fc_b of the side's tower.
    ``kind`` / ``head``: ``pair_grad``'s kind and parameters, the per-row ones (q_bias, xu; c_bias, xi) PER PAIR.
    ``target`` fp32 [n_p]; ``direction`` 0 down / 1 up; ``budget`` 1 .. 64.  ``start_*`` int64 [n_p] (None = 0): the
    reviews already removed; ``cand_*`` int64 [n_p] (None: the side is not searched): the slots that may be removed,
    bits at or beyond the side's S ignored.  ``budget`` steps of fixed shape are enqueued -- r4r_fold_search_rows,
    compose + fc per searched side, one r4r_pair_grad over [the pairs' current rows ; the candidate rows],
    r4r_fold_search_pick -- and the host reads nothing in between."""
    if kind not in PAIR_GRAD_KINDS:
        raise RuntimeError('reviews4rec_amd.ops: fold_search kind must be one of %r, got %r' % (tuple(PAIR_GRAD_KINDS), kind))
    direction, B, T = int(direction), int(budget), int(T)
    own_u, own_i = _i64(own_u, 'own_u').reshape(-1), _i64(own_i, 'own_i').reshape(-1)
    target = _f32(target, 'target').reshape(-1)
    n_p, dev = int(own_u.numel()), own_u.device
    if own_i.numel() != n_p or target.numel() != n_p:
        raise RuntimeError('reviews4rec_amd.ops: fold_search takes equally long own_u, own_i and target, got %d, %d and %d'
                           % (n_p, own_i.numel(), target.numel()))
    masks = {}
    for name, m in (('start_u', start_u), ('start_i', start_i), ('cand_u', cand_u), ('cand_i', cand_i)):
        if m is not None:
            m = _i64(m, name).reshape(-1)
            if m.numel() != n_p:
                raise RuntimeError('reviews4rec_amd.ops: %s must be [n_p] = [%d], got %d masks' % (name, n_p, m.numel()))
        masks[name] = m
    order = torch.empty((n_p, max(B, 0)), dtype=torch.int32, device=dev)
    scores = torch.empty((n_p, max(B, 0) + 1), dtype=torch.float32, device=dev)
    steps = torch.empty((n_p,), dtype=torch.int32, device=dev)
    crossed = torch.empty((n_p,), dtype=torch.int32, device=dev)
    done = torch.empty((n_p,), dtype=torch.int32, device=dev)
    S_u = int(side_u['seg'].shape[1]) if masks['cand_u'] is not None else 0
    S_i = int(side_i['seg'].shape[1]) if masks['cand_i'] is not None else 0
    C = S_u + S_i
    if C == 0:
        raise RuntimeError('reviews4rec_amd.ops: fold_search needs cand_u or cand_i: no side to search')
    if n_p == 0:                                                # (the limits are still checked)
        call('r4r_fold_search_begin', None, None, direction, B, 0, None, None, None, None, None)
        return order, scores, steps, crossed
    L = int(side_u['fc_w'].shape[0])
    rows = n_p + n_p * C
    pairs = torch.arange(n_p, dtype=torch.int64, device=dev)
    cols = torch.arange(C, dtype=torch.int64, device=dev)
    cand_rows = (n_p + pairs[:, None] * C + cols[None, :])
    every = lambda: pairs[:, None].expand(n_p, C)
    # the pairs' current rows, then the candidate rows; a side that is not searched keeps the current rows alone
    idx_u = torch.where(cols[None, :] < S_u, cand_rows, every()).reshape(-1).contiguous()
    idx_i = torch.where(cols[None, :] >= S_u, cand_rows, every()).reshape(-1).contiguous()
    z_u = torch.zeros((rows if S_u else n_p, L), dtype=torch.float32, device=dev)
    z_i = torch.zeros((rows if S_i else n_p, L), dtype=torch.float32, device=dev)
    spread = lambda t, on: torch.cat([t, t.repeat_interleave(C, 0)]).contiguous() if on else t.contiguous()
    per_row = {'q_bias': S_u, 'xu': S_u, 'c_bias': S_i, 'xi': S_i}
    head_c = {k: (spread(v, per_row[k]) if k in per_row and v is not None else v) for k, v in head.items()}
    mask_u = (masks['start_u'] if masks['start_u'] is not None else torch.zeros(n_p, dtype=torch.int64, device=dev)).clone()
    mask_i = (masks['start_i'] if masks['start_i'] is not None else torch.zeros(n_p, dtype=torch.int64, device=dev)).clone()
    fold_latents(side_u, own_u, T, drop=mask_u, out=z_u[:n_p])
    fold_latents(side_i, own_i, T, drop=mask_i, out=z_i[:n_p])
    score0 = pair_grad(kind, z_u, z_i, pairs, pairs, want=('score',), **head_c)['score']
    call('r4r_fold_search_begin', ptr(score0), ptr(target), direction, B, n_p, ptr(order), ptr(scores), ptr(steps),
         ptr(crossed), ptr(done))
    i64 = lambda on: torch.empty((n_p, C), dtype=torch.int64, device=dev) if on else None
    ro_u, dr_u, ro_i, dr_i = i64(S_u), i64(S_u), i64(S_i), i64(S_i)
    pu, pi = _fold_pool(side_u['pool']), _fold_pool(side_i['pool'])
    ids_u, ids_i = _i64(side_u['ids'], 'ids').reshape(-1), _i64(side_i['ids'], 'ids').reshape(-1)
    for _ in range(B):
        call('r4r_fold_search_rows', ptr(pu[1]), ptr(pu[2]), ptr(ids_u), ptr(own_u), ptr(mask_u), ptr(masks['cand_u']), S_u,
             ptr(pi[1]), ptr(pi[2]), ptr(ids_i), ptr(own_i), ptr(mask_i), ptr(masks['cand_i']), S_i, ptr(done), n_p, T,
             ptr(ro_u), ptr(dr_u), ptr(ro_i), ptr(dr_i))
        if S_u:
            fold_latents(side_u, ro_u, T, drop=dr_u, out=z_u[n_p:])
        if S_i:
            fold_latents(side_i, ro_i, T, drop=dr_i, out=z_i[n_p:])
        cand_score = pair_grad(kind, z_u, z_i, idx_u, idx_i, want=('score',), **head_c)['score']
        call('r4r_fold_search_pick', ptr(cand_score), ptr(ro_u), ptr(ro_i), S_u, S_i, ptr(target), direction, B, n_p,
             ptr(mask_u), ptr(mask_i), ptr(z_u), ptr(z_i), L, ptr(order), ptr(scores), ptr(steps), ptr(crossed), ptr(done))
    return order, scores, steps, crossed


PAIR_GRAD_KINDS = {'fm': 0, 'mlp': 1, 'pfm': 2}              # R4R_PAIR_GRAD_* of include/r4r.h
PAIR_GRAD_OUTPUTS = ('score', 'g_user', 'g_item', 'w_user', 'w_item')
_PAIR_GRAD_PARAMS = {'fm': ('V', 'lw'), 'mlp': ('W0', 'b0', 'w3'), 'pfm': ('W0', 'b0', 'W2', 'b2', 'V', 'lw')}


def pair_grad(kind, zu, zi, u_idx, i_idx, q_bias=None, c_bias=None, W0=None, b0=None, W2=None, b2=None, w3=None, V=None,
              lw=None, xu=None, xi=None, fc_u=None, fc_i=None, want=PAIR_GRAD_OUTPUTS):
    """r4r_pair_grad (include/r4r.h, "Pair gradients"): for the pairs (u_idx[p], i_idx[p]) over the eval-mode tower
    latents ``zu`` [n_u, L] / ``zi`` [n_i, L], the prediction, its gradient with respect to both latents and that
    gradient carried back through ``fc_u`` / ``fc_i`` [L, F] (the towers' fc.weight) to the pooled features.

    ``kind``: 'fm' (deepconn: ``V`` [2L, 8], ``lw`` [2L]), 'mlp' (deepconn++: ``W0`` [L, 2L], ``b0`` [L], ``w3`` [L]) or
    'pfm' (transnet(++): ``W0``, ``b0``, ``W2`` [L, L], ``b2`` [L], ``V`` [2P + L, 8], ``lw`` [2P + L] and, with P > 0,
    the id-embedding rows ``xu`` [n_u, P] / ``xi`` [n_i, P]).  ``q_bias`` [n_u] / ``c_bias`` [n_i]: the score's scalars,
    None = 0.  ``want``: the outputs to compute, names of ``PAIR_GRAD_OUTPUTS``.  No autograd
    -> a dict name -> tensor: score [n_p], g_user / g_item [n_p, L], w_user / w_item [n_p, F]."""
    if kind not in PAIR_GRAD_KINDS:
        raise RuntimeError('reviews4rec_amd.ops: pair_grad kind must be one of %r, got %r' % (tuple(PAIR_GRAD_KINDS), kind))
    want = tuple(want)
    if not want or set(want) - set(PAIR_GRAD_OUTPUTS):
        raise RuntimeError('reviews4rec_amd.ops: pair_grad want must name some of %r, got %r' % (PAIR_GRAD_OUTPUTS, want))
    zu, zi = _f32(zu, 'zu'), _f32(zi, 'zi')
    u_idx, i_idx = _i64(u_idx, 'u_idx').reshape(-1), _i64(i_idx, 'i_idx').reshape(-1)
    if zu.dim() != 2 or zi.dim() != 2 or zu.shape[1] != zi.shape[1] or u_idx.numel() != i_idx.numel():
        raise RuntimeError('reviews4rec_amd.ops: pair_grad takes zu [n_u, L], zi [n_i, L] and equally long u_idx / i_idx, '
                           'got %s, %s, %d and %d' % (tuple(zu.shape), tuple(zi.shape), u_idx.numel(), i_idx.numel()))
    n_u, n_i, L, n_p = int(zu.shape[0]), int(zi.shape[0]), int(zu.shape[1]), int(u_idx.numel())
    given = dict(W0=W0, b0=b0, W2=W2, b2=b2, w3=w3, V=V, lw=lw, xu=xu, xi=xi, fc_u=fc_u, fc_i=fc_i, q_bias=q_bias,
                 c_bias=c_bias)
    given = {k: None if v is None else _f32(v, k) for k, v in given.items()}
    P = 0
    if kind == 'pfm' and given['xu'] is not None:
        P = int(given['xu'].shape[1])
    n = 2 * L if kind == 'fm' else 2 * P + L
    shapes = dict(W0=(L, 2 * L), b0=(L,), W2=(L, L), b2=(L,), w3=(L,), V=(n, 8), lw=(n,), xu=(n_u, P), xi=(n_i, P),
                  q_bias=(n_u,), c_bias=(n_i,))
    for name in _PAIR_GRAD_PARAMS[kind]:
        if given[name] is None:
            raise RuntimeError('reviews4rec_amd.ops: pair_grad kind %r needs %s' % (kind, name))
    for name, shape in shapes.items():
        t = given[name]
        if t is not None and name in ('w3', 'lw', 'b0', 'b2', 'q_bias', 'c_bias'):
            t = given[name] = t.reshape(-1)
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError('reviews4rec_amd.ops: pair_grad %s must be %s, got %s' % (name, shape, tuple(t.shape)))
    F = 1
    for name, out in (('fc_u', 'w_user'), ('fc_i', 'w_item')):
        t = given[name]
        if t is None:
            if out in want:
                raise RuntimeError('reviews4rec_amd.ops: pair_grad %s needs %s' % (out, name))
        elif t.dim() != 2 or t.shape[0] != L:
            raise RuntimeError('reviews4rec_amd.ops: pair_grad %s must be [L, F] = [%d, F], got %s' % (name, L, tuple(t.shape)))
        else:
            F = int(t.shape[1])
    if given['fc_u'] is not None and given['fc_i'] is not None and given['fc_u'].shape != given['fc_i'].shape:
        raise RuntimeError('reviews4rec_amd.ops: pair_grad fc_u and fc_i must share a shape')
    dev = zu.device
    sizes = dict(score=(n_p,), g_user=(n_p, L), g_item=(n_p, L), w_user=(n_p, F), w_item=(n_p, F))
    out = {name: torch.empty(sizes[name], dtype=torch.float32, device=dev) for name in PAIR_GRAD_OUTPUTS if name in want}
    g = given
    call('r4r_pair_grad', PAIR_GRAD_KINDS[kind], ptr(zu), n_u, ptr(zi), n_i, ptr(u_idx), ptr(i_idx), n_p, ptr(g['q_bias']),
         ptr(g['c_bias']), ptr(g['W0']), ptr(g['b0']), ptr(g['W2']), ptr(g['b2']), ptr(g['w3']), ptr(g['V']), ptr(g['lw']),
         ptr(g['xu']) if P else None, ptr(g['xi']) if P else None, P, ptr(g['fc_u']), ptr(g['fc_i']), L, F,
         *(ptr(out.get(name)) for name in PAIR_GRAD_OUTPUTS))
    return out


def textcnn_wgrad_raw(idx, table, g_pooled, argmax, conv_w_shape):
    idx, table, g_pooled = _i64(idx, 'idx'), _f32(table, 'table'), _f32(g_pooled, 'g_pooled')
    E_model = table.shape[1]
    table = _padded_table(table)
    conv_w_shape = tuple(conv_w_shape[:-1]) + (table.shape[1],)
    N, T = idx.shape
    V, E = table.shape
    F = g_pooled.shape[1]
    d_w = torch.empty(conv_w_shape, dtype=torch.float32, device=idx.device)
    d_b = torch.empty((F,), dtype=torch.float32, device=idx.device)
    nb = _lib.lib().r4r_textcnn_ws_bytes(N, T, E, F, V)
    ws = _workspace(nb, idx.device)
    call('r4r_textcnn_wgrad', ptr(table), V, ptr(idx), ptr(g_pooled), ptr(argmax), ptr(d_w), ptr(d_b),
         ptr(ws), ws.numel(), N, T, E, F)
    if E != E_model:
        d_w = d_w[..., :E_model].contiguous()
    return d_w, d_b


class TextCNNPool(Function):
    """pooled[n,f] = max_p relu(conv(word2vec[idx[n]]))[f,p]  (frozen table: no grad to it)."""

    @staticmethod
    def forward(ctx, idx, table, conv_w, conv_b):
        pooled, argmax = textcnn_fwd_raw(idx, table, conv_w, conv_b)
        ctx.save_for_backward(idx, table, argmax)
        ctx.w_shape = tuple(conv_w.shape)
        ctx.mark_non_differentiable(argmax)
        return pooled, argmax

    @staticmethod
    def backward(ctx, g_pooled, _g_arg):
        idx, table, argmax = ctx.saved_tensors
        d_w, d_b = textcnn_wgrad_raw(idx, table, g_pooled, argmax, ctx.w_shape)
        return None, None, d_w, d_b


# ------------------------------------------------------------------- linear
class Linear(Function):
    @staticmethod
    def forward(ctx, x, w, b, relu):
        x, w, b = _f32(x, 'x'), _f32(w, 'w'), _f32(b, 'b')
        lead = x.shape[:-1]
        n_in, n_out = x.shape[-1], w.shape[0]
        x2 = x.reshape(-1, n_in)
        y = torch.empty((x2.shape[0], n_out), dtype=torch.float32, device=x.device)
        call('r4r_linear_fwd', ptr(x2), ptr(w), ptr(b), ptr(y), x2.shape[0], n_in, n_out, int(relu))
        ctx.save_for_backward(x2, w, y)
        ctx.relu, ctx.lead = bool(relu), lead
        ctx.need_gx = ctx.needs_input_grad[0]
        return y.view(*lead, n_out)

    @staticmethod
    def backward(ctx, g_y):
        x2, w, y = ctx.saved_tensors
        n_in, n_out = x2.shape[1], w.shape[0]
        g_y = _f32(g_y, 'g_y').reshape(-1, n_out)
        g_x = torch.empty_like(x2) if ctx.need_gx else None
        g_w = torch.empty_like(w)
        g_b = torch.empty((n_out,), dtype=torch.float32, device=w.device)
        nb = _lib.lib().r4r_linear_bwd_ws_bytes(x2.shape[0], n_in, n_out)
        ws = _workspace(nb, w.device) if nb else None
        call('r4r_linear_bwd', ptr(x2), ptr(w), ptr(y), ptr(g_y), ptr(g_x), ptr(g_w), ptr(g_b),
             ptr(ws), nb, x2.shape[0], n_in, n_out, int(ctx.relu))
        return (g_x.view(*ctx.lead, n_in) if g_x is not None else None), g_w, g_b, None


def linear(x, weight, bias, relu=False):
    return Linear.apply(x, weight, bias, relu)


# ------------------------------------------------------------------ dropout
class DropoutState:
    """Philox stream position for the dropout kernels (per process / per rank).

    Eager mode keeps the position on the host (``offset``).  For hipGraph capture
    (``device_counter`` set, see graph.py) it lives in a device int64 tensor that the dropout
    launch itself advances, so every replay of a captured step draws fresh masks."""
    seed = 0x5EED5EED
    offset = 0
    record = None          # dict: site -> multiplier tensor, when a test wants the masks
    device_counter = None  # torch int64 [1] on the device, or None

    @classmethod
    def manual_seed(cls, seed, rank=0):
        cls.seed = (int(seed) * 0x9E3779B97F4A7C15 + int(rank) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        cls.offset = 0
        if cls.device_counter is not None:
            cls.device_counter.zero_()

    @classmethod
    def draw(cls, x, y, mult, p):
        """Launch the dropout kernel on x -> (y, mult) and advance the stream position."""
        n = x.numel()
        if cls.device_counter is not None:
            call('r4r_dropout_fwd', ptr(x), ptr(y), ptr(mult), n, float(p), cls.seed, 0, ptr(cls.device_counter))
        else:
            call('r4r_dropout_fwd', ptr(x), ptr(y), ptr(mult), n, float(p), cls.seed, cls.offset, None)
            cls.offset += (n + 3) // 4


class Dropout(Function):
    @staticmethod
    def forward(ctx, x, p, site):
        x = _f32(x, 'x')
        y = torch.empty_like(x)
        mult = torch.empty_like(x)
        DropoutState.draw(x, y, mult, p)
        if DropoutState.record is not None and site is not None:
            DropoutState.record[site] = mult
        ctx.save_for_backward(mult)
        return y

    @staticmethod
    def backward(ctx, g_y):
        (mult,) = ctx.saved_tensors
        g_y = _f32(g_y, 'g_y')
        g_x = torch.empty_like(g_y)
        call('r4r_mul', ptr(g_y), ptr(mult), ptr(g_x), g_y.numel())
        return g_x, None, None


def dropout(x, p, training, site=None):
    """nn.Dropout semantics; identity in eval mode or at p == 0 (no kernel launched)."""
    if not training or p == 0.0:
        return x
    return Dropout.apply(x, p, site)


class Mul(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, 'a'), _f32(b, 'b')
        out = torch.empty_like(a)
        call('r4r_mul', ptr(a), ptr(b), ptr(out), a.numel())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _f32(g, 'g')
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        call('r4r_mul', ptr(g), ptr(b), ptr(ga), g.numel())
        call('r4r_mul', ptr(g), ptr(a), ptr(gb), g.numel())
        return ga, gb


class Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, 'a'), _f32(b, 'b')
        out = torch.empty_like(a)
        call('r4r_add', ptr(a), ptr(b), ptr(out), a.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def mul(a, b):
    return Mul.apply(a, b)


def add(a, b):
    return Add.apply(a, b)


# ----------------------------------------------------------------------- FM
class FM(Function):
    """TorchFM without global bias: x [N,n] -> [N]."""

    @staticmethod
    def forward(ctx, x, V, lin_w, lin_b):
        x, V, lin_w, lin_b = _f32(x, 'x'), _f32(V, 'V'), _f32(lin_w, 'lin_w'), _f32(lin_b, 'lin_b')
        N, n = x.shape
        k = V.shape[1]
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
        call('r4r_fm_fwd', ptr(x), ptr(V), ptr(lin_w), ptr(lin_b), ptr(out), N, n, k)
        ctx.save_for_backward(x, V, lin_w)
        ctx.lw_shape = tuple(lin_w.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, V, lin_w = ctx.saved_tensors
        N, n = x.shape
        k = V.shape[1]
        g_out = _f32(g_out, 'g_out')
        g_x, g_V = torch.empty_like(x), torch.empty_like(V)
        g_lw = torch.empty(ctx.lw_shape, dtype=torch.float32, device=x.device)
        g_lb = torch.empty((1,), dtype=torch.float32, device=x.device)
        call('r4r_fm_bwd', ptr(x), ptr(V), ptr(lin_w), ptr(g_out), ptr(g_x), ptr(g_V), ptr(g_lw), ptr(g_lb), N, n, k)
        return g_x, g_V, g_lw, g_lb


def fm(x, V, lin_w, lin_b):
    return FM.apply(x, V, lin_w, lin_b)


# ------------------------------------------------------- embeddings / biases
class SparseGradCapture:
    """Data-parallel mode for ID tables / bias vectors (dist.DataParallel turns it on).

    When ``active`` the backward of an embedding / bias gather does NOT build the dense table
    gradient; it records the compact contribution ``(row ids, gradient rows)`` under the table's
    storage address and hands autograd an uninitialised placeholder.  DataParallel all-gathers the
    compact lists and rebuilds the identical dense gradient on every rank
    (``rebuild_dense``), so a dense table gradient never crosses xGMI."""
    active = False
    contributions = {}          # table.data_ptr() -> list[(idx [n] int64, g [n, D] fp32)]

    @classmethod
    def record(cls, table_ptr, idx, g):
        cls.contributions.setdefault(table_ptr, []).append((idx, g))

    @classmethod
    def clear(cls):
        cls.contributions = {}


def rebuild_dense(idx, g, R, D, out=None):
    """Dense [R, D] gradient from a compact list, deterministic summation order."""
    idx, g = _i64(idx, 'idx').reshape(-1), _f32(g, 'g').reshape(-1, D)
    if out is None:
        out = torch.empty((R, D), dtype=torch.float32, device=g.device)
    call('r4r_embed_scatter_add_ordered', ptr(g), ptr(idx), ptr(out), R, D, idx.numel())
    return out


class EmbedGather(Function):
    """rows = table[idx]; backward is the reference's DENSE table gradient."""

    @staticmethod
    def forward(ctx, table, idx):
        table, idx = _f32(table, 'table'), _i64(idx, 'idx')
        R, D = table.shape
        flat = idx.reshape(-1)
        out = torch.empty((flat.numel(), D), dtype=torch.float32, device=table.device)
        call('r4r_embed_gather', ptr(table), ptr(flat), ptr(out), R, D, flat.numel())
        ctx.save_for_backward(flat)
        ctx.shape = (R, D)
        ctx.table_ptr = table.data_ptr()
        return out.view(*idx.shape, D)

    @staticmethod
    def backward(ctx, g):
        (flat,) = ctx.saved_tensors
        R, D = ctx.shape
        g = _f32(g, 'g').reshape(-1, D)
        g_table = torch.empty((R, D), dtype=torch.float32, device=g.device)
        if SparseGradCapture.active:
            SparseGradCapture.record(ctx.table_ptr, flat, g)   # dense gradient rebuilt after the exchange
            return g_table, None
        call('r4r_embed_scatter_add', ptr(g), ptr(flat), ptr(g_table), R, D, flat.numel())
        return g_table, None


def embed(table, idx):
    return EmbedGather.apply(table, idx)


class RowDot(Function):
    @staticmethod
    def forward(ctx, a, c):
        a, c = _f32(a, 'a'), _f32(c, 'c')
        N, D = a.shape
        out = torch.empty((N,), dtype=torch.float32, device=a.device)
        call('r4r_rowdot_fwd', ptr(a), ptr(c), ptr(out), N, D)
        ctx.save_for_backward(a, c)
        return out

    @staticmethod
    def backward(ctx, g):
        a, c = ctx.saved_tensors
        g = _f32(g, 'g')
        ga, gc = torch.empty_like(a), torch.empty_like(c)
        call('r4r_rowdot_bwd', ptr(a), ptr(c), ptr(g), ptr(ga), ptr(gc), a.shape[0], a.shape[1])
        return ga, gc


def rowdot(a, c):
    return RowDot.apply(a, c)


class BiasHead(Function):
    """out = (r +) user_bias[uid] + item_bias[iid] + global_bias; with user_bias None: r + global_bias."""

    @staticmethod
    def forward(ctx, r, user_bias, item_bias, global_bias, uid, iid):
        global_bias = _f32(global_bias, 'global_bias')
        ctx.has_ids = user_bias is not None
        if ctx.has_ids:
            user_bias, item_bias = _f32(user_bias, 'user_bias'), _f32(item_bias, 'item_bias')
            uid, iid = _i64(uid, 'uid').reshape(-1), _i64(iid, 'iid').reshape(-1)
            N = uid.numel()
            ctx.save_for_backward(uid, iid)
            ctx.sizes = (user_bias.numel(), item_bias.numel())
            ctx.ptrs = (user_bias.data_ptr(), item_bias.data_ptr())
        if r is not None:
            r = _f32(r, 'r')
            N = r.numel()
        out = torch.empty((N,), dtype=torch.float32, device=global_bias.device)
        call('r4r_bias_head_fwd', ptr(r), ptr(user_bias), ptr(item_bias), ptr(global_bias), ptr(uid), ptr(iid),
             ptr(out), N)
        ctx.has_r = r is not None
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32(g, 'g')
        g_gb = torch.empty((1,), dtype=torch.float32, device=g.device)
        g_ub = g_ib = uid = iid = None
        RU = RI = 0
        if ctx.has_ids:
            uid, iid = ctx.saved_tensors
            RU, RI = ctx.sizes
            g_ub = torch.empty((RU,), dtype=torch.float32, device=g.device)
            g_ib = torch.empty((RI,), dtype=torch.float32, device=g.device)
            if SparseGradCapture.active:
                SparseGradCapture.record(ctx.ptrs[0], uid, g.reshape(-1, 1))
                SparseGradCapture.record(ctx.ptrs[1], iid, g.reshape(-1, 1))
                call('r4r_bias_head_bwd', ptr(g), None, None, None, None, ptr(g_gb), 0, 0, g.numel())
                return (g if ctx.has_r else None), g_ub, g_ib, g_gb, None, None
        call('r4r_bias_head_bwd', ptr(g), ptr(uid), ptr(iid), ptr(g_ub), ptr(g_ib), ptr(g_gb), RU, RI, g.numel())
        return (g if ctx.has_r else None), g_ub, g_ib, g_gb, None, None


def bias_head(r, user_bias, item_bias, global_bias, uid, iid):
    return BiasHead.apply(r, user_bias, item_bias, global_bias, uid, iid)


# ---------------------------------------------------------- NARRE attention
class NarreAttention(Function):
    @staticmethod
    def forward(ctx, x, other, W0, b0, w3, b3, p, training, site):
        x, other = _f32(x, 'x'), _f32(other, 'other')
        W0, b0, w3, b3 = _f32(W0, 'W0'), _f32(b0, 'b0'), _f32(w3, 'w3'), _f32(b3, 'b3')
        N, R, L = x.shape
        mult = None
        if training and p > 0.0:
            # the scorer's dropout multiplier, drawn by the same Philox kernel as every other site
            ones = torch.ones((N, R, L), dtype=torch.float32, device=x.device)
            mult = torch.empty_like(ones)
            scratch = torch.empty_like(ones)
            DropoutState.draw(ones, scratch, mult, p)
            if DropoutState.record is not None and site is not None:
                DropoutState.record[site] = mult
        out = torch.empty((N, L), dtype=torch.float32, device=x.device)
        h = torch.empty((N, R, L), dtype=torch.float32, device=x.device)
        a = torch.empty((N, R), dtype=torch.float32, device=x.device)
        call('r4r_narre_attn_fwd', ptr(x), ptr(other), ptr(W0), ptr(b0), ptr(w3), ptr(b3), ptr(mult),
             ptr(out), ptr(h), ptr(a), N, R, L)
        ctx.save_for_backward(x, other, W0, w3, h, a)
        ctx.mult = mult
        ctx.w3_shape = tuple(w3.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, other, W0, w3, h, a = ctx.saved_tensors
        N, R, L = x.shape
        g_out = _f32(g_out, 'g_out')
        g_x, g_other = torch.empty_like(x), torch.empty_like(other)
        g_W0 = torch.empty_like(W0)
        g_b0 = torch.empty((L,), dtype=torch.float32, device=x.device)
        g_w3 = torch.empty(ctx.w3_shape, dtype=torch.float32, device=x.device)
        g_b3 = torch.empty((1,), dtype=torch.float32, device=x.device)
        ws = _workspace(_lib.lib().r4r_narre_attn_ws_bytes(N, R, L), x.device)
        call('r4r_narre_attn_bwd', ptr(x), ptr(other), ptr(W0), ptr(w3), ptr(ctx.mult), ptr(h), ptr(a), ptr(g_out),
             ptr(g_x), ptr(g_other), ptr(g_W0), ptr(g_b0), ptr(g_w3), ptr(g_b3), ptr(ws), ws.numel(), N, R, L)
        return g_x, g_other, g_W0, g_b0, g_w3, g_b3, None, None, None


def narre_attention(x, other, W0, b0, w3, b3, p=0.0, training=False, site=None):
    return NarreAttention.apply(x, other, W0, b0, w3, b3, p, training, site)


def narre_explain(z, nb, other_table, W0, b0, w3, b3, own_table=None, owner=None, live=None, k=0, want_out=True,
                  want_attn=True):
    """r4r_narre_explain (include/r4r.h, "NARRE explanations"): the eval-mode attention over review latents ``z``
    [N, R, L] weighed by the rows ``nb`` [N, R] (int64) of ``other_table`` [rows, L], R and L up to 64, forward only and
    without autograd -> (out [N, L] or None, attn [N, R] or None, top_slot int32 [N, k] or None, top_w [N, k] or None).
    ``own_table`` with ``owner`` (int64 [N], rows of it): out += own_table[owner].  ``live`` (int32 [N]): the slots
    that may be listed, the first live[n] of each owner; None: all R."""
    z, other_table = _f32(z, 'z'), _f32(other_table, 'other_table')
    W0, b0, w3, b3 = _f32(W0, 'W0'), _f32(b0, 'b0'), _f32(w3, 'w3'), _f32(b3, 'b3')
    nb = _i64(nb, 'nb')
    if z.dim() != 3 or tuple(nb.shape) != tuple(z.shape[:2]):
        raise RuntimeError('reviews4rec_amd.ops: narre_explain takes z [N, R, L] and nb [N, R], got %s and %s'
                           % (tuple(z.shape), tuple(nb.shape)))
    N, R, L = (int(d) for d in z.shape)
    if other_table.dim() != 2 or other_table.shape[1] != L or tuple(W0.shape) != (L, 2 * L) or b0.numel() != L \
            or w3.numel() != L or b3.numel() != 1:
        raise RuntimeError('reviews4rec_amd.ops: narre_explain: other_table [*, L], W0 [L, 2L], b0 [L], w3 [L], b3 [1] '
                           'with L = %d expected' % L)
    if (own_table is None) != (owner is None):
        raise RuntimeError('reviews4rec_amd.ops: narre_explain: own_table and owner go together')
    if own_table is not None:
        own_table, owner = _f32(own_table, 'own_table'), _i64(owner, 'owner')
        if own_table.dim() != 2 or own_table.shape[1] != L or owner.numel() != N:
            raise RuntimeError('reviews4rec_amd.ops: narre_explain: own_table [*, L] and owner [N] expected')
        if N and (int(owner.min()) < 0 or int(owner.max()) >= own_table.shape[0]):
            raise RuntimeError('reviews4rec_amd.ops: narre_explain: owner outside own_table\'s %d rows' % own_table.shape[0])
    if live is not None:
        if not live.is_cuda or live.dtype != torch.int32 or live.numel() != N:
            raise RuntimeError('reviews4rec_amd.ops: live must be int32 [N] on a ROCm device')
        live = live.contiguous()
    k = int(k)
    dev = z.device
    out = torch.empty((N, L), dtype=torch.float32, device=dev) if want_out else None
    attn = torch.empty((N, R), dtype=torch.float32, device=dev) if want_attn else None
    top_slot = torch.empty((N, k), dtype=torch.int32, device=dev) if k > 0 else None
    top_w = torch.empty((N, k), dtype=torch.float32, device=dev) if k > 0 else None
    call('r4r_narre_explain', ptr(z), ptr(nb), ptr(other_table), int(other_table.shape[0]), ptr(own_table), ptr(owner),
         ptr(live), ptr(W0), ptr(b0), ptr(w3), ptr(b3), ptr(out), ptr(attn), ptr(top_slot), ptr(top_w), k, N, R, L)
    return out, attn, top_slot, top_w


NARRE_JAC_OUTPUTS = ('attn', 'pooled_attn', 'out', 'D', 'E', 'dz')
NARRE_PAIR_OUTPUTS = ('score', 'g_user', 'g_item', 'glogit_user', 'glogit_item', 'rev_user', 'rev_item', 'w_user', 'w_item')


def narre_attn_jac(z, nb, other_table, W0, b0, w3, b3, fc=None, own_table=None, owner=None, want=NARRE_JAC_OUTPUTS):
    """r4r_narre_attn_jac (include/r4r.h, "NARRE pair gradients"), the owner pass: ``narre_explain``'s inputs plus the
    side's tower ``fc`` [L, F] (needed for 'E').  ``want``: the outputs to compute, names of ``NARRE_JAC_OUTPUTS``.
    No autograd -> a dict name -> tensor: attn [N, R] and out [N, L] (``narre_explain``'s bits), pooled_attn [N, L] (out
    without the own row), D [N, R, L], E [N, R, F], dz [N, R]."""
    want = tuple(want)
    if not want or set(want) - set(NARRE_JAC_OUTPUTS):
        raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac want must name some of %r, got %r' % (NARRE_JAC_OUTPUTS, want))
    z, other_table = _f32(z, 'z'), _f32(other_table, 'other_table')
    W0, b0, w3, b3 = _f32(W0, 'W0'), _f32(b0, 'b0'), _f32(w3, 'w3'), _f32(b3, 'b3')
    nb = _i64(nb, 'nb')
    if z.dim() != 3 or tuple(nb.shape) != tuple(z.shape[:2]):
        raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac takes z [N, R, L] and nb [N, R], got %s and %s'
                           % (tuple(z.shape), tuple(nb.shape)))
    N, R, L = (int(d) for d in z.shape)
    if other_table.dim() != 2 or other_table.shape[1] != L or tuple(W0.shape) != (L, 2 * L) or b0.numel() != L \
            or w3.numel() != L or b3.numel() != 1:
        raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac: other_table [*, L], W0 [L, 2L], b0 [L], w3 [L], b3 [1] '
                           'with L = %d expected' % L)
    if (own_table is None) != (owner is None):
        raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac: own_table and owner go together')
    if own_table is not None:
        own_table, owner = _f32(own_table, 'own_table'), _i64(owner, 'owner')
        if own_table.dim() != 2 or own_table.shape[1] != L or owner.numel() != N:
            raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac: own_table [*, L] and owner [N] expected')
        if N and (int(owner.min()) < 0 or int(owner.max()) >= own_table.shape[0]):
            raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac: owner outside own_table\'s %d rows' % own_table.shape[0])
    F = 1
    if fc is None:
        if 'E' in want:
            raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac E needs fc')
    else:
        fc = _f32(fc, 'fc')
        if fc.dim() != 2 or fc.shape[0] != L:
            raise RuntimeError('reviews4rec_amd.ops: narre_attn_jac fc must be [L, F] = [%d, F], got %s' % (L, tuple(fc.shape)))
        F = int(fc.shape[1])
    sizes = dict(attn=(N, R), pooled_attn=(N, L), out=(N, L), D=(N, R, L), E=(N, R, F), dz=(N, R))
    out = {name: torch.empty(sizes[name], dtype=torch.float32, device=z.device) for name in NARRE_JAC_OUTPUTS if name in want}
    call('r4r_narre_attn_jac', ptr(z), ptr(nb), ptr(other_table), int(other_table.shape[0]), ptr(own_table), ptr(owner),
         ptr(W0), ptr(b0), ptr(w3), ptr(b3), ptr(fc), F, *(ptr(out.get(name)) for name in NARRE_JAC_OUTPUTS), N, R, L)
    return out


def narre_pair_grad(user, item, u_idx, i_idx, W1, b1, w, q_bias=None, c_bias=None, want=NARRE_PAIR_OUTPUTS):
    """r4r_narre_pair_grad (include/r4r.h, "NARRE pair gradients"), the pair pass.  ``user`` / ``item``: one dict per
    side with the owner pass's ``p`` [n, L] (its 'out'), ``z`` [n, R, L], ``attn`` [n, R] and, where the asked outputs
    need them, ``E`` [n, R, F], ``dz`` [n, R] and the tower's ``fc`` [L, F]; the sides may differ in R.  ``W1`` [L, L],
    ``b1`` [L], ``w`` [L]: final.1 and final.3.weight; ``q_bias`` [n_u] / ``c_bias`` [n_i]: the score's scalars, None = 0.
    ``want``: names of ``NARRE_PAIR_OUTPUTS``.  No autograd -> a dict name -> tensor: score [n_p], g_* [n_p, L],
    glogit_* / rev_* [n_p, R], w_* [n_p, R, F]."""
    want = tuple(want)
    if not want or set(want) - set(NARRE_PAIR_OUTPUTS):
        raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad want must name some of %r, got %r'
                           % (NARRE_PAIR_OUTPUTS, want))
    u_idx, i_idx = _i64(u_idx, 'u_idx').reshape(-1), _i64(i_idx, 'i_idx').reshape(-1)
    if u_idx.numel() != i_idx.numel():
        raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad takes equally long u_idx / i_idx, got %d and %d'
                           % (u_idx.numel(), i_idx.numel()))
    n_p = int(u_idx.numel())
    W1, b1, w = _f32(W1, 'W1'), _f32(b1, 'b1').reshape(-1), _f32(w, 'w').reshape(-1)
    L = int(b1.numel())
    if tuple(W1.shape) != (L, L) or w.numel() != L:
        raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad: W1 [L, L], b1 [L], w [L] expected, got %s, %d and %d'
                           % (tuple(W1.shape), L, w.numel()))
    sides, F = [], None
    for name, side in (('user', user), ('item', item)):
        s = {k: None if side.get(k) is None else _f32(side[k], '%s %s' % (name, k)) for k in ('p', 'z', 'attn', 'E', 'dz', 'fc')}
        if s['p'] is None or s['p'].dim() != 2 or s['p'].shape[1] != L or s['z'] is None or s['z'].dim() != 3 \
                or s['attn'] is None:
            raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad %s side needs p [n, L], z [n, R, L] and attn [n, R] '
                               'with L = %d' % (name, L))
        n, R = int(s['z'].shape[0]), int(s['z'].shape[1])
        if s['p'].shape[0] != n or s['z'].shape[2] != L or tuple(s['attn'].shape) != (n, R):
            raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad %s side: p %s, z %s, attn %s do not match'
                               % (name, tuple(s['p'].shape), tuple(s['z'].shape), tuple(s['attn'].shape)))
        if 'rev_' + name in want and (s['dz'] is None or tuple(s['dz'].shape) != (n, R)):
            raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad rev_%s needs dz [%d, %d]' % (name, n, R))
        if 'w_' + name in want:
            if s['fc'] is None or s['fc'].dim() != 2 or s['fc'].shape[0] != L:
                raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad w_%s needs fc [L, F] = [%d, F]' % (name, L))
            if s['E'] is None or tuple(s['E'].shape) != (n, R, int(s['fc'].shape[1])):
                raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad w_%s needs E [%d, %d, %d]'
                                   % (name, n, R, int(s['fc'].shape[1])))
            if F is not None and F != int(s['fc'].shape[1]):
                raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad: the two fc must share F')
            F = int(s['fc'].shape[1])
        else:
            s['E'] = s['fc'] = None                           # not read: no shape to hold them to
        if 'rev_' + name not in want:
            s['dz'] = None
        sides.append((s, n, R))
    F = 1 if F is None else F
    (su, n_u, R_u), (si, n_i, R_i) = sides
    biases = []
    for name, t, n in (('q_bias', q_bias, n_u), ('c_bias', c_bias, n_i)):
        t = None if t is None else _f32(t, name).reshape(-1)
        if t is not None and t.numel() != n:
            raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad %s must be [%d], got %s' % (name, n, tuple(t.shape)))
        biases.append(t)
    if n_p and (n_u == 0 or n_i == 0):
        raise RuntimeError('reviews4rec_amd.ops: narre_pair_grad: %d pairs over %d / %d owners' % (n_p, n_u, n_i))
    dev = su['p'].device
    sizes = dict(score=(n_p,), g_user=(n_p, L), g_item=(n_p, L), glogit_user=(n_p, R_u), glogit_item=(n_p, R_i),
                 rev_user=(n_p, R_u), rev_item=(n_p, R_i), w_user=(n_p, R_u, F), w_item=(n_p, R_i, F))
    out = {name: torch.empty(sizes[name], dtype=torch.float32, device=dev) for name in NARRE_PAIR_OUTPUTS if name in want}
    side_args = lambda s, n, R: (ptr(s['p']), ptr(s['z']), ptr(s['attn']), ptr(s['E']), ptr(s['dz']), ptr(s['fc']), n, R)
    call('r4r_narre_pair_grad', *side_args(su, n_u, R_u), *side_args(si, n_i, R_i), ptr(u_idx), ptr(i_idx), n_p,
         ptr(biases[0]), ptr(biases[1]), ptr(W1), ptr(b1), ptr(w), L, F,
         *(ptr(out.get(name)) for name in NARRE_PAIR_OUTPUTS))
    return out


NARRE_WHATIF_MAX = 64               # r4r_narre_logits / r4r_narre_whatif: S, R and L up to 64


def narre_logits(z, nb, other_table, W0, b0, w3, b3):
    """r4r_narre_logits (include/r4r.h, "NARRE what-if scores"), the owner pass: ``narre_explain``'s attention inputs
    over S slots, ``z`` [N, S, L] and ``nb`` [N, S] (int64 rows of ``other_table`` [rows, L]; an id outside reads as
    zeros) -> the PRE-softmax logits, float32 [N, S].  No autograd."""
    z, other_table = _f32(z, 'z'), _f32(other_table, 'other_table')
    W0, b0, w3, b3 = _f32(W0, 'W0'), _f32(b0, 'b0'), _f32(w3, 'w3'), _f32(b3, 'b3')
    nb = _i64(nb, 'nb')
    if z.dim() != 3 or tuple(nb.shape) != tuple(z.shape[:2]):
        raise RuntimeError('reviews4rec_amd.ops: narre_logits takes z [N, S, L] and nb [N, S], got %s and %s'
                           % (tuple(z.shape), tuple(nb.shape)))
    N, S, L = (int(d) for d in z.shape)
    if other_table.dim() != 2 or other_table.shape[1] != L or tuple(W0.shape) != (L, 2 * L) or b0.numel() != L \
            or w3.numel() != L or b3.numel() != 1:
        raise RuntimeError('reviews4rec_amd.ops: narre_logits: other_table [*, L], W0 [L, 2L], b0 [L], w3 [L], b3 [1] '
                           'with L = %d expected' % L)
    logit = torch.empty((N, S), dtype=torch.float32, device=z.device)
    call('r4r_narre_logits', ptr(z), ptr(nb), ptr(other_table), int(other_table.shape[0]), ptr(W0), ptr(b0), ptr(w3),
         ptr(b3), ptr(logit), N, S, L)
    return logit


def _narre_variant_args(op, user, item, u_idx, i_idx, W1, b1, w, q_bias, c_bias):
    """What ``narre_whatif`` and ``narre_search`` (``op``) share: u_idx / i_idx, W1 / b1 / w, the two side dicts and the
    biases, checked and normalised -> (n_p, device, head, tail, keep).  ``head``: the C arguments from z_u to i_idx,
    ``tail``: those from q_bias to L; ``keep`` holds the normalised tensors until the call is enqueued."""
    u_idx, i_idx = _i64(u_idx, 'u_idx').reshape(-1), _i64(i_idx, 'i_idx').reshape(-1)
    if u_idx.numel() != i_idx.numel():
        raise RuntimeError('reviews4rec_amd.ops: %s takes equally long u_idx / i_idx, got %d and %d'
                           % (op, u_idx.numel(), i_idx.numel()))
    n_p = int(u_idx.numel())
    W1, b1, w = _f32(W1, 'W1'), _f32(b1, 'b1').reshape(-1), _f32(w, 'w').reshape(-1)
    L = int(b1.numel())
    if tuple(W1.shape) != (L, L) or w.numel() != L:
        raise RuntimeError('reviews4rec_amd.ops: %s: W1 [L, L], b1 [L], w [L] expected, got %s, %d and %d'
                           % (op, tuple(W1.shape), L, w.numel()))
    keep, head, owners = [u_idx, i_idx, W1, b1, w], [], []
    for name, side in (('user', user), ('item', item)):
        s = {k: None if side.get(k) is None else _f32(side[k], '%s %s' % (name, k)) for k in ('z', 'logit', 'own', 'z_pad')}
        if s['z'] is None or s['z'].dim() != 3 or s['z'].shape[2] != L or s['logit'] is None or s['z_pad'] is None:
            raise RuntimeError('reviews4rec_amd.ops: %s %s side needs z [n, S, L], logit [n, S] and z_pad [L] '
                               'with L = %d' % (op, name, L))
        n, S = int(s['z'].shape[0]), int(s['z'].shape[1])
        if tuple(s['logit'].shape) != (n, S) or s['z_pad'].numel() != L \
                or (s['own'] is not None and tuple(s['own'].shape) != (n, L)):
            raise RuntimeError('reviews4rec_amd.ops: %s %s side: z %s, logit %s, z_pad %s, own %s do not match'
                               % (op, name, tuple(s['z'].shape), tuple(s['logit'].shape), tuple(s['z_pad'].shape),
                                  None if s['own'] is None else tuple(s['own'].shape)))
        R = side.get('R')
        if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= S:
            raise RuntimeError('reviews4rec_amd.ops: %s %s side: R = %r outside 1 .. S = %d' % (op, name, R, S))
        keep.append(s)
        owners.append(n)
        head += [ptr(s['z']), ptr(s['logit']), ptr(s['own']), ptr(s['z_pad']), float(side['logit_pad']), n, S, R]
    biases = []
    for name, t, n in (('q_bias', q_bias, owners[0]), ('c_bias', c_bias, owners[1])):
        t = None if t is None else _f32(t, name).reshape(-1)
        if t is not None and t.numel() != n:
            raise RuntimeError('reviews4rec_amd.ops: %s %s must be [%d], got %s' % (op, name, n, tuple(t.shape)))
        biases.append(t)
    if n_p and 0 in owners:
        raise RuntimeError('reviews4rec_amd.ops: %s: %d pairs over %d / %d owners' % (op, n_p, owners[0], owners[1]))
    head += [ptr(u_idx), ptr(i_idx)]
    tail = [ptr(biases[0]), ptr(biases[1]), ptr(W1), ptr(b1), ptr(w), L]
    return n_p, keep[5]['z'].device, head, tail, keep + biases           # the device: the user side's


def narre_whatif(user, item, u_idx, i_idx, drop_u, drop_i, W1, b1, w, q_bias=None, c_bias=None):
    """r4r_narre_whatif (include/r4r.h, "NARRE what-if scores"), the variant pass.  ``user`` / ``item``: one dict per
    side with ``z`` [n, S, L], ``logit`` [n, S] (``narre_logits``), ``z_pad`` [L], ``logit_pad`` (a float), ``R`` (the
    slots the model attends, 1 .. S) and optionally ``own`` [n, L]; the sides may differ in R and S.  ``drop_u`` /
    ``drop_i``: int64 [n_p, V] bit masks, bit s = slot s removed; None = nothing removed (one of them fixes V; both None:
    V = 1).  ``W1`` [L, L], ``b1`` [L], ``w`` [L]: final.1 and final.3.weight; ``q_bias`` [n_u] / ``c_bias`` [n_i]: the
    score's scalars, None = 0.  No autograd -> scores, float32 [n_p, V]."""
    n_p, dev, head, tail, keep = _narre_variant_args('narre_whatif', user, item, u_idx, i_idx, W1, b1, w, q_bias, c_bias)
    V, drops = None, []
    for name, d in (('drop_u', drop_u), ('drop_i', drop_i)):
        if d is not None:
            d = _i64(d, name)
            if d.dim() != 2 or d.shape[0] != n_p or d.shape[1] < 1 or (V is not None and d.shape[1] != V):
                raise RuntimeError('reviews4rec_amd.ops: narre_whatif %s must be [n_p, V] = [%d, %s], got %s'
                                   % (name, n_p, 'V' if V is None else V, tuple(d.shape)))
            V = int(d.shape[1])
        drops.append(d)
    V = 1 if V is None else V
    out = torch.empty((n_p, V), dtype=torch.float32, device=dev)
    call('r4r_narre_whatif', *head, ptr(drops[0]), ptr(drops[1]), n_p, V, *tail, ptr(out))
    return out


NARRE_SEARCH_MAX_BUDGET = 64        # r4r_narre_search: removals per pair
NARRE_SEARCH_ITEM = 64              # a step's number c: the slot on the user side, 64 + the slot on the item side


def narre_search(user, item, u_idx, i_idx, W1, b1, w, target, direction, budget, start_u=None, start_i=None,
                 cand_u=None, cand_i=None, q_bias=None, c_bias=None):
    """r4r_narre_search (include/r4r.h, "NARRE counterfactual search"): per pair, the greedy removal of reviews until
    the score passes ``target``, whole on the device.  ``user`` / ``item``: ``narre_whatif``'s side dicts.  ``target``:
    float32 [n_p]; ``direction``: 0 = down (done when score < target), 1 = up; ``budget``: 1 .. 64 removals.
    ``start_u`` / ``start_i``: int64 [n_p] masks of the slots already removed (None = none); ``cand_u`` / ``cand_i``:
    int64 [n_p] masks of the slots the search may remove (None = none on that side).  No autograd ->
    (order int32 [n_p, B], scores float32 [n_p, B + 1], steps int32 [n_p], crossed int32 [n_p])."""
    n_p, dev, head, tail, keep = _narre_variant_args('narre_search', user, item, u_idx, i_idx, W1, b1, w, q_bias, c_bias)
    for name, v, ok in (('direction', direction, (0, 1)), ('budget', budget, range(1, NARRE_SEARCH_MAX_BUDGET + 1))):
        if isinstance(v, bool) or not isinstance(v, int) or v not in ok:
            raise RuntimeError('reviews4rec_amd.ops: narre_search %s = %r outside %d .. %d' % (name, v, ok[0], ok[-1]))
    target = _f32(target, 'target').reshape(-1)
    if target.numel() != n_p:
        raise RuntimeError('reviews4rec_amd.ops: narre_search target must be [%d], got %s' % (n_p, tuple(target.shape)))
    masks = []
    for name, m in (('start_u', start_u), ('start_i', start_i), ('cand_u', cand_u), ('cand_i', cand_i)):
        if m is not None:
            m = _i64(m, name).reshape(-1)
            if m.numel() != n_p:
                raise RuntimeError('reviews4rec_amd.ops: narre_search %s must be [%d], got %s' % (name, n_p, tuple(m.shape)))
        masks.append(m)
    order = torch.empty((n_p, budget), dtype=torch.int32, device=dev)
    scores = torch.empty((n_p, budget + 1), dtype=torch.float32, device=dev)
    steps = torch.empty((n_p,), dtype=torch.int32, device=dev)
    crossed = torch.empty((n_p,), dtype=torch.int32, device=dev)
    call('r4r_narre_search', *head, *(ptr(m) for m in masks), ptr(target), direction, budget, n_p, *tail, ptr(order),
         ptr(scores), ptr(steps), ptr(crossed))
    return order, scores, steps, crossed


NARRE_SHAPLEY_MAX_PLAYERS = 16      # r4r_narre_shapley: players of one pair (2^16 coalitions)
NARRE_SHAPLEY_CHUNK_LOG = 10        # a pair's coalitions go 2^10 to a wave; beyond, the chunk sums pass through scratch


def narre_shapley(user, item, u_idx, i_idx, W1, b1, w, play_u=None, play_i=None, start_u=None, start_i=None, P=None,
                  q_bias=None, c_bias=None, values=False):
    """r4r_narre_shapley (include/r4r.h, "NARRE Shapley values"): per pair, the exact Shapley value of every playing
    review in the game "which of the players' reviews are present", whole on the device.  ``user`` / ``item``:
    ``narre_whatif``'s side dicts.  ``play_u`` / ``play_i``: int64 [n_p] masks of the slots that play (None = none on that
    side); ``start_u`` / ``start_i``: int64 [n_p] masks of the slots removed in every coalition (None = none).  ``P``:
    1 .. 16, the most players of a pair (a pair with more plays its lowest-numbered P: ``n`` tells); None = the most any
    pair of the call has, which reads the masks back to the host.  ``values=True`` also returns every coalition's score.
    No autograd -> (phi_u float32 [n_p, S_u], phi_i float32 [n_p, S_i], base float32 [n_p], empty float32 [n_p],
    n int32 [n_p], values float32 [n_p, 2^P] or None); only the first 2^n[p] entries of ``values[p]`` are written."""
    n_p, dev, head, tail, keep = _narre_variant_args('narre_shapley', user, item, u_idx, i_idx, W1, b1, w, q_bias, c_bias)
    S_u, S_i = int(keep[5]['z'].shape[1]), int(keep[6]['z'].shape[1])
    masks = []
    for name, m in (('start_u', start_u), ('start_i', start_i), ('play_u', play_u), ('play_i', play_i)):
        if m is not None:
            m = _i64(m, name).reshape(-1)
            if m.numel() != n_p:
                raise RuntimeError('reviews4rec_amd.ops: narre_shapley %s must be [%d], got %s' % (name, n_p, tuple(m.shape)))
        masks.append(m)
    if P is None:
        most = 0
        if n_p:
            count = torch.zeros(n_p, dtype=torch.int64, device=dev)
            for play, start, S in ((masks[2], masks[0], S_u), (masks[3], masks[1], S_i)):
                if play is not None:
                    live = play if start is None else play & ~start
                    count += ((live[:, None] >> torch.arange(S, device=dev)[None, :]) & 1).sum(1)
            most = int(count.max())
        P = min(max(most, 1), NARRE_SHAPLEY_MAX_PLAYERS)
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= NARRE_SHAPLEY_MAX_PLAYERS:
        raise RuntimeError('reviews4rec_amd.ops: narre_shapley P = %r outside 1 .. %d' % (P, NARRE_SHAPLEY_MAX_PLAYERS))
    if values and n_p << P >= 1 << 31:
        raise RuntimeError('reviews4rec_amd.ops: narre_shapley values of %d pairs x 2^%d coalitions pass 2^31 - 1' % (n_p, P))
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    phi_u, phi_i, base, empty = f32(n_p, S_u), f32(n_p, S_i), f32(n_p), f32(n_p)
    n = torch.empty((n_p,), dtype=torch.int32, device=dev)
    vals = f32(n_p, 1 << P) if values else None
    scratch = None
    if P > NARRE_SHAPLEY_CHUNK_LOG:
        scratch = torch.empty((n_p, 1 << (P - NARRE_SHAPLEY_CHUNK_LOG), P), dtype=torch.float64, device=dev)
    call('r4r_narre_shapley', *head, *(ptr(m) for m in masks), P, n_p, *tail, ptr(phi_u), ptr(phi_i), ptr(base),
         ptr(empty), ptr(n), ptr(vals), ptr(scratch))
    return phi_u, phi_i, base, empty, n, vals


class TransformLoss(Function):
    """mean_n ||a_n - b_n||^2 (TransNet's source/target representation loss)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, 'a'), _f32(b, 'b')
        out = torch.empty((1,), dtype=torch.float32, device=a.device)
        call('r4r_sqdist_mean_fwd', ptr(a), ptr(b), ptr(out), a.shape[0], a.shape[1])
        ctx.save_for_backward(a, b)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _f32(g, 'g').reshape(1)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        call('r4r_sqdist_mean_bwd', ptr(a), ptr(b), ptr(g), ptr(ga), ptr(gb), a.shape[0], a.shape[1])
        return ga, gb


def transform_loss(a, b):
    return TransformLoss.apply(a, b)


# --------------------------------------------------------------------- loss
def mse_fwd_bwd(out, y, denom, want_grad=True):
    """(per-example SE, d mean(SE)/d out) in one pass over the predictions."""
    out, y = _f32(out, 'out').reshape(-1), _f32(y, 'y').reshape(-1)
    se = torch.empty_like(out)
    g = torch.empty_like(out) if want_grad else None
    call('r4r_mse_fwd_bwd', ptr(out), ptr(y), ptr(se), ptr(g), out.numel(), float(denom))
    return se, g
