"""Evaluation (counterpart of the reference's eval.py).

``evaluate`` returns exactly what eval.py:11-62 returns -- ``{'MSE': round(sum SE / N,
4)}`` (+ MSE_right / MSE_transform for TransNet) and the two train-frequency -> [SE]
maps -- but keeps the per-example SE on the device during the pass, copies once per split and
groups on the host with numpy instead of the reference's two scalar reads per example
(eval.py:42-53).  ``eval_ranking`` is HR@1
over negatives-shaped batches (eval.py:64-92).

With a native engine and a device loader both passes run through the scoring spans (include/r4r.h, "Scoring
spans"): the launches are enqueued from C, the per-rating values come back in one copy and everything
the reference computes per slice is computed from them on the host.  ``R4R_SPANS=0`` or
``hyper_params['eval_spans'] = False`` keeps the per-launch loops below.
"""
import os

import torch


def _count_maps(ids, ses, counts):
    """{train frequency of the id: [SE, ...] in encounter order} (eval.py:45-53), vectorised:
    one dict lookup per DISTINCT id instead of per example; ids the map has not seen are
    entered with 0, as the reference does."""
    import numpy as np
    uniq, inv = np.unique(ids, return_inverse=True)
    freq = np.empty(len(uniq), dtype=np.int64)
    for k, u in enumerate(uniq.tolist()):
        freq[k] = counts.setdefault(u, 0)
    f = freq[inv]
    order = np.argsort(f, kind='stable')                     # stable: encounter order inside a group
    fs, ss = f[order], ses[order]
    cuts = np.flatnonzero(np.diff(fs)) + 1
    keys = fs[np.concatenate(([0], cuts))] if len(fs) else []
    return {int(k): grp.tolist() for k, grp in zip(keys, np.split(ss, cuts))}


EVAL_LAUNCH = 8          # x batch_size ratings per launch of a validation pass scored by a native engine
EVAL_LAUNCH_CAP = 4096   # ... but never more than max(batch_size, this) ratings
RANK_LAUNCH = 4          # x batch_size ranking rows (of 6 candidates each)


def _launch_size(reader, hyper_params, engine, factor):
    """Slice length of a validation pass.  The reference scores slices of ``batch_size`` (eval.py:24,
    data.py:379); a native engine's eval forward scores every rating by itself -- distinct-token
    projection, gather, one workgroup or wave per rating -- so larger slices of the same stream give the
    same scores with fewer launches and less Python per rating (``eval_batch_size`` overrides; the
    op-by-op module path keeps the reference's slices: its Linear layers are rocBLAS GEMMs over the
    batch).  TransNet's MSE_right / MSE_transform are means of per-slice means (eval.py:33-35): evaluate()
    takes them over the reference's slices INSIDE each launch, from the engine's per-rating values."""
    if engine is None or not getattr(reader, 'takes_batch', False):
        return None
    bsz = int(hyper_params['batch_size'])
    # the larger slices only pay while a launch is small: past EVAL_LAUNCH_CAP ratings the slice stays at
    # batch_size (the device batcher allocates n * (3 * doc + 20) * 8 bytes per launch and the engine keeps a
    # workspace per launch shape: a batch_size that trains must not run the validation pass out of memory)
    n = int(hyper_params.get('eval_batch_size') or min(factor * bsz, max(bsz, EVAL_LAUNCH_CAP)))
    if hyper_params['model_type'] in ['transnet', 'transnet++']:
        n = max(bsz, n - n % bsz)                            # launches must start on the reference's slice boundaries
    return n


def _spans_on(reader, hyper_params, engine):
    """The spanned path: an engine with scoring spans, a loader on the device, and nobody switched them off."""
    return (engine is not None and hasattr(engine, 'score_split') and hasattr(reader, 'score_descriptor')
            and reader._on_device() and os.environ.get('R4R_SPANS', '1') != '0'
            and hyper_params.get('eval_spans', True) is not False)


def slice_means(values, bsz):
    """Sum over the reference's slices of `bsz` ratings (the last one ragged) of the per-slice means of `values`
    [N, ...] (float64), and the number of slices: what eval.py:33-35 accumulates batch by batch."""
    import numpy as np
    n = values.shape[0]
    full = n // bsz
    total = np.zeros(values.shape[1:], np.float64)
    if full:
        total = total + values[:full * bsz].reshape((full, bsz) + values.shape[1:]).mean(axis=1).sum(axis=0)
    if n > full * bsz:
        total = total + values[full * bsz:].mean(axis=0)
    return total, full + int(n > full * bsz)


def metrics_from_se(ses, aux, bsz):
    """evaluate()'s metrics from the split's per-rating values on the host (float64): MSE = sum SE / N rounded to four
    decimals (eval.py:59); with `aux` [N, 2] (TransNet: target SE, transform distance) MSE_right / MSE_transform = the
    mean over the reference's slices of the per-slice means (eval.py:33-35, 60)."""
    import numpy as np
    ses = np.asarray(ses, np.float64)
    metrics = {'MSE': round(float(ses.sum()) / float(len(ses)), 4)}       # no ratings: ZeroDivisionError, like eval.py:59
    if aux is not None:
        total, slices = slice_means(np.asarray(aux, np.float64), bsz)
        metrics['MSE_right'] = round(float(total[0]) / float(slices), 4)
        metrics['MSE_transform'] = round(float(total[1]) / float(slices), 4)
    return metrics


def _evaluate_spanned(reader, hyper_params, user_count, item_count, engine, n):
    """evaluate() through engine.score_split: ONE device -> host copy of the SEs (and TransNet's pairs), the rest on
    the host.  None: this reader / engine pair has no scoring-span form."""
    out = engine.score_split(reader, reader.score_descriptor(n))
    if out is None:
        return None
    _, se, aux = out
    is_tn = hyper_params['model_type'] in ['transnet', 'transnet++']
    if is_tn and aux is not None:                            # one copy: [N, 3] = SE | target SE | transform distance
        both = torch.cat([se.reshape(-1, 1), aux], dim=1).double().cpu().numpy()
        ses, aux = both[:, 0].copy(), both[:, 1:]
    else:
        ses, aux = se.double().cpu().numpy(), None
    metrics = metrics_from_se(ses, aux, int(hyper_params['batch_size']))
    return metrics, _count_maps(reader._u, ses, user_count), _count_maps(reader._i, ses, item_count)


def evaluate(model, criterion, reader, hyper_params, user_count, item_count, review, engine=None):
    metrics = {}
    big = _launch_size(reader, hyper_params, engine, EVAL_LAUNCH)
    if big and len(reader.data) and _spans_on(reader, hyper_params, engine):
        model.eval()
        done = _evaluate_spanned(reader, hyper_params, user_count, item_count, engine, big)
        if done is not None:
            return done
    batches = reader.iter(eval=True, batch=big) if big else reader.iter(eval=True)
    total_n, total_batches = 0.0, 0.0
    bsz = int(hyper_params['batch_size'])
    is_tn = hyper_params['model_type'] in ['transnet', 'transnet++']
    se_parts, user_parts, item_parts = [], [], []
    total_se = mse_right = conv_loss = None                  # device scalars: no sync inside the pass
    model.eval()
    with torch.no_grad():
        for data, y in batches:
            user, item = data[5], data[6]
            if engine is not None:
                output, mse = engine.predict(data, y)
                mse = mse.clone()                            # the engine reuses its output buffer
                if is_tn:                                    # TransNetEngine: per rating (target pred, its SE, transform)
                    aux = engine.aux(data)[:, 1:3]
                    n_here, full = aux.shape[0], aux.shape[0] // bsz
                    if full:                                 # the reference's slices of batch_size inside this launch
                        rc = aux[:full * bsz].reshape(full, bsz, 2).mean(dim=1).sum(dim=0)
                        mse_right = rc[0] if mse_right is None else mse_right + rc[0]
                        conv_loss = rc[1] if conv_loss is None else conv_loss + rc[1]
                    if n_here > full * bsz:                  # ... and the ragged last one
                        rc = aux[full * bsz:].mean(dim=0)
                        mse_right = rc[0] if mse_right is None else mse_right + rc[0]
                        conv_loss = rc[1] if conv_loss is None else conv_loss + rc[1]
                    total_batches += float(full + (n_here > full * bsz)) - 1.0      # (+ 1.0 below)
            else:
                output = model(data)
                if is_tn:
                    mse = criterion(output[0], y, return_mean=False).data
                    r, c = criterion(output[1], y).data, output[2].data
                    mse_right = r if mse_right is None else mse_right + r
                    conv_loss = c if conv_loss is None else conv_loss + c
                else:
                    mse = criterion(output, y, return_mean=False).data
            s = torch.sum(mse)
            total_se = s if total_se is None else total_se + s
            total_n += float(int(y.shape[0]))
            se_parts.append(mse.reshape(-1))
            user_parts.append(user.reshape(-1))
            item_parts.append(item.reshape(-1))
            total_batches += 1.0
        # ONE device -> host copy for the whole split (the reference reads two scalars per example,
        # eval.py:42-53, which after acceleration costs more than the epoch it follows)
        ses = torch.cat(se_parts).double().cpu().numpy() if se_parts else None
        metrics['MSE'] = round(float(total_se) / total_n, 4)
        if is_tn:
            metrics['MSE_right'] = round(float(mse_right) / total_batches, 4)
            metrics['MSE_transform'] = round(float(conv_loss) / total_batches, 4)
    if ses is None:
        return metrics, {}, {}
    users = torch.cat(user_parts).cpu().numpy()
    items = torch.cat(item_parts).cpu().numpy()
    return metrics, _count_maps(users, ses, user_count), _count_maps(items, ses, item_count)


def _rank_spanned(reader, review, engine, rows_per_launch):
    """eval_ranking() through engine.score_split: the [rows, 6] scores stay on the device, r4r_rank_top1 counts the rows
    whose positive beats every negative and the rows it cannot decide (an exact tie with the best negative, a NaN); ONE
    copy of the two counters.  Any undecided row: the scores are copied and the batched host torch.topk decides, as the
    per-launch path does -- ties keep resolving the way the reference's ATen call resolves them.  None: no
    scoring-span form for this reader / engine pair."""
    from . import _lib
    if not reader.negs:                                      # no ranking rows: the loop below raises what it always raised
        return None
    out = engine.score_split(reader, reader.score_descriptor(6 * rows_per_launch, negs=True, review=review))
    if out is None:
        return None
    scores = out[0].view(-1, 6)
    rows = int(scores.shape[0])
    counts = torch.zeros(2, dtype=torch.int64, device=scores.device)
    _lib.check(_lib.lib().r4r_rank_top1(_lib.ptr(scores), rows, 6, _lib.ptr(counts), _lib.current_stream()),
               'r4r_rank_top1')
    hits, undecided = (int(c) for c in counts.cpu())
    if undecided:
        top = torch.topk(scores.float().cpu(), k=1, dim=-1, sorted=True).indices[:, 0]
        hits = int((top == 0).sum())
    return {'HR@1': round(100.0 * float(hits) / float(rows), 2)}     # no ranking rows: ZeroDivisionError, like eval.py:90


def eval_ranking(model, reader, hyper_params, review=False, engine=None):
    """HR@1 (eval.py:64-92): % of ranking rows whose positive -- column 0 of the [B, 6] scores -- is what
    ``torch.topk(scores[row], k=1)`` returns.  The scores of the whole split stay on the device and are
    copied ONCE; the top-1 is then taken on the host by the same ATen routine the reference calls per
    row (batched here), so exact score ties resolve the way they do there (a device-side topk may order
    ties differently).  ``engine``: a native engine of `model` -- its fused eval forward scores the batches."""
    parts = []
    is_tn = hyper_params['model_type'] in ['transnet', 'transnet++']
    big = _launch_size(reader, hyper_params, engine, RANK_LAUNCH)
    if big and _spans_on(reader, hyper_params, engine):
        done = _rank_spanned(reader, review, engine, big)
        if done is not None:
            return done
    with torch.no_grad():
        for data, y in (reader.iter_negs(review, batch=big) if big else reader.iter_negs(review)):
            if engine is not None:
                output = engine.predict(data, None)[0].clone()   # the engine reuses its output buffer
            else:
                output = model(data)
                if is_tn:
                    output = output[0]
            parts.append(output.reshape(-1, output.shape[-1]))
    scores = torch.cat(parts).float().cpu() if parts else torch.zeros(0, 6)
    # batched host topk == the reference's per-row call, ties included (probed: 10k rows of 3-valued scores)
    top = torch.topk(scores, k=1, dim=-1, sorted=True).indices[:, 0]
    hits, total = float((top == 0).sum()), float(scores.shape[0])
    return {'HR@1': round(100.0 * hits / total, 2)}        # no ranking rows: ZeroDivisionError, like eval.py:90


def eval_catalogue(model, train_reader, test_reader, hyper_params, ks=(1, 5, 10), engine=None, catalogue=None):
    """Full-catalogue ranking metrics: every row (u, i) of ``test_reader.data`` is placed in u's ranking over ALL
    eligible items, u's training items left out (recommend.Catalogue.rank: one fused pass on the device, one copy of
    the ranks) -- what eval.py:64-92 does against five sampled negatives, done against the catalogue.
    -> {'cat_HR@k', 'cat_NDCG@k', 'cat_MRR'} as percentages rounded to two places like HR@1, and 'cat_ranked' /
    'cat_unranked': a row whose item has no training rating cannot be ranked; it is counted, not averaged.  No
    ranked row: ZeroDivisionError, like eval.py:90."""
    import numpy as np
    from .recommend import Catalogue, ranking_metrics
    cat = catalogue if catalogue is not None else Catalogue(model, hyper_params, train_reader, engine=engine)
    data = np.asarray(test_reader.data)
    if len(data):
        users, items = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64)
    else:
        users = items = np.zeros(0, np.int64)
    ranks, _ = cat.rank(users, items, exclude_seen=True)
    m = ranking_metrics(ranks, ks)
    out = {'cat_' + k: round(100.0 * v, 2) for k, v in m.items() if k not in ('ranked', 'unranked')}
    out['cat_ranked'], out['cat_unranked'] = m['ranked'], m['unranked']
    return out


def eval_sampled(model, train_reader, test_reader, hyper_params, n_negatives=99, ks=(1, 5, 10), seed=0, engine=None,
                 catalogue=None, negatives=None):
    """Sampled-negative ranking metrics -- the protocol of eval.py:64-92 (HR@1 of one positive against five sampled
    negatives, rows from data.py:375-447) at any number of negatives and any K, NeuMF's 99 negatives with HR@10 /
    NDCG@10 by default: every row (u, i) of ``test_reader.data`` is placed among ``n_negatives`` items drawn from the
    eligible items u has no training rating for (recommend.sample_negatives, a function of ``seed``).  ONE
    Catalogue.rank_among call over the cached two sides -- no forward per candidate -- then recommend.ranking_metrics.
    ``negatives='dataset'`` takes the reference's own rows instead: per ranking user of ``test_reader.negs``, u ->
    ([positive, ...], [five negatives]), the first positive against those negatives (repeats dropped).  The slates are
    ranked as given: nothing further is excluded.
    -> {'samp_HR@k', 'samp_NDCG@k', 'samp_MRR'} as percentages rounded to two places like cat_* and HR@1, and
    'samp_ranked' / 'samp_unranked' (a row whose positive has no training rating cannot be ranked; it is counted, not
    averaged) / 'samp_short' (rows that got fewer than the negatives asked for: the user's pool is smaller).  No ranked
    row: ZeroDivisionError, like eval.py:90."""
    import numpy as np
    from .recommend import Catalogue, ranking_metrics, sample_negatives
    if negatives not in (None, 'dataset'):
        raise ValueError("eval_sampled: negatives must be None or 'dataset', got %r" % (negatives,))
    cat = catalogue if catalogue is not None else Catalogue(model, hyper_params, train_reader, engine=engine)
    if negatives == 'dataset':
        rows = [(int(u), int(v[0][0]), np.unique(np.asarray(v[1], dtype=np.int64))) for u, v in test_reader.negs.items()]
        users = np.array([r[0] for r in rows], np.int64)
        items = np.array([r[1] for r in rows], np.int64)
        rows = [r[2][r[2] != r[1]] for r in rows]
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        ids = np.concatenate(rows + [np.zeros(0, np.int64)])
        asked = max([len(v[1]) for v in test_reader.negs.values()] + [0])
    else:
        data = np.asarray(test_reader.data)
        if len(data):
            users, items = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64)
        else:
            users = items = np.zeros(0, np.int64)
        off, ids = sample_negatives(users, items, cat.eligible, cat.seen, n_negatives, seed)
        asked = int(n_negatives)
    ranks, _ = cat.rank_among(users, items, (off, ids), exclude_seen=False)
    m = ranking_metrics(ranks, ks)
    out = {'samp_' + k: round(100.0 * v, 2) for k, v in m.items() if k not in ('ranked', 'unranked')}
    out['samp_ranked'], out['samp_unranked'] = m['ranked'], m['unranked']
    out['samp_short'] = int((np.diff(off) < asked).sum())
    return out
