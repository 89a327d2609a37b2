#!/usr/bin/env python
"""Times the document fold (include/r4r.h, "Document fold") in the form of tools/bench_textcnn_whatif.py,
on that tool's synthetic pools at cfg3's cardinalities (DeepCoNN, T = 1000):

(a) r4r_fold_project and r4r_fold_segments (every owner of the side's pool) per side.
(b) compose + fc per variant row against r4r_tower_span_variants per row, over the same distinct leave-one-out rows of
    the item side.
(c) ``leave_one_out`` of every training user's top-10 with ``fold`` on and off (towers='device').
(d) ``review_counterfactual(k=10, side='item', budget=3)`` on a subsample against the host loop of tower-path
    ``what_if`` calls that takes the same steps; the share of pairs that crossed and the mean number of steps.

Device events around back-to-back calls for (a) and (b), wall clock with a device synchronise for (c) and (d); warmed up,
sides interleaved, `repeats` repeats, min .. max.  No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_tower_fold.py [--parts a,b,c,d] [--top 10] [--scale 1.0] [--tower-batch 256] [--pairs 512] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_textcnn_whatif import build, interleaved, wall  # noqa: E402


def project_and_segments(args, say, rows, cat):
    from reviews4rec_amd import ops
    say('# (a) r4r_fold_project (the whole vocabulary) and r4r_fold_segments (every owner), %d interleaved repeats, '
        'microseconds per call (min .. max)' % args.repeats)
    sides = {}
    for side in ('user', 'item'):
        pool, tower, _ = cat._phrase_side(side)
        conv = tower.convs[0]
        words, w, b = cat._words().detach(), conv.weight.detach(), conv.bias.detach()
        ptab = ops.fold_project(words, w)
        own = np.arange(pool.owners, dtype=np.int64)
        ids = torch.from_numpy(own).to(cat.dev)
        S = int(min(64, (pool.first[1:] - pool.first[:-1]).max()))
        pd = pool.device(cat.dev)
        sides['project, %s (V = %d, E = %d)' % (side, words.shape[0], words.shape[1])] = \
            lambda words=words, w=w: ops.fold_project(words, w)
        sides['segments, %s (%d owners, S = %d)' % (side, len(own), S)] = \
            lambda ptab=ptab, b=b, pd=pd, ids=ids, S=S: ops.fold_segments(ptab, b, pd, ids, S)
    for name, ts in interleaved(sides, args.repeats).items():
        rows.append(dict(part='a', what=name, us=[min(ts), max(ts)]))
        say('  %-44s | %10.1f .. %10.1f us' % (name, min(ts), max(ts)))


def per_row(args, say, rows, hp, cat, items):
    from reviews4rec_amd import ops
    T = int(hp['input_length'])
    pool, tower, _ = cat._phrase_side('item')
    ru, du, _, _, nb = cat._loo_rows(pool, items, 64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(cat.dev)
    own, inv = np.unique(ru, return_inverse=True)
    side = cat._fold_side(tower, pool, own)
    conv = tower.convs[0]
    w = (cat._words().detach(), conv.weight.detach(), conv.bias.detach(), tower.fc.weight.detach(), tower.fc.bias.detach())
    pd, d_ids, d_inv, d_drop = pool.device(cat.dev), t(ru), t(inv), t(du)
    keep = {}
    sides = {'compose + fc': lambda: keep.__setitem__('fold', ops.fold_latents(side, d_inv, T, drop=d_drop)),
             'r4r_tower_span_variants': lambda: keep.__setitem__('tower', ops.tower_span_variants(
                 pd, d_ids, T, *w, max(1, cat.tower_batch), drop=d_drop))}
    say('# (b) the item side\'s %d distinct leave-one-out rows (%d owners, T = %d), %d interleaved repeats, milliseconds per '
        'pass (min .. max) and microseconds per row' % (len(ru), nb, T, args.repeats))
    times = interleaved(sides, args.repeats, window_us=1)
    gap = float((keep['fold'] - keep['tower']).abs().max())
    for name, ts in times.items():
        rows.append(dict(part='b', what=name, rows=len(ru), ms=[min(ts) / 1e3, max(ts) / 1e3], us_per_row=min(ts) / len(ru)))
        say('  %-26s | %9.2f .. %9.2f ms | %7.3f us per row' % (name, min(ts) / 1e3, max(ts) / 1e3, min(ts) / len(ru)))
    say('  largest |latent(fold) - latent(tower)| over the rows: %.3g' % gap)
    rows.append(dict(part='b', what='gap', max_abs_latent_difference=gap))


def leave_one_out(args, say, rows, cat, users, items):
    say('# (c) leave_one_out of every training user\'s top-%d (%d pairs), towers=device, %d interleaved repeats, wall-clock '
        'milliseconds per pass (min .. max)' % (args.top, len(users), args.repeats))
    times = {'fold off': [], 'fold on': []}
    for on in (False, True):
        cat.fold = on
        cat.leave_one_out(users, items)                      # warm-up
    for _ in range(args.repeats):
        for name, on in (('fold off', False), ('fold on', True)):
            cat.fold = on
            ms, out = wall(lambda: cat.leave_one_out(users, items))
            times[name].append(ms)
    cat.fold = False
    for name, ts in times.items():
        rows.append(dict(part='c', what=name, pairs=len(users), ms=[min(ts), max(ts)]))
        say('  %-10s | %10.1f .. %10.1f ms' % (name, min(ts), max(ts)))


def host_search(cat, users, items, target, budget):
    """``review_counterfactual(side='item', direction='down')`` as a host loop of tower-path ``what_if`` calls: per step
    every review of the item that shows in its current document removed in turn, the lowest score kept."""
    T = int(cat.hp['input_length'])
    pool = cat._phrase_side('item')[0]
    n = len(users)
    S = int(min(64, (pool.first[items + 1] - pool.first[items]).max()))
    lens = np.zeros((n, S), np.int64)
    for p, o in enumerate(items):
        c = min(int(pool.first[o + 1] - pool.first[o]), S)
        lens[p, :c] = np.diff(pool.rev_off[pool.first[o]:pool.first[o] + c + 1])
    gone = np.zeros((n, S), bool)
    score = cat.what_if(users, items).base.cpu().numpy()
    done = score < target
    steps = np.zeros(n, np.int64)
    bit = (np.uint64(1) << np.arange(S, dtype=np.uint64))
    for _ in range(budget):
        kept = np.where(gone, 0, lens)
        start = np.cumsum(kept, 1) - kept
        cand = ~gone & (lens > 0) & (start < T) & ~done[:, None]
        mask = (gone * bit[None, :]).sum(1, dtype=np.uint64)
        variants = (mask[:, None] | bit[None, :]).view(np.int64)
        sc = cat.what_if(users, items, drop_item=torch.from_numpy(variants)).scores.cpu().numpy()
        sc = np.where(cand, sc, np.inf)
        best = sc.argmin(1)
        take = cand.any(1)
        done |= ~take
        gone[np.nonzero(take)[0], best[take]] = True
        score = np.where(take, sc[np.arange(n), best], score)
        steps += take
        done |= score < target
    return steps, score < target


def search(args, say, rows, cat, users, items):
    n = min(args.pairs, len(users))
    pick = np.random.default_rng(0).choice(len(users), n, replace=False)
    u, i = users[pick], items[pick]
    k, budget = args.top, 3
    say('# (d) review_counterfactual(k=%d, side=\'item\', budget=%d) over %d of those pairs against the host loop of tower-path '
        'what_if calls, %d interleaved repeats, wall-clock milliseconds (min .. max)' % (k, budget, n, args.repeats))
    cat.fold = False
    cf = cat.review_counterfactual(u, i, k=k, side='item', budget=budget)
    target = cf.target.cpu().numpy()
    host_search(cat, u, i, target, budget)
    times = {'review_counterfactual': [], 'host loop, tower path': []}
    for _ in range(args.repeats):
        ms, cf = wall(lambda: cat.review_counterfactual(u, i, k=k, side='item', budget=budget))
        times['review_counterfactual'].append(ms)
        ms, (h_steps, h_hit) = wall(lambda: host_search(cat, u, i, target, budget))
        times['host loop, tower path'].append(ms)
    for name, ts in times.items():
        rows.append(dict(part='d', what=name, pairs=n, ms=[min(ts), max(ts)]))
        say('  %-24s | %10.1f .. %10.1f ms' % (name, min(ts), max(ts)))
    steps, hit = cf.steps.cpu().numpy(), cf.crossed.cpu().numpy()
    rows.append(dict(part='d', what='outcome', crossed_share=float(hit.mean()), mean_steps=float(steps.mean()),
                     host_crossed_share=float(h_hit.mean()), host_mean_steps=float(h_steps.mean()),
                     same_steps_share=float((steps == h_steps).mean())))
    say('  %.1f%% of the pairs crossed, %.2f steps on average (host loop, in the tower path\'s bits: %.1f%%, %.2f; the same '
        'number of steps for %.1f%% of the pairs)' % (100 * hit.mean(), steps.mean(), 100 * h_hit.mean(), h_steps.mean(),
                                                       100 * (steps == h_steps).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b,c,d')
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the configuration's users, items and ratings")
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--pairs', type=int, default=512, help="(d)'s subsample")
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tower_fold: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_tower_fold: at least five repeats per side')
    from reviews4rec_amd.recommend import recommended_pairs
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    say('# document fold; %s; scale %g' % (torch.cuda.get_device_name(0), args.scale))
    hp, reader, model, cats = build(args)
    cat = cats['device']
    parts = args.parts.split(',')
    if 'a' in parts:
        project_and_segments(args, say, rows, cat)
        save()
    users, items = recommended_pairs(cat, args.top)
    for part, fn in (('b', lambda: per_row(args, say, rows, hp, cat, items)),
                     ('c', lambda: leave_one_out(args, say, rows, cat, users, items)),
                     ('d', lambda: search(args, say, rows, cat, users, items))):
        if part in parts:
            fn()
            save()
    print(json.dumps({'bench_tower_fold': rows}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
