#!/usr/bin/env python
"""Times the what-if documents of the single-document families (include/r4r.h, "What-if documents"), in
the form of tools/bench_pair_explain.py, on the synthetic pools that tool uses at cfg3's cardinalities (DeepCoNN,
T = 1000):

(a) the writer and the span over every eligible item: r4r_tower_build_variants -- with one review of each row removed,
    and with 15 occluded positions per row on top -- against r4r_tower_build, and r4r_tower_span_variants (one review
    removed) against r4r_tower_span_fwd.  Device events around `inner` back-to-back calls, warmed up, sides
    INTERLEAVED, `repeats` repeats, min .. max; the writers with the share of the HBM write stream their int64 output
    (8 T bytes per row) reaches.
(b) ``leave_one_out`` end to end for every training user's top-10 list, towers='device' against towers='host' -- the
    latter over the first --host-pairs pairs, with the device side timed over the same subsample next to it; the variant
    rows, the rows the "same document" rule did not run, and the time per row.
(c) ``deletion_curve`` (k = 5, by='pair', the user side) over 8,192 and 131,072 of those pairs, towers='device'.

Wall clock with a device synchronise inside every window for (b) and (c).  No ratio is a gate: every row is printed,
whichever side it favours.

    python tools/bench_textcnn_whatif.py [--parts a,b,c] [--top 10] [--scale 1.0] [--tower-batch 256] [--host-pairs 2000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

CONFIG = 'cfg3_deepconn_electronics_e300'
HBM_PEAK = 8.0e12                                           # bytes / s, the part's specification
OCCLUDED = 15
CURVE_PAIRS = (8192, 131072)


def timed(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner * 1e3            # microseconds per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out             # milliseconds


def interleaved(sides, repeats, window_us=20000):
    for _ in range(2):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    inner = {name: max(1, min(200, int(window_us / max(timed(fn, 2), 1.0)))) for name, fn in sides.items()}
    times = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            times[name].append(timed(fn, inner[name]))
    return times


def build(args):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    cfg = synthetic.hyper_params_for(CONFIG)
    n_users, n_items, n_ratings = (max(1, int(cfg[k] * args.scale)) for k in ('total_users', 'total_items', 'n_train'))
    E, V = int(cfg['word_embed_size']), int(cfg['vocab'])
    d = synthesize(n_ratings, n_users, n_items, V)
    hp = dict(cfg, total_users=n_users, total_items=n_items, total_words=V, engine='native')
    hp['word_vectors'] = synthetic.word_table(V, E)
    reader = DataLoader(hp, d['train'], d['user_reviews'], d['item_reviews'], None,
                        this_index_user_item=d['this_index_user_item'], device='cuda')
    torch.manual_seed(0)
    model = reviews4rec_amd.get_model_class('deepconn')(hp)
    xavier_init(model)
    model = model.cuda().eval()
    return hp, reader, model, {t: Catalogue(model, hp, reader, tower_batch=args.tower_batch, towers=t) for t in ('device', 'host')}


def writer_and_span(args, say, rows, hp, cat):
    from reviews4rec_amd import _lib, ops
    from reviews4rec_amd._lib import ptr
    dev, T = cat.dev, int(hp['input_length'])
    pool, tower, _ = cat._phrase_side('item')
    ids = np.ascontiguousarray(cat.eligible, dtype=np.int64)
    n = len(ids)
    count = pool.first[ids + 1] - pool.first[ids]
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drop = t((np.uint64(1) << (rng.integers(0, 1 << 30, n) % np.maximum(np.minimum(count, 64), 1)).astype(np.uint64)).view(np.int64))
    occ_off = t(np.arange(n + 1, dtype=np.int64) * OCCLUDED)
    occ_pos = t(rng.integers(0, T, n * OCCLUDED).astype(np.int32))
    pool_dev, d_ids = pool.device(dev), t(ids)
    tok, rev_off, first, nb = pool_dev
    docs = torch.empty((n, T), dtype=torch.int64, device=dev)
    sides = {
        'r4r_tower_build': lambda: _lib.call('r4r_tower_build', ptr(tok), ptr(rev_off), ptr(first), ptr(nb), int(pool.owners),
                                             ptr(d_ids), n, T, 0, 0, 0, ptr(docs), None),
        'variants, nothing removed': lambda: _lib.call('r4r_tower_build_variants', ptr(tok), ptr(rev_off), ptr(first),
                                                       int(pool.owners), ptr(d_ids), None, None, None, n, T, ptr(docs)),
        'variants, one review removed': lambda: _lib.call('r4r_tower_build_variants', ptr(tok), ptr(rev_off), ptr(first),
                                                          int(pool.owners), ptr(d_ids), ptr(drop), None, None, n, T, ptr(docs)),
        'variants, removed + %d occluded' % OCCLUDED: lambda: _lib.call(
            'r4r_tower_build_variants', ptr(tok), ptr(rev_off), ptr(first), int(pool.owners), ptr(d_ids), ptr(drop),
            ptr(occ_off), ptr(occ_pos), n, T, ptr(docs)),
    }
    say('# (a) the writers over %d rows of T = %d (%.1f MB of int64 output per call), %d interleaved repeats, microseconds '
        'per call (min .. max)' % (n, T, n * T * 8 / 1e6, args.repeats))
    times = interleaved(sides, args.repeats)
    for name, ts in times.items():
        share = n * T * 8 / (min(ts) * 1e-6) / HBM_PEAK
        rows.append(dict(part='a', what=name, rows=n, T=T, us=[min(ts), max(ts)], write_tb_s=n * T * 8 / (min(ts) * 1e-6) / 1e12,
                         share_of_hbm_peak=share))
        say('  %-36s | %9.1f .. %9.1f us | %5.2f TB/s written, %4.1f%% of the %.0f TB/s peak' % (
            name, min(ts), max(ts), rows[-1]['write_tb_s'], 100 * share, HBM_PEAK / 1e12))
    del docs
    conv = tower.convs[0]
    w = (cat._words().detach(), conv.weight.detach(), conv.bias.detach(), tower.fc.weight.detach(), tower.fc.bias.detach())
    keep = {}
    sides = {'r4r_tower_span_fwd': lambda: keep.__setitem__('fwd', cat._span_latents(tower, pool, ids)),
             'span_variants, nothing removed': lambda: keep.__setitem__('plain', ops.tower_span_variants(
                 pool_dev, d_ids, T, *w, max(1, cat.tower_batch))),
             'span_variants, one review removed': lambda: keep.__setitem__('drop', ops.tower_span_variants(
                 pool_dev, d_ids, T, *w, max(1, cat.tower_batch), drop=drop))}
    say('# (a) the spans over the same rows, tower_batch %d, milliseconds per pass (min .. max)' % cat.tower_batch)
    times = interleaved(sides, args.repeats, window_us=1)
    assert torch.equal(keep['fwd'], keep['plain']), 'with nothing removed the span is not r4r_tower_span_fwd'
    for name, ts in times.items():
        rows.append(dict(part='a', what=name, rows=n, T=T, ms=[min(ts) / 1e3, max(ts) / 1e3]))
        say('  %-36s | %9.2f .. %9.2f ms' % (name, min(ts) / 1e3, max(ts) / 1e3))
    say('# with nothing removed the span\'s latents are r4r_tower_span_fwd\'s, bit for bit')


def end_to_end(args, say, rows, cats, users, items):
    dev, host = cats['device'], cats['host']
    sub = slice(0, min(args.host_pairs, len(users)))
    say('# (b) leave_one_out of every training user\'s top-%d; tower_batch %d, %d interleaved repeats, wall-clock milliseconds '
        'per pass (min .. max)' % (args.top, args.tower_batch, args.repeats))
    stats = {}
    for side, ids in (('user', users), ('item', items)):
        pool = dev._phrase_side(side)[0]
        own = np.unique(ids)
        has, seen = dev._whatif_slots(pool, own)
        stats[side] = (len(own), int(has.sum()), int(seen.sum()))
    for c in (dev, host):
        c.leave_one_out(users[sub], items[sub])              # warm-up
    dev.leave_one_out(users, items)
    ran = dev.whatif_rows
    assert ran == (stats['user'][2], stats['item'][2])
    times = {'device, all pairs': [], 'device, subsample': [], 'host, subsample': []}
    for _ in range(args.repeats):
        ms, full = wall(lambda: dev.leave_one_out(users, items))
        times['device, all pairs'].append(ms)
        ms, a = wall(lambda: dev.leave_one_out(users[sub], items[sub]))
        times['device, subsample'].append(ms)
        sub_rows = sum(dev.whatif_rows)
        ms, b = wall(lambda: host.leave_one_out(users[sub], items[sub]))
        times['host, subsample'].append(ms)
    for x, y in zip(a, b):
        assert torch.equal(x, y), 'towers=device does not give the bits of towers=host'
    n_rows = {'device, all pairs': sum(ran) + stats['user'][0] + stats['item'][0]}
    for name, ts in times.items():
        pairs = len(users) if name.endswith('all pairs') else sub.stop
        rows.append(dict(part='b', what=name, pairs=pairs, ms=[min(ts), max(ts)]))
        say('  %-20s %9d pairs | %10.1f .. %10.1f ms' % (name, pairs, min(ts), max(ts)))
    for side in ('user', 'item'):
        owners, slots, run = stats[side]
        say('  %s side: %d distinct owners, %d (owner, review) slots, %d variant rows run, %d not run (the same document)'
            % (side, owners, slots, run, slots - run))
    per_row = min(times['device, all pairs']) * 1e3 / n_rows['device, all pairs']
    rows.append(dict(part='b', what='rows', stats=stats, tower_rows=n_rows['device, all pairs'], us_per_tower_row=per_row,
                     subsample_variant_rows=sub_rows, without_user_shape=list(full.without_user.shape),
                     without_item_shape=list(full.without_item.shape)))
    say('  %d tower rows in all (variants + base documents): %.2f us per row end to end; the subsample runs %d variant rows; '
        'host / device on it %.1fx' % (n_rows['device, all pairs'], per_row, sub_rows,
                                      min(times['host, subsample']) / min(times['device, subsample'])))


def curves(args, say, rows, cat, users, items):
    say('# (c) deletion_curve, k = 5, by=\'pair\', the user side, towers=device; wall-clock milliseconds per call (min .. max)')
    for n in CURVE_PAIRS:
        n = min(max(1, int(n * args.scale)), len(users))
        u, i = users[:n], items[:n]
        cat.deletion_curve(u, i, k=5)
        ts = []
        for _ in range(args.repeats):
            ms, dc = wall(lambda: cat.deletion_curve(u, i, k=5))
            ts.append(ms)
        rows.append(dict(part='c', pairs=n, ms=[min(ts), max(ts)], variant_rows=list(cat.whatif_rows),
                         mean_aopc=float(dc.aopc.mean())))
        say('  %9d pairs | %10.1f .. %10.1f ms | %d variant rows | mean AOPC %.4g' % (n, min(ts), max(ts), sum(cat.whatif_rows),
                                                                                 rows[-1]['mean_aopc']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b,c')
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the configuration's users, items, ratings and of (c)'s pairs")
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--host-pairs', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_textcnn_whatif: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_textcnn_whatif: at least five repeats per side')
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

    say('# what-if documents; %s; scale %g' % (torch.cuda.get_device_name(0), args.scale))
    hp, reader, model, cats = build(args)
    parts = args.parts.split(',')
    if 'a' in parts:
        writer_and_span(args, say, rows, hp, cats['device'])
        save()
    if 'b' in parts or 'c' in parts:
        users, items = recommended_pairs(cats['device'], args.top)
    if 'b' in parts:
        end_to_end(args, say, rows, cats, users, items)
        save()
    if 'c' in parts:
        curves(args, say, rows, cats['device'], users, items)
    print(json.dumps({'bench_textcnn_whatif': rows}))
    save()
    return 0


if __name__ == '__main__':
    sys.exit(main())
