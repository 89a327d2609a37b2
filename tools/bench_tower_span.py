#!/usr/bin/env python
"""Times a catalogue's tower passes with towers='host' against towers='device' (recommend.Catalogue):

    refresh()    one tower forward per eligible item, folded into the cache
    _queries()   one tower forward per user, over ALL users (what write_recommendations / eval_catalogue pay)

    host     every owner's document built with numpy, copied to the device tower_batch owners at a time, one Python call
             per chunk through the tower -- the path before tower spans, unchanged, so it is the yardstick
    device   one r4r_tower_span_fwd call per pass (csrc/tower_span.hip): documents from the HBM-resident pools, the same
             per-chunk launches enqueued from C; the folds run over the same slices

Same process, same model, same reader; both sides warmed up, then `repeats` repeats of each side INTERLEAVED, a device
synchronise inside every timed window (wall clock: the host's share is what is being measured); min .. max of the repeats
are reported with the ratio of the minima.  The caches and the queries of the timed shapes are asserted bit-equal.  The
H2D column counts the bytes of tower INPUT each side copies per pass, from the shapes: n doc 8 (+ n 10 8 neighbour ids
for NARRE) on the host path, n 8 (the ids) on the device path; the pools are resident once per dataset on both.

Shapes: synthetic pools at the cardinalities, T and E of BASELINE.json configs[2] (DeepCoNN) and configs[3] (NARRE)
(reviews4rec_amd/synthetic.py CONFIGS), drawn as tools/bench_epoch.py draws its loader's data (tools/synth_reviews.py);
--scale shrinks users, items and ratings together.

    python tools/bench_tower_span.py [--models deepconn,NARRE] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

CONFIG = {'deepconn': 'cfg3_deepconn_electronics_e300', 'NARRE': 'cfg4_narre_kindle'}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out             # milliseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='deepconn,NARRE')
    ap.add_argument('--scale', type=float, default=1.0, help="of the configurations' users, items and ratings")
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tower_span: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_tower_span: at least five repeats per side')
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue, NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# catalogue tower passes, towers=host against towers=device; %s; tower_batch %d, %d interleaved repeats, '
        'wall-clock milliseconds per pass (min .. max), device synchronised inside each window'
        % (torch.cuda.get_device_name(0), args.tower_batch, args.repeats))
    say('# %-9s %-9s %7s | %21s | %21s | %8s | %13s %11s' % ('model', 'pass', 'owners', 'host ms', 'device ms', 'speedup',
                                                              'host H2D MB', 'device MB'))
    for mt in args.models.split(','):
        cfg = synthetic.hyper_params_for(CONFIG[mt])
        n_users, n_items, n_ratings = (max(1, int(cfg[k] * args.scale)) for k in ('total_users', 'total_items', 'n_train'))
        E, T, R, W, V = (int(cfg[k]) for k in ('word_embed_size', 'input_length', 'narre_num_reviews', 'narre_num_words', 'vocab'))
        d = synthesize(n_ratings, n_users, n_items, V)
        say('# %s (%s): %d users, %d items, %d training ratings, E = %d, %s'
            % (mt, CONFIG[mt], n_users, n_items, n_ratings, E, 'R x W = %d x %d' % (R, W) if mt == 'NARRE' else 'T = %d' % T))
        hp = dict(cfg, total_users=n_users, total_items=n_items, total_words=V, engine='native')
        hp['word_vectors'] = synthetic.word_table(V, E)
        reader = DataLoader(hp, d['train'], d['user_reviews'], d['item_reviews'], None,
                            this_index_user_item=d['this_index_user_item'], device='cuda')
        torch.manual_seed(0)
        model = reviews4rec_amd.get_model_class(mt)(hp)
        xavier_init(model)
        model = model.cuda().eval()
        cls = NarreCatalogue if mt == 'NARRE' else Catalogue
        cats = {t: cls(model, hp, reader, tower_batch=args.tower_batch, towers=t) for t in ('host', 'device')}   # (warms refresh)
        users = torch.arange(n_users, dtype=torch.int64)
        doc = R * W if mt == 'NARRE' else T
        extra = 10 if mt == 'NARRE' else 0
        passes = (('refresh', len(cats['host'].eligible), lambda c: c.refresh()),
                  ('queries', n_users, lambda c: c._queries(users)))
        for name, n, run in passes:
            for c in cats.values():
                run(c)                                       # warm-up: workspaces, code objects, the pools on the device
            times = {'host': [], 'device': []}
            for _ in range(args.repeats):
                for t in ('host', 'device'):
                    ms, out = wall(lambda: run(cats[t]))
                    times[t].append(ms)
                    if name == 'queries':
                        cats[t].last_queries = out
            if name == 'refresh':
                equal = torch.equal(cats['host'].c, cats['device'].c) and torch.equal(cats['host'].c_bias, cats['device'].c_bias)
            else:
                equal = all(torch.equal(a, b) for a, b in zip(cats['host'].last_queries, cats['device'].last_queries))
            assert equal, '%s %s: towers=device does not give the bits of towers=host' % (mt, name)
            h2d = {'host': n * (doc + extra) * 8 / 1e6, 'device': n * 8 / 1e6}
            row = dict(model_type=mt, pass_=name, owners=n, E=E, doc=doc, tower_batch=args.tower_batch,
                       host_ms=[min(times['host']), max(times['host'])], device_ms=[min(times['device']), max(times['device'])],
                       speedup=min(times['host']) / min(times['device']), h2d_mb=h2d, bit_equal=bool(equal),
                       device_range_below_host=max(times['device']) < min(times['host']))
            rows.append(row)
            say('  %-9s %-9s %7d | %9.1f .. %9.1f | %9.1f .. %9.1f | %7.2fx | %13.1f %11.3f%s' % (
                mt, name, n, row['host_ms'][0], row['host_ms'][1], row['device_ms'][0], row['device_ms'][1], row['speedup'],
                h2d['host'], h2d['device'], '' if row['device_range_below_host'] else '   DEVICE RANGE NOT BELOW THE HOST\'S'))
        del cats, model, reader, d
        torch.cuda.empty_cache()
    say('# c / c_bias after refresh() and (q, q_bias) of every user: bit-equal between the two sides on every shape above')
    print(json.dumps({'bench_tower_span': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
