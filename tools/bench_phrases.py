#!/usr/bin/env python
"""Times the phrase explanations (include/r4r.h, "Phrase explanations"), in the form of
tools/bench_narre_explain.py and tools/bench_tower_span.py:

(a) r4r_textcnn_phrases alone (csrc/phrases.hip) at the row counts of cfg3 and cfg4 (reviews4rec_amd/synthetic.py) --
    61,610 documents of T = 1000 words, 61,934 x 10 reviews of W = 100 -- against what a user could do before in plain
    torch over the same pooled / argmax: scatter_add of the live filters' values into a dense [N, T + 2] and torch.topk.
    F = 100 filters, all five outputs written (the tokens from an [N, T] int64 document block), synthetic inputs: argmax
    uniform over the T + 2 positions with one filter in twenty dead -- MORE distinct windows per row than a trained tower
    leaves, where many filters fire on the same phrase.  Device events around `inner` back-to-back calls (~20 ms
    windows), every shape warmed up, sides INTERLEAVED, `repeats` repeats, min .. max.
(b) ``explain_words`` over every eligible item with towers='device' (one r4r_tower_span_phrases call) against
    towers='host' (numpy documents, one textcnn_fwd_raw + textcnn_phrases call per tower_batch owners) on synthetic pools
    at cfg3's (DeepCoNN) and cfg4's (NARRE) cardinalities: one catalogue, its ``towers`` flipped between the windows,
    wall clock with a device synchronise inside every window, sides interleaved, min .. max; the two sides' outputs are
    asserted bit-equal.

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_phrases.py [--parts a,b] [--k 5] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
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

SHAPES = (('cfg3 documents', 61610, 1000), ('cfg4 reviews', 61934 * 10, 100))      # (what, rows, words per row)
CONFIG = {'deepconn': 'cfg3_deepconn_electronics_e300', 'NARRE': 'cfg4_narre_kindle'}
F = 100


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


def kernel_alone(args, say, rows):
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    dev, K = 'cuda', args.k
    say('# (a) r4r_textcnn_phrases against torch scatter_add + topk; F = %d, K = %d, %d interleaved repeats, microseconds '
        'per call (min .. max)' % (F, K, args.repeats))
    say('# %-15s %7s %5s %9s | %22s | %22s | %8s' % ('shape', 'rows', 'T', 'weights', 'phrases us', 'torch us', 'vs torch'))
    for what, N, T in SHAPES:
        N = max(1, int(N * args.scale))
        gen = torch.Generator(device=dev).manual_seed(7000 + T)
        pooled = torch.rand((N, F), generator=gen, device=dev) * 3
        argmax = torch.randint(0, T + 2, (N, F), generator=gen, device=dev).to(torch.int32)
        argmax[torch.rand((N, F), generator=gen, device=dev) < 0.05] = -1
        idx = torch.randint(0, 50000, (N, T), generator=gen, device=dev)
        wt = torch.randn((N, F), generator=gen, device=dev)
        pos = torch.empty((N, K), dtype=torch.int32, device=dev)
        score = torch.empty((N, K), dtype=torch.float32, device=dev)
        filt, win = torch.empty_like(pos), torch.empty((N,), dtype=torch.int32, device=dev)
        tok = torch.empty((N, K, 3), dtype=torch.int64, device=dev)
        keep = {}
        for form, w in (('none', None), ('[N, F]', wt)):
            def phrases():
                _lib.call('r4r_textcnn_phrases', ptr(pooled), ptr(argmax), ptr(w), 0 if w is None else F, ptr(idx), N, T, F, K,
                          ptr(pos), ptr(score), ptr(filt), ptr(tok), ptr(win))

            def plain():
                live = (argmax >= 0) & (argmax < T + 2)
                v = pooled if w is None else pooled * w
                dense = torch.zeros((N, T + 2), dtype=torch.float32, device=dev)
                dense.scatter_add_(1, argmax.clamp(0, T + 1).long(), torch.where(live, v, torch.zeros_like(v)))
                keep['torch'] = torch.topk(dense, K)

            sides = (('phrases', phrases), ('torch', plain))
            for _ in range(2):
                for _, fn in sides:
                    fn()
            torch.cuda.synchronize()
            # (a sanity line, not a test: torch's dense form has a 0 in every empty position and sums in another order)
            first = float((pos[:, 0].long() == keep['torch'].indices[:, 0]).float().mean())
            inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in sides}
            times = {name: [] for name, _ in sides}
            for _ in range(args.repeats):
                for name, fn in sides:
                    times[name].append(timed(fn, inner[name]))
            row = dict(part='a', shape=what, rows=N, T=T, F=F, K=K, weights=form,
                       **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                       torch_over_phrases=min(times['torch']) / min(times['phrases']), first_window_equal_to_torch=first,
                       calls_per_window=inner)
            rows.append(row)
            say('  %-15s %7d %5d %9s | %9.1f .. %9.1f | %9.1f .. %9.1f | %7.2fx   (heaviest window equal to torch\'s: %.4f)' % (
                what, N, T, form, min(times['phrases']), max(times['phrases']), min(times['torch']), max(times['torch']),
                row['torch_over_phrases'], first))
        del pooled, argmax, idx, wt, tok, keep
        torch.cuda.empty_cache()


def whole_pass(args, say, rows):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue, NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (b) explain_words over every eligible item, towers=host against towers=device; tower_batch %d, k = %d, %d '
        'interleaved repeats, wall-clock milliseconds per pass (min .. max)' % (args.tower_batch, args.k, args.repeats))
    say('# %-9s %7s %9s | %21s | %21s | %8s' % ('model', 'items', 'rows', 'host ms', 'device ms', 'speedup'))
    for mt in ('deepconn', 'NARRE'):
        cfg = synthetic.hyper_params_for(CONFIG[mt])
        n_users, n_items, n_ratings = (max(1, int(cfg[k] * args.scale)) for k in ('total_users', 'total_items', 'n_train'))
        E, V = int(cfg['word_embed_size']), int(cfg['vocab'])
        d = synthesize(n_ratings, n_users, n_items, V)
        hp = dict(cfg, total_users=n_users, total_items=n_items, total_words=V, engine='native')
        hp['word_vectors'] = synthetic.word_table(V, E)
        reader = DataLoader(hp, d['train'], d['user_reviews'], d['item_reviews'], None,
                            this_index_user_item=d['this_index_user_item'], device='cuda')
        torch.manual_seed(0)
        model = reviews4rec_amd.get_model_class(mt)(hp)
        xavier_init(model)
        model = model.cuda().eval()
        cls = NarreCatalogue if mt == 'NARRE' else Catalogue
        cat = cls(model, hp, reader, tower_batch=args.tower_batch, towers='device')
        per = int(hp['narre_num_reviews']) if mt == 'NARRE' else 1

        def run(towers):
            cat.towers = towers
            return cat.explain_words(cat.eligible, k=args.k)

        last = {}
        for t in ('device', 'host'):
            last[t] = run(t)                                  # warm-up: workspaces, code objects, the pools on the device
        times = {'host': [], 'device': []}
        for _ in range(args.repeats):
            for t in ('host', 'device'):
                ms, last[t] = wall(lambda: run(t))
                times[t].append(ms)
        equal = all(torch.equal(a, b) for a, b in zip(last['host'][:7], last['device'][:7]))
        assert equal, '%s: towers=device does not give the bits of towers=host' % mt
        n = len(cat.eligible)
        row = dict(part='b', model_type=mt, items=n, rows=n * per, k=args.k, tower_batch=args.tower_batch,
                   host_ms=[min(times['host']), max(times['host'])], device_ms=[min(times['device']), max(times['device'])],
                   speedup=min(times['host']) / min(times['device']), bit_equal=bool(equal))
        rows.append(row)
        say('  %-9s %7d %9d | %9.1f .. %9.1f | %9.1f .. %9.1f | %7.2fx' % (
            mt, n, n * per, row['host_ms'][0], row['host_ms'][1], row['device_ms'][0], row['device_ms'][1], row['speedup']))
        del cat, model, reader, d, last
        torch.cuda.empty_cache()
    say('# every field of the two sides\' Phrases: bit-equal on both shapes above')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b')
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--scale', type=float, default=1.0, help="of the shapes' rows / the configurations' users, items, ratings")
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_phrases: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_phrases: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# phrase explanations; %s' % torch.cuda.get_device_name(0))
    if 'a' in args.parts.split(','):
        kernel_alone(args, say, rows)
    if 'b' in args.parts.split(','):
        whole_pass(args, say, rows)
    print(json.dumps({'bench_phrases': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
