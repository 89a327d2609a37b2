#!/usr/bin/env python
"""Times the pair explanations (include/r4r.h, "Pair gradients"), in the form of tools/bench_phrases.py:

(a) r4r_pair_grad alone (csrc/pair_grad.hip) for the three head kinds at L in {32, 64}, F = 100, all five outputs
    written, n_p in {128, 8,192, 1,048,576} random pairs over 4,096 users and 4,096 items (pfm with the five id-embedding
    columns of transnet++) -- against the same closed forms written as batched torch matmuls on the device (gathers of
    the pairs' rows, matmuls, elementwise ops; nothing the kernel could not be compared with bit for bit is claimed:
    torch sums in another order).  Device events around `inner` back-to-back calls (~20 ms windows), every shape
    warmed up, sides INTERLEAVED, `repeats` repeats, min .. max.
(b) ``explain_pair`` end to end for every training user's top-10 list with towers='device' on synthetic pools at cfg3's
    cardinalities (DeepCoNN): the towers of the distinct owners, one r4r_pair_grad call, and the two phrase passes over
    the pairs' rows; wall clock with a device synchronise inside every window, min .. max, and the share of the
    ``pair_weights`` step alone.

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_pair_explain.py [--parts a,b] [--k 5] [--top 10] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
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

LS, F, P, RANK = (32, 64), 100, 5, 8
PAIRS = (128, 8192, 1048576)
OWNERS = 4096
CONFIG = 'cfg3_deepconn_electronics_e300'


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


def torch_forms(kind, zu, zi, u, i, p, fc_u, fc_i, qb, cb, L):
    """The closed forms of include/r4r.h as batched torch ops -> (score, g_user, g_item, w_user, w_item)."""
    x = torch.cat([zu[u], zi[i]], 1)

    def fm(y, V, lw):
        s = y @ V
        v2 = (V * V).sum(1)
        head = 0.5 * ((s * s).sum(1) - (y * y) @ v2) + y @ lw
        return head, lw + s @ V.T - y * v2

    if kind == 'fm':
        head, g = fm(x, p['V'], p['lw'])
    else:
        a = torch.addmm(p['b0'], x, p['W0'].T)
        on = a > 0
        if kind == 'mlp':
            head = torch.relu(a) @ p['w3']
            up = on * p['w3']
        else:
            ir = torch.addmm(p['b2'], torch.relu(a), p['W2'].T)
            head, gy = fm(torch.cat([p['xu'][u], p['xi'][i], ir], 1), p['V'], p['lw'])
            up = on * (gy[:, 2 * P:] @ p['W2'])
        g = up @ p['W0']
    return head + qb[u] + cb[i], g[:, :L], g[:, L:], g[:, :L] @ fc_u, g[:, L:] @ fc_i


def kernel_alone(args, say, rows):
    from reviews4rec_amd import ops
    dev = 'cuda'
    say('# (a) r4r_pair_grad against batched torch matmuls; F = %d, all outputs, %d users x %d items, %d interleaved repeats, '
        'microseconds per call (min .. max)' % (F, OWNERS, OWNERS, args.repeats))
    say('# %-5s %3s %9s | %22s | %22s | %8s | %s' % ('kind', 'L', 'pairs', 'pair_grad us', 'torch us', 'vs torch', 'max |w - torch|'))
    for kind in ('fm', 'mlp', 'pfm'):
        for L in LS:
            gen = torch.Generator(device=dev).manual_seed(9000 + L)
            r = lambda *s: torch.randn(s, generator=gen, device=dev)
            n = 2 * L if kind == 'fm' else 2 * P + L
            p = {}
            if kind != 'fm':
                p.update(W0=r(L, 2 * L) * 0.2, b0=r(L) * 0.1)
            if kind == 'mlp':
                p.update(w3=r(L) * 0.4)
            if kind == 'pfm':
                p.update(W2=r(L, L) * 0.2, b2=r(L) * 0.1, xu=r(OWNERS, P), xi=r(OWNERS, P))
            if kind != 'mlp':
                p.update(V=r(n, RANK) * 0.3, lw=r(n) * 0.3)
            zu, zi, fc_u, fc_i = r(OWNERS, L), r(OWNERS, L), r(L, F) * 0.3, r(L, F) * 0.3
            qb, cb = r(OWNERS), r(OWNERS)
            for n_p in PAIRS:
                n_p = max(1, int(n_p * args.scale))
                u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
                i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
                keep = {}

                def native():
                    keep['native'] = ops.pair_grad(kind, zu, zi, u, i, q_bias=qb, c_bias=cb, fc_u=fc_u, fc_i=fc_i, **p)

                def plain():
                    keep['torch'] = torch_forms(kind, zu, zi, u, i, p, fc_u, fc_i, qb, cb, L)

                sides = (('native', native), ('torch', plain))
                for _ in range(2):
                    for _, fn in sides:
                        fn()
                torch.cuda.synchronize()
                # (sanity figures, not a test: tests/test_gpu_pair_grad.py holds the kernel to float64.  A pair is "apart"
                # when some w_user element differs by more than 1e-3: among a million pairs a few pre-activations lie
                # within rounding of zero, and the two summation orders then take different ReLU branches)
                diff = (keep['native']['w_user'] - keep['torch'][3]).abs().amax(1)
                apart, apart_pairs = float(diff[diff <= 1e-3].max()), int((diff > 1e-3).sum())
                inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in sides}
                times = {name: [] for name, _ in sides}
                for _ in range(args.repeats):
                    for name, fn in sides:
                        times[name].append(timed(fn, inner[name]))
                row = dict(part='a', kind=kind, L=L, F=F, pairs=n_p, **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                           torch_over_native=min(times['torch']) / min(times['native']), max_abs_w_user_apart=apart, pairs_on_another_relu_branch=apart_pairs,
                           calls_per_window=inner)
                rows.append(row)
                say('  %-5s %3d %9d | %9.1f .. %9.1f | %9.1f .. %9.1f | %7.2fx | %.2e, %d pairs on another ReLU branch' % (
                    kind, L, n_p, min(times['native']), max(times['native']), min(times['torch']), max(times['torch']),
                    row['torch_over_native'], apart, apart_pairs))
                del keep, u, i
                torch.cuda.empty_cache()


def whole_pass(args, say, rows):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.recommend import recommended_pairs
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (b) explain_pair of every training user\'s top-%d, towers=device; tower_batch %d, k = %d, %d repeats, wall-clock '
        'milliseconds per pass (min .. max)' % (args.top, args.tower_batch, args.k, args.repeats))
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
    cat = Catalogue(model, hp, reader, tower_batch=args.tower_batch, towers='device')
    users, items = recommended_pairs(cat, args.top)
    cat.explain_pair(users[:64], items[:64], k=args.k)       # warm-up: workspaces, code objects, the pools on the device
    cat.pair_weights(users, items)
    whole, weights = [], []
    for _ in range(args.repeats):
        ms, _ = wall(lambda: cat.pair_weights(users, items))
        weights.append(ms)
        ms, e = wall(lambda: cat.explain_pair(users, items, k=args.k))
        whole.append(ms)
    row = dict(part='b', model_type='deepconn', users=int(len(set(users.tolist()))), items=int(len(cat.eligible)),
               pairs=int(len(users)), k=args.k, tower_batch=args.tower_batch, explain_pair_ms=[min(whole), max(whole)],
               pair_weights_ms=[min(weights), max(weights)])
    rows.append(row)
    say('# %-9s %7s %7s %9s | %23s | %23s' % ('model', 'users', 'items', 'pairs', 'explain_pair ms', 'of which pair_weights ms'))
    say('  %-9s %7d %7d %9d | %10.1f .. %10.1f | %10.1f .. %10.1f' % (
        'deepconn', row['users'], row['items'], row['pairs'], min(whole), max(whole), min(weights), max(weights)))
    assert tuple(e.user.positions.shape) == (len(users), args.k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b')
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the pair counts / the configuration's users, items, ratings")
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pair_explain: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_pair_explain: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# pair explanations; %s' % torch.cuda.get_device_name(0))
    if 'a' in args.parts.split(','):
        kernel_alone(args, say, rows)
    if 'b' in args.parts.split(','):
        whole_pass(args, say, rows)
    print(json.dumps({'bench_pair_explain': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
