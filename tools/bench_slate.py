#!/usr/bin/env python
"""Times the slate calls (csrc/slate_device.h; include/r4r.h "Slates") on synthetic tables against two yardsticks, same
process, same inputs, per score form at a small and at its largest head:

    lists      one r4r_slate_topk_<form> call at K = 10 over n_s slates of C entries
    ranks      one r4r_slate_rank_<form> call over the same slates, one target each
    (a) pairs  what a user can do without them: r4r_pair_<form> over every entry (n_s x C pairs, the indices already on
               the device) + torch.topk over the [n_s, C] scores
    (b) full   r4r_rank_<form> over the WHOLE catalogue for the same pairs: what eval_catalogue costs

Device events around `inner` back-to-back calls, `repeats` repeats of the four sides INTERLEAVED, every shape warmed up
first; min .. max of the repeats are reported with the ratios of the minima.  No ratio is a gate: every row is
reported, the losing ones too.  A size whose yardstick (a) needs more than --fit-bytes of indices and scores is dropped
and named.

    python tools/bench_slate.py [--n-c 63001] [--slates 100,1000] [--n-s 1,1024,131072] [--forms dot,relu,hmlp,rfm,pfm]
                                [--out profiles/slate_ab.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# form -> [(label, shape)]: a small head and the largest instantiation
HEADS = {
    'dot': [('D=8', (8,)), ('D=256', (256,))],
    'relu': [('H=8 P=8', (8, 8)), ('H=128 P=128', (128, 128))],
    'hmlp': [('D=8 H=8', (8, 8)), ('D=64 H=64', (64, 64))],
    'rfm': [('H=6 P=8 M=15', (6, 8, 15)), ('H=64 P=16 M=80', (64, 16, 80))],
    'pfm': [('H=6 G=6 M=12', (6, 6, 12)), ('H=64 G=64 M=128', (64, 64, 128))],
}


def timed(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner * 1e3            # microseconds per call


def head_tail(form, shape, gen, dev):
    """-> (row width, the head's trailing arguments after c_bias as tensors / ints, kept alive by the caller)."""
    f = lambda *s: torch.randn(s, generator=gen, device=dev)
    if form == 'dot':
        return shape[0], [shape[0]]
    if form == 'relu':
        H, P = shape
        return H + P, [f(H), H, P]
    if form == 'hmlp':
        D, H = shape
        return D, [f(H, D) / max(D, 1) ** 0.5, 0.1 * f(H), f(H), D, H]
    if form == 'rfm':
        H, P, M = shape
        D = H + P
        s = torch.full((M,), -0.5, device=dev)
        s[:8] = 0.5
        l = torch.zeros((M,), device=dev)
        l[-1] = 1.0
        return D, [f(M, D) / D ** 0.5, 0.1 * f(M), s, l, H, P, M]
    H, G, M = shape
    D = H + G
    s = torch.full((M,), -0.5, device=dev)
    s[:M // 2] = 0.5
    return D, [f(M, D) / D ** 0.5, 0.1 * f(M), s, -0.5 / D * f(D) ** 2, f(D) / D ** 0.5, H, G, M]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-c', type=int, default=63001)
    ap.add_argument('--slates', default='100,1000')
    ap.add_argument('--n-s', default='1,1024,131072')
    ap.add_argument('--forms', default='dot,relu,hmlp,rfm,pfm')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window-us', type=float, default=5000.0, help='work per timed window')
    ap.add_argument('--fit-bytes', type=int, default=1 << 30, help='most that yardstick (a) may hold in indices and scores')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_slate: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, n_c, K = 'cuda', args.n_c, 10
    lines, rows, dropped = [], [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_slate_topk_<form> at K = %d and r4r_slate_rank_<form> against (a) r4r_pair_<form> over every entry + torch.topk '
        'and (b) r4r_rank_<form> over the whole catalogue; %s; n_c = %d, piece = %d, %d interleaved repeats, microseconds per '
        'call (min .. max)' % (K, torch.cuda.get_device_name(0), n_c, lib.r4r_slate_piece(), args.repeats))
    say('# %-5s %-16s %5s %7s | %21s | %21s | %21s | %23s | %9s %9s' % (
        'form', 'head', 'C', 'n_s', 'lists us', 'ranks us', '(a) pairs + topk us', '(b) full-catalogue rank us', '(a)/lists',
        '(b)/ranks'))
    for form in args.forms.split(','):
        for label, shape in HEADS[form]:
            gen = torch.Generator(device=dev).manual_seed(1000 + sum(shape))
            width, tail = head_tail(form, shape, gen, dev)
            c = torch.randn((n_c, max(width, 1)), generator=gen, device=dev)
            c_bias = 0.3 * torch.randn((n_c,), generator=gen, device=dev)
            targs = [ptr(a) if isinstance(a, torch.Tensor) else a for a in tail]
            for C in (int(x) for x in args.slates.split(',')):
                for n_s in (int(x) for x in args.n_s.split(',')):
                    if n_s * C * 20 > args.fit_bytes:
                        dropped.append('%s %s C=%d n_s=%d' % (form, label, C, n_s))
                        continue
                    n_q = n_s                                              # one query row per slate
                    q = torch.randn((n_q, max(width, 1)), generator=gen, device=dev)
                    q_bias = torch.randn((n_q,), generator=gen, device=dev)
                    head = [ptr(q), n_q, ptr(q_bias), ptr(c), n_c, max(width, 1), ptr(c_bias)] + targs
                    qi = torch.arange(n_s, dtype=torch.int64, device=dev)
                    start = torch.randint(0, n_c, (n_s, 1), generator=gen, device=dev)
                    stride = torch.randint(1, max(2, n_c // C), (n_s, 1), generator=gen, device=dev)
                    ids = ((start + stride * torch.arange(C, device=dev)[None, :]) % n_c).contiguous()   # distinct per slate
                    off = torch.arange(n_s + 1, dtype=torch.int64, device=dev) * C
                    ti = ids[:, 0].contiguous()
                    pq = qi[:, None].expand(n_s, C).contiguous()
                    out_i = torch.empty((n_s, K), dtype=torch.int64, device=dev)
                    out_s = torch.empty((n_s, K), dtype=torch.float32, device=dev)
                    ranks = torch.empty((n_s,), dtype=torch.int64, device=dev)
                    rsc = torch.empty((n_s,), dtype=torch.float32, device=dev)
                    full_r, full_s = torch.empty_like(ranks), torch.empty_like(rsc)
                    scores = torch.empty((n_s, C), dtype=torch.float32, device=dev)
                    nb = lib.r4r_slate_ws_bytes(n_s, C, K)
                    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
                    top = []

                    def lists():
                        _lib.call('r4r_slate_topk_' + form, *head, ptr(qi), ptr(off), ptr(ids), n_s, C, None, None, K,
                                  ptr(ws), int(nb), ptr(out_i), ptr(out_s))

                    def slate_ranks():
                        _lib.call('r4r_slate_rank_' + form, *head, ptr(qi), ptr(ti), ptr(off), ptr(ids), n_s, C, None, None,
                                  ptr(ranks), ptr(rsc))

                    def pairs_topk():
                        _lib.call('r4r_pair_' + form, *head, ptr(pq), ptr(ids), n_s * C, ptr(scores))
                        top[:] = [torch.topk(scores, min(K, C), dim=1)]

                    def full_rank():
                        _lib.call('r4r_rank_' + form, *head, ptr(qi), ptr(ti), n_s, None, None, 0, ptr(full_r), ptr(full_s))

                    sides = (lists, slate_ranks, pairs_topk, full_rank)
                    for f in sides + sides:                                # warm-up: code objects, ATen's choice
                        f()
                    torch.cuda.synchronize()
                    agree = float((top[0].values == out_s[:, :min(K, C)]).float().mean())
                    inner = [max(1, min(200, int(args.window_us / max(timed(f, 1), 1.0)))) for f in sides]
                    t = [[] for _ in sides]
                    for _ in range(args.repeats):
                        for k, f in enumerate(sides):
                            t[k].append(timed(f, inner[k]))
                    lo, hi = [min(x) for x in t], [max(x) for x in t]
                    row = dict(form=form, head=label, C=C, n_s=n_s, n_c=n_c, lists_us=[lo[0], hi[0]], ranks_us=[lo[1], hi[1]],
                               pairs_topk_us=[lo[2], hi[2]], full_rank_us=[lo[3], hi[3]], pairs_over_lists=lo[2] / lo[0],
                               full_over_ranks=lo[3] / lo[1], list_scores_equal_to_topk=agree, calls_per_window=inner)
                    rows.append(row)
                    say('  %-5s %-16s %5d %7d | %9.1f .. %9.1f | %9.1f .. %9.1f | %9.1f .. %9.1f | %10.1f .. %10.1f | %8.2fx %8.2fx' % (
                        form, label, C, n_s, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], row['pairs_over_lists'],
                        row['full_over_ranks']))
            torch.cuda.empty_cache()
    say('# dropped (yardstick (a) above %d bytes of indices and scores): %s' % (args.fit_bytes, ', '.join(dropped) or 'none'))
    say('# list scores equal to torch.topk over the pair scores, worst share: %.4f'
        % min([r['list_scores_equal_to_topk'] for r in rows] + [1.0]))
    print(json.dumps({'bench_slate': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
