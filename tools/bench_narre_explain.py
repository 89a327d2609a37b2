#!/usr/bin/env python
"""Times r4r_narre_explain (csrc/narre_explain.hip) at cfg4's owner counts against what a user could do before, same
process, same inputs (the method of DESIGN.md 4.14, as tools/bench_narre_catalogue.py):

    explain    one r4r_narre_explain call: attn [N, R] and the K heaviest live slots of every owner; the neighbour rows
               gathered by id inside the kernel, nothing else written
    torch      the same in plain torch (ATen + rocBLAS): other_table[nb], cat, @ W0.T + b0, relu, @ w3 + b3, softmax,
               topk over a copy with the padded slots masked to -1
    attn_fwd   at L <= 32 only: r4r_narre_attn_fwd over the materialised other_table[nb] (its out, h_save and a_save
               written), plus torch.topk over the masked a_save

Both sides of cfg4 (reviews4rec_amd/synthetic.py: 61,934 items whose neighbours are rows of the 68,225-row user table,
68,223 users against the 61,936-row item table), R = 10, K = 3.  Device events around `inner` back-to-back calls (roughly
20 ms windows), `repeats` repeats with the sides INTERLEAVED, every shape warmed up first; min .. max of the repeats are
reported.  No ratio is a gate: every row is printed, the losing ones too.

    python tools/bench_narre_explain.py [--latent 32,64] [--reviews 10] [--k 3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIDES = (('item', 61934, 68223 + 2), ('user', 68223, 61934 + 2))      # (side, owners, rows of the other side's table)


def timed(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner * 1e3            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--latent', default='32,64')
    ap.add_argument('--reviews', type=int, default=10)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_narre_explain: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    dev, R, K = 'cuda', args.reviews, args.k
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_narre_explain against plain torch and against r4r_narre_attn_fwd + torch.topk; %s; R = %d, K = %d, %d '
        'interleaved repeats, microseconds per call (min .. max)' % (torch.cuda.get_device_name(0), R, K, args.repeats))
    say('# %4s %3s %6s | %22s | %22s | %22s | %8s %9s' % ('side', 'L', 'N', 'explain us', 'torch us', 'attn_fwd + topk us',
                                                          'vs torch', 'vs attn'))
    for L in (int(x) for x in args.latent.split(',')):
        for side, N, other_rows in SIDES:
            gen = torch.Generator(device=dev).manual_seed(3000 + 17 * L + N)
            z = torch.randn((N, R, L), generator=gen, device=dev)
            table = torch.randn((other_rows, L), generator=gen, device=dev)
            nb = torch.randint(0, other_rows, (N, R), generator=gen, device=dev)
            live = torch.randint(0, R + 1, (N,), generator=gen, device=dev).to(torch.int32)
            W0 = torch.randn((L, 2 * L), generator=gen, device=dev) * 0.4
            b0 = torch.randn((L,), generator=gen, device=dev) * 0.1
            w3 = torch.randn((1, L), generator=gen, device=dev) * 0.4
            b3 = torch.randn((1,), generator=gen, device=dev)
            attn = torch.empty((N, R), dtype=torch.float32, device=dev)
            slot = torch.empty((N, K), dtype=torch.int32, device=dev)
            tw = torch.empty((N, K), dtype=torch.float32, device=dev)
            padded = torch.arange(R, device=dev)[None, :] >= live[:, None]
            keep = {}

            def explain():
                _lib.call('r4r_narre_explain', ptr(z), ptr(nb), ptr(table), other_rows, None, None, ptr(live), ptr(W0),
                          ptr(b0), ptr(w3), ptr(b3), None, ptr(attn), ptr(slot), ptr(tw), K, N, R, L)

            def plain():
                h = torch.relu(torch.cat([z, table[nb]], -1) @ W0.T + b0)
                a = torch.softmax((h @ w3.reshape(-1)) + b3, dim=1)
                keep['torch'] = (a, torch.topk(a.masked_fill(padded, -1.0), K))

            old_ok = R <= 32 and L <= 32
            out = torch.empty((N, L), dtype=torch.float32, device=dev)
            h_save = torch.empty((N, R, L), dtype=torch.float32, device=dev) if old_ok else None
            a_save = torch.empty((N, R), dtype=torch.float32, device=dev)

            def attn_fwd():
                other = table[nb].contiguous()
                _lib.call('r4r_narre_attn_fwd', ptr(z), ptr(other), ptr(W0), ptr(b0), ptr(w3), ptr(b3), None, ptr(out),
                          ptr(h_save), ptr(a_save), N, R, L)
                keep['old'] = torch.topk(a_save.masked_fill(padded, -1.0), K)

            sides = [('explain', explain), ('torch', plain)] + ([('attn_fwd', attn_fwd)] if old_ok else [])
            for _ in range(2):                                # warm-up: code objects, rocBLAS' choice
                for _, fn in sides:
                    fn()
            torch.cuda.synchronize()
            # (a sanity line, not a test: the same heaviest slot as torch wherever torch lists a live one)
            t_slot = keep['torch'][1].indices[:, 0]
            first_ok = float(((slot[:, 0].long() == t_slot) | (live == 0)).float().mean())
            worst = float((attn - keep['torch'][0]).abs().max())
            inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in sides}
            times = {name: [] for name, _ in sides}
            for _ in range(args.repeats):
                for name, fn in sides:
                    times[name].append(timed(fn, inner[name]))
            row = dict(side=side, L=L, N=N, R=R, K=K, other_rows=other_rows,
                       **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                       torch_over_explain=min(times['torch']) / min(times['explain']),
                       attn_fwd_over_explain=(min(times['attn_fwd']) / min(times['explain'])) if old_ok else None,
                       first_slot_equal_to_torch=first_ok, max_abs_attn_difference_to_torch=worst, calls_per_window=inner)
            rows.append(row)
            cell = lambda name: ('%9.1f .. %9.1f' % (min(times[name]), max(times[name]))) if name in times else '%22s' % 'refused (L > 32)'
            say('  %4s %3d %6d | %s | %s | %s | %8.2fx %9s' % (
                side, L, N, cell('explain'), cell('torch'), cell('attn_fwd'), row['torch_over_explain'],
                ('%8.2fx' % row['attn_fwd_over_explain']) if old_ok else '-'))
    say('# heaviest slot equal to torch\'s / max |attn - torch|: ' + ', '.join(
        '%s L=%d %.4f / %.1e' % (r['side'], r['L'], r['first_slot_equal_to_torch'], r['max_abs_attn_difference_to_torch'])
        for r in rows))
    print(json.dumps({'bench_narre_explain': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
