#!/usr/bin/env python
"""Times r4r_topk_relu (csrc/topk_relu.hip) on synthetic tables against the plain-torch yardstick, same process, same
inputs (the method of DESIGN.md 4.14, as tools/bench_recommend.py):

    fused      one r4r_topk_relu call (scan + merge launches), scores never written to memory
    yardstick  torch.topk((torch.relu(qa[:, None, :] + ca[None, :, :]) * w).sum(-1) + qp @ cp.T + c_bias + q_bias[:, None], K)
               in query chunks of at most 2 GiB of the [queries, n_c, H] intermediate (ATen + rocBLAS, materialised)

Device events around `inner` back-to-back calls (roughly 20 ms windows), `repeats` repeats of each side INTERLEAVED,
every shape warmed up first; min .. max of the repeats are reported, with the ratio of the minima and the share of the
VALU roof the fused call reaches: (3 H + P) lane-instructions per pair at 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz =
39.3 T lane-instructions/s (a roof, not a measurement; packed fp32 instructions can go below it).

    python tools/bench_relu_catalogue.py [--n-c 1000000] [--shapes 10x0,64x0,64x64] [--queries 1,128,4096] [--k 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9
YARDSTICK_BYTES = 1 << 31


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
    ap.add_argument('--n-c', type=int, default=1000000)
    ap.add_argument('--shapes', default='10x0,64x0,64x64', help='HxP, comma separated')
    ap.add_argument('--queries', default='1,128,4096')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_relu_catalogue: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, K, n_c = 'cuda', args.k, args.n_c
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_topk_relu against torch.topk over the materialised ReLU-sum; %s; n_c = %d, K = %d, %d interleaved repeats, '
        'microseconds per call (min .. max)' % (torch.cuda.get_device_name(0), n_c, K, args.repeats))
    say('# %4s %4s %6s | %23s | %25s | %8s | %9s' % ('H', 'P', 'n_q', 'fused us', 'yardstick us', 'speedup', 'of VALU'))
    for H, P in (tuple(int(x) for x in s.split('x')) for s in args.shapes.split(',')):
        gen = torch.Generator(device=dev).manual_seed(1000 + 17 * H + P)
        c = torch.randn((n_c, H + P), generator=gen, device=dev)
        c_bias = torch.randn((n_c,), generator=gen, device=dev)
        w = torch.randn((max(H, 1),), generator=gen, device=dev)
        ca, cp = c[:, :H], c[:, H:]
        for n_q in (int(n) for n in args.queries.split(',')):
            q = torch.randn((n_q, H + P), generator=gen, device=dev)
            q_bias = torch.randn((n_q,), generator=gen, device=dev)
            ids = torch.empty((n_q, K), dtype=torch.int64, device=dev)
            sc = torch.empty((n_q, K), dtype=torch.float32, device=dev)
            nb = lib.r4r_topk_relu_ws_bytes(n_q, n_c, K, args.chunk)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)

            def fused():
                _lib.call('r4r_topk_relu', ptr(q), n_q, ptr(q_bias), ptr(c), n_c, H + P, ptr(c_bias), ptr(w), H, P, None,
                          None, K, args.chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))

            step = max(1, min(n_q, YARDSTICK_BYTES // (4 * n_c * max(H, 1))))
            yard_out = []

            def yardstick():
                yard_out.clear()
                for a in range(0, n_q, step):
                    qa, qp = q[a:a + step, :H], q[a:a + step, H:]
                    s = c_bias + q_bias[a:a + step, None]
                    if H:
                        s = s + (torch.relu(qa[:, None, :] + ca[None, :, :]) * w[:H]).sum(-1)
                    if P:
                        s = s + qp @ cp.T
                    yard_out.append(torch.topk(s, K))

            fused(); yardstick(); fused(); yardstick()                       # warm-up: code objects, rocBLAS' choice
            torch.cuda.synchronize()
            y_ids = torch.cat([y.indices for y in yard_out])
            agree = float((y_ids == ids).float().mean())
            inner_f = max(1, min(200, int(20000 / max(timed(fused, 3), 1.0))))      # ~20 ms of work per timed window
            inner_y = max(1, min(200, int(20000 / max(timed(yardstick, 1), 1.0))))
            tf, ty = [], []
            for _ in range(args.repeats):
                tf.append(timed(fused, inner_f))
                ty.append(timed(yardstick, inner_y))
            roof = float(n_q) * n_c * (3 * H + P) / VALU_LANE_OPS * 1e6
            row = dict(H=H, P=P, n_q=n_q, n_c=n_c, K=K, fused_us=[min(tf), max(tf)], yardstick_us=[min(ty), max(ty)],
                       speedup=min(ty) / min(tf), valu_roof_us=roof, share_of_valu_roof=roof / min(tf),
                       fused_range_above_yardstick=min(tf) > max(ty), ids_equal_to_torch=agree,
                       calls_per_window=[inner_f, inner_y])
            rows.append(row)
            say('  %4d %4d %6d | %10.1f .. %10.1f | %11.1f .. %11.1f | %7.2fx | %8.1f%%%s' % (
                H, P, n_q, min(tf), max(tf), min(ty), max(ty), row['speedup'], 100 * row['share_of_valu_roof'],
                '   FUSED RANGE ABOVE THE YARDSTICK' if row['fused_range_above_yardstick'] else ''))
        del c, ca, cp
        torch.cuda.empty_cache()
    say('# ids equal to torch.topk (which breaks ties and rounds its sums differently): ' +
        ', '.join('H=%d P=%d n_q=%d %.4f' % (r['H'], r['P'], r['n_q'], r['ids_equal_to_torch']) for r in rows))
    print(json.dumps({'bench_relu_catalogue': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
