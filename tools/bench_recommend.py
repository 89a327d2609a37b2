#!/usr/bin/env python
"""Times r4r_topk_dot (csrc/topk.hip) on synthetic tables against the plain-torch yardstick, same process, same inputs:

    fused      one r4r_topk_dot call (scan + merge launches), scores never written to memory
    yardstick  torch.topk(q @ c.T + c_bias + q_bias[:, None], K) in query chunks of at most 2 GiB of scores
               (rocBLAS + ATen, the scores materialised)

Device events around `inner` back-to-back calls, `repeats` repeats of each side INTERLEAVED (fused, yardstick, fused,
...), every shape warmed up first; min .. max of the repeats are reported, with the ratio of the minima and the share of
each roof the fused call reaches:

    bytes   n_c x D x 4 read once per query tile (16 queries, or 64 when n_q >= 512 and D <= 128) at 6.3 TB/s
    flops   2 x n_q x n_c x D at 155 TFLOP/s of fp32 MFMA

    python tools/bench_recommend.py [--n-c 1000000] [--dims 8,64] [--queries 1,128,4096] [--k 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S, MFMA_F32_FLOPS = 6.3e12, 155e12
YARDSTICK_SCORE_BYTES = 1 << 31


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
    ap.add_argument('--dims', default='8,64')
    ap.add_argument('--queries', default='1,128,4096')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_recommend: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, K, n_c = 'cuda', args.k, args.n_c
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_topk_dot against torch.topk(q @ c.T + c_bias + q_bias[:, None], K); %s; n_c = %d, K = %d, %d interleaved '
        'repeats, microseconds per call (min .. max)' % (torch.cuda.get_device_name(0), n_c, K, args.repeats))
    say('# %5s %6s | %23s | %23s | %7s | %9s %9s' % ('D', 'n_q', 'fused us', 'yardstick us', 'speedup', 'of bytes', 'of flops'))
    for D in (int(d) for d in args.dims.split(',')):
        gen = torch.Generator(device=dev).manual_seed(1000 + D)
        c = torch.randn((n_c, D), generator=gen, device=dev)
        c_bias = torch.randn((n_c,), generator=gen, device=dev)
        for n_q in (int(n) for n in args.queries.split(',')):
            q = torch.randn((n_q, D), generator=gen, device=dev)
            q_bias = torch.randn((n_q,), generator=gen, device=dev)
            ids = torch.empty((n_q, K), dtype=torch.int64, device=dev)
            sc = torch.empty((n_q, K), dtype=torch.float32, device=dev)
            nb = lib.r4r_topk_dot_ws_bytes(n_q, n_c, K, args.chunk)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)

            def fused():
                _lib.call('r4r_topk_dot', ptr(q), n_q, ptr(q_bias), ptr(c), n_c, D, ptr(c_bias), D, None, None, K,
                          args.chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))

            step = max(1, min(n_q, YARDSTICK_SCORE_BYTES // (4 * n_c)))
            yard_out = []

            def yardstick():
                yard_out.clear()
                for a in range(0, n_q, step):
                    yard_out.append(torch.topk(q[a:a + step] @ c.T + c_bias + q_bias[a:a + step, None], K))

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
            tile = 64 if (n_q >= 512 and D <= 128) else 16
            roof_b = -(-n_q // tile) * n_c * D * 4 / HBM_BYTES_PER_S * 1e6
            roof_f = 2.0 * n_q * n_c * D / MFMA_F32_FLOPS * 1e6
            row = dict(D=D, n_q=n_q, n_c=n_c, K=K, fused_us=[min(tf), max(tf)], yardstick_us=[min(ty), max(ty)],
                       speedup=min(ty) / min(tf), bytes_roof_us=roof_b, flops_roof_us=roof_f,
                       share_of_bytes_roof=roof_b / min(tf), share_of_flops_roof=roof_f / min(tf),
                       fused_range_above_yardstick=min(tf) > max(ty), ids_equal_to_torch=agree,
                       calls_per_window=[inner_f, inner_y])
            rows.append(row)
            say('  %5d %6d | %10.1f .. %10.1f | %10.1f .. %10.1f | %6.2fx | %8.1f%% %8.1f%%%s' % (
                D, n_q, min(tf), max(tf), min(ty), max(ty), row['speedup'], 100 * row['share_of_bytes_roof'],
                100 * row['share_of_flops_roof'], '   FUSED RANGE ABOVE THE YARDSTICK' if row['fused_range_above_yardstick'] else ''))
        torch.cuda.empty_cache()
    say('# ids equal to torch.topk (which breaks ties and rounds its GEMM differently): ' +
        ', '.join('D=%d n_q=%d %.4f' % (r['D'], r['n_q'], r['ids_equal_to_torch']) for r in rows))
    print(json.dumps({'bench_recommend': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
