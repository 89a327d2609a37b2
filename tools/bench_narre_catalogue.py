#!/usr/bin/env python
"""Times r4r_topk_hmlp (csrc/topk_hmlp.hip) on synthetic tables against the plain-torch yardstick, same process, same
inputs (the method of DESIGN.md 4.14, as tools/bench_recommend.py and tools/bench_relu_catalogue.py):

    fused      one r4r_topk_hmlp call (scan + merge launches), neither q * c nor a score ever written to memory
    yardstick  torch.topk(relu((q[:, None] * c[None]).reshape(-1, D) @ W.T + b) @ w + c_bias + q_bias[:, None], K)
               in query chunks of at most 2 GiB of the [queries, n_c, D] and [queries, n_c, H] intermediates (ATen +
               rocBLAS, materialised) and at most 2^24 rows of them: with 22 * 10^6 rows (D = 8, H = 16) the yardstick's
               ids agreed with a float64 reference in a fifth of the places only, with 8 * 10^6 in all of them, and the
               fused call's in all of them either way

Device events around `inner` back-to-back calls (roughly 20 ms windows), `repeats` repeats of each side INTERLEAVED,
every shape warmed up first; min .. max of the repeats are reported, with the ratio of the minima and the share of the
flops roof the fused call reaches: 2 n_q n_c H D flops (H and D as given, not as padded) against the 155 TF of fp32
MFMA that DESIGN.md uses (a roof, not a measurement).

    python tools/bench_narre_catalogue.py [--n-c 1000000] [--shapes 8x16,32x32,64x64] [--queries 1,128,1024] [--k 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_FLOPS = 155e12
YARDSTICK_BYTES = 1 << 31
YARDSTICK_ROWS = 1 << 24


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
    ap.add_argument('--shapes', default='8x16,32x32,64x64', help='DxH, comma separated')
    ap.add_argument('--queries', default='1,128,1024')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_narre_catalogue: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, K, n_c = 'cuda', args.k, args.n_c
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_topk_hmlp against torch.topk over the materialised product-MLP head; %s; n_c = %d, K = %d, %d interleaved '
        'repeats, microseconds per call (min .. max)' % (torch.cuda.get_device_name(0), n_c, K, args.repeats))
    say('# %4s %4s %6s | %23s | %25s | %8s | %9s' % ('D', 'H', 'n_q', 'fused us', 'yardstick us', 'speedup', 'of roof'))
    for D, H in (tuple(int(x) for x in s.split('x')) for s in args.shapes.split(',')):
        gen = torch.Generator(device=dev).manual_seed(2000 + 17 * D + H)
        c = torch.randn((n_c, D), generator=gen, device=dev)
        c_bias = torch.randn((n_c,), generator=gen, device=dev)
        W = torch.randn((H, D), generator=gen, device=dev)
        b = torch.randn((H,), generator=gen, device=dev)
        w = torch.randn((H,), generator=gen, device=dev)
        for n_q in (int(n) for n in args.queries.split(',')):
            q = torch.randn((n_q, D), generator=gen, device=dev)
            q_bias = torch.randn((n_q,), generator=gen, device=dev)
            ids = torch.empty((n_q, K), dtype=torch.int64, device=dev)
            sc = torch.empty((n_q, K), dtype=torch.float32, device=dev)
            nb = lib.r4r_topk_hmlp_ws_bytes(n_q, n_c, K, args.chunk)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)

            def fused():
                _lib.call('r4r_topk_hmlp', ptr(q), n_q, ptr(q_bias), ptr(c), n_c, D, ptr(c_bias), ptr(W), ptr(b), ptr(w), D, H,
                          None, None, K, args.chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))

            step = max(1, min(n_q, YARDSTICK_BYTES // (4 * n_c * (D + H)), YARDSTICK_ROWS // n_c))
            yard_out = []

            def yardstick():
                yard_out.clear()
                for a in range(0, n_q, step):
                    qa = q[a:a + step]
                    x = (qa[:, None, :] * c[None, :, :]).reshape(-1, D)
                    s = (torch.relu(x @ W.T + b) @ w).view(qa.shape[0], n_c) + c_bias + q_bias[a:a + step, None]
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
            roof = 2.0 * n_q * n_c * H * D / MFMA_F32_FLOPS * 1e6
            row = dict(D=D, H=H, n_q=n_q, n_c=n_c, K=K, fused_us=[min(tf), max(tf)], yardstick_us=[min(ty), max(ty)],
                       speedup=min(ty) / min(tf), flops_roof_us=roof, share_of_flops_roof=roof / min(tf),
                       fused_range_above_yardstick=min(tf) > max(ty), fused_range_below_yardstick=max(tf) < min(ty),
                       ids_equal_to_torch=agree, calls_per_window=[inner_f, inner_y])
            rows.append(row)
            say('  %4d %4d %6d | %10.1f .. %10.1f | %11.1f .. %11.1f | %7.2fx | %8.1f%%%s' % (
                D, H, n_q, min(tf), max(tf), min(ty), max(ty), row['speedup'], 100 * row['share_of_flops_roof'],
                '' if row['fused_range_below_yardstick'] else '   FUSED RANGE NOT BELOW THE YARDSTICK'))
        del c
        torch.cuda.empty_cache()
    say('# ids equal to torch.topk (which breaks ties and rounds its sums differently): ' +
        ', '.join('D=%d H=%d n_q=%d %.4f' % (r['D'], r['H'], r['n_q'], r['ids_equal_to_torch']) for r in rows))
    print(json.dumps({'bench_narre_catalogue': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
