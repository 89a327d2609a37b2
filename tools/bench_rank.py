#!/usr/bin/env python
"""Times r4r_rank_dot (csrc/topk.hip) on synthetic tables against two yardsticks, same process, same inputs:

    fused      one r4r_rank_dot call (target and scan launches; no exclusions: neither yardstick has them), scores never written
    torch      ((q[qi] @ c.T + cb + qb[qi, None]) > s_t[:, None]).sum(1) in pair chunks of at most 2 GiB of scores
               (rocBLAS + ATen, the scores materialised; ties and ineligible rows not even handled)
    lists      r4r_topk_dot at K = 10 for as many query ROWS as there are pairs: what the sorted lists cost on top

Device events around `inner` back-to-back calls, `repeats` repeats of the three sides INTERLEAVED, every shape warmed
up first; min .. max of the repeats are reported, with the ratios of the minima and the share of each roof of
DESIGN 4.14 the fused call reaches:

    bytes   n_c x D x 4 read once per pair tile (16 pairs, or 64 as the library chooses) at 6.3 TB/s
    flops   2 x n_p x n_c x D at 155 TFLOP/s of fp32 MFMA

    python tools/bench_rank.py [--n-c 1000000] [--dims 8,64] [--pairs 1,128,4096,131072] [--wide-from 512] [--out FILE]
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
    ap.add_argument('--pairs', default='1,128,4096,131072')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--wide-from', type=int, default=512, help='pairs from which the library runs 64-pair tiles (roof only)')
    ap.add_argument('--window-us', type=float, default=20000.0, help='work per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rank: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, n_c, K = 'cuda', args.n_c, 10
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_rank_dot against plain torch (scores materialised, > only) and against r4r_topk_dot at K = %d for as many '
        'query rows; %s; n_c = %d, %d interleaved repeats, microseconds per call (min .. max)'
        % (K, torch.cuda.get_device_name(0), n_c, args.repeats))
    say('# %5s %7s | %23s | %25s | %23s | %8s %8s | %9s %9s' % ('D', 'n_p', 'fused us', 'torch us', 'lists us', '/ torch',
                                                               '/ lists', 'of bytes', 'of flops'))
    for D in (int(d) for d in args.dims.split(',')):
        gen = torch.Generator(device=dev).manual_seed(1000 + D)
        c = torch.randn((n_c, D), generator=gen, device=dev)
        c_bias = torch.randn((n_c,), generator=gen, device=dev)
        for n_p in (int(n) for n in args.pairs.split(',')):
            n_q = n_p                                                      # one query row per pair, as the lists need
            q = torch.randn((n_q, D), generator=gen, device=dev)
            q_bias = torch.randn((n_q,), generator=gen, device=dev)
            qi = torch.arange(n_p, dtype=torch.int64, device=dev)
            ti = torch.randint(0, n_c, (n_p,), generator=gen, device=dev)
            ranks = torch.empty((n_p,), dtype=torch.int64, device=dev)
            sc = torch.empty((n_p,), dtype=torch.float32, device=dev)
            ids = torch.empty((n_q, K), dtype=torch.int64, device=dev)
            lsc = torch.empty((n_q, K), dtype=torch.float32, device=dev)
            nb = lib.r4r_topk_dot_ws_bytes(n_q, n_c, K, args.chunk)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)

            def fused():
                _lib.call('r4r_rank_dot', ptr(q), n_q, ptr(q_bias), ptr(c), n_c, D, ptr(c_bias), D, ptr(qi), ptr(ti), n_p,
                          None, None, args.chunk, ptr(ranks), ptr(sc))

            def lists():
                _lib.call('r4r_topk_dot', ptr(q), n_q, ptr(q_bias), ptr(c), n_c, D, ptr(c_bias), D, None, None, K,
                          args.chunk, ptr(ws), int(nb), ptr(ids), ptr(lsc))

            step = max(1, min(n_p, YARDSTICK_SCORE_BYTES // (4 * n_c)))
            s_t = (q[qi] * c[ti]).sum(1) + c_bias[ti] + q_bias[qi]
            yard_out = []

            def yardstick():
                yard_out.clear()
                for a in range(0, n_p, step):
                    rows_q = qi[a:a + step]
                    yard_out.append(((q[rows_q] @ c.T + c_bias + q_bias[rows_q, None]) > s_t[a:a + step, None]).sum(1))

            fused(); yardstick(); lists(); fused(); yardstick(); lists()          # warm-up: code objects, rocBLAS' choice
            torch.cuda.synchronize()
            agree = float((torch.cat(yard_out) == ranks).float().mean())
            inner = [max(1, min(200, int(args.window_us / max(timed(f, 1), 1.0)))) for f in (fused, yardstick, lists)]
            tf, ty, tl = [], [], []
            for _ in range(args.repeats):
                tf.append(timed(fused, inner[0]))
                ty.append(timed(yardstick, inner[1]))
                tl.append(timed(lists, inner[2]))
            tile = 64 if (n_p >= args.wide_from and D <= 128) else 16
            roof_b = -(-n_p // tile) * n_c * D * 4 / HBM_BYTES_PER_S * 1e6
            roof_f = 2.0 * n_p * n_c * D / MFMA_F32_FLOPS * 1e6
            row = dict(D=D, n_p=n_p, n_c=n_c, fused_us=[min(tf), max(tf)], torch_us=[min(ty), max(ty)],
                       lists_us=[min(tl), max(tl)], torch_over_fused=min(ty) / min(tf), lists_over_fused=min(tl) / min(tf),
                       bytes_roof_us=roof_b, flops_roof_us=roof_f, share_of_bytes_roof=roof_b / min(tf),
                       share_of_flops_roof=roof_f / min(tf), fused_range_above_torch=min(tf) > max(ty),
                       fused_range_above_lists=min(tf) > max(tl), ranks_equal_to_torch=agree, calls_per_window=inner)
            rows.append(row)
            flag = ''.join(w for w, on in (('   FUSED RANGE ABOVE TORCH', row['fused_range_above_torch']),
                                           ('   FUSED RANGE ABOVE THE LISTS', row['fused_range_above_lists'])) if on)
            say('  %5d %7d | %10.1f .. %10.1f | %11.1f .. %11.1f | %10.1f .. %10.1f | %7.2fx %7.2fx | %8.1f%% %8.1f%%%s' % (
                D, n_p, min(tf), max(tf), min(ty), max(ty), min(tl), max(tl), row['torch_over_fused'],
                row['lists_over_fused'], 100 * row['share_of_bytes_roof'], 100 * row['share_of_flops_roof'], flag))
        torch.cuda.empty_cache()
    say('# ranks equal to the torch count (which rounds its GEMM differently and ignores ties): ' +
        ', '.join('D=%d n_p=%d %.4f' % (r['D'], r['n_p'], r['ranks_equal_to_torch']) for r in rows))
    print(json.dumps({'bench_rank': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
