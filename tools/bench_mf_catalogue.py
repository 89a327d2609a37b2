#!/usr/bin/env python
"""Times r4r_topk_pfm / r4r_pair_pfm / r4r_rank_pfm (csrc/topk_pfm.hip) on synthetic tables against the plain-torch
yardstick, same process, same cached rows (the method of DESIGN.md 4.14, as tools/bench_transnet_catalogue.py):

    lists  fused      one r4r_topk_pfm call (scan + merge launches), neither x nor a score ever written to memory
           yardstick  x = [relu(q[:, None, :H] + c[None, :, :H]) | q[:, None, H:] * c[None, :, H:]], y = x @ W.T + b,
                      torch.topk((s * y * y).sum(-1) + (x * (g * x + e)).sum(-1) + c_bias + q_bias[:, None], K), in query
                      chunks of at most 2 GiB of the [queries, n_c, D] and [queries, n_c, M] intermediates and at most
                      2^24 rows of them
    pairs  fused      one r4r_pair_pfm call over n_q * 1024 pairs
           yardstick  the same expression over the gathered rows q[q_idx], c[c_idx]
    ranks  fused      one r4r_rank_pfm call (target, scan and no exclusion launch), one pair per query row
           yardstick  the yardstick's score rows, then ((s > s_t) | ((s == s_t) & (id < t))).sum(-1)
           check      untimed: the same count over float64 score rows, and per pair the interval of ranks that the rounding
                      of an fp32 evaluation can move it through -- a candidate counts as surely ahead (behind) when its
                      float64 score exceeds (falls below) the target's by more than the sum of the two a-priori bounds
                      (2 D + D / 4 + M / 4 + 10) 2^-24 Mag of tests/test_gpu_mf_catalogue.py's test 4; the shares of fused
                      and torch ranks that equal the float64 rank and that lie inside the interval are reported

The shapes are an MF's at latent sizes L: H = G = L, M = 2 L (L = 8, 32, 64).  Device events around `inner` back-to-back
calls (roughly 20 ms windows), `repeats` repeats of each side INTERLEAVED, every shape warmed up first; min .. max of the
repeats are reported, with the ratio of the minima and the share of the flops roof the fused call reaches:
2 n_q n_c M_pad D_pad flops (as PADDED to the instantiation that runs: D to a multiple of 4, M to a multiple of 16 -- the
MFMAs issued) against the 157.3 TF of fp32 MFMA (a roof, not a measurement).

    python tools/bench_mf_catalogue.py [--n-c 1000000] [--latent 8,32,64] [--queries 1,128,1024] [--k 10] [--repeats 7] [--out FILE]
(profiles/mf_catalogue_ab.txt: --repeats 5 --out profiles/mf_catalogue_ab.txt)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_FLOPS = 157.3e12
YARDSTICK_BYTES = 1 << 31
YARDSTICK_ROWS = 1 << 24
PAIRS_PER_QUERY = 1024


def timed(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner * 1e3            # microseconds per call


def measure(fused, yardstick, repeats):
    """-> (fused [min, max], yardstick [min, max]) in microseconds per call; both warmed up by the caller."""
    inner_f = max(1, min(200, int(20000 / max(timed(fused, 3), 1.0))))      # ~20 ms of work per timed window
    inner_y = max(1, min(200, int(20000 / max(timed(yardstick, 1), 1.0))))
    tf, ty = [], []
    for _ in range(repeats):
        tf.append(timed(fused, inner_f))
        ty.append(timed(yardstick, inner_y))
    return [min(tf), max(tf)], [min(ty), max(ty)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-c', type=int, default=1000000)
    ap.add_argument('--latent', default='8,32,64', help='latent sizes L, comma separated: H = G = L, M = 2 L')
    ap.add_argument('--queries', default='1,128,1024')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mf_catalogue: no GPU; nothing is measured without one')
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    lib = _lib.lib()
    dev, K, n_c = 'cuda', args.k, args.n_c
    lines, rows, checks = [], [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# r4r_topk_pfm / r4r_pair_pfm / r4r_rank_pfm against plain torch over the materialised product-FM head; %s; n_c = %d, '
        'K = %d, %d interleaved repeats, microseconds per call (min .. max)'
        % (torch.cuda.get_device_name(0), n_c, K, args.repeats))
    say('# %5s %4s %2s %3s %6s | %23s | %25s | %8s | %9s' % ('call', 'H', 'G', 'M', 'n_q', 'fused us', 'yardstick us',
                                                              'speedup', 'of roof'))
    for L in (int(x) for x in args.latent.split(',')):
        H, G, M = L, L, 2 * L
        D = H + G
        D_pad, M_pad = -(-D // 4) * 4, -(-M // 16) * 16
        gen = torch.Generator(device=dev).manual_seed(3000 + L)
        c = torch.randn((n_c, D), generator=gen, device=dev)
        c_bias = torch.randn((n_c,), generator=gen, device=dev)
        W = torch.randn((M, D), generator=gen, device=dev) / D ** 0.5
        b = 0.1 * torch.randn((M,), generator=gen, device=dev)
        s = torch.cat([torch.full((L,), 0.5), torch.full((L,), -0.5)]).to(dev)
        g = torch.cat([torch.zeros(L, device=dev), -0.5 * torch.randn((L,), generator=gen, device=dev) ** 2 / D])
        e = torch.randn((D,), generator=gen, device=dev) / D ** 0.5

        def inputs(qa, ca):
            """x [n, m, D] of query rows qa against candidate rows ca (or [n, D] of gathered rows)"""
            return torch.cat([torch.relu(qa[..., :H] + ca[..., :H]), qa[..., H:] * ca[..., H:]], -1)

        def score_rows(qa, qba, ca, cba):
            """[n, m, .] scores of query rows qa against candidate rows ca, materialised"""
            x = inputs(qa[:, None, :], ca[None, :, :]).reshape(-1, D)
            y = x @ W.T + b
            return ((s * y * y).sum(-1) + (x * (g * x + e)).sum(-1)).view(qa.shape[0], ca.shape[0]) + cba + qba[:, None]

        for n_q in (int(n) for n in args.queries.split(',')):
            q = torch.randn((n_q, D), generator=gen, device=dev)
            q_bias = torch.randn((n_q,), generator=gen, device=dev)
            head = (ptr(q), n_q, ptr(q_bias), ptr(c), n_c, D, ptr(c_bias), ptr(W), ptr(b), ptr(s), ptr(g), ptr(e), H, G, M)
            step = max(1, min(n_q, YARDSTICK_BYTES // (4 * n_c * (D + M)), YARDSTICK_ROWS // n_c))

            # lists
            ids = torch.empty((n_q, K), dtype=torch.int64, device=dev)
            sc = torch.empty((n_q, K), dtype=torch.float32, device=dev)
            nb = lib.r4r_topk_pfm_ws_bytes(n_q, n_c, K, args.chunk)
            ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=dev)
            yard_out = []

            def fused_lists():
                _lib.call('r4r_topk_pfm', *head, None, None, K, args.chunk, ptr(ws), int(nb), ptr(ids), ptr(sc))

            def yard_lists():
                yard_out.clear()
                for a in range(0, n_q, step):
                    yard_out.append(torch.topk(score_rows(q[a:a + step], q_bias[a:a + step], c, c_bias), K))

            # pairs
            n_p = n_q * PAIRS_PER_QUERY
            qi = torch.randint(0, n_q, (n_p,), generator=gen, device=dev)
            ci = torch.randint(0, n_c, (n_p,), generator=gen, device=dev)
            out = torch.empty((n_p,), dtype=torch.float32, device=dev)
            yard_pairs_out = []

            def fused_pairs():
                _lib.call('r4r_pair_pfm', *head, ptr(qi), ptr(ci), n_p, ptr(out))

            def yard_pairs():
                x = inputs(q[qi], c[ci])
                y = x @ W.T + b
                yard_pairs_out[:] = [(s * y * y).sum(-1) + (x * (g * x + e)).sum(-1) + c_bias[ci] + q_bias[qi]]

            # ranks: one held-out item per query row
            ri = torch.arange(n_q, device=dev)
            ti = torch.randint(0, n_c, (n_q,), generator=gen, device=dev)
            ranks = torch.empty((n_q,), dtype=torch.int64, device=dev)
            rsc = torch.empty((n_q,), dtype=torch.float32, device=dev)
            cand = torch.arange(n_c, device=dev)
            yard_ranks_out = []

            def fused_ranks():
                _lib.call('r4r_rank_pfm', *head, ptr(ri), ptr(ti), n_q, None, None, args.chunk, ptr(ranks), ptr(rsc))

            def yard_ranks():
                yard_ranks_out.clear()
                for a in range(0, n_q, step):
                    sr = score_rows(q[a:a + step], q_bias[a:a + step], c, c_bias)
                    t = ti[a:a + step, None]
                    st = sr.gather(1, t)
                    yard_ranks_out.append(((sr > st) | ((sr == st) & (cand[None, :] < t))).sum(-1))

            def check_ranks():
                """-> shares of (fused == f64, torch == f64, fused inside, torch inside), the mean interval width and the
                largest |rank - float64 rank| of (fused, torch)"""
                W64, b64, s64, g64, e64, c64, cb64, qb64 = (t.double() for t in (W, b, s, g, e, c, c_bias, q_bias))
                mine, theirs = ranks, torch.cat(yard_ranks_out)
                hit = torch.zeros(4, dtype=torch.float64, device=dev)
                width, far = 0.0, [0, 0]
                cstep = max(1, step // 4)                                       # (float64, and two more [., D] arrays)
                for a in range(0, n_q, cstep):
                    x = inputs(q[a:a + cstep].double()[:, None, :], c64[None, :, :])
                    n = x.shape[0]
                    x = x.reshape(-1, D)
                    y = x @ W64.T + b64
                    sr = ((s64 * y * y).sum(-1) + (x * (g64 * x + e64)).sum(-1)).view(n, n_c) + cb64 + qb64[a:a + cstep, None]
                    X = x.abs()
                    Y = X @ W64.abs().T + b64.abs()
                    band = ((s64.abs() * Y * Y).sum(-1) + (g64.abs() * X * X + e64.abs() * X).sum(-1)).view(n, n_c)
                    band = band + cb64.abs() + qb64[a:a + cstep, None].abs()
                    band *= (2 * D + -(-D // 4) + -(-M // 4) + 10) * 2.0 ** -24
                    del x, y, X, Y
                    t = ti[a:a + cstep, None]
                    st, both = sr.gather(1, t), band + band.gather(1, t)
                    r64 = ((sr > st) | ((sr == st) & (cand[None, :] < t))).sum(-1)
                    lo = (sr - st > both).sum(-1)
                    hi = n_c - 1 - (st - sr > both).sum(-1)                 # (the target is neither ahead nor behind itself)
                    for k, r in enumerate((mine[a:a + cstep], theirs[a:a + cstep])):
                        hit[k] += (r == r64).sum()
                        hit[2 + k] += ((r >= lo) & (r <= hi)).sum()
                        far[k] = max(far[k], int((r - r64).abs().max()))
                    width += float((hi - lo).sum())
                return [float(v) / n_q for v in hit] + [width / n_q] + far

            for name, fused, yard in (('lists', fused_lists, yard_lists), ('pairs', fused_pairs, yard_pairs),
                                      ('ranks', fused_ranks, yard_ranks)):
                fused(); yard(); fused(); yard()                             # warm-up: code objects, rocBLAS' choice
                torch.cuda.synchronize()
                if name == 'lists':
                    agree = float((torch.cat([y.indices for y in yard_out]) == ids).float().mean())
                elif name == 'pairs':
                    agree = float(torch.isclose(yard_pairs_out[0], out, rtol=1e-4, atol=1e-4).float().mean())
                else:
                    agree = float((torch.cat(yard_ranks_out) == ranks).float().mean())
                    checks.append((H, n_q) + tuple(check_ranks()))
                tf, ty = measure(fused, yard, args.repeats)
                work = n_q * n_c if name != 'pairs' else n_p
                roof = 2.0 * work * M_pad * D_pad / MFMA_F32_FLOPS * 1e6
                row = dict(call=name, H=H, G=G, M=M, n_q=n_q, n_c=n_c, K=K, fused_us=tf, yardstick_us=ty, speedup=ty[0] / tf[0],
                           flops_roof_us=roof, share_of_flops_roof=roof / tf[0], fused_range_below_yardstick=tf[1] < ty[0],
                           agreement_with_torch=agree)
                rows.append(row)
                say('  %5s %4d %2d %3d %6d | %10.1f .. %10.1f | %11.1f .. %11.1f | %7.2fx | %8.1f%%%s' % (
                    name, H, G, M, n_q, tf[0], tf[1], ty[0], ty[1], row['speedup'], 100 * row['share_of_flops_roof'],
                    '' if row['fused_range_below_yardstick'] else '   FUSED RANGE NOT BELOW THE YARDSTICK'))
            del yard_out[:], yard_pairs_out[:], yard_ranks_out[:]
        del c
        torch.cuda.empty_cache()
    say('# agreement with torch (ids / scores within 1e-4 / ranks; torch breaks ties and rounds its sums differently): ' +
        ', '.join('%s H=%d n_q=%d %.4f' % (r['call'], r['H'], r['n_q'], r['agreement_with_torch']) for r in rows))
    say('# ranks against the same count over float64 scores: share of pairs whose rank equals it (fused, torch), the largest '
        'distance from it in places, the share whose rank lies inside the interval the fp32 rounding bound allows, and the mean '
        'width of that interval in places')
    for H, n_q, f_eq, t_eq, f_in, t_in, width, f_far, t_far in checks:
        say('#   H=%2d n_q=%5d | equal to float64: fused %.4f torch %.4f | farthest: fused %d torch %d | inside the interval: '
            'fused %.4f torch %.4f | mean width %.1f' % (H, n_q, f_eq, t_eq, f_far, t_far, f_in, t_in, width))
    print(json.dumps({'bench_mf_catalogue': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
