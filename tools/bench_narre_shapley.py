#!/usr/bin/env python
"""Times NARRE's Shapley values (include/r4r.h, "NARRE Shapley values"), in the form of
tools/bench_narre_counterfactual.py:

(a) r4r_narre_shapley through ``ops`` -- one launch per call -- for one-side games of R = 10 players (1,024 coalitions)
    of n_p in {128, 8,192, 131,072} random pairs over 4,096 users and 4,096 items, S = 2 R on the played side, L in
    {32, 64}, against
      baseline  what a caller can write without the kernel: ``ops.narre_whatif`` over host-built [n_p, 2^n] int64 masks
                and one ``torch.matmul`` with the [2^n, n] coefficient matrix, on the same inputs in the same process.
                The time to build the masks on the host and copy them is reported separately (wall clock), and so is
                the r4r_narre_whatif launch alone: the same number of variants through the existing kernel.
    r4r_narre_whatif takes n_p 2^n < 2^31, so at 1,024 coalitions the baseline stops fitting at 2,097,152 pairs (16 GiB of
    masks); every row here is below that.
(b) a JOINT game of 16 players (10 user reviews, 6 item reviews: 65,536 coalitions, 64 chunks per pair and the combine
    launch) at 16 and 1,024 pairs, against the same baseline.
    Device events around `inner` back-to-back calls (~20 ms windows), every shape warmed up, sides INTERLEAVED,
    `repeats` repeats, min .. max.  The largest |phi difference| between the two sides is printed.
(c) ``shapley(side='item')`` end to end for every training user's top-10 list with towers='device' on synthetic pools
    at cfg4's cardinalities, next to ``leave_one_out`` on the same pairs: wall clock with a device synchronise, min ..
    max.  The model is RANDOMLY INITIALISED.
(t) for a kernel trace: five r4r_narre_shapley launches and five r4r_narre_whatif launches of the same 8,192 x 1,024
    variants at L = 64, nothing else timed (run under the profiler's kernel trace; counters, if any, in a run of their own).

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_narre_shapley.py [--parts a,b,c] [--top 10] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_narre_whatif import CONFIG, timed, wall  # noqa: E402

LS, R = (32, 64), 10
PAIRS = (128, 8192, 131072)
JOINT_PAIRS = (16, 1024)
OWNERS = 4096


def coefficient_matrix(n, dev):
    """[2^n, n] float32: coef_t(c) of the coalition form, from float64."""
    f = math.factorial
    a = np.array([0.0] + [f(k - 1) * f(n - k) / f(n) for k in range(1, n + 1)] + [0.0])
    c = np.arange(1 << n)
    inside = ((c[:, None] >> np.arange(n)[None, :]) & 1) == 1
    k = inside.sum(1)
    return torch.from_numpy(np.where(inside, a[k][:, None], -a[k + 1][:, None]).astype(np.float32)).to(dev)


def host_masks(n_p, n_u, n_i, dev):
    """The baseline's masks, built on the host and copied: [n_p, 2^n] int64 a side (None for a side without players);
    player t of the user side is slot t, of the item side slot t - n_u; a clear bit of c removes the slot."""
    c = np.arange(1 << (n_u + n_i), dtype=np.int64)
    mu = (~c) & ((1 << n_u) - 1)
    mi = ((~c) >> n_u) & ((1 << n_i) - 1)
    put = lambda m, n: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m, (n_p, len(m))))).to(dev) if n else None
    return put(mu, n_u), put(mi, n_i)


def make_sides(ops, L, S_u, S_i, gen, dev):
    r = lambda *s: torch.randn(s, generator=gen, device=dev)
    sides = []
    for S in (S_u, S_i):
        s = dict(W0=r(L, 2 * L) * 0.2, b0=r(L) * 0.1, w3=r(L) * 0.4, b3=r(1), other_table=r(OWNERS + 2, L),
                 nb=torch.randint(0, OWNERS + 2, (OWNERS, S), generator=gen, device=dev), z=r(OWNERS, S, L),
                 z_pad=r(L) * 0.5, own=r(OWNERS, L), R=R)
        s['logit'] = ops.narre_logits(s['z'], s['nb'], s['other_table'], s['W0'], s['b0'], s['w3'], s['b3'])
        pad_id = torch.full((1, 1), OWNERS + 1, dtype=torch.int64, device=dev)
        s['logit_pad'] = float(ops.narre_logits(s['z_pad'].view(1, 1, L), pad_id, s['other_table'], s['W0'], s['b0'],
                                                s['w3'], s['b3']).reshape(()))
        sides.append(s)
    return sides


def games(args, say, rows, part):
    from reviews4rec_amd import ops
    dev = 'cuda'
    n_u, n_i = (R, 0) if part == 'a' else (R, 6)
    n = n_u + n_i
    say('# (%s) r4r_narre_shapley against r4r_narre_whatif over host-built [n_p, %d] masks + one matmul; %d owners a side, '
        'R = %d, %s, %d interleaved repeats, microseconds per call (min .. max); masks: wall-clock ms to build and copy'
        % (part, 1 << n, OWNERS, R, 'one-side game of %d players, S_u = %d' % (n_u, 2 * R) if part == 'a' else
           'joint game of %d + %d players, S_u = %d, S_i = %d' % (n_u, n_i, 2 * R, R + n_i), args.repeats))
    say('# %3s %9s | %23s | %23s | %23s | %19s | %s' % ('L', 'pairs', 'shapley us', 'whatif + matmul us', 'whatif alone us',
                                                        'masks ms', 'baseline / shapley'))
    coef = coefficient_matrix(n, dev)
    for L in LS:
        gen = torch.Generator(device=dev).manual_seed(9400 + L)
        r = lambda *s: torch.randn(s, generator=gen, device=dev)
        h = dict(W1=r(L, L) * 0.2, b1=r(L) * 0.1, w=r(L) * 0.4, qb=r(OWNERS), cb=r(OWNERS))
        su, si = make_sides(ops, L, 2 * R, R + n_i, gen, dev)
        for n_p in (PAIRS if part == 'a' else JOINT_PAIRS):
            n_p = max(1, int(n_p * args.scale))
            u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
            i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
            play_u = torch.full((n_p,), (1 << n_u) - 1, dtype=torch.int64, device=dev)
            play_i = torch.full((n_p,), (1 << n_i) - 1, dtype=torch.int64, device=dev) if n_i else None
            mask_ms = []
            for _ in range(args.repeats):
                ms, (mu, mi) = wall(lambda: host_masks(n_p, n_u, n_i, dev))
                mask_ms.append(ms)
            keep = {}

            def shapley():
                keep['shapley'] = ops.narre_shapley(su, si, u, i, h['W1'], h['b1'], h['w'], play_u=play_u, play_i=play_i, P=n,
                                                    q_bias=h['qb'], c_bias=h['cb'])

            def whatif():
                keep['scores'] = ops.narre_whatif(su, si, u, i, mu, mi, h['W1'], h['b1'], h['w'], q_bias=h['qb'], c_bias=h['cb'])

            def baseline():
                whatif()
                keep['phi'] = torch.matmul(keep['scores'], coef)

            calls = (('shapley', shapley), ('baseline', baseline), ('whatif', whatif))
            for _ in range(2):
                for _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            mine = torch.cat([keep['shapley'][0][:, :n_u], keep['shapley'][1][:, :n_i]], 1)
            apart = float((mine.double() - keep['phi'].double()).abs().max())
            inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in calls}
            times = {name: [] for name, _ in calls}
            for _ in range(args.repeats):
                for name, fn in calls:
                    times[name].append(timed(fn, inner[name]))
            row = dict(part=part, L=L, R=R, players=[n_u, n_i], coalitions=1 << n, owners=OWNERS, pairs=n_p,
                       **{name + '_us': [min(t), max(t)] for name, t in times.items()}, masks_ms=[min(mask_ms), max(mask_ms)],
                       baseline_over_shapley=min(times['baseline']) / min(times['shapley']), largest_phi_difference=apart,
                       calls_per_window=inner)
            rows.append(row)
            say('  %3d %9d | %10.1f .. %10.1f | %10.1f .. %10.1f | %10.1f .. %10.1f | %8.1f .. %8.1f | %.2fx; largest |phi '
                'difference| %.3g' % (L, n_p, min(times['shapley']), max(times['shapley']), min(times['baseline']),
                                      max(times['baseline']), min(times['whatif']), max(times['whatif']), min(mask_ms),
                                      max(mask_ms), row['baseline_over_shapley'], apart))
            del u, i, mu, mi, keep
            torch.cuda.empty_cache()


def for_a_trace(args, say):
    from reviews4rec_amd import ops
    dev, L, n_p = 'cuda', 64, 8192
    gen = torch.Generator(device=dev).manual_seed(9464)
    r = lambda *s: torch.randn(s, generator=gen, device=dev)
    h = dict(W1=r(L, L) * 0.2, b1=r(L) * 0.1, w=r(L) * 0.4, qb=r(OWNERS), cb=r(OWNERS))
    su, si = make_sides(ops, L, 2 * R, R, gen, dev)
    u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
    i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
    play_u = torch.full((n_p,), (1 << R) - 1, dtype=torch.int64, device=dev)
    mu, _ = host_masks(n_p, R, 0, dev)
    for _ in range(5):
        ops.narre_shapley(su, si, u, i, h['W1'], h['b1'], h['w'], play_u=play_u, P=R, q_bias=h['qb'], c_bias=h['cb'])
        ops.narre_whatif(su, si, u, i, mu, None, h['W1'], h['b1'], h['w'], q_bias=h['qb'], c_bias=h['cb'])
    torch.cuda.synchronize()
    say('# (t) five launches each of r4r_narre_shapley and r4r_narre_whatif: %d pairs x %d variants, L = %d' % (n_p, 1 << R, L))


def whole_pass(args, say, rows):
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.recommend import recommended_pairs
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (c) shapley(side=item) of every training user\'s top-%d next to leave_one_out on the same pairs, towers=device, a '
        'RANDOMLY INITIALISED model; tower_batch %d, %d repeats, wall-clock milliseconds per pass (min .. max)'
        % (args.top, args.tower_batch, args.repeats))
    cfg = synthetic.hyper_params_for(CONFIG)
    n_users, n_items, n_ratings = (max(1, int(cfg[k] * args.scale)) for k in ('total_users', 'total_items', 'n_train'))
    E, Vw = int(cfg['word_embed_size']), int(cfg['vocab'])
    d = synthesize(n_ratings, n_users, n_items, Vw)
    hp = dict(cfg, total_users=n_users, total_items=n_items, total_words=Vw, engine='native')
    hp['word_vectors'] = synthetic.word_table(Vw, E)
    reader = DataLoader(hp, d['train'], d['user_reviews'], d['item_reviews'], None,
                        this_index_user_item=d['this_index_user_item'], device='cuda')
    torch.manual_seed(0)
    model = reviews4rec_amd.get_model_class('NARRE')(hp)
    xavier_init(model)
    model = model.cuda().eval()
    cat = NarreCatalogue(model, hp, reader, tower_batch=args.tower_batch, towers='device')
    users, items = recommended_pairs(cat, args.top)
    if args.max_pairs and len(users) > args.max_pairs:
        users, items = users[:args.max_pairs], items[:args.max_pairs]
    cat.shapley(users[:64], items[:64], side='item')          # warm-up: workspaces, code objects, the pools
    cat.shapley(users, items, side='item')
    cat.leave_one_out(users, items)
    sh_ms, loo_ms = [], []
    for _ in range(args.repeats):
        ms, sh = wall(lambda: cat.shapley(users, items, side='item'))
        sh_ms.append(ms)
        ms, _ = wall(lambda: cat.leave_one_out(users, items))
        loo_ms.append(ms)
    live = sh.live_item.double()
    gap = (sh.phi_item.double().sum(1) - (sh.base.double() - sh.empty_item.double())).abs().max()
    row = dict(part='c', model_type='NARRE', users=int(len(set(users.tolist()))), items=int(len(cat.eligible)),
               pairs=int(len(users)), tower_batch=args.tower_batch, pair_batch=int(cat.pair_batch),
               shapley_ms=[min(sh_ms), max(sh_ms)], leave_one_out_ms=[min(loo_ms), max(loo_ms)],
               mean_players=float(live.mean()), coalitions=float((2.0 ** live).sum()),
               largest_efficiency_gap=float(gap), model='randomly initialised')
    rows.append(row)
    say('# %-9s %7s %7s %9s | %27s | %27s' % ('model', 'users', 'items', 'pairs', 'shapley(side=item) ms', 'leave_one_out ms'))
    say('  %-9s %7d %7d %9d | %12.1f .. %12.1f | %12.1f .. %12.1f' % (
        'NARRE', row['users'], row['items'], row['pairs'], min(sh_ms), max(sh_ms), min(loo_ms), max(loo_ms)))
    say('# %.2f players per pair on average, %.3g coalitions in all; largest |sum phi - (base - empty)| %.3g'
        % (row['mean_players'], row['coalitions'], row['largest_efficiency_gap']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b,c')
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the pair counts / the configuration's users, items, ratings")
    ap.add_argument('--max-pairs', type=int, default=0, help='(c): at most this many of the recommended pairs; 0 = all')
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_narre_shapley: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_narre_shapley: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# NARRE Shapley values; %s' % torch.cuda.get_device_name(0))
    parts = args.parts.split(',')
    t0 = time.perf_counter()
    if 'a' in parts:
        games(args, say, rows, 'a')
    if 'b' in parts:
        games(args, say, rows, 'b')
    if 'c' in parts:
        whole_pass(args, say, rows)
    if 't' in parts:
        for_a_trace(args, say)
    say('# %.0f s in all' % (time.perf_counter() - t0))
    print(json.dumps({'bench_narre_shapley': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
