#!/usr/bin/env python
"""Times NARRE's counterfactual search (include/r4r.h, "NARRE counterfactual search"), in the form of
tools/bench_narre_whatif.py:

(a) r4r_narre_search through ``ops`` -- ONE launch for the whole search of n_p in {128, 8,192, 131,072} random pairs over
    4,096 users and 4,096 items, R = 10, S = R + budget, L in {32, 64}, budget in {1, 3, 10}, both sides' attended
    slots as candidates, a NaN target (every pair runs the whole budget, so both sides do the same work) -- against
      loop    the search a caller could write before, in the same process on the same inputs: per step the attended
              slots of both sides out of the masks and one mask column per candidate (torch ops on the device), ONE
              ``ops.narre_whatif`` over the [n_p, 2 R] masks, ``torch.argmin`` and the mask update on the device.
    Device events around `inner` back-to-back searches (~20 ms windows), every shape warmed up, sides INTERLEAVED,
    `repeats` repeats, min .. max.  The loop's last scores must be the kernel's bits; the count of pairs where they are
    not is printed (torch.argmin's tie rule is the lowest index too).
(b) ``counterfactual(k=10, side='item')`` end to end for every training user's top-10 list (``recommended_pairs``) with
    towers='device' on synthetic pools at cfg4's cardinalities, next to ``leave_one_out`` on the same pairs: wall clock
    with a device synchronise inside every window, min .. max.  The model is RANDOMLY INITIALISED: the printed share of
    crossed pairs says that the tool runs, nothing about NARRE.

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_narre_counterfactual.py [--parts a,b] [--top 10] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_narre_whatif import CONFIG, timed, wall  # noqa: E402

LS, R = (32, 64), 10
PAIRS = (128, 8192, 131072)
BUDGETS = (1, 3, 10)
OWNERS = 4096


def attended(mask, S):
    """[n] int64 masks -> [n, R] int64: the first R clear slots of 0 .. S - 1 (there are always R: S = R + budget)."""
    clear = ((mask[:, None] >> torch.arange(S, device=mask.device)) & 1) == 0
    return torch.sort((~clear).to(torch.int8), dim=1, stable=True).indices[:, :R]


def loop_search(ops, su, si, u, i, h, S, budget):
    """The host loop: per step one narre_whatif over every candidate's masks, argmin and the update, on the device."""
    n = u.numel()
    mu = torch.zeros(n, dtype=torch.int64, device=u.device)
    mi = torch.zeros_like(mu)
    one = torch.ones((), dtype=torch.int64, device=u.device)
    best = None
    for _ in range(budget):
        au, ai = attended(mu, S), attended(mi, S)
        du = torch.cat([mu[:, None] | (one << au), mu[:, None].expand(n, R)], 1).contiguous()
        di = torch.cat([mi[:, None].expand(n, R), mi[:, None] | (one << ai)], 1).contiguous()
        sc = ops.narre_whatif(su, si, u, i, du, di, h['W1'], h['b1'], h['w'], q_bias=h['qb'], c_bias=h['cb'])
        at = torch.argmin(sc, dim=1, keepdim=True)
        best = sc.gather(1, at)[:, 0]
        mu, mi = du.gather(1, at)[:, 0], di.gather(1, at)[:, 0]
    return best


def kernels_alone(args, say, rows):
    from reviews4rec_amd import ops
    dev = 'cuda'
    say('# (a) r4r_narre_search (one launch) against a loop of r4r_narre_whatif + torch.argmin + mask updates per step; %d owners '
        'a side, R = %d, S = R + budget, both sides, %d interleaved repeats, microseconds per search (min .. max)'
        % (OWNERS, R, args.repeats))
    say('# %3s %9s %6s | %23s | %23s | %s' % ('L', 'pairs', 'budget', 'search us', 'loop us', 'loop / search'))
    for L in LS:
        gen = torch.Generator(device=dev).manual_seed(9300 + L)
        r = lambda *s: torch.randn(s, generator=gen, device=dev)
        h = dict(W1=r(L, L) * 0.2, b1=r(L) * 0.1, w=r(L) * 0.4, qb=r(OWNERS), cb=r(OWNERS))
        for budget in BUDGETS:
            S = R + budget
            sides = []
            for _ in range(2):
                s = dict(W0=r(L, 2 * L) * 0.2, b0=r(L) * 0.1, w3=r(L) * 0.4, b3=r(1), other_table=r(OWNERS + 2, L),
                         nb=torch.randint(0, OWNERS + 2, (OWNERS, S), generator=gen, device=dev), z=r(OWNERS, S, L),
                         z_pad=r(L) * 0.5, own=r(OWNERS, L), R=R)
                s['logit'] = ops.narre_logits(s['z'], s['nb'], s['other_table'], s['W0'], s['b0'], s['w3'], s['b3'])
                pad_id = torch.full((1, 1), OWNERS + 1, dtype=torch.int64, device=dev)
                s['logit_pad'] = float(ops.narre_logits(s['z_pad'].view(1, 1, L), pad_id, s['other_table'], s['W0'], s['b0'],
                                                        s['w3'], s['b3']).reshape(()))
                sides.append(s)
            su, si = sides
            for n_p in PAIRS:
                n_p = max(1, int(n_p * args.scale))
                u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
                i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
                every = torch.full((n_p,), -1, dtype=torch.int64, device=dev)
                target = torch.full((n_p,), float('nan'), device=dev)
                keep = {}

                def search():
                    keep['search'] = ops.narre_search(su, si, u, i, h['W1'], h['b1'], h['w'], target, 0, budget, cand_u=every,
                                                      cand_i=every, q_bias=h['qb'], c_bias=h['cb'])

                def loop():
                    keep['loop'] = loop_search(ops, su, si, u, i, h, S, budget)

                calls = (('search', search), ('loop', loop))
                for _ in range(2):
                    for _, fn in calls:
                        fn()
                torch.cuda.synchronize()
                apart = int((keep['search'][1][:, budget].view(torch.int32) != keep['loop'].view(torch.int32)).sum())
                inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in calls}
                times = {name: [] for name, _ in calls}
                for _ in range(args.repeats):
                    for name, fn in calls:
                        times[name].append(timed(fn, inner[name]))
                row = dict(part='a', L=L, R=R, S=S, budget=budget, owners=OWNERS, pairs=n_p,
                           **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                           loop_over_search=min(times['loop']) / min(times['search']), pairs_with_other_bits=apart,
                           searches_per_window=inner)
                rows.append(row)
                say('  %3d %9d %6d | %10.1f .. %10.1f | %10.1f .. %10.1f | %.2fx; %d pairs whose last score differs in bits'
                    % (L, n_p, budget, min(times['search']), max(times['search']), min(times['loop']), max(times['loop']),
                       row['loop_over_search'], apart))
                del u, i, every, target, keep
                torch.cuda.empty_cache()


def whole_pass(args, say, rows):
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.recommend import recommended_pairs
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (b) counterfactual(k=%d, side=item) of every training user\'s top-%d next to leave_one_out on the same pairs, '
        'towers=device, a RANDOMLY INITIALISED model; tower_batch %d, %d repeats, wall-clock milliseconds per pass (min .. max)'
        % (args.top, args.top, args.tower_batch, args.repeats))
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
    cat.counterfactual(users[:64], items[:64], k=args.top, side='item')       # warm-up: workspaces, code objects, the pools
    cat.counterfactual(users, items, k=args.top, side='item')
    cat.leave_one_out(users, items)
    cf_ms, loo_ms = [], []
    for _ in range(args.repeats):
        ms, cf = wall(lambda: cat.counterfactual(users, items, k=args.top, side='item'))
        cf_ms.append(ms)
        ms, _ = wall(lambda: cat.leave_one_out(users, items))
        loo_ms.append(ms)
    row = dict(part='b', model_type='NARRE', users=int(len(set(users.tolist()))), items=int(len(cat.eligible)),
               pairs=int(len(users)), k=args.top, budget=int(cf.order.shape[1]), tower_batch=args.tower_batch,
               pair_batch=int(cat.pair_batch), counterfactual_ms=[min(cf_ms), max(cf_ms)],
               leave_one_out_ms=[min(loo_ms), max(loo_ms)], crossed_share=float(cf.crossed.double().mean()),
               mean_steps=float(cf.steps.double().mean()), model='randomly initialised')
    rows.append(row)
    say('# %-9s %7s %7s %9s | %27s | %27s' % ('model', 'users', 'items', 'pairs', 'counterfactual (budget %d) ms' % row['budget'],
                                               'leave_one_out ms'))
    say('  %-9s %7d %7d %9d | %12.1f .. %12.1f | %12.1f .. %12.1f' % (
        'NARRE', row['users'], row['items'], row['pairs'], min(cf_ms), max(cf_ms), min(loo_ms), max(loo_ms)))
    say('# %.1f %% of the pairs left the top-%d within the budget, %.2f removals per pair on average (a randomly initialised '
        'model: a statement about the tool, not about NARRE)' % (100 * row['crossed_share'], args.top, row['mean_steps']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b')
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the pair counts / the configuration's users, items, ratings")
    ap.add_argument('--max-pairs', type=int, default=0, help='(b): at most this many of the recommended pairs; 0 = all')
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_narre_counterfactual: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_narre_counterfactual: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# NARRE counterfactual search; %s' % torch.cuda.get_device_name(0))
    if 'a' in args.parts.split(','):
        kernels_alone(args, say, rows)
    if 'b' in args.parts.split(','):
        whole_pass(args, say, rows)
    print(json.dumps({'bench_narre_counterfactual': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
