#!/usr/bin/env python
"""Times NARRE's what-if scores (include/r4r.h, "NARRE what-if scores"), in the form of
tools/bench_narre_pair.py:

(a) the two kernels through ``ops`` -- r4r_narre_logits over 4,096 users and 4,096 items (one call per side, S = R + 3
    slots) and r4r_narre_whatif over n_p in {128, 8,192, 131,072} random pairs x V = 21 variants (nothing, every single
    slot, and ten masks of up to three drops, on both sides), R = 10, L in {32, 64} -- against
      torch   the same computation (logits; per variant the selected list out of the mask, its softmax, the pooled
              vectors, the head) as batched torch ops on the device, 8,192 pairs per batch.
    Device events around `inner` back-to-back calls (~20 ms windows), every shape warmed up, sides INTERLEAVED,
    `repeats` repeats, min .. max.  torch sums in another order; the printed difference is a sanity figure,
    tests/test_gpu_narre_whatif.py holds the kernels to float64.
(b) ``leave_one_out`` end to end for every training user's top-10 list (as ``recommended_pairs`` gives it) with
    towers='device' on synthetic pools at cfg4's cardinalities: wall clock with a device synchronise inside every window,
    min .. max; next to it the honest alternative for ONE variant -- the attended vectors of the distinct users and items
    computed again (``score_pairs``, which runs the user side, plus ``_attended`` of the items) -- which a removal by
    re-running the model would spend once per variant, 2 R = 20 times for a leave-one-out; and the mean AOPC of
    ``deletion_curve`` by 'rev' against by 'attention' over the same pairs.  The model is RANDOMLY INITIALISED: the two
    AOPC figures say that the tool runs and what it prints, nothing about NARRE's explanations.

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_narre_whatif.py [--parts a,b] [--top 10] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
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

LS, R, V, SPARE = (32, 64), 10, 21, 3
PAIRS = (128, 8192, 131072)
OWNERS = 4096
TORCH_BATCH = 8192
CONFIG = 'cfg4_narre_kindle'


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


def torch_logits(s, z, nb):
    return torch.relu(torch.cat([z, s['other_table'][nb]], -1) @ s['W0'].T + s['b0']) @ s['w3'] + s['b3']


def torch_pooled(s, logit, logit_pad, ix, mask):
    """One side of a batch of pairs: owners ``ix`` [c], masks [c, V] -> p' [c, V, L] as batched torch ops."""
    S = s['z'].shape[1]
    keep = ((mask[..., None] >> torch.arange(S, device=mask.device)) & 1) == 0                  # [c, V, S]
    order = torch.sort((~keep).to(torch.int8), dim=-1, stable=True).indices[..., :R]
    sel = torch.where(torch.arange(R, device=mask.device) < keep.sum(-1, keepdim=True), order, torch.full_like(order, S))
    rows = ix[:, None, None].expand(sel.shape)
    zf = torch.cat([s['z'], s['z_pad'][None, None, :].expand(s['z'].shape[0], 1, -1)], 1)
    lf = torch.cat([logit, logit_pad.expand(logit.shape[0], 1)], 1)
    a = torch.softmax(lf[rows, sel], dim=-1)
    return (a[..., None] * zf[rows, sel]).sum(2) + s['own'][ix][:, None, :]


def torch_whatif(su, si, lu, li, lpu, lpi, u, i, du, di, h):
    out = []
    for s0 in range(0, u.numel(), TORCH_BATCH):
        sl = slice(s0, s0 + TORCH_BATCH)
        x = torch_pooled(su, lu, lpu, u[sl], du[sl]) * torch_pooled(si, li, lpi, i[sl], di[sl])
        out.append(torch.relu(x @ h['W1'].T + h['b1']) @ h['w'] + h['qb'][u[sl]][:, None] + h['cb'][i[sl]][:, None])
    return torch.cat(out)


def variant_masks(n_p, gen, dev):
    """[n_p, V]: nothing, every single slot of the R, then masks of up to three drops among the first R + 3 slots."""
    single = torch.cat([torch.zeros(1, dtype=torch.int64), torch.ones(R, dtype=torch.int64) << torch.arange(R)]).to(dev)
    m = torch.zeros((n_p, V), dtype=torch.int64, device=dev)
    m[:, :R + 1] = single
    for _ in range(SPARE):
        m[:, R + 1:] |= torch.ones((), dtype=torch.int64, device=dev) << torch.randint(0, R + SPARE, (n_p, V - R - 1), generator=gen, device=dev)
    return m


def kernels_alone(args, say, rows):
    from reviews4rec_amd import ops
    dev = 'cuda'
    S = R + SPARE
    say('# (a) r4r_narre_logits (both sides, %d owners each, S = %d) + r4r_narre_whatif against the same computation as batched '
        'torch ops; R = %d, V = %d, %d interleaved repeats, microseconds per call (min .. max)' % (OWNERS, S, R, V, args.repeats))
    say('# %3s %9s | %19s | %21s | %23s | %23s | %s' % ('L', 'pairs', 'logits x2 us', 'whatif us', 'torch logits x2 us',
                                                          'torch variants us', 'max |score - torch|'))
    for L in LS:
        gen = torch.Generator(device=dev).manual_seed(9200 + L)
        r = lambda *s: torch.randn(s, generator=gen, device=dev)
        sides = []
        for _ in range(2):
            sides.append(dict(W0=r(L, 2 * L) * 0.2, b0=r(L) * 0.1, w3=r(L) * 0.4, b3=r(1), other_table=r(OWNERS + 2, L),
                              nb=torch.randint(0, OWNERS + 2, (OWNERS, S), generator=gen, device=dev), z=r(OWNERS, S, L),
                              z_pad=r(L) * 0.5, own=r(OWNERS, L), R=R))
        su, si = sides
        h = dict(W1=r(L, L) * 0.2, b1=r(L) * 0.1, w=r(L) * 0.4, qb=r(OWNERS), cb=r(OWNERS))
        keep = {}
        pad_id = torch.full((1, 1), OWNERS + 1, dtype=torch.int64, device=dev)

        def logits():
            keep['logits'] = [ops.narre_logits(s['z'], s['nb'], s['other_table'], s['W0'], s['b0'], s['w3'], s['b3']) for s in sides]

        def logits_torch():
            keep['logits_torch'] = [torch_logits(s, s['z'], s['nb']) for s in sides]

        logits()
        logits_torch()
        pads = [ops.narre_logits(s['z_pad'].view(1, 1, L), pad_id, s['other_table'], s['W0'], s['b0'], s['w3'], s['b3']) for s in sides]
        nat = [dict(s, logit=lg, logit_pad=float(lp.reshape(()))) for s, lg, lp in zip(sides, keep['logits'], pads)]
        for n_p in PAIRS:
            n_p = max(1, int(n_p * args.scale))
            u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
            i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
            du, di = variant_masks(n_p, gen, dev), variant_masks(n_p, gen, dev).flip(1).contiguous()

            def whatif():
                keep['whatif'] = ops.narre_whatif(nat[0], nat[1], u, i, du, di, h['W1'], h['b1'], h['w'], q_bias=h['qb'], c_bias=h['cb'])

            def variants_torch():
                keep['torch'] = torch_whatif(su, si, keep['logits'][0], keep['logits'][1], pads[0], pads[1], u, i, du, di, h)

            calls = (('logits', logits), ('whatif', whatif), ('logits_torch', logits_torch), ('torch', variants_torch))
            for _ in range(2):
                for _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            diff = (keep['whatif'] - keep['torch']).abs()
            near = diff[diff <= 1e-3]
            apart, apart_n = float(near.max()) if near.numel() else 0.0, int((diff > 1e-3).sum())
            inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in calls}
            times = {name: [] for name, _ in calls}
            for _ in range(args.repeats):
                for name, fn in calls:
                    times[name].append(timed(fn, inner[name]))
            row = dict(part='a', L=L, R=R, S=S, V=V, owners=OWNERS, pairs=n_p,
                       **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                       torch_variants_over_whatif=min(times['torch']) / min(times['whatif']),
                       torch_logits_over_logits=min(times['logits_torch']) / min(times['logits']),
                       max_abs_score_apart=apart, variants_on_another_relu_branch=apart_n, calls_per_window=inner)
            rows.append(row)
            say('  %3d %9d | %8.1f .. %8.1f | %9.1f .. %9.1f | %10.1f .. %10.1f | %10.1f .. %10.1f | %.2e, %d variants on another '
                'ReLU branch; torch variants / whatif %.2fx, torch logits / logits %.2fx' % (
                    L, n_p, min(times['logits']), max(times['logits']), min(times['whatif']), max(times['whatif']),
                    min(times['logits_torch']), max(times['logits_torch']), min(times['torch']), max(times['torch']), apart, apart_n,
                    row['torch_variants_over_whatif'], row['torch_logits_over_logits']))
            for name in ('whatif', 'torch'):
                keep.pop(name, None)
            del u, i, du, di
            torch.cuda.empty_cache()


def whole_pass(args, say, rows):
    import numpy as np
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.recommend import recommended_pairs
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (b) leave_one_out of every training user\'s top-%d, towers=device, a RANDOMLY INITIALISED model; tower_batch %d, %d '
        'repeats, wall-clock milliseconds per pass (min .. max)' % (args.top, args.tower_batch, args.repeats))
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
    cat.leave_one_out(users[:64], items[:64])                        # warm-up: workspaces, code objects, the pools
    cat.leave_one_out(users, items)
    distinct_items = np.unique(items)

    def one_variant_by_rerunning():
        cat.score_pairs(users, items)                                # the user side's towers and attention, then the head
        for _ in cat._attended_chunks('item', distinct_items):       # the item side's, which score_pairs reads from its cache
            pass

    one_variant_by_rerunning()
    loo_ms, rerun_ms = [], []
    for _ in range(args.repeats):
        ms, loo = wall(lambda: cat.leave_one_out(users, items))
        loo_ms.append(ms)
        ms, _ = wall(one_variant_by_rerunning)
        rerun_ms.append(ms)
    aopc = {}
    for by in ('rev', 'attention'):
        for side in ('user', 'item'):
            dc = cat.deletion_curve(users, items, by=by, side=side)
            aopc['%s_%s' % (by, side)] = float(dc.aopc.double().mean())
    variants = 2 * int(hp['narre_num_reviews'])
    row = dict(part='b', model_type='NARRE', users=int(len(set(users.tolist()))), items=int(len(cat.eligible)),
               pairs=int(len(users)), variants_per_pair=variants, tower_batch=args.tower_batch, pair_batch=int(cat.pair_batch),
               leave_one_out_ms=[min(loo_ms), max(loo_ms)], one_variant_by_rerunning_ms=[min(rerun_ms), max(rerun_ms)],
               mean_aopc=aopc, model='randomly initialised')
    rows.append(row)
    say('# %-9s %7s %7s %9s | %25s | %31s' % ('model', 'users', 'items', 'pairs', 'leave_one_out (%d variants) ms' % variants,
                                               'ONE variant by re-running, ms'))
    say('  %-9s %7d %7d %9d | %11.1f .. %11.1f | %14.1f .. %14.1f' % (
        'NARRE', row['users'], row['items'], row['pairs'], min(loo_ms), max(loo_ms), min(rerun_ms), max(rerun_ms)))
    say('# mean AOPC over those pairs, deletion_curve by rev / by attention (a randomly initialised model: a statement about '
        'the tool, not about NARRE): user side %.3e / %.3e, item side %.3e / %.3e'
        % (aopc['rev_user'], aopc['attention_user'], aopc['rev_item'], aopc['attention_item']))
    assert tuple(loo.without_user.shape) == (len(users), int(hp['narre_num_reviews']))


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
        raise SystemExit('bench_narre_whatif: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_narre_whatif: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# NARRE what-if scores; %s' % torch.cuda.get_device_name(0))
    if 'a' in args.parts.split(','):
        kernels_alone(args, say, rows)
    if 'b' in args.parts.split(','):
        whole_pass(args, say, rows)
    print(json.dumps({'bench_narre_whatif': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
