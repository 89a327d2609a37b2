#!/usr/bin/env python
"""Times NARRE's pair gradients (include/r4r.h, "NARRE pair gradients"), in the form of
tools/bench_pair_explain.py:

(a) the two kernels through ``ops`` -- r4r_narre_attn_jac over 4,096 users and 4,096 items (one call per side) and
    r4r_narre_pair_grad over n_p in {128, 8,192, 131,072} random pairs, R = 10, L in {32, 64}, F = 100, every output
    written -- against
      torch   the same closed form (owner pass and pair pass) as batched torch ops on the device, and
      autograd  torch autograd through a plain restatement of the forward over the pairs' gathered pooled features (one
                backward of the summed scores: a pair's score depends on its own rows only), which is what a backward per
                pair spends.
    Device events around `inner` back-to-back calls (~20 ms windows), every shape warmed up, sides INTERLEAVED,
    `repeats` repeats, min .. max.  Nothing the kernels could not be compared with bit for bit is claimed: torch sums
    in another order; the printed difference is a sanity figure, tests/test_gpu_narre_pair.py holds the kernels to float64.
(b) ``explain_pair_reviews`` end to end for every training user's top-10 list (as ``recommended_pairs`` gives it) with
    towers='device' on synthetic pools at cfg4's cardinalities: wall clock with a device synchronise inside every window,
    min .. max, and the share of ``pair_reviews`` alone.

No ratio is a gate: every row is printed, whichever side it favours.

    python tools/bench_narre_pair.py [--parts a,b] [--k 5] [--top 10] [--scale 1.0] [--tower-batch 256] [--repeats 5] [--out FILE]
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

LS, R, F = (32, 64), 10, 100
PAIRS = (128, 8192, 131072)
OWNERS = 4096
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


def torch_owner(s):
    """The owner pass of include/r4r.h as batched torch ops -> dict(p, attn, E, dz)."""
    L = s['z'].shape[2]
    pre = torch.cat([s['z'], s['other_table'][s['nb']]], -1) @ s['W0'].T + s['b0']
    a = torch.softmax(torch.relu(pre) @ s['w3'] + s['b3'], dim=1)
    p = (a[..., None] * s['z']).sum(1) + s['own_table'][s['owner']]
    D = ((pre > 0) * s['w3']) @ s['W0'][:, :L]
    return dict(p=p, attn=a, E=D @ s['fc'], dz=(D * s['z']).sum(-1))


def torch_pair(su, ou, si, oi, u, i, h):
    """The pair pass as batched torch ops -> (score, w_user, w_item, rev_user, rev_item)."""
    pu, pi = ou['p'][u], oi['p'][i]
    t = torch.addmm(h['b1'], pu * pi, h['W1'].T)
    score = torch.relu(t) @ h['w'] + h['qb'][u] + h['cb'][i]
    gx = ((t > 0) * h['w']) @ h['W1']
    out = [score]
    revs = []
    for g, s, o, ix in ((gx * pi, su, ou, u), (gx * pu, si, oi, i)):
        z, a = s['z'][ix], o['attn'][ix]
        ga = torch.einsum('nl,nrl->nr', g, z)
        dl = a * (ga - (a * ga).sum(1, keepdim=True))
        out.append(a[..., None] * (g @ s['fc'])[:, None, :] + dl[..., None] * o['E'][ix])
        revs.append(a * ga + dl * o['dz'][ix])
    return tuple(out + revs)


def autograd_pairs(su, si, u, i, h, pooled_u, pooled_i, bias_u, bias_i):
    """torch autograd through a plain restatement of NARRE.py's eval forward over the pairs' gathered pooled features."""
    leaves, ps = [], []
    for s, pooled, bias, ix in ((su, pooled_u, bias_u, u), (si, pooled_i, bias_i, i)):
        leaf = pooled[ix].detach().requires_grad_()
        z = leaf @ s['fc'].T + bias
        pre = torch.cat([z, s['other_table'][s['nb'][ix]]], -1) @ s['W0'].T + s['b0']
        a = torch.softmax(torch.relu(pre) @ s['w3'] + s['b3'], dim=1)
        ps.append((a[..., None] * z).sum(1) + s['own_table'][s['owner'][ix]])
        leaves.append(leaf)
    score = torch.relu(torch.addmm(h['b1'], ps[0] * ps[1], h['W1'].T)) @ h['w'] + h['qb'][u] + h['cb'][i]
    w_user, w_item = torch.autograd.grad(score.sum(), leaves)
    return score.detach(), w_user, w_item


def kernels_alone(args, say, rows):
    from reviews4rec_amd import ops
    dev = 'cuda'
    say('# (a) r4r_narre_attn_jac (both sides, %d owners each) + r4r_narre_pair_grad against the closed form as batched torch ops '
        'and against torch autograd; R = %d, F = %d, every output, %d interleaved repeats, microseconds per call (min .. max)'
        % (OWNERS, R, F, args.repeats))
    say('# %3s %9s | %19s | %21s | %23s | %23s | %s' % ('L', 'pairs', 'attn_jac x2 us', 'pair_grad us', 'torch closed form us',
                                                          'torch autograd us', 'max |w_user - torch|'))
    for L in LS:
        gen = torch.Generator(device=dev).manual_seed(9100 + L)
        r = lambda *s: torch.randn(s, generator=gen, device=dev)
        sides, pooled, biases = [], [], []
        for _ in range(2):
            fc, bias, pl = r(L, F) * 0.1, r(L) * 0.1, r(OWNERS, R, F).abs()
            s = dict(W0=r(L, 2 * L) * 0.2, b0=r(L) * 0.1, w3=r(L) * 0.4, b3=r(1), fc=fc, other_table=r(OWNERS + 2, L),
                     own_table=r(OWNERS + 2, L), nb=torch.randint(0, OWNERS + 2, (OWNERS, R), generator=gen, device=dev),
                     owner=torch.arange(OWNERS, device=dev), z=(pl @ fc.T + bias).contiguous())
            sides.append(s)
            pooled.append(pl)
            biases.append(bias)
        su, si = sides
        h = dict(W1=r(L, L) * 0.2, b1=r(L) * 0.1, w=r(L) * 0.4, qb=r(OWNERS), cb=r(OWNERS))
        keep = {}

        def jac():
            keep['jac'] = [ops.narre_attn_jac(s['z'], s['nb'], s['other_table'], s['W0'], s['b0'], s['w3'], s['b3'], fc=s['fc'],
                                              own_table=s['own_table'], owner=s['owner'], want=('attn', 'out', 'E', 'dz'))
                           for s in sides]

        def owner_torch():
            keep['owner_torch'] = [torch_owner(s) for s in sides]

        jac()
        owner_torch()
        nat = [dict(p=o['out'], z=s['z'], attn=o['attn'], E=o['E'], dz=o['dz'], fc=s['fc']) for o, s in zip(keep['jac'], sides)]
        for n_p in PAIRS:
            n_p = max(1, int(n_p * args.scale))
            u = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)
            i = torch.randint(0, OWNERS, (n_p,), generator=gen, device=dev)

            def pair():
                keep['pair'] = ops.narre_pair_grad(nat[0], nat[1], u, i, h['W1'], h['b1'], h['w'], q_bias=h['qb'], c_bias=h['cb'])

            def closed():
                owner_torch()
                keep['closed'] = torch_pair(su, keep['owner_torch'][0], si, keep['owner_torch'][1], u, i, h)

            def auto():
                keep['auto'] = autograd_pairs(su, si, u, i, h, pooled[0], pooled[1], biases[0], biases[1])

            calls = (('jac', jac), ('pair', pair), ('closed', closed), ('auto', auto))
            for _ in range(2):
                for _, fn in calls:
                    fn()
            torch.cuda.synchronize()
            diff = (keep['pair']['w_user'] - keep['closed'][1]).abs().amax((1, 2))
            near = diff[diff <= 1e-3]
            apart, apart_pairs = float(near.max()) if near.numel() else 0.0, int((diff > 1e-3).sum())
            diff_auto = float((keep['closed'][1] - keep['auto'][1]).abs().max())
            inner = {name: max(1, min(200, int(20000 / max(timed(fn, 3), 1.0)))) for name, fn in calls}
            times = {name: [] for name, _ in calls}
            for _ in range(args.repeats):
                for name, fn in calls:
                    times[name].append(timed(fn, inner[name]))
            native = min(times['jac']) + min(times['pair'])
            row = dict(part='a', L=L, R=R, F=F, owners=OWNERS, pairs=n_p, **{name + '_us': [min(t), max(t)] for name, t in times.items()},
                       closed_over_native=min(times['closed']) / native, autograd_over_native=min(times['auto']) / native,
                       max_abs_w_user_apart=apart, pairs_on_another_relu_branch=apart_pairs,
                       max_abs_closed_minus_autograd=diff_auto, calls_per_window=inner)
            rows.append(row)
            say('  %3d %9d | %8.1f .. %8.1f | %9.1f .. %9.1f | %10.1f .. %10.1f | %10.1f .. %10.1f | %.2e, %d pairs on another ReLU '
                'branch; closed form / native %.2fx, autograd / native %.2fx' % (
                    L, n_p, min(times['jac']), max(times['jac']), min(times['pair']), max(times['pair']), min(times['closed']),
                    max(times['closed']), min(times['auto']), max(times['auto']), apart, apart_pairs,
                    row['closed_over_native'], row['autograd_over_native']))
            for name in ('pair', 'closed', 'auto'):
                keep.pop(name, None)
            del u, i
            torch.cuda.empty_cache()


def whole_pass(args, say, rows):
    import reviews4rec_amd
    from reviews4rec_amd import NarreCatalogue, synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.recommend import recommended_pairs
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    say('# (b) explain_pair_reviews of every training user\'s top-%d, towers=device; tower_batch %d, k = %d, %d repeats, '
        'wall-clock milliseconds per pass (min .. max)' % (args.top, args.tower_batch, args.k, args.repeats))
    cfg = synthetic.hyper_params_for(CONFIG)
    n_users, n_items, n_ratings = (max(1, int(cfg[k] * args.scale)) for k in ('total_users', 'total_items', 'n_train'))
    E, V = int(cfg['word_embed_size']), int(cfg['vocab'])
    d = synthesize(n_ratings, n_users, n_items, V)
    hp = dict(cfg, total_users=n_users, total_items=n_items, total_words=V, engine='native')
    hp['word_vectors'] = synthetic.word_table(V, E)
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
    cat.explain_pair_reviews(users[:64], items[:64], k=args.k)       # warm-up: workspaces, code objects, the pools
    cat.pair_reviews(users, items)
    whole, weights = [], []
    for _ in range(args.repeats):
        ms, _ = wall(lambda: cat.pair_reviews(users, items))
        weights.append(ms)
        ms, e = wall(lambda: cat.explain_pair_reviews(users, items, k=args.k))
        whole.append(ms)
    row = dict(part='b', model_type='NARRE', users=int(len(set(users.tolist()))), items=int(len(cat.eligible)),
               pairs=int(len(users)), k=args.k, tower_batch=args.tower_batch, pair_batch=int(cat.pair_batch),
               explain_pair_reviews_ms=[min(whole), max(whole)], pair_reviews_ms=[min(weights), max(weights)])
    rows.append(row)
    say('# %-9s %7s %7s %9s | %25s | %23s' % ('model', 'users', 'items', 'pairs', 'explain_pair_reviews ms', 'of which pair_reviews ms'))
    say('  %-9s %7d %7d %9d | %11.1f .. %11.1f | %10.1f .. %10.1f' % (
        'NARRE', row['users'], row['items'], row['pairs'], min(whole), max(whole), min(weights), max(weights)))
    assert tuple(e.user.positions.shape) == (len(users), int(hp['narre_num_reviews']), args.k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='a,b')
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--scale', type=float, default=1.0, help="of the pair counts / the configuration's users, items, ratings")
    ap.add_argument('--max-pairs', type=int, default=0, help='(b): at most this many of the recommended pairs; 0 = all')
    ap.add_argument('--tower-batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_narre_pair: no GPU; nothing is measured without one')
    if args.repeats < 5:
        raise SystemExit('bench_narre_pair: at least five repeats per side')
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# NARRE pair gradients; %s' % torch.cuda.get_device_name(0))
    if 'a' in args.parts.split(','):
        kernels_alone(args, say, rows)
    if 'b' in args.parts.split(','):
        whole_pass(args, say, rows)
    print(json.dumps({'bench_narre_pair': rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
