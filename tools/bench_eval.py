"""Validation throughput on one MI355X: `eval.evaluate` (MSE + the two count -> [SE] maps)
over a held-out split and `eval.eval_ranking` (HR@1 over [B, 6] candidate rows), batches built on the device
from the token pools, scored by the fused eval forward of the native engine -- and, beside it, by the
op-by-op HIP module path.

    python tools/bench_eval.py [--model-type deepconn|NARRE|MF_dot|...] [--test 20000] [--rank-users 2000]
                               [--spans on|off|both] [--repeats 3] [--no-module] [--cache FILE]

--spans: the native engine's passes through the scoring spans, through the per-launch loop
(hyper_params['eval_spans'] = False), or both in turn.  An Electronics-sized test split is --test 169000; --rank-users
20000 gives 20,000 ranking rows.  --cache: keep the synthesized dataset in a pickle (several runs on one machine).

Prints one JSON line per timed repeat (after one untimed warm-up pass each), then one JSON line with, per path, the
best repeat: ratings/s of evaluate(), candidates/s of eval_ranking(), the metrics they returned."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ratings', type=int, default=200000)
    ap.add_argument('--test', type=int, default=20000)
    ap.add_argument('--rank-users', type=int, default=2000)
    ap.add_argument('--users', type=int, default=40000)
    ap.add_argument('--items', type=int, default=15000)
    ap.add_argument('--vocab', type=int, default=50002)
    ap.add_argument('--embed', type=int, default=300)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--model-type', default='deepconn')
    ap.add_argument('--spans', choices=['on', 'off', 'both'], default='on')
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--no-module', action='store_true', help='skip the op-by-op module path')
    ap.add_argument('--cache', default=None, help='pickle of the synthesized dataset (written if missing)')
    args = ap.parse_args()
    import reviews4rec_amd
    from reviews4rec_amd import synthetic
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.eval import evaluate, eval_ranking
    from reviews4rec_amd.loss import MSELoss
    from reviews4rec_amd.main import make_engine
    from reviews4rec_amd.utils import xavier_init
    from synth_reviews import synthesize
    if args.cache and os.path.exists(args.cache):
        import pickle
        d = pickle.load(open(args.cache, 'rb'))
    else:
        d = synthesize(args.ratings, args.users, args.items, args.vocab, test=args.test, rank_users=args.rank_users)
        if args.cache:
            import pickle
            pickle.dump(d, open(args.cache, 'wb'), 4)
    hp = dict(model_type=args.model_type, batch_size=args.batch, input_length=1000, narre_num_reviews=10,
              narre_num_words=100, total_users=args.users, total_items=args.items, latent_size=10,
              word_embed_size=args.embed, dropout=0.6, lr=0.002, weight_decay=1e-6, vocab=args.vocab,
              total_words=args.vocab, engine='native')
    hp['word_vectors'] = synthetic.word_table(args.vocab, args.embed)
    train = DataLoader(hp, d['train'], d['user_reviews'], d['item_reviews'], d['negs'],
                       this_index_user_item=d['this_index_user_item'], device='cuda')
    test = DataLoader(hp, d['test'], d['user_reviews'], d['item_reviews'], d['negs'], test_reviews=d['test_reviews'],
                      train_loader=train, device='cuda')
    torch.manual_seed(0)
    model = reviews4rec_amd.get_model_class(args.model_type)(hp)
    xavier_init(model)
    model = model.cuda()
    engine = make_engine(hp, model)
    criterion = MSELoss(hp)
    review = args.model_type not in ('bias_only', 'MF', 'MF_dot', 'NeuMF')
    out = {'model_type': args.model_type, 'test_ratings': len(d['test']), 'ranking_rows': len(d['negs']),
           'batch': args.batch, 'embed': args.embed}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    paths = [('spans_' + k, engine, dict(hp, eval_spans=(k == 'on')))
             for k in (('on', 'off') if args.spans == 'both' else (args.spans,))]
    if not args.no_module:
        paths.append(('module', None, hp))
    for label, eng, h in paths:
        ev = lambda: evaluate(model, criterion, test, h, dict(train.user_count), dict(train.item_count), review,  # noqa: E731
                              engine=eng)
        rk = lambda: eval_ranking(model, test, h, review=review, engine=eng)   # noqa: E731
        ev(), rk()                                           # warm: workspaces, token pools, descriptors on the device
        best = None
        for r in range(max(1, args.repeats)):
            (m, umap, imap), t = timed(ev)
            hr, t2 = timed(rk)
            row = {'evaluate_ratings_per_s': round(len(d['test']) / t), 'evaluate_s': round(t, 4), 'MSE': m['MSE'],
                   'eval_ranking_candidates_per_s': round(6 * len(d['negs']) / t2), 'eval_ranking_s': round(t2, 4),
                   'HR@1': hr['HR@1']}
            print(json.dumps(dict(row, model_type=args.model_type, path=label, repeat=r)), flush=True)
            if best is None:
                best = dict(row)
            for k in ('evaluate_ratings_per_s', 'eval_ranking_candidates_per_s'):
                best[k] = max(best[k], row[k])
            for k in ('evaluate_s', 'eval_ranking_s'):
                best[k] = min(best[k], row[k])
        if label == 'spans_on':
            # where a spanned evaluate() spends its time: the scoring pass alone (device work + its enqueue), the rest
            # is the one copy and the reference-shaped host work (the two count -> [SE] maps, the rounding)
            from reviews4rec_amd.eval import EVAL_LAUNCH, _launch_size
            n = _launch_size(test, h, eng, EVAL_LAUNCH)
            _, t = timed(lambda: eng.score_split(test, test.score_descriptor(n)))
            best['score_split_s'] = round(t, 4)
        out[label] = best
    print(json.dumps(out))


if __name__ == '__main__':
    main()
