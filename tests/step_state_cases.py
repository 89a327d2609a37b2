"""The cases of the step-state tests: per native engine the smallest shapes that reach each path of the duplicate-row
summation (hits spread over lanes, chunk boundaries, pairs of entry waves, the 2,048-rating scan, the 4,096 / 16,384
entry caps).  tests/test_step_state_checker.py runs the float32 oracle through the checker on these inputs (CPU),
tests/test_gpu_step_state.py the engines.  Two steps per case, a different batch each; dropout 0 unless stated.

Every text case has twins with dropout on (`-p0.5` / `-p0.3`): the named case's shapes, seeds and batches, so each head
instantiation the dropout-0 cases reach is reached with masks too.  Their masks are the ones the device will draw
(stream_multipliers), so the CPU checker sees the GPU test's inputs."""
import numpy as np
import torch

import oracle
import philox_ref
from helpers import WEIGHTS_CLOSE, synthetic_review_batch, weights_outliers

LR, WD = 0.002, 1e-6
ENGINE_SEED = (0x5EED5EED * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF    # the engines' default seed, rank 0; position 0


class Case:
    def __init__(self, id, engine, hp, make_batches, vocab=None, seed=0, weights=None, draws=0, sites=None, table=None,
                 stream=False):
        self.id, self.engine, self.hp, self.vocab, self.seed = id, engine, hp, vocab, seed
        self.weights = weights                  # the engine tests' own weight criterion at this shape
        self.draws, self.sites = draws, sites   # dropout: multipliers per rating, and how they map to the oracle's sites
        self.stream = stream                    # the CPU stand-in masks are the device's Philox stream
        self.table = table                      # (an ID table or bias vector, the slots of `data` that name its rows)
        self._make, self._batches = make_batches, None

    def params(self):
        return oracle.init_params(self.hp, vocab_size=self.vocab, seed=self.seed)

    def batches(self):
        if self._batches is None:
            self._batches = self._make()
        return self._batches

    def __repr__(self):
        return self.id


def _ratings(B, gen):
    return torch.randint(1, 6, (B,), generator=gen).float()


def id_batches(B, U, I, seed, hot_user, last_rows=False):
    """Item 7 on ~14 % of the ratings, `hot_user` on ~5 %; an id whose ratings are the first and the last of the batch
    (and one on the second and the last but one); rows named exactly once and exactly twice; with last_rows the last
    row of each table (index U / I: the tables hold U + 1 / I + 1 rows).  The top 16 ids below U / I are kept out of
    the random draw: U-3 / I-3 are named once, U-4 / I-4 twice, U-5 .. U-16 never."""
    def make():
        gen = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(2):
            uid = torch.randint(0, U - 16, (B,), generator=gen)
            iid = torch.randint(0, I - 16, (B,), generator=gen)
            iid[torch.rand(B, generator=gen) < 0.14] = 7
            uid[torch.rand(B, generator=gen) < 0.05] = hot_user
            uid[0] = uid[B - 1] = U - 2
            iid[1] = iid[B - 2] = I - 2
            uid[B // 2], iid[B // 3] = U - 3, I - 3
            uid[5] = uid[B // 2 + 7] = U - 4
            iid[6] = iid[B // 2 + 9] = I - 4
            if last_rows:
                uid[2], iid[B - 3] = U, I
            out.append(([None] * 5 + [uid, iid], _ratings(B, gen)))
        return out
    return make


def mf_cases():
    U, I = 12000, 3000
    out = []
    for D, B, p in [(4, 1000, 0.0), (10, 2100, 0.0), (64, 1000, 0.0), (64, 2100, 0.0), (100, 1000, 0.0), (256, 2100, 0.0),
                    (64, 16384, 0.0), (10, 1000, 0.5)]:
        hp = dict(model_type='MF_dot', latent_size=D, dropout=p, total_users=U, total_items=I, lr=LR, weight_decay=WD,
                  batch_size=B)
        out.append(Case('mf_dot-D%d-B%d%s' % (D, B, '-dropout' if p else ''), 'MFEngine', hp,
                        id_batches(B, U, I, 1000 + D + B, 123), seed=11, weights=WEIGHTS_CLOSE, draws=2 * D if p else 0,
                        sites=(lambda mult, D=D: {'dropout.user': mult[:, :D], 'dropout.item': mult[:, D:]}),
                        table=('item_embedding.weight', (6,))))
    hp = dict(model_type='bias_only', latent_size=8, dropout=0.0, total_users=U, total_items=I, lr=LR, weight_decay=WD,
              batch_size=2100)
    out.append(Case('bias_only-B2100', 'MFEngine', hp, id_batches(2100, U, I, 77, 123), seed=13, weights=WEIGHTS_CLOSE,
                    table=('item_bias', (6,))))
    return out


def idnet_cases():
    U, I = 4000, 900
    out = []
    for kind, L, B in [('MF', 32, 2100), ('GMF', 5, 2100), ('NeuMF', 48, 900), ('MLP', 64, 500), ('MF', 16, 16384)]:
        hp = dict(model_type='MF' if kind == 'MF' else 'NeuMF', latent_size=L, dropout=0.0, total_users=U, total_items=I,
                  lr=LR, weight_decay=WD, word_embed_size=16, input_length=10, batch_size=B)
        if kind != 'MF':
            hp['neumf_stage'] = kind
        pre = 'gmf_' if kind == 'NeuMF' else ''
        out.append(Case('idnet-%s-L%d-B%d' % (kind, L, B), 'IdNetEngine', hp, id_batches(B, U, I, B + L, 11, last_rows=True),
                        seed=3, weights=weights_outliers(5e-3, 2.1 * LR),
                        table=(pre + 'item_embedding.weight', (6,))))
    return out


# ------------------------------------------------------------------------------------ the text families' dropout
def text_layout(hp):
    """The dropout draws of one rating of a native text step, in stream order (ND of include/r4r.h, site-major):
    [(oracle site, draws per rating, shape of the site's tensor for B ratings)].  A site of None is drawn and unused:
    plain `transnet` draws the ten ID-vector multipliers of `transnet++` and has no ID vectors."""
    mt, L, R = hp['model_type'], int(hp['latent_size']), int(hp.get('narre_num_reviews') or 0)
    row = lambda B: (B, L)                                                                         # noqa: E731
    if mt in ('deepconn', 'deepconn++'):
        out = [('user_conv.dropout', L, row), ('item_conv.dropout', L, row)]
        return out + ([('final.2', L, row)] if mt == 'deepconn++' else [])                          # 2L, 3L
    if mt == 'NARRE':
        return [('user_conv.dropout', R * L, lambda B: (B * R, L)), ('item_conv.dropout', R * L, lambda B: (B * R, L)),
                ('attention_scorer_user.2', R * L, lambda B: (B, R, L)),
                ('attention_scorer_item.2', R * L, lambda B: (B, R, L)),
                ('dropout.user', L, row), ('dropout.item', L, row), ('final.0', L, row)]            # 4RL + 3L
    assert mt in ('transnet', 'transnet++'), mt
    ids = mt == 'transnet++'
    return [('source.user_conv.dropout', L, row), ('source.item_conv.dropout', L, row), ('target.conv.dropout', L, row),
            ('source.dropout', L, row), ('target.dropout', L, row),
            ('dropout.user' if ids else None, 5, lambda B: (B, 5)),
            ('dropout.item' if ids else None, 5, lambda B: (B, 5))]                                 # 5L + 10


def text_draws(hp):
    return sum(n for _, n, _ in text_layout(hp))


def text_sites(hp):
    """[B, ND] multipliers -> {oracle site: its multipliers}."""
    def sites(mult):
        out, at = {}, 0
        for site, n, shape in text_layout(hp):
            if site is not None:
                out[site] = mult[:, at:at + n].reshape(shape(mult.shape[0]))
            at += n
        assert at == mult.shape[1], (at, tuple(mult.shape))
        return out
    return sites


def with_dropout(cases, twins):
    """`cases` followed by their dropout-on twins: twins = [(id of a case in `cases`, p)]."""
    by_id = {c.id: c for c in cases}
    out = list(cases)
    for id, p in twins:
        c = by_id[id]
        hp = dict(c.hp, dropout=p)
        twin = Case('%s-p%s' % (id, p), c.engine, hp, c._make, vocab=c.vocab, seed=c.seed, weights=c.weights,
                    draws=text_draws(hp), sites=text_sites(hp), table=c.table, stream=True)
        twin.batches = c.batches                             # the same batches, made once
        out.append(twin)
    return out


def pooled(docs, pool, gen):
    """Every document of `docs` ([..., T]) replaced by one of its first `pool` documents.  The large-batch text cases
    are about the ID rows; with thousands of distinct documents some max-pool always sits within rounding of a tie, where
    float32 and float64 legitimately pick different positions and differ by a whole document's gradient."""
    flat = docs.reshape(-1, docs.shape[-1])
    return flat[torch.randint(0, pool, (flat.shape[0],), generator=gen)].reshape(docs.shape)


def narre_batches(B, R, W, V, U, I, seed, few_users):
    """~45 % of the neighbour entries of the user table on user 7, ~30 % of the item table's on item 3; with few_users a
    dozen users rate everything (their own rows repeat).  Neighbour ids stay below U - 2 / I - 2: the last four rows of
    each table (U + 2 / I + 2 rows) are named by nobody."""
    def make():
        out = []
        for step in range(2):
            data, y = synthetic_review_batch(B, W, V, U - 2, I - 2, seed=seed + step, R=R, W=W)
            gen = torch.Generator().manual_seed(seed + 10 + step)
            who = torch.randint(0, U - 2, (B, R), generator=gen)
            what = torch.randint(0, I - 2, (B, R), generator=gen)
            who[torch.rand((B, R), generator=gen) < 0.45] = 7
            what[torch.rand((B, R), generator=gen) < 0.30] = 3
            data[1], data[2] = who, what
            if B > 12:
                data[3], data[4] = pooled(data[3], 8, gen), pooled(data[4], 8, gen)
            if few_users:
                data[5] = torch.randint(0, 12, (B,), generator=gen)
            out.append((data, y))
        return out
    return make


def narre_cases():
    out = []
    #        id                      B    R   L   W   E   V    U     I    few    max weight diff
    for id, B, R, L, W, E, V, U, I, few, wmax in [
            ('fused-B96', 96, 10, 10, 12, 32, 300, 60, 50, True, 5e-4),            # pairs of entry waves, hundreds of hits a row
            ('L24-R20', 6, 20, 24, 14, 32, 300, 50, 40, False, 5e-4),              # the <= 32 instantiation
            ('L33-R33', 12, 33, 33, 12, 16, 300, 60, 50, False, 2.5e-3),           # split form -> rows_apply_large
            ('L48-R10', 12, 10, 48, 12, 16, 300, 60, 50, False, 2.5e-3),
            ('B372', 372, 10, 8, 12, 16, 200, 600, 500, False, 2.5e-3),             # 4,092 entries: the last fused size
            ('B373', 373, 10, 8, 12, 16, 200, 600, 500, False, 2.5e-3),             # 4,103: the first split one
            ('B512', 512, 10, 8, 4, 16, 200, 600, 500, False, 2.5e-3),             # 5,632 entries -> the rows-apply launch
            ('B2048', 2048, 10, 8, 4, 16, 200, 600, 500, False, 2.5e-3)]:          # 22,528 entries -> rows_apply_large
        hp = dict(model_type='NARRE', latent_size=L, word_embed_size=E, input_length=W, dropout=0.0, total_users=U,
                  total_items=I, lr=LR, weight_decay=WD, narre_num_reviews=R, narre_num_words=W, batch_size=B)
        out.append(Case('narre-' + id, 'NarreEngine', hp, narre_batches(B, R, W, V, U, I, 40 + B + L, few), vocab=V, seed=12,
                        weights=weights_outliers(2e-3, wmax),
                        table=('user_embedding.weight', (1, 5))))
    return with_dropout(out, [('narre-fused-B96', 0.5), ('narre-L24-R20', 0.5), ('narre-L33-R33', 0.3),
                              ('narre-L48-R10', 0.5), ('narre-B373', 0.3)])


def doc_batches(B, T, V, U, I, seed, users=None, items=None):
    def make():
        out = []
        for step in range(2):
            data, y = synthetic_review_batch(B, T, V, U, I, seed=seed + step)
            gen = torch.Generator().manual_seed(seed + 10 + step)
            if B > 12:
                data[0], data[3], data[4] = (pooled(data[k], 8, gen) for k in (0, 3, 4))
            if users:
                data[5] = torch.randint(0, users, (B,), generator=gen)
            if items:
                data[6] = torch.randint(0, items, (B,), generator=gen)
            out.append((data, y))
        return out
    return make


def _doc_hp(mt, L, B, T, E, U, I):
    return dict(model_type=mt, latent_size=L, word_embed_size=E, input_length=T, dropout=0.0, total_users=U, total_items=I,
                lr=LR, weight_decay=WD, batch_size=B)


def deepconnpp_cases():
    T, E, V, U, I = 40, 32, 300, 40, 30
    out = []
    for L, B, users, items in [(16, 12, None, None), (17, 12, None, None), (32, 12, None, None), (33, 12, None, None),
                               (64, 12, None, None), (16, 300, 12, 8)]:
        out.append(Case('deepconnpp-L%d-B%d' % (L, B), 'DeepCoNNPPEngine', _doc_hp('deepconn++', L, B, T, E, U, I),
                        doc_batches(B, T, V, U, I, 140 + L + B, users, items), vocab=V, seed=83,
                        weights=weights_outliers(2e-3, 5e-4 if L <= 32 else 2.5e-3),
                        table=('user_bias', (5,))))
    return with_dropout(out, [('deepconnpp-L16-B12', 0.5), ('deepconnpp-L17-B12', 0.3), ('deepconnpp-L32-B12', 0.3),
                              ('deepconnpp-L33-B12', 0.5), ('deepconnpp-L64-B12', 0.3), ('deepconnpp-L16-B300', 0.3)])


def transnet_cases():
    T, E, V, U, I = 40, 32, 300, 40, 30
    out = []
    for mt, L, B, users in [('transnet', 24, 12, None), ('transnet', 48, 12, None), ('transnet', 64, 12, None),
                            ('transnet++', 24, 12, None), ('transnet++', 48, 12, None), ('transnet++', 64, 12, None),
                            ('transnet++', 24, 300, 12)]:
        out.append(Case('%s-L%d-B%d' % (mt, L, B), 'TransNetEngine', _doc_hp(mt, L, B, T, E, U, I),
                        doc_batches(B, T, V, U, I, 160 + L + B, users), vocab=V, seed=4,
                        weights=weights_outliers(2e-3, 5e-4 if L <= 32 else 2.5e-3),
                        table=('user_embedding.weight', (5,)) if mt == 'transnet++' else None))
    return with_dropout(out, [('transnet-L24-B12', 0.3), ('transnet-L48-B12', 0.5), ('transnet-L64-B12', 0.3),
                              ('transnet++-L24-B12', 0.5), ('transnet++-L48-B12', 0.3), ('transnet++-L64-B12', 0.5),
                              ('transnet++-L24-B300', 0.3)])


def deepconn_cases():
    B, T, E, V, U, I = 12, 60, 32, 300, 40, 30
    out = [Case('deepconn-L%d' % L, 'DeepCoNNEngine', _doc_hp('deepconn', L, B, T, E, U, I),
                doc_batches(B, T, V, U, I, 90 + L), vocab=V, seed=61,
                weights=weights_outliers(2e-3, 5e-4 if L <= 32 else 2.5e-3)) for L in (16, 17, 64, 65, 128)]
    return with_dropout(out, [('deepconn-L16', 0.3), ('deepconn-L17', 0.5), ('deepconn-L64', 0.3), ('deepconn-L65', 0.5),
                              ('deepconn-L128', 0.3)])


def deepconn_batch_cases():
    """r4r_deepconn_step along its batch axis: the split count (min(16, ceil(B / 16)) splits of ceil(B / nsplit)
    documents), the tail (four launches while B <= 256, per_split <= 16, nsplit E / 4 <= 1,024 and L <= 64; else five),
    the rounds of a split in the five-launch tail, and head_grad_block's passes of 128 ratings."""
    V, U, I = 300, 40, 30
    out = []
    #        B    T    E   L
    for B, T, E, L in [
            (1, 40, 32, 16),         # one document; 15 of head_grad_block's 16 row groups have no rating
            (16, 40, 32, 16),        # one full split
            (17, 40, 32, 16),        # two splits of 9 and 8
            (128, 40, 32, 16),       # eight splits of 16, head_grad_block's one full pass
            (129, 40, 32, 16),       # nine splits of 15 + 9, a second pass with one live row
            (241, 40, 32, 16),       # sixteen splits, the last holds one document
            (255, 40, 32, 16),       # ragged last split
            (256, 40, 32, 16),       # every LDS row array of wgrad_row_block full: the last folded batch size
            (257, 40, 32, 16),       # per_split 17: first batch of the five-launch tail by B; rounds of 16 + 1; last split 2
            (256, 40, 256, 16),      # nsplit E / 4 = 1,024 threads and 256 documents at once: both limits of the fold
            (256, 40, 260, 16),      # 1,040 threads: five-launch tail at per_split = 16
            (256, 40, 32, 64),       # widest folded head
            (256, 40, 32, 65),       # the 65 .. 128 head instantiation keeps the old tail
            (256, 200, 32, 16),      # documents of two 128-position gather segments under the fold
            (1000, 40, 32, 16)]:     # per_split 63: rounds 16, 16, 16, 15; last split 55
        id = 'deepconn-B%d' % B + ''.join('-%s%d' % (k, v) for k, v, d in (('T', T, 40), ('E', E, 32), ('L', L, 16)) if v != d)
        out.append(Case(id, 'DeepCoNNEngine', _doc_hp('deepconn', L, B, T, E, U, I),
                        doc_batches(B, T, V, U, I, 500 + B + E), vocab=V, seed=61,
                        weights=weights_outliers(2e-3, 5e-4 if L <= 32 else 2.5e-3)))
    return with_dropout(out, [('deepconn-B17', 0.5), ('deepconn-B256', 0.5), ('deepconn-B257', 0.3),
                              ('deepconn-B256-E256', 0.3),
                              ('deepconn-B1000', 0.3)])              # (its second step starts at stream position 32,000)


def all_cases():
    return (mf_cases() + idnet_cases() + narre_cases() + deepconnpp_cases() + transnet_cases() + deepconn_cases()
            + deepconn_batch_cases())


def stream_keep(case, step):
    """bool [B, ND]: the keep pattern the case's engine draws on `step` (0 or 1).  The engines of the step-state tests
    have the default seed and start at position 0; draw k of rating b of a step that starts at `at` is position
    at + b ND + k, and a step of B ratings advances the position by B ND (tests/test_gpu_dropout_stream.py pins that)."""
    sizes = [y.numel() for _, y in case.batches()]
    at, B = sum(sizes[:step]) * case.draws, sizes[step]
    keep = philox_ref.engine_keep(ENGINE_SEED, at, B * case.draws, np.float32(case.hp['dropout']))
    return torch.from_numpy(keep.reshape(B, case.draws))


def stream_multipliers(case, step):
    """Stand-in for the multipliers the device draws on `step`, where no device is: its own stream."""
    return stream_keep(case, step).float() * float(philox_ref.scale(case.hp['dropout']))


def stand_in_multipliers(case, step):
    if case.stream:
        return stream_multipliers(case, step)
    return random_multipliers(case, case.batches()[step][1].numel(), step)


def random_multipliers(case, B, step):
    """Stand-in for the multipliers a device draws, where no device is: 0 or 1 / (1 - p), as nn.Dropout multiplies."""
    p = float(case.hp['dropout'])
    gen = torch.Generator().manual_seed(900 + step)
    return (torch.rand((B, case.draws), generator=gen) >= p).float() / (1.0 - p)
