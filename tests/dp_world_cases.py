"""The cases of the data-parallel world tests: per native engine the smallest worlds, shard shapes and gathered sizes at
which the index arithmetic of the data-parallel step changes (tests/dp_mesh.py runs them; tests/test_dp_mesh_host.py
checks on the CPU that they reach what they claim; tests/test_gpu_dp_worlds.py runs the engines).

Every family: an odd world and a world of 8; on step 1 an empty shard that is neither the first nor the last, a shard of
one rating and padding in every block (a rank's n ratings are padded to B_pad with id -1), on step 2 full shards where
the case is about a size (no padding at all), another ragged cut otherwise.  The thresholds are those of engine.py and
the C entry points' R4R_REQUIRE lines:

  MF_dot / bias_only   r4r_mf_apply: world * B_pad <= 2,048 is the one-launch form (MF_SCAN_MAX_B), beyond it a registering
                       launch runs first; more than 2,048 also selects the 8-wave update; the entry point admits
                       1,048,576 gathered entries (MF_MAX_B_STEP), so 16,384 is a size, not an edge
  NARRE                world * B_pad * (1 + R) <= 16,384 and L <= 32: the block form (r4r_narre_dp_block ->
                       r4r_narre_rows_apply_blocks); otherwise the generic payload form, which -- with more than 16,384
                       entries OR L > 32 -- ends in r4r_narre_rows_apply_large.  (r4r_narre_rows_apply itself is not
                       reachable from a step of more than one rank: every size it admits takes the block form.)
  TransNet++           world * B_pad <= 2,048: r4r_transnet_dp_block -> r4r_transnet_rows_apply_blocks; beyond, the generic
                       payload form -> r4r_transnet_rows_apply
  MF / NeuMF, DeepCoNN++   one form (gather_entry_fields -> r4r_idnet_rows_apply / r4r_deepconnpp_rows_apply)

Row 0 of every ID table and bias vector is named by nobody (ids 0 are moved to 1): a padding entry that an update counts
onto row 0 shows as a row that should hold the pure weight-decay moments and does not.  Documents are short and pooled
beyond 12 ratings (step_state_cases.pooled has the reason)."""
import torch

from dp_mesh import shard_bounds
from helpers import WEIGHTS_CLOSE, weights_outliers
from step_state_cases import LR, WD, Case, _doc_hp, _ratings, doc_batches, id_batches, narre_batches

ID_SLOTS = (1, 2, 5, 6)


class WorldCase(Case):
    """A step-state Case + world, shards (per step: the ranks' shard sizes; hp['batch_size'] is the per-rank B_pad),
    the exchange to pin (DeepCoNN), defer (the blocked sweep + flush()), and what the case claims:
      entries, side, limit   the gathered entry count the engine compares, '<=' or '>', and the threshold it sits at
      collectives            {kind: calls per step} the step must make
      hot                    [(slots, id)]: ids that several ranks' shards must name
      last_rows              (U, I): ids the LAST rank's shard must name in slots 5 / 6
      rows                   the family has ID rows (the padding defect applies)"""

    def __init__(self, id, engine, hp, make_batches, world, shards, collectives, exchange=None, defer=False, entries=None,
                 side=None, limit=None, hot=(), last_rows=None, rows=True, widen=(), **kw):
        super().__init__(id, engine, hp, make_batches, **kw)
        self.world, self.shards, self.collectives = world, [list(s) for s in shards], dict(collectives)
        self.exchange, self.defer = exchange, defer
        self.entries, self.side, self.limit = entries, side, limit
        self.hot, self.last_rows, self.rows = list(hot), last_rows, rows
        self.widen = list(widen)                             # [(kind, name)]: tensors held to helpers.oracle_atol instead
        self.B_pad = int(hp['batch_size'])

    def plain(self):
        """The same case without the blocked sweep."""
        assert self.defer
        return WorldCase(self.id + '-plain', self.engine, self.hp, self._make, self.world, self.shards, self.collectives,
                         exchange=self.exchange, vocab=self.vocab, seed=self.seed, weights=self.weights)


def ragged(world, P):
    """Step 1's cut: full shards except an empty one in the middle, one of a single rating and one three short (three
    ranks: (7, 0, 4) at B_pad 7, (4, 0, 3) at B_pad 4; their shard of one rating comes on step 2)."""
    if world == 3:
        return [P, 0, P - 3 if P >= 7 else P - 1]
    sizes = [P] * world
    sizes[1], sizes[2], sizes[world - 2] = 1, 0, P - 3
    return sizes


def second(world, P, full):
    return [P] * world if full else [1, P, P - 2] + [P] * (world - 3)


def steps_of(makers, shards, plant=None):
    """Step k's batch from makers[k] (a step_state_cases batch maker for that step's global size); ids 0 moved to 1;
    plant(step, data, bounds) then writes the ids the case is about."""
    def make():
        out = []
        for step, (mk, sizes) in enumerate(zip(makers, shards)):
            data, y = mk()[step]
            assert y.numel() == sum(sizes)
            data = [None if d is None else d.clone() for d in data]
            for s in ID_SLOTS:
                if data[s] is not None:
                    data[s][data[s] == 0] = 1
            if plant is not None:
                plant(step, data, shard_bounds(sizes))
            out.append((data, y))
        return out
    return make


def tiny_id_batches(B, U, I, seed):
    """id_batches needs 19 ratings for the positions it plants; below, random ids only (the case plants its own)."""
    def make():
        gen = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(2):
            uid = torch.randint(1, U - 16, (B,), generator=gen)
            iid = torch.randint(1, I - 16, (B,), generator=gen)
            out.append(([None] * 5 + [uid, iid], _ratings(B, gen)))
        return out
    return make


def plant_ids(hot_user, hot_item, last=None):
    """The hot item on the first rating of every non-empty shard, the hot user on the last one; last = (U, I): the last
    row of each table on the last rank (its shard holds at least three ratings)."""
    def plant(step, data, bounds):
        for lo, hi in bounds:
            if hi > lo:
                if hot_item is not None:
                    data[6][lo] = hot_item
                if hot_user is not None:
                    data[5][hi - 1] = hot_user
        if last is not None:
            lo, hi = bounds[-1]
            assert hi - lo >= 3
            data[5][hi - 2], data[6][hi - 2] = last[0], last[1]
    return plant


def _id_maker(B, U, I, seed, hot_user, last_rows=False):
    return id_batches(B, U, I, seed, hot_user, last_rows=last_rows) if B >= 19 else tiny_id_batches(B, U, I, seed)


def mf_cases():
    U, I = 12000, 3000
    out = []
    #    id              model        W   D   B_pad  full 2nd  defer
    for id, mt, W, D, P, full, defer in [
            ('W3-D10-B7', 'MF_dot', 3, 10, 7, False, False),          # shards (7, 0, 4), then (1, 7, 5)
            ('W3-D10-B7-deferred', 'MF_dot', 3, 10, 7, False, True),  # ... with the blocked sweep, then flush()
            ('W5-D64-B100', 'MF_dot', 5, 64, 100, True, False),
            ('W8-D10-B256', 'MF_dot', 8, 10, 256, True, False),       # 2,048 gathered entries: the last one-launch size
            ('W8-D10-B257', 'MF_dot', 8, 10, 257, True, False),       # 2,056: the first behind the registering launch
            ('W8-D64-B2048', 'MF_dot', 8, 64, 2048, True, False),     # 16,384 entries
            ('W3-bias_only-B7', 'bias_only', 3, 8, 7, False, False)]:
        shards = [ragged(W, P), second(W, P, full)]
        hp = dict(model_type=mt, latent_size=D, dropout=0.0, total_users=U, total_items=I, lr=LR, weight_decay=WD,
                  batch_size=P)
        makers = [_id_maker(sum(s), U, I, 3000 + D + P + W, 123) for s in shards]
        n = W * P
        out.append(WorldCase('mf-' + id, 'MFEngine', hp, steps_of(makers, shards, plant_ids(123, 7)), W, shards,
                             {'all_gather': 1}, defer=defer, entries=n, side='<=' if n <= 2048 else '>', limit=2048,
                             hot=[((5,), 123), ((6,), 7)], seed=11, weights=WEIGHTS_CLOSE))
    return out


def idnet_cases():
    U, I = 4000, 900
    out = []
    for kind, L, W, P, full in [('MF', 32, 3, 7, False), ('GMF', 5, 8, 300, True), ('NeuMF', 48, 5, 60, True)]:
        shards = [ragged(W, P), second(W, P, full)]
        hp = dict(model_type='MF' if kind == 'MF' else 'NeuMF', latent_size=L, dropout=0.0, total_users=U, total_items=I,
                  lr=LR, weight_decay=WD, word_embed_size=16, input_length=10, batch_size=P)
        if kind != 'MF':
            hp['neumf_stage'] = kind
        makers = [_id_maker(sum(s), U, I, 500 + L + P, 11) for s in shards]
        out.append(WorldCase('idnet-%s-L%d-W%d-B%d' % (kind, L, W, P), 'IdNetEngine', hp,
                             steps_of(makers, shards, plant_ids(11, 7, last=(U, I))), W, shards,
                             {'all_reduce': 1, 'all_gather': 1}, entries=W * P, side='<=', limit=32768,
                             hot=[((5,), 11), ((6,), 7)], last_rows=(U, I), seed=3, weights=weights_outliers(5e-3, 2.1 * LR)))
    return out


def narre_cases():
    out = []
    blocks, generic = {'all_reduce': 1, 'all_gather': 1}, {'all_reduce': 1, 'all_gather': 2}
    #    id           W   P   R   L  words E   V    U    I   full  collectives  max weight diff
    for id, W, P, R, L, words, E, V, U, I, full, coll, wmax in [
            ('W3-L10-B4', 3, 4, 10, 10, 12, 32, 300, 60, 50, False, blocks, 5e-4),            # shards (4, 0, 3): the block form
            ('W8-L8-B186', 8, 186, 10, 8, 12, 16, 200, 600, 500, True, blocks, 2.5e-3),       # 16,368 entries: the last block-form size
            ('W8-L8-B187', 8, 187, 10, 8, 12, 16, 200, 600, 500, True, generic, 2.5e-3),      # 16,456: -> r4r_narre_rows_apply_large
            ('W3-L33-B4', 3, 4, 10, 33, 12, 16, 300, 60, 50, False, generic, 2.5e-3)]:        # L > 32 at a small size: the same
        shards = [ragged(W, P), second(W, P, full)]
        hp = dict(model_type='NARRE', latent_size=L, word_embed_size=E, input_length=words, dropout=0.0, total_users=U,
                  total_items=I, lr=LR, weight_decay=WD, narre_num_reviews=R, narre_num_words=words, batch_size=P)
        makers = [narre_batches(sum(s), R, words, V, U, I, 700 + P + L, False) for s in shards]
        n = W * P * (1 + R)
        out.append(WorldCase('narre-' + id, 'NarreEngine', hp, steps_of(makers, shards), W, shards, coll, entries=n,
                             side='<=' if n <= 16384 else '>', limit=16384, hot=[((1, 5), 7), ((2, 6), 3)], vocab=V,
                             seed=12, weights=weights_outliers(2e-3, wmax)))
    return out


def plant_user(hot):
    def plant(step, data, bounds):
        for lo, hi in bounds:
            if hi > lo:
                data[5][lo] = hot
    return plant


def deepconnpp_cases():
    T, E, V, U, I = 40, 32, 300, 40, 30
    out = []
    for L, W, P, full, users, items in [(16, 3, 7, False, None, None), (16, 8, 40, True, 12, 8)]:
        shards = [ragged(W, P), second(W, P, full)]
        makers = [doc_batches(sum(s), T, V, U, I, 240 + L + P, users, items) for s in shards]
        out.append(WorldCase('deepconnpp-L%d-W%d-B%d' % (L, W, P), 'DeepCoNNPPEngine', _doc_hp('deepconn++', L, P, T, E, U, I),
                             steps_of(makers, shards, plant_user(3)), W, shards, {'all_reduce': 1, 'all_gather': 1},
                             entries=W * P, side='<=', limit=32768, hot=[((5,), 3)], vocab=V, seed=83,
                             weights=weights_outliers(2e-3, 5e-4)))
    return out


def transnet_cases():
    T, E, V, U, I = 40, 32, 300, 40, 30
    out = []
    blocks, generic = {'all_reduce': 1, 'all_gather': 1}, {'all_reduce': 1, 'all_gather': 2}
    for mt, L, W, P, full, users, coll in [('transnet++', 24, 3, 7, False, None, blocks),
                                           ('transnet++', 24, 8, 256, True, 12, blocks),      # 2,048 ratings: the last block-form size
                                           ('transnet++', 24, 8, 257, True, 12, generic),     # 2,056 -> r4r_transnet_rows_apply
                                           ('transnet', 24, 3, 7, False, None, {'all_reduce': 1})]:   # no ID rows at all
        shards = [ragged(W, P), second(W, P, full)]
        makers = [doc_batches(sum(s), T, V, U, I, 260 + L + P, users) for s in shards]
        plus = mt == 'transnet++'
        n = W * P
        out.append(WorldCase('%s-L%d-W%d-B%d' % (mt, L, W, P), 'TransNetEngine', _doc_hp(mt, L, P, T, E, U, I),
                             steps_of(makers, shards, plant_user(3) if plus else None), W, shards, coll, entries=n,
                             side='<=' if n <= 2048 else '>', limit=2048, hot=[((5,), 3)] if plus else [], rows=plus,
                             vocab=V, seed=4, weights=weights_outliers(2e-3, 5e-4)))
    return out


def deepconn_cases():
    T, E, V, U, I = 60, 32, 300, 40, 30
    out = []
    for L, W, P in [(16, 3, 7), (64, 8, 4)]:                 # step 1 of both has an empty shard
        shards = [ragged(W, P), second(W, P, False)]
        makers = [doc_batches(sum(s), T, V, U, I, 190 + L) for s in shards]
        for exchange, coll in [('allreduce', {'all_reduce': 1}), ('gather', {'gather_flat': 1})]:
            out.append(WorldCase('deepconn-L%d-W%d-%s' % (L, W, exchange), 'DeepCoNNEngine', _doc_hp('deepconn', L, P, T, E, U, I),
                                 steps_of(makers, shards), W, shards, coll, exchange=exchange, rows=False, vocab=V, seed=61,
                                 weights=weights_outliers(2e-3, 5e-4 if L <= 32 else 2.5e-3)))
    return out


def all_cases():
    return mf_cases() + idnet_cases() + narre_cases() + deepconnpp_cases() + transnet_cases() + deepconn_cases()
