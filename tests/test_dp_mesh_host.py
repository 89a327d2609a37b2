"""The data-parallel world tests' own machinery, without a GPU (tests/dp_mesh.py, tests/dp_world_cases.py):

  - the mesh alone, on CPU tensors, at worlds 1, 3 and 8: layouts, summation order, identical bits, a rank that raises,
    a rank that skips a collective;
  - the checker notices what the cases aim at: at every case's inputs the float32 oracle stepped in the case's shards
    (summed in rank order, scaled by 1 / B_global) passes helpers.assert_step_state against the float64 step on the
    concatenated batch, and fails with the last rank's shard dropped, with a 1 / B_local loss scale, and with the padding
    entries counted onto row 0;
  - the cases reach what they claim: hot ids in several ranks' shards, entry counts on the stated side of each
    threshold, no shard beyond B_pad."""
import time

import pytest
import torch

from dp_mesh import DEFECTS, Mesh, MeshMismatch, ShardedOracle, shard_bounds
from dp_world_cases import all_cases
from helpers import StateStandIn, assert_step_state, float64_step_reference

CASES = all_cases()
WORLDS = [1, 3, 8]


# ---------------------------------------------------------------------------------------------------- the mesh alone
@pytest.mark.parametrize('world', WORLDS)
def test_gathers_are_rank_major_and_every_rank_receives_the_same_bits(world):
    mesh = Mesh(world, wait_s=20)

    def body(rank):
        t = torch.arange(5, dtype=torch.int64) + 100 * rank.rank
        out = torch.full((world * 5,), -7, dtype=torch.int64)
        rank.all_gather(out, t)
        flat = torch.full((3,), float(rank.rank) + 0.5)
        out2 = torch.zeros(world * 3)
        rank.gather_flat(flat, out2)
        t += 1000                                            # (what a rank does to its buffer afterwards reaches nobody)
        return out, out2

    got = mesh.run(body)
    want = torch.cat([torch.arange(5, dtype=torch.int64) + 100 * r for r in range(world)])
    want2 = torch.cat([torch.full((3,), r + 0.5) for r in range(world)])
    for out, out2 in got:
        assert torch.equal(out, want) and torch.equal(out2, want2)
    assert mesh.calls == [('all_gather', 40), ('gather_flat', 12)]
    assert mesh.count('all_gather') == 1 and mesh.count('gather_flat') == 1 and mesh.count('all_reduce') == 0


@pytest.mark.parametrize('world', WORLDS)
def test_the_all_reduce_adds_float32_in_rank_order(world):
    """Terms whose float32 sum depends on the order: 2^24, then ones (each lost when added to 2^24 one at a time),
    then -2^24.  Rank order gives exactly what the loop below gives; any other association another number."""
    terms = [16777216.0] + [1.0] * (world - 2) + [-16777216.0] if world >= 3 else [0.1] * world
    mesh = Mesh(world, wait_s=20)

    def body(rank):
        flat = torch.tensor([terms[rank.rank], float(rank.rank)], dtype=torch.float32)
        rank.allreduce_flat(flat)
        return flat

    got = mesh.run(body)
    acc = torch.tensor([terms[0], 0.0], dtype=torch.float32)
    for r in range(1, world):
        acc = acc + torch.tensor([terms[r], float(r)], dtype=torch.float32)
    for flat in got:
        assert flat.dtype == torch.float32 and torch.equal(flat, acc)
    if world >= 3:
        assert float(acc[0]) == 0.0 and sum(terms) == world - 2      # (every 1 was lost on the way, in rank order)
    assert mesh.calls == [('all_reduce', 8)]


@pytest.mark.parametrize('world', WORLDS)
def test_a_rank_that_raises_ends_the_run_with_its_exception(world):
    mesh = Mesh(world, wait_s=20)

    def body(rank):
        t = torch.zeros(4)
        rank.allreduce_flat(t)
        if rank.rank == world - 1:
            raise KeyError('rank %d fell over' % rank.rank)
        rank.allreduce_flat(t)                               # the others are inside this one when it happens
        return t

    t0 = time.monotonic()
    with pytest.raises(KeyError, match='fell over'):
        mesh.run(body)
    assert time.monotonic() - t0 < 10                        # released, not timed out
    assert len(mesh.run(lambda rank: rank.rank)) == world    # and the mesh is usable again


@pytest.mark.parametrize('world', [3, 8])
def test_a_rank_that_skips_a_collective_is_a_mismatch_not_a_wait(world):
    mesh = Mesh(world, wait_s=20)

    def skips(rank):
        t = torch.zeros(4)
        rank.allreduce_flat(t)
        if rank.rank != 1:
            rank.all_gather(torch.zeros(world * 4), t)
        return t

    t0 = time.monotonic()
    with pytest.raises(MeshMismatch):
        mesh.run(skips)
    assert time.monotonic() - t0 < 10

    def another_size(rank):
        rank.allreduce_flat(torch.zeros(4 if rank.rank else 8))

    with pytest.raises(MeshMismatch, match='all_reduce'):
        mesh.run(another_size)

    def another_kind(rank):
        t = torch.zeros(4)
        if rank.rank == world - 1:
            rank.gather_flat(t, torch.zeros(world * 4))
        else:
            rank.all_gather(torch.zeros(world * 4), t)

    with pytest.raises(MeshMismatch):
        mesh.run(another_kind)


# ---------------------------------------------------------------------------------------------------- the checker
_FIRST = {}


def first_step(case):
    """The float64 step 1 on the concatenated batch, from the initial weights: shared by the clean run and the defects."""
    if case.id not in _FIRST:
        data, y = case.batches()[0]
        _FIRST[case.id] = float64_step_reference(case.params(), case.hp).step(data, y)
    return _FIRST[case.id]


def unique_inputs(cases):
    """DeepCoNN's two exchanges share their inputs: one of each on the CPU."""
    seen, out = set(), []
    for c in cases:
        key = c.id.replace('-gather', '').replace('-allreduce', '').replace('-deferred', '')
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize('case', unique_inputs(CASES), ids=repr)
def test_the_sharded_float32_oracle_passes_the_checker_on_every_case(case):
    o32 = ShardedOracle(case.params(), case.hp)
    ref = float64_step_reference(case.params(), case.hp)
    before = None
    for step, ((data, y), sizes) in enumerate(zip(case.batches(), case.shards)):
        s32 = o32.step(data, y, sizes)
        s64 = ref.step(data, y, start=before)
        torch.testing.assert_close(s32.se.double().sum(), torch.tensor(s64.sse, dtype=torch.float64), rtol=1e-4, atol=1e-3)
        assert_step_state(StateStandIn(s32, with_grads=False), StateStandIn(s32), s64, weights=case.weights, what=case.id)
        before = s32.params
    if case.rows:                                            # row 0 is named by nobody: what the padding defect shows in
        for k, zero in s64.zero_so_far.items():
            assert bool(zero[0].all()), k


# (DeepCoNN, plain TransNet: no entries, so nothing is padded)
PLANTED = [(c, d) for c in unique_inputs(CASES) for d in DEFECTS if c.rows or d != 'padding_on_row_0']


@pytest.mark.parametrize('case,defect', PLANTED, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_a_planted_defect_fails_the_checker(case, defect):
    data, y = case.batches()[0]
    sizes = case.shards[0]
    assert sizes[-1] > 0 and any(n < case.B_pad for n in sizes)
    s32 = ShardedOracle(case.params(), case.hp, defect=defect).step(data, y, sizes, B_pad=case.B_pad)
    with pytest.raises(AssertionError, match='exp_avg'):
        assert_step_state(StateStandIn(s32, with_grads=False), StateStandIn(s32), first_step(case), what=case.id)


# ---------------------------------------------------------------------------------------------------- the cases
def test_every_family_has_the_worlds_and_shards_the_issue_names():
    for family in ('MFEngine', 'IdNetEngine', 'NarreEngine', 'DeepCoNNPPEngine', 'TransNetEngine', 'DeepCoNNEngine'):
        mine = [c for c in CASES if c.engine == family]
        assert any(c.world % 2 == 1 for c in mine) and any(c.world == 8 for c in mine), family
        sizes = [s for c in mine for s in c.shards]
        assert any(0 in s[1:-1] for s in sizes), family      # an empty shard that is neither the first nor the last
        assert any(1 in s for s in sizes), family            # a shard of one rating
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_the_case_reaches_what_it_claims(case):
    assert len(case.shards) == len(case.batches()) == 2
    for (data, y), sizes in zip(case.batches(), case.shards):
        assert len(sizes) == case.world and sum(sizes) == y.numel()
        assert max(sizes) <= case.B_pad == case.hp['batch_size']
        bounds = shard_bounds(sizes)
        live = sum(1 for n in sizes if n)
        for slots, hot in case.hot:
            ranks = sum(1 for lo, hi in bounds if any(bool((data[s][lo:hi] == hot).any()) for s in slots))
            assert ranks >= min(3 if case.world > 3 else 2, live), (slots, hot, ranks)
        for s in (1, 2, 5, 6):
            if data[s] is not None and case.rows:
                assert not bool((data[s] == 0).any())
        if case.last_rows is not None:
            lo, hi = bounds[-1]
            assert bool((data[5][lo:hi] == case.last_rows[0]).any()) and bool((data[6][lo:hi] == case.last_rows[1]).any())
            P = case.params()
            tables = [k for k in P if k.endswith('embedding.weight')]
            assert tables and all(P[k].shape[0] == case.last_rows['user' not in k] + 1 for k in tables)
    if case.entries is not None:
        assert (case.entries <= case.limit) == (case.side == '<='), (case.entries, case.side, case.limit)


def test_the_size_cases_sit_on_the_thresholds():
    by_id = {c.id: c for c in CASES}
    at = lambda id: (by_id[id].entries, by_id[id].side, by_id[id].limit)   # noqa: E731
    assert at('mf-W8-D10-B256') == (2048, '<=', 2048) and at('mf-W8-D10-B257') == (2056, '>', 2048)
    assert at('mf-W8-D64-B2048')[0] == 16384
    assert at('narre-W8-L8-B186') == (16368, '<=', 16384) and at('narre-W8-L8-B187') == (16456, '>', 16384)
    assert by_id['narre-W3-L33-B4'].hp['latent_size'] == 33 and at('narre-W3-L33-B4')[1] == '<='
    assert at('transnet++-L24-W8-B256') == (2048, '<=', 2048) and at('transnet++-L24-W8-B257') == (2056, '>', 2048)
    # the one-exchange forms and the payload forms differ by one all_gather
    assert by_id['narre-W8-L8-B186'].collectives['all_gather'] == 1 and by_id['narre-W8-L8-B187'].collectives['all_gather'] == 2
    assert by_id['narre-W3-L33-B4'].collectives['all_gather'] == 2
    assert by_id['transnet++-L24-W8-B257'].collectives['all_gather'] == 2


def test_the_thresholds_are_the_engines_own():
    """Where engine.py carries the threshold as a constant, the cases' limits are read against it."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'reviews4rec_amd', 'engine.py')).read()
    assert re.search(r'ROWS_APPLY_MAX = 16384\b', src) and re.search(r'BLOCKS_MAX_ENTRIES = 2048\b', src)
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'reviews4rec_amd', 'csrc')
    mf = open(os.path.join(csrc, 'mf_engine.hip')).read()
    assert re.search(r'MF_SCAN_MAX_B = 2048;', mf) and re.search(r'MF_MAX_B_STEP = 1 << 20;', mf)
    assert 'B <= MF_MAX_B_STEP, "mf_apply' in mf
