"""The data-parallel steps at 3 to 8 ranks, against the oracle in float64.

tests/test_gpu_dist.py spawns two processes on a dozen ratings; the index arithmetic of the data-parallel kernels
(blocks back to back at rank * block_bytes, B_pad self entries then the neighbour entries inside a block, id -1 past a
rank's own count, rows summed across block boundaries in (rank, in-block) order, another form of the update beyond
world * B_pad thresholds) depends on `world`.  Here W engine replicas run their own `_train_step_dp` in ONE process over
a stand-in communicator (tests/dp_mesh.py; its docstring says what that cannot reach: the RCCL spans, the peer
exchange, a real fabric), on the cases of tests/dp_world_cases.py.  After each of two steps:

  1. every weight, exp_avg and exp_avg_sq of ranks 1 .. W-1 equals rank 0's, bit for bit;
  2. rank 0's moments and weights against the float64 step on the concatenated batch from the weights held before the
     step (helpers.assert_step_state: STATE_RTOL, GRAD_ATOL, EXP_AVG_SQ_ATOL, PURE_WD_ATOL, the family's weight
     criterion), and the ranks' per-example SE, concatenated, against its SSE;
  3. MF_dot / bias_only: weights and moments equal, bit for bit, one MFEngine stepping the concatenated batch;
  4. a second run of the case leaves the same bits;
  5. the collectives the step made: kind and number.

No tolerance is introduced and none is widened: no case lists a tensor in `widen` (a tensor listed there would be held
to helpers.oracle_atol -- 8 x the distance of the float32 oracle stepped in the same W shards from float64 -- instead of
the base atol).  Every test prints, per step, the engine's worst distances and that sharded oracle's."""
import pytest
import torch

from dp_mesh import ShardedOracle, run_single, run_world
from dp_world_cases import deepconn_cases, deepconnpp_cases, idnet_cases, mf_cases, narre_cases, transnet_cases
from helpers import StateStandIn, assert_step_state, float64_step_reference, oracle_atol, state_distances

pytestmark = pytest.mark.gpu


def worst(d):
    return ', '.join('%s %.3g (%s)' % ((kind,) + max((v, k) for k, v in per.items())) for kind, per in d.items() if per)


def same_bits(a, b, what):
    for kind, x, z in (('weight', a.sd, b.sd), ('exp_avg', a.m, b.m), ('exp_avg_sq', a.v, b.v)):
        assert set(x) == set(z), (what, kind)
        for k in x:
            assert torch.equal(x[k], z[k]), '%s: %s %s differs' % (what, kind, k)


def check_world(case):
    first = run_world(case)
    P0 = case.params()
    ref = float64_step_reference(P0, case.hp)
    o32 = ShardedOracle(P0, case.hp)
    before = None
    for step, ((snaps, calls), (data, y), sizes) in enumerate(zip(first, case.batches(), case.shards)):
        assert len(snaps) == case.world
        for r in range(1, case.world):                       # 1. replicas hold the same bits
            same_bits(snaps[r], snaps[0], '%s step %d: rank %d against rank 0' % (case.id, step + 1, r))
        r64 = ref.step(data, y, None, start=before)          # 2. against float64, from the weights held before the step
        r32 = o32.step(data, y, sizes, start=before)
        print('DP-WORLD %s %s W%d step %d | engine: %s | float32 sharded oracle: %s'
              % (case.engine, case.id, case.world, r64.step, worst(state_distances(snaps[0], r64)),
                 worst(state_distances(StateStandIn(r32, with_grads=False), r64))))
        assert [s.se.numel() for s in snaps] == list(sizes)
        se = torch.cat([s.se.reshape(-1) for s in snaps])
        torch.testing.assert_close(se.double().sum(), torch.tensor(r64.sse, dtype=torch.float64), rtol=1e-4, atol=1e-3)
        atol = {(kind, name): oracle_atol(r64, r32, kind, name) for kind, name in case.widen}
        assert_step_state(snaps[0], snaps[0], r64, weights=case.weights, atol=atol, what=case.id)
        kinds = {}                                           # 5. the collectives of the step
        for kind, _ in calls:
            kinds[kind] = kinds.get(kind, 0) + 1
        assert kinds == case.collectives, (case.id, step + 1, calls)
        before = snaps[0].sd
    if case.engine == 'MFEngine':                            # 3. the single-process step on the concatenated batch
        for step, ((snaps, _), single) in enumerate(zip(first, run_single(case))):
            same_bits(snaps[0], single, '%s step %d: rank 0 against the single-process step' % (case.id, step + 1))
    if case.defer:                                           # the blocked sweep + flush(): the bits of the plain sweep
        for step, ((snaps, _), (plain, _)) in enumerate(zip(first, run_world(case.plain()))):
            same_bits(snaps[0], plain[0], '%s step %d: deferred against plain' % (case.id, step + 1))
    for step, ((snaps, _), (again, _)) in enumerate(zip(first, run_world(case))):   # 4. a second run: the same bits
        for r in range(case.world):
            same_bits(snaps[r], again[r], '%s step %d rank %d: second run' % (case.id, step + 1, r))
            assert torch.equal(snaps[r].se, again[r].se), '%s step %d rank %d: per-example SE of a second run' % (case.id, step + 1, r)


@pytest.mark.parametrize('case', mf_cases(), ids=repr)
def test_mf_worlds(case):
    """r4r_mf_grad -> one all_gather -> r4r_mf_apply at W 3 (shards (7, 0, 4)), 5 and 8; 2,048 gathered entries (the
    last one-launch size), 2,056 (the first behind the registering launch), 16,384; bias_only; one case with the blocked
    sweep and flush(), bit-equal to the plain sweep.  All bit-equal to the single-process step."""
    check_world(case)


@pytest.mark.parametrize('case', idnet_cases(), ids=repr)
def test_idnet_worlds(case):
    """gather_entry_fields -> r4r_idnet_rows_apply: MF at L 32 / W 3, GMF at L 5 / W 8 / B_pad 300, NeuMF at L 48 / W 5;
    the last row of each table named on the last rank."""
    check_world(case)


@pytest.mark.parametrize('case', narre_cases(), ids=repr)
def test_narre_worlds(case):
    """r4r_narre_dp_block -> r4r_narre_rows_apply_blocks at W 3 (shards (4, 0, 3)) and at 16,368 entries over 8 ranks;
    16,456 entries, and L 33 at a small size: the payload form (two all_gathers) -> r4r_narre_rows_apply_large."""
    check_world(case)


@pytest.mark.parametrize('case', deepconnpp_cases(), ids=repr)
def test_deepconnpp_worlds(case):
    """gather_entry_fields -> r4r_deepconnpp_rows_apply at W 3 ragged and W 8 with users drawn from 12 ids."""
    check_world(case)


@pytest.mark.parametrize('case', transnet_cases(), ids=repr)
def test_transnet_worlds(case):
    """TransNet++: r4r_transnet_dp_block -> r4r_transnet_rows_apply_blocks at W 3 and at 2,048 ratings over 8 ranks, the
    payload form -> r4r_transnet_rows_apply at 2,056; plain TransNet at W 3: the three optimisers' dense groups only."""
    check_world(case)


@pytest.mark.parametrize('case', deepconn_cases(), ids=repr)
def test_deepconn_worlds(case):
    """DeepCoNN at W 3 and W 8 under both exchanges: the all-reduce -> r4r_adam_multi, and gather_flat ->
    r4r_adam_gathered (which adds the ranks in rank order); step 1 has an empty shard."""
    check_world(case)
