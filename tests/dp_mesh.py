"""W data-parallel ranks in one process, on one GPU: a stand-in for dist.DataParallel, the runner that steps W engine
replicas through it, and the float32 oracle stepped in the same shards.

The native engines touch their communicator only through `dp.on`, `dp.world`, `dp.group`, `dp.stream_rccl`,
`dp.all_gather(out, t)`, `dp.allreduce_flat(t)` and `dp.gather_flat(t, out)` whenever `n_global` is passed to train_step,
and a rank's contribution to a step depends only on the shared state and on its own shard.  `Mesh(world)` hands out one
`RankStandIn` per rank with that surface; the result layouts are dist.DataParallel's (rank-major back-to-back slots for
the gathers, an in-place sum for the all-reduce: float32, the ranks added in rank order, computed the same way for every
rank, so the replicas receive identical bits).

The ranks run as W Python threads that pass a baton: exactly one thread is inside an engine or the library at any time
(its host side has unsynchronised function-local statics).  A rank runs until its next collective, synchronises the
device, deposits a copy of its tensor and hands the baton to the next rank; it continues when the baton returns, when
all W deposits are there.  Every wait has a time limit; an exception in one rank aborts the mesh, releases the others
and is re-raised by `Mesh.run`; a rank that made fewer collective calls than the others, or one of another kind or size,
is reported as a MeshMismatch, not waited for.  `Mesh.calls` holds the (kind, bytes) sequence of the last run.

`run_world(case)` takes a case of tests/dp_world_cases.py through its two steps on W engines built by
main.make_engine(..., dp=standin, rank=r): the engines' own `_train_step_dp` code at any W.

NOT reached from here: the one-process RCCL spans (`r4r_*_span_dp` call ncclAllReduce / ncclAllGather themselves: they
need a real communicator), the peer exchange (`R4R_DP_EXCHANGE=peer` maps other PROCESSES' segments), and anything a real
fabric does (the collectives' own arithmetic, their streams, their failure modes)."""
import threading

import torch

import oracle
from helpers import StepState, TRANSNET_GROUPS

WAIT_S = 120.0                      # the time limit of every wait of the mesh (a step takes milliseconds)


class MeshMismatch(RuntimeError):
    """The ranks did not make the same sequence of collective calls."""


class MeshTimeout(RuntimeError):
    """A wait of the mesh ran into its time limit."""


class _Aborted(BaseException):
    """Raised in the ranks that were waiting when another rank failed (never leaves Mesh.run)."""


class RankStandIn:
    """One rank's view of the mesh, with the attributes and methods of dist.DataParallel that the native engines use."""
    on, group, stream_rccl = True, None, None

    def __init__(self, mesh, rank):
        self.mesh, self.rank, self.world = mesh, rank, mesh.world

    def all_gather(self, out, t):
        """Rank r's contiguous `t` into out[r * n : (r + 1) * n]."""
        assert out.dtype == t.dtype and out.is_contiguous() and t.is_contiguous() and out.numel() == self.world * t.numel()
        self._gather('all_gather', out, t)

    def gather_flat(self, flat, out):
        """All ranks' flat buffers back to back in `out` [world * n], rank order."""
        assert out.dtype == flat.dtype and out.is_contiguous() and flat.is_contiguous()
        assert out.numel() == self.world * flat.numel()
        self._gather('gather_flat', out, flat)

    def _gather(self, kind, out, t):
        parts = self.mesh.collective(self.rank, kind, t)
        slots = out.view(-1).view(self.world, t.numel())
        for r, part in enumerate(parts):
            slots[r].copy_(part.view(-1))

    def allreduce_flat(self, flat):
        """In-place float32 sum of `flat` over the ranks, added in rank order."""
        assert flat.dtype == torch.float32
        parts = self.mesh.collective(self.rank, 'all_reduce', flat)
        total = parts[0].clone()
        for part in parts[1:]:
            total += part
        flat.copy_(total.view_as(flat))


class Mesh:
    def __init__(self, world, wait_s=WAIT_S):
        self.world, self.wait_s = int(world), float(wait_s)
        self.ranks = [RankStandIn(self, r) for r in range(self.world)]
        self.cv = threading.Condition()
        self.calls = []
        self._reset()

    def _reset(self):
        self.turn, self.failed = 0, None
        self.done = [False] * self.world
        self.log = [[] for _ in range(self.world)]
        self.rounds = {}                                     # round -> {rank: (kind, bytes, deposited copy)}
        self.taken = {}                                      # round -> how many ranks have read it

    # ---- the baton (every method below is called with self.cv held)
    def _wait_for_baton(self, rank):
        ok = self.cv.wait_for(lambda: self.failed is not None or self.turn == rank, self.wait_s)
        if self.failed is not None:
            raise _Aborted()
        if not ok:
            raise MeshTimeout('rank %d waited %.0f s for the baton (rank %d holds it)' % (rank, self.wait_s, self.turn))

    def _pass_baton(self, rank):
        for k in range(1, self.world + 1):
            nxt = (rank + k) % self.world
            if not self.done[nxt]:
                self.turn = nxt
                break
        self.cv.notify_all()

    def _fail(self, exc):
        if self.failed is None:
            self.failed = exc
        self.cv.notify_all()

    def collective(self, rank, kind, t):
        """Deposit `t` for this rank's next collective, hand the baton on, and return all ranks' deposits (rank order)
        once the baton is back."""
        if t.is_cuda:
            torch.cuda.synchronize()
        mine = (kind, t.numel() * t.element_size(), t.detach().clone())
        if t.is_cuda:
            torch.cuda.synchronize()
        with self.cv:
            k = len(self.log[rank])
            self.log[rank].append(mine[:2])
            self.rounds.setdefault(k, {})[rank] = mine
            self._pass_baton(rank)
            self._wait_for_baton(rank)
            # the baton went once round: every other rank has run to ITS k-th collective, or to its end
            got = self.rounds[k]
            missing = [r for r in range(self.world) if r not in got]
            if missing:
                raise MeshMismatch('collective %d (%s) of rank %d: ranks %s ended after fewer collectives'
                                   % (k, kind, rank, missing))
            kinds = sorted({v[:2] for v in got.values()})
            if len(kinds) != 1:
                raise MeshMismatch('collective %d: the ranks called %s' % (k, kinds))
            parts = [got[r][2] for r in range(self.world)]
            self.taken[k] = self.taken.get(k, 0) + 1
            if self.taken[k] == self.world:
                del self.rounds[k]
            return parts

    def run(self, body):
        """body(rank_stand_in) on every rank, as W threads under the baton -> the W results.  The first exception of a
        rank is re-raised here; the ranks' collective sequences must agree to the end."""
        self._reset()
        out, threads = [None] * self.world, []

        def rank_main(r):
            try:
                with self.cv:
                    self._wait_for_baton(r)
                res = body(self.ranks[r])
                if torch.is_tensor(res) and res.is_cuda:
                    torch.cuda.synchronize()
                out[r] = res
                with self.cv:
                    self.done[r] = True
                    self._pass_baton(r)
            except _Aborted:
                pass
            except BaseException as e:                       # noqa: BLE001 -- re-raised by run()
                with self.cv:
                    self._fail(e)

        for r in range(self.world):
            th = threading.Thread(target=rank_main, args=(r,), name='dp-mesh-rank-%d' % r, daemon=True)
            threads.append(th)
            th.start()
        for th in threads:
            th.join(self.wait_s * 2)
            if th.is_alive():
                with self.cv:
                    self._fail(MeshTimeout('%s did not end within %.0f s' % (th.name, self.wait_s * 2)))
        if self.failed is not None:
            raise self.failed
        if any(seq != self.log[0] for seq in self.log):
            raise MeshMismatch('the ranks made different collective calls: %s' % (self.log,))
        self.calls = list(self.log[0])
        return out

    def count(self, kind):
        return sum(1 for k, _ in self.calls if k == kind)


# ---------------------------------------------------------------------------------------------------- shards
def shard_bounds(sizes):
    """[(lo, hi)] of contiguous shards of the given sizes, rank order."""
    out, lo = [], 0
    for n in sizes:
        out.append((lo, lo + int(n)))
        lo += int(n)
    return out


def cut(data, y, lo, hi):
    return [None if d is None else d[lo:hi] for d in data], y[lo:hi]


# ---------------------------------------------------------------------------------------------------- the runner
class Snapshot:
    """What one rank held after a step, behind the duck type helpers.assert_step_state reads: moments() and
    state_dict() only.  (The engines' gradient introspection rebuilds ONE rank's shard: it stays hidden.)"""

    def __init__(self, se, sd, m, v):
        self.se, self.sd, self.m, self.v = se, sd, m, v

    def moments(self):
        return self.m, self.v

    def state_dict(self):
        return self.sd


def build_replica(case, dp, rank, dev='cuda'):
    import reviews4rec_amd
    from reviews4rec_amd import main as M
    P0 = case.params()
    hp = dict(case.hp)                                       # batch_size: the per-rank B_pad
    key = 'target.word2vec.weight' if hp['model_type'].startswith('transnet') else 'word2vec.weight'
    if key in P0:
        hp['word_vectors'] = P0[key].numpy()
    model = reviews4rec_amd.get_model_class(hp['model_type'])(hp)
    model.load_state_dict(P0)
    model = model.to(dev).train()
    eng = M.make_engine(dict(case.hp, engine='native', log_file=None), model, dp=dp, rank=rank)
    assert type(eng).__name__ == case.engine, type(eng).__name__
    if dp is not None:
        assert eng.dp is dp
        if case.exchange is not None:
            eng.exchange = case.exchange
    return model, eng


def snapshot(model, eng, se, deferred=False):
    if deferred:
        eng.flush()
    m, v = eng.moments()                                     # (flushes blocked sweeps)
    return Snapshot(se.detach().cpu().clone(), {k: t.detach().cpu().clone() for k, t in model.state_dict().items()},
                    {k: t.detach().cpu().clone() for k, t in m.items()}, {k: t.detach().cpu().clone() for k, t in v.items()})


def run_world(case, dev='cuda'):
    """The case's two steps on `case.world` engine replicas over a Mesh.  -> per step (snapshots by rank, the mesh's
    (kind, bytes) calls).  Each rank trains on its contiguous shard with n_global = the sum of the shard sizes;
    hyper_params['batch_size'] is the case's per-rank B_pad."""
    mesh = Mesh(case.world)
    reps = [build_replica(case, mesh.ranks[r], r, dev) for r in range(case.world)]
    steps = []
    kw = {'defer_sweep': True} if case.defer else {}
    for (data, y), sizes in zip(case.batches(), case.shards):
        assert sum(sizes) == y.numel() and len(sizes) == case.world
        on_dev = [None if d is None else d.to(dev) for d in data], y.to(dev)
        shards = [cut(*on_dev, lo, hi) for lo, hi in shard_bounds(sizes)]

        def body(rank):
            sd, sy = shards[rank.rank]
            return reps[rank.rank][1].train_step(sd, sy, n_global=int(y.numel()), **kw).clone()

        ses = mesh.run(body)
        steps.append(([snapshot(model, eng, se, case.defer) for (model, eng), se in zip(reps, ses)], list(mesh.calls)))
    return steps


def run_single(case, dev='cuda'):
    """The same two steps by ONE engine of the family on the concatenated batches (no data parallelism)."""
    model, eng = build_replica(case, None, 0, dev)
    out = []
    for data, y in case.batches():
        se = eng.train_step([None if d is None else d.to(dev) for d in data], y.to(dev))
        out.append(snapshot(model, eng, se))
    return out


# ---------------------------------------------------------------------------------------------------- the sharded oracle
DEFECTS = ('last_rank_dropped', 'local_loss_scale', 'padding_on_row_0')


class ShardedOracle:
    """The oracle stepped as the data-parallel engines step: every shard's gradient of sum(SE) / B_global from the same
    weights, the shards' gradients added in rank order (an empty shard adds nothing), one Adam step.  dtype float32: an
    independent implementation at the kernels' precision with the kernels' W partial sums -- the yardstick of
    helpers.oracle_atol, and (tests/test_dp_mesh_host.py) what the checker must pass, and must fail with a `defect`:

      last_rank_dropped   the last rank's shard never arrives
      local_loss_scale    every shard scaled by 1 / B_local
      padding_on_row_0    every padding entry (B_pad - n of each rank) lands on row 0 of every ID table and bias vector,
                          carrying a typical entry's gradient (the table's gradient per rating): what an update does
                          that clamps id -1 to 0 and reads a payload nobody cleared

    TransNet's three optimisers: each steps the gradient of its own loss (target: the target MSE; source: the transform
    loss; source_fm and the ID vectors: the source MSE).  The reference's retained-graph passes see post-step weights
    only where no stepped gradient depends on them, so all three are taken from the weights before the step."""

    def __init__(self, params, hyper_params, dtype=torch.float32, defect=None):
        assert defect is None or defect in DEFECTS
        self.hp, self.dtype, self.defect = dict(hyper_params), dtype, defect
        self.params = {k: v.detach().clone().to(dtype) for k, v in params.items()}
        self.transnet = self.hp['model_type'] in ('transnet', 'transnet++')
        self.states = {g: oracle.AdamState() for g in TRANSNET_GROUPS} if self.transnet else oracle.AdamState()
        self.steps = 0

    def _groups(self, names):
        if not self.transnet:
            return {None: list(names)}
        ids = ['user_embedding.weight', 'item_embedding.weight'] if self.hp['model_type'] == 'transnet++' else []
        return {'target': [k for k in names if k.startswith('target.')],
                'source': [k for k in names if k.startswith('source.')],
                'source_fm': [k for k in names if k.startswith('source_fm.')] + ids}

    def _shard_grads(self, data, y, scale_sum, scale_mean):
        """{name: gradient or None} of one shard; scale_sum multiplies a sum over the shard's ratings, scale_mean a
        mean over them."""
        names = oracle.trainable_names(self.params)
        leaves = {k: self.params[k].detach().clone().requires_grad_(True) for k in names}
        full = dict(self.params)
        full.update(leaves)
        out = oracle.model_forward(full, data, self.hp, train=True)
        y = y.to(self.dtype)
        groups = self._groups(names)
        if not self.transnet:
            se = oracle.mse_loss(out, y, return_mean=False)
            losses = {None: se.sum() * scale_sum}
        else:
            src, tgt, transform = out
            se = oracle.mse_loss(src, y, return_mean=False)
            losses = {'target': oracle.mse_loss(tgt, y) * scale_mean, 'source': transform * scale_mean,
                      'source_fm': se.sum() * scale_sum}
        grads = {}
        for g, loss in losses.items():
            got = torch.autograd.grad(loss, [leaves[k] for k in groups[g]], retain_graph=True, allow_unused=True)
            grads.update(zip(groups[g], got))
        return se.detach().reshape(-1), grads

    def step(self, data, y, sizes, B_pad=None, start=None):
        """One step on the batch cut into contiguous shards of `sizes`; start: the weights to step from (as
        helpers.float64_step_reference's).  -> StepState."""
        if start is not None:
            for k in oracle.trainable_names(self.params):
                self.params[k] = start[k].detach().cpu().to(self.dtype).clone()
        B = int(y.numel())
        assert sum(sizes) == B
        bounds = shard_bounds(sizes)
        if self.defect == 'last_rank_dropped':
            bounds = bounds[:-1]
        total, ses = {}, []
        for lo, hi in bounds:
            n = hi - lo
            if n == 0:
                continue
            local = self.defect == 'local_loss_scale'
            se, grads = self._shard_grads(*cut(data, y, lo, hi), scale_sum=1.0 / (n if local else B),
                                          scale_mean=1.0 if local else n / float(B))
            ses.append(se)
            for k, g in grads.items():
                total[k] = g if total.get(k) is None else (total[k] if g is None else total[k] + g)
        if self.defect == 'padding_on_row_0':
            pad = sum(int(B_pad) - n for n in sizes)
            for k, g in total.items():
                if g is not None and (k.endswith('embedding.weight') or k in ('user_bias', 'item_bias')):
                    g = g.clone()
                    g[0] += pad * g.sum(0) / B
                    total[k] = g
        names = oracle.trainable_names(self.params)
        for group, members in self._groups(names).items():
            state = self.states[group] if self.transnet else self.states
            oracle.adam_step(self.params, {k: total.get(k) for k in members}, state, self.hp['lr'], self.hp['weight_decay'])
        self.steps += 1
        m, v = {}, {}
        for st in (self.states.values() if self.transnet else [self.states]):
            m.update({k: t.clone() for k, t in st.m.items()})
            v.update({k: t.clone() for k, t in st.v.items()})
        se = torch.cat(ses) if ses else torch.zeros(0, dtype=self.dtype)
        return StepState(self.steps, float(se.sum()), se, {k: total.get(k) for k in names}, m, v,
                         {k: t.detach().clone() for k, t in self.params.items()}, {})
