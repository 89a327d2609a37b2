"""Data-parallel spans of every native family other than DeepCoNN (include/r4r.h, r4r_<family>_span_dp; engine._Spans):
an epoch of main.train whose full batches go through the span entry -- the step, RCCL's collectives and the updates
enqueued from C, K steps per host call -- must leave EXACTLY what the same epoch leaves through the per-step
data-parallel path (_train_step_dp): the epoch metrics, every parameter, every Adam moment, the step count, the dropout
stream position, the sweep schedule.  Dropout on, a ragged last batch, two epochs, SPAN_STEPS = 9 (not a divisor of the
batch groups).

As a ONE-rank RCCL job (R4R_DP_SINGLE=1: the test box has one GPU, RCCL wants one per rank): every call of the N > 1
path is made with the real communicator; the collectives move nothing.  The loop the spans replace is the reference's
main.py:23-60 on every rank."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = ['NARRE', 'deepconn++', 'transnet', 'transnet++', 'MF_dot', 'bias_only', 'MF', 'NeuMF']
# configurations the C side does not take: every step through train_step, no span call, the same bits
FALLBACKS = {'MF_dot@peer': ('MF_dot', {}, {'R4R_DP_EXCHANGE': 'peer'}),
             'NARRE@L40': ('NARRE', {'latent_size': 40}, {})}
SPAN_STEPS = 9
FULL_BATCHES = 1500 // 32                # tiny_corpus' ratings at test_gpu_span.hyper's batch_size: 46 full, a ragged 28


def _run(mt, corpus, spans, hp_kw, rank):
    import reviews4rec_amd
    from reviews4rec_amd import dist as r4dist, main as M
    from reviews4rec_amd.data import DataLoader
    from reviews4rec_amd.loss import MSELoss
    from reviews4rec_amd.utils import xavier_init
    from test_gpu_span import hyper
    kw = dict(hp_kw)
    if mt == 'NeuMF':
        kw['neumf_stage'] = 'NeuMF'                          # NeuMF.py's full model: two table pairs
    hp = hyper(mt, spans=spans, **kw)
    reader = DataLoader(hp, corpus['train'], corpus['user_reviews'], corpus['item_reviews'], None,
                        this_index_user_item=corpus['this_index_user_item'], device='cuda')
    torch.manual_seed(5)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    xavier_init(model)
    model = model.cuda()
    dp = r4dist.DataParallel(model)
    dp.broadcast_parameters()
    engine = M.make_engine(hp, model, dp=dp, rank=rank)
    engine.SPAN_STEPS = SPAN_STEPS
    calls = [0]
    inner = engine._span

    def counting(*a, _inner=inner, **k):
        calls[0] += 1
        return _inner(*a, **k)
    engine._span = counting
    metrics = [M.train(model, MSELoss(hp), None, reader, hp, engine=engine, dp=dp) for _ in range(2)]
    torch.cuda.synchronize()
    sweep = tuple(getattr(engine, a, None) for a in ('_tb_base', '_tb_period', '_tb_used'))   # (before a flush moves it)
    weights = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}   # (the ID tables flushed)
    opt = engine.state_dict()
    moments = {k: v.detach().cpu().clone() for part in ('exp_avg', 'exp_avg_sq') for k, v in
               ((part + '/' + n, t) for n, t in opt[part].items())}
    dp.close()
    return dict(metrics=metrics, weights=weights, moments=moments, counts=(engine.step_count, engine.offset),
                sweep=sweep, calls=calls[0])


def _worker(rank, world, port, out_dir):
    import traceback
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), R4R_DIST_BACKEND='nccl', R4R_DP_SINGLE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    from reviews4rec_amd import dist as r4dist
    from test_gpu_span import tiny_corpus
    r4dist.init_from_env()
    corpus = tiny_corpus(seed=16)
    res = {}
    cases = [(mt, mt, {}, {}) for mt in FAMILIES] + [(name,) + v for name, v in FALLBACKS.items()]
    for name, mt, hp_kw, env in cases:
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            res[name] = {spans: _run(mt, corpus, spans, hp_kw, rank) for spans in (False, True)}
        except Exception:                                    # noqa: BLE001 -- reported by the family's own test
            res[name] = traceback.format_exc()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    torch.save(res, os.path.join(out_dir, 'span_dp.pt'))
    torch.distributed.destroy_process_group()


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    import socket
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_dist import _need_rccl
    _need_rccl()
    out = tmp_path_factory.mktemp('span_dp')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(1, port, str(out)), nprocs=1, join=True)
    return torch.load(os.path.join(out, 'span_dp.pt'))


def _same(a, b):
    assert a['metrics'] == b['metrics']
    assert set(a['weights']) == set(b['weights']) and set(a['moments']) == set(b['moments'])
    for part in ('weights', 'moments'):
        bad = [k for k in a[part] if not torch.equal(a[part][k], b[part][k])]
        assert not bad, (part, bad)
    assert a['counts'] == b['counts'] and a['sweep'] == b['sweep'], (a['counts'], b['counts'], a['sweep'], b['sweep'])


@pytest.mark.parametrize('mt', FAMILIES)
def test_dp_span_epochs_leave_the_bits_of_the_per_step_exchange(results, mt):
    r = results[mt]
    assert not isinstance(r, str), r
    per_step, spans = r[False], r[True]
    assert per_step['calls'] == 0, per_step['calls']
    assert spans['calls'] >= 2 * (FULL_BATCHES // SPAN_STEPS), spans['calls']   # the epochs really went through C
    _same(per_step, spans)


@pytest.mark.parametrize('case', sorted(FALLBACKS))
def test_configurations_outside_the_c_forms_stay_per_step(results, case):
    r = results[case]
    assert not isinstance(r, str), r
    assert r[False]['calls'] == 0 and r[True]['calls'] == 0, (r[False]['calls'], r[True]['calls'])
    _same(r[False], r[True])


@pytest.mark.parametrize('workload', ['cfg4_narre_kindle', 'cfg2_mfdot_electronics'])
def test_rccl_one_rank_bench_line_enqueues_dp_spans(workload):
    """bench.py as the driver launches it for N > 1, with one rank over RCCL: the data-parallel steps go through the
    resident descriptor's span entry (engine._span_dp_ok), and the replicas stay identical."""
    import json
    import subprocess
    from test_gpu_dist import _free_port, _need_rccl
    _need_rccl()
    env = dict(os.environ, R4R_DP_SINGLE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('R4R_DIST_BACKEND', None)
    cmd = ['timeout', '-k', '10', '540', sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node',
           '1', '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus',
           '1', '--steps', '20', '--warmup', '5', '--no-cpu-baseline', '--no-config-legs', '--strong-leg', '1024',
           '--workload', workload]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    cfg = line['config']
    assert cfg['dist_backend'] == 'nccl' and cfg['rccl_ranks'] == 1 and cfg['replicas_identical'] is True, cfg
    assert cfg['enqueue'].startswith('spans'), cfg['enqueue']
    assert line['value'] > 0
