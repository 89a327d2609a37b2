"""bench.py's host-side logic that needs no GPU: the self-launch of `--gpus N`, the one-line device-count error, the
walked-position count behind the gather leg's bytes (a restatement of the kernel's rule, slice by slice)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(argv):
    old = sys.argv
    sys.argv = ['bench.py'] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_bare_multi_gpu_command_relaunches_itself_under_torch_distributed_run(monkeypatch):
    """`python bench.py --gpus 2 ...` with no launcher: the process runs the N-rank job (one rank per GPU, static
    rendezvous on 127.0.0.1) as its child, passing its own arguments through, and exits with the job's status."""
    seen = {}
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.setenv('R4R_DIST_BACKEND', 'gloo')           # (no GPU here: the device-count check is RCCL's)
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd: seen.update(cmd=cmd) or 3)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '20', '--warmup', '5'])
    with pytest.raises(SystemExit) as e:
        bench.self_launch(bench.parse())
    assert e.value.code == 3
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node' in cmd and cmd[cmd.index('--nproc-per-node') + 1] == '2'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and int(cmd[cmd.index('--master-port') + 1]) > 0
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == ['--gpus', '2', '--steps', '20', '--warmup', '5']


def test_no_relaunch_inside_a_launched_job_or_at_one_gpu(monkeypatch):
    monkeypatch.setattr(bench.subprocess, 'call', lambda *a: pytest.fail('re-launched'))
    monkeypatch.setenv('WORLD_SIZE', '2')
    bench.self_launch(_args(['--gpus', '2']))
    monkeypatch.delenv('WORLD_SIZE')
    monkeypatch.delenv('RANK', raising=False)
    bench.self_launch(_args(['--gpus', '1']))


def test_more_ranks_than_gpus_is_one_clear_line(monkeypatch):
    monkeypatch.delenv('R4R_DIST_BACKEND', raising=False)
    with pytest.raises(SystemExit) as e:
        bench.check_device_count(64)
    assert '--gpus 64' in str(e.value) and 'visible' in str(e.value) and '\n' not in str(e.value)


def _walked_by_the_kernels_rule(doc):
    """proj_gather_max_kernel, one document: P = T + 2 positions in segments of 128, a segment dealt to four workers in
    equal slices (32 positions of a full segment, ceil(len / 4) of a shorter one); a worker's tokens are p_lo - 2 ..
    p_hi - 1; a token outside [0, T) has slot -1; all slots equal -> one position walked."""
    T = len(doc)
    P = T + 2
    walked = 0
    for seg in range((P + 127) // 128):
        seg_len = min(128, P - seg * 128)
        slen = 32 if seg_len == 128 else (seg_len + 3) // 4
        for worker in range(4):
            p_lo = seg * 128 + worker * slen
            p_hi = min(min(P, (seg + 1) * 128), p_lo + slen)
            if p_hi <= p_lo:
                continue
            slots = [int(doc[t]) if 0 <= t < T else -1 for t in range(p_lo - 2, p_hi)]
            walked += 1 if len(set(slots)) == 1 else p_hi - p_lo
    return walked


@pytest.mark.parametrize('T', [100, 126, 127, 250, 1000])
def test_walked_positions_follow_the_kernels_slice_rule(T):
    rng = np.random.default_rng(T)
    docs = rng.integers(1, 50, size=(6, T))
    docs[0, :] = 0                                           # an all-padding document
    docs[1, T // 3:] = 0                                     # a padded tail
    docs[2, :] = 7                                           # one word repeated: uniform inside, not at the edges
    docs[3, 40:200] = 0                                      # padding in the middle
    w, total = bench.walked_positions(docs)
    assert total == 6 * (T + 2)
    assert w == sum(_walked_by_the_kernels_rule(d) for d in docs)
    w3, t3 = bench.walked_positions(docs.reshape(2, 3, T))   # NARRE's [B, R, W] documents
    assert (w3, t3) == (w, total)


def test_config_legs_ride_on_the_default_line_only():
    assert bench.config_legs_wanted(_args([]), dp_job=False)
    assert bench.config_legs_wanted(_args(['--gpus', '1', '--steps', '20', '--warmup', '5']), dp_job=False)
    assert not bench.config_legs_wanted(_args([]), dp_job=True)
    assert not bench.config_legs_wanted(_args(['--no-cpu-baseline']), dp_job=False)
    assert bench.config_legs_wanted(_args(['--no-cpu-baseline', '--config-legs']), dp_job=False)
    assert not bench.config_legs_wanted(_args(['--workload', 'cfg2_mfdot_electronics']), dp_job=False)
    assert not bench.config_legs_wanted(_args(['--doc-fill', 'full']), dp_job=False)
    labels = [l for l, _ in bench.CONFIG_LEGS]
    for want in ('cfg1_bias_only_musical', 'cfg2_mfdot_electronics', 'cfg2_mfdot_electronics_b8192', 'cfg4_narre_kindle',
                 'cfg5_transnetpp_synthetic', 'cfg3_full_uniform', 'cfg5_full_uniform_hbm_gather'):
        assert want in labels


def test_dump_outputs_writes_every_array_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: one DIR/<name>.npy per array, float32 (float64 where the tensor is), a large tensor as a sample of
    its elements at positions drawn from a fixed seed -- the same positions on every run -- and 64 MB at most in all."""
    import torch
    assert _args(['--dump-outputs', str(tmp_path)]).dump_outputs == str(tmp_path)
    assert _args([]).dump_outputs is None
    g = torch.Generator().manual_seed(0)
    arrays = {'pred': torch.randn(128, generator=g), 'se': torch.randn(128, generator=g, dtype=torch.float64),
              'param.table': torch.randn(1000, 300, generator=g), 'param.ids': torch.arange(10)}
    n1 = bench.dump_outputs(str(tmp_path / 'a'), arrays)
    n2 = bench.dump_outputs(str(tmp_path / 'b'), arrays)
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(k + '.npy' for k in arrays) and n1 == n2
    for k, t in arrays.items():
        a, b = np.load(tmp_path / 'a' / (k + '.npy')), np.load(tmp_path / 'b' / (k + '.npy'))
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32) and np.array_equal(a, b)
        if t.numel() <= bench.DUMP_SAMPLE:
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.numpy().astype(a.dtype))
        else:
            assert a.shape == (bench.DUMP_SAMPLE,) and np.isin(a, t.numpy().reshape(-1)).all()
    # many large tensors: each one's share of the budget, 64 MB in all
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 1 << 20)
    big = {'p%d' % i: torch.zeros(1 << 16, dtype=torch.float64) for i in range(40)}
    bench.dump_outputs(str(tmp_path / 'c'), big)
    assert sum(os.path.getsize(tmp_path / 'c' / f) for f in os.listdir(tmp_path / 'c')) <= 1 << 20


def test_dump_outputs_of_the_module_path_are_the_last_steps_tensors():
    import torch
    model = torch.nn.Linear(3, 1)
    last = {'pred': torch.ones(4), 'se': torch.zeros(4)}
    got = bench.last_step_arrays(model, None, None, last, 4)
    assert sorted(got) == ['param.bias', 'param.weight', 'pred', 'se'] and got['pred'] is last['pred']


@pytest.mark.gpu
def test_dump_outputs_of_two_runs_with_the_same_arguments_agree(tmp_path):
    """The flagship command with --dump-outputs, twice: the same inputs every run, so the same files -- the last timed
    step's per-rating prediction and SE of the 128-rating batch and every parameter after its update."""
    import json
    import subprocess
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'R4R_DP_SINGLE'):
        env.pop(k, None)
    got = []
    for run in ('a', 'b'):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2', '--ramp', '0',
               '--no-cpu-baseline', '--no-steady-leg', '--dump-outputs', str(tmp_path / run)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line['steps'] == 5 and line['ms_per_step'] > 0
        got.append({f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    a, b = got
    assert sorted(a) == sorted(b) and a['pred.npy'].shape == a['se.npy'].shape == (128,)
    assert any(f.startswith('param.') for f in a) and sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f
