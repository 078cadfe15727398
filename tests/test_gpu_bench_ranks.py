"""`python bench.py --gpus N` must start N ranks by itself (round-2 verdict: without a launcher around
it, it silently measured ONE GPU and printed n_gpus: 1 for a --gpus 8 command).

The gpurun box has one GPU and RCCL refuses two ranks on one device, so the two ranks share cuda:0
over gloo (MTR_BENCH_SHARED_DEVICE=1): this runs the N > 1 code path end to end -- self-spawn through
torch.distributed.run, rank binding, sharding of internal batches (multiperson_model.py:189-220's unit),
barrier + max-over-ranks timing, the single gather -- but is not a scaling measurement."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
                 'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'}


def run_bench(*flags, shared=True, timeout=1200):
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    if shared:
        env['MTR_BENCH_SHARED_DEVICE'] = '1'
    else:
        env.pop('MTR_BENCH_SHARED_DEVICE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *flags], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    return r, (json.loads(lines[-1]) if lines else None), lines


def keep(name, line):
    out = os.path.join(ROOT, 'gpurun_out')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), 'w') as f:
            f.write(json.dumps(line) + '\n')
    except OSError:
        pass


def test_plain_line_and_dumped_outputs_are_reproducible(hip_lib, tmp_path):
    """A plain run prints the contract line without the probes (roofline / cpu_baseline null), times exactly
    --steps steps, and --dump-outputs writes the last step's poses; the same arguments give the same inputs,
    hence the same poses in a second process up to the reconstruction's fp32 run-to-run jitter (measured
    <= 0.013 mm).  The random network puts a few poses' joints at the camera plane, where the 2D projection
    is ill-conditioned (tens of px apart from run to run): poses2d is compared on the poses in front."""
    import numpy as np
    lines = []
    for run in ('a', 'b'):
        r, line, _ = run_bench('--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / run),
                               shared=False, timeout=600)
        assert r.returncode == 0 and line is not None, r.stderr[-2000:]
        lines.append(line)
    line = lines[0]
    assert CONTRACT_KEYS <= set(line) and line['roofline'] is None and line['cpu_baseline'] is None
    assert line['steps'] == 2 and line['unit'] == 'crops/s' and line['higher_is_better'] is True
    assert abs(line['value'] - line['config']['global_batch'] / line['ms_per_step'] * 1e3) < 1e-6 * line['value']
    dumps = {}
    for name, shape in (('poses3d', (64, 17, 3)), ('poses2d', (64, 17, 2))):
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
        dumps[name] = a, b
    (a3, b3), (a2, b2) = dumps['poses3d'], dumps['poses2d']
    assert float(np.abs(a3 - b3).max()) <= 0.05
    front = (a3[..., 2] > 100).all(axis=1)   # (mm: every joint at least 10 cm in front of the camera)
    assert front.sum() >= 32 and float(np.abs(a2[front] - b2[front]).max()) <= 1e-2


def test_gpus_2_on_one_gpu_refuses_instead_of_measuring_one(hip_lib):
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('a multi-GPU box: nothing to refuse')
    r, line, _ = run_bench('--gpus', '2', '--steps', '1', '--warmup', '0', '--quick', shared=False, timeout=300)
    assert r.returncode != 0 and line is None
    assert 'refusing' in (r.stderr + r.stdout)


def test_launcher_and_flag_disagreeing_is_an_error(hip_lib):
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--quick', '--steps', '1'],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and 'disagree' in (r.stderr + r.stdout)


def test_gpus_2_weak_scaling_line(hip_lib):
    r1, one, _ = run_bench('--gpus', '1', '--steps', '3', '--warmup', '1', '--quick', shared=False)
    assert r1.returncode == 0 and one is not None, r1.stderr[-2000:]
    r, two, lines = run_bench('--gpus', '2', '--steps', '3', '--warmup', '1', '--quick')
    assert r.returncode == 0 and two is not None, r.stderr[-2000:]
    assert len(lines) == 1, 'only rank 0 prints the line'
    assert CONTRACT_KEYS <= set(two)
    assert two['n_gpus'] == 2 and one['n_gpus'] == 1
    assert two['scaling'] == 'weak' and two['config']['global_batch'] == 2 * one['config']['global_batch']
    m = two['multi_gpu']
    assert len(m['per_rank_ms_per_step']) == 2 and m['backend'] == 'gloo'
    assert abs(max(m['per_rank_ms_per_step']) - two['ms_per_step']) < 1e-2  # the max over ranks is the job's time
    # two ranks SHARE one GPU here: the job moves twice the crops in about twice the time, i.e. about the
    # one-GPU rate (graphs of the two processes interleave; the host-side gloo gather adds a little)
    assert 0.45 * one['value'] <= two['value'] <= 1.35 * one['value'], (one['value'], two['value'])
    keep('bench_gpus2_shared_device_config1.json', two)


def test_gpus_2_strong_scaling_line(hip_lib):
    r, two, lines = run_bench('--gpus', '2', '--steps', '2', '--warmup', '1', '--quick', '--config', '2',
                              '--total-crops', '128')
    assert r.returncode == 0 and two is not None, r.stderr[-2000:]
    assert len(lines) == 1 and CONTRACT_KEYS <= set(two)
    assert two['n_gpus'] == 2 and two['scaling'] == 'strong'
    assert two['config']['global_batch'] == 128 and 'configs[2]' in two['config']['workload']
    assert len(two['multi_gpu']['per_rank_ms_per_step']) == 2
    assert two['value'] > 0
    keep('bench_gpus2_shared_device_config2.json', two)


@pytest.mark.parametrize('config, global_batch, scaling', [(1, 8 * 64, 'weak'), (2, 256, 'strong')])
def test_gpus_8_line(hip_lib, config, global_batch, scaling):
    """The command the driver's 8-GPU run issues (VERDICT r5 next #4a), all eight ranks on cuda:0 over gloo:
    self-spawn of 8 ranks, rank binding, sharding, barrier + max-over-ranks timing, the gather, and -- with
    --full -- rank 0's whole post-timing analysis while seven ranks wait at the final barrier.  The line must
    carry a roofline object and no `<probe>_error` key."""
    flags = ['--gpus', '8', '--steps', '3', '--warmup', '1']
    if config == 1:
        flags += ['--full']
    else:
        flags += ['--config', str(config), '--quick']   # (the post-timing analysis at N = 8 is exercised by configs[1])
    r, line, lines = run_bench(*flags, timeout=1500)
    assert r.returncode == 0 and line is not None, r.stderr[-3000:]
    assert len(lines) == 1, 'only rank 0 prints the line'
    assert CONTRACT_KEYS <= set(line)
    assert line['n_gpus'] == 8 and line['scaling'] == scaling
    assert line['config']['global_batch'] == global_batch
    m = line['multi_gpu']
    assert len(m['per_rank_ms_per_step']) == 8 and m['world_size'] == 8
    assert abs(max(m['per_rank_ms_per_step']) - line['ms_per_step']) < 1e-2
    assert line['value'] > 0 and abs(line['value'] - global_batch / line['ms_per_step'] * 1e3) < 1e-6 * line['value'] + 1e-3
    if config == 1:
        assert line['roofline'] is not None and 0 < line['roofline']['frac'] < 1
    assert line['cpu_baseline'] is None   # (rank 0 at N = 1 only)
    errors = {k: v for k, v in line.items() if k.endswith('_error')}
    assert not errors, errors
    keep(f'bench_gpus8_shared_device_config{config}.json', line)


def test_a_failing_probe_does_not_lose_the_line(hip_lib):
    """every probe of the post-timing analysis is guarded.  MTR_BENCH_FAIL_PROBE makes the named
    probes raise; the contract line still comes out, with roofline / cpu_baseline computed (they run first) and the
    failures named."""
    env_before = os.environ.get('MTR_BENCH_FAIL_PROBE')
    os.environ['MTR_BENCH_FAIL_PROBE'] = 'parity,pcie_inclusive,detector_pre'
    try:
        r, line, _ = run_bench('--full', '--steps', '3', '--warmup', '1', '--no-pmc', '--no-depth72', '--no-api-path',
                               '--no-decode-roofline', '--cpu-seconds', '2', shared=False, timeout=900)
    finally:
        if env_before is None:
            os.environ.pop('MTR_BENCH_FAIL_PROBE')
        else:
            os.environ['MTR_BENCH_FAIL_PROBE'] = env_before
    assert r.returncode == 0 and line is not None, r.stderr[-3000:]
    assert CONTRACT_KEYS <= set(line)
    assert line['roofline'] is not None and line['cpu_baseline'] is not None
    assert {'parity_error', 'pcie_inclusive_error', 'detector_pre_error'} <= set(line)
    assert line['parity'] is None
