"""End-to-end rehearsal of ``bench.py`` at N>1 on the one GPU of a test box.

The driver runs ``torch.distributed.run --nproc-per-node N bench.py --gpus N`` on a whole node; nothing
of that path (rendezvous, slab split, ZSlabOp Function, barrier + max-over-ranks timing, the JSON line)
may first execute there. Two ranks share cuda:0 over ``gloo`` (RCCL refuses two ranks on one device);
the launcher is a fresh child process, never an exec of this (GPU-initialised) interpreter. The rehearsal runs
``--full`` (secondary workload, CPU baseline); a plain one-GPU run with ``--dump-outputs`` is checked on its own.
"""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.parametrize('nproc,workload', [(2, 'diffusion7_f32'), (2, 'stencil27_f16')])
def test_bench_two_ranks_end_to_end(nproc, workload):
    env = dict(os.environ, PSAD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.join(ROOT, 'bench.py'), '--gpus', str(nproc), '--edge', '128', '--steps', '3', '--warmup', '1',
           '--workload', workload, '--cpu-seconds', '1', '--secondary-edge', '96', '--full']
    t0 = time.perf_counter()
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    assert res['n_gpus'] == nproc
    assert res['config']['decomposition'] == f'z-slab x{nproc}'
    assert res['steps'] == 3 and res['value'] > 0
    assert res['ms_per_step'] * res['steps'] / 1e3 <= wall
    assert res['value'] == pytest.approx(128 ** 3 * 3 / (res['ms_per_step'] * 3 / 1e3) / 1e6, rel=1e-3)
    assert res['config']['name'] == workload
    assert res['metric'].endswith('128^3') and ('27-point fp16' in res['metric']) == (workload == 'stencil27_f16')
    rl = res['roofline']
    bpc = 8 if workload == 'diffusion7_f32' else 4
    assert rl['bytes_per_launch'] == bpc * 64 * 128 * 128 and rl['bytes_per_step'] == 2 * bpc * 128 ** 3
    # frac is the step-level figure: both sweeps' algorithmic bytes / ms_per_step / (N x peak)
    step_frac = 2 * bpc * 128 ** 3 / (res['ms_per_step'] * 1e-3) / 1e9 / (rl['peak'] * nproc)
    assert rl['frac'] == pytest.approx(step_frac, rel=1e-2) and rl['frac_fwd'] > 0 and rl['frac_bwd'] > 0
    assert rl['traffic'] is None            # no PMC entry for a slab-shaped launch: never the 1-GPU figure
    # rank 0 times the CPU path after the timed loop at every N (north_star: "in the same run")
    if workload == 'diffusion7_f32':            # config 5 timed in the same run (the driver's scaling runs)
        sec = res['secondary']
        assert sec['name'] == 'stencil27_f16' and sec['n_gpus'] == nproc and sec['value'] > 0
        assert sec['decomposition'] == f'z-slab x{nproc}' and sec['cells'] == 96 ** 3
    else:
        assert 'secondary' not in res
    cpu = res['cpu_baseline']
    assert cpu is not None and cpu['value'] > 0 and cpu['cores'] == 1 and cpu['kind'] == 'port', cpu


def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    """A plain run (no ``--full``) times only the headline workload — no secondary workload, CPU baseline or
    default-engine rerun — and ``--dump-outputs`` writes the last timed step's output and gradient: float32, a seeded
    sample (192^3 cells > ``DUMP_ELEMS``), equal to the float64 oracle on the same seeded inputs at smoke()'s bound."""
    import numpy as np
    import torch

    import bench
    from oracle import stencils as S
    n = 192
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--edge', str(n), '--steps', '2',
           '--warmup', '1', '--dump-outputs', str(tmp_path / 'dump')]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    assert res['full'] is False and 'secondary' not in res and res['cpu_baseline'] is None
    assert 'value_default_engine' not in res
    assert res['steps'] == 2 and res['warmup'] == 1 and res['n_gpus'] == 1
    assert res['unit'] == 'Mcells/s' and res['higher_is_better'] is True and res['dtype'] == 'f32'
    assert res['value'] == pytest.approx(n ** 3 / (res['ms_per_step'] / 1e3) / 1e6, rel=1e-3)
    assert sorted(os.listdir(tmp_path / 'dump')) == ['diffu.npy', 'out.npy']
    got = {k: np.load(tmp_path / 'dump' / f'{k}.npy') for k in ('out', 'diffu')}
    assert sum(a.nbytes for a in got.values()) <= 64e6

    # the inputs of bench.py's rank 0 and its sample of the cells
    g = torch.Generator(device='cuda').manual_seed(0)
    u = torch.rand((n, n, n), generator=g, device='cuda', dtype=torch.float32).cpu().numpy()
    g1 = torch.Generator(device='cuda').manual_seed(1000)
    d = (torch.rand((n, n, n), generator=g1, device='cuda', dtype=torch.float32) * 2 - 1).cpu().numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n ** 3, size=bench.DUMP_ELEMS))
    taps = S.taps_diffusion_7pt()
    for name, ref in (('out', S.linear_stencil(u, taps)), ('diffu', S.linear_stencil(d, S.flip(taps)))):
        a = got[name]
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_ELEMS,), (name, a.dtype, a.shape)
        err = float(np.max(np.abs(a.astype(np.float64) - ref.reshape(-1)[idx])))
        tol = 1e-6 * float(np.max(np.abs(ref)))
        assert err <= tol, f'{name}: max err {err:.3e} > {tol:.3e}'
