"""bench.py without --full: the headline run alone (no legs of their own after the timed steps), and --dump-outputs writes what the
last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    dump = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--settle', '1',
           '--dump-outputs', str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert list(d)[:7] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step"]
    assert d['steps'] == 3 and d['warmup'] == 1 and d['unit'] == 'mel-frames/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['ms_per_step'] > 0
    assert abs(d['value'] - d['config']['frames_per_step'] / (d['ms_per_step'] * 1e-3)) < 1e-3 * d['value']
    for k in ('roofline', 'decode', 'frontend', 'secondary', 'cpu_baseline', 'graph_vs_eager_ms'):
        assert k not in d, k
    files = sorted(os.listdir(dump))
    for name in ('loss', 'recon_loss', 'kl_loss', 'kl_weight', 'grad_norm', 'bn_running_stats', 'params_sample',
                 'grads_sample'):
        assert name + '.npy' in files, (name, files)
    arrs = {f[:-4]: np.load(os.path.join(dump, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 1024 * 1024
    assert all(np.isfinite(a).all() for a in arrs.values())
    assert abs(float(arrs['loss'][0]) - d['final_loss']) <= 1e-5 * max(1.0, abs(d['final_loss']))
    assert arrs['params_sample'].size == arrs['grads_sample'].size > 1000000
    assert np.abs(arrs['grads_sample']).max() > 0
