"""GPU: bench.py's plain run at a small shape. The line carries the headline keys for exactly --steps timed steps and nothing the
plain run does not measure (the probe, rooflines, other legs and the CPU baseline are --full only); --dump-outputs writes the last
timed step's loss sums, gradient and parameter samples as float32 / float64 .npy files that agree with the line's train_loss."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_its_last_step(tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '2', '--layers', '2', '--hs', '256',
                        '--ffn', '512', '--heads', '4', '--seq', '256', '--batch', '2', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['steps'] == 3 and rec['warmup'] == 2 and rec['ms_per_step'] > 0 and rec['value'] > 0
    assert rec['unit'] == 'tokens/s' and rec['higher_is_better'] is True and rec['dtype'] == 'bf16'
    assert not {'roofline', 'roofline_secondary', 'cpu_baseline', 'padded_step', 'decode'} & set(rec)

    files = sorted(os.listdir(out))
    assert files == ['grad_sample.npy', 'loss_sums.npy', 'param_sample.npy'], files
    arrays = {f: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    s = arrays['loss_sums.npy']
    assert s.shape == (24,) and (s[8:16] > 0).all()
    w8 = np.array([262, 134, 262, 134, 38, 135, 55, 260], dtype=np.float64)
    assert abs(float(((s[0:8] / s[8:16]) * w8).sum() / w8.sum()) - rec['train_loss']) < 1e-9 * abs(rec['train_loss'])
    g, p = arrays['grad_sample.npy'], arrays['param_sample.npy']
    assert g.shape == p.shape and g.ndim == 1 and g.size > 0 and np.abs(g).max() > 0
