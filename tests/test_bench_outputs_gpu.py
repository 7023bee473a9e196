"""bench.py's plain run and --dump-outputs: the one JSON line carries the headline and none of --full's extras, the last
timed step's results land in DIR/<name>.npy (float32 / float64, within the size limit, large tensors as a fixed sample),
and a second run with the same arguments writes the same arrays bit for bit (seeded inputs, bitwise reproducible step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
ARGS = ['--steps', '3', '--warmup', '2', '--batch', '1', '--size', '64', '--grid', '4']


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, BENCH] + ARGS + ['--dump-outputs', str(out_dir)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    arrays = {f[:-len('.npy')]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    from bench import DUMP_SAMPLE
    from oracle import wesup_oracle as orc
    line, arrays = _run(tmp_path / 'a')
    assert line['steps'] == 3 and line['warmup'] == 2 and line['n_gpus'] == 1
    assert line['unit'] == 'images/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['value'] > 0 and abs(line['value'] * line['ms_per_step'] - 1e3) <= 2e-3 * 1e3      # batch 1: images/s = 1000 / ms
    for extra in ('roofline', 'roofline_step', 'kernels', 'cpu_baseline'):
        assert extra not in line, extra
    assert line['box'] is None and line['ms_per_step_median'] is None

    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays['loss'][0]) == line['config']['last_loss']
    weights = orc.make_weights(0, feat_scale=0.05)
    for name, w in weights.items():
        for prefix in ('param', 'grad'):
            a = arrays[f'{prefix}.{name}']
            assert a.shape == (min(w.size, DUMP_SAMPLE),) and np.isfinite(a).all(), (prefix, name)
    # the parameters written are the updated ones: the SGD steps moved the seeded start
    assert not np.array_equal(arrays['param.classifier.0.weight'], weights['classifier.0.weight'].reshape(-1))

    _, again = _run(tmp_path / 'b')
    assert sorted(again) == sorted(arrays)
    for k, a in arrays.items():
        assert np.array_equal(a, again[k]), k
