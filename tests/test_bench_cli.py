"""bench.py's own options: a plain run times the headline only, --full adds the extras after the timed region, --dump-outputs
writes what the last timed Loop returned (a fixed sample, under 64 MB, the same from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench      # noqa: E402


def _load_dump(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_is_a_fixed_sample_under_64_mb(tmp_path):
    n, d = bench.DUMP_STATE_ROWS + 12345, 64
    rng = np.random.default_rng(3)
    state, output = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((n, 2), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / 'a'), 30.0, state, output)
    bench.dump_outputs(str(tmp_path / 'b'), 30.0, state, output)
    a, b = _load_dump(tmp_path / 'a'), _load_dump(tmp_path / 'b')
    assert sorted(a) == ['iterations', 'output', 'state', 'state_rows']
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= 64 * 2 ** 20
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a['state_rows'].astype(np.int64)
    assert len(rows) == bench.DUMP_STATE_ROWS and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(a['state'], state[rows]) and np.array_equal(a['output'], output[rows]) and a['iterations'][0] == 30.0


def test_dump_outputs_keeps_every_row_of_a_small_graph(tmp_path):
    state, output = np.arange(40, dtype=np.float32).reshape(10, 4), np.ones((10, 2), np.float32)
    bench.dump_outputs(str(tmp_path), 7.0, state, output)
    z = _load_dump(tmp_path)
    assert np.array_equal(z['state'], state) and np.array_equal(z['output'], output) and np.array_equal(z['state_rows'], np.arange(10))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr


def _bench(args):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--nodes', '60000'] + args
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_full_run_dumps(tmp_path):
    plain = _bench(['--dump-outputs', str(tmp_path / 'plain')])
    assert plain['steps'] == 3 and plain['warmup'] == 1 and plain['value'] > 0 and plain['ms_per_step'] > 0
    assert plain['config']['iterations_per_step'] == 30.0 and plain['roofline']['avg_launch_ms'] > 0
    assert plain['parity_ok'] is None and 'cpu_baseline' not in plain and 'other_configs' not in plain['config']
    assert plain['config']['exact_f32_mfma_path'] is None and plain['config']['cold_aggregates_ms_per_step'] is None
    full = _bench(['--full', '--no-cpu-baseline', '--no-other-configs', '--dump-outputs', str(tmp_path / 'full')])
    assert full['config']['exact_f32_mfma_path']['ms_per_step'] > 0 and full['config']['cold_aggregates_ms_per_step'] > 0
    assert full['config']['pcie_inclusive_updates_per_s'] > 0
    a, b = _load_dump(tmp_path / 'plain'), _load_dump(tmp_path / 'full')
    assert sorted(a) == sorted(b) == ['iterations', 'output', 'state', 'state_rows']
    assert a['iterations'][0] == 30.0 and a['state'].shape == (60000, 64) and a['output'].shape == (60000, 2)
    assert np.isfinite(a['state']).all() and np.isfinite(a['output']).all()
    assert all(np.array_equal(a[k], b[k]) for k in a), 'same arguments, same inputs: the timed path must return the same values'
