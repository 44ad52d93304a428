"""bench.py on the GPU, end to end, at the smallest BASELINE configuration: a plain run prints the headline line and nothing that
takes runs of its own; --full adds the CPU baseline (the extra legs belong to the default workload only)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ, SARAGAN_BENCH_NO_SETTLE='1')      # (the settle steps are for the board, not for this test)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', '1', '--steps', '3',
                        '--warmup', '2'] + list(args), capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only():
    rec = _bench()
    assert rec['value'] > 0 and rec['ms_per_step'] > 0 and rec['unit'] == 'volumes/s' and rec['higher_is_better'] is True
    assert rec['metric'].startswith('3D volumes/sec/node') and rec['dtype'] == 'f32'
    assert (rec['n_gpus'], rec['steps'], rec['warmup']) == (1, 3, 2)
    assert 'extras' not in rec and 'cpu_baseline' not in rec


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline():
    rec = _bench('--full', '--cpu-budget-s', '0.5')
    assert rec['value'] > 0 and 'extras' not in rec
    assert rec['cpu_baseline']['value'] > 0 and rec['cpu_baseline']['kind'] == 'port'
