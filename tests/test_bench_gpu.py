"""GPU: a plain `bench.py` line (the headline configuration, small batch) - the result fields, nothing of what `--full` adds, and
`--dump-outputs` writing the last timed step's results, equal to the same closed loop replayed in this process."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    steps, warmup, B = 3, 2, 64
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                          '--batch', str(B), '--dump-outputs', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == steps and line['warmup'] == warmup and line['unit'] == 'steps/s' and line['dtype'] == 'f64'
    assert line['higher_is_better'] is True and line['value'] > 0 and line['ms_per_step'] > 0
    assert abs(line['value'] - B * 1e3 / line['ms_per_step']) <= 1e-9 * line['value']
    assert 'cpu_baseline' not in line and 'settled_loop' not in line
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {'u0', 'status', 'iters', 'x_next', 'nlp_x', 'nlp_f'} <= set(got)
    assert all(a.dtype == np.float64 and a.shape[0] == B for a in got.values())
    assert np.all((got['status'] == 1) | (got['status'] == 2))
    # the same workload in this process: warm-up and timed steps, then the outputs of its last step
    dev = torch.device('cuda', 0)
    args = argparse.Namespace(batch=B, steps=steps, warmup=warmup, kf_steps=16, full=False)
    wl = bench.build_workload('C2', args, torch, dev, 0, 1)
    bench.timed_region(wl, warmup, steps, 1, dev)
    again = bench.dump_outputs(wl['outputs'](), str(tmp_path / 'again'))
    for p in again:
        np.testing.assert_allclose(np.load(p), got[os.path.basename(p)[:-4]], rtol=1e-12, atol=0)
