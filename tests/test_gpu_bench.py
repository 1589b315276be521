"""bench.py's plain run on the device: the headline steps only, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch', '8', '--steps', '2', '--warmup', '1',
           '--dump-outputs', str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['steps'] == 2 and line['ms_per_step'] > 0 and line['value'] > 0 and line['dtype'] == 'f32'
    assert line['sustained'] is None and line['cpu_baseline'] is None and line['roofline'] is None and line['small_batch'] is None
    got = {p.name[:-4]: np.load(p) for p in tmp_path.glob('*.npy')}
    assert {'record', 'smpl_vertices', 'smpl_joints3d', 'smpl_joints2d', 'pred_cam_t', 'cam_vfov'} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert got['smpl_vertices'].shape == (8, 6890, 3) and got['record'].shape[0] == 8
    np.testing.assert_array_equal(got['record'][:, :6890 * 3].reshape(8, 6890, 3), got['smpl_vertices'])
