"""bench.py --dump-outputs: what the timed path computed in its last step, written after the timed region, is the oracle's
result on the same seeded batch (so two builds of the project can be compared output for output), and --steps sets the
number of timed steps the line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_dumped_outputs_are_the_oracles(cuda, oracle, tmp_path):
    import bench
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    got = {name: np.load(os.path.join(tmp_path, name + ".npy")) for name in bench.DUMPED}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    xyz = S.sphere_clouds(bench.B, bench.N, 1000)                  # rank 0's batch of a weak run
    fps = oracle.farthest_point_sample(bench.M, xyz)
    new_xyz = oracle.gather_point(xyz, fps)
    idx, cnt = oracle.query_ball_point(bench.RADIUS, bench.NS, xyz, new_xyz)
    grouped = oracle.group_point(xyz, idx) - new_xyz[:, :, None, :]
    assert np.array_equal(got["fps_idx"], fps)
    assert np.array_equal(got["new_xyz"], new_xyz)
    assert np.array_equal(got["idx"], idx)
    assert np.array_equal(got["pts_cnt"], cnt)
    assert np.array_equal(got["grouped_xyz"], grouped)
