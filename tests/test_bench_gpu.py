"""GPU: bench.py's plain line and --dump-outputs, each run in a fresh child process (never re-executed from a process that has touched the GPU)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_line_and_its_dumped_outputs(tmp_path):
    """a plain run: the headline line without the --full legs; --dump-outputs gives the last timed step's Jc and costs, the same from run to run"""
    dumps = []
    for i in range(2):
        line = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"d{i}")])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "roofline"):
            assert k in line
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert "cpu_baseline" not in line and "other_workloads" not in line["config"]
        jc, cs = np.load(tmp_path / f"d{i}" / "Jc.npy"), np.load(tmp_path / f"d{i}" / "cs.npy")
        assert jc.dtype == np.float32 and jc.shape == () and cs.dtype == np.float32 and cs.shape == (7,)
        assert float(jc) == line["config"]["Jc"] and np.all(np.isfinite(cs))
        dumps.append((jc, cs))
    np.testing.assert_allclose(dumps[0][0], dumps[1][0], rtol=1e-6)
    np.testing.assert_allclose(dumps[0][1], dumps[1][1], rtol=1e-6)


def test_shock_sweep_dump(tmp_path):
    line = _run(["--workload", "singlequad-shock", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    z = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(z) == ["costs1", "costs2", "ctrl", "nShock", "traj", "x_shocked"]
    assert sum(a.nbytes for a in z.values()) <= 64 << 20
    assert z["traj"].shape[:3] == (9, 512, 12) and z["ctrl"].shape[:2] == (9, 512) and z["costs2"].shape == (9, 8)
    assert float(z["costs2"][-1, 0]) == line["config"]["Jc_last_segment"]
    assert all(np.all(np.isfinite(a)) for a in z.values())
