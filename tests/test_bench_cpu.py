"""CPU: bench.py's options and its --dump-outputs writer (the timed path itself needs the MI355X: tests/test_bench_gpu.py)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def test_dump_outputs_writes_float32_and_float64_npy(tmp_path):
    bench = _bench()
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), {"Jc": torch.tensor(1.5), "cs": torch.arange(7, dtype=torch.float32),
                                  "d": torch.arange(3, dtype=torch.float64), "k": np.array([1, 2, 3])})
    assert sorted(os.listdir(out)) == ["Jc.npy", "cs.npy", "d.npy", "k.npy"]
    jc, cs, d, k = (np.load(out / f"{n}.npy") for n in ("Jc", "cs", "d", "k"))
    assert jc.dtype == np.float32 and jc.shape == () and float(jc) == 1.5
    assert cs.dtype == np.float32 and np.array_equal(cs, np.arange(7, dtype=np.float32))
    assert d.dtype == np.float64 and k.dtype == np.float64 and np.array_equal(k, [1.0, 2.0, 3.0])


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    bench = _bench()
    big = torch.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="limit"):
        bench.dump_outputs(str(tmp_path / "dump"), {"big": big})
    assert not (tmp_path / "dump").exists()


def test_sample_rows_is_fixed_sorted_and_distinct():
    bench = _bench()
    a, b = bench.sample_rows(4096, 512), bench.sample_rows(4096, 512)
    assert np.array_equal(a, b) and len(np.unique(a)) == 512 and np.all(np.diff(a) > 0) and a[-1] < 4096
    assert np.array_equal(bench.sample_rows(100, 512), np.arange(100))


def test_options_are_listed_and_steps_must_be_positive():
    h = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout, h.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr[-2000:]
