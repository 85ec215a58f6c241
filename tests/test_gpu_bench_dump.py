"""bench.py --dump-outputs: the file holds what the last timed step returned
(signal.data), bitwise the same from run to run; a large array is written as
a fixed sample of whole rows x columns.  A plain run (no --full) measures no
CPU baseline and no gpu_power."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sig:
    def __init__(self, data):
        self.data = data


@pytest.mark.gpu
def test_dump_outputs_whole_and_sample(hip_lib, tmp_path, monkeypatch):
    import torch
    import bench
    rows, n = 37, 1001
    full = torch.arange(rows * n, dtype=torch.float32, device="cuda").reshape(rows, n)   # value = row * n + col
    bench.dump_outputs(str(tmp_path / "whole"), _Sig(full), 0, 1)
    got = np.load(str(tmp_path / "whole" / "data.npy"))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, full.cpu().numpy())
    # above the size limit: DUMP_ROWS x DUMP_COLS distinct, sorted rows and columns
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_ROWS", 5)
    monkeypatch.setattr(bench, "DUMP_COLS", 64)
    bench.dump_outputs(str(tmp_path / "a"), _Sig(full), 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), _Sig(full), 1, 2)
    a = np.load(str(tmp_path / "a" / "data.npy"))
    b = np.load(str(tmp_path / "b" / "data_rank1.npy"))
    assert a.dtype == np.float32 and a.shape == (5, 64)
    np.testing.assert_array_equal(a, b)                     # the same sample every time
    r, c = (a // n).astype(int), (a % n).astype(int)
    assert (r == r[:, :1]).all() and (np.diff(r[:, 0]) > 0).all()
    assert (c == c[:1]).all() and (np.diff(c[0]) > 0).all()


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(hip_lib, tmp_path):
    nchan, log2n, steps, warmup = 7, 16, 2, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--nchan", str(nchan), "--log2n", str(log2n),
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["unit"] == "channel-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # (ms_per_step is rounded to 0.001 ms, value is not)
    assert line["value"] == pytest.approx(nchan * (1 << log2n) / (line["ms_per_step"] * 1e-3),
                                          rel=0.0006 / line["ms_per_step"] + 1e-6)
    assert line["cpu_baseline"] is None and line["cpu_baseline_allcore"] is None and line["gpu_power"] is None
    assert os.listdir(str(tmp_path / "out")) == ["data.npy"]
    got = np.load(str(tmp_path / "out" / "data.npy"))
    assert got.dtype == np.float32 and got.shape == (nchan, 1 << log2n)
    # the same calls in this process: seed, then warm-up + timed steps; the last one's data
    import bench
    import psrsigsim_amd as pss
    pss.seed(1776)
    with contextlib.redirect_stdout(sys.stderr):
        for _ in range(warmup + steps):
            sig = bench.c3_step(pss, nchan, (0, nchan), log2n)
    np.testing.assert_array_equal(got, sig.data.cpu().numpy())
