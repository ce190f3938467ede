"""bench.py as it is run for every change: a plain run (set-up, warm-up, one timed block of exactly --steps steps, the line) with
--dump-outputs, in a fresh child process; what it wrote is what the timed path computes for the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 40 and line["warmup"] == 5 and line["repeats"] == 1 and line["higher_is_better"] is True
    assert line["value"] > 1e6 and 0 < line["ms_per_step"] < 10.0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 512) < 1e-3 * 512           # B evaluations a step
    for k in ("cpu_baseline", "also_measured", "end_to_end", "roofline", "kernels_us"):   # --full's, not a plain run's
        assert k not in line, k
    assert sorted(os.listdir(out)) == ["lnl.npy"]
    got = np.load(out / "lnl.npy")
    assert got.dtype == np.float64 and got.shape == (512,) and np.isfinite(got).sum() >= 508

    import torch
    import bench
    P = bench.make_problem("C2", 512, 0, 0)
    eng = P["engines"][0]
    eng.lnlike_batch(P["theta"], out=P["lnl"])
    torch.cuda.synchronize()
    ref = P["lnl"].cpu().numpy()
    eng.close()
    assert np.array_equal(got, ref, equal_nan=True), np.nanmax(np.abs(got - ref))
