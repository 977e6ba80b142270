"""bench.py's command line on the GPU: a plain run (its own process, a small box) prints one JSON
line with the headline fields and none of the --full legs, times exactly --steps steps, and
--dump-outputs writes the state after warm-up + timed steps -- bit for bit what the same model gives
when stepped in this process (fp64, the reference's order: no tolerance)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 300, 5, 2


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--n", str(N), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "cell-updates/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N * N / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert "cpu_baseline" not in d and "multi_gpu_parity_512" not in d
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in bench.DUMP_FIELDS)

    import ocean_model_arch_amd as amd
    m = amd.OceanModel(amd.BasinConfig(nx=N + 4, ny=N + 4), amd.SWConfig(), amd.ParallelConfig(1, 1), device=0)
    m.init().step(WARMUP + STEPS).synchronize()
    try:
        for f in bench.DUMP_FIELDS:
            got, ref = np.load(out / (f + ".npy")), m.download(0, f)
            assert got.dtype == np.float64 and got.shape == (N + 4, N + 4)
            assert got.tobytes(order="F") == ref.tobytes(order="F"), f
    finally:
        m.close()
