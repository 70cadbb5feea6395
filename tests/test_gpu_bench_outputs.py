"""GPU tier: bench.py --dump-outputs on the real headline GEMM. The inputs come from fixed seeds, so two runs -- with
different step counts -- write the same output of the last timed step; the file is float32, within the 64 MB budget, and
the result line reports the steps it was given and the time of one of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(out_dir, steps):
    env = dict(os.environ)
    for k in ("QNNP_BENCH_STUB", "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--no-extra",
                          "--no-cpu-baseline", "--full-out", "", "--dump-outputs", str(out_dir)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.rstrip().splitlines()[-1])


def test_bench_dumps_the_same_gemm_output_in_every_run(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    first, second = _bench(tmp_path / "a", 3), _bench(tmp_path / "b", 7)
    assert first["steps"] == 3 and second["steps"] == 7
    assert first["ms_per_step"] > 0 and second["ms_per_step"] > 0
    assert os.listdir(tmp_path / "a") == os.listdir(tmp_path / "b") == ["q8gemm_output.npy"]
    path = tmp_path / "a" / "q8gemm_output.npy"
    assert os.path.getsize(path) <= bench.DUMP_MAX_BYTES
    a, b = np.load(path), np.load(tmp_path / "b" / "q8gemm_output.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ROWS, 4096)
    assert np.array_equal(a, b)
    # uint8 values inside the GEMM's clamp [1, 254] (bench/q8gemm.cc:103), and a real spread of them
    assert np.array_equal(a, np.round(a)) and a.min() >= 1 and a.max() <= 254
    assert len(np.unique(a)) > 64
