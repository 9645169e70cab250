"""bench.py as the driver runs it: a plain run prints the headline figure and nothing measured beside it, and
--dump-outputs writes what the last timed step computed - on a small sequence, every position against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(sm, oracle, gpu, tmp_path):
    n, steps = 3_000_000, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--bases", str(n), "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Gbases/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    for key in ("extra", "cpu_baseline", "median_of_5", "end_to_end"):
        assert key not in line, key  # measured with --full only

    files = sorted(os.listdir(tmp_path))
    assert files == ["block_sums.npy", "count.npy", "positions.npy"]
    arrays = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    # the headline workload: canonical k=21 w=11 on generator G seed 3 (fewer positions than the sample: all of them)
    want = oracle.run(oracle.gen_packed(3, n), n, 21, 11, canonical=True).astype(np.float64)
    assert arrays["count"].tolist() == [len(want)]
    assert np.array_equal(arrays["positions"], want)
    block = 1 << 16
    padded = np.concatenate([want, np.zeros(-len(want) % block)])
    assert np.array_equal(arrays["block_sums"], padded.reshape(-1, block).sum(axis=1))
