"""bench.py --dump-outputs on the GPU: a run writes what its last timed step computed, the same arrays for the same arguments,
and --steps decides which step that is (the resident batches are cycled and each brings its own boxes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(tmp_path, tag, steps):
    d = tmp_path / tag
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LPF_LIBRARY")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--points", "200000",
                        "--frames", "2", "--buffers", "2", "--preheat-ms", "0", "--no-cpu", "--no-secondary", "--no-events",
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps
    files = sorted(os.listdir(d))
    assert files and all(f.endswith(".npy") for f in files)
    return {f[:-4]: np.load(d / f) for f in files}


@pytest.mark.gpu
def test_bench_dump_outputs_is_reproducible_and_follows_steps(tmp_path):
    a = _run(tmp_path, "a", 3)
    b = _run(tmp_path, "b", 3)
    c = _run(tmp_path, "c", 4)
    assert sorted(a) == sorted(b) == sorted(c)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["n_valid"].shape == (2,) and a["count_mb"].shape == (8 * 2 * 32,) and a["u_sample"].size == 2 * 200000
    assert all(v.any() for v in a.values()), [k for k, v in a.items() if not v.any()]
    # step 3 ran on batch 0, step 4 on batch 1: the same clouds (permuted) with other boxes
    assert np.array_equal(a["n_valid"], c["n_valid"])
    assert not np.array_equal(a["count_mb"], c["count_mb"])
