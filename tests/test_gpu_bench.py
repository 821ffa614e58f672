"""-m gpu: a plain `bench.py` run (no --full) times exactly --steps steps, carries none of the --full legs, and its
--dump-outputs arrays are the same from run to run (the seeded inputs and weights do not change between processes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "4", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_times_steps_and_dumps_the_same_outputs_every_run(dev, tmp_path):
    recs = [_plain_run(tmp_path / f"run{i}") for i in range(2)]
    for rec in recs:
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "pairs/s"
        assert rec["config"]["windows"]["n"] == 1 and rec["config"]["windows"]["steps_per_window"] == 3
        assert not {"roofline", "knn", "train", "vox", "netvlad", "cpu_baseline", "reference_deps"} & set(rec)
        assert rec["config"]["replay_equals_eager"] is None and rec["config"]["ms_per_step_one_in_flight"] is None
    for name in ("query_embedding", "database_embedding"):
        a, b = (np.load(tmp_path / f"run{i}" / f"{name}.npy") for i in range(2))
        assert a.dtype == np.float32 and a.shape[0] == 4 and np.isfinite(a).all() and np.abs(a).sum() > 0
        assert np.array_equal(a, b), name
