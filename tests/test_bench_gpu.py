"""bench.py's plain run on the GPU: one line with the headline fields, `steps` = --steps, nothing of --full in it, and
--dump-outputs writing the same arrays on two runs with the same arguments (same seeded inputs, a bit-reproducible step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode, expect", [("train", {"logits.npy", "preds.npy", "ce.npy", "reg.npy", "grad_bufs_0.npy", "encoder_state.npy", "head_state.npy"}),
                                          ("fps", {"indices.npy"})])
def test_plain_run_line_and_dumped_outputs(tmp_path, mode, expect):
    dirs = [tmp_path / "run0", tmp_path / "run1"]
    for d in dirs:
        line = _bench("--mode", mode, "--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "roofline" not in line and "cpu_baseline" not in line            # --full only
    names = set(os.listdir(dirs[0]))
    assert expect <= names and names == set(os.listdir(dirs[1]))
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64_000_000
    for n in sorted(names):
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), f"{n} differs between two runs with the same arguments"
