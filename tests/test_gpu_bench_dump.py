"""bench.py --dump-outputs: two fresh child processes with the same arguments time exactly --steps steps, report
ms_per_step, and write the same float32 arrays (logits, loss, aux losses, gradient norm, weight sample) of their last
timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "micro", "--batch", "4",
           "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_are_written_and_reproducible(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = _bench(a)
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    _bench(b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"logits.npy", "loss.npy", "grad_norm.npy", "param_sample.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(a / "logits.npy").shape == (4, 100)
    assert np.load(a / "loss.npy").shape == ()
