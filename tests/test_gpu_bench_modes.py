"""bench.py: a plain run prints the headline and the figures of its own timed region only; --full adds the per-family
kernel breakdown, the stand-alone renorm timing, parity against the exact-f32 mode and the CPU oracle baseline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernel_ms_per_step", "hbm_kernels", "family_breakdown_from", "parity", "cpu_baseline")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "micro", "--batch", "4",
           "--steps", "2", "--warmup", "1", *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_reports_its_timed_region_only():
    res = _bench()
    for k in HEADLINE:
        assert k in res, k
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "images/sec" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["timed_with_event_profiling"] == "gemm_nt launches only"
    assert res["roofline"]["launches"] > 0 and "families" not in res["roofline"]
    for k in FULL_ONLY:
        assert k not in res, k


def test_full_run_adds_breakdown_parity_and_cpu_baseline():
    res = _bench("--full")
    for k in HEADLINE + FULL_ONLY:
        assert k in res, k
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["roofline"]["families"] and res["roofline"]["weakest_family"] in res["roofline"]["families"]
    assert res["kernel_ms_per_step"]["gemm_nt"] > 0
    assert "renorm_standalone" in res["hbm_kernels"]
    assert res["parity"]["max_abs"] < 1e-2
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["c1_tiny"]["value"] > 0
    assert "cpu_baseline" not in _bench("--full", "--no-cpu-baseline")
