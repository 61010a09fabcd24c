"""bench.py's command line, without a GPU: --full is offered next to the options the driver passes."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_the_driver_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    for opt in ("--full", "--gpus", "--steps", "--warmup", "--dump-outputs", "--no-cpu-baseline"):
        assert opt in p.stdout, opt
