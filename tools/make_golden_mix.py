#!/usr/bin/env python3
"""Writes tests/golden/beta_quantiles.npz: scipy's Beta(alpha, alpha) quantiles at k/1024, k = 0..1024, in fp64, for the
alphas that tests/test_mix_ref.py holds nvit_amd.mix.beta_quantile_table to (Mixup / CutMix).

CPU only, needs scipy (the fixture was written with 1.15.3); the product itself never imports scipy.

    python tools/make_golden_mix.py
"""
import os

import numpy as np
from scipy.special import betaincinv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS = (0.1, 0.2, 0.8, 1.0, 4.0)
KNOTS = 1024


def main():
    p = np.arange(KNOTS + 1, dtype=np.float64) / KNOTS
    arrays = {"alphas": np.array(ALPHAS), "p": p}
    for a in ALPHAS:
        arrays[f"q/{a}"] = betaincinv(a, a, p)
    path = os.path.join(ROOT, "tests", "golden", "beta_quantiles.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
