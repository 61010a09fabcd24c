#!/usr/bin/env python3
"""Writes tests/golden/affine_rows.npz: the parameter-table rows that `augment.op_row` (16.16 fixed point, the half-pixel
centre folded in) and `randaug.op_row` (fp64 pairs) write for every geometric op, at magnitude indices 0, 5 and 9, both
signs, and image sizes 32x32, 24x40 and 1x1 - the fixture that tests/test_stages_api.py holds the two functions to, so
that the affine arithmetic they share cannot move by a bit.  Needs the package only (no device, no built library).

cases int32 [N,5] = (AutoAugment's op id, magnitude index, sign, H, W); augment int32 [N, augment.ROW] and randaug int32
[N, randaug.ROW], row i belonging to cases[i].  AutoAugment's argument is `augment.magnitude`'s, RandAugment's is
`randaug.level_arg`'s with the increasing maps and the default translate_pct, filter "bilinear"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nvit_amd import augment, randaug  # noqa: E402

GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
MAGNITUDES = (0, 5, 9)
SIZES = ((32, 32), (24, 40), (1, 1))


def rows(case):
    op, m, sign, H, W = (int(v) for v in case)
    name = augment.OPS[op]
    return (augment.op_row(name, augment.magnitude(name, m, sign, W), H, W),
            randaug.op_row(name, randaug.level_arg(name, float(m), sign, True, H, W), "bilinear", H=H, W=W))


def main():
    cases = np.array([(augment.OPS.index(n), m, sg, H, W) for n in GEOMETRIC for m in MAGNITUDES for sg in (0, 1)
                      for H, W in SIZES], dtype=np.int32)
    aa, ra = zip(*(rows(c) for c in cases))
    path = os.path.join(ROOT, "tests", "golden", "affine_rows.npz")
    np.savez_compressed(path, cases=cases, augment=np.array(aa, dtype=np.int32), randaug=np.array(ra, dtype=np.int32))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
