#!/usr/bin/env python3
"""Writes tests/golden/center_crop_pil.npz: a few source images, the evaluation transform's geometry for each and what
Pillow makes of them, `Image.resize((W2, H2), BILINEAR | BICUBIC).crop((left, top, left + size, top + size))` - the
fixture that tests/test_center_crop_ref.py holds the numpy restatement tests/center_crop_ref.py to (Resize
+ CenterCrop).  Needs Pillow and numpy only.

The cases are the small pinned geometries of tests/center_crop_ref.py and its strong shrink, each with three channels
and with one.  Per case i: {i}_src uint8 [Hs,Ws,C], {i}_geom int [5] = (H2, W2, top, left, size), {i}_bilinear and
{i}_bicubic uint8 [size,size,C].  The images are patterns (ramps that wrap, a checkerboard of 8-pixel blocks, a
per-channel phase), so that the file stays small."""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from center_crop_ref import SMALL, STRONG_SHRINK, geometry  # noqa: E402

FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def pattern(Hs, Ws, C):
    y, x = np.mgrid[0:Hs, 0:Ws]
    chans = [((x // 8 + y // 8) % 2) * 180 + (x * (3 + c) + y * (5 - c) + 37 * c) % 76 for c in range(C)]
    return np.stack(chans, axis=2).astype(np.uint8)


def pil_resize_crop(src, H2, W2, top, left, size, resample):
    C = src.shape[2]
    im = Image.fromarray(src[:, :, 0] if C == 1 else src)
    return np.asarray(im.resize((W2, H2), resample).crop((left, top, left + size, top + size))).reshape(size, size, C)


def main():
    out, i = {}, 0
    for Hs, Ws, size, crop_pct in SMALL + [STRONG_SHRINK]:
        H2, W2, top, left = geometry(Hs, Ws, size, crop_pct)
        for C in (3, 1):
            src = pattern(Hs, Ws, C)
            out[f"{i}_src"], out[f"{i}_geom"] = src, np.array([H2, W2, top, left, size], dtype=np.int64)
            for name, resample in FILTERS.items():
                out[f"{i}_{name}"] = pil_resize_crop(src, H2, W2, top, left, size, resample)
            i += 1
    out["n_cases"] = np.int64(i)
    path = os.path.join(ROOT, "tests", "golden", "center_crop_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
