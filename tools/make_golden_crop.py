#!/usr/bin/env python3
"""Writes tests/golden/crop_pil.npz: a few source images, crop boxes and what Pillow makes of them,
`Image.crop(box).resize((size, size), BILINEAR | BICUBIC)` - the fixture that tests/test_crop_ref.py holds the numpy
restatement tests/crop_ref.py to (RandomResizedCrop).  Needs Pillow and numpy only.

Per case i: {i}_src uint8 [Hs,Ws,C], {i}_size, {i}_boxes int [n,4] = (top, left, h, w), {i}_bilinear and {i}_bicubic
uint8 [n,size,size,C].  The images are patterns (ramps that wrap, a checkerboard of 8-pixel blocks, a per-channel
phase), so that the file stays small."""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Hs, Ws, C, size, boxes)
CASES = [
    (24, 40, 3, 16, [(0, 0, 24, 40), (5, 7, 1, 1), (3, 0, 1, 40), (0, 9, 24, 1), (0, 0, 10, 15), (14, 25, 10, 15),
                     (0, 30, 24, 10), (4, 6, 13, 21)]),
    (24, 40, 1, 16, [(0, 0, 24, 40), (5, 7, 1, 1), (3, 0, 1, 40), (0, 9, 24, 1), (14, 25, 10, 15), (4, 6, 13, 21)]),
    (9, 7, 3, 16, [(0, 0, 9, 7), (2, 1, 5, 4), (8, 6, 1, 1)]),              # upscale
    (16, 16, 3, 16, [(0, 0, 16, 16), (3, 3, 8, 8)]),                       # the identity, and a 2x upscale
    (5, 33, 3, 8, [(0, 0, 5, 33), (1, 4, 3, 20)]),
    (1, 1, 3, 8, [(0, 0, 1, 1)]),
    (64, 64, 3, 8, [(0, 0, 64, 64), (7, 0, 50, 64)]),                      # 8x downscale: 17 and 33 taps
    (256, 256, 3, 224, [(16, 8, 230, 240)]),
]
FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def pattern(Hs, Ws, C):
    y, x = np.mgrid[0:Hs, 0:Ws]
    block = 8
    if Hs >= 128:   # the large case: flat 32-pixel blocks with steps between them (its outputs are most of the file)
        block = 32
        y, x = y // block * block, x // block * block
    chans = [((x // block + y // block) % 2) * 180 + (x * (3 + c) + y * (5 - c) + 37 * c) % 76 for c in range(C)]
    return np.stack(chans, axis=2).astype(np.uint8)


def pil_crop_resize(src, box, size, resample):
    top, left, h, w = box
    C = src.shape[2]
    im = Image.fromarray(src[:, :, 0] if C == 1 else src)
    return np.asarray(im.crop((left, top, left + w, top + h)).resize((size, size), resample)).reshape(size, size, C)


def main():
    out = {}
    for i, (Hs, Ws, C, size, boxes) in enumerate(CASES):
        src = pattern(Hs, Ws, C)
        out[f"{i}_src"], out[f"{i}_size"], out[f"{i}_boxes"] = src, np.int64(size), np.array(boxes, dtype=np.int64)
        for name, resample in FILTERS.items():
            out[f"{i}_{name}"] = np.stack([pil_crop_resize(src, box, size, resample) for box in boxes])
    out["n_cases"] = np.int64(len(CASES))
    path = os.path.join(ROOT, "tests", "golden", "crop_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
