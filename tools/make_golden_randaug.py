#!/usr/bin/env python3
"""Writes tests/golden/randaug_pil.npz: Pillow's result for what RandAugment adds to AutoAugment's ops.

CPU only, needs Pillow (the fixture was written with 12.2.0).  Inputs: a random image at 32x32x3, 24x40x3 and 24x40x1.
Per image: every geometric op with both filters at the level arguments of m = 0, 4.5, 9 and 10 (both signs above 0), a
rotation and a translate per axis that push most of the image out, SolarizeAdd at 0 / 99 / 128, Posterize at 0 and 4
bits, Solarize at the thresholds 0 and 256.  The fill is (124, 116, 104): not grey, so swapped channels show.  The level
arguments come from tests/randaug_ref.py, so the fixture pins the ops, not the level maps.

    python tools/make_golden_randaug.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import randaug_ref as R  # noqa: E402

FILL = (124, 116, 104)
RESAMPLE = {R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC}
FILTER_NAMES = {R.BILINEAR: "bilinear", R.BICUBIC: "bicubic"}


def to_pil(a):
    return Image.fromarray(a[:, :, 0], "L") if a.shape[2] == 1 else Image.fromarray(a, "RGB")


def from_pil(im, C):
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], C).copy()


def pil_op(a, name, value, filt=R.BILINEAR, fill=FILL):
    """The op as timm's auto_augment.py calls Pillow; `value` as tests/randaug_ref.level_arg returns it."""
    im = to_pil(a)
    kw = {"resample": RESAMPLE[filt], "fillcolor": tuple(fill) if a.shape[2] == 3 else int(fill[0])}
    if name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, (1, value, 0, 0, 1, 0), **kw)
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, value, 1, 0), **kw)
    elif name == "TranslateX":
        out = im.transform(im.size, Image.AFFINE, (1, 0, value, 0, 1, 0), **kw)
    elif name == "TranslateY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, value), **kw)
    elif name == "Rotate":
        out = im.rotate(value, **kw)
    elif name == "SolarizeAdd":
        lut = [min(255, i + value) if i < 128 else i for i in range(256)]
        out = im.point(lut * len(im.getbands()))
    elif name == "Posterize":
        out = ImageOps.posterize(im, value)
    elif name == "Solarize":
        out = ImageOps.solarize(im, value)
    else:
        raise ValueError(name)
    return from_pil(out, a.shape[2])


def images():
    g = np.random.default_rng(20241020)
    return {"rand_32x32": g.integers(0, 256, (32, 32, 3), dtype=np.uint8),
            "rand_24x40": g.integers(0, 256, (24, 40, 3), dtype=np.uint8),
            "rand_24x40x1": g.integers(0, 256, (24, 40, 1), dtype=np.uint8)}


def cases(H, W):
    """(key, op, raw argument, filter) of every fixture entry of an HxW image."""
    for name in R.GEOMETRIC:
        for filt in (R.BILINEAR, R.BICUBIC):
            for m in (0, 4.5, 9, 10):
                for neg in ((0,) if m == 0 else (0, 1)):
                    yield f"{name}/{FILTER_NAMES[filt]}/m{m}/{neg}", name, R.level_arg(name, m, neg, True, H, W), filt
    for filt in (R.BILINEAR, R.BICUBIC):
        for tag, name, value in (("far0", "Rotate", 77.7), ("far1", "Rotate", -98.6), ("far", "TranslateX", 0.9 * W + 0.3),
                                 ("far", "TranslateY", -(0.8 * H + 0.6))):
            yield f"{name}/{FILTER_NAMES[filt]}/{tag}", name, value, filt
    for add in (0, 99, 128):
        yield f"SolarizeAdd/{add}", "SolarizeAdd", add, R.BILINEAR
    for bits in (0, 4):
        yield f"Posterize/{bits}", "Posterize", bits, R.BILINEAR
    for th in (0, 256):
        yield f"Solarize/{th}", "Solarize", th, R.BILINEAR


def main():
    arrays = {}
    for tag, a in images().items():
        arrays[f"in/{tag}"] = a
        for key, name, value, filt in cases(a.shape[0], a.shape[1]):
            arrays[f"out/{tag}/{key}"] = pil_op(a, name, value, filt)
    path = os.path.join(ROOT, "tests", "golden", "randaug_pil.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "augment_pil.npz"))


if __name__ == "__main__":
    main()
