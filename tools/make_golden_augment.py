#!/usr/bin/env python3
"""Writes tests/golden/augment_pil.npz: Pillow's result for every AutoAugment op.

CPU only, needs Pillow (the fixture was written with 12.2.0).  Inputs: a random and a low-contrast image at 32x32x3 and
24x40x3, a random 24x40x1, and a 32x32x3 image whose middle channel is constant.  For every op: magnitude indices 0, 4
and 9 and both signs (one call for ops without a magnitude, three for the unsigned ones).  The magnitudes come from
tests/augment_ref.py, so the fixture pins the ops, not the magnitude table.

    python tools/make_golden_augment.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref as R  # noqa: E402


def to_pil(a):
    return Image.fromarray(a[:, :, 0], "L") if a.shape[2] == 1 else Image.fromarray(a, "RGB")


def from_pil(im, C):
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], C).copy()


def pil_op(a, name, value):
    """The op through Pillow's own entry points; `value` as tests/augment_ref.magnitude returns it."""
    im = to_pil(a)
    if name == "Identity":
        out = im.copy()
    elif name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, (1, value, 0, 0, 1, 0))
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, value, 1, 0))
    elif name == "TranslateX":
        out = im.transform(im.size, Image.AFFINE, (1, 0, value, 0, 1, 0))
    elif name == "TranslateY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, value))
    elif name == "Rotate":
        out = im.rotate(value)
    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
        out = getattr(ImageEnhance, name)(im).enhance(value)
    elif name == "Posterize":
        out = ImageOps.posterize(im, value)
    elif name == "Solarize":
        out = ImageOps.solarize(im, value)
    elif name == "AutoContrast":
        out = ImageOps.autocontrast(im)
    elif name == "Equalize":
        out = ImageOps.equalize(im)
    elif name == "Invert":
        out = ImageOps.invert(im)
    else:
        raise ValueError(name)
    return from_pil(out, a.shape[2])


def images():
    g = np.random.default_rng(20240607)
    out = {}
    for tag, (H, W) in (("32x32", (32, 32)), ("24x40", (24, 40))):
        out[f"rand_{tag}"] = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out[f"low_{tag}"] = (g.integers(100, 140, (H, W, 3)) + np.array([0, 20, -30])).astype(np.uint8)
    out["rand_24x40x1"] = g.integers(0, 256, (24, 40, 1), dtype=np.uint8)
    c = g.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    c[:, :, 1] = 77
    out["const_32x32"] = c
    return out


def cases():
    for name in R.OPS:
        if name not in R.HAS_MAGNITUDE:
            yield name, 0, 0
            continue
        for m in (0, 4, 9):
            for sign in ((0, 1) if name in R.SIGNED else (0,)):
                yield name, m, sign


def main():
    arrays = {}
    for tag, a in images().items():
        arrays[f"in/{tag}"] = a
        for name, m, sign in cases():
            arrays[f"out/{tag}/{name}/{m}/{sign}"] = pil_op(a, name, R.magnitude(name, m, sign, a.shape[1]))
    path = os.path.join(ROOT, "tests", "golden", "augment_pil.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
