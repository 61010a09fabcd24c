"""numpy restatement of the on-device Resize + CenterCrop for evaluation batches: timm's
`transforms_imagenet_eval` geometry, the window of Pillow's two-pass 8-bit resample, and ToTensor + Normalize with the
kernel's roundings.

Independent of nvit_amd/crop.py and of the kernels on purpose: the GPU tests compare both against this file, and
tests/test_center_crop_ref.py holds this file to Pillow (`Image.resize((W2, H2), f).crop(window)`).  The resampler is
crop_ref's: a window of the resized image is the whole pass with only the window's outputs kept."""
import math
import os

import numpy as np

from crop_ref import FILTERS, resample_axis, taps

# (Hs, Ws, size, crop_pct) -> (H2, W2, top, left): the pinned geometries; two of them round a half to even
PINNED = [
    ((256, 256, 224, 0.875), (256, 256, 16, 16)),
    ((37, 53, 24, 0.875), (27, 38, 2, 7)),      # 1.5 -> 2
    ((53, 37, 24, 0.9), (37, 26, 6, 1)),        # 6.5 -> 6
    ((64, 48, 20, 0.8), (33, 25, 6, 2)),
    ((300, 200, 64, 0.95), (100, 67, 18, 2)),
    ((32, 32, 32, 0.875), (36, 36, 2, 2)),      # enlarging
    ((32, 32, 32, 1.0), (32, 32, 0, 0)),        # the identity resize
]
SMALL = [case for case, _ in PINNED if case[0] < 256]   # what the fixture holds; 256x256 is held to live Pillow
STRONG_SHRINK = (300, 200, 8, 1.0)                       # -> (12, 8, 2, 0): a tap set longer than a 16-wide tile


def half_up(x):
    """floor(x + 1/2): the rounding that center_crop does not use."""
    return math.floor(x + 0.5)


def geometry(Hs, Ws, size, crop_pct, crop_mode="center", rounding=round):
    """(H2, W2, top, left): Resize(floor(size / crop_pct)) of the shorter side (torchvision: the longer one is int(scale *
    long / short)) or, "squash", of both; then center_crop's corner, int(round((H2 - size) / 2.0)) with Python's round."""
    scale = math.floor(size / crop_pct)
    if crop_mode == "squash":
        H2 = W2 = scale
    elif Ws <= Hs:
        H2, W2 = int(scale * Hs / Ws), scale
    else:
        H2, W2 = scale, int(scale * Ws / Hs)
    return H2, W2, int(rounding((H2 - size) / 2.0)), int(rounding((W2 - size) / 2.0))


def window(u8, H2, W2, top, left, size, interpolation):
    """What nvit_center_crop_apply writes as uint8: u8 [B,Hs,Ws,C] -> [B,size,size,C].  The whole image is resampled
    horizontally to W2 and the window's columns are kept, then vertically to H2 and the window's rows are kept."""
    u8 = np.asarray(u8, dtype=np.uint8)
    B, _, _, C = u8.shape
    out = np.empty((B, size, size, C), np.uint8)
    for b in range(B):
        mid = resample_axis(u8[b], W2, interpolation)[:, left:left + size, :]                  # [Hs, size, C]
        res = resample_axis(mid.transpose(1, 0, 2), H2, interpolation).transpose(1, 0, 2)      # [H2, size, C]
        out[b] = res[top:top + size]
    return out


def rows_read(Hs, H2, top, size, interpolation):
    """(first, count) of the source rows that the vertical taps of the window's rows read: what the horizontal pass
    visits and the intermediate holds."""
    ymins, counts, _ = taps(Hs, H2, interpolation)
    first = int(ymins[top:top + size].min())
    return first, int((ymins + counts)[top:top + size].max()) - first


def workspace_bytes(B, Hs, Ws, C, H2, W2, top, left, size, interpolation):
    """nvit_center_crop_ws_bytes: per axis B x size tap sets of 2 + ksize ints, each table rounded up to 256 bytes, then the
    uint8 [B,rows read,size,C] intermediate."""
    S = FILTERS[interpolation][1]
    tables = 0
    for n_in, n_out in ((Ws, W2), (Hs, H2)):
        ksize = int(math.ceil(S * max(n_in / n_out, 1.0))) * 2 + 1
        tables += (B * size * (ksize + 2) * 4 + 255) // 256 * 256
    return tables + B * rows_read(Hs, H2, top, size, interpolation)[1] * size * C


def normalize(u8, mean, std):
    """What nvit_center_crop_apply writes as fp32: uint8 [B,H,W,C] -> float32 [B,C,H,W] = fma(x, 1/255, -mean) * (1 / std)
    in fp32, the operations of nvit_normalize_images.  The fused multiply-subtract is computed in fp64, where it is exact
    (an 8-bit x times a 24-bit constant, minus a 24-bit mean of similar magnitude), and rounded to fp32 once."""
    x = np.asarray(u8, dtype=np.uint8).astype(np.float64)
    k, m = np.float64(np.float32(1.0) / np.float32(255.0)), np.float64(np.float32(mean))
    inv_std = np.float32(1.0) / np.float32(std)
    return ((x * k - m).astype(np.float32) * inv_std).astype(np.float32).transpose(0, 3, 1, 2).copy()


def golden_cases():
    """tests/golden/center_crop_pil.npz (tools/make_golden_center_crop.py): [(src uint8 [Hs,Ws,C], (H2, W2, top, left,
    size), {filter name: Pillow's uint8 [size,size,C]})]."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "center_crop_pil.npz"))
    return [(z[f"{i}_src"], tuple(int(v) for v in z[f"{i}_geom"]), {f: z[f"{i}_{f}"] for f in FILTERS})
            for i in range(int(z["n_cases"]))]
