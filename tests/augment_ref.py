"""numpy restatement of the AutoAugment ops, magnitudes, policies' draw and Philox4x32-10.

Independent of nvit_amd/augment.py on purpose: the GPU tests compare the kernels and the host tables against this file,
and tests/test_augment_ref.py compares this file against Pillow (the written definition of the ops).  Images are uint8
[H,W,C] arrays, C in {1,3}; every op returns a new array."""
import math

import numpy as np

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize", "Invert")
ID = {n: i for i, n in enumerate(OPS)}
SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
HAS_MAGNITUDE = SIGNED + ("Posterize", "Solarize")


# ------------------------------------------------------------------------------------------------- magnitudes
def lin(a, b, m):
    return a + (b - a) * m / 9


def magnitude(op, m, sign, W):
    """The op's argument at magnitude index m (0..9), sign 0 = +, 1 = -: a float, or an int for pixels/bits/threshold."""
    name = OPS[op] if isinstance(op, int) else op
    neg = -1 if sign else 1
    if name in ("ShearX", "ShearY"):
        return neg * lin(0.0, 0.3, m)
    if name in ("TranslateX", "TranslateY"):
        return neg * int(lin(0.0, 150.0 / 331.0 * W, m))
    if name == "Rotate":
        return neg * lin(0.0, 30.0, m)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return 1.0 + neg * lin(0.0, 0.9, m)
    if name == "Posterize":
        return 8 - round(m / 2.25)
    if name == "Solarize":
        return int(lin(255.0, 0.0, m))
    return 0


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def affine_fixed(coef):
    """Six output-to-input coefficients -> Pillow's six 16.16 integers (the half-pixel centre folded into a2, a5)."""
    a0, a1, a2, a3, a4, a5 = coef
    return [fix(a0), fix(a1), fix(a2 + a0 * 0.5 + a1 * 0.5), fix(a3), fix(a4), fix(a5 + a3 * 0.5 + a4 * 0.5)]


def affine_coef(name, value, H, W):
    if name == "ShearX":
        return (1.0, value, 0.0, 0.0, 1.0, 0.0)
    if name == "ShearY":
        return (1.0, 0.0, 0.0, value, 1.0, 0.0)
    if name == "TranslateX":
        return (1.0, 0.0, float(value), 0.0, 1.0, 0.0)
    if name == "TranslateY":
        return (1.0, 0.0, 0.0, 0.0, 1.0, float(value))
    assert name == "Rotate"
    r = -math.radians(value)
    c, s = round(math.cos(r), 15), round(math.sin(r), 15)
    cx, cy = W / 2.0, H / 2.0
    return (c, s, c * -cx + s * -cy + 0.0 + cx, -s, c, -s * -cx + c * -cy + 0.0 + cy)


def f32_bits(f):
    return int(np.array([f], dtype=np.float32).view(np.int32)[0])


def op_row(op, value, H, W):
    """One 8-int row of the parameter table: op id, then six fixed-point coefficients or the argument's bits."""
    name = OPS[op] if isinstance(op, int) else op
    row = [ID[name]] + [0] * 7
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        row[1:7] = affine_fixed(affine_coef(name, value, H, W))
    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
        row[1] = f32_bits(value)
    elif name in ("Posterize", "Solarize"):
        row[1] = int(value)
    return row


def arg_table(H, W):
    """int32 [15,10,2,8]: op_row for every op, magnitude index and sign."""
    t = np.zeros((len(OPS), 10, 2, 8), dtype=np.int64)
    for o, name in enumerate(OPS):
        for m in range(10):
            for sg in range(2):
                t[o, m, sg] = op_row(name, magnitude(name, m, sg, W), H, W)
    assert np.abs(t).max() < 2 ** 31
    return t.astype(np.int32)


# ------------------------------------------------------------------------------------------------- the ops
def gray(img):
    if img.shape[2] == 1:
        return img[:, :, 0].copy()
    x = img.astype(np.int64)
    return ((19595 * x[:, :, 0] + 38470 * x[:, :, 1] + 7471 * x[:, :, 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, x, f):
    """(uint8) clamp(deg + f * (x - deg), 0, 255) in fp32, multiply then add, truncating."""
    f = np.float32(f)
    d = (x.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    t = deg.astype(np.float32) + f * d
    assert t.dtype == np.float32
    return np.clip(t, 0, 255).astype(np.uint8)


def affine(img, fixed):
    a0, a1, a2, a3, a4, a5 = (int(v) for v in fixed)
    H, W, _ = img.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def contrast_mean(img):
    n = img.shape[0] * img.shape[1]
    return (2 * int(gray(img).astype(np.int64).sum()) + n) // (2 * n)


def smooth(img):
    x = img.astype(np.int64)
    out = x.copy()
    H, W, _ = img.shape
    if H >= 3 and W >= 3:
        acc = np.zeros_like(x[1:-1, 1:-1])
        for dy in range(3):
            for dx in range(3):
                acc += x[dy:H - 2 + dy, dx:W - 2 + dx] * (5 if dy == 1 and dx == 1 else 1)
        out[1:-1, 1:-1] = (2 * acc + 13) // 26
    return out.astype(np.uint8)


def autocontrast_lut(ch):
    lo, hi = int(ch.min()), int(ch.max())
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.array([min(255, max(0, int(i * scale + off))) for i in range(256)], dtype=np.uint8)


def equalize_lut(ch):
    h = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return ident
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return ident
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def apply_row(img, row):
    """One op, given as its 8-int parameter row."""
    op, a = int(row[0]), [int(v) for v in row[1:]]
    name = OPS[op]
    f = np.array([a[0]], dtype=np.int32).view(np.float32)[0]
    if name == "Identity":
        return img.copy()
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        return affine(img, a[:6])
    if name == "Brightness":
        return blend(np.zeros_like(img), img, f)
    if name == "Color":
        return blend(np.repeat(gray(img)[:, :, None], img.shape[2], axis=2), img, f)
    if name == "Contrast":
        return blend(np.full_like(img, contrast_mean(img)), img, f)
    if name == "Sharpness":
        return blend(smooth(img), img, f)
    if name == "Posterize":
        return img & np.uint8(~(0xFF >> a[0]) & 0xFF)
    if name == "Solarize":
        return np.where(img.astype(np.int32) >= a[0], 255 - img, img).astype(np.uint8)
    if name == "AutoContrast":
        return np.stack([autocontrast_lut(img[:, :, c])[img[:, :, c]] for c in range(img.shape[2])], axis=2)
    if name == "Equalize":
        return np.stack([equalize_lut(img[:, :, c])[img[:, :, c]] for c in range(img.shape[2])], axis=2)
    if name == "Invert":
        return 255 - img
    raise ValueError(op)


def apply_op(img, op, value=0):
    H, W, _ = img.shape
    return apply_row(img, op_row(op, value, H, W))


def apply_params(batch, params):
    """batch uint8 [B,H,W,C], params int [B,2,8] -> augmented uint8 batch (the two ops in sequence)."""
    return np.stack([apply_row(apply_row(batch[b], params[b, 0]), params[b, 1]) for b in range(batch.shape[0])])


def normalize(u8, mean=0.5, std=0.5):
    """ToTensor + Normalize in fp32: [B,H,W,C] uint8 -> [B,C,H,W] float32 (for sanity checks; the GPU tests compare bits
    with ops.normalize_images instead)."""
    x = u8.astype(np.float32) * np.float32(1.0 / 255.0)
    return ((x - np.float32(mean)) * (np.float32(1.0) / np.float32(std))).transpose(0, 3, 1, 2).copy()


# ------------------------------------------------------------------------------------------------- policies
def _p(*subs):
    return [[(a, pa, ma), (b, pb, mb)] for (a, pa, ma, b, pb, mb) in subs]


POLICIES = {
    "cifar10": _p(
        ("Invert", .1, 0, "Contrast", .2, 6), ("Rotate", .7, 2, "TranslateX", .3, 9), ("Sharpness", .8, 1, "Sharpness", .9, 3),
        ("ShearY", .5, 8, "TranslateY", .7, 9), ("AutoContrast", .5, 0, "Equalize", .9, 0), ("ShearY", .2, 7, "Posterize", .3, 7),
        ("Color", .4, 3, "Brightness", .6, 7), ("Sharpness", .3, 9, "Brightness", .7, 9), ("Equalize", .6, 0, "Equalize", .5, 0),
        ("Contrast", .6, 7, "Sharpness", .6, 5), ("Color", .7, 7, "TranslateX", .5, 8), ("Equalize", .3, 0, "AutoContrast", .4, 0),
        ("TranslateY", .4, 3, "Sharpness", .2, 6), ("Brightness", .9, 6, "Color", .2, 8), ("Solarize", .5, 2, "Invert", .0, 0),
        ("Equalize", .2, 0, "AutoContrast", .6, 0), ("Equalize", .2, 0, "Equalize", .6, 0), ("Color", .9, 9, "Equalize", .6, 0),
        ("AutoContrast", .8, 0, "Solarize", .2, 8), ("Brightness", .1, 3, "Color", .7, 0), ("Solarize", .4, 5, "AutoContrast", .9, 0),
        ("TranslateY", .9, 9, "TranslateY", .7, 9), ("AutoContrast", .9, 0, "Solarize", .8, 3), ("Equalize", .8, 0, "Invert", .1, 0),
        ("TranslateY", .7, 9, "AutoContrast", .9, 0)),
    "imagenet": _p(
        ("Posterize", .4, 8, "Rotate", .6, 9), ("Solarize", .6, 5, "AutoContrast", .6, 0), ("Equalize", .8, 0, "Equalize", .6, 0),
        ("Posterize", .6, 7, "Posterize", .6, 6), ("Equalize", .4, 0, "Solarize", .2, 4), ("Equalize", .4, 0, "Rotate", .8, 8),
        ("Solarize", .6, 3, "Equalize", .6, 0), ("Posterize", .8, 5, "Equalize", 1., 0), ("Rotate", .2, 3, "Solarize", .6, 8),
        ("Equalize", .6, 0, "Posterize", .4, 6), ("Rotate", .8, 8, "Color", .4, 0), ("Rotate", .4, 9, "Equalize", .6, 0),
        ("Equalize", .0, 0, "Equalize", .8, 0), ("Invert", .6, 0, "Equalize", 1., 0), ("Color", .6, 4, "Contrast", 1., 8),
        ("Rotate", .8, 8, "Color", 1., 2), ("Color", .8, 8, "Solarize", .8, 7), ("Sharpness", .4, 7, "Invert", .6, 0),
        ("ShearX", .6, 5, "Equalize", 1., 0), ("Color", .4, 0, "Equalize", .6, 0), ("Equalize", .4, 0, "Solarize", .2, 4),
        ("Solarize", .6, 5, "AutoContrast", .6, 0), ("Invert", .6, 0, "Equalize", 1., 0), ("Color", .6, 4, "Contrast", 1., 8),
        ("Equalize", .8, 0, "Equalize", .6, 0)),
}


# ------------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """counter: four uint32, key: two uint32 -> four uint32 (Salmon et al. 2011)."""
    c = [int(v) & 0xFFFFFFFF for v in counter]
    k = [int(v) & 0xFFFFFFFF for v in key]
    for r in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def draw(policy, seed, step, first_index, B, H, W):
    """The parameter table int32 [B,2,8] of one step: what nvit_augment_draw writes."""
    tab = arg_table(H, W)
    P = len(policy)
    out = np.zeros((B, 2, 8), dtype=np.int32)
    for i in range(B):
        g = first_index + i
        r = philox4x32_10((g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        sub = policy[(r[0] * P) >> 32]
        for k in range(2):
            name, p, m = sub[k]
            u = np.float32(r[1 + k] >> 8) * np.float32(2.0 ** -24)
            if u < np.float32(p):
                out[i, k] = tab[ID[name], m, (r[3] >> k) & 1]
    return out
