"""numpy restatement of the on-device RandAugment: timm's rand-m9-mstd0.5-inc1 family.

Independent of nvit_amd/randaug.py on purpose: the GPU tests compare nvit_randaug_draw / nvit_randaug_apply and the host
tables against this file, and tests/test_randaug_ref.py compares this file against Pillow.  It is the arbiter of which
Philox word feeds which decision:

    one Philox4x32-10 call per (image, layer): counter = (first_index + image, step), key = seed with DOMAIN + layer
    xor-ed into its high word.
    r0  op index (r0 * 15) >> 32 into CHOICES (timm's list order)
    r1  on iff float32(r1 >> 8) * 2^-24 < float32(prob)
    r2  the magnitude's 24-bit uniform u = r2 >> 8: the normal quantile table at knot u >> 14, the low 14 bits
        interpolating (mstd finite and > 0), or magnitude * u * 2^-24 (mstd infinite)
    r3  bit 0: the sign (1 negates); bit 1: the filter under "random" (0 bilinear, 1 bicubic)

The 13 ops that are not geometric are AutoAugment's (tests/augment_ref.py) plus SolarizeAdd.  Images are uint8 [H,W,C]
arrays, C in {1,3}."""
import math
import statistics

import numpy as np

import augment_ref as A

OPS = A.OPS + ("SolarizeAdd",)      # op ids: AutoAugment's 0..14, then the one new op
ID = {n: i for i, n in enumerate(OPS)}
CHOICES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
           "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY")   # the last two are timm's ...Rel
GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
ENHANCE = ("Brightness", "Color", "Contrast", "Sharpness")
ROW = 16
BILINEAR, BICUBIC, RANDOM = 0, 1, 2
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC, "random": RANDOM}
DOMAIN = 0x52414E44
KNOTS = 1024
NOISE_TAIL = 2.0 ** -15


# ------------------------------------------------------------------------------------------------- level maps (fp64)
def level_arg(name, m, neg, increasing, H, W, translate_pct=0.45):
    """The argument of op `name` at magnitude m (a float in [0, 10]); neg: the drawn sign bit.  Degrees, shear factor,
    pixels (a float: not rounded), enhancement factor, bits kept, threshold, or the amount added."""
    lv = m / 10.0
    if name == "Rotate":
        v = lv * 30.0
        return -v if neg else v
    if name in ("ShearX", "ShearY"):
        v = lv * 0.3
        return -v if neg else v
    if name in ("TranslateX", "TranslateY"):
        v = lv * translate_pct
        return (-v if neg else v) * float(W if name == "TranslateX" else H)
    if name in ENHANCE:
        if increasing:
            v = lv * 0.9
            return max(0.1, 1.0 + (-v if neg else v))
        return lv * 1.8 + 0.1
    if name == "Posterize":
        return 4 - int(lv * 4.0) if increasing else int(lv * 4.0)
    if name == "Solarize":
        t = min(256, int(lv * 256.0))
        return 256 - t if increasing else t
    if name == "SolarizeAdd":
        return min(128, int(lv * 110.0))
    return 0


# ------------------------------------------------------------------------------------------------- parameter rows
def affine_coef(name, value, H, W):
    """Six output-to-input coefficients as Pillow receives them: Image.transform's data, or Image.rotate's matrix."""
    if name == "Rotate":
        r = -math.radians(value % 360.0)
        c, s = round(math.cos(r), 15), round(math.sin(r), 15)
        cx, cy = W / 2.0, H / 2.0
        return (c, s, c * -cx + s * -cy + 0.0 + cx, -s, c, -s * -cx + c * -cy + 0.0 + cy)
    return A.affine_coef(name, float(value), H, W)


def row_of(name, filt=BILINEAR, coef=None, arg=0):
    """One int32 [16] row: id, filter, then six fp64 coefficients (geometric ops) or the argument in int 2."""
    row = np.zeros(ROW, dtype=np.int32)
    if name is None:
        return row   # layer off
    row[0] = ID[name]
    if name in GEOMETRIC:
        row[1] = filt
        row[2:14] = np.array(coef, dtype=np.float64).view(np.int32)
    elif name in ENHANCE:
        row[2] = A.f32_bits(arg)
    else:
        row[2] = int(arg)
    return row


def op_row(name, value=0, filt=BILINEAR, H=None, W=None):
    """The row of op `name` with its raw argument `value` (what level_arg returns), Pillow's exact matrix for Rotate."""
    if name in GEOMETRIC:
        return row_of(name, filt, affine_coef(name, value, H, W))
    return row_of(name, arg=value)


# ------------------------------------------------------------------------------------------------- the ops
def _clip(v, n):
    return np.clip(v, 0, n - 1)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, a, filt, fill):
    """Pillow's ImagingGenericTransform with affine_transform and the BILINEAR / BICUBIC filter of 8-bit images."""
    H, W, C = img.shape
    a = [float(v) for v in a]
    ys, xs = np.mgrid[0:H, 0:W]
    xi, yi = xs + 0.5, ys + 0.5
    xin = a[0] * xi + a[1] * yi + a[2]
    yin = a[3] * xi + a[4] * yi + a[5]
    ok = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(ok, xin - 0.5, 0.0), np.where(ok, yin - 0.5, 0.0)
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    src = img.astype(np.float64)
    if filt == BILINEAR:
        x0, x1 = _clip(x, W), _clip(x + 1, W)

        def row(yy):
            p0, p1 = src[yy, x0], src[yy, x1]
            return p0 + (p1 - p0) * dx
        v1 = row(_clip(y, H))
        has = (y + 1 >= 0) & (y + 1 < H)
        v2 = np.where(has[..., None], row(_clip(y + 1, H)), v1)
        v = v1 + (v2 - v1) * dy
        res = np.clip(v.astype(np.int64), 0, 255)
    else:
        cols = [_clip(x + k, W) for k in (-1, 0, 1, 2)]

        def row(yy):
            return _cubic(src[yy, cols[0]], src[yy, cols[1]], src[yy, cols[2]], src[yy, cols[3]], dx)

        def following(k, prev):
            has = (y + k >= 0) & (y + k < H)
            return np.where(has[..., None], row(_clip(y + k, H)), prev)
        v1 = row(_clip(y - 1, H))
        v2 = following(0, v1)
        v3 = following(1, v2)
        v4 = following(2, v3)
        v = _cubic(v1, v2, v3, v4, dy)
        res = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))
    fill = np.array(list(fill)[:C] if len(fill) >= C else list(fill) * C, dtype=np.int64)
    return np.where(ok[..., None], res, fill[None, None, :]).astype(np.uint8)


def solarize_add(img, add):
    lut = np.array([min(255, i + add) if i < 128 else i for i in range(256)], dtype=np.uint8)
    return lut[img]


def apply_row(img, row, fill):
    row = np.asarray(row, dtype=np.int32)
    op = int(row[0])
    if op <= 0 or op >= len(OPS):
        return img.copy()
    name = OPS[op]
    if name in GEOMETRIC:
        return affine(img, row[2:14].copy().view(np.float64), int(row[1]), fill)
    if name == "SolarizeAdd":
        return solarize_add(img, int(row[2]))
    return A.apply_row(img, [op, int(row[2]), 0, 0, 0, 0, 0, 0])


def apply_params(batch, params, fill):
    """batch uint8 [B,H,W,C], params int32 [B,L,16] -> the augmented uint8 batch (the L ops in sequence)."""
    out = []
    for b in range(batch.shape[0]):
        img = batch[b]
        for k in range(params.shape[1]):
            img = apply_row(img, params[b, k], fill)
        out.append(img)
    return np.stack(out)


# ------------------------------------------------------------------------------------------------- the draw
def normal_quantile_table():
    nd = statistics.NormalDist()
    q = [0.0] * (KNOTS + 1)
    q[0] = nd.inv_cdf(NOISE_TAIL)
    for k in range(1, KNOTS // 2):
        q[k] = nd.inv_cdf(k / KNOTS)
    for k in range(KNOTS // 2):
        q[KNOTS - k] = -q[k]
    return np.array(q, dtype=np.float64)


def rot_table(mmax):
    """fp64 [2, KNOTS + 1]: cos and sin at k / KNOTS * 3 * mmax degrees."""
    deg = [k / KNOTS * (3.0 * mmax) for k in range(KNOTS + 1)]
    return np.array([[math.cos(math.radians(d)) for d in deg], [math.sin(math.radians(d)) for d in deg]], dtype=np.float64)


def magnitude_of(u, magnitude, mstd, mmax, q):
    """The clamped magnitude from the 24-bit uniform u, and the value before the clamp."""
    if mstd == 0:
        raw = float(magnitude)
    elif math.isinf(mstd):
        raw = magnitude * (float(u) * 2.0 ** -24)
    else:
        k, f = u >> 14, float(u & 0x3FFF) * 2.0 ** -14
        raw = magnitude + mstd * (float(q[k]) + f * (float(q[k + 1]) - float(q[k])))
    m = mmax if raw > mmax else raw
    return (0.0 if m < 0.0 else m), raw


def drawn_rotate_coef(lv, neg, H, W, rot, mmax):
    """The matrix the device writes for Rotate: cos / sin interpolated from the table, no rounding to 15 digits."""
    pos = (lv * 30.0) * (float(KNOTS) / (3.0 * mmax))
    k = min(int(pos), KNOTS - 1)
    f = pos - float(k)
    c = float(rot[0, k]) + f * (float(rot[0, k + 1]) - float(rot[0, k]))
    sa = float(rot[1, k]) + f * (float(rot[1, k + 1]) - float(rot[1, k]))
    s = sa if neg else -sa
    cx, cy = W / 2.0, H / 2.0
    return (c, s, c * -cx + s * -cy + 0.0 + cx, -s, c, -s * -cx + c * -cy + 0.0 + cy)


def draw(seed, step, first_index, B, H, W, num_layers=2, magnitude=9.0, mstd=0.5, mmax=10.0, increasing=True, prob=0.5,
         interpolation="random", translate_pct=0.45, details=None):
    """int32 [B,L,16]: what nvit_randaug_draw writes.  details: a list that receives (op index, on, raw magnitude, sign
    bit, filter bit) of every (image, layer), for the distribution tests."""
    q, rot = normal_quantile_table(), rot_table(mmax)
    interp = FILTERS[interpolation]
    out = np.zeros((B, num_layers, ROW), dtype=np.int32)
    for i in range(B):
        g = first_index + i
        for layer in range(num_layers):
            r = A.philox4x32_10((g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF),
                                (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ ((DOMAIN + layer) & 0xFFFFFFFF)))
            choice = (r[0] * len(CHOICES)) >> 32
            name = CHOICES[choice]
            on = bool(np.float32(r[1] >> 8) * np.float32(2.0 ** -24) < np.float32(prob))
            m, raw = magnitude_of(r[2] >> 8, magnitude, mstd, mmax, q)
            neg, fbit = r[3] & 1, (r[3] >> 1) & 1
            filt = fbit if interp == RANDOM else interp
            if details is not None:
                details.append((choice, on, raw, neg, fbit))
            if not on:
                continue
            if name == "Rotate":
                out[i, layer] = row_of(name, filt, drawn_rotate_coef(m / 10.0, neg, H, W, rot, mmax))
            elif name in GEOMETRIC:
                v = level_arg(name, m, neg, increasing, H, W, translate_pct)
                out[i, layer] = row_of(name, filt, A.affine_coef(name, v, H, W))
            else:
                out[i, layer] = row_of(name, arg=level_arg(name, m, neg, increasing, H, W, translate_pct))
    return out
