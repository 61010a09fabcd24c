"""numpy restatement of the on-device RandomResizedCrop (+ horizontal flip) and RandomErasing: both
draws, Pillow's tap computation and two-pass 8-bit resample, the flip, and the erasing with its noise.

Independent of nvit_amd/crop.py and of the kernels on purpose: the GPU tests compare both against this file, and
tests/test_crop_ref.py holds this file to Pillow.  What it takes from outside are the two host tables (the aspect table
and the normal quantile table), as arguments.

Draws.  Philox4x32-10, counter = (first_index + b, step), key = (seed low, seed high ^ (DOMAIN + a)): a = 0..9 are the ten
attempts (words: area, aspect, top, left), a = 10 the flip bit (crop) or the gate (erasing), a = 11 the noise sub-key."""
import numpy as np

from mix_ref import M32, philox_vec

CROP_DOMAIN = 0x43524F50
ERASE_DOMAIN = 0x45524153
ATTEMPTS = 10
KNOTS = 1024
PRECISION_BITS = 22


def golden_cases():
    """tests/golden/crop_pil.npz (tools/make_golden_crop.py): [(src uint8 [Hs,Ws,C], size, boxes int [n,4] = (top, left, h,
    w), {filter name: Pillow's uint8 [n,size,size,C]})]."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crop_pil.npz"))
    return [(z[f"{i}_src"], int(z[f"{i}_size"]), z[f"{i}_boxes"], {f: z[f"{i}_{f}"] for f in FILTERS})
            for i in range(int(z["n_cases"]))]


def words(seed, step, first_index, n, domain):
    """The four 32-bit words of images 0..n-1 under one key domain, as uint64 arrays."""
    g = np.array([first_index + b for b in range(n)], dtype=np.uint64)
    one = np.ones(n, dtype=np.uint64)
    return philox_vec(g & M32, g >> np.uint64(32), one * np.uint64(step & 0xFFFFFFFF), one * np.uint64(step >> 32),
                      seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ domain)


def unit64(r):
    return (r >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def aspect_of(r, table):
    """exp(U(log r0, log r1)) from the 1025-knot fp64 table: linear between knots, multiply then add, in fp64."""
    t = np.asarray(table, dtype=np.float64)
    u = (r >> np.uint64(8)).astype(np.int64)
    k = u >> 14
    f = (u & 0x3FFF).astype(np.float64) * 2.0 ** -14
    return t[k] + f * (t[k + 1] - t[k])


def int_range(r, n):
    """(r * n) >> 32 for n up to 2^31."""
    return ((r * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


# ---------------------------------------------------------------------------------------------- RandomResizedCrop: the draw
def crop_draw(seed, step, first_index, B, Hs, Ws, scale, ratio, table, hflip):
    """What nvit_crop_draw writes: int32 [B,8] = (top, left, h, w, flip, 0, 0, 0); torchvision's get_params."""
    out = np.zeros((B, 8), dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    s0, s1 = np.float64(scale[0]), np.float64(scale[1])
    for a in range(ATTEMPTS):
        r0, r1, r2, r3 = words(seed, step, first_index, B, CROP_DOMAIN + a)
        target = np.float64(Hs * Ws) * (s0 + unit64(r0) * (s1 - s0))
        aspect = aspect_of(r1, table)
        w, h = np.rint(np.sqrt(target * aspect)), np.rint(np.sqrt(target / aspect))
        ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs) & ~done
        wi, hi = np.where(ok, w, 1).astype(np.int64), np.where(ok, h, 1).astype(np.int64)
        top, left = int_range(r2, Hs - hi + 1), int_range(r3, Ws - wi + 1)
        out[ok, 0], out[ok, 1], out[ok, 2], out[ok, 3] = top[ok], left[ok], hi[ok], wi[ok]
        done |= ok
    # the central fallback
    in_ratio = np.float64(Ws) / np.float64(Hs)
    if in_ratio < np.float64(min(ratio)):
        w = Ws
        h = int(np.rint(np.float64(w) / np.float64(min(ratio))))
    elif in_ratio > np.float64(max(ratio)):
        h = Hs
        w = int(np.rint(np.float64(h) * np.float64(max(ratio))))
    else:
        w, h = Ws, Hs
    h, w = min(max(h, 1), Hs), min(max(w, 1), Ws)
    out[~done, :4] = [(Hs - h) // 2, (Ws - w) // 2, h, w]
    r0 = words(seed, step, first_index, B, CROP_DOMAIN + ATTEMPTS)[0]
    out[:, 4] = (r0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) < np.float32(hflip)
    return out


# ---------------------------------------------------------------------------------------------- Pillow's resampler
def bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bicubic_filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"bilinear": (bilinear_filter, 1.0), "bicubic": (bicubic_filter, 2.0)}


def taps(in_size, out_size, interpolation):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the box [0, in_size): (xmin [out], count [out],
    int taps [out, ksize]).  Python floats are fp64 and nothing here fuses."""
    filt, S = FILTERS[interpolation]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    xmins, counts = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins[xx], counts[xx] = xmin, xmax
    return xmins, counts, kk


def resample_axis(img, out_size, interpolation):
    """One pass along axis 1 of img uint8 [R, in, C] -> uint8 [R, out, C]."""
    xmins, counts, kk = taps(img.shape[1], out_size, interpolation)
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    for xx in range(out_size):
        x0, n = xmins[xx], counts[xx]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + n, :], kk[xx, :n], axes=([1], [0]))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def sanitize(row, Hs, Ws):
    """(top, left, h, w, flip) of a table row; a box that leaves the image is the whole image."""
    top, left, h, w = (int(v) for v in row[:4])
    if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and h <= Hs and w <= Ws and top <= Hs - h and left <= Ws - w):
        top, left, h, w = 0, 0, Hs, Ws
    return top, left, h, w, int(row[4]) != 0


def crop_apply(u8, table, size, interpolation):
    """What nvit_crop_apply writes: u8 [B,Hs,Ws,C], table int [B,8] -> uint8 [B,size,size,C]: crop, horizontal pass into
    a uint8 intermediate, vertical pass, flip."""
    u8 = np.asarray(u8, dtype=np.uint8)
    B, Hs, Ws, C = u8.shape
    out = np.empty((B, size, size, C), np.uint8)
    for b in range(B):
        top, left, h, w, flip = sanitize(table[b], Hs, Ws)
        box = u8[b, top:top + h, left:left + w, :]
        mid = resample_axis(box, size, interpolation)                                           # [h, size, C]
        res = resample_axis(mid.transpose(1, 0, 2), size, interpolation).transpose(1, 0, 2)     # [size, size, C]
        out[b] = res[:, ::-1, :] if flip else res
    return out


# ---------------------------------------------------------------------------------------------- RandomErasing
def erase_draw(seed, step, first_index, B, H, W, prob, area, table):
    """What nvit_erase_draw writes: int32 [B,8] = (on, top, left, h, w, noise key low, noise key high, 0); timm's
    RandomErasing._erase with count 1: no fallback, and the strict `<`."""
    out = np.zeros((B, 8), dtype=np.int32)
    gate = (words(seed, step, first_index, B, ERASE_DOMAIN + ATTEMPTS)[0] >> np.uint64(8)).astype(np.float32) \
        * np.float32(2.0 ** -24) < np.float32(prob)
    done = ~gate
    a0, a1 = np.float64(area[0]), np.float64(area[1])
    for a in range(ATTEMPTS):
        r0, r1, r2, r3 = words(seed, step, first_index, B, ERASE_DOMAIN + a)
        target = np.float64(H * W) * (a0 + unit64(r0) * (a1 - a0))
        aspect = aspect_of(r1, table)
        h, w = np.rint(np.sqrt(target * aspect)), np.rint(np.sqrt(target / aspect))
        ok = (w < W) & (h < H) & ~done
        wi, hi = np.where(ok, w, 0).astype(np.int64), np.where(ok, h, 0).astype(np.int64)
        top, left = int_range(r2, H - hi + 1), int_range(r3, W - wi + 1)
        out[ok, 0] = 1
        out[ok, 1], out[ok, 2], out[ok, 3], out[ok, 4] = top[ok], left[ok], hi[ok], wi[ok]
        done |= ok
    k0, k1 = words(seed, step, first_index, B, ERASE_DOMAIN + ATTEMPTS + 1)[:2]
    out[:, 5], out[:, 6] = k0.astype(np.uint32).view(np.int32), k1.astype(np.uint32).view(np.int32)
    return out


def noise(k0, k1, n, q):
    """The N(0,1) noise of an image of n elements (n % 4 == 0) under sub-key (k0, k1): element block e takes
    philox(counter = (e, 0, 0, 0)); each word indexes the 1025-knot fp32 quantile table q, linear between knots."""
    q = np.asarray(q, dtype=np.float32)
    e = np.arange(n // 4, dtype=np.uint64)
    z = np.zeros(n // 4, dtype=np.uint64)
    r = np.stack(philox_vec(e, z, z, z, int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF), axis=1).reshape(-1)
    u = (r >> np.uint64(8)).astype(np.int64)
    k = u >> 14
    f = (u & 0x3FFF).astype(np.float32) * np.float32(2.0 ** -14)
    return (q[k] + (f * (q[k + 1] - q[k])).astype(np.float32)).astype(np.float32)


def erase_apply(X, table, mode, q=None):
    """What nvit_erase_apply writes: X float32 [B,C,H,W], table int [B,8]; mode "const" (0.0) or "pixel" (the noise)."""
    X = np.asarray(X, dtype=np.float32)
    B, C, H, W = X.shape
    out = X.copy()
    for b in range(B):
        on, top, left, h, w = (int(v) for v in table[b, :5])
        if not on or not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and h <= H and w <= W and top <= H - h
                          and left <= W - w):
            continue
        if mode == "const":
            out[b, :, top:top + h, left:left + w] = 0.0
        else:
            z = noise(table[b, 5], table[b, 6], C * H * W, q).reshape(C, H, W)
            out[b, :, top:top + h, left:left + w] = z[:, top:top + h, left:left + w]
    return out


def table_moments(q):
    """(variance, kurtosis) of Q(U), U uniform on [0,1), Q the piecewise-linear function through the knots: exact
    integrals of the segments, in fp64.  The mean is 0 by the table's symmetry."""
    q = np.asarray(q, dtype=np.float64)
    a, b = q[:-1], q[1:]
    n = len(a)
    m1 = np.sum((a + b) / 2) / n
    m2 = np.sum((a * a + a * b + b * b) / 3) / n
    m4 = np.sum((a ** 4 + a ** 3 * b + a * a * b * b + a * b ** 3 + b ** 4) / 5) / n
    return m1, m2, m4 / (m2 * m2)
