"""Independent restatement of the learning-rate schedules that nvit_lr_schedule evaluates on the device, for the tests.

`get_lr` is the reference trainer's method (train.py:1025-1035) as a free function of its four settings; `closed_form`
adds the linear and constant kinds and a warm-up that starts above 0.  Everything is Python float (fp64) arithmetic in
the operation order the issue fixes, so the results can be compared bit for bit.  `row_lr` is the fp32 a table row
receives, `row_bound` the derived bound of the cosine segment."""
import math
import struct

import numpy as np


def get_lr(iter_num, learning_rate, min_lr, warmup_iters, lr_decay_iters):
    if iter_num < warmup_iters:
        return learning_rate * iter_num / warmup_iters
    if iter_num > lr_decay_iters:
        return min_lr
    decay_ratio = (iter_num - warmup_iters) / (lr_decay_iters - warmup_iters)
    assert 0 <= decay_ratio <= 1
    coeff = 0.5 * (1.0 + math.cos(math.pi * decay_ratio))
    return min_lr + coeff * (learning_rate - min_lr)


def closed_form(kind, s, lr, min_lr, W, D, warmup_init=0.0):
    if s < W:
        return warmup_init + (lr - warmup_init) * s / W
    if kind == "constant":
        return lr
    if s > D:
        return min_lr
    r = (s - W) / (D - W)
    if kind == "cosine":
        return min_lr + (0.5 * (1.0 + math.cos(math.pi * r))) * (lr - min_lr)
    assert kind == "linear"
    return lr + (min_lr - lr) * r


def in_cosine_segment(kind, s, W, D):
    """True where the device's fp64 cos enters the value (it may differ from the host's in the last place)."""
    return kind == "cosine" and W <= s <= D


def row_lr(L, scale):
    """(float)(L * (double)scale) for an fp32 scale: one fp64 product, one rounding to fp32."""
    return np.float32(L * float(np.float32(scale)))


def row_bound(L, scale, lr):
    """|lr_row - L * scale| <= 2^-24 |L * scale| + 2^-40 lr: the rounding to fp32 (half an ulp, at most 2^-24 relative)
    plus a margin far below an fp32 ulp of any rate of interest and far above the error of an fp64 cos (a few 2^-53)."""
    return 2.0 ** -24 * abs(L * float(np.float32(scale))) + 2.0 ** -40 * lr


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]
