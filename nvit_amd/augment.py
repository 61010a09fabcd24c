"""Batched AutoAugment on the device: a uint8 [B,H,W,C] batch in, the model's fp32 [B,C,H,W] input out.

The randomised half of the reference's input pipeline (train.py:1081-1092) as two HIP launches per
batch (nvit_augment_draw, nvit_augment_apply), without host synchronisation, so that it sits inside a captured train
step.  Semantics: the ops run on the uint8 image and are Pillow's, bit for bit, with the magnitude ranges
and the policies of Cubuk et al. 2019; ToTensor + Normalize come last, with the arithmetic of `ops.normalize_images`.

A policy is data: a list of sub-policies, each two (op, probability, magnitude index 0..9) entries.  The draw is a
counter-based generator (Philox4x32-10, key = seed, counter = (global image index, step)): image i of step s gets the
same ops whatever the batch split, and `state_dict()` (seed, step) resumes the sequence.
"""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import call
from .ops import _chk_dev, _s, round_up
from .stages import DeviceStepCounter, StagedBatch, check_sides, check_u8_batch   # noqa: F401 (DeviceStepCounter: re-exported)

Tensor = torch.Tensor

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize", "Invert")
_ID = {n: i for i, n in enumerate(OPS)}
_AFFINE = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
_ENHANCE = ("Brightness", "Color", "Contrast", "Sharpness")
N_MAGNITUDES = _lib.const("AUG_NMAG")
ROW = _lib.const("AUG_ROW")             # ints per op in the parameter table: id + seven arguments
MAX_SIDE = _lib.const("AUG_MAX_SIDE")   # nvit_augment_apply: 16.16 coordinates in 32 bits
assert len(OPS) == _lib.const("AUG_NOPS"), "the op ids of nvit_augment_apply (include/nvit_hip.h NVIT_AUG_NOPS)"


def _sub(a, pa, ma, b, pb, mb):
    return ((a, pa, ma), (b, pb, mb))


# Cubuk et al. 2019, Appendix (the magnitude index of an op without a magnitude is written 0)
POLICIES = {
    "cifar10": (
        _sub("Invert", .1, 0, "Contrast", .2, 6), _sub("Rotate", .7, 2, "TranslateX", .3, 9),
        _sub("Sharpness", .8, 1, "Sharpness", .9, 3), _sub("ShearY", .5, 8, "TranslateY", .7, 9),
        _sub("AutoContrast", .5, 0, "Equalize", .9, 0), _sub("ShearY", .2, 7, "Posterize", .3, 7),
        _sub("Color", .4, 3, "Brightness", .6, 7), _sub("Sharpness", .3, 9, "Brightness", .7, 9),
        _sub("Equalize", .6, 0, "Equalize", .5, 0), _sub("Contrast", .6, 7, "Sharpness", .6, 5),
        _sub("Color", .7, 7, "TranslateX", .5, 8), _sub("Equalize", .3, 0, "AutoContrast", .4, 0),
        _sub("TranslateY", .4, 3, "Sharpness", .2, 6), _sub("Brightness", .9, 6, "Color", .2, 8),
        _sub("Solarize", .5, 2, "Invert", .0, 0), _sub("Equalize", .2, 0, "AutoContrast", .6, 0),
        _sub("Equalize", .2, 0, "Equalize", .6, 0), _sub("Color", .9, 9, "Equalize", .6, 0),
        _sub("AutoContrast", .8, 0, "Solarize", .2, 8), _sub("Brightness", .1, 3, "Color", .7, 0),
        _sub("Solarize", .4, 5, "AutoContrast", .9, 0), _sub("TranslateY", .9, 9, "TranslateY", .7, 9),
        _sub("AutoContrast", .9, 0, "Solarize", .8, 3), _sub("Equalize", .8, 0, "Invert", .1, 0),
        _sub("TranslateY", .7, 9, "AutoContrast", .9, 0)),
    "imagenet": (
        _sub("Posterize", .4, 8, "Rotate", .6, 9), _sub("Solarize", .6, 5, "AutoContrast", .6, 0),
        _sub("Equalize", .8, 0, "Equalize", .6, 0), _sub("Posterize", .6, 7, "Posterize", .6, 6),
        _sub("Equalize", .4, 0, "Solarize", .2, 4), _sub("Equalize", .4, 0, "Rotate", .8, 8),
        _sub("Solarize", .6, 3, "Equalize", .6, 0), _sub("Posterize", .8, 5, "Equalize", 1., 0),
        _sub("Rotate", .2, 3, "Solarize", .6, 8), _sub("Equalize", .6, 0, "Posterize", .4, 6),
        _sub("Rotate", .8, 8, "Color", .4, 0), _sub("Rotate", .4, 9, "Equalize", .6, 0),
        _sub("Equalize", .0, 0, "Equalize", .8, 0), _sub("Invert", .6, 0, "Equalize", 1., 0),
        _sub("Color", .6, 4, "Contrast", 1., 8), _sub("Rotate", .8, 8, "Color", 1., 2),
        _sub("Color", .8, 8, "Solarize", .8, 7), _sub("Sharpness", .4, 7, "Invert", .6, 0),
        _sub("ShearX", .6, 5, "Equalize", 1., 0), _sub("Color", .4, 0, "Equalize", .6, 0),
        _sub("Equalize", .4, 0, "Solarize", .2, 4), _sub("Solarize", .6, 5, "AutoContrast", .6, 0),
        _sub("Invert", .6, 0, "Equalize", 1., 0), _sub("Color", .6, 4, "Contrast", 1., 8),
        _sub("Equalize", .8, 0, "Equalize", .6, 0)),
}
POLICIES["cifar100"] = POLICIES["cifar10"]   # the paper reports CIFAR-100 with the policy found on CIFAR-10


# ---------------------------------------------------------------------------------------------- host tables (fp64)
def _op_id(op) -> int:
    if isinstance(op, str):
        if op not in _ID:
            raise ValueError(f"unknown op {op!r} (known: {', '.join(OPS)})")
        return _ID[op]
    if isinstance(op, bool) or not isinstance(op, int):
        raise TypeError(f"an op is a name or an id 0..{len(OPS) - 1} (got {op!r})")
    if not 0 <= op < len(OPS):
        raise ValueError(f"unknown op id {op} (0..{len(OPS) - 1})")
    return op


def _check_magnitude(m) -> int:
    if isinstance(m, bool) or not isinstance(m, int):
        raise TypeError(f"a magnitude index is an int 0..{N_MAGNITUDES - 1} (got {m!r})")
    if not 0 <= m < N_MAGNITUDES:
        raise ValueError(f"magnitude index {m} outside 0..{N_MAGNITUDES - 1}")
    return m


def _lin(a: float, b: float, m: int) -> float:
    return a + (b - a) * m / 9


def magnitude(op, m: int, sign: int, W: int):
    """The argument of `op` at magnitude index m, sign 0 = +, 1 = -: shear factor, pixels, degrees, enhancement factor,
    bits or threshold (0 for an op without one).  TranslateY also scales with the width, as the paper's code does."""
    name = OPS[_op_id(op)]
    m = _check_magnitude(m)
    neg = -1 if sign else 1
    if name in ("ShearX", "ShearY"):
        return neg * _lin(0.0, 0.3, m)
    if name in ("TranslateX", "TranslateY"):
        return neg * int(_lin(0.0, 150.0 / 331.0 * W, m))
    if name == "Rotate":
        return neg * _lin(0.0, 30.0, m)
    if name in _ENHANCE:
        return 1.0 + neg * _lin(0.0, 0.9, m)
    if name == "Posterize":
        return 8 - round(m / 2.25)
    if name == "Solarize":
        return int(_lin(255.0, 0.0, m))
    return 0


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def _f32_bits(f: float) -> int:
    return struct.unpack("<i", struct.pack("<f", f))[0]


def affine_coefficients(name: str, value: float, H: int, W: int) -> tuple:
    """Pillow's six coefficients (a, b, c, d, e, f) of a geometric op, output to input: x_in = a x + b y + c, y_in = d x +
    e y + f.  value: the shear factor, the pixels, or Image.rotate's degrees about (W/2, H/2)."""
    value = float(value)
    if name == "ShearX":
        return 1.0, value, 0.0, 0.0, 1.0, 0.0
    if name == "ShearY":
        return 1.0, 0.0, 0.0, value, 1.0, 0.0
    if name == "TranslateX":
        return 1.0, 0.0, value, 0.0, 1.0, 0.0
    if name == "TranslateY":
        return 1.0, 0.0, 0.0, 0.0, 1.0, value
    r = -math.radians(value)
    c, s = round(math.cos(r), 15), round(math.sin(r), 15)
    cx, cy = W / 2.0, H / 2.0
    return c, s, c * -cx + s * -cy + 0.0 + cx, -s, c, -s * -cx + c * -cy + 0.0 + cy


def op_row(op, value, H: int, W: int):
    """The eight ints of one op in the parameter table: id, then Pillow's six 16.16 affine coefficients (output to
    input, the half-pixel centre folded into the two offsets), or the argument's bits and zeros."""
    name = OPS[_op_id(op)]
    row = [_ID[name]] + [0] * (ROW - 1)
    if name in _AFFINE:
        a = affine_coefficients(name, value, H, W)
        row[1:7] = [_fix(a[0]), _fix(a[1]), _fix(a[2] + a[0] * 0.5 + a[1] * 0.5),
                    _fix(a[3]), _fix(a[4]), _fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
        # offset + coefficient * y + coefficient * x stays inside 32 bits for sides up to MAX_SIDE
        if any(abs(row[i]) > 2 ** 17 for i in (1, 2, 4, 5)) or any(abs(row[i]) >= 2 ** 29 for i in (3, 6)):
            raise ValueError(f"{name}({value}) at {H}x{W} leaves the 16.16 range")
    elif name in _ENHANCE:
        row[1] = _f32_bits(float(value))
    elif name == "Posterize":
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= 8:
            raise ValueError(f"Posterize keeps 0..8 bits (got {value!r})")
        row[1] = value
    elif name == "Solarize":
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= 256:
            raise ValueError(f"Solarize takes a threshold 0..256 (got {value!r})")
        row[1] = value
    return row


def _check_hw(H: int, W: int, name: str = "AutoAugment") -> None:
    check_sides(name, H, W, MAX_SIDE)


def arg_table(H: int, W: int) -> Tensor:
    """int32 [15,10,2,8] on the host: op_row of every (op, magnitude index, sign) at this image size."""
    _check_hw(H, W)
    rows = [op_row(o, magnitude(o, m, sg, W), H, W) for o in range(len(OPS)) for m in range(N_MAGNITUDES)
            for sg in range(2)]
    return torch.tensor(rows, dtype=torch.int32).view(len(OPS), N_MAGNITUDES, 2, ROW)


def validate_policy(policy) -> tuple:
    """A policy in canonical form ((op name, probability, magnitude index) x 2 per sub-policy); ValueError/TypeError
    for an empty policy, a sub-policy that is not two entries, an unknown op, a probability outside [0,1] or a
    magnitude index outside 0..9."""
    if isinstance(policy, str):
        if policy not in POLICIES:
            raise ValueError(f"unknown policy {policy!r} (shipped: {', '.join(sorted(POLICIES))})")
        policy = POLICIES[policy]
    try:
        subs = [tuple(tuple(e) for e in sub) for sub in policy]
    except TypeError:
        raise TypeError("a policy is a list of sub-policies, each two (op, probability, magnitude index) entries")
    if not subs:
        raise ValueError("empty policy")
    out = []
    for sub in subs:
        if len(sub) != 2 or any(len(e) != 3 for e in sub):
            raise ValueError(f"a sub-policy is two (op, probability, magnitude index) entries (got {sub!r})")
        canon = []
        for op, p, m in sub:
            name = OPS[_op_id(op)]
            if isinstance(p, bool) or not isinstance(p, (int, float)):
                raise TypeError(f"a probability is a number in [0,1] (got {p!r})")
            if not 0.0 <= p <= 1.0:   # also refuses NaN
                raise ValueError(f"probability {p} outside [0,1]")
            canon.append((name, float(p), _check_magnitude(m)))
        out.append(tuple(canon))
    return tuple(out)


def _check_images(u8, name: str = "AutoAugment") -> tuple:
    return check_u8_batch(name, u8, MAX_SIDE)


def _apply_buffers(u8: Tensor, return_u8: bool) -> tuple:
    """(workspace, its bytes, fp32 [B,C,H,W] output or None, uint8 [B,H,W,C] output or None) of an apply kernel."""
    B, H, W, C = u8.shape
    ws_bytes = 2 * B * round_up(H * W * C, 256)
    ws = torch.empty(ws_bytes, device=u8.device, dtype=torch.uint8)
    if return_u8:
        return ws, ws_bytes, None, torch.empty_like(u8)
    return ws, ws_bytes, torch.empty((B, C, H, W), device=u8.device, dtype=torch.float32), None


class AugmentedBatch(StagedBatch):
    """A uint8 [B,H,W,C] batch together with the AutoAugment (or the RandAugment of randaug.py: anything whose call
    turns such a batch into fp32 [B,C,H,W]) that makes it the model's input: what `AutoAugment.batch(u8)` /
    `RandAugment.batch(u8)` return and `train_step` / `GraphedTrainStep` accept in place of X.  u8: the tensor, or a
    `RandomResizedCrop.batch(u8)` (crop.py) whose crops are then what the policies see, or a `DeviceLoader.batch()` (data.py)
    whose gathered batch is.  `.shape` is u8's."""

    key, word, accepts, names = "augment", "augmentation", ("crop", "data"), ("augment", "u8")

    def __init__(self, augment: "AutoAugment", u8):
        name = type(augment).__name__
        if self.takes(u8):
            _check_hw(u8.shape[1], u8.shape[2], name)
        else:
            _check_images(u8, name)
        if u8.shape[2] % 4:
            raise ValueError(f"{name}: the fp32 output needs W % 4 == 0")
        super().__init__(augment, u8, u8.shape)

    def augmented(self) -> Tensor:
        return self._launch(None)[0]


class AutoAugment(DeviceStepCounter):
    """AutoAugment(policy="cifar10", seed=0, first_index=0, mean=0.5, std=0.5).to(device)

    policy: "cifar10", "imagenet" (the published tables, 25 sub-policies each), "cifar100" (the CIFAR-10 table: the
    paper found no separate one), or a list of sub-policies [((op, p, m), (op, p, m)), ...].
    first_index: the global index of this batch's first image in the step; a data-parallel rank passes rank * B, and
    the ranks then draw what one process would for the whole step's batch.

    `aug(u8)` draws the step's parameters and returns the fp32 [B,C,H,W] model input; `draw` and `apply` are its two
    halves; `params_for` writes a parameter table by hand.  The step counter lives on the device and is advanced by
    the draw kernel, so a captured graph that contains the call draws fresh parameters at every replay."""

    def __init__(self, policy="cifar10", seed: int = 0, first_index: int = 0, mean: float = 0.5, std: float = 0.5):
        self.policy = validate_policy(policy)
        super().__init__(seed, first_index)
        if std == 0:
            raise ValueError("std must not be 0")
        self.mean, self.std = float(mean), float(std)
        self._policy_dev: Optional[Tensor] = None
        self._argtabs = {}

    # ------------------------------------------------------------------ device state
    def to(self, device) -> "AutoAugment":
        device = self._step_to(device)
        rows = [[_ID[n], _f32_bits(p), m] for sub in self.policy for (n, p, m) in sub]
        self._policy_dev = torch.tensor(rows, dtype=torch.int32).view(len(self.policy), 2, 3).to(device)
        self._argtabs = {}
        return self

    def _argtab(self, H: int, W: int) -> Tensor:
        t = self._argtabs.get((H, W))
        if t is None:
            t = self._argtabs[(H, W)] = arg_table(H, W).to(self.device)
        return t

    # ------------------------------------------------------------------ the two launches
    def draw(self, B: int, H: int, W: int) -> Tensor:
        """int32 [B,2,8] parameter table of the next step (nvit_augment_draw); advances the step counter.  The first
        call at a new (H, W) uploads that size's argument table, so warm a size up before capturing a graph."""
        self._need_device()
        if B < 1:
            raise ValueError("AutoAugment.draw: B must be >= 1")
        tab = self._argtab(H, W)
        params = torch.empty((B, 2, ROW), device=self.device, dtype=torch.int32)
        call("nvit_augment_draw", self._policy_dev, len(self.policy), self.seed, self._step, self.first_index, tab, params,
             B, _s())
        return params

    def apply(self, u8: Tensor, params: Tensor, return_u8: bool = False):
        """The two ops of params[b] on image b, then ToTensor + Normalize: fp32 [B,C,H,W] (needs W % 4 == 0, as
        ops.normalize_images does); with return_u8 the augmented uint8 [B,H,W,C] instead."""
        B, H, W, C = _check_images(u8)
        if not isinstance(params, Tensor) or params.dtype != torch.int32 or tuple(params.shape) != (B, 2, ROW):
            raise ValueError(f"AutoAugment.apply: params must be int32 [{B},2,{ROW}]")
        if not return_u8 and W % 4:
            raise ValueError("AutoAugment.apply: the fp32 output needs W % 4 == 0")
        _chk_dev(u8, params)
        u8, params = u8.contiguous(), params.contiguous()
        ws, ws_bytes, f32, o8 = _apply_buffers(u8, return_u8)
        call("nvit_augment_apply", u8, params, f32, o8, ws, ws_bytes, B, H, W, C, self.mean, self.std, _s())
        return o8 if return_u8 else f32

    def __call__(self, u8: Tensor) -> Tensor:
        B, H, W, C = _check_images(u8)
        if W % 4:
            raise ValueError("AutoAugment: the fp32 output needs W % 4 == 0")
        _chk_dev(u8)
        return self.apply(u8, self.draw(B, H, W))

    def batch(self, u8: Tensor) -> AugmentedBatch:
        """The X of `train_step(model, optimizer, aug.batch(u8), y)` and of `GraphedTrainStep`: the augmentation runs
        inside the step (and inside its captured graph), once per batch."""
        return AugmentedBatch(self, u8)

    # ------------------------------------------------------------------ parameter tables by hand
    def params_for(self, ops: Sequence, H: int, W: int) -> Tensor:
        """int32 [B,2,8] from ops[b] = (first, second), each entry (op, magnitude index, sign) - what the draw writes
        for that choice - or (op, {"value": v}) with the op's raw argument: shear factor, translate pixels, rotate
        degrees, enhancement factor, posterize bits or solarize threshold.  A bare op name takes magnitude 0."""
        _check_hw(H, W)
        rows = []
        for pair in ops:
            pair = list(pair)
            if len(pair) != 2:
                raise ValueError("params_for: two ops per image")
            for e in pair:
                e = (e,) if isinstance(e, (str, int)) else tuple(e)
                if len(e) == 2 and isinstance(e[1], dict):
                    rows.append(op_row(e[0], e[1]["value"], H, W))
                else:
                    op, m, sign = (e + (0, 0))[:3]
                    if sign not in (0, 1):
                        raise ValueError(f"sign is 0 (+) or 1 (-) (got {sign!r})")
                    rows.append(op_row(op, magnitude(op, m, sign, W), H, W))
        if not rows:
            raise ValueError("params_for: no images")
        t = torch.tensor(rows, dtype=torch.int32).view(-1, 2, ROW)
        return t if self.device is None else t.to(self.device)
