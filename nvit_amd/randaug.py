"""Batched RandAugment on the device: timm's `rand-m9-mstd0.5-inc1` family in AutoAugment's place in the input chain.

    RandomResizedCrop -> flip -> RandAugment -> normalize -> RandomErasing -> Mixup / CutMix
    mix.batch(erase.batch(ra.batch(rrc.batch(u8))))

The DeiT, AugReg and Swin recipes do not use AutoAugment's policies but RandAugment: per image `num_layers` ops, each
chosen uniformly among 15, applied with probability `prob` at a magnitude drawn around `magnitude`, with the
"increasing" level maps, the op SolarizeAdd, and geometric ops that resample bilinearly or bicubically onto a fill colour.
Two HIP launches per batch (nvit_randaug_draw, nvit_randaug_apply), no host synchronisation, so the stage sits inside a
captured train step and every replay draws afresh.  Semantics (tests/randaug_ref.py restates them in numpy):
the geometric ops are Pillow's `Image.transform(size, AFFINE, data, BILINEAR | BICUBIC, fillcolor=fill)` and
`Image.rotate(deg, BILINEAR | BICUBIC, fillcolor=fill)`, bit for bit, in fp64; the other ops are AutoAugment's kernels.

The draw is the counter-based generator of augment.py (Philox4x32-10; counter = (first_index + image, step), key = seed
with this class's domain constant + the layer index in its high word).  No transcendental runs on the device: the
normal deviate of the magnitude is interpolated from `crop.normal_quantile_table()`, Rotate's cosine and sine from
`rot_table(magnitude_max)`.  A drawn rotation therefore deviates from Pillow's matrix by `rot_table_deviation` (about
3.3e-8 relative at magnitude_max 10) and skips Pillow's rounding of cos / sin to 15 digits; `params_for` writes Pillow's
exact matrix.
"""
from __future__ import annotations

import functools
import math
import struct
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import call
from .augment import OPS as _AA_OPS, AugmentedBatch, _apply_buffers, _f32_bits, affine_coefficients
from .augment import _check_hw as _aa_check_hw, _check_images as _aa_check_images
from .crop import normal_quantile_table
from .ops import _chk_dev, _s
from .stages import DeviceStepCounter, check_finite, check_name, check_number, check_unit

Tensor = torch.Tensor

ROW = _lib.const("RA_ROW")               # ints per (image, layer): id, filter, six fp64 coefficients or one argument
MAX_LAYERS = _lib.const("RA_MAX_LAYERS")
ROT_KNOTS = _lib.const("RA_ROT_KNOTS")   # the cos / sin table holds ROT_KNOTS + 1 values each
OPS = _AA_OPS + ("SolarizeAdd",)         # op ids of the parameter table: AutoAugment's, then the one new op
_ID = {n: i for i, n in enumerate(OPS)}
# timm's _RAND_INCREASING_TRANSFORMS in its order (TranslateX / TranslateY are its TranslateXRel / TranslateYRel)
CHOICES = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
           "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY")
_GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
_ENHANCE = ("Brightness", "Color", "Contrast", "Sharpness")
INTERPOLATIONS = {"bilinear": _lib.const("RA_BILINEAR"), "bicubic": _lib.const("RA_BICUBIC"), "random": _lib.const("RA_RANDOM")}
LEVEL_DENOM = 10.0
assert len(OPS) == _lib.const("RA_NOPS") and _ID["SolarizeAdd"] == _lib.const("RA_SOLARIZE_ADD"), "op ids (include/nvit_hip.h)"
assert len(CHOICES) == _lib.const("RA_NCHOICES")


# ---------------------------------------------------------------------------------------------- host tables (fp64)
@functools.lru_cache(maxsize=None)
def rot_table(magnitude_max: float) -> tuple:
    """(cos, sin) at k / ROT_KNOTS * 3 * magnitude_max degrees, k = 0..ROT_KNOTS, cosines first: what the draw
    interpolates Rotate's matrix from (30 degrees at level 10)."""
    deg = [k / ROT_KNOTS * (3.0 * magnitude_max) for k in range(ROT_KNOTS + 1)]
    return tuple(math.cos(math.radians(d)) for d in deg) + tuple(math.sin(math.radians(d)) for d in deg)


def rot_table_deviation(magnitude_max: float) -> float:
    """The bound on the chord's distance from the cosine / sine it replaces, relative to the unit circle's radius:
    with d the knots' distance in radians, a chord of a function whose second derivative is at most 1 in magnitude lies
    within d^2 / 8 of it."""
    d = math.radians(3.0 * magnitude_max) / ROT_KNOTS
    return d * d / 8.0


def level_arg(op: str, m: float, neg: int, increasing: bool, H: int, W: int, translate_pct: float = 0.45):
    """timm's level maps in fp64: the argument of `op` at magnitude m (0..10), neg = the drawn sign bit.  Rotate:
    degrees; ShearX/Y: the factor; TranslateX/Y: pixels (translate_pct of the side at level 10, not rounded); the
    enhance ops: the factor; Posterize: bits kept; Solarize: the threshold; SolarizeAdd: the amount added."""
    if op not in CHOICES:
        raise ValueError(f"unknown op {op!r} (known: {', '.join(CHOICES)})")
    lv = m / LEVEL_DENOM
    if op == "Rotate":
        v = lv * 30.0
        return -v if neg else v
    if op in ("ShearX", "ShearY"):
        v = lv * 0.3
        return -v if neg else v
    if op in ("TranslateX", "TranslateY"):
        v = lv * translate_pct
        return (-v if neg else v) * float(W if op == "TranslateX" else H)
    if op in _ENHANCE:
        if increasing:
            v = lv * 0.9
            return max(0.1, 1.0 + (-v if neg else v))
        return lv * 1.8 + 0.1
    if op == "Posterize":
        return 4 - int(lv * 4.0) if increasing else int(lv * 4.0)
    if op == "Solarize":
        t = min(256, int(lv * 256.0))
        return 256 - t if increasing else t
    if op == "SolarizeAdd":
        return min(128, int(lv * 110.0))
    return 0


def _f64_ints(v: float) -> list:
    return list(struct.unpack("<ii", struct.pack("<d", float(v))))


def op_row(op: str, value=0, filter: str = "bilinear", H: Optional[int] = None, W: Optional[int] = None) -> list:
    """The ROW ints of one op with its raw argument (what `level_arg` returns): id, filter, then Pillow's six fp64
    coefficients (Image.rotate's exact matrix for Rotate), or the argument in int 2."""
    if not isinstance(op, str):
        raise TypeError(f"an op is a name (got {op!r})")
    if op not in CHOICES:
        raise ValueError(f"unknown op {op!r} (known: {', '.join(CHOICES)})")
    row = [_ID[op]] + [0] * (ROW - 1)
    if op in _GEOMETRIC:
        if not isinstance(filter, str):
            raise TypeError(f"a filter is a name (got {filter!r})")
        if filter not in ("bilinear", "bicubic"):
            raise ValueError(f"the filter of an op is bilinear or bicubic (got {filter!r})")
        value = check_finite(f"{op}'s argument", value)
        row[1] = INTERPOLATIONS[filter]
        if op == "Rotate":   # Image.rotate reduces the angle first
            _check_hw(H, W)
            value %= 360.0
        for j, v in enumerate(affine_coefficients(op, value, H, W)):
            row[2 + 2 * j:4 + 2 * j] = _f64_ints(v)
    elif op in _ENHANCE:
        row[2] = _f32_bits(check_finite(f"{op}'s factor", value))
    elif op in ("Posterize", "Solarize", "SolarizeAdd"):
        top = {"Posterize": 8, "Solarize": 256, "SolarizeAdd": 255}[op]
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= top:
            raise ValueError(f"{op} takes an int 0..{top} (got {value!r})")
        row[2] = value
    return row


# ---------------------------------------------------------------------------------------------- argument checks
def _check_fill(fill) -> tuple:
    if isinstance(fill, int) and not isinstance(fill, bool):
        fill = (fill,)
    try:
        fill = tuple(fill)
    except TypeError:
        raise TypeError(f"fill is an int or one int per channel (got {fill!r})") from None
    if any(isinstance(v, bool) or not isinstance(v, int) for v in fill):
        raise TypeError(f"fill is an int or one int per channel (got {fill!r})")
    if len(fill) not in (1, 3) or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"fill is one or three values 0..255 (got {fill!r})")
    return fill


def _check_images(u8) -> tuple:
    return _aa_check_images(u8, "RandAugment")


def _check_hw(H, W) -> None:
    _aa_check_hw(H, W, "RandAugment")


def parse_config(config: str) -> dict:
    """timm's RandAugment string ("rand-m9-mstd0.5-inc1") -> constructor arguments.  Keys: m (magnitude), n (layers),
    mstd (above 100: infinite, the uniform magnitude), mmax, inc, p.  The weighted choice `w` and unknown keys raise."""
    if not isinstance(config, str):
        raise TypeError(f"a RandAugment config is a string such as 'rand-m9-mstd0.5-inc1' (got {config!r})")
    parts = config.split("-")
    if parts[0] != "rand":
        raise ValueError(f"a RandAugment config starts with 'rand' (got {config!r})")
    kw = {}
    for part in parts[1:]:
        key = part.rstrip("0123456789.")
        val = part[len(key):]
        if not key or not val:
            raise ValueError(f"RandAugment config {config!r}: cannot read {part!r}")
        try:
            if key == "mstd":
                v = float(val)
                kw["magnitude_std"] = math.inf if v > 100 else v
            elif key == "mmax":
                kw["magnitude_max"] = float(val) if "." in val else int(val)
            elif key == "inc":
                kw["increasing"] = bool(int(val))
            elif key == "m":
                kw["magnitude"] = float(val) if "." in val else int(val)
            elif key == "n":
                kw["num_layers"] = int(val)
            elif key == "p":
                kw["prob"] = float(val)
            elif key == "w":
                raise ValueError(f"RandAugment config {config!r}: the weighted op choice (w) is not supported")
            else:
                raise ValueError(f"RandAugment config {config!r}: unknown key {key!r}")
        except ValueError as e:
            if "RandAugment config" in str(e):
                raise
            raise ValueError(f"RandAugment config {config!r}: cannot read {part!r}") from None
    return kw


class RandAugment(DeviceStepCounter):
    """RandAugment(magnitude=9, num_layers=2, magnitude_std=0.5, magnitude_max=10, increasing=True, prob=0.5,
    interpolation="random", fill=(128, 128, 128), translate_pct=0.45, mean=0.5, std=0.5, seed=0, first_index=0).to(device)

    timm's RandAugment on a uint8 [B,H,W,C] batch (C 1 or 3): per image `num_layers` (1..4) ops in sequence, each chosen
    uniformly among the 15 of `CHOICES`, skipped with probability 1 - prob, at magnitude m = magnitude + magnitude_std * z
    (z ~ N(0,1); magnitude itself for magnitude_std 0; uniform(0, magnitude) for math.inf), clamped to [0, magnitude_max].
    increasing: timm's "inc1" level maps.  interpolation: the filter of the geometric ops, "random" = one of the two per
    op application (timm's default).  fill: the colour of the pixels a geometric op uncovers, one value per channel (for
    a real run timm's img_mean, round(255 * mean)); a single value serves every channel.  mean, std: the Normalize that
    follows, as AutoAugment's.  first_index: the global index of this batch's first image in the step; a data-parallel
    rank passes rank * B.

    `ra(u8)` draws the step's table and returns the fp32 [B,C,H,W] model input; `draw` and `apply` are its halves;
    `params_for` writes a table by hand.  The step counter lives on the device and the draw kernel advances it, so a
    captured graph that contains the call draws fresh parameters at every replay.  `from_config` reads timm's string."""

    def __init__(self, magnitude=9, num_layers: int = 2, magnitude_std=0.5, magnitude_max=10, increasing: bool = True,
                 prob: float = 0.5, interpolation: str = "random", fill=(128, 128, 128), translate_pct: float = 0.45,
                 mean: float = 0.5, std: float = 0.5, seed: int = 0, first_index: int = 0):
        if isinstance(num_layers, bool) or not isinstance(num_layers, int):
            raise TypeError(f"num_layers must be an int (got {num_layers!r})")
        if not 1 <= num_layers <= MAX_LAYERS:
            raise ValueError(f"num_layers must be in 1..{MAX_LAYERS} (got {num_layers})")
        for what, v in (("magnitude", magnitude), ("magnitude_std", magnitude_std), ("magnitude_max", magnitude_max)):
            check_number(what, v)
        if not 0.0 < magnitude_max <= LEVEL_DENOM:   # (every comparison also refuses NaN)
            raise ValueError(f"magnitude_max must be in (0, {LEVEL_DENOM:g}] (got {magnitude_max!r})")
        if not 0.0 <= magnitude <= LEVEL_DENOM:
            raise ValueError(f"magnitude must be in [0, {LEVEL_DENOM:g}] (got {magnitude!r})")
        if not magnitude_std >= 0.0:
            raise ValueError(f"magnitude_std must be >= 0, math.inf for the uniform magnitude (got {magnitude_std!r})")
        check_unit("prob", prob)
        check_unit("translate_pct", translate_pct)
        if not isinstance(increasing, (bool, int)):
            raise TypeError(f"increasing must be a bool (got {increasing!r})")
        check_name("interpolation", interpolation, INTERPOLATIONS)
        check_finite("mean", mean)
        if check_finite("std", std) == 0:
            raise ValueError("std must not be 0")
        self.magnitude, self.num_layers, self.magnitude_std = float(magnitude), num_layers, float(magnitude_std)
        self.magnitude_max, self.increasing, self.prob = float(magnitude_max), bool(increasing), float(prob)
        self.interpolation, self.fill, self.translate_pct = interpolation, _check_fill(fill), float(translate_pct)
        self.mean, self.std = float(mean), float(std)
        super().__init__(seed, first_index)
        self._q: Optional[Tensor] = None
        self._rot: Optional[Tensor] = None

    @classmethod
    def from_config(cls, config: str, **kw) -> "RandAugment":
        """RandAugment.from_config("rand-m9-mstd0.5-inc1", fill=..., seed=...): timm's string, then keyword arguments
        (which win over the string's)."""
        return cls(**{**parse_config(config), **kw})

    # ------------------------------------------------------------------ device state
    def to(self, device) -> "RandAugment":
        device = self._step_to(device)
        self._q = torch.tensor(normal_quantile_table(), dtype=torch.float64).to(device)
        self._rot = torch.tensor(rot_table(self.magnitude_max), dtype=torch.float64).to(device)
        return self

    def _fill3(self, C: int) -> tuple:
        f = self.fill
        if len(f) == 1:
            return f * 3
        if C == 1 and not f[0] == f[1] == f[2]:
            raise ValueError(f"RandAugment: fill {f} has three different values but the batch one channel")
        return f

    # ------------------------------------------------------------------ the two launches
    def draw(self, B: int, H: int, W: int) -> Tensor:
        """int32 [B,num_layers,ROW] parameter table of the next step (nvit_randaug_draw); advances the step counter."""
        self._need_device()
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError("RandAugment.draw: B must be an int >= 1")
        _check_hw(H, W)
        params = torch.empty((B, self.num_layers, ROW), device=self.device, dtype=torch.int32)
        call("nvit_randaug_draw", self.seed, self._step, self.first_index, self._q, self._rot, self.magnitude,
             self.magnitude_std, self.magnitude_max, int(self.increasing), self.prob, INTERPOLATIONS[self.interpolation],
             self.translate_pct, params, B, self.num_layers, H, W, _s())
        return params

    def apply(self, u8: Tensor, params: Tensor, return_u8: bool = False):
        """The ops of params[b] on image b in sequence, then ToTensor + Normalize: fp32 [B,C,H,W] (needs W % 4 == 0, as
        ops.normalize_images does); with return_u8 the augmented uint8 [B,H,W,C] instead.  params: int32 [B,L,ROW] with
        L in 1..MAX_LAYERS (a hand-written table may hold another number of layers than num_layers)."""
        B, H, W, C = _check_images(u8)
        if (not isinstance(params, Tensor) or params.dtype != torch.int32 or params.dim() != 3 or params.shape[0] != B
                or not 1 <= params.shape[1] <= MAX_LAYERS or params.shape[2] != ROW):
            raise ValueError(f"RandAugment.apply: params must be int32 [{B},1..{MAX_LAYERS},{ROW}]")
        if not return_u8 and W % 4:
            raise ValueError("RandAugment.apply: the fp32 output needs W % 4 == 0")
        fill = self._fill3(C)
        _chk_dev(u8, params)
        u8, params = u8.contiguous(), params.contiguous()
        ws, ws_bytes, f32, o8 = _apply_buffers(u8, return_u8)
        call("nvit_randaug_apply", u8, params, f32, o8, ws, ws_bytes, B, H, W, C, params.shape[1], fill[0], fill[1], fill[2],
             self.mean, self.std, _s())
        return o8 if return_u8 else f32

    def __call__(self, u8: Tensor) -> Tensor:
        B, H, W, C = _check_images(u8)
        if W % 4:
            raise ValueError("RandAugment: the fp32 output needs W % 4 == 0")
        self._fill3(C)
        _chk_dev(u8)
        return self.apply(u8, self.draw(B, H, W))

    def batch(self, u8) -> AugmentedBatch:
        """The X of `train_step(model, optimizer, ra.batch(u8), y)`, of `GraphedTrainStep`, `RandomErasing.batch` and
        `Mixup.batch`: the augmentation runs inside the step (and inside its captured graph), once per batch.  u8: the
        uint8 [B,H,W,C] tensor or a `RandomResizedCrop.batch(u8)`."""
        xb = AugmentedBatch(self, u8)
        self._fill3(xb.shape[3])
        return xb

    # ------------------------------------------------------------------ parameter tables by hand
    def params_for(self, ops: Sequence, H: int, W: int) -> Tensor:
        """int32 [B,L,ROW] from ops[b] = a sequence of L entries (the same L, 1..MAX_LAYERS, for every image), each
        None (layer off), an op name (its argument at magnitude 0), (op, m, sign) or (op, m, sign, filter) - magnitude m
        in [0, 10] through the level maps, sign 0 = +, 1 = - - or (op, {"value": v}) / (op, {"value": v}, filter) with
        the op's raw argument: degrees, shear factor, pixels, enhancement factor, bits kept, threshold, amount added.
        filter: "bilinear" (default) or "bicubic".  Rotate gets Pillow's exact matrix, which the draw only approaches."""
        _check_hw(H, W)
        rows, L = [], None
        for entries in ops:
            entries = list(entries)
            if L is None:
                L = len(entries)
            if len(entries) != L or not 1 <= L <= MAX_LAYERS:
                raise ValueError(f"params_for: the same number of ops, 1..{MAX_LAYERS}, for every image")
            for e in entries:
                if e is None:
                    rows.append([0] * ROW)
                    continue
                e = (e,) if isinstance(e, str) else tuple(e)
                if len(e) >= 2 and isinstance(e[1], dict):
                    rows.append(op_row(e[0], e[1]["value"], *(e[2:3] or ("bilinear",)), H=H, W=W))
                    continue
                op, m, sign, filt = (e + (0, 0, "bilinear")[len(e) - 1:])[:4]
                m = check_finite("a magnitude", m)
                if not 0.0 <= m <= LEVEL_DENOM:
                    raise ValueError(f"magnitude {m} outside [0, {LEVEL_DENOM:g}]")
                if sign not in (0, 1):
                    raise ValueError(f"sign is 0 (+) or 1 (-) (got {sign!r})")
                if not isinstance(op, str):
                    raise TypeError(f"an op is a name (got {op!r})")
                rows.append(op_row(op, level_arg(op, m, sign, self.increasing, H, W, self.translate_pct), filt, H=H, W=W))
        if not rows:
            raise ValueError("params_for: no images")
        t = torch.tensor(rows, dtype=torch.int32).view(-1, L, ROW)
        return t if self.device is None else t.to(self.device)
