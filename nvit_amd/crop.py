"""RandomResizedCrop + horizontal flip and RandomErasing on the device: the per-image geometric half of the DeiT / timm
from-scratch recipe (AutoAugment in augment.py is the augmentation half, Mixup / CutMix in mix.py the batch-level half).

    RandomResizedCrop(224, interpolation="bicubic") -> flip -> AutoAugment -> normalize -> RandomErasing -> Mixup / CutMix
    mix.batch(erase.batch(aug.batch(rrc.batch(u8))))

(`aug` an `AutoAugment`, or the recipes' own `RandAugment` of randaug.py, which has the same interface.)  A stored uint8 [B,Hs,Ws,C] batch becomes the mixed fp32 model input with no host work and no synchronisation, so the
whole chain sits inside a captured train step.  Semantics (tests/crop_ref.py restates them in numpy):

RandomResizedCrop: image b is `PIL.Image.crop(box).resize((size, size), BILINEAR | BICUBIC)`, bit for bit, then mirrored
if its flip bit is set; the box is torchvision's `get_params` (ten attempts, then the central fallback).  Three launches
(nvit_crop_draw, and the two passes of nvit_crop_apply).
RandomErasing: timm's, count 1, per image, on the normalised fp32 batch: a box of `area` x the image at a log-uniform
aspect is overwritten by 0 ("const") or by N(0,1) noise ("pixel").  Two launches (nvit_erase_draw, nvit_erase_apply).

ResizeCenterCrop: evaluation's side of the same pipeline, timm's `transforms_imagenet_eval` for a square target: image b
is `PIL.Image.resize((W2, H2)).crop(window)`, bit for bit, normalised; only the window is computed, nothing is drawn.  Two
launches (nvit_center_crop_apply).  `predict`, `validate`, `estimate_loss` and `GraphedEval` take `rcc.batch(u8)` as X.

Both draws are the counter-based generator of augment.py (Philox4x32-10; counter = (first_index + image, step), key = seed
with the class's own domain constant per attempt in its high word): an image's box depends only on (seed, global index,
step), whatever the batch split.  No transcendental runs on the device: exp(U(log r0, log r1)) comes from a table of
KNOTS + 1 fp64 values that the host computes and the kernel interpolates linearly (`aspect_table`), the noise from a
table of normal quantiles (`normal_quantile_table`).
"""
from __future__ import annotations

import functools
import math
import statistics
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import call
from .augment import MAX_SIDE
from .ops import _chk_dev, _s, normalize_images
from .stages import (DeviceStepCounter, StagedBatch, check_f32_batch, check_finite, check_name, check_number, check_sides,
                     check_u8_batch, check_unit)

Tensor = torch.Tensor

ROW = _lib.const("CROP_ROW")            # ints per row of the crop table: top, left, h, w, flip, 0, 0, 0
KNOTS = _lib.const("CROP_KNOTS")        # the aspect table holds KNOTS + 1 values
ATTEMPTS = _lib.const("CROP_ATTEMPTS")
MAX_SRC = _lib.const("CROP_MAX_SRC")    # largest source side
MAX_BATCH = _lib.const("CROP_MAX_BATCH")   # images per call of the two apply kernels (their grids' second dimension)
INTERPOLATIONS = {"bilinear": _lib.const("CROP_BILINEAR"), "bicubic": _lib.const("CROP_BICUBIC")}
ERASE_ROW = _lib.const("ERASE_ROW")     # on, top, left, h, w, noise key low, noise key high, 0
ERASE_KNOTS = _lib.const("ERASE_KNOTS")
ERASE_MODES = {"const": _lib.const("ERASE_CONST"), "pixel": _lib.const("ERASE_PIXEL")}
NOISE_TAIL = 2.0 ** -15   # the end knots of the normal quantile table: the quantiles at NOISE_TAIL and 1 - NOISE_TAIL
assert KNOTS == ERASE_KNOTS, "one interpolation (10 + 14 bits of a 24-bit uniform) serves both tables"


# ---------------------------------------------------------------------------------------------- host tables (fp64)
@functools.lru_cache(maxsize=None)
def aspect_table(lo: float, hi: float) -> tuple:
    """T[k] = exp(log lo + k / KNOTS * (log hi - log lo)), k = 0..KNOTS, in fp64: what exp(U(log lo, log hi)) is
    interpolated from."""
    l0, l1 = math.log(lo), math.log(hi)
    return tuple(math.exp(l0 + k / KNOTS * (l1 - l0)) for k in range(KNOTS + 1))


def aspect_table_deviation(lo: float, hi: float) -> float:
    """The largest relative deviation of the chord through two neighbouring knots from the exponential it replaces
    (always above it): with d the knots' distance in the logarithm and m = (e^d - 1) / d the chord's slope, the maximum of
    (1 + m t) e^-t - 1 lies at t = (m - 1) / m and is m e^-((m - 1) / m) - 1, about d^2 / 8."""
    d = (math.log(hi) - math.log(lo)) / KNOTS
    if d == 0:
        return 0.0
    m = math.expm1(d) / d
    return m * math.exp(-(m - 1.0) / m) - 1.0


@functools.lru_cache(maxsize=None)
def normal_quantile_table() -> tuple:
    """Q[k] = the k / ERASE_KNOTS quantile of N(0,1), k = 1..ERASE_KNOTS-1, in fp64 (statistics.NormalDist), with the
    finite end knots Q[0] = the NOISE_TAIL quantile = -Q[ERASE_KNOTS]; symmetric: Q[ERASE_KNOTS - k] = -Q[k]."""
    nd = statistics.NormalDist()
    q = [0.0] * (ERASE_KNOTS + 1)
    q[0] = nd.inv_cdf(NOISE_TAIL)
    for k in range(1, ERASE_KNOTS // 2):
        q[k] = nd.inv_cdf(k / ERASE_KNOTS)
    for k in range(ERASE_KNOTS // 2):
        q[ERASE_KNOTS - k] = -q[k]
    return tuple(q)


# ---------------------------------------------------------------------------------------------- argument checks
def _check_range(what: str, r, top: Optional[float] = None) -> tuple:
    try:
        lo, hi = r
    except (TypeError, ValueError):
        raise TypeError(f"{what} is a pair (low, high) (got {r!r})") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"{what} is a pair of numbers (got {r!r})")
    if not (0.0 < lo <= hi < math.inf) or (top is not None and hi > top):   # also refuses NaN
        raise ValueError(f"{what} must be 0 < low <= high{'' if top is None else f' <= {top}'} (got {r!r})")
    return float(lo), float(hi)


def _check_size(size) -> int:
    if isinstance(size, bool) or not isinstance(size, int):
        raise TypeError(f"size must be an int (got {size!r})")
    if not 4 <= size <= MAX_SIDE or size % 4:
        raise ValueError(f"size must be a multiple of 4 in 4..{MAX_SIDE} (got {size})")
    return size


def _check_source(u8, name: str = "RandomResizedCrop") -> tuple:
    return check_u8_batch(name, u8, MAX_SRC, MAX_BATCH, source=True)


def _check_src_hw(Hs, Ws, name: str = "RandomResizedCrop") -> None:
    check_sides(name, Hs, Ws, MAX_SRC, "source")


def _check_f32(X) -> tuple:
    return check_f32_batch("RandomErasing", X, MAX_SIDE, MAX_BATCH)


def _check_hw(H, W) -> None:
    check_sides("RandomErasing", H, W, MAX_SIDE)


# ---------------------------------------------------------------------------------------------- RandomResizedCrop
class CroppedBatch(StagedBatch):
    """A stored uint8 [B,Hs,Ws,C] batch together with the RandomResizedCrop that cuts it: what `rrc.batch(u8)` returns
    and `AutoAugment.batch` / `RandomErasing.batch` accept in place of a tensor.  u8: the tensor, or a `DeviceLoader.batch()`
    (data.py) whose gathered batch is then what is cut.  `.shape` is that of its output."""

    key, word, accepts, names = "crop", "RandomResizedCrop", ("data",), ("crop", "u8")

    def __init__(self, crop: "RandomResizedCrop", u8):
        if self.takes(u8):   # a loader's batch (data.py): the gathered [B,Hs,Ws,C]
            B, Hs, Ws, C = u8.shape
            if B > MAX_BATCH:
                raise ValueError(f"RandomResizedCrop: a batch holds 1..{MAX_BATCH} images (got {B})")
            _check_src_hw(Hs, Ws)
        else:
            B, _, _, C = _check_source(u8)
        super().__init__(crop, u8, (B, crop.size, crop.size, C))

    def check_step(self) -> None:
        raise TypeError("a RandomResizedCrop.batch(u8) is uint8: wrap it in AutoAugment.batch or RandomErasing.batch")

    def cropped(self) -> Tensor:
        return self._launch(None)[0]


class RandomResizedCrop(DeviceStepCounter):
    """RandomResizedCrop(size, scale=(0.08, 1.0), ratio=(3/4, 4/3), interpolation="bilinear", hflip=0.5, seed=0,
    first_index=0).to(device)

    torchvision's RandomResizedCrop followed by RandomHorizontalFlip(hflip), on a uint8 [B,Hs,Ws,C] batch (C 1 or 3, one
    source size per batch): uint8 [B,size,size,C] out, image b Pillow's crop(box).resize((size, size)) bit for bit.
    size: a multiple of 4 up to MAX_SIDE (the fp32 stages behind it need W % 4 == 0); source sides up to MAX_SRC.
    first_index: the global index of this batch's first image in the step; a data-parallel rank passes rank * B.

    `rrc(u8)` draws the step's boxes and returns the crops; `draw` and `apply` are its halves; `params_for` writes a
    table by hand.  The step counter lives on the device and the draw kernel advances it, so a captured graph that
    contains the call draws fresh boxes at every replay."""

    def __init__(self, size: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation: str = "bilinear",
                 hflip: float = 0.5, seed: int = 0, first_index: int = 0):
        self.size = _check_size(size)
        self.scale, self.ratio = _check_range("scale", scale), _check_range("ratio", ratio)
        self.interpolation = check_name("interpolation", interpolation, INTERPOLATIONS)
        self.hflip = check_unit("hflip", hflip)
        super().__init__(seed, first_index)
        self._aspect: Optional[Tensor] = None

    def to(self, device) -> "RandomResizedCrop":
        device = self._step_to(device)
        self._aspect = torch.tensor(aspect_table(*self.ratio), dtype=torch.float64).to(device)
        return self

    # ------------------------------------------------------------------ the launches
    def draw(self, B: int, Hs: int, Ws: int) -> Tensor:
        """int32 [B,8] table of the next step (nvit_crop_draw): top, left, h, w, flip; advances the step counter."""
        self._need_device()
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError("RandomResizedCrop.draw: B must be an int >= 1")
        _check_src_hw(Hs, Ws)
        table = torch.empty((B, ROW), device=self.device, dtype=torch.int32)
        call("nvit_crop_draw", self.seed, self._step, self.first_index, self._aspect, self.scale[0], self.scale[1],
             self.ratio[0], self.ratio[1], self.hflip, table, B, Hs, Ws, _s())
        return table

    def apply(self, u8: Tensor, table: Tensor) -> Tensor:
        """uint8 [B,size,size,C]: the box of table[b] of image b, resized and flipped (nvit_crop_apply, two launches).  A
        row whose box leaves the image counts as the whole image."""
        B, Hs, Ws, C = _check_source(u8)
        if not isinstance(table, Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (B, ROW):
            raise ValueError(f"RandomResizedCrop.apply: the table must be int32 [{B},{ROW}]")
        _chk_dev(u8, table)
        u8, table = u8.contiguous(), table.contiguous()
        interp = INTERPOLATIONS[self.interpolation]
        ws_bytes = _lib.load().nvit_crop_ws_bytes(B, Hs, Ws, C, self.size, interp)   # taps + the [Hs,size,C] intermediates
        if ws_bytes < 0:
            raise ValueError(f"RandomResizedCrop.apply: unsupported shape {tuple(u8.shape)} -> {self.size}")
        ws = torch.empty(ws_bytes, device=u8.device, dtype=torch.uint8)
        out = torch.empty((B, self.size, self.size, C), device=u8.device, dtype=torch.uint8)
        call("nvit_crop_apply", u8, table, out, ws, ws_bytes, B, Hs, Ws, C, self.size, interp, _s())
        return out

    def __call__(self, u8: Tensor) -> Tensor:
        B, Hs, Ws, _ = _check_source(u8)
        _chk_dev(u8)
        return self.apply(u8, self.draw(B, Hs, Ws))

    def batch(self, u8: Tensor) -> CroppedBatch:
        """What `AutoAugment.batch` / `RandomErasing.batch` take in place of a tensor: the crop then runs inside the
        step (and inside its captured graph), once per batch."""
        return CroppedBatch(self, u8)

    # ------------------------------------------------------------------ tables by hand
    def params_for(self, boxes: Sequence, flips: Optional[Sequence] = None) -> Tensor:
        """int32 [B,8] from boxes[b] = (top, left, h, w) and flips[b] (default: none), as the draw writes them."""
        boxes = [tuple(int(v) for v in box) for box in boxes]
        if not boxes or any(len(box) != 4 for box in boxes):
            raise ValueError("params_for: one (top, left, h, w) per image")
        flips = [0] * len(boxes) if flips is None else [1 if f else 0 for f in flips]
        if len(flips) != len(boxes):
            raise ValueError("params_for: one flip per box")
        t = torch.tensor([[*box, f, 0, 0, 0] for box, f in zip(boxes, flips)], dtype=torch.int32)
        return t if self.device is None else t.to(self.device)


# ---------------------------------------------------------------------------------------------- Resize + CenterCrop
CROP_MODES = ("center", "squash")


class CenterCroppedBatch(StagedBatch):
    """A stored uint8 [B,Hs,Ws,C] batch together with the ResizeCenterCrop that cuts it: what `rcc.batch(u8)` returns and
    `predict`, `validate`, `estimate_loss` and `GraphedEval` accept in place of X.  `.shape` is that of the model input,
    [B,C,size,size].  Two of them fit one captured graph if their transforms' parameters are equal."""

    key, word, accepts, names = None, "ResizeCenterCrop", (), ("crop", "u8")

    def __init__(self, crop: "ResizeCenterCrop", u8: Tensor):
        B, _, _, C = crop._check_source(u8)
        super().__init__(crop, u8, (B, C, crop.size, crop.size))

    def fit_key(self) -> tuple:
        return self.crop.params()

    def cropped(self) -> Tensor:
        """The fp32 model input: the transform's two launches on the current stream."""
        return self._launch(None)[0]


class ResizeCenterCrop:
    """ResizeCenterCrop(size, crop_pct=0.875, interpolation="bilinear", crop_mode="center", mean=0.5, std=0.5)

    timm's `transforms_imagenet_eval` for a square target, on a uint8 [B,Hs,Ws,C] batch (C 1 or 3, one source size per
    batch): Resize to scale_size = floor(size / crop_pct) (crop_mode "center": the shorter side, aspect kept, torchvision's
    Resize(int); "squash": both sides), CenterCrop(size), ToTensor, Normalize(mean, std).  Image b is Pillow's
    resize((W2, H2)).crop(window) bit for bit, normalised with `ops.normalize_images`' arithmetic; only the window is
    computed (nvit_center_crop_apply, two launches).  size: a multiple of 4 up to MAX_SIDE; source sides up to MAX_SRC.

    Stateless: nothing is drawn and nothing lives on the device, so there is no `.to()` and no `state_dict`.
    `rcc(u8)` returns the fp32 [B,C,size,size] model input, `rcc(u8, return_u8=True)` the uint8 [B,size,size,C] crop;
    `geometry` is the host arithmetic, `apply` the raw window."""

    def __init__(self, size: int, crop_pct: float = 0.875, interpolation: str = "bilinear", crop_mode: str = "center",
                 mean: float = 0.5, std: float = 0.5):
        _check_size(size)
        if not 0.0 < check_number("crop_pct", crop_pct) <= 1.0:   # also refuses NaN
            raise ValueError(f"crop_pct must be in (0, 1] (got {crop_pct!r})")
        check_name("interpolation", interpolation, INTERPOLATIONS)
        check_name("crop_mode", crop_mode, CROP_MODES)
        check_number("std", std)
        check_finite("mean", mean)
        if not 0.0 < std < math.inf:   # also refuses NaN
            raise ValueError(f"std must be positive (got {std!r})")
        self.size, self.crop_pct, self.interpolation, self.crop_mode = size, float(crop_pct), interpolation, crop_mode
        self.mean, self.std = float(mean), float(std)
        self.scale_size = math.floor(size / crop_pct)

    def params(self) -> tuple:
        """What two transforms must share to give the same output on the same source."""
        return self.size, self.crop_pct, self.interpolation, self.crop_mode, self.mean, self.std

    # ------------------------------------------------------------------ host arithmetic
    def geometry(self, Hs: int, Ws: int) -> tuple:
        """(H2, W2, top, left): the size the source is resized to and the window's corner in it.  torchvision's
        Resize(scale_size) / Resize((scale_size, scale_size)) and center_crop: int() truncates, round() is Python's (half
        to even)."""
        _check_src_hw(Hs, Ws, "ResizeCenterCrop")
        s = self.scale_size
        if self.crop_mode == "squash":
            H2 = W2 = s
        elif Ws <= Hs:
            H2, W2 = int(s * Hs / Ws), s
        else:
            H2, W2 = s, int(s * Ws / Hs)
        if H2 > MAX_SIDE or W2 > MAX_SIDE:
            raise ValueError(f"ResizeCenterCrop: a {Hs}x{Ws} source is resized to {H2}x{W2}; sides up to {MAX_SIDE}")
        return H2, W2, int(round((H2 - self.size) / 2.0)), int(round((W2 - self.size) / 2.0))

    def _check_source(self, u8) -> tuple:
        B, Hs, Ws, C = _check_source(u8, "ResizeCenterCrop")
        self.geometry(Hs, Ws)   # raises for a source it cannot take
        return B, Hs, Ws, C

    # ------------------------------------------------------------------ the launches
    def apply(self, u8: Tensor, H2: int, W2: int, top: int, left: int, return_u8: bool = False, both: bool = False):
        """The size x size window at (top, left) of every image resized to [H2,W2] (nvit_center_crop_apply, two launches):
        fp32 [B,C,size,size] normalised, uint8 [B,size,size,C] with return_u8, (fp32, uint8) from the one call with both."""
        B, Hs, Ws, C = self._check_source(u8)
        for what, v in (("H2", H2), ("W2", W2), ("top", top), ("left", left)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"ResizeCenterCrop.apply: {what} must be an int (got {v!r})")
        if not (self.size <= H2 <= MAX_SIDE and self.size <= W2 <= MAX_SIDE):
            raise ValueError(f"ResizeCenterCrop.apply: H2 and W2 must be {self.size}..{MAX_SIDE} (got {H2}x{W2})")
        if not (0 <= top <= H2 - self.size and 0 <= left <= W2 - self.size):
            raise ValueError(f"ResizeCenterCrop.apply: the window at ({top}, {left}) leaves the {H2}x{W2} image")
        _chk_dev(u8)
        u8 = u8.contiguous()
        interp, size = INTERPOLATIONS[self.interpolation], self.size
        ws_bytes = _lib.load().nvit_center_crop_ws_bytes(B, Hs, Ws, C, H2, W2, top, left, size, interp)
        if ws_bytes < 0:
            raise ValueError(f"ResizeCenterCrop.apply: unsupported shape {tuple(u8.shape)} -> {H2}x{W2} -> {size}")
        ws = torch.empty(ws_bytes, device=u8.device, dtype=torch.uint8)   # taps + the [rows read,size,C] intermediates
        o8 = torch.empty((B, size, size, C), device=u8.device, dtype=torch.uint8) if return_u8 or both else None
        of = torch.empty((B, C, size, size), device=u8.device, dtype=torch.float32) if both or not return_u8 else None
        call("nvit_center_crop_apply", u8, o8, of, ws, ws_bytes, B, Hs, Ws, C, H2, W2, top, left, size, interp, self.mean,
             self.std, _s())
        return (of, o8) if both else (o8 if return_u8 else of)

    def __call__(self, u8: Tensor, return_u8: bool = False):
        _, Hs, Ws, _ = self._check_source(u8)
        return self.apply(u8, *self.geometry(Hs, Ws), return_u8=return_u8)

    def batch(self, u8: Tensor) -> CenterCroppedBatch:
        """The X of `predict`, `validate`, `estimate_loss` and `GraphedEval`: the transform then runs in front of the
        forward (and inside its captured graph)."""
        return CenterCroppedBatch(self, u8)


# ---------------------------------------------------------------------------------------------- RandomErasing
class ErasedBatch(StagedBatch):
    """A batch together with the RandomErasing that runs on it inside the step: what `erase.batch(X)` returns and
    `Mixup.batch`, `train_step` and `GraphedTrainStep` accept in place of X.  X: an fp32 [B,C,H,W] tensor, an
    `AutoAugment.batch(...)`, or a `RandomResizedCrop.batch(u8)` (then normalised with mean, std by
    `ops.normalize_images`' kernel)."""

    key, word, accepts, names = "erase", "RandomErasing", ("augment", "crop"), ("erase", "X")

    def __init__(self, erase: "RandomErasing", X, mean: float = 0.5, std: float = 0.5):
        if self.takes(X):
            B, H, W, C = X.shape
            _check_hw(H, W)
            if W % 4:
                raise ValueError("RandomErasing: W % 4 == 0 is required (as of every model input)")
            shape = (B, C, H, W)
        else:
            shape = _check_f32(X)
        if std == 0:
            raise ValueError("std must not be 0")
        self.mean, self.std = float(mean), float(std)
        super().__init__(erase, X, shape, (self.mean, self.std))

    def _run(self, x: Tensor, y, inplace: bool):
        if x.dtype == torch.uint8:   # a crop's output: normalised here
            x = normalize_images(x, self.mean, self.std)
        return self.erase(x, inplace=inplace), y

    def erased(self) -> Tensor:
        """The launches of what X carries, then the draw and the apply; in place on a buffer made here."""
        return self._launch(None)[0]


class RandomErasing(DeviceStepCounter):
    """RandomErasing(prob=0.25, area=(0.02, 1/3), aspect=(0.3, 1/0.3), mode="pixel", seed=0, first_index=0).to(device)

    timm's RandomErasing with count 1, per image, on the normalised fp32 [B,C,H,W] batch: with probability `prob` a box
    of `area` x the image at a log-uniform aspect h/w in `aspect` is overwritten in every channel, by 0.0 ("const": the
    mean after the normalise) or by per-element N(0,1) noise ("pixel").  Ten attempts to fit the box (w < W and h < H),
    then nothing is erased.  first_index: as for RandomResizedCrop.

    `erase(X)` returns the erased batch (a new tensor unless `inplace`); `draw` and `apply` are its halves; `params_for`
    writes a table by hand."""

    def __init__(self, prob: float = 0.25, area=(0.02, 1.0 / 3.0), aspect=(0.3, 1.0 / 0.3), mode: str = "pixel",
                 seed: int = 0, first_index: int = 0):
        self.prob = check_unit("prob", prob)
        self.area, self.aspect = _check_range("area", area, top=1.0), _check_range("aspect", aspect)
        self.mode = check_name("mode", mode, ERASE_MODES)
        super().__init__(seed, first_index)
        self._aspect: Optional[Tensor] = None
        self._q: Optional[Tensor] = None

    def to(self, device) -> "RandomErasing":
        device = self._step_to(device)
        self._aspect = torch.tensor(aspect_table(*self.aspect), dtype=torch.float64).to(device)
        self._q = torch.tensor(normal_quantile_table(), dtype=torch.float64).to(torch.float32).to(device)
        return self

    def draw(self, B: int, H: int, W: int) -> Tensor:
        """int32 [B,8] table of the next step (nvit_erase_draw): on, top, left, h, w, the image's noise sub-key; advances
        the step counter."""
        self._need_device()
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError("RandomErasing.draw: B must be an int >= 1")
        _check_hw(H, W)
        table = torch.empty((B, ERASE_ROW), device=self.device, dtype=torch.int32)
        call("nvit_erase_draw", self.seed, self._step, self.first_index, self._aspect, self.area[0], self.area[1], self.prob,
             table, B, H, W, _s())
        return table

    def apply(self, X: Tensor, table: Tensor, inplace: bool = False) -> Tensor:
        """The erased fp32 [B,C,H,W] batch (nvit_erase_apply).  Out of place unless `inplace` (then X itself is returned,
        erased): a caller's tensor is never modified behind their back."""
        B, C, H, W = _check_f32(X)
        if not isinstance(table, Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (B, ERASE_ROW):
            raise ValueError(f"RandomErasing.apply: the table must be int32 [{B},{ERASE_ROW}]")
        self._need_device()
        _chk_dev(X, table)
        if inplace and not X.is_contiguous():
            raise ValueError("RandomErasing.apply: in place needs a contiguous batch")
        X, table = X.contiguous(), table.contiguous()
        out = X if inplace else torch.empty_like(X)
        call("nvit_erase_apply", X, table, self._q, out, ERASE_MODES[self.mode], B, C, H, W, _s())
        return out

    def __call__(self, X: Tensor, inplace: bool = False) -> Tensor:
        B, _, H, W = _check_f32(X)
        _chk_dev(X)
        return self.apply(X, self.draw(B, H, W), inplace=inplace)

    def batch(self, X, mean: float = 0.5, std: float = 0.5) -> ErasedBatch:
        """The X of `train_step(model, optimizer, erase.batch(X), y)`, of `GraphedTrainStep` and of `Mixup.batch`.  X: fp32
        [B,C,H,W], an `AutoAugment.batch(...)`, or a `RandomResizedCrop.batch(u8)`; mean and std serve the last."""
        return ErasedBatch(self, X, mean, std)

    def params_for(self, boxes: Sequence, keys: Optional[Sequence] = None) -> Tensor:
        """int32 [B,8] from boxes[b] = (top, left, h, w) or None (not erased) and keys[b] = the image's 64-bit noise
        sub-key (default b), as the draw writes them."""
        boxes = list(boxes)
        if not boxes:
            raise ValueError("params_for: no images")
        keys = list(range(len(boxes))) if keys is None else [int(k) for k in keys]
        if len(keys) != len(boxes):
            raise ValueError("params_for: one key per box")

        def i32(v):
            v &= 0xFFFFFFFF
            return v - (1 << 32) if v >= 1 << 31 else v

        rows = []
        for box, key in zip(boxes, keys):
            on, box = (0, (0, 0, 0, 0)) if box is None else (1, tuple(int(v) for v in box))
            if len(box) != 4:
                raise ValueError("params_for: a box is (top, left, h, w) or None")
            rows.append([on, *box, i32(key), i32(key >> 32), 0])
        t = torch.tensor(rows, dtype=torch.int32)
        return t if self.device is None else t.to(self.device)
