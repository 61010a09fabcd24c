"""What the stages of the device input chain share: the batch-object protocol, the counter of the counter-based draws, and
the argument checks.  augment.py, randaug.py, crop.py and mix.py import this module; it imports none of them.

    mix.batch(erase.batch(aug.batch(rrc.batch(u8)), mean, std))      training: any stage may be left out
    mix.batch(erase.batch(aug.batch(rrc.batch(ld.batch())), mean, std))   the same on a device-resident dataset (data.py)
    rcc.batch(u8)                                                     evaluation

A `stage.batch(X)` is a `StagedBatch`: the stage object together with what it runs on, a tensor or another StagedBatch.
The protocol ("The batch-object protocol") is `resolve`, `rebind`, `source` and `fit_key`; the one legal
nesting order is what the six subclasses declare in `accepts`.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

Tensor = torch.Tensor


# ---------------------------------------------------------------------------------------------- argument checks
def check_number(what: str, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{what} must be a number (got {v!r})")
    return v


def check_finite(what: str, v) -> float:
    if not math.isfinite(check_number(what, v)):
        raise ValueError(f"{what} must be finite (got {v!r})")
    return float(v)


def check_unit(what: str, p, open_top: bool = False) -> float:
    check_number(what, p)
    if not (0.0 <= p < 1.0 if open_top else 0.0 <= p <= 1.0):   # also refuses NaN
        raise ValueError(f"{what} must be in [0, 1{')' if open_top else ']'} (got {p!r})")
    return float(p)


def check_name(what: str, v, names) -> str:
    if not isinstance(v, str):
        raise TypeError(f"{what} is a name: {', '.join(names)} (got {v!r})")
    if v not in names:
        raise ValueError(f"unknown {what} {v!r} (known: {', '.join(names)})")
    return v


def check_sides(name: str, H, W, max_side: int, what: str = "image") -> None:
    if not (isinstance(H, int) and isinstance(W, int) and 1 <= H <= max_side and 1 <= W <= max_side):
        raise ValueError(f"{name}: {what} sides must be 1..{max_side} (got {H}x{W})")


def _check_count(name: str, B: int, max_batch: Optional[int]) -> None:
    if B < 1 or (max_batch is not None and B > max_batch):
        raise ValueError(f"{name}: empty batch" if max_batch is None else f"{name}: a batch holds 1..{max_batch} images (got {B})")


def check_u8_batch(name: str, u8, max_side: int, max_batch: Optional[int] = None, source: bool = False) -> tuple:
    """(B, H, W, C) of a uint8 [B,H,W,C] batch with C 1 or 3, sides up to max_side and, if given, at most max_batch images
    (the second dimension of a grid); source: the words for a stored batch that a crop reads."""
    layout = "[B,Hs,Ws,C]" if source else "[B,H,W,C]"
    if not isinstance(u8, Tensor) or u8.dtype != torch.uint8:
        raise TypeError(f"{name} takes a uint8 {layout} batch")
    if u8.dim() != 4:
        raise ValueError(f"{name} takes a uint8 {layout} batch (got rank {u8.dim()})")
    B, H, W, C = u8.shape
    if C not in (1, 3):
        raise ValueError(f"{name}: C must be 1 or 3 (got {C}; the layout is {layout})")
    _check_count(name, B, max_batch)
    check_sides(name, H, W, max_side, "source" if source else "image")
    return B, H, W, C


def check_f32_batch(name: str, X, max_side: int, max_batch: Optional[int] = None) -> tuple:
    """(B, C, H, W) of a normalised fp32 [B,C,H,W] batch, W % 4 == 0 as of every model input."""
    if not isinstance(X, Tensor) or X.dtype != torch.float32:
        raise TypeError(f"{name} takes an fp32 [B,C,H,W] batch")
    if X.dim() != 4:
        raise ValueError(f"{name} takes an fp32 [B,C,H,W] batch (got rank {X.dim()})")
    B, C, H, W = X.shape
    if C < 1:
        raise ValueError(f"{name}: a batch of at least one channel (got {C})")
    _check_count(name, B, max_batch)
    check_sides(name, H, W, max_side)
    if W % 4:
        raise ValueError(f"{name}: W % 4 == 0 is required (as of every model input)")
    return B, C, H, W


# ---------------------------------------------------------------------------------------------- the draws' counter
class DeviceStepCounter:
    """What the counter-based draws (AutoAugment, Mixup) share: seed, first_index and the step counter, a device int64 that
    the draw kernel advances (a host int until `.to(device)`); `state_dict()` is (seed, step)."""

    def __init__(self, seed: int, first_index: int):
        for what, v, hi in (("seed", seed, 2 ** 64), ("first_index", first_index, 2 ** 62)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"{what} must be an int")
            if not 0 <= v < hi:
                raise ValueError(f"{what} must be in [0, {hi})")
        self.seed, self.first_index = seed, first_index
        self.device: Optional[torch.device] = None
        self._step_host = 0          # until .to(device)
        self._step: Optional[Tensor] = None

    def _step_to(self, device) -> torch.device:   # the common half of `.to(device)`: the counter moves, keeping its count
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the HIP device (no CPU path)")
        step = self.step
        self.device = device
        self._step = torch.tensor([step], dtype=torch.int64).to(device)
        return device

    @property
    def step(self) -> int:
        """Steps drawn so far (reads the device counter: synchronises)."""
        return self._step_host if self._step is None else int(self._step.item())

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        seed, step = int(state["seed"]), int(state["step"])
        if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 63:
            raise ValueError(f"{type(self).__name__}.load_state_dict: seed or step out of range")
        self.seed = seed
        if self._step is None:
            self._step_host = step
        else:
            self._step.fill_(step)   # in place: a captured graph holds this address

    def _need_device(self):
        if self._step is None:
            raise RuntimeError(f"{type(self).__name__}: call .to(device) first (it runs on the HIP device, no CPU path)")


# ---------------------------------------------------------------------------------------------- the batch objects
class StagedBatch:
    """A stage object together with what it runs on inside a step: what every `stage.batch(X)` returns.  A subclass
    declares, as data: `key`, the stage's name in a train step (None: evaluation's transform, no stage of one); `word`,
    what a captured step's refusal calls it; `accepts`, the keys of the batch objects that may stand where its tensor
    stands; `names`, the attributes under which it also shows its stage and what it wraps.  Its constructor checks the
    arguments (a batch object that may not stand inside fails the tensor's check: TypeError) and hands `shape`, that of
    the stage's output, to this one.  `extra`: the further arguments of `stage.batch` (erase.batch's mean, std)."""

    key: Optional[str] = None
    word = ""
    accepts: tuple = ()
    names = ("stage", "inner")

    def __init__(self, stage, inner, shape, extra: tuple = ()):
        self.stage, self.inner, self.extra, self.shape = stage, inner, extra, torch.Size(shape)
        setattr(self, self.names[0], stage)
        setattr(self, self.names[1], inner)

    @classmethod
    def takes(cls, inner) -> bool:
        return isinstance(inner, StagedBatch) and inner.key in cls.accepts

    @property
    def device(self):
        return self.source().device

    def source(self) -> Tensor:
        """The innermost tensor."""
        return self.inner.source() if isinstance(self.inner, StagedBatch) else self.inner

    def fit_key(self) -> tuple:
        """What two batch objects must share for one captured graph to serve both: the stage object itself and `extra`."""
        return (self.stage, *self.extra)

    def rebind(self, tensor: Tensor) -> "StagedBatch":
        """The same chain of the same stage objects around another innermost tensor."""
        return self.stage.batch(self.inner.rebind(tensor) if isinstance(self.inner, StagedBatch) else tensor, *self.extra)

    def labels(self):
        """The labels that the chain itself supplies, as far as a check of them needs (int64 [B]): those of a loader batch
        (data.py), None for a chain around a tensor, whose step is handed its y."""
        return self.inner.labels() if isinstance(self.inner, StagedBatch) else None

    def check_step(self) -> None:
        """Raises if this object cannot be the X of a step by itself."""

    def resolve(self, y=None):
        """(the model's input, the loss's target): every launch of the chain, innermost first, on the current stream."""
        self.check_step()
        return self._launch(y)

    def _launch(self, y):
        x, fresh = self.inner, isinstance(self.inner, StagedBatch)
        if fresh:   # what a stage inside made is a buffer of this call: the stage around it may work in place
            x, y = x._launch(y)
        return self._run(x, y, fresh)

    def _run(self, x: Tensor, y, inplace: bool):
        return self.stage(x), y


def chain(X) -> list:
    """The train-step batch objects of X, outermost first; [] for a tensor (and for evaluation's batch object)."""
    out = []
    while isinstance(X, StagedBatch) and X.key is not None:
        out.append(X)
        X = X.inner
    return out
