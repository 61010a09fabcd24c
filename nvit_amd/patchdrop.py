"""Patch dropout (timm's `PatchDropout` / `patch_drop_rate`; FLIP, Li et al. 2023) on the HIP path.

After the position embeddings are added, a training forward keeps a random subset of K = num_keep(T) of the T tokens of
every sample and runs everything downstream - cross-attention, block chain, pooling - on K tokens; evaluation runs on all
T.  `PatchDropout.draw` is one call (nvit_patchdrop_draw) that writes the kept indices `keep` [B,K], ascending, and their
inverse `slot` [B,T]; nvit_rows_gather / nvit_rows_scatter move the rows (model.py: _TokenDropFn).  Like the other draws
it is counter based (Philox4x32-10 over the sample's global index, the step and the token) and its step counter lives on
the device, advanced on the stream behind the draw kernel: a captured train step draws afresh at every replay with no
host code in between, and (seed, step) resumes a run exactly.  DESIGN.md §4 has the semantics.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._lib import call
from .augment import DeviceStepCounter
from .ops import _s

Tensor = torch.Tensor
MAX_TOKENS = _lib.const("PATCHDROP_MAX_TOKENS")


class PatchDropout(DeviceStepCounter):
    """PatchDropout(rate, seed=0, first_index=0).to(device); attach with `model.attach_patch_drop(pd)`.

    rate: the share of the tokens that is dropped, in [0, 1); `num_keep(T)` = max(1, int(T * (1 - rate))) tokens of every
    sample are kept (timm's count), the same number for every sample, in their original order.  The kept tokens are not
    rescaled (timm does not).
    first_index: the global index of this batch's first sample; a data-parallel rank passes rank * B, and the ranks then
    draw what one process would for the whole step's batch."""

    def __init__(self, rate: float, seed: int = 0, first_index: int = 0):
        if isinstance(rate, bool) or not isinstance(rate, (int, float)):
            raise TypeError("rate must be a number")
        if not 0.0 <= rate < 1.0:   # (a NaN fails both comparisons)
            raise ValueError(f"rate must be in [0, 1) (got {rate!r})")
        super().__init__(seed, first_index)
        self.rate = float(rate)

    def to(self, device) -> "PatchDropout":
        self._step_to(device)
        return self

    def num_keep(self, T: int) -> int:
        """Tokens kept of T: max(1, int(T * (1 - rate))), timm's PatchDropout."""
        if isinstance(T, bool) or not isinstance(T, int) or T < 1:
            raise ValueError(f"T must be an int >= 1 (got {T!r})")
        return max(1, int(T * (1.0 - self.rate)))

    def draw(self, B: int, T: int) -> Tuple[Tensor, Tensor]:
        """(keep int32 [B, K], slot int32 [B, T]) of the next step, K = num_keep(T) (nvit_patchdrop_draw); advances the
        step counter.  The call allocates its two outputs, so warm a model up before capturing a graph."""
        self._need_device()
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"PatchDropout.draw: B must be an int >= 1 (got {B!r})")
        if isinstance(T, bool) or not isinstance(T, int) or not 1 <= T <= MAX_TOKENS:
            raise ValueError(f"PatchDropout.draw: T must be an int in 1..{MAX_TOKENS} (got {T!r})")
        K = self.num_keep(T)
        keep = torch.empty((B, K), device=self.device, dtype=torch.int32)
        slot = torch.empty((B, T), device=self.device, dtype=torch.int32)
        call("nvit_patchdrop_draw", self.seed, self._step, self.first_index, keep, slot, B, T, K, _s())
        return keep, slot
