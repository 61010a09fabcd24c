"""Stochastic depth (DropPath; Huang et al. 2016, as timm builds it into every ViT block) on the HIP path.

One gate per sample, block and branch (0 attention, 1 MLP): 0.0 when the branch is dropped for that sample, else 1.0, or
1 / keep with scale_by_keep.  `DropPath.draw` is one launch (nvit_droppath_draw) that writes the whole fp32 table
[2*n_layer, B]; the row kernels read row 2*l + br for block l (their `gate` argument: nvit_lerp_*, nvit_res_*).  Like the
input pipeline's draws it is counter based (Philox4x32-10 over the sample's global index, the step and the row) and its
step counter lives on the device, advanced by the draw kernel: a captured train step draws afresh at every replay with
no host code in between, and (seed, step) resumes a run exactly.  DESIGN.md §4 has the semantics.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import call
from .augment import DeviceStepCounter
from .ops import _s

Tensor = torch.Tensor
MAX_GATES = _lib.const("DROPPATH_MAX_GATES")


class DropPath(DeviceStepCounter):
    """DropPath(rate, seed=0, first_index=0, scale_by_keep=None).to(device); attach with `model.attach_drop_path(dp)`.

    rate: the drop probability of the LAST block, in [0, 1); block l of n_layer drops each of its two branches with
    p_l = rate * l / (n_layer - 1) (timm's linspace(0, rate, depth); a single block never drops), independently per
    sample and branch.
    scale_by_keep: a kept branch is scaled by 1 / (1 - p_l).  None resolves when attached: True for the plain ViT (timm's
    behaviour), False for nViT, where the gate scales the step of a LERP between unit vectors that is re-normalised
    afterwards - the expectation argument behind 1 / keep does not survive that, and lam / keep is just another step size.
    first_index: the global index of this batch's first sample; a data-parallel rank passes rank * B, and the ranks then
    draw what one process would for the whole step's batch."""

    def __init__(self, rate: float, seed: int = 0, first_index: int = 0, scale_by_keep: Optional[bool] = None):
        if isinstance(rate, bool) or not isinstance(rate, (int, float)):
            raise TypeError("rate must be a number")
        if not 0.0 <= rate < 1.0:   # (a NaN fails both comparisons)
            raise ValueError(f"rate must be in [0, 1) (got {rate!r})")
        if scale_by_keep is not None and not isinstance(scale_by_keep, bool):
            raise TypeError("scale_by_keep must be True, False or None")
        super().__init__(seed, first_index)
        self.rate = float(rate)
        self.scale_by_keep = scale_by_keep
        self._rates_dev: Dict[int, Tensor] = {}

    def to(self, device) -> "DropPath":
        self._step_to(device)
        self._rates_dev = {}
        return self

    def rates(self, n_layer: int) -> np.ndarray:
        """fp32 [n_layer]: p_l = rate * l / (n_layer - 1), computed in fp64 and rounded once; [0] for one layer."""
        if isinstance(n_layer, bool) or not isinstance(n_layer, int) or n_layer < 1:
            raise ValueError(f"n_layer must be an int >= 1 (got {n_layer!r})")
        if n_layer == 1:
            return np.zeros(1, dtype=np.float32)
        return np.linspace(0.0, self.rate, n_layer).astype(np.float32)

    def _rates(self, n_layer: int) -> Tensor:
        t = self._rates_dev.get(n_layer)
        if t is None:
            t = self._rates_dev[n_layer] = torch.from_numpy(self.rates(n_layer)).to(self.device)
        return t

    def draw(self, n_layer: int, B: int) -> Tensor:
        """fp32 [2*n_layer, B] gate table of the next step (nvit_droppath_draw); advances the step counter.  The first
        call at a new n_layer uploads its rates, so warm a model up before capturing a graph.  A scale_by_keep of None
        (never attached to a model) draws unscaled gates."""
        self._need_device()
        if isinstance(B, bool) or not isinstance(B, int) or B < 1 or 2 * n_layer * B > MAX_GATES:
            raise ValueError(f"DropPath.draw: B must be an int >= 1 with 2 * n_layer * B <= {MAX_GATES}")
        rates = self._rates(n_layer)
        table = torch.empty((2 * n_layer, B), device=self.device, dtype=torch.float32)
        call("nvit_droppath_draw", self.seed, self._step, self.first_index, rates, int(bool(self.scale_by_keep)), table,
             n_layer, B, _s())
        return table
