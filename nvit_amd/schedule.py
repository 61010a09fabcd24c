"""Learning-rate schedule on the device: warm-up, then cosine / linear decay or a constant rate, and layer-wise lr decay.

The reference trainer rewrites `param_group["lr"] = get_lr(iter_num)` on the host before every step (train.py:874-876,
get_lr at :1025-1035).  Here a schedule is an object attached to the optimizer (`FusedAdamW.attach_schedule`), like a
`ModelEma`: its step counter is a device int64, and one small launch per optimizer step (nvit_lr_schedule) evaluates L(s)
in fp64 and writes (float)(L(s) * lr_scale) into the lr half of every row of the table the update kernel reads.  A
captured train step therefore follows the schedule at every replay with no host code in between, and (parameters, step)
resumes a run exactly.  `lr_at` restates L on the host, operation for operation.  DESIGN.md §4 has the semantics.

`layer_decay_groups` builds the param groups of layer-wise lr decay (BEiT, MAE, timm --layer-decay): every group carries
its depth's multiplier as `lr_scale`, which the launch applies per row.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import _lib, ops
from .augment import DeviceStepCounter

Tensor = torch.Tensor
KINDS = {"cosine": _lib.const("LR_COSINE"), "linear": _lib.const("LR_LINEAR"), "constant": _lib.const("LR_CONSTANT")}
THREADS = _lib.const("LR_SCHEDULE_THREADS")   # the launch's one workgroup; a table of more rows takes several passes


def _rate(what: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{what} must be a number")
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0 (got {v!r})")
    return v


def _iters(what: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{what} must be an int")
    if not 0 <= v < 2 ** 62:
        raise ValueError(f"{what} must be in [0, 2**62) (got {v!r})")
    return v


class LRSchedule(DeviceStepCounter):
    """LRSchedule(kind, lr, min_lr=0.0, warmup_iters=0, decay_iters=None, warmup_init=0.0).to(device); attach with
    `optimizer.attach_schedule(sched)`.

    kind: "cosine", "linear" or "constant".  With s = optimizer steps attempted so far (from 0; a step that skip_nonfinite
    leaves out counts, as the reference's iter_num does), W = warmup_iters, D = decay_iters:

        s <  W : warmup_init + (lr - warmup_init) * s / W
        s >  D : min_lr
        else   : r = (s - W) / (D - W)
          cosine : min_lr + (0.5 * (1.0 + cos(pi * r))) * (lr - min_lr)
          linear : lr + (min_lr - lr) * r
        constant : lr after the warm-up (min_lr and decay_iters are ignored)

    in fp64, in exactly this operation order.  cosine with warmup_init = 0 is the reference's get_lr (`from_reference`).
    Needs W >= 0, D > W for cosine and linear, finite rates >= 0 (ValueError otherwise, before any device work).

    `step` reads the device counter (synchronises); `last_lr` is the fp32 device tensor [1] holding the L of the last
    launch, for logging with no synchronisation (`last_lr64`: the same in fp64)."""

    def __init__(self, kind: str, lr: float, min_lr: float = 0.0, warmup_iters: int = 0,
                 decay_iters: Optional[int] = None, warmup_init: float = 0.0):
        super().__init__(0, 0)
        self._set(kind, lr, min_lr, warmup_iters, decay_iters, warmup_init)
        self._last: Optional[Tensor] = None
        self._last64: Optional[Tensor] = None

    def _set(self, kind, lr, min_lr, warmup_iters, decay_iters, warmup_init) -> None:
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)} (got {kind!r})")
        lr, min_lr, warmup_init = _rate("lr", lr), _rate("min_lr", min_lr), _rate("warmup_init", warmup_init)
        W = _iters("warmup_iters", warmup_iters)
        if kind == "constant":
            D = 0 if decay_iters is None else _iters("decay_iters", decay_iters)
        else:
            if decay_iters is None:
                raise ValueError(f"kind {kind!r} needs decay_iters")
            D = _iters("decay_iters", decay_iters)
            if D <= W:
                raise ValueError(f"decay_iters must be > warmup_iters (got {D} <= {W})")
        self.kind, self.lr, self.min_lr, self.warmup_init = kind, lr, min_lr, warmup_init
        self.warmup_iters, self.decay_iters = W, D

    @classmethod
    def from_reference(cls, learning_rate: float, min_lr: float, warmup_iters: int, lr_decay_iters: int) -> "LRSchedule":
        """The reference trainer's get_lr (train.py:1025-1035) from its four `optimizer.*` settings."""
        return cls("cosine", learning_rate, min_lr, warmup_iters, lr_decay_iters, 0.0)

    # ------------------------------------------------------------------ host restatement
    def lr_at(self, s: int) -> float:
        """L(s) in Python floats (fp64), the operations of the kernel in the kernel's order."""
        W, D, lr, min_lr = self.warmup_iters, self.decay_iters, self.lr, self.min_lr
        if s < W:
            return self.warmup_init + (lr - self.warmup_init) * s / W
        if self.kind == "constant":
            return lr
        if s > D:
            return min_lr
        r = (s - W) / (D - W)
        if self.kind == "cosine":
            return min_lr + (0.5 * (1.0 + math.cos(math.pi * r))) * (lr - min_lr)
        return lr + (min_lr - lr) * r

    # ------------------------------------------------------------------ device state
    def to(self, device) -> "LRSchedule":
        device = self._step_to(device)
        self._last = torch.zeros(1, device=device, dtype=torch.float32)
        self._last64 = torch.zeros(1, device=device, dtype=torch.float64)
        return self

    @property
    def last_lr(self) -> Tensor:
        self._need_device()
        return self._last

    @property
    def last_lr64(self) -> Tensor:
        self._need_device()
        return self._last64

    def apply(self, table: Optional[Tensor] = None, n: int = 0, lr_scale: Optional[Tensor] = None) -> None:
        """The launch (nvit_lr_schedule) on the current stream: this step's lr into the n rows of an optimizer table
        (int64 [n, NVIT_OPT_TABLE_COLS]; lr_scale fp32 [n]), `last_lr`, and the counter advances by one.  With no table
        only the counter and `last_lr` move: a stand-alone schedule, stepped by hand."""
        self._need_device()
        ops.lr_schedule(table, n, lr_scale, self._step, KINDS[self.kind], self.lr, self.min_lr, self.warmup_init,
                        self.warmup_iters, self.decay_iters, self._last, self._last64)

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        return {"kind": self.kind, "lr": self.lr, "min_lr": self.min_lr, "warmup_iters": self.warmup_iters,
                "decay_iters": self.decay_iters, "warmup_init": self.warmup_init, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        """In place: a captured graph holds the counter's address (the parameters travel by value with every launch, so
        a graph captured before the load keeps the ones it was captured with)."""
        step = int(state["step"])
        if not 0 <= step < 2 ** 62:
            raise ValueError("LRSchedule.load_state_dict: step out of range")
        self._set(state["kind"], state["lr"], state["min_lr"], int(state["warmup_iters"]),
                  None if state["decay_iters"] is None else int(state["decay_iters"]), state["warmup_init"])
        if self._step is None:
            self._step_host = step
        else:
            self._step.fill_(step)


def param_depth(name: str, n_layer: int) -> int:
    """Depth of a ViT parameter for layer-wise lr decay: patch embeddings and position tables 0, the cross-attention
    block 1, transformer.h[i] i + 2, everything else (head, sz, Kohonen and reconstruction parameters) n_layer + 2."""
    if name.startswith(("local_patch_embed.", "global_patch_embed.")) or name in ("local_pos_embed", "global_pos_embed"):
        return 0
    if name.startswith("cross_attention."):
        return 1
    if name.startswith("transformer.h."):
        return int(name.split(".")[2]) + 2
    return n_layer + 2


def layer_decay_groups(model, weight_decay: float, learning_rate: float, layer_decay: float) -> List[Dict]:
    """Param groups for FusedAdamW with layer-wise lr decay: the decay / no-decay / sz split of
    `ViT.configure_optimizers`, each further split by `param_depth`.  A group of depth d carries lr_scale = layer_decay **
    (n_layer + 2 - d), which an attached LRSchedule multiplies into every step's lr, and lr = learning_rate * lr_scale,
    so the groups are also right with no schedule attached.  Empty groups are left out."""
    if isinstance(layer_decay, bool) or not isinstance(layer_decay, (int, float)):
        raise TypeError("layer_decay must be a number")
    if not (math.isfinite(layer_decay) and layer_decay > 0.0):
        raise ValueError(f"layer_decay must be finite and > 0 (got {layer_decay!r})")
    m = model.module if hasattr(model, "module") else model
    n_layer = m.config.n_layer
    pd = {n: p for n, p in m.named_parameters() if p.requires_grad}
    if m.config.use_nvit:
        base = [([n for n, p in pd.items() if "sz" not in n and p.dim() >= 2], weight_decay),
                ([n for n, p in pd.items() if "sz" not in n and p.dim() < 2], 0.0),
                (["sz"], 0.0)]
    else:
        base = [([n for n, p in pd.items() if p.dim() >= 2], weight_decay),
                ([n for n, p in pd.items() if p.dim() < 2], 0.0)]
    groups = []
    for names, wd in base:
        for depth in range(n_layer + 3):
            params = [pd[n] for n in names if param_depth(n, n_layer) == depth]
            if params:
                scale = float(layer_decay) ** (n_layer + 2 - depth)
                groups.append({"params": params, "weight_decay": wd, "lr_scale": scale, "lr": learning_rate * scale,
                               "depth": depth})
    return groups
