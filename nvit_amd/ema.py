"""Exponential moving average of the weights (`--model-ema` of the DeiT / timm recipe, timm's ModelEmaV2) on the device.

    ema = ModelEma(model)            # decay 0.9998, timm's warm-up min(decay, (1 + t) / (10 + t))
    optimizer.attach_ema(ema)        # before a GraphedTrainStep is built: the captured step then holds the update
    ...train_step / GraphedTrainStep calls...
    validate(ema.module, batches)    # a ready-to-evaluate ViT

One optimizer step is one update, two launches (nvit_ema_tick, nvit_ema_update) over a device table built here; the
update count and the factor of the update about to run live on the device, so a replayed step updates the average with
no host work, and a step that `skip_nonfinite` left out leaves the average bit-identical (the tick reads the optimizer's
own skip state).

The shadow is one flat fp32 buffer that holds the plain linear average e <- e + (1 - d)(p - e) of every floating-point
parameter (the SOM nodes among them; a parameter that never changes comes back bit for bit, since p == e gives e).
For a plain ViT `ema.module`'s parameters are views of that buffer.  An nViT forward assumes unit-norm matrices, which a
linear average of unit vectors is not: there `ema.module` owns its tensors, and `sync()` copies the shadow into them
(one launch of the same kernel) and runs `normalize_matrices` on the module.  The shadow keeps the exact recurrence; what
is evaluated is its projection back onto the sphere.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import ops
from .train import _unwrap, normalize_matrices

Tensor = torch.Tensor


class ModelEma:
    def __init__(self, model, decay: float = 0.9998, warmup: bool = True, renorm: Optional[bool] = None):
        """model: a ViT on the HIP device (or its data-parallel wrapper: every rank averages the same weights).
        decay in [0, 1); warmup: d = min(decay, (1 + t) / (10 + t)) at update t (counted from 0).  renorm: `module`
        carries re-normalised copies of the average (default: model.config.use_nvit)."""
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"ModelEma: decay must lie in [0, 1) (got {decay!r})")
        m = _unwrap(model)
        dev = next(m.parameters()).device
        if dev.type != "cuda":
            m._prepare(dev)   # raises the model's own error, before anything is allocated
        self.model = m
        self.decay, self.warmup = float(decay), bool(warmup)
        self.renorm = bool(m.config.use_nvit) if renorm is None else bool(renorm)
        self._names = [n for n, p in m.named_parameters() if p.is_floating_point()]
        params = self._params()
        offs, total = [], 0
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("ModelEma: parameters must be contiguous fp32 tensors on the HIP device")
            offs.append(total)
            total += ops.round_up(p.numel(), 4)   # every entry starts 16-byte aligned
        self._flat = torch.zeros(total, device=dev, dtype=torch.float32)
        self._shadow: Dict[str, Tensor] = {n: self._flat[o:o + p.numel()].view(p.shape)
                                           for n, o, p in zip(self._names, offs, params)}
        # device state of nvit_ema_tick: updates applied, omd of the update about to run, two spare words
        self._state = torch.zeros(4, device=dev, dtype=torch.float32)
        # the tables are built now: their host images are pinned, which a stream capture does not allow
        self._key, self._table, self._chunks = None, None, 0
        self._build_table()
        init, chunks = ops.ema_table([(p.detach(), self._shadow[n], True) for n, p in zip(self._names, params)], dev)
        ops.ema_update(init, chunks)   # shadow = weights, through the kernel's copy rows
        self._module_flat = torch.zeros(total, device=dev, dtype=torch.float32) if self.renorm else None
        self._sync_table = ops.ema_table([(self._flat, self._module_flat, True)], dev) if self.renorm else None
        self._module = self._build_module(offs)
        self._dirty = True

    # ------------------------------------------------------------------ construction
    def _params(self):
        named = dict(self.model.named_parameters())
        return [named[n] for n in self._names]

    def _build_table(self) -> None:
        params = self._params()
        self._key = tuple(p.data_ptr() for p in params)
        self._table, self._chunks = ops.ema_table([(p.detach(), self._shadow[n]) for n, p in zip(self._names, params)],
                                                  self._flat.device)

    def _build_module(self, offs):
        from .model import ViT
        m = self.model
        with torch.random.fork_rng(devices=[]):   # the twin's random init must not move the caller's generator
            mod = ViT(m.config)
        mod.precision = m.precision
        mod.step, mod.total_steps = m.step, m.total_steps
        flat = self._module_flat if self.renorm else self._flat
        for n, o in zip(self._names, offs):
            owner, _, leaf = n.rpartition(".")
            s = self._shadow[n]
            owner = mod.get_submodule(owner)
            owner._parameters[leaf] = nn.Parameter(flat[o:o + s.numel()].view(s.shape), requires_grad=False)
        left = [n for n, p in mod.named_parameters() if p.device != self._flat.device]
        if left:
            raise RuntimeError(f"ModelEma: parameters without a shadow: {left}")
        for n, b in m.named_buffers():   # the integer index buffers (locations, offsets) are shared
            owner, _, leaf = n.rpartition(".")
            mod.get_submodule(owner)._buffers[leaf] = b
        mod.eval()
        mod.requires_grad_(False)
        return mod

    # ------------------------------------------------------------------ the update
    @torch.no_grad()
    def update(self, skip_state: Optional[Tensor] = None) -> None:
        """One update from the model's current weights: the tick and the table launch, no host synchronisation.
        skip_state: the optimizer's (FusedAdamW.skip_state) when its step was guarded; a step it left out leaves the
        average and the count as they are.  FusedAdamW.step_fused calls this for an attached EMA."""
        if not torch.cuda.is_current_stream_capturing():
            # parameter addresses are stable in this project; after something that moved one (model.to, a state dict
            # loaded by assignment) the table follows.  A captured step keeps the addresses it was recorded with.
            if tuple(p.data_ptr() for p in self._params()) != self._key:
                self._build_table()
        ops.ema_tick(self._state, self.decay, self.warmup, skip_state)
        ops.ema_update(self._table, self._chunks, self._state)
        self._dirty = True

    def mark_dirty(self) -> None:
        """Updates ran that this object did not launch itself (a replayed step): `module` must be refreshed."""
        self._dirty = True

    @torch.no_grad()
    def sync(self) -> None:
        """Bring `module` up to date with the shadow.  renorm=False: nothing to do, its parameters are the shadow.
        renorm=True: one copy launch shadow -> module, then normalize_matrices(module).  Public for holders of a
        GraphedEval(ema.module, ...): its graphs hold the module's addresses and rebuild the operand shadows inside the
        replay, so they see the refreshed weights."""
        if self.renorm:
            ops.ema_update(self._sync_table[0], self._sync_table[1])
            normalize_matrices(self._module)
        self._dirty = False

    @property
    def module(self):
        """The averaged weights as a ViT in eval() mode without gradients, for validate / estimate_loss / predict /
        GraphedEval; refreshed first when updates happened since the last sync()."""
        if self._dirty:
            self.sync()
        return self._module

    # ------------------------------------------------------------------ state
    @property
    def shadow(self) -> Dict[str, Tensor]:
        """name -> the live average of that parameter, a view into the one flat buffer (read it, do not assign to it;
        `state_dict()["shadow"]` holds copies)."""
        return dict(self._shadow)

    @property
    def state(self) -> Tensor:
        """fp32 device tensor [4]: (updates applied, 1 - d of the last update or 0 when that step was left out, spare,
        spare).  Written by nvit_ema_tick only; reading it on the host synchronises."""
        return self._state

    @property
    def updates(self) -> int:
        """Updates applied so far, skipped steps not counted (one host synchronisation)."""
        return int(self._state[0].item())

    def state_dict(self) -> dict:
        """{"shadow": {name: fp32 tensor}, "updates": int, "decay": float, "warmup": bool}: tensors and plain values."""
        return {"shadow": {n: t.detach().clone() for n, t in self._shadow.items()}, "updates": self.updates,
                "decay": self.decay, "warmup": self.warmup}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Restore a `state_dict()` (shadow, count, decay, warmup).  Load before a GraphedTrainStep is built: a captured
        tick keeps the decay and warm-up flag it was recorded with."""
        shadow = state["shadow"]
        if set(shadow) != set(self._shadow):
            missing, extra = sorted(set(self._shadow) - set(shadow)), sorted(set(shadow) - set(self._shadow))
            raise RuntimeError(f"ModelEma.load_state_dict: missing {missing}, unexpected {extra}")
        for n, t in self._shadow.items():
            if tuple(shadow[n].shape) != tuple(t.shape):
                raise RuntimeError(f"ModelEma.load_state_dict: {n} has shape {tuple(shadow[n].shape)}, "
                                   f"expected {tuple(t.shape)}")
        for n, t in self._shadow.items():
            t.copy_(shadow[n])
        self._state.copy_(torch.tensor([float(int(state["updates"])), 0.0, 0.0, 0.0]))
        self.decay, self.warmup = float(state["decay"]), bool(state["warmup"])
        self._dirty = True
