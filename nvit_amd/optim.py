"""AdamW whose step is fused with gradient clipping and the nGPT weight re-normalisation.

`FusedAdamW` IS a `torch.optim.AdamW` (same constructor, param groups, `state_dict()` layout: per-parameter
`step`, `exp_avg`, `exp_avg_sq`), so everything the reference trainer does with its optimizer keeps working
(/root/reference/nvit/train.py:456-459 build, :942-946 step / zero_grad, :640-650 checkpointing).  What changes
is how a step runs on the MI355X: `step_fused(model, grad_clip)` performs

    clip_grad_norm_(params, grad_clip)  ->  AdamW.step()  ->  Trainer.normalize_matrices()
    (train.py:935-941)                     (train.py:942-944)  (train.py:461-480, 989-990)

in two HIP launches (`nvit_grad_sqnorm`, `nvit_adamw_renorm`) over a device-side parameter table, reading each of
p, g, m, v once and writing p, m, v once; with `skip_nonfinite=True` a guarded tick between them decides, on the device,
whether the step is applied at all (GradScaler.step of the reference, train.py:930-942).  Plain `step()` (no clip, no renorm) uses the same kernel, so code that
calls `optimizer.step()` followed by `normalize_matrices(model)` gives identical weights.  There is no torch
fallback: the parameters must live on the HIP device.  With an `LRSchedule` attached (`attach_schedule`, schedule.py) one
more launch ahead of them (`nvit_lr_schedule`) writes the step's learning rate into the table, instead of the host.

One step counter serves all parameters (it lives on the device so that a captured step replays correctly).  torch
keeps one per parameter; the two agree as long as every parameter that is ever updated receives a gradient from the
first step on - true for this model, whose never-updated parameters (rmsnorm_*, the recon head without the Kohonen
loss) never get a gradient at all.  A parameter whose first gradient arrives late would be bias-corrected with the
global count; `_loaded_step` refuses checkpoints whose per-parameter counts disagree.
"""
from __future__ import annotations

import math
import struct
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import call
from .ops import _s

_TABLE_COLS = _lib.const("OPT_TABLE_COLS")  # the item geometry of nvit_grad_sqnorm / nvit_adamw_renorm (nvit_hip.h):
_CHUNK = _lib.const("OPT_CHUNK")
_ROWS_PER_ITEM = _lib.const("OPT_ROWS_PER_ITEM")
_SLAB_COLS = _lib.const("OPT_SLAB_COLS")    # column slab of a column-normalised matrix of at most _SLAB_ROWS rows,
_SLAB_ROWS = _lib.const("OPT_SLAB_ROWS")
_TALL_COLS = _lib.const("OPT_TALL_COLS")    # of a taller one (at most _TALL_ROWS rows): the slab must fit the LDS of a CU
_TALL_ROWS = _lib.const("OPT_TALL_ROWS")
_ROW_COLS = _lib.const("OPT_ROW_COLS")      # rows of a row-normalised matrix stay in registers up to this width,
_WIDE_COLS = _lib.const("OPT_WIDE_COLS")    # wider ones (up to this) are parked in LDS, which must then hold an item's rows:
_WIDE_LDS_ROWS = _lib.const("OPT_WIDE_LDS_ROWS")   # the LDS of a slab of this many rows does
_NPART = 1024                               # workgroups of the gradient-norm kernel (rows of its partials)
assert _NPART <= _lib.const("OPT_MAX_PART")


def _hyper_bits(group) -> int:
    """f32bits(lr) | f32bits(weight_decay) << 32 of a param group as the signed int64 of the table's last column."""
    return struct.unpack("<q", struct.pack("<ff", float(group["lr"]), float(group["weight_decay"])))[0]


def table_items(kind: int, rows: int, cols: int) -> Tuple[int, int, int]:
    """One table entry -> (items of nvit_adamw_renorm, gradient-norm chunks, slab rows of LDS it needs); kind -1: plain
    (rows * cols elements), 1: rows normalised, 0: columns normalised.  RuntimeError outside the kernel's range."""
    chunks = math.ceil(rows * cols / _CHUNK)
    if kind == 1:
        if cols % 4 or cols > _WIDE_COLS:
            raise RuntimeError(f"FusedAdamW: row-normalised matrix needs cols % 4 == 0 and <= {_WIDE_COLS} (got {cols})")
        return math.ceil(rows / _ROWS_PER_ITEM), chunks, _WIDE_LDS_ROWS if cols > _ROW_COLS else 0
    if kind == 0:
        if rows > _TALL_ROWS:
            raise RuntimeError(f"FusedAdamW: column-normalised matrix with {rows} rows exceeds the LDS slab ({_TALL_ROWS})")
        return math.ceil(cols / (_SLAB_COLS if rows <= _SLAB_ROWS else _TALL_COLS)), chunks, rows
    return chunks, chunks, 0


def renorm_matrices(model):
    """(weight, dim) of every matrix that Trainer.normalize_matrices re-normalises (reference train.py:461-480): dim 1 =
    unit rows, 0 = unit columns; nothing for a plain ViT.  The one list behind train.normalize_matrices (its table rows,
    hence the kernel's work order, follow this order) and the fused step."""
    m = model.module if hasattr(model, "module") else model
    if not m.config.use_nvit:
        return
    for blk in m.transformer.h:
        for lin, dim in ((blk.query, 1), (blk.key, 1), (blk.value, 1), (blk.att_c_proj, 0), (blk.c_fc, 1),
                         (blk.mlp_c_proj, 0)):
            yield lin.weight, dim


class FusedAdamW(torch.optim.AdamW):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        # the torch base class is only the container (param groups, state, state_dict); its kernels never run
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False)
        self._cache = None
        self._t = 0          # optimizer steps taken (host mirror of the device counter hyper[0])
        self._hyper = None   # device float[3]: step, 1/(1-b1^t), 1/sqrt(1-b2^t) - maintained by nvit_adamw_tick
        self._staging = None  # pinned host image of the device table
        self._hyper_pin = None   # pinned image of the lr/weight_decay column (eager lr schedules)
        self._hyper_ev = None
        self._skip_state = None   # device float[2], see skip_state
        self._guarded = False     # a skip_nonfinite step has run: only the device knows how many steps were applied
        self._ema = None          # attach_ema: a ModelEma that every step updates
        self._schedule = None     # attach_schedule: an LRSchedule whose launch writes every step's lr into the table
        self._scale_staging = None   # pinned host image of the rows' lr_scale (a captured step under a schedule)

    # ------------------------------------------------------------------ state
    def _ensure_state(self, p: torch.Tensor) -> Dict:
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _table(self, renorm_dims: Dict[int, int]):
        """Device table for the current (param, grad, state) pointers; rebuilt only when one of them moves."""
        rows: List[List[int]] = []
        key = []
        hypers: List[int] = []   # per row: lr | weight_decay bits (the last column of the table)
        groups: List[int] = []   # per row: index of its param group
        scales: List[float] = []  # per row: its group's lr_scale (layer-wise lr decay; read by an attached schedule)
        first_item = first_chunk = 0
        max_slab_rows = 0
        beta_eps = None
        for gi, group in enumerate(self.param_groups):
            be = (group["betas"][0], group["betas"][1], group["eps"])
            if group.get("amsgrad") or group.get("maximize"):
                raise RuntimeError("FusedAdamW: amsgrad / maximize are not supported")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if beta_eps is None:
                    beta_eps = be
                elif be != beta_eps:
                    raise RuntimeError("FusedAdamW: all parameter groups must share betas and eps")
                if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamW: parameters must be contiguous fp32 tensors on the HIP device")
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                    raise RuntimeError("FusedAdamW: gradients must be dense contiguous fp32")
                st = self._ensure_state(p)
                kind = renorm_dims.get(id(p), -1)
                if kind >= 0 and p.dim() == 2:
                    r, c = p.shape
                else:
                    kind, r, c = -1, 1, p.numel()
                items, chunks, slab = table_items(kind, r, c)
                max_slab_rows = max(max_slab_rows, slab)
                hyper = _hyper_bits(group)
                rows.append([p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             r, c, kind, first_item, first_chunk, hyper])
                key.append((p.data_ptr(), g.data_ptr(), kind))
                hypers.append(hyper)
                groups.append(gi)
                scales.append(float(group.get("lr_scale", 1.0)))
                first_item += items
                first_chunk += chunks
        key = tuple(key)
        if self._cache is not None and self._cache["key"] == key and self._cache["hypers"] != hypers:
            # only lr / weight_decay moved (the reference trainer rewrites lr every iteration): update the hyper column in
            # place instead of rebuilding table, workspaces and a pinned image.  Under an attached schedule the lr half
            # belongs to the device (group["lr"] is the peak rate, kept for the record): only a weight_decay counts.
            if self._schedule is None or [h >> 32 for h in self._cache["hypers"]] != [h >> 32 for h in hypers]:
                self._write_hyper_column(hypers)
        if self._cache is None or self._cache["key"] != key:
            if not rows:
                return None
            dev = next(p.device for group in self.param_groups for p in group["params"])
            n = len(rows)
            host = torch.tensor(rows, dtype=torch.int64)
            table = torch.empty((n, _TABLE_COLS), dtype=torch.int64, device=dev)
            if torch.cuda.is_current_stream_capturing():
                # Inside a hipGraph capture (the gradients autograd allocates there have new addresses, so the table is
                # rebuilt once): pinned memory cannot be allocated now, so the image goes through the persistent
                # staging buffer that GraphedTrainStep reserved; the captured memcpy re-sends that buffer on every
                # replay, which is also how a later learning-rate change reaches the captured step.
                if self._staging is None or self._staging.shape[0] < n:
                    raise RuntimeError("FusedAdamW: call reserve_staging() before capturing a step")
                self._staging[:n].copy_(host)
                table.copy_(self._staging[:n], non_blocking=True)
                staged = True
                if self._schedule is not None:   # the rows' lr_scale follows the table's rule
                    if self._scale_staging is None or self._scale_staging.shape[0] < n:
                        raise RuntimeError("FusedAdamW: call reserve_staging() before capturing a step")
                    self._scale_staging[:n].copy_(torch.tensor(scales, dtype=torch.float32))
                    lr_scale = torch.empty(n, dtype=torch.float32, device=dev)
                    lr_scale.copy_(self._scale_staging[:n], non_blocking=True)
            else:
                # eager: a fresh pinned image per rebuild (the host allocator keeps it alive until the async copy has
                # run; re-using one buffer would race with copies still queued behind a GPU that runs steps behind)
                table.copy_(host.pin_memory(), non_blocking=True)
                staged = False
                if self._schedule is not None:
                    lr_scale = torch.tensor(scales, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
            self._cache = {
                "key": key,
                "hypers": hypers,
                "groups": groups,
                "table": table,
                "lr_scale": lr_scale if self._schedule is not None else None,   # fp32 [n], built with the table
                "n": len(rows), "items": first_item, "chunks": first_chunk, "slab": max_slab_rows,
                "partial": torch.empty(_NPART, device=dev, dtype=torch.float32),
                "gnorm": torch.empty(1, device=dev, dtype=torch.float32),
                "betas_eps": beta_eps,
                "staged": staged,
                "n_elems": sum(r[4] * r[5] for r in rows),
            }
        return self._cache

    # ------------------------------------------------------------------ steps
    @torch.no_grad()
    def step_fused(self, model=None, grad_clip: float = 0.0, skip_nonfinite: bool = False) -> Optional[torch.Tensor]:
        """clip (if grad_clip > 0) + AdamW + (if `model` is given) normalize_matrices; returns the pre-clip grad norm
        as a 1-element device tensor when clipping or skip_nonfinite is on.

        skip_nonfinite=True is what GradScaler.step does for the reference (train.py:930-942): a step whose gradients
        hold inf or NaN is left out.  Three launches: nvit_grad_sqnorm (always, also with grad_clip == 0), the guarded
        tick, which sums the norm partials, decides once and writes `skip_state`, and the guarded update, in which every
        workgroup reads that one flag.  A skipped step leaves every parameter, exp_avg, exp_avg_sq and the step counter
        bit-identical and returns the inf / NaN norm; an applied step gives the bits of the unguarded step.  Two things to
        know: gradients whose squared norm overflows fp32 (norm above ~1.8e19) count as non-finite although every
        element is finite; and the reference re-runs normalize_matrices on the unchanged weights after a skipped step
        (a change of at most an ulp), while here nothing moves.  Under DataParallel every rank holds the same averaged
        gradients when this runs, hence takes the same decision."""
        dims: Dict[int, int] = {} if model is None else {id(w): dim for w, dim in renorm_matrices(model)}
        c = self._table(dims)
        if c is None:
            return None
        b1, b2, eps = c["betas_eps"]
        dev = c["table"].device
        if self._hyper is None:
            self._t = self._loaded_step()
            self._hyper = torch.tensor([float(self._t), 0.0, 0.0], dtype=torch.float32).pin_memory().to(
                dev, non_blocking=True)
        if self._schedule is not None:
            # this step's lr into the table, ahead of everything that reads it; also when skip_nonfinite then leaves the
            # step out (the reference's iter_num advances on a skipped step too)
            self._schedule.apply(c["table"], c["n"], c["lr_scale"])
        # the step counter lives on the device (bias corrections are computed there), so a captured step replays
        # correctly; the host mirror only feeds state_dict()
        clip = grad_clip is not None and grad_clip > 0.0
        if skip_nonfinite:
            skip = self.skip_state
            self._guarded = True
            self._t += 1   # as if applied; state_dict() reads the count of applied steps back from the device
            call("nvit_grad_sqnorm", c["table"], c["n"], c["chunks"], c["partial"], _NPART, _s())
            call("nvit_adamw_tick_guarded", self._hyper, b1, b2, c["partial"], _NPART, skip, _s())
            call("nvit_adamw_renorm_guarded", c["table"], c["n"], c["items"], c["slab"], b1, b2, eps, c["partial"], _NPART,
                 float(grad_clip) if clip else 0.0, c["gnorm"], self._hyper, skip, _s())
            if self._ema is not None:
                self._ema.update(skip)   # the tick reads the decision just taken: a step left out is no update
            return c["gnorm"]
        call("nvit_adamw_tick", self._hyper, b1, b2, _s())
        self._t += 1
        if clip:
            call("nvit_grad_sqnorm", c["table"], c["n"], c["chunks"], c["partial"], _NPART, _s())
        call("nvit_adamw_renorm", c["table"], c["n"], c["items"], c["slab"], b1, b2, eps, 0.0, 0.0,
             c["partial"] if clip else None, _NPART if clip else 0, float(grad_clip) if clip else 0.0,
             c["gnorm"] if clip else None, self._hyper, _s())
        if self._ema is not None:
            self._ema.update()
        return c["gnorm"] if clip else None

    # ------------------------------------------------------------------ weight EMA
    def attach_ema(self, ema) -> None:
        """ema: a `ModelEma` of the model this optimizer steps, or None to detach.  Every step (step_fused, step()) then
        ends with `ema.update()`, two more launches: one optimizer step is one update whatever accumulation_steps is, and a
        step that skip_nonfinite leaves out leaves the average alone.  Attach before a GraphedTrainStep is built, so that
        the captured step holds the update."""
        if ema is not None and not (callable(getattr(ema, "update", None)) and callable(getattr(ema, "mark_dirty", None))):
            raise TypeError("attach_ema: a ModelEma (or None) expected")
        self._ema = ema

    @property
    def ema(self):
        """The attached ModelEma, or None."""
        return self._ema

    # ------------------------------------------------------------------ learning-rate schedule
    def attach_schedule(self, schedule) -> None:
        """schedule: an `LRSchedule` on the parameters' device, or None to detach.  Every step (step_fused, step()) then
        starts with one more launch (nvit_lr_schedule) that writes lr = L(s) * lr_scale into every row of the device table
        and advances the schedule's counter: one optimizer step is one schedule step whatever accumulation_steps is, and a
        step that skip_nonfinite leaves out is one too.  lr_scale is the row's `group.get("lr_scale", 1.0)`
        (`layer_decay_groups`).  While a schedule is attached the host pushes no lr: `group["lr"]` keeps the value it was
        given (the peak rate) and changing it does nothing; `current_lr()` reads the rate in use.  Attach before a
        GraphedTrainStep is built, so that the captured step holds the launch.  Attaching or detaching rebuilds the table
        on the next step, from the groups' lr."""
        if schedule is not None and not (callable(getattr(schedule, "apply", None)) and hasattr(schedule, "lr_at")):
            raise TypeError("attach_schedule: an LRSchedule (or None) expected")
        if schedule is not self._schedule:
            self._cache = None
        self._schedule = schedule

    @property
    def schedule(self):
        """The attached LRSchedule, or None."""
        return self._schedule

    def current_lr(self) -> float:
        """The L(s) of the last step under the attached schedule, before any lr_scale (one host synchronisation); 0.0
        before the first step.  `schedule.last_lr` is the same value as a device tensor."""
        if self._schedule is None:
            raise RuntimeError("FusedAdamW.current_lr: no schedule attached (the groups' lr is the rate in use)")
        return float(self._schedule.last_lr.item())

    # ------------------------------------------------------------------ skipped steps
    @property
    def skip_state(self) -> torch.Tensor:
        """fp32 device tensor [2]: (the last skip_nonfinite step was skipped: 0 / 1, steps skipped so far).  Written by
        the guarded tick only; reading it on the host synchronises."""
        if self._skip_state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: take one skip_nonfinite step (or read skip_state) before capturing one")
            dev = next(p.device for group in self.param_groups for p in group["params"])
            if dev.type != "cuda":
                raise RuntimeError("FusedAdamW: parameters must live on the HIP device")
            self._skip_state = torch.zeros(2, device=dev, dtype=torch.float32)
        return self._skip_state

    def skipped_steps(self) -> int:
        """Steps that skip_nonfinite left out so far (one host synchronisation)."""
        return 0 if self._skip_state is None else int(self._skip_state[1].item())

    # ------------------------------------------------------------------ step counter <-> torch's per-parameter state
    def _loaded_step(self) -> int:
        """Step count found in the (possibly loaded) per-parameter state; all parameters must agree."""
        t = None
        for st in self.state.values():
            if "step" in st:
                v = int(float(st["step"]))
                if t is not None and v != t:
                    raise RuntimeError("FusedAdamW: parameters with different step counts are not supported")
                t = v
        return t or 0

    def _write_hyper_column(self, hypers: List[int], c=None) -> None:
        c = self._cache if c is None else c
        hcol = torch.tensor(hypers, dtype=torch.int64)
        if c["staged"]:
            torch.cuda.current_stream().synchronize()   # no replay may be reading the staging buffer while it changes
            self._staging[:c["n"], _TABLE_COLS - 1].copy_(hcol)
            c["table"].copy_(self._staging[:c["n"]], non_blocking=True)
        else:
            # one persistent pinned column, guarded by an event: the previous async copy must have left it
            if self._hyper_pin is None or self._hyper_pin.numel() < c["n"]:
                self._hyper_pin = torch.empty(max(c["n"], 64), dtype=torch.int64).pin_memory()
                self._hyper_ev = torch.cuda.Event()
            else:
                self._hyper_ev.synchronize()
            self._hyper_pin[:c["n"]].copy_(hcol)
            c["table"][:, _TABLE_COLS - 1].copy_(self._hyper_pin[:c["n"]], non_blocking=True)
            self._hyper_ev.record()
        c["hypers"] = list(hypers)

    def rewrite_hyper(self, cache=None) -> None:
        """Push the param groups' current lr / weight_decay into the device table in place (same addresses, so a
        captured step picks them up on its next replay).  cache: the table a captured step was recorded with
        (GraphedTrainStep keeps it: an eager step taken after the capture builds a table of its own)."""
        c = self._cache if cache is None else cache
        if c is None:
            return
        self._write_hyper_column([_hyper_bits(self.param_groups[gi]) for gi in c["groups"]], c)

    def reserve_staging(self) -> None:
        """Pinned host image for the parameter table, allocated ahead of a hipGraph capture."""
        n = sum(len(g["params"]) for g in self.param_groups)
        if self._staging is None or self._staging.shape[0] < n:
            self._staging = torch.empty((max(n, 64), _TABLE_COLS), dtype=torch.int64).pin_memory()
        if self._schedule is not None and (self._scale_staging is None or self._scale_staging.shape[0] < n):
            self._scale_staging = torch.empty(max(n, 64), dtype=torch.float32).pin_memory()

    def note_replay(self, n: int = 1) -> None:
        """A captured step was replayed n times (the device counter advanced; keep the host mirror in sync)."""
        self._t += n
        if self._ema is not None:
            self._ema.mark_dirty()   # the replay updated the average on the device

    def _sync_state_steps(self) -> None:
        if self._guarded and self._hyper is not None:
            # skipped steps are known to the device alone: hyper[0] counts the applied ones (the one synchronisation)
            self._t = int(self._hyper[0].item())
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(float(self._t), dtype=torch.float32)

    def state_dict(self):
        self._sync_state_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._cache = None
        self._hyper = None   # re-created from the loaded step count on the next step

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.step_fused(None, 0.0)
        return loss
