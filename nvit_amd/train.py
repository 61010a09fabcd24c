"""Post-step weight re-normalisation and the reference's train-step order.

`normalize_matrices(model)` replaces Trainer.normalize_matrices
(/root/reference/nvit/train.py:461-480): same six matrices per block, same axes, fp32 in
place — but ONE persistent HIP launch instead of ~30 torch kernels per block.

`train_step` reproduces the call sequence of the reference hot loop
(train.py:898-946,989-990): forward -> cross_entropy -> backward -> clip_grad_norm_(1.0) ->
AdamW.step -> zero_grad(set_to_none) -> normalize_matrices, with the loop's gradient accumulation
(`accumulation_steps`) and its GradScaler's skipped step (`skip_nonfinite`) as options.  With the FusedAdamW that
`configure_optimizers` returns, clip + AdamW + renorm run as two HIP launches (optim.py);
with a plain torch optimizer the three steps run separately, same result.
"""
from __future__ import annotations

from contextlib import nullcontext

import torch

from . import ops
from ._lib import call
from .crop import CenterCroppedBatch
from .mix import MixedTargets
from .ops import _s
from .optim import FusedAdamW, renorm_matrices
from .stages import StagedBatch, chain


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def normalize_matrices(model) -> None:
    m = _unwrap(model)
    mats = [(w.data, dim) for w, dim in renorm_matrices(m)]
    if not mats:
        return
    dev = mats[0][0].device
    if dev.type != "cuda":
        raise RuntimeError("normalize_matrices: parameters must live on the HIP device (no CPU fallback)")
    key = tuple(w.data_ptr() for w, _ in mats)
    cache = getattr(m, "_renorm_cache", None)
    if cache is None or cache[0] != key:
        table, items = ops.renorm_table(mats, dev)
        cache = (key, table, items)
        object.__setattr__(m, "_renorm_cache", cache)
    ops.renorm_weights(cache[1], cache[2])


class CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy(logits, y) (reference train.py:906) as one HIP pass that also produces the gradient.  y: int64
    labels (nvit_ce_loss), or the `MixedTargets` of a Mixup (mix.py): two labels and a lambda per row plus label
    smoothing, timm's mixup_target (nvit_ce_loss_soft)."""

    @staticmethod
    def forward(ctx, logits, y):
        soft = y if isinstance(y, MixedTargets) else None
        if soft is not None:
            y = soft.y
        if logits.device.type != "cuda" or logits.dtype != torch.float32 or y.dtype != torch.int64:
            raise RuntimeError("CrossEntropyFn: fp32 logits and int64 labels on the HIP device (no CPU path)")
        logits = logits.contiguous()
        B, N = logits.shape
        rowloss = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty(1, device=logits.device, dtype=torch.float32)
        dlogits = torch.empty_like(logits)
        if soft is not None:
            if soft.y.shape[0] != B:
                raise ValueError(f"CrossEntropyFn: {soft.y.shape[0]} targets for {B} rows of logits")
            ops._chk_dev(soft.y2, soft.lam)
            call("nvit_ce_loss_soft", logits, y.contiguous(), soft.y2.contiguous(), soft.lam.contiguous(), soft.smoothing,
                 rowloss, loss, dlogits, B, N, _s())
        else:
            call("nvit_ce_loss", logits, y.contiguous(), rowloss, loss, dlogits, B, N, _s())
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


def total_loss(config, logits: torch.Tensor, aux, y: torch.Tensor, consistency_weight: float = 0.1,
               smoothness_weight: float = 0.1) -> torch.Tensor:
    """Loss of the reference loop (train.py:906-926): CE, plus the weighted aux losses iff the Kohonen head is on
    (consistency/smoothness weights are settings.yaml `training.*`, the others come from the model config).  y: int64
    labels or a `MixedTargets` (the soft-target cross-entropy)."""
    return add_aux_losses(config, CrossEntropyFn.apply(logits, y), aux, consistency_weight, smoothness_weight)


def add_aux_losses(config, loss: torch.Tensor, aux, consistency_weight: float = 0.1,
                   smoothness_weight: float = 0.1) -> torch.Tensor:
    """`loss` (the cross-entropy) plus the weighted aux losses iff the Kohonen head is on: the weighting of the training
    loss (train.py:906-926) and of the reference's estimate_loss (train.py:495-502), kept in one place."""
    if config.use_kohonen:
        loss = (loss + consistency_weight * aux["kohonen_consistency"] + smoothness_weight * aux["kohonen_smoothness"]
                + config.local_quantization_weight * aux["local_quantization"]
                + config.global_quantization_weight * aux["global_quantization"]
                + config.reconstruction_weight * aux["reconstruction"])
    return loss


def _loader_batch(X):
    """The `DeviceLoader.batch()` (data.py) that the chain X stands on, or None."""
    batches = chain(X)
    return batches[-1] if batches and batches[-1].key == "data" else None


def _check_step_args(optimizer, X, accumulation_steps, skip_nonfinite, y=None) -> None:
    """The argument checks of train_step / GraphedTrainStep: ValueError (TypeError for evaluation's batch object), before
    any device work."""
    if isinstance(X, CenterCroppedBatch):
        raise TypeError("a ResizeCenterCrop.batch(u8) (CenterCroppedBatch) is evaluation's input; a train step takes a tensor "
                        "or the chain of RandomResizedCrop.batch(u8)")
    if y is not None and _loader_batch(X) is not None:
        raise ValueError("the labels of a DeviceLoader.batch() come from the dataset: pass y=None")
    n = accumulation_steps
    if not isinstance(n, int) or isinstance(n, bool) or n < 1:
        raise ValueError(f"accumulation_steps must be an int >= 1 (got {n!r})")
    if X.shape[0] % n:
        raise ValueError(f"accumulation_steps={n} does not divide the batch of {X.shape[0]} rows")
    if skip_nonfinite and not isinstance(optimizer, FusedAdamW):
        raise ValueError("skip_nonfinite=True needs the FusedAdamW returned by ViT.configure_optimizers")


def _unwrap_input(X):
    """X of a step -> ({"mix": Mixup, "erase": (RandomErasing, mean, std), "augment": AutoAugment, "crop":
    RandomResizedCrop, "data": DeviceLoader}, the stages it carries, outermost first; the tensor underneath - under a
    loader its dataset's own): the chain as a dict."""
    if isinstance(X, StagedBatch):
        X.check_step()
    batches = chain(X)
    return {b.key: b.fit_key() if b.extra else b.stage for b in batches}, (batches[-1].inner if batches else X)


def _wrap_input(stages: dict, X):
    """The chain of `_unwrap_input` around another tensor."""
    for fit in reversed(stages.values()):
        X = fit[0].batch(X, *fit[1:]) if isinstance(fit, tuple) else fit.batch(X)
    return X


def _resolve_input(X, y):
    """(X, y) of a step -> the model's input and the loss's target: every launch of the chain that X carries (crop,
    augmentation, erasing, Mixup - each once, for the whole batch), in order.  A tensor X comes back as it is."""
    return X.resolve(y) if isinstance(X, StagedBatch) else (X, y)


def _forward_backward(model, X, y, n: int, before_micro=None):
    """The n forward/backward passes of one optimizer step (reference train.py:898-928); returns (logits, loss, aux),
    all attached for n == 1 (exactly the single pass, no division is launched) and detached sums for n > 1.
    before_micro(i), if given, runs ahead of micro-step i (GraphedTrainStep hands the SOM maps their rate there)."""
    cfg = _unwrap(model).config
    if n == 1:
        if before_micro is not None:
            before_micro(0)
        logits, aux = model(X)
        loss = total_loss(cfg, logits, aux, y)
        loss.backward()
        return logits, loss, aux
    b = X.shape[0] // n
    no_sync = getattr(model, "no_sync", None)
    parts, loss, aux = [], None, None
    for i in range(n):
        if before_micro is not None:
            before_micro(i)
        # data parallel: only the last micro-step communicates (train.py:899-902)
        with (no_sync() if no_sync is not None and i < n - 1 else nullcontext()):
            logits_i, aux_i = model(X[i * b:(i + 1) * b])
            loss_i = total_loss(cfg, logits_i, aux_i, y[i * b:(i + 1) * b]) / n
            loss_i.backward()
        parts.append(logits_i.detach())
        scaled = {k: v.detach() / n for k, v in aux_i.items()}
        loss = loss_i.detach() if loss is None else loss + loss_i.detach()
        aux = scaled if aux is None else {k: aux[k] + scaled[k] for k in aux}
    return torch.cat(parts), loss, aux


def train_step(model, optimizer, X: torch.Tensor, y: torch.Tensor, grad_clip: float = 1.0,
               sync_grads=None, *, accumulation_steps: int = 1, skip_nonfinite: bool = False):
    """One optimizer step in the reference's order; returns (logits, loss, aux, grad_norm).

    accumulation_steps = N > 1 (`training.gradient_accumulation_steps`, train.py:898-928): the batch (a multiple of N
    rows) is cut into N micro-batches, micro-batch i being rows [i*b, (i+1)*b); each runs a training forward, then
    total_loss / N, then backward, and the gradients add up in autograd; one optimizer step follows.  `model.step`
    advances by N, and the Kohonen head updates its SOM nodes N times, each at the rate of its own `model.step`.  A
    model with a `no_sync()` (DataParallel) runs micro-steps 0..N-2 inside it; `sync_grads` is called once, after the
    last backward.  Returned: the N logits concatenated [N*b, classes], loss = the sum of the N scaled losses in
    micro-step order, aux[k] = the sum of aux_i[k] / N, grad_norm as for N = 1.  The reference feeds the SAME (X, y)
    to all N micro-steps (train.py:885-905 fetches once per iteration); X.repeat(N, 1, 1, 1), y.repeat(N) reproduces
    that.

    skip_nonfinite=True (the reference runs GradScaler for bf16 too, train.py:135-136, 930-942): a step whose
    gradients hold inf or NaN - in any micro-batch - is left out on the device, weights, moments and step count
    untouched; see FusedAdamW.step_fused.  grad_norm is then returned also with grad_clip == 0, and is inf / NaN for a
    skipped step; `optimizer.skipped_steps()` counts them.  Under DataParallel every rank sees the same averaged
    gradients, hence the same decision.  Needs FusedAdamW.

    X may be a chain of the input stages, `mix.batch(erase.batch(aug.batch(rrc.batch(u8))))` or any part of it in that
    order, with a `DeviceLoader.batch()` (data.py) where the uint8 tensor stands - y is then None, batch and labels are
    drawn and gathered on the device by the chain's first two launches (stages.py; DESIGN.md §7, "The batch-object
    protocol"): every stage's launches run once for the whole batch, ahead of the forward and of any accumulation split,
    and every stage's counter advances by one per call.  With a Mixup the loss
    is the soft-target cross-entropy of the drawn `MixedTargets`, the returned logits belong to the mixed batch, and under
    accumulation micro-batch i takes rows [i*b, (i+1)*b) of the mixed batch and of the targets (a row's partner may lie in
    another micro-batch; the targets carry the partner's label).  A tensor X takes exactly the launches it always took.

    A `DropPath` attached to the model (`ViT.attach_drop_path`) needs nothing here: every training forward draws its own
    gate table, so with accumulation_steps = N its counter advances by N, each micro-batch drawing for its own rows.  The
    same holds for a `PatchDropout` (`ViT.attach_patch_drop`): one draw of kept tokens per training forward.

    An `LRSchedule` attached to the optimizer (`FusedAdamW.attach_schedule`, schedule.py) needs nothing here either: the
    fused step starts with its launch, which writes this step's lr into the optimizer's device table and advances the
    schedule's device counter - once per call whatever accumulation_steps is, also when skip_nonfinite leaves the update out.

    Wrong accumulation_steps (no int, < 1, no divisor of the batch) or skip_nonfinite with another optimizer raise
    ValueError before any device work."""
    _check_step_args(optimizer, X, accumulation_steps, skip_nonfinite, y)
    X, y = _resolve_input(X, y)   # the chain's launches for the whole batch, ahead of any accumulation split
    logits, loss, aux = _forward_backward(model, X, y, accumulation_steps)
    if sync_grads is not None:
        sync_grads()
    if isinstance(optimizer, FusedAdamW):
        # clip + AdamW + normalize_matrices in two launches (nvit_grad_sqnorm, nvit_adamw_renorm); three when guarded
        gnorm = optimizer.step_fused(model, grad_clip, skip_nonfinite=skip_nonfinite)
        if gnorm is not None:
            gnorm = gnorm[0].clone()
        optimizer.zero_grad(set_to_none=True)
    else:
        params = [p for p in _unwrap(model).parameters() if p.grad is not None]
        gnorm = torch.nn.utils.clip_grad_norm_(params, grad_clip) if grad_clip != 0.0 else None
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        normalize_matrices(model)
    # detached: a live reference to the step's autograd graph would also pin its AccumulateGrad nodes (and the stream
    # they were created on), which breaks a later hipGraph capture of the step
    return logits.detach(), loss.detach(), {k: v.detach() for k, v in aux.items()}, gnorm


class GraphedTrainStep:
    """The whole train step (forward, loss, backward, clip + AdamW + renorm) captured once as a hipGraph and replayed.

    SURVEY.md §8f F2: for C1-sized models the eager step is bound by ~600 kernel launches, not by the GPU.  Needs the
    FusedAdamW optimizer (its step counter and bias corrections live on the device, so replays stay correct), a fixed
    batch shape and a single process (the data-parallel wrapper launches RCCL work from autograd hooks and stays
    eager).  The learning rate is the one in the optimizer's param groups at capture time; `set_lr` rewrites it on the
    device between replays.

    The Kohonen head's SOM schedule stays host state (`model.step`, `get_kohonen_lr`): the captured SOM updates read
    their rate (learning rate x the map's alpha, what the eager call passes by value) from one device float per map
    (nvit_som_update_dev), which `__call__` rewrites from a pinned host twin ahead of every replay.  Only the capture
    pass takes that route; the warm-up steps and any eager `train_step` on the same model pass the rate by value.
    After N calls `model.step`, the optimizer's step count, the weights and the SOM nodes are those of N eager steps.
    The model's `training` flag at capture time is part of the graph.  Like the eager step, a call leaves every
    `p.grad` None (the graph keeps its own gradient buffers), so eager and graphed steps can alternate on one model.

    accumulation_steps = N and skip_nonfinite mean what they mean for `train_step`.  The N forward/backward passes and
    the one optimizer step are ONE graph over a static X of N*b rows; the SOM rates are then N x maps device floats
    (micro-step i of the capture hands each map its own element), filled from get_kohonen_lr(step+1 .. step+N) ahead
    of a replay, and a call advances `model.step` by N.  With skip_nonfinite the replay itself leaves a non-finite step
    out (no host code runs between backward and update, so only the device can): `optimizer.skipped_steps()` and
    `state_dict()` read the counts back.

    With X a chain of the input stages (stages.py; DESIGN.md §7, "The batch-object protocol", also for what a call may
    then carry) the static inputs are the chain's innermost tensor and y, and every stage's launches are captured in order
    ahead of the forward.  A stage's step counter is a device int64 that its draw kernel advances itself, so every replay
    draws afresh with no host code in between: the warm-up steps are steps of every stage (they advance its counter, as
    they advance the weights), the capture pass is not, every replay is.

    With a `DeviceLoader.batch()` (data.py) as the chain's innermost stage the static input is the dataset's own tensor
    (`self.X` is it, not a copy) and there is no static y: a call copies nothing to the device, and K steps are K replays.
    The call takes the chain around the captured loader's batch and y=None; another loader or another dataset tensor is
    refused.  The loader's counter counts like every stage's: warm-up steps yes, the capture pass no.  `ld.record` holds
    the (epoch, step in the epoch) of the last replay, readable whenever the host chooses to wait.

    `self.targets` (every captured step has it, beside `self.logits` and `self.loss`) is the static target that the
    captured loss reads, as of the last replay: the static y itself for a tensor X or a chain without a Mixup, the
    `MixedTargets` a Mixup drew, a loader's gathered labels (or the `MixedTargets` drawn from them).

    A `ModelEma` (ema.py) attached to the optimizer before this object is built is part of the captured step: its tick and
    its update follow the optimizer's launches, and its count lives on the device.  The warm-up steps are updates, as they
    are optimizer steps; the capture pass is not (it executes nothing).  A call with another EMA attached than at capture
    time (or none, or one where there was none) raises ValueError.

    A `DropPath` attached to the model (`ViT.attach_drop_path`) draws inside the forward, so its draw is captured with it:
    the counter is a device int64 the draw kernel advances, every replay drops other branches, and with
    accumulation_steps = N a replay is N draws.  Warm-up steps advance the counter, the capture pass does not.  A call
    with another DropPath attached than at capture time (or none, or one where there was none) raises ValueError.

    A `PatchDropout` (`ViT.attach_patch_drop`) likewise: its draw and the token gather are captured with the forward, every
    replay keeps other tokens, accumulation_steps = N is N draws, and a call with another PatchDropout attached than at
    capture time raises ValueError.  Its draw allocates, like every first call at a new shape: the warm-up steps cover it.

    An `LRSchedule` (schedule.py) attached to the optimizer before this object is built is part of the captured step: its
    launch follows the captured table copy and precedes the optimizer's, its counter is a device int64 the launch
    advances, and every replay steps at the next lr with no host code in between.  The warm-up steps are schedule steps, as
    they are optimizer steps; the capture pass is not (it executes nothing).  One replay is one schedule step whatever
    accumulation_steps is, also when skip_nonfinite leaves the update out.  A call with another schedule attached than at
    capture time (or none, or one where there was none) raises ValueError, and so does `set_lr` while one is attached: the
    next replay would overwrite what it wrote.

    With `ViT.set_dynamic_img_size(True)` X may have another image size than the model's: the resampling of the two
    position tables and its backward are captured with the step (their tap tables are sent to the device by the warm-up
    steps; a capture cannot).  The graph is bound to that size, as to the batch size.  After `ViT.set_input_size` changed
    the model, a call raises ValueError: the graph and the optimizer hold the parameters it replaced.
    """

    def __init__(self, model, optimizer, X: torch.Tensor, y: torch.Tensor, grad_clip: float = 1.0, warmup: int = 3,
                 *, accumulation_steps: int = 1, skip_nonfinite: bool = False):
        _check_step_args(optimizer, X, accumulation_steps, skip_nonfinite, y)
        m = _unwrap(model)
        if not isinstance(optimizer, FusedAdamW):
            raise RuntimeError("GraphedTrainStep needs the FusedAdamW returned by ViT.configure_optimizers")
        if hasattr(model, "module"):
            raise RuntimeError("GraphedTrainStep: wrap the bare model (data-parallel steps run eagerly)")
        if X.device.type != "cuda":
            raise RuntimeError("GraphedTrainStep: inputs must live on the HIP device")
        # the captured chain: per stage key what a call's stage must match, and the chain itself around the static input
        self._fit = {b.key: b.fit_key() for b in chain(X)}
        self.mix, self.erase, self.augment, self.crop = (self._fit.get(k, (None,))[0]
                                                         for k in ("mix", "erase", "augment", "crop"))
        if self.mix is not None:
            X.check_labels(y)
        if self._fit:
            X.check_step()
        if "data" in self._fit:   # the dataset's own tensor, not a copy of it, and no y: nothing is sent per call
            self.X, self.y = X.source(), None
        else:
            self.X, self.y = (X.source() if self._fit else X).clone(), y.clone()
        self._input = X.rebind(self.X) if self._fit else self.X
        self.model, self.optimizer, self.grad_clip = model, optimizer, grad_clip
        self.ema = optimizer.ema   # the ModelEma (or none) whose update the warm-up steps run and the capture records
        self.schedule = optimizer.schedule   # the LRSchedule (or none) whose launch the captured optimizer step contains
        self.drop_path = m.drop_path   # the DropPath (or none) whose draw the captured forwards contain
        self.patch_drop = m.patch_drop   # the PatchDropout (or none), likewise
        self._size_epoch = m._size_epoch   # ViT.set_input_size replaces parameters whose addresses the graph holds
        # what a call must find as it was at capture time: (the refusal's words, where a call finds it, what it was)
        self._attached = (
            ("this graph was captured with another ModelEma (or none)", lambda: optimizer.ema, self.ema),
            ("this graph was captured with another LRSchedule (or none)", lambda: optimizer.schedule, self.schedule),
            ("this graph was captured with another DropPath (or none)", lambda: m.drop_path, self.drop_path),
            ("this graph was captured with another PatchDropout (or none)", lambda: m.patch_drop, self.patch_drop),
            ("ViT.set_input_size replaced the position embeddings this graph was captured with; build a new optimizer and "
             "a new GraphedTrainStep", lambda: m._size_epoch, self._size_epoch))
        self.accumulation_steps, self.skip_nonfinite = accumulation_steps, bool(skip_nonfinite)
        N = accumulation_steps
        side = torch.cuda.Stream()   # warm-up and capture share one stream: autograd's gradient accumulators are
        side.wait_stream(torch.cuda.current_stream())   # bound to the stream they are first used on
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):   # builds every cache (shadow/renorm tables, LDS attributes, workspaces)
                train_step(model, optimizer, self._input, self.y, grad_clip, accumulation_steps=N,
                           skip_nonfinite=self.skip_nonfinite)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        optimizer.zero_grad(set_to_none=True)
        optimizer.reserve_staging()
        # SOM rates: one device float per micro-step and map and their pinned host twin, guarded by an event (the copy
        # queued by the previous call must have read the twin before it is overwritten)
        self._maps = [m.local_kohonen, m.global_kohonen] if m.config.use_kohonen else []
        self._steps = bool(m.training)   # the captured forwards are training ones: a replay is N model.steps
        if self._maps:
            self._rate_dev = torch.zeros(N, len(self._maps), device=X.device, dtype=torch.float32)
            self._rate_pin = torch.zeros(N, len(self._maps), dtype=torch.float32).pin_memory()
            self._rate_ev = torch.cuda.Event()
        step0 = m.step
        self.graph = torch.cuda.CUDAGraph()

        def hand_rates(i):
            for j, km in enumerate(self._maps):
                object.__setattr__(km, "_rate_dev", self._rate_dev[i, j:j + 1])

        try:
            with torch.cuda.graph(self.graph, stream=side):
                Xin, yin = _resolve_input(self._input, self.y)
                logits, loss, aux = _forward_backward(model, Xin, yin, N, hand_rates)
                gnorm = optimizer.step_fused(model, grad_clip, skip_nonfinite=self.skip_nonfinite)
        finally:
            for km in self._maps:
                object.__setattr__(km, "_rate_dev", None)
        self.logits, self.loss = logits.detach(), loss.detach()
        self.targets = yin   # the loss's target of the last replay: y, a Mixup's MixedTargets, a loader's gathered labels
        self.aux = {k: v.detach() for k, v in aux.items()}
        self.gnorm = gnorm
        optimizer.note_replay(-1)   # the capture pass records the step but does not execute it,
        m.step = step0              # nor is it a step of the SOM schedule
        # the graph's gradient buffers and optimizer table stay alive here; the parameters are left as the eager step
        # leaves them (grad None), so an eager step on this model does not accumulate into a replay's gradients
        self._grads = [p.grad for p in m.parameters() if p.grad is not None]
        self._table = optimizer._cache
        optimizer.zero_grad(set_to_none=True)

    def set_lr(self, lr: float) -> None:
        if self.optimizer.schedule is not None:
            raise ValueError("GraphedTrainStep.set_lr: an LRSchedule is attached to the optimizer; the next replay would "
                             "overwrite the rate")
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        self.optimizer.rewrite_hyper(self._table)

    def _advance_som(self) -> None:
        """model.step += 1 per micro-step and, per micro-step and map, the rate the eager forward of that step would
        pass by value, sent to the device scalars on the current stream (ahead of the replay)."""
        m = _unwrap(self.model)
        step0 = m.step
        if self._steps:
            m.step += self.accumulation_steps
        if not self._maps:
            return
        self._rate_ev.synchronize()
        for i in range(self.accumulation_steps):
            lr = m.get_kohonen_lr(step0 + i + 1 if self._steps else step0)
            for j, km in enumerate(self._maps):
                self._rate_pin[i, j] = float(lr) * float(km.alpha)   # rounded to fp32 as the by-value argument is
        self._rate_dev.copy_(self._rate_pin, non_blocking=True)
        self._rate_ev.record()

    def __call__(self, X: torch.Tensor, y: torch.Tensor):
        """One optimizer step on (X, y); returns (logits, loss, aux, grad_norm) as static device tensors that the
        next call overwrites."""
        for b in chain(X):   # any of the captured stages, each the captured object (the batch-object protocol)
            fit = self._fit.get(b.key, (None,))
            if b.stage is not fit[0]:
                raise ValueError(f"GraphedTrainStep: this graph was captured with another {b.word} (or none)")
            if b.fit_key() != fit:
                raise ValueError(f"GraphedTrainStep: this graph was captured with another mean / std of {b.key}.batch "
                                 f"{fit[1:]} (got {b.extra})")
            X = b.inner
        for words, now, captured in self._attached:
            if now() != captured:
                raise ValueError(f"GraphedTrainStep: {words}")
        if "data" in self._fit:
            if not isinstance(X, torch.Tensor) or X.data_ptr() != self.X.data_ptr() or X.shape != self.X.shape or y is not None:
                raise ValueError("GraphedTrainStep: this graph was captured with another dataset tensor: call it with the "
                                 "chain around the captured DeviceLoader.batch() and y=None")
        else:
            self.X.copy_(X, non_blocking=True)
            self.y.copy_(y, non_blocking=True)
        self._advance_som()
        self.graph.replay()
        self.optimizer.note_replay()
        return self.logits, self.loss, self.aux, (self.gnorm[0] if self.gnorm is not None else None)
