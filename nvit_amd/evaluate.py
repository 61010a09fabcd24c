"""Evaluation: the reference trainer's forward-only calls on the HIP path.

`validate` and `estimate_loss` replace Trainer.validate / Trainer.estimate_loss (reference train.py:577-627, 482-506);
`predict` is the forward a served checkpoint runs.  All three run the model in eval mode under torch.no_grad, where
the block functions take their forward-only route (model._lean): the logits are those of `model(X)` bit for bit, but
nothing that only a backward reads is stored.  The per-batch metrics come from one launch (nvit_eval_metrics: loss
and the rank of the target, which replaces F.cross_entropy + topk) and are summed on the device; the host waits once
per call, not up to seven times per batch.

Wherever X stands, a `ResizeCenterCrop.batch(u8)` (crop.py) may stand instead: evaluation from the stored uint8 data.  The
transform's two launches then run in front of the forward on the current stream, with no host synchronisation.
"""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

import torch

from . import ops
from .stages import StagedBatch, chain
from .train import _unwrap, add_aux_losses

Tensor = torch.Tensor
_KOHONEN_KEYS = (("val/consistency_loss", "kohonen_consistency"), ("val/smoothness_loss", "kohonen_smoothness"),
                 ("val/local_quantization_loss", "local_quantization"),
                 ("val/global_quantization_loss", "global_quantization"))


def _split(X) -> tuple:
    """X of an evaluation call -> (its fit key, its tensor): those of a `ResizeCenterCrop.batch(u8)`, the one batch object
    that is no stage of a train step (stages.py); (None, X) for anything else.  A chain on a `DeviceLoader.batch()` (data.py)
    is refused: it draws a training batch and advances the loader."""
    if any(b.key == "data" for b in chain(X)):
        raise TypeError("a DeviceLoader.batch() is a train step's input; evaluation takes DeviceDataset.eval_batches(...)")
    return (X.fit_key(), X.source()) if isinstance(X, StagedBatch) and X.key is None else (None, X)


def _model_input(X):
    """X of an evaluation call -> the model's input: a `ResizeCenterCrop.batch(u8)` runs its two launches here."""
    return X.resolve()[0] if _split(X)[0] is not None else X


class _eval_mode:
    """eval() + no_grad for the duration; the module's `training` flag is put back as it was.  A CPU-resident model
    is refused here with ViT._prepare's error, before anything is changed."""

    def __init__(self, model):
        self.m = _unwrap(model)
        dev = next(self.m.parameters()).device
        if dev.type != "cuda":
            self.m._prepare(dev)   # raises
        self.no_grad = torch.no_grad()

    def __enter__(self):
        self.was = self.m.training
        self.m.eval()
        self.no_grad.__enter__()
        return self.m

    def __exit__(self, *exc):
        self.no_grad.__exit__(*exc)
        self.m.train(self.was)
        return False


def predict(model, X: Tensor) -> Tensor:
    """Logits of `model(X)` (bit-identical) from the forward-only route, without the reconstruction head: its GEMM,
    its loss kernel and the stream's bf16 copy that only it reads (plain ViT) are skipped."""
    _split(X)   # (refuses a loader's batch before anything else)
    with _eval_mode(model) as m:
        return m._forward(_model_input(X), False)[0]


def validate(model, batches: Iterable[Tuple[Tensor, Tensor]], consistency_weight: float = 0.1,
             smoothness_weight: float = 0.1) -> Dict[str, float]:
    """Trainer.validate (reference train.py:577-627) over `batches` of (X, y) on the device: val/loss, val/top1_accuracy,
    val/top5_accuracy (top-min(5, classes)), each the mean over batches of the per-batch value as the reference
    reports them (with a short last batch that is not the mean over samples), plus, with the Kohonen head, the four
    unweighted val/*_loss terms.  The two weights are taken for call compatibility with estimate_loss; like the
    reference, validate reports the terms unweighted.  One host synchronisation, at the end."""
    with _eval_mode(model) as m:
        koh = m.config.use_kohonen
        acc = aux_acc = None
        for X, y in batches:
            # (the reconstruction term is not among the reported ones: the head is left out with the Kohonen head too)
            logits, aux = m._forward(_model_input(X), False)
            if acc is None:
                acc = torch.zeros(4, device=logits.device, dtype=torch.float32)
                aux_acc = torch.zeros(len(_KOHONEN_KEYS), device=logits.device, dtype=torch.float32)
            ops.eval_metrics(logits, y, acc)
            if koh:
                aux_acc += torch.stack([aux[k].reshape(()) for _, k in _KOHONEN_KEYS])
        if acc is None:
            raise ValueError("validate: no batches")
        host = torch.cat([acc, aux_acc]).tolist()   # the call's one synchronisation
    n = host[3]
    out = {"val/loss": host[0] / n, "val/top1_accuracy": host[1] / n, "val/top5_accuracy": host[2] / n}
    if koh:
        out.update({name: host[4 + i] / n for i, (name, _) in enumerate(_KOHONEN_KEYS)})
    return out


def estimate_loss(model, batches: Iterable[Tuple[Tensor, Tensor]], eval_iters: int, consistency_weight: float = 0.1,
                  smoothness_weight: float = 0.1) -> float:
    """One split of Trainer.estimate_loss (reference train.py:482-506): the mean, over the first `eval_iters` batches
    (fewer if `batches` ends first), of the cross-entropy plus - iff the Kohonen head is on - the weighted aux losses
    of the training loss (train.add_aux_losses).  One host synchronisation, at the end."""
    if eval_iters < 1:
        raise ValueError("estimate_loss: eval_iters must be at least 1")
    with _eval_mode(model) as m:
        koh = m.config.use_kohonen
        total, n = None, 0
        for X, y in batches:
            if n >= eval_iters:
                break
            # (the reconstruction loss is a term of the sum only with the head)
            logits, aux = m._forward(_model_input(X), koh)
            acc = torch.zeros(4, device=logits.device, dtype=torch.float32)
            ops.eval_metrics(logits, y, acc)
            loss = add_aux_losses(m.config, acc[0], aux, consistency_weight, smoothness_weight)
            total = loss if total is None else total + loss
            n += 1
        if total is None:
            raise ValueError("estimate_loss: no batches")
        return total.item() / n


class GraphedEval:
    """`predict`, `validate` and `estimate_loss` with the forward of one batch shape captured as hipGraphs and replayed:
    a small model's evaluation is bound by its few hundred launches per batch, like its train step (GraphedTrainStep).

    Two graphs are captured for the shape, dtype and device of (X, y).  `predict` and `validate` share one: the
    forward-only route without the reconstruction head, nvit_eval_metrics adding into a device accumulator that
    `validate` zeroes once per call, and the stacked Kohonen terms adding into a second one (`predict` ignores both
    and returns a copy of the logits).  `estimate_loss` has its own, because with the Kohonen head its forward runs the
    reconstruction head: it zeroes a per-batch accumulator, runs nvit_eval_metrics, weights the aux terms
    (train.add_aux_losses, with the two weights given here) and adds the batch's loss to the running total.  These are
    the fp32 additions of the module-level functions in their order, so every result is bit-identical to theirs.  A
    batch of another shape, dtype or device (the short last batch of a loader) runs eagerly through the same code.

    The weight shadows are rebuilt inside the captured forward, so weight changes between calls (training) are picked
    up.  Every call restores the model's `training` flag and leaves `model.step` and the SOM nodes alone.  The object is
    invalid after `model.set_precision(...)` and after anything that reallocates the parameters or the SOM nodes
    (`model.to(...)`, loading a state dict by assignment, a resize): the graphs hold their addresses; build a new one.

    With `ViT.set_dynamic_img_size(True)` X may have another image size than the model's: the captured forward then holds
    the resampling of the position tables, which reads the parameters on every replay like the weight shadows do, so
    training between two calls is picked up.  `ViT.set_input_size` replaces the two parameters: every call afterwards
    raises ValueError.

    X may be a `ResizeCenterCrop.batch(u8)`: the transform's two launches are captured with the forward, and the static
    input is the uint8 source.  Which batches then fit the graphs, and that anything else (a plain tensor too, or such an
    object on graphs built on a tensor) runs eagerly: DESIGN.md §7, "The batch-object protocol".
    """

    def __init__(self, model, X, y: Tensor, consistency_weight: float = 0.1, smoothness_weight: float = 0.1):
        _split(X)   # (refuses a loader's batch before anything else)
        self.model = model
        self.cw, self.sw = consistency_weight, smoothness_weight
        self._size_epoch = _unwrap(model)._size_epoch
        with _eval_mode(model) as m:   # (refuses a CPU-resident model before anything is changed)
            if X.device.type != "cuda" or y.device != X.device:
                raise RuntimeError("GraphedEval: inputs must live on the HIP device")
            # the static input: the tensor, or the uint8 source under the transform that `_static` wraps around it
            self._fit, src = _split(X)
            self.X = X.clone() if self._fit is None else src.clone(memory_format=torch.contiguous_format)
            self._static = self.X if self._fit is None else X.rebind(self.X)
            self.y = y.clone()
            dev = X.device
            self._acc = torch.zeros(4, device=dev, dtype=torch.float32)
            self._aux_acc = torch.zeros(len(_KOHONEN_KEYS), device=dev, dtype=torch.float32)
            self._bacc = torch.zeros(4, device=dev, dtype=torch.float32)
            self._total = torch.zeros((), device=dev, dtype=torch.float32)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):   # builds every cache (shadow tables, LDS attributes) ahead of the capture
                self._metrics_batch(m, self._static, self.y)
                self._loss_batch(m, self._static, self.y)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self._g_metrics, self._g_loss = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g_metrics, stream=side):
                self._logits = self._metrics_batch(m, self._static, self.y)
            with torch.cuda.graph(self._g_loss, stream=side):
                self._loss_batch(m, self._static, self.y)

    # ---- one batch, eagerly or under capture: the loop bodies of validate / estimate_loss on this object's accumulators
    def _metrics_batch(self, m, X, y: Tensor) -> Tensor:
        logits, aux = m._forward(_model_input(X), False)
        ops.eval_metrics(logits, y, self._acc)
        if m.config.use_kohonen:
            self._aux_acc += torch.stack([aux[k].reshape(()) for _, k in _KOHONEN_KEYS])
        return logits

    def _loss_batch(self, m, X, y: Tensor) -> None:
        logits, aux = m._forward(_model_input(X), m.config.use_kohonen)
        self._bacc.zero_()
        ops.eval_metrics(logits, y, self._bacc)
        self._total += add_aux_losses(m.config, self._bacc[0], aux, self.cw, self.sw)

    def _check_model(self) -> None:
        if _unwrap(self.model)._size_epoch != self._size_epoch:
            raise ValueError("GraphedEval: ViT.set_input_size replaced the position embeddings these graphs were captured "
                             "with; build a new GraphedEval")

    def _fits_x(self, X) -> bool:
        fit, X = _split(X)
        return fit == self._fit and X.shape == self.X.shape and X.dtype == self.X.dtype and X.device == self.X.device

    def _fits(self, X, y: Tensor) -> bool:
        return self._fits_x(X) and y.shape == self.y.shape and y.dtype == self.y.dtype and y.device == self.y.device

    def _load_x(self, X) -> None:
        self.X.copy_(_split(X)[1], non_blocking=True)

    def _load(self, X, y: Tensor) -> None:
        self._load_x(X)
        self.y.copy_(y, non_blocking=True)

    def predict(self, X) -> Tensor:
        """evaluate.predict(model, X); a new tensor."""
        self._check_model()
        if not self._fits_x(X):
            return predict(self.model, X)
        with _eval_mode(self.model):
            self._load_x(X)
            self._g_metrics.replay()
            return self._logits.clone()

    def validate(self, batches: Iterable[Tuple[Tensor, Tensor]]) -> Dict[str, float]:
        """evaluate.validate(model, batches)."""
        self._check_model()
        with _eval_mode(self.model) as m:
            koh = m.config.use_kohonen
            self._acc.zero_()
            self._aux_acc.zero_()
            n = 0
            for X, y in batches:
                if self._fits(X, y):
                    self._load(X, y)
                    self._g_metrics.replay()
                else:
                    self._metrics_batch(m, X, y)
                n += 1
            if n == 0:
                raise ValueError("validate: no batches")
            host = torch.cat([self._acc, self._aux_acc]).tolist()   # the call's one synchronisation
        n = host[3]
        out = {"val/loss": host[0] / n, "val/top1_accuracy": host[1] / n, "val/top5_accuracy": host[2] / n}
        if koh:
            out.update({name: host[4 + i] / n for i, (name, _) in enumerate(_KOHONEN_KEYS)})
        return out

    def estimate_loss(self, batches: Iterable[Tuple[Tensor, Tensor]], eval_iters: int) -> float:
        """evaluate.estimate_loss(model, batches, eval_iters) with the weights given to the constructor."""
        self._check_model()
        if eval_iters < 1:
            raise ValueError("estimate_loss: eval_iters must be at least 1")
        with _eval_mode(self.model) as m:
            self._total.zero_()
            n = 0
            for X, y in batches:
                if n >= eval_iters:
                    break
                if self._fits(X, y):
                    self._load(X, y)
                    self._g_loss.replay()
                else:
                    self._loss_batch(m, X, y)
                n += 1
            if n == 0:
                raise ValueError("estimate_loss: no batches")
            return self._total.item() / n
