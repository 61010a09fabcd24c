"""Evaluation: the reference trainer's forward-only calls on the HIP path.

`validate` and `estimate_loss` replace Trainer.validate / Trainer.estimate_loss (reference train.py:577-627, 482-506);
`predict` is the forward a served checkpoint runs.  All three run the model in eval mode under torch.no_grad, where
the block functions take their forward-only route (model._lean): the logits are those of `model(X)` bit for bit, but
nothing that only a backward reads is stored.  The per-batch metrics come from one launch (nvit_eval_metrics: loss
and the rank of the target, which replaces F.cross_entropy + topk) and are summed on the device; the host waits once
per call, not up to seven times per batch.
"""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

import torch

from . import ops
from .train import _unwrap, add_aux_losses

Tensor = torch.Tensor
_KOHONEN_KEYS = (("val/consistency_loss", "kohonen_consistency"), ("val/smoothness_loss", "kohonen_smoothness"),
                 ("val/local_quantization_loss", "local_quantization"),
                 ("val/global_quantization_loss", "global_quantization"))


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
    with _eval_mode(model) as m:
        return m._forward(X, False)[0]


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
            logits, aux = m._forward(X, False)
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
            logits, aux = m._forward(X, koh)   # the reconstruction loss is a term of the sum only with the head
            acc = torch.zeros(4, device=logits.device, dtype=torch.float32)
            ops.eval_metrics(logits, y, acc)
            loss = add_aux_losses(m.config, acc[0], aux, consistency_weight, smoothness_weight)
            total = loss if total is None else total + loss
            n += 1
        if total is None:
            raise ValueError("estimate_loss: no batches")
        return total.item() / n
