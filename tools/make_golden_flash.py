"""Golden vectors of the flash_attn=True models - runs ONLY where the reference is importable.

The reference imports `flash_attn_func` unconditionally and calls it when config.flash_attn is set (model.py:7,121-122,
252-253), on tensors of logical shape [B, H, T, d].  flash-attn 2 reads its arguments as [batch, seqlen, nheads, headdim],
so the softmax runs over the H heads of each token.  flash-attn itself is CUDA-only; here the module is
replaced by a stub written for this project that implements flash-attn 2's documented contract: non-causal softmax over
`seqlen` (dim 1) for every (batch, head), arithmetic in fp32 from the given inputs, output in v's dtype, differentiable.

Then, as oracle/make_golden.py (nViT) and tools/make_golden_vit.py (plain ViT, with the §9.1-Q1 repair) do: the real
reference model is imported on the CPU, the closed-form formula weights (nvit_amd/weights.py) are loaded, and small
input/output records are written to tests/golden/fa_*.npz.  Nothing of the reference travels; only these numbers do.

Recorded per case (`fa_<config>_b<batch>.npz`, nViT cases in the renormed weight state the GPU tests run): the sorted
state_dict names and shapes; fp32 logits, loss (the reference loop's total loss) and reconstruction loss (Kohonen: the
four aux losses); per-parameter gradient norms and the first 8 gradient values; the gradient norm and the logits after
one step (clip 1.0, AdamW, renorm for nViT); and the logits under `torch.autocast("cpu", bfloat16)` (train.py:254,905).
Base (B=2) records logits only (fp32 and autocast).

Usage:  python tools/make_golden_flash.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)

import numpy as np
import torch
import torch.nn.functional as F

REF_ROOT = os.environ.get("NVIT_REFERENCE", "/root/reference")


def flash_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, **unused):
    """flash-attn 2's contract: q, k, v [batch, seqlen, nheads, headdim]; softmax(scale * q k^T) v over seqlen for each
    (batch, head); fp32 arithmetic from the given inputs; output [batch, seqlen, nheads, headdim] in v's dtype."""
    assert not causal and dropout_p == 0.0
    scale = softmax_scale if softmax_scale is not None else q.shape[-1] ** -0.5
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))      # [batch, nheads, seqlen, headdim]
    p = torch.softmax(torch.matmul(qf, kf.transpose(-1, -2)) * scale, dim=-1)
    return torch.matmul(p, vf).transpose(1, 2).to(v.dtype)


_stub = types.ModuleType("flash_attn")
_stub.flash_attn_func = flash_attn_func
sys.modules["flash_attn"] = _stub
sys.path.insert(0, REF_ROOT)
import nvit.model as refmod  # noqa: E402

from dataclasses import asdict  # noqa: E402

from nvit_amd.config import named_config  # noqa: E402
from nvit_amd.weights import formula_state_dict, synthetic_batch  # noqa: E402

OUT = os.path.join(_REPO, "tests", "golden")
CASES = [("micro_fa", 8), ("micro_k_fa", 8), ("mini_fa", 4), ("tiny_fa", 32), ("micro_vit_fa", 8)]
LOGITS_ONLY = [("base_fa", 2)]
AUX_KEYS = ("kohonen_consistency", "kohonen_smoothness", "local_quantization", "global_quantization")


def _repair_q1() -> None:
    """Add the two RMSNorm modules the use_nvit=False forward calls, as tools/make_golden_vit.py does."""
    orig = refmod.Block.__init__
    if getattr(orig, "_q1_repaired", False):
        return

    def init(self, config):
        orig(self, config)
        if not config.use_nvit:
            self.rmsnorm_att = refmod.RMSNorm(config.n_embd)
            self.rmsnorm_mlp = refmod.RMSNorm(config.n_embd)

    init._q1_repaired = True
    refmod.Block.__init__ = init


@torch.no_grad()
def _normalize_matrices(model) -> None:
    for blk in model.transformer.h:
        for lin, dim in ((blk.query, 1), (blk.key, 1), (blk.value, 1), (blk.att_c_proj, 0),
                         (blk.c_fc, 1), (blk.mlp_c_proj, 0)):
            w = lin.weight.data
            lin.weight.data.copy_((w.float() / w.float().norm(p=2, dim=dim, keepdim=True)).to(w.dtype))


def _total_loss(cfg, logits, aux, y):
    """train.py:906-926 with settings.yaml consistency_weight = smoothness_weight = 0.1."""
    loss = F.cross_entropy(logits, y)
    if cfg.use_kohonen:
        loss = (loss + 0.1 * aux["kohonen_consistency"] + 0.1 * aux["kohonen_smoothness"]
                + cfg.local_quantization_weight * aux["local_quantization"]
                + cfg.global_quantization_weight * aux["global_quantization"]
                + cfg.reconstruction_weight * aux["reconstruction"])
    return loss


def build_ref(name: str):
    cfg = named_config(name)
    assert cfg.flash_attn
    ref = refmod.ViT(refmod.ViTConfig(**asdict(cfg)))
    res = ref.load_state_dict(formula_state_dict(cfg, perturb_scalars=True), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys), res
    if cfg.use_nvit:
        _normalize_matrices(ref)
    return cfg, ref.train()


def _autocast_logits(name: str, X: torch.Tensor) -> np.ndarray:
    _, ref = build_ref(name)   # fresh module: the Kohonen forward mutates the SOM nodes
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        lbf, _ = ref(X)
    return lbf.float().numpy()


def one_case(name: str, batch: int, full: bool) -> dict:
    cfg, ref = build_ref(name)
    X, y = synthetic_batch(cfg, batch)
    sd = ref.state_dict()
    names = sorted(sd)
    rec = {"sd_names": np.array(names), "sd_shapes": np.array(["x".join(str(v) for v in sd[n].shape) for n in names])}
    if not full:
        with torch.no_grad():
            logits, _ = ref(X)
        rec["logits"] = logits.numpy()
        rec["logits_autocast"] = _autocast_logits(name, X)
        return rec
    logits, aux = ref(X)
    loss = _total_loss(cfg, logits, aux, y)
    loss.backward()
    rec.update({"logits": logits.detach().numpy(), "loss": np.float64(loss.item()),
                "recon": np.float64(aux["reconstruction"].item())})
    if cfg.use_kohonen:
        rec["aux"] = np.array([aux[k].item() for k in AUX_KEYS])
    gnames, gn, heads_ = [], [], []
    for n, p in ref.named_parameters():
        if p.grad is None:
            continue
        gnames.append(n)
        gn.append(p.grad.double().norm().item())
        g = p.grad.reshape(-1)
        heads_.append(g[:8].numpy().copy() if g.numel() >= 8 else np.resize(g.numpy(), 8))
    rec["grad_names"] = np.array(gnames)
    rec["grad_norms"] = np.array(gn)
    rec["grad_heads"] = np.stack(heads_)
    opt = ref.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")
    gnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    opt.step()
    opt.zero_grad(set_to_none=True)
    if cfg.use_nvit:
        _normalize_matrices(ref)
    rec["gnorm"] = np.float64(gnorm.item())
    with torch.no_grad():
        logits1, aux1 = ref(X)
    rec["logits1"] = logits1.numpy()
    rec["loss1"] = np.float64(_total_loss(cfg, logits1, aux1, y).item())
    rec["recon1"] = np.float64(aux1["reconstruction"].item())
    rec["logits_autocast"] = _autocast_logits(name, X)
    return rec


def main() -> None:
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    _repair_q1()
    os.makedirs(OUT, exist_ok=True)
    for (name, batch), full in [(c, True) for c in CASES] + [(c, False) for c in LOGITS_ONLY]:
        rec = one_case(name, batch, full)
        path = os.path.join(OUT, f"fa_{name[:-3]}_b{batch}.npz")
        np.savez_compressed(path, **rec)
        d = np.abs(rec["logits_autocast"] - rec["logits"])
        print(path, os.path.getsize(path), "bytes; autocast max|d| %.3e" % d.max(),
              "loss %.6f" % rec["loss"] if "loss" in rec else "", flush=True)


if __name__ == "__main__":
    main()
