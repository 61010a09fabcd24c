"""Golden vectors of the plain-ViT baseline (use_nvit=False) - runs ONLY where the reference is importable.

Same procedure as oracle/make_golden.py for the nViT path: the real reference model is imported on the CPU (with an
empty `flash_attn` stub: it is only called when config.flash_attn=True), the closed-form formula weights
(nvit_amd/weights.py) are loaded through `load_state_dict`, and small input/output records are written to
tests/golden/vit_*.npz.  Nothing of the reference travels; only these numbers do.

The reference's use_nvit=False path cannot run as shipped: `Block.__init__` builds `rmsnorm_att` / `rmsnorm_mlp` only for
use_nvit=True while `Block.forward` calls them only for use_nvit=False.  The repair applied here is
the one the HIP model implements: after the reference's own constructor has run, the two `RMSNorm(n_embd)` modules are
added (registration order as in the nViT mode, so the state_dict layout is the same), nothing else is changed.

Recorded per case (`vit_<config>_b<batch>.npz`): the sorted state_dict names and shapes; fp32 logits, loss (cross
entropy, the reference loop's loss without the Kohonen head) and the reconstruction aux loss; per-parameter gradient
norms and the first 8 gradient values; the gradient norm and the logits after one AdamW step (clip 1.0; no renorm,
which does nothing for use_nvit=False); and the reference's own bf16 path (`torch.autocast("cpu", bfloat16)` around the
forward, train.py:254,905) as logits.  Base (B=2) records logits only.

Usage:  python tools/make_golden_vit.py
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

_stub = types.ModuleType("flash_attn")


def _no_flash(*a, **k):
    raise RuntimeError("flash_attn is not available here")


_stub.flash_attn_func = _no_flash
sys.modules.setdefault("flash_attn", _stub)
sys.path.insert(0, REF_ROOT)
import nvit.model as refmod  # noqa: E402

from dataclasses import asdict  # noqa: E402

from nvit_amd.config import named_config  # noqa: E402
from nvit_amd.weights import formula_state_dict, synthetic_batch  # noqa: E402

OUT = os.path.join(_REPO, "tests", "golden")
CASES = [("micro_vit", 8), ("mini_vit", 4), ("tiny_vit", 32)]
LOGITS_ONLY = [("base_vit", 2)]


def _repair_q1() -> None:
    """Add the two RMSNorm modules the use_nvit=False forward calls, at run time."""
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


def build_ref(name: str):
    cfg = named_config(name)
    assert not cfg.use_nvit and not cfg.use_kohonen
    ref = refmod.ViT(refmod.ViTConfig(**asdict(cfg)))
    res = ref.load_state_dict(formula_state_dict(cfg, perturb_scalars=True), strict=True)
    assert not res.missing_keys and not res.unexpected_keys, res
    return cfg, ref.train()


def _autocast_logits(name: str, X: torch.Tensor) -> np.ndarray:
    _, ref = build_ref(name)
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
    loss = F.cross_entropy(logits, y)
    loss.backward()
    rec.update({"logits": logits.detach().numpy(), "loss": np.float64(loss.item()),
                "recon": np.float64(aux["reconstruction"].item())})
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
    assert len(opt.param_groups) == 2
    gnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    opt.step()
    opt.zero_grad(set_to_none=True)
    rec["gnorm"] = np.float64(gnorm.item())
    with torch.no_grad():
        logits1, aux1 = ref(X)
    rec["logits1"] = logits1.numpy()
    rec["loss1"] = np.float64(F.cross_entropy(logits1, y).item())
    rec["recon1"] = np.float64(aux1["reconstruction"].item())
    rec["logits_autocast"] = _autocast_logits(name, X)
    return rec


def main() -> None:
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    _repair_q1()
    os.makedirs(OUT, exist_ok=True)
    for (name, batch), full in [(c, True) for c in CASES] + [(c, False) for c in LOGITS_ONLY]:
        rec = one_case(name, batch, full)
        path = os.path.join(OUT, f"vit_{name[:-4]}_b{batch}.npz")
        np.savez_compressed(path, **rec)
        d = np.abs(rec["logits_autocast"] - rec["logits"])
        print(path, os.path.getsize(path), "bytes; autocast max|d| %.3e" % d.max(),
              "loss %.6f" % rec["loss"] if "loss" in rec else "", flush=True)


if __name__ == "__main__":
    main()
