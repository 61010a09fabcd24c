"""CPU: the flash_attn=True configurations (the reference's head-axis attention) construct with the
reference's parameter set, refuse head counts the kernels are not built for, and the torch restatement the GPU tests use
as an oracle (tests/fa_torch_ref.py) reproduces the numbers recorded from the reference itself (tests/golden/fa_*.npz,
tools/make_golden_flash.py)."""
import os

import numpy as np
import pytest
import torch

from nvit_amd.config import named_config
from nvit_amd.model import ViT
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

import fa_torch_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NVIT_CASES = [("micro", 8), ("micro_k", 8), ("mini", 4), ("tiny", 32)]
AUX_KEYS = ("kohonen_consistency", "kohonen_smoothness", "local_quantization", "global_quantization")


def _gold(name, batch):
    return np.load(os.path.join(GOLD, f"fa_{name}_b{batch}.npz"))


def oracle_params(cfg):
    p = O.make_params(formula_state_dict(cfg))
    O.renorm_(p, cfg)
    return p


@pytest.mark.parametrize("name", ["micro", "micro_k", "mini", "tiny", "base", "micro_vit"])
def test_fa_configs_are_the_plain_configs_with_flash_attn(name):
    cfg, fa = named_config(name), named_config(name + "_fa")
    assert fa.flash_attn and not cfg.flash_attn
    assert {**vars(fa), "flash_attn": False} == vars(cfg)


@pytest.mark.parametrize("name,batch", NVIT_CASES + [("micro_vit", 8), ("base", 2)])
def test_state_dict_matches_the_reference(name, batch):
    g = _gold(name, batch)
    sd = ViT(named_config(name + "_fa")).state_dict()
    names = sorted(n for n in sd if not n.endswith((".locations", ".offsets")))
    rec = [n for n in g["sd_names"] if not n.endswith((".locations", ".offsets"))]
    assert names == rec


def test_head_count_limit_only_with_flash_attn():
    over = dict(n_embd=1088, n_head=34, n_layer=1)   # head dim 32, 34 heads
    with pytest.raises(ValueError, match="at most 32 heads"):
        ViT(named_config("micro_fa", **over))
    ViT(named_config("micro", **over))               # the SDPA form has no such limit
    ViT(named_config("micro_fa", n_embd=1024, n_head=32, n_layer=1))


@pytest.mark.parametrize("name,batch", NVIT_CASES)
def test_nvit_restatement_reproduces_the_reference(name, batch):
    g = _gold(name, batch)
    cfg = named_config(name + "_fa")
    X, y = synthetic_batch(cfg, batch)
    p = oracle_params(cfg)
    with fa_torch_ref.nvit_flash():
        logits, loss, aux = O.loss_and_grads(p, cfg, X, y, want_aux=True)
    tol = 2e-5 if cfg.use_kohonen else 1e-5
    assert np.abs(logits.numpy() - g["logits"]).max() < tol
    assert abs(loss.item() - float(g["loss"])) < tol
    assert abs(aux["reconstruction"].item() - float(g["recon"])) < 1e-5
    if cfg.use_kohonen:
        assert np.abs(np.array([aux[k].item() for k in AUX_KEYS]) - g["aux"]).max() < 1e-5
    grads = {n: t.grad for n, t in p.items() if t.grad is not None}
    for n, gn, head in zip(g["grad_names"], g["grad_norms"], g["grad_heads"]):
        gr = grads[n].reshape(-1)
        assert abs(gr.double().norm().item() - gn) <= 2e-4 * gn + 1e-8, n
        k = min(8, gr.numel())
        assert np.abs(gr[:k].numpy() - head[:k]).max() <= 2e-4 * np.abs(gr.numpy()).max() + 1e-8, n


@pytest.mark.parametrize("name,batch", [("micro", 8), ("mini", 4)])
def test_nvit_restatement_one_step(name, batch):
    g = _gold(name, batch)
    cfg = named_config(name + "_fa")
    X, y = synthetic_batch(cfg, batch)
    p = oracle_params(cfg)
    opt = O.make_optimizer(p)
    with fa_torch_ref.nvit_flash():
        _, _, _, gnorm = O.train_step(p, cfg, opt, X, y)
        with torch.no_grad():
            logits1, _ = O.forward(p, cfg, X)
    assert abs(gnorm.item() - float(g["gnorm"])) <= 2e-4 * float(g["gnorm"])
    assert np.abs(logits1.numpy() - g["logits1"]).max() < 2e-4


def test_vit_restatement_reproduces_the_reference():
    g = _gold("micro_vit", 8)
    cfg = named_config("micro_vit_fa")
    X, y = synthetic_batch(cfg, 8)
    logits, loss, recon, grads = fa_torch_ref.vit_loss_and_grads(formula_state_dict(cfg), cfg, X, y)
    assert np.abs(logits.numpy() - g["logits"]).max() < 1e-5
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    assert abs(recon.item() - float(g["recon"])) < 1e-5
    assert sorted(grads) == sorted(g["grad_names"])
    for n, gn, head in zip(g["grad_names"], g["grad_norms"], g["grad_heads"]):
        gr = grads[n].reshape(-1)
        assert abs(gr.norm().item() - gn) <= 2e-4 * gn + 1e-8, n
        k = min(8, gr.numel())
        assert np.abs(gr[:k].numpy() - head[:k]).max() <= 2e-4 * np.abs(gr.numpy()).max() + 1e-8, n


def test_base_restatement_logits():
    g = _gold("base", 2)
    cfg = named_config("base_fa")
    X, _ = synthetic_batch(cfg, 2)
    with fa_torch_ref.nvit_flash(), torch.no_grad():
        logits, _ = O.forward(oracle_params(cfg), cfg, X)
    assert np.abs(logits.numpy() - g["logits"]).max() < 2e-5


@pytest.mark.parametrize("name,batch", NVIT_CASES + [("micro_vit", 8), ("base", 2)])
def test_flash_attn_changes_the_model(name, batch):
    """The recorded flash_attn=True logits are not those of the SDPA form (a model-level difference, not rounding), and
    the reference's own bf16 path deviates measurably from its fp32 path (the bf16 bar of the GPU tests)."""
    g = _gold(name, batch)
    cfg = named_config(name)
    X, _ = synthetic_batch(cfg, batch)
    if cfg.use_nvit:
        with torch.no_grad():
            sdpa, _ = O.forward(oracle_params(cfg), cfg, X)
    else:
        import vit_torch_ref
        with torch.no_grad():
            sdpa, _ = vit_torch_ref.forward(formula_state_dict(cfg), cfg, X)
    assert np.abs(sdpa.numpy() - g["logits"]).max() > 1e-3
    d = np.abs(g["logits_autocast"] - g["logits"]).max()
    assert 1e-4 < d < 5e-2, d
