"""CPU: the plain-ViT baseline (use_nvit=False) constructs with the reference's parameter set (Q1 repaired), and the
torch restatement the GPU tests use as an oracle reproduces the numbers recorded from the reference itself."""
import os

import numpy as np
import pytest
import torch

from nvit_amd.config import named_config
from nvit_amd.model import ViT
from nvit_amd.weights import formula_state_dict, param_shapes, synthetic_batch

import vit_torch_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("micro", 8), ("mini", 4), ("tiny", 32)]
NVIT_ONLY = ("sz", "sqk", "suv", "attn_alpha", "mlp_alpha")


def _gold(name, batch):
    return np.load(os.path.join(GOLD, f"vit_{name}_b{batch}.npz"))


@pytest.mark.parametrize("name,batch", CASES + [("base", 2)])
def test_state_dict_matches_the_reference(name, batch):
    g = _gold(name, batch)
    m = ViT(named_config(name + "_vit"))
    sd = m.state_dict()
    assert sorted(sd) == list(g["sd_names"])
    assert ["x".join(str(v) for v in sd[n].shape) for n in sorted(sd)] == list(g["sd_shapes"])
    assert {n: tuple(t.shape) for n, t in sd.items()} == param_shapes(m.config)
    for n in sd:
        assert n.split(".")[-1] not in NVIT_ONLY, n
    assert not hasattr(m, "sz")


def test_mini_vit_constructs_with_two_optimizer_groups():
    m = ViT(named_config("mini_vit"))
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")
    assert len(opt.param_groups) == 2
    n_params = sum(len(g["params"]) for g in opt.param_groups)
    assert n_params == len(list(m.parameters()))
    assert all(p.dim() >= 2 for p in opt.param_groups[0]["params"])
    assert all(p.dim() < 2 for p in opt.param_groups[1]["params"])
    assert opt.param_groups[1]["weight_decay"] == 0.0


def test_kohonen_head_with_plain_vit_is_refused():
    with pytest.raises(NotImplementedError, match="use_kohonen"):
        ViT(named_config("mini_vit", use_kohonen=True, kohonen_nodes=32))


def test_head_dim_rules_unchanged_for_plain_vit():
    for heads in (1, 4):   # d = 128, 32
        ViT(named_config("mini_vit", n_head=heads))
    with pytest.raises(ValueError):
        ViT(named_config("mini_vit", n_head=8))   # d = 16
    with pytest.raises(ValueError):
        ViT(named_config("mini_vit", n_embd=96, n_head=1))


@pytest.mark.parametrize("name", ["micro", "mini", "tiny", "base", "large", "micro_k", "mini_k", "base_k"])
def test_nvit_state_dict_unchanged(name):
    """The nViT parameter set keeps its names and shapes (the RMSNorm modules were always built there) and its three
    optimizer groups."""
    cfg = named_config(name)
    sd = ViT(cfg).state_dict()
    shapes = param_shapes(cfg)
    for n, s in shapes.items():
        assert tuple(sd[n].shape) == s, n
    extra = {n for n in sd if n not in shapes and not n.endswith((".locations", ".offsets"))}
    assert not extra, extra
    if not cfg.use_kohonen:
        assert len(ViT(cfg).configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu").param_groups) == 3


def test_formula_weights_load_strictly():
    for name in ("micro_vit", "mini_vit", "tiny_vit"):
        cfg = named_config(name)
        m = ViT(cfg)
        m.load_state_dict(formula_state_dict(cfg), strict=True)
        w = m.transformer.h[0].rmsnorm_att.weight
        assert not torch.equal(w, torch.ones_like(w))   # live in this mode: perturbed around one


@pytest.mark.parametrize("name,batch", CASES)
def test_torch_restatement_reproduces_the_reference(name, batch):
    g = _gold(name, batch)
    cfg = named_config(name + "_vit")
    X, y = synthetic_batch(cfg, batch)
    logits, loss, recon, grads = vit_torch_ref.loss_and_grads(formula_state_dict(cfg), cfg, X, y)
    assert np.abs(logits.numpy() - g["logits"]).max() < 1e-5
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    assert abs(recon.item() - float(g["recon"])) < 1e-5
    assert sorted(grads) == sorted(g["grad_names"])
    for n, gn, head in zip(g["grad_names"], g["grad_norms"], g["grad_heads"]):
        gr = grads[n].reshape(-1)
        assert abs(gr.norm().item() - gn) <= 2e-4 * gn + 1e-8, n
        k = min(8, gr.numel())
        assert np.abs(gr[:k].numpy() - head[:k]).max() <= 2e-4 * np.abs(gr.numpy()).max() + 1e-8, n


def test_autocast_records_are_the_bf16_bar():
    """The reference's own bf16 path deviates measurably from its fp32 path (the bar the GPU bf16 mode is held to)."""
    for name, batch in CASES + [("base", 2)]:
        g = _gold(name, batch)
        d = np.abs(g["logits_autocast"] - g["logits"])
        assert 1e-4 < d.max() < 5e-2, (name, d.max())
