"""No GPU: head dims 72, 80, 88 and 104 (zero-padded to the 128-wide attention kernels) are accepted by the model, the
named configs that use them, and their reference fixtures (tools/make_golden_headdim.py), which the CPU oracle and the
float64 plain-ViT restatement reproduce at the bars of tests/test_oracle_golden.py / tests/test_vit_baseline_config.py."""
import os

import numpy as np
import pytest
import torch

from nvit_amd.config import named_config, train_flops_per_image
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

import vit_torch_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SMALL = [("hd80", 80), ("hd72", 72), ("hd104_b", 104), ("hd88_vit", 88), ("hd80_k", 80)]
NVIT_CASES = [("hd80", 4), ("hd72", 2), ("hd80_k", 2), ("hd104_b", 2)]


@pytest.mark.parametrize("name,d", SMALL)
def test_padded_head_dim_configs_construct(name, d):
    from nvit_amd.model import HEAD_DIMS, PADDED_HEAD_DIMS, ViT
    assert HEAD_DIMS == (32, 64, 128) and PADDED_HEAD_DIMS == (72, 80, 88, 104)
    cfg = named_config(name)
    assert cfg.n_embd // cfg.n_head == d and cfg.n_embd % cfg.n_head == 0 and cfg.num_classes == 16
    assert cfg.use_nvit == (name != "hd88_vit") and cfg.use_kohonen == (name == "hd80_k") and cfg.bias == (name == "hd104_b")
    m = ViT(cfg)
    assert m.set_precision("bf16")._attn_impl() == 1
    assert m.set_precision("fp32")._attn_impl() == 0
    assert tuple(m.transformer.h[0].query.weight.shape) == (cfg.n_embd, cfg.n_embd)


def test_hd80_geometry():
    from nvit_amd.model import ViT
    cfg = named_config("hd80")
    assert (cfg.image_size, cfg.n_embd, cfg.n_head, cfg.n_layer) == (56, 320, 4, 2)
    assert ViT(cfg).n_tokens == 49   # ragged: no multiple of any attention tile


def test_huge16_constructs():
    """The true ViT-H geometry.  Built on the meta device: the constructor runs whole, without the seconds and gigabytes
    that 630 M parameters cost on the CPU."""
    from nvit_amd.model import PADDED_HEAD_DIMS
    cfg = named_config("huge16")
    assert (cfg.image_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.num_classes) == (224, 1280, 32, 16, 1000)
    assert cfg.n_embd // cfg.n_head == 80 and 80 in PADDED_HEAD_DIMS and cfg.use_nvit and not cfg.flash_attn
    assert train_flops_per_image(cfg) == train_flops_per_image(named_config("huge"))
    from nvit_amd.model import ViT
    with torch.device("meta"):
        m = ViT(cfg)
    assert len(m.transformer.h) == 32 and m.n_tokens == 784
    assert tuple(m.transformer.h[31].query.weight.shape) == (1280, 1280)
    assert m.set_precision("bf16")._attn_impl() == 1 and m.set_precision("fp32")._attn_impl() == 0


def test_flash_attn_with_a_padded_head_dim_is_refused():
    from nvit_amd.model import ViT
    with pytest.raises(ValueError, match="flash_attn"):
        ViT(named_config("hd80", flash_attn=True))


def test_other_head_dims_are_still_refused():
    from nvit_amd.model import ViT
    for n_embd, n_head in ((192, 12), (192, 4), (192, 2), (640, 16), (320, 5)):   # 16, 48, 96, 40, 64
        if n_embd // n_head == 64:
            ViT(named_config("mini", n_embd=n_embd, n_head=n_head, n_layer=1))
            continue
        with pytest.raises(ValueError, match="32, 64, 128"):
            ViT(named_config("mini", n_embd=n_embd, n_head=n_head))


@pytest.mark.parametrize("name,batch", NVIT_CASES)
def test_nvit_fixtures_match_the_formula_weights(name, batch):
    path = os.path.join(GOLD, f"{name}_b{batch}.npz")
    assert os.path.exists(path), path
    g = np.load(path)
    sd = formula_state_dict(named_config(name))
    names = sorted(sd)
    assert [str(n) for n in g["sd_names"]] == names
    assert [str(s) for s in g["sd_shapes"]] == ["x".join(str(v) for v in sd[n].shape) for n in names]
    for k in ("logits", "loss", "recon", "grad_names", "grad_norms", "grad_heads", "gnorm", "logits1", "q0_head1",
              "p_last_head1", "logits_fp32", "logits_autocast_bf16", "max_abs_dev"):
        assert k in g.files, k
    assert os.path.getsize(path) < 1 << 20
    dev = np.abs(g["logits_autocast_bf16"] - g["logits_fp32"]).max()
    assert abs(dev - float(g["max_abs_dev"])) < 1e-9 and dev > 1e-4       # a bf16 path, not a copy of the fp32 one


@pytest.mark.parametrize("name,batch", NVIT_CASES)
def test_oracle_reproduces_the_nvit_fixtures(name, batch):
    """The body and bars of test_oracle_matches_reference_golden (tests/test_oracle_golden.py), renormalised state."""
    torch.set_num_threads(4)
    g = np.load(os.path.join(GOLD, f"{name}_b{batch}.npz"))
    cfg = named_config(name)
    p = O.make_params(formula_state_dict(cfg, perturb_scalars=True))
    O.renorm_(p, cfg)
    X, y = synthetic_batch(cfg, batch)
    opt = O.make_optimizer(p)
    logits, loss, aux = O.loss_and_grads(p, cfg, X, y, step=1, want_aux=True)
    assert np.abs(logits.numpy() - g["logits"]).max() < 2e-5
    assert np.abs(logits.numpy() - g["logits_fp32"]).max() < 2e-5
    assert abs(loss.item() - float(g["loss"])) < 2e-5 * max(1.0, float(g["loss"]))
    assert abs(aux["reconstruction"].item() - float(g["recon"])) < 2e-5
    if cfg.use_kohonen:
        got = np.array([aux[k].item() for k in ("kohonen_consistency", "kohonen_smoothness", "local_quantization",
                                                 "global_quantization")])
        assert np.abs(got - g["aux"]).max() < 2e-5 * max(1.0, np.abs(g["aux"]).max())
        ln = p["local_kohonen.nodes"].detach().reshape(-1)[:8].numpy()
        gn = p["global_kohonen.nodes"].detach().reshape(-1)[:8].numpy()
        assert np.abs(ln - g["lnodes_head"]).max() < 2e-6 and np.abs(gn - g["gnodes_head"]).max() < 2e-6
    names = [str(n) for n in g["grad_names"]]
    assert {n for n, t in p.items() if t.grad is not None} == set(names)
    for n, gn, gh in zip(names, g["grad_norms"], g["grad_heads"]):
        grad = p[n].grad
        mine = grad.double().norm().item()
        assert abs(mine - gn) <= 2e-4 * gn + 1e-7, (n, mine, gn)
        head = grad.reshape(-1)[:8].numpy() if grad.numel() >= 8 else np.resize(grad.reshape(-1).numpy(), 8)
        assert np.abs(head - gh).max() <= 2e-4 * max(np.abs(gh).max(), 1e-30) + 2e-7, n
    gnorm = torch.nn.utils.clip_grad_norm_([t for t in p.values() if t.grad is not None], 1.0)
    assert abs(gnorm.item() - float(g["gnorm"])) < 2e-4 * float(g["gnorm"])
    opt.step()
    opt.zero_grad(set_to_none=True)
    O.renorm_(p, cfg)
    with torch.no_grad():
        logits1, aux1 = O.forward(p, cfg, X, training=True, step=2)
        loss1 = O.total_loss(cfg, logits1, aux1, y)
    assert np.abs(logits1.numpy() - g["logits1"]).max() < 5e-5
    assert abs(loss1.item() - float(g["loss1"])) < 5e-5 * max(1.0, float(g["loss1"]))
    assert abs(aux1["reconstruction"].item() - float(g["recon1"])) < 5e-5
    q0 = p["transformer.h.0.query.weight"].detach().reshape(-1)[:8].numpy()
    assert np.abs(q0 - g["q0_head1"]).max() < 1e-6
    pl = p[f"transformer.h.{cfg.n_layer - 1}.mlp_c_proj.weight"].detach().reshape(-1)[:8].numpy()
    assert np.abs(pl - g["p_last_head1"]).max() < 1e-6


def test_torch_restatement_reproduces_the_plain_vit_fixture():
    """The body and bars of test_torch_restatement_reproduces_the_reference (tests/test_vit_baseline_config.py)."""
    path = os.path.join(GOLD, "hd88_vit_b2.npz")
    g = np.load(path)
    assert os.path.getsize(path) < 1 << 20
    cfg = named_config("hd88_vit")
    sd = formula_state_dict(cfg)
    names = sorted(sd)
    assert [str(n) for n in g["sd_names"]] == names
    assert [str(s) for s in g["sd_shapes"]] == ["x".join(str(v) for v in sd[n].shape) for n in names]
    X, y = synthetic_batch(cfg, 2)
    logits, loss, recon, grads = vit_torch_ref.loss_and_grads(sd, cfg, X, y)
    assert np.abs(logits.numpy() - g["logits"]).max() < 1e-5
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    assert abs(recon.item() - float(g["recon"])) < 1e-5
    assert sorted(grads) == sorted(g["grad_names"])
    for n, gn, head in zip(g["grad_names"], g["grad_norms"], g["grad_heads"]):
        gr = grads[n].reshape(-1)
        assert abs(gr.norm().item() - gn) <= 2e-4 * gn + 1e-8, n
        k = min(8, gr.numel())
        assert np.abs(gr[:k].numpy() - head[:k]).max() <= 2e-4 * np.abs(gr.numpy()).max() + 1e-8, n
    d = np.abs(g["logits_autocast"] - g["logits"])
    assert 1e-4 < d.max() < 5e-2
