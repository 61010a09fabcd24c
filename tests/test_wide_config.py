"""No GPU: the wide configurations (n_embd 1280 and 2048), the n_embd limit of the model, and the reference fixtures of
tests/test_gpu_wide.py (tools/make_golden_wide.py)."""
import os

import numpy as np
import pytest

from nvit_amd.config import named_config, train_flops_per_image
from nvit_amd.weights import formula_state_dict

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name,C,H,d", [("wide", 1280, 20, 64), ("wide2k", 2048, 16, 128), ("wide_k", 1280, 20, 64)])
def test_wide_configs_construct(name, C, H, d):
    from nvit_amd.model import ViT
    cfg = named_config(name)
    assert (cfg.n_embd, cfg.n_head, cfg.n_embd // cfg.n_head) == (C, H, d)
    assert cfg.use_nvit and cfg.image_size == 32 and cfg.num_classes == 16
    assert cfg.use_kohonen == (name == "wide_k")
    m = ViT(cfg)
    blk = m.transformer.h[-1]
    assert tuple(blk.att_c_proj.weight.shape) == (C, C) and tuple(blk.mlp_c_proj.weight.shape) == (C, 4 * C)
    assert tuple(blk.c_fc.weight.shape) == (8 * C, C)


def test_huge_config_fields():
    """Only the config: building its 630 M parameters on the CPU would cost seconds and gigabytes for nothing."""
    cfg = named_config("huge")
    assert (cfg.image_size, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.num_classes) == (224, 1280, 32, 20, 1000)
    assert cfg.n_embd // cfg.n_head == 64 and cfg.use_nvit and not cfg.use_kohonen
    assert train_flops_per_image(cfg) > 0


def test_n_embd_over_2048_is_refused_at_construction():
    from nvit_amd.model import ViT
    with pytest.raises(ValueError, match="2048"):
        ViT(named_config("mini", n_embd=2112, n_head=33))
    ViT(named_config("mini", n_embd=2048, n_head=32, n_layer=1))   # the limit itself is accepted


@pytest.mark.parametrize("name", ["wide", "wide2k", "wide_k"])
def test_wide_fixtures_match_the_formula_weights(name):
    path = os.path.join(GOLD, f"{name}_b2.npz")
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
