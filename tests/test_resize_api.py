"""CPU: the argument checks of the image-size feature, all raised before any device work (this file runs without a GPU):
ViT.forward on images it cannot take, ViT.set_input_size, ViT.set_dynamic_img_size, nvit_amd.resample_pos_embed,
load_checkpoint(image_size=...), and the new entry points of the C header."""
import dataclasses
import os
import re

import pytest
import torch

from nvit_amd.config import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model(name="micro"):
    from nvit_amd.model import ViT
    return ViT(named_config(name))


def test_forward_refuses_what_it_cannot_take_before_any_device_work():
    m = model()                                        # 32 px, patches 8 / 16
    step = m.step
    for shape in ((2, 3, 32, 40), (2, 3, 40, 32)):     # non-square, with the flag off and on
        for flag in (False, True):
            m.set_dynamic_img_size(flag)
            with pytest.raises(ValueError, match="square"):
                m(torch.zeros(shape))
    m.set_dynamic_img_size(False)
    for S in (48, 36, 16):                             # another size with the flag off
        with pytest.raises(ValueError, match="set_dynamic_img_size"):
            m(torch.zeros(2, 3, S, S))
    m.set_dynamic_img_size(True)
    with pytest.raises(ValueError, match="multiple"):  # not a multiple of the local patch
        m(torch.zeros(2, 3, 36, 36))
    with pytest.raises(ValueError, match="taps"):      # grid 4 -> 40: over the tap cap
        m(torch.zeros(1, 3, 320, 320))
    with pytest.raises(ValueError):
        m(torch.zeros(3, 32, 32))
    assert m.step == step and m._rt.grid is None and m._rt.tokens is None
    # the sizes it does take reach the device check (a CPU tensor: RuntimeError, as for the native size)
    for S in (32, 48):
        with pytest.raises(RuntimeError):
            m(torch.zeros(2, 3, S, S))
    assert m._rt.grid is None


def test_reflect_pad_must_be_smaller_than_the_image():
    from nvit_amd.model import ViT
    m = ViT(named_config("micro", image_size=32, local_patch_size=4, global_patch_size=12))   # pad 4
    m.set_dynamic_img_size(True)
    with pytest.raises(ValueError, match="reflect pad"):
        m(torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="reflect pad"):
        m.set_input_size(4)


def test_set_input_size_to_the_current_size_is_a_no_op():
    m = model()
    cfg = m.config
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ids = (id(m.local_pos_embed), id(m.global_pos_embed))
    assert m.set_input_size(32) is m
    assert m.config is cfg and m.n_tokens == 16 and m._size_epoch == 0
    assert ids == (id(m.local_pos_embed), id(m.global_pos_embed))
    after = m.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_set_input_size_argument_checks():
    m = model()
    for bad in (36, 0, -32, 32.0, True, None, "48"):
        with pytest.raises(ValueError):
            m.set_input_size(bad)
    with pytest.raises(ValueError, match="taps"):
        m.set_input_size(320)
    with pytest.raises(RuntimeError, match="HIP device"):   # a real resize needs the device: no CPU fallback
        m.set_input_size(48)
    assert m.config.image_size == 32 and m.n_tokens == 16 and m._size_epoch == 0


def test_dynamic_flag_defaults_to_off_and_is_no_config_field():
    from nvit_amd.config import ViTConfig
    m = model()
    assert m._dynamic_img_size is False
    assert m.set_dynamic_img_size(True) is m and m._dynamic_img_size is True
    assert m.set_dynamic_img_size(False)._dynamic_img_size is False
    assert "dynamic_img_size" not in {f.name for f in dataclasses.fields(ViTConfig)}
    assert len(dataclasses.fields(ViTConfig)) == 26            # the reference's dataclass, field for field
    assert "_dynamic_img_size" not in m.state_dict()


def test_resample_pos_embed_argument_checks():
    import nvit_amd
    f = nvit_amd.resample_pos_embed
    p = torch.zeros(1, 16, 64)
    p2 = p[0]
    assert f(p, 4) is p and f(p2, 4) is p2                     # equal grids: the table itself
    for bad in (torch.zeros(2, 16, 64), torch.zeros(16), torch.zeros(1, 15, 64), torch.zeros(1, 16, 62),
                torch.zeros(1, 16, 4096), torch.zeros(1, 16, 64, dtype=torch.float64)):
        with pytest.raises(ValueError):
            f(bad, 7)
    for grid in (0, -3, 7.0, True):
        with pytest.raises(ValueError):
            f(p, grid)
    with pytest.raises(ValueError, match="taps"):
        f(p, 40)
    with pytest.raises(RuntimeError, match="HIP device"):
        f(p, 7)


def test_load_checkpoint_refuses_a_stale_optimizer_state(tmp_path):
    from nvit_amd.checkpoint import load_checkpoint, save_checkpoint
    m = model()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    save_checkpoint(tmp_path / "ck.pt", m, opt, 0, {})
    with pytest.raises(ValueError, match="optimizer"):
        load_checkpoint(tmp_path / "ck.pt", "cpu", optimizer_factory=lambda mm: torch.optim.AdamW(mm.parameters()),
                        image_size=48)
    m2, opt2, ck = load_checkpoint(tmp_path / "ck.pt", "cpu", image_size=32)   # the saved size: a plain load
    assert opt2 is None and ck["model_args"]["image_size"] == 32 and m2.n_tokens == 16
    assert torch.equal(m2.local_pos_embed, m.local_pos_embed)


def test_header_declares_the_entry_points_and_the_tap_cap():
    from nvit_amd import _lib, resample
    h = open(os.path.join(ROOT, "include", "nvit_hip.h")).read()
    for name in ("nvit_pos_resample_fwd", "nvit_pos_resample_bwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 9
    assert resample.MAX_TAPS == _lib.const("POS_RESAMPLE_MAX_TAPS") == 32
    assert len(re.findall(r"#define\s+NVIT_POS_RESAMPLE_MAX_TAPS\b", h)) == 1
    src = open(os.path.join(ROOT, "nvit_amd", "csrc", "pos_resample.hip")).read()
    assert "NVIT_POS_RESAMPLE_MAX_TAPS" in src and not re.search(r"MAX_TAPS\s*=\s*\d", src)   # the number is written once
    assert "atomic" not in src.replace("no atomics", "")
