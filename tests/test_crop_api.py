"""CPU: the public face of nvit_amd.crop.  Wrong arguments are refused with ValueError / TypeError before any device
work, the chain wrappers only nest in the order crop -> AutoAugment -> erasing -> Mixup, the entry points are bound, and
the Python constants are the header's."""
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_signatures_and_bindings():
    import nvit_amd
    from nvit_amd import _lib, crop
    from nvit_amd.augment import DeviceStepCounter
    for name in ("RandomResizedCrop", "CroppedBatch", "RandomErasing", "ErasedBatch"):
        assert getattr(nvit_amd, name) is getattr(crop, name)
    assert issubclass(crop.RandomResizedCrop, DeviceStepCounter) and issubclass(crop.RandomErasing, DeviceStepCounter)
    sig = inspect.signature(crop.RandomResizedCrop.__init__)
    assert list(sig.parameters)[1:] == ["size", "scale", "ratio", "interpolation", "hflip", "seed", "first_index"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [(0.08, 1.0), (3 / 4, 4 / 3), "bilinear", 0.5, 0, 0]
    sig = inspect.signature(crop.RandomErasing.__init__)
    assert list(sig.parameters)[1:] == ["prob", "area", "aspect", "mode", "seed", "first_index"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [0.25, (0.02, 1 / 3), (0.3, 1 / 0.3), "pixel", 0, 0]
    for name in ("nvit_crop_draw", "nvit_crop_apply", "nvit_crop_ws_bytes", "nvit_erase_draw", "nvit_erase_apply"):
        assert name in _lib.SIGNATURES
    r = crop.RandomResizedCrop(32, seed=5, first_index=7)
    assert r.state_dict() == {"seed": 5, "step": 0} and r.first_index == 7
    r.load_state_dict({"seed": 6, "step": 9})
    assert r.state_dict() == {"seed": 6, "step": 9}
    with pytest.raises(RuntimeError):
        r.draw(4, 32, 32)                      # no CPU path: .to(device) first
    with pytest.raises(RuntimeError):
        crop.RandomErasing().to("cpu")


def test_python_constants_equal_their_header_macros():
    from nvit_amd import crop
    macros = {}
    for ln in open(os.path.join(ROOT, "include", "nvit_hip.h")):
        parts = ln.split()
        if len(parts) >= 3 and parts[0] == "#define" and parts[1].startswith(("NVIT_CROP_", "NVIT_ERASE_")):
            macros[parts[1][len("NVIT_"):]] = int(parts[2], 10)
    assert set(macros) == {"CROP_ROW", "CROP_KNOTS", "CROP_ATTEMPTS", "CROP_MAX_SRC", "CROP_MAX_BATCH", "CROP_BILINEAR", "CROP_BICUBIC",
                           "ERASE_ROW", "ERASE_KNOTS", "ERASE_CONST", "ERASE_PIXEL"}
    assert (crop.ROW, crop.KNOTS, crop.ATTEMPTS, crop.MAX_SRC) == tuple(macros["CROP_" + k] for k in ("ROW", "KNOTS", "ATTEMPTS", "MAX_SRC"))
    assert crop.MAX_BATCH == macros["CROP_MAX_BATCH"]
    assert crop.INTERPOLATIONS == {"bilinear": macros["CROP_BILINEAR"], "bicubic": macros["CROP_BICUBIC"]}
    assert (crop.ERASE_ROW, crop.ERASE_KNOTS) == (macros["ERASE_ROW"], macros["ERASE_KNOTS"])
    assert crop.ERASE_MODES == {"const": macros["ERASE_CONST"], "pixel": macros["ERASE_PIXEL"]}
    import crop_ref
    assert (crop_ref.KNOTS, crop_ref.ATTEMPTS) == (crop.KNOTS, crop.ATTEMPTS)


def test_the_new_source_file_is_built_into_the_library():
    """crop.hip is listed in the Makefile, holds the entry points and compiles under contract(off), next to the one
    copy of the Philox function."""
    import re
    csrc = os.path.join(ROOT, "nvit_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "crop.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    src = open(os.path.join(csrc, "crop.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "philox.h"' in src
    copies = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h")) and "0xD2511F53" in open(os.path.join(csrc, f)).read()]
    assert copies == ["philox.h"]


def test_random_resized_crop_refuses_wrong_arguments():
    from nvit_amd.crop import RandomResizedCrop
    for size in (30, 0, -4, 2, 4100):
        with pytest.raises(ValueError):
            RandomResizedCrop(size)
    with pytest.raises(TypeError):
        RandomResizedCrop(32.0)
    for kw in ({"scale": (1.0, 0.08)}, {"scale": (0.0, 1.0)}, {"scale": (-0.1, 1.0)}, {"ratio": (4 / 3, 3 / 4)},
               {"ratio": (0.0, 1.0)}, {"ratio": (1.0, float("inf"))}, {"scale": (float("nan"), 1.0)},
               {"interpolation": "nearest"}, {"hflip": 1.5}, {"hflip": -0.1}, {"seed": -1}, {"first_index": -1}):
        with pytest.raises(ValueError):
            RandomResizedCrop(32, **kw)
    for kw in ({"scale": 0.5}, {"scale": ("a", 1.0)}, {"ratio": None}, {"interpolation": 2}, {"hflip": "x"}, {"seed": 1.0}):
        with pytest.raises(TypeError):
            RandomResizedCrop(32, **kw)
    r = RandomResizedCrop(16, interpolation="bicubic")
    u8 = torch.zeros(2, 24, 40, 3, dtype=torch.uint8)
    for bad in (u8.float(), u8.to(torch.int32), [1, 2]):
        with pytest.raises(TypeError):
            r.batch(bad)
    for bad in (u8[0], torch.zeros(2, 24, 40, 2, dtype=torch.uint8), torch.zeros(2, 24, 40, 4, dtype=torch.uint8),
                torch.zeros(0, 24, 40, 3, dtype=torch.uint8), torch.zeros(1, 4096, 8, 3, dtype=torch.uint8),
                torch.zeros(1, 8, 8, 3, dtype=torch.uint8).expand(65536, 8, 8, 3)):   # more images than a grid's second dimension
        with pytest.raises(ValueError):
            r.batch(bad)
    b = r.batch(u8)
    assert tuple(b.shape) == (2, 16, 16, 3) and b.device == u8.device and b.crop is r
    assert tuple(r.batch(torch.zeros(5, 8, 9, 1, dtype=torch.uint8)).shape) == (5, 16, 16, 1)
    t = r.params_for([(0, 0, 24, 40), (1, 2, 3, 4)], [0, 1])
    assert t.dtype == torch.int32 and t.tolist() == [[0, 0, 24, 40, 0, 0, 0, 0], [1, 2, 3, 4, 1, 0, 0, 0]]
    for bad in ([], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            r.params_for(bad)
    with pytest.raises(ValueError):
        r.params_for([(0, 0, 1, 1)], [0, 1])
    with pytest.raises(ValueError):
        r.apply(u8, torch.zeros(3, 8, dtype=torch.int32))     # one row per image
    with pytest.raises(ValueError):
        r.apply(u8, torch.zeros(2, 8, dtype=torch.int64))


def test_random_erasing_refuses_wrong_arguments():
    from nvit_amd.crop import RandomErasing
    for kw in ({"prob": 1.5}, {"prob": -0.1}, {"prob": float("nan")}, {"area": (0.5, 0.02)}, {"area": (0.0, 0.3)},
               {"area": (0.02, 1.5)}, {"aspect": (3.0, 0.3)}, {"aspect": (0.0, 1.0)}, {"mode": "rand"}, {"seed": 2 ** 64}):
        with pytest.raises(ValueError):
            RandomErasing(**kw)
    for kw in ({"prob": "x"}, {"area": 0.1}, {"aspect": (None, 1.0)}, {"mode": 1}, {"first_index": 0.0}):
        with pytest.raises(TypeError):
            RandomErasing(**kw)
    e = RandomErasing(mode="const")
    x = torch.zeros(2, 3, 16, 16)
    for bad in (x.double(), x.to(torch.uint8), None):
        with pytest.raises(TypeError):
            e.batch(bad)
    for bad in (x[0], torch.zeros(2, 3, 16, 18), torch.zeros(0, 3, 16, 16), torch.zeros(1, 3, 8, 8).expand(65536, 3, 8, 8)):
        with pytest.raises(ValueError):
            e.batch(bad)
    with pytest.raises(ValueError):
        e.batch(x, std=0.0)
    assert tuple(e.batch(x).shape) == (2, 3, 16, 16)
    t = e.params_for([(1, 2, 3, 4), None], keys=[2 ** 63 + 5, 7])
    assert t.tolist() == [[1, 1, 2, 3, 4, 5, -2 ** 31, 0], [0, 0, 0, 0, 0, 7, 0, 0]]
    with pytest.raises(ValueError):
        e.params_for([])
    with pytest.raises(ValueError):
        e.apply(x, torch.zeros(2, 7, dtype=torch.int32))


def test_chains_nest_in_one_order_only():
    from nvit_amd.augment import AutoAugment
    from nvit_amd.crop import RandomErasing, RandomResizedCrop
    from nvit_amd.mix import Mixup
    from nvit_amd.train import _unwrap_input, _wrap_input
    rrc, aug, erase, mix = RandomResizedCrop(32), AutoAugment("cifar10"), RandomErasing(), Mixup()
    u8 = torch.zeros(4, 40, 40, 3, dtype=torch.uint8)
    f32 = torch.zeros(4, 3, 32, 32)
    full = mix.batch(erase.batch(aug.batch(rrc.batch(u8))))
    assert tuple(full.shape) == (4, 3, 32, 32) and full.B == 4
    stages, inner = _unwrap_input(full)
    assert inner is u8 and stages == {"mix": mix, "erase": (erase, 0.5, 0.5), "augment": aug, "crop": rrc}
    again, inner2 = _unwrap_input(_wrap_input(stages, u8))
    assert again == stages and inner2 is u8
    # every sub-chain in the right order
    for X in (aug.batch(rrc.batch(u8)), erase.batch(rrc.batch(u8), mean=0.4, std=0.2), erase.batch(aug.batch(u8[:, :32, :32])),
              erase.batch(f32), mix.batch(erase.batch(f32)), mix.batch(erase.batch(rrc.batch(u8))),
              mix.batch(aug.batch(rrc.batch(u8))), mix.batch(f32)):
        stages, inner = _unwrap_input(X)
        assert inner is u8 or inner is f32 or inner.shape == (4, 32, 32, 3)
        assert _unwrap_input(_wrap_input(stages, inner))[0] == stages
    assert _unwrap_input(f32) == ({}, f32)
    # the wrong order, and a crop with nothing behind it that makes fp32 of it
    for bad in (lambda: rrc.batch(aug.batch(u8)), lambda: rrc.batch(erase.batch(f32)), lambda: aug.batch(erase.batch(f32)),
                lambda: aug.batch(mix.batch(f32)), lambda: erase.batch(mix.batch(f32)), lambda: erase.batch(erase.batch(f32)),
                lambda: mix.batch(rrc.batch(u8)), lambda: mix.batch(mix.batch(f32)), lambda: _unwrap_input(rrc.batch(u8))):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(ValueError):
        aug.batch(RandomResizedCrop(32).batch(torch.zeros(4, 40, 40, 2, dtype=torch.uint8)))
