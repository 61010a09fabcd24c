"""CPU: the public face of nvit_amd.crop.ResizeCenterCrop, evaluation's Resize + CenterCrop.  The geometry is host
arithmetic and is pinned here, wrong arguments are refused with ValueError / TypeError before any device work, `.batch()`
reports the model input's shape, the train step refuses the batch object, and the entry points are declared."""
import inspect
import os

import pytest
import torch

import center_crop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_signature_and_declared_symbols():
    import nvit_amd
    from nvit_amd import _lib, crop
    for name in ("ResizeCenterCrop", "CenterCroppedBatch"):
        assert getattr(nvit_amd, name) is getattr(crop, name)
    sig = inspect.signature(crop.ResizeCenterCrop.__init__)
    assert list(sig.parameters)[1:] == ["size", "crop_pct", "interpolation", "crop_mode", "mean", "std"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0.875, "bilinear", "center", 0.5, 0.5]
    rcc = crop.ResizeCenterCrop(32)
    assert not hasattr(rcc, "to") and not hasattr(rcc, "state_dict")   # stateless
    header = open(os.path.join(ROOT, "include", "nvit_hip.h")).read()
    source = open(os.path.join(ROOT, "nvit_amd", "csrc", "crop.hip")).read()
    for name, nargs in (("nvit_center_crop_ws_bytes", 10), ("nvit_center_crop_apply", 18)):
        assert len(_lib.SIGNATURES[name]) == nargs
        assert f" {name}(" in header and f'extern "C" ' in source and f" {name}(" in source
    assert _lib._RESTYPES["nvit_center_crop_ws_bytes"] is _lib.C.c_int64
    assert "nvit_normalize_images" in _lib.SIGNATURES   # whose arithmetic the fp32 output restates


def test_geometry_is_pinned():
    from nvit_amd.crop import ResizeCenterCrop
    for (Hs, Ws, size, crop_pct), want in R.PINNED:
        rcc = ResizeCenterCrop(size, crop_pct)
        assert rcc.geometry(Hs, Ws) == want == R.geometry(Hs, Ws, size, crop_pct), (Hs, Ws, size, crop_pct)
        assert all(type(v) is int for v in rcc.geometry(Hs, Ws))
    # Python's round, half to even: 1.5 -> 2 and 6.5 -> 6 (floor(x + 1/2) gives 7 for the second)
    assert ResizeCenterCrop(24, 0.875).geometry(37, 53)[2] == 2
    assert ResizeCenterCrop(24, 0.9).geometry(53, 37)[2] == 6
    assert R.geometry(53, 37, 24, 0.9, rounding=R.half_up)[2] == 7
    assert ResizeCenterCrop(8, 1.0).geometry(300, 200) == (12, 8, 2, 0)


def test_squash_resizes_both_sides():
    from nvit_amd.crop import ResizeCenterCrop
    assert ResizeCenterCrop(24, 0.875, crop_mode="squash").geometry(37, 53) == (27, 27, 2, 2)
    assert ResizeCenterCrop(224, crop_mode="squash").geometry(300, 500) == (256, 256, 16, 16)
    assert ResizeCenterCrop(224).geometry(300, 500) == (256, 426, 16, 101)
    assert ResizeCenterCrop(64, 0.95, crop_mode="squash").geometry(300, 200) == R.geometry(300, 200, 64, 0.95, "squash")


def test_refuses_wrong_arguments():
    from nvit_amd.crop import MAX_SIDE, CenterCroppedBatch, ResizeCenterCrop
    for size in (30, 0, -4, 2, MAX_SIDE + 4):
        with pytest.raises(ValueError, match="size"):
            ResizeCenterCrop(size)
    for size in (32.0, True, "32"):
        with pytest.raises(TypeError, match="size"):
            ResizeCenterCrop(size)
    for crop_pct in (0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="crop_pct"):
            ResizeCenterCrop(32, crop_pct)
    with pytest.raises(TypeError, match="crop_pct"):
        ResizeCenterCrop(32, "0.875")
    with pytest.raises(ValueError, match="interpolation"):
        ResizeCenterCrop(32, interpolation="nearest")
    with pytest.raises(TypeError, match="interpolation"):
        ResizeCenterCrop(32, interpolation=2)
    with pytest.raises(ValueError, match="crop_mode"):
        ResizeCenterCrop(32, crop_mode="border")
    with pytest.raises(TypeError, match="crop_mode"):
        ResizeCenterCrop(32, crop_mode=None)
    for std in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="std"):
            ResizeCenterCrop(32, std=std)
    with pytest.raises(TypeError, match="std"):
        ResizeCenterCrop(32, std="1")
    with pytest.raises(ValueError, match="mean"):
        ResizeCenterCrop(32, mean=float("nan"))
    rcc = ResizeCenterCrop(16, interpolation="bicubic")
    u8 = torch.zeros(2, 24, 40, 3, dtype=torch.uint8)
    for take in (rcc.batch, rcc, lambda x: rcc.apply(x, 18, 30, 1, 7)):
        for bad in (u8.float(), u8.to(torch.int32), [1, 2]):
            with pytest.raises(TypeError, match="uint8"):
                take(bad)
        for bad in (u8[0], torch.zeros(2, 24, 40, 2, dtype=torch.uint8), torch.zeros(2, 24, 40, 4, dtype=torch.uint8),
                    torch.zeros(0, 24, 40, 3, dtype=torch.uint8), torch.zeros(1, 4096, 8, 3, dtype=torch.uint8),
                    torch.zeros(1, 8, 8, 3, dtype=torch.uint8).expand(65536, 8, 8, 3)):
            with pytest.raises(ValueError):
                take(bad)
    # a source whose resized longer side passes the cap: 2048 x 8 -> scale 18 on the short side, 4608 on the long one
    long = torch.zeros(1, 2048, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=str(MAX_SIDE)):
        rcc.geometry(2048, 8)
    with pytest.raises(ValueError, match=str(MAX_SIDE)):
        rcc.batch(long)
    assert ResizeCenterCrop(16, crop_mode="squash").batch(long).shape == (1, 3, 16, 16)
    # the raw window: host integers inside the resized image, refused before any device work
    for H2, W2, top, left in ((15, 30, 0, 0), (18, MAX_SIDE + 1, 0, 0), (18, 30, 3, 0), (18, 30, 0, 15), (18, 30, -1, 0)):
        with pytest.raises(ValueError):
            rcc.apply(u8, H2, W2, top, left)
    with pytest.raises(TypeError, match="top"):
        rcc.apply(u8, 18, 30, 1.0, 7)
    with pytest.raises(RuntimeError):
        rcc(u8)   # no CPU path
    assert isinstance(rcc.batch(u8), CenterCroppedBatch)


def test_batch_reports_the_model_input_shape():
    from nvit_amd.crop import ResizeCenterCrop
    for C in (1, 3):
        u8 = torch.zeros(5, 72, 80, C, dtype=torch.uint8)
        rcc = ResizeCenterCrop(56, interpolation="bicubic", mean=0.45, std=0.225)
        b = rcc.batch(u8)
        assert tuple(b.shape) == (5, C, 56, 56) and b.shape[0] == 5 and b.device == u8.device
        assert b.crop is rcc and b.u8 is u8
    assert rcc.params() == (56, 0.875, "bicubic", "center", 0.45, 0.225)
    assert rcc.params() != ResizeCenterCrop(56, interpolation="bicubic", mean=0.45, std=0.25).params()


def test_train_steps_refuse_the_batch_object():
    from nvit_amd.crop import ResizeCenterCrop
    from nvit_amd.train import GraphedTrainStep, train_step
    xb = ResizeCenterCrop(32).batch(torch.zeros(4, 40, 40, 3, dtype=torch.uint8))
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(TypeError, match="CenterCroppedBatch"):
        train_step(None, None, xb, y)
    with pytest.raises(TypeError, match="CenterCroppedBatch"):
        GraphedTrainStep(None, None, xb, y)
