"""GPU: evaluation's Resize + CenterCrop (nvit_center_crop_apply, nvit_amd.crop.ResizeCenterCrop) against the numpy
restatement tests/center_crop_ref.py, bit for bit, and its fp32 output against `ops.normalize_images` of its own uint8
output, bit for bit.  tests/test_center_crop_ref.py holds the restatement to Pillow.

The shapes are the pinned geometries (sizes 20, 24, 32 and 64: a 16-wide tile with and without a ragged tail, one tile and
several; enlarging; the identity resize), a size of 36, a strong shrink whose tap sets are longer than a tile, the four
corner windows, where the taps are cut at the image's edge, and one 256x256 -> 224 batch.  Every batch holds distinct
images, so a wrong batch stride shows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import center_crop_ref as R

FILTERS = ("bilinear", "bicubic")
SIZE_36 = (50, 44, 36, 0.9)   # -> (45, 40, 4, 2), 4.5 -> 4
CASES = R.SMALL + [R.STRONG_SHRINK, SIZE_36]
B = 3


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def source(Hs, Ws, C, n=B):
    """The case's batch: (numpy, device tensor), made once and never modified."""
    u8 = np.random.default_rng(Hs * 1000 + Ws * 10 + C).integers(0, 256, (n, Hs, Ws, C), dtype=np.uint8)
    u8.setflags(write=False)
    return u8, torch.from_numpy(u8.copy()).to(dev())


@functools.lru_cache(maxsize=None)
def kernel_u8(case, interpolation, C):
    """The kernel's uint8 output of a case, computed once and shared by the tests."""
    from nvit_amd.crop import ResizeCenterCrop
    Hs, Ws, size, crop_pct = case
    return ResizeCenterCrop(size, crop_pct, interpolation)(source(Hs, Ws, C)[1], return_u8=True).cpu().numpy()


@functools.lru_cache(maxsize=None)
def twin_u8(case, interpolation, C, shift=0, rounding=round):
    Hs, Ws, size, crop_pct = case
    H2, W2, top, left = R.geometry(Hs, Ws, size, crop_pct, rounding=rounding)
    return R.window(source(Hs, Ws, C)[0], H2, W2, top, left + shift, size, interpolation)


def differing(got, want):
    return [k for k in range(len(want)) if not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("interpolation", FILTERS)
def test_uint8_output_equals_the_restatement(interpolation, C):
    assert {c[2] for c in CASES} >= {20, 24, 36} and SIZE_36 not in R.SMALL
    assert R.geometry(*SIZE_36) == (45, 40, 4, 2)
    for case in CASES:
        got, want = kernel_u8(case, interpolation, C), twin_u8(case, interpolation, C)
        assert got.shape == want.shape == (B, case[2], case[2], C) and got.dtype == np.uint8
        assert not differing(got, want), (case, interpolation, C, differing(got, want))
        assert differing(got[[1, 2, 0]], want) == [0, 1, 2], "the images of the batch are distinct"


@pytest.mark.parametrize("interpolation", FILTERS)
def test_a_corrupted_window_fails(interpolation):
    """The comparison above tells a window one column off, and a corner rounded half up, from the right one: the
    restatement under either change differs from the kernel's output on at least one of the chosen cases."""
    shifted = [c for c in CASES if R.geometry(*c)[3] + 1 <= R.geometry(*c)[1] - c[2]]
    assert len(shifted) >= 4
    assert any(differing(kernel_u8(c, interpolation, 3), twin_u8(c, interpolation, 3, shift=1)) for c in shifted)
    half = [c for c in CASES if R.geometry(*c, rounding=R.half_up) != R.geometry(*c)]
    assert (53, 37, 24, 0.9) in half and (37, 53, 24, 0.875) not in half
    assert any(differing(kernel_u8(c, interpolation, 3), twin_u8(c, interpolation, 3, rounding=R.half_up)) for c in half)


@pytest.mark.parametrize("mean,std", [(0.5, 0.5), (0.45, 0.225)])
def test_fp32_output_equals_normalize_images_of_the_uint8_output(mean, std):
    from nvit_amd import ops
    from nvit_amd.crop import ResizeCenterCrop
    for case in CASES:
        Hs, Ws, size, crop_pct = case
        for interpolation in FILTERS:
            for C in (3, 1):
                rcc = ResizeCenterCrop(size, crop_pct, interpolation, mean=mean, std=std)
                ud = source(Hs, Ws, C)[1]
                got = rcc(ud)
                u8 = torch.from_numpy(kernel_u8(case, interpolation, C)).to(dev())
                want = ops.normalize_images(u8, mean, std)
                assert got.dtype == torch.float32 and got.shape == want.shape == (B, C, size, size)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (case, interpolation, C)
                twin = R.normalize(kernel_u8(case, interpolation, C), mean, std)
                assert np.array_equal(got.cpu().numpy().view(np.int32), twin.view(np.int32)), (case, interpolation, C)


def test_both_outputs_from_one_call():
    from nvit_amd import ops
    from nvit_amd.crop import ResizeCenterCrop
    case = (37, 53, 24, 0.875)
    for C in (3, 1):
        rcc = ResizeCenterCrop(24, 0.875, "bicubic", mean=0.45, std=0.225)
        f32, u8 = rcc.apply(source(37, 53, C)[1], *rcc.geometry(37, 53), both=True)
        assert np.array_equal(u8.cpu().numpy(), twin_u8(case, "bicubic", C))
        assert torch.equal(f32.view(torch.int32), ops.normalize_images(u8, 0.45, 0.225).view(torch.int32))


@pytest.mark.parametrize("interpolation", FILTERS)
def test_corner_windows_through_apply(interpolation):
    """The windows at the four corners of the resized image, where Pillow cuts the taps at the edge: a shrink (37x53 ->
    27x38) and an enlargement (32x32 -> 36x36)."""
    from nvit_amd.crop import ResizeCenterCrop
    for (Hs, Ws, size), (H2, W2) in (((37, 53, 24), (27, 38)), ((32, 32, 32), (36, 36))):
        rcc = ResizeCenterCrop(size, interpolation=interpolation)
        for C in (3, 1):
            u8, ud = source(Hs, Ws, C)
            for top in (0, H2 - size):
                for left in (0, W2 - size):
                    got = rcc.apply(ud, H2, W2, top, left, return_u8=True).cpu().numpy()
                    want = R.window(u8, H2, W2, top, left, size, interpolation)
                    assert not differing(got, want), (Hs, Ws, size, top, left, C)


def test_256_to_224():
    from nvit_amd import ops
    from nvit_amd.crop import ResizeCenterCrop
    u8, ud = source(256, 256, 3, 2)
    rcc = ResizeCenterCrop(224, interpolation="bicubic")
    assert rcc.geometry(256, 256) == (256, 256, 16, 16)
    f32, got = rcc.apply(ud, 256, 256, 16, 16, both=True)
    assert not differing(got.cpu().numpy(), R.window(u8, 256, 256, 16, 16, 224, "bicubic"))
    assert torch.equal(f32.view(torch.int32), ops.normalize_images(got, 0.5, 0.5).view(torch.int32))
    got = ResizeCenterCrop(224)(ud, return_u8=True).cpu().numpy()
    assert not differing(got, R.window(u8, 256, 256, 16, 16, 224, "bilinear"))


def test_workspace_is_sized_by_the_rows_read_and_bad_windows_are_refused():
    from nvit_amd import _lib
    from nvit_amd.crop import INTERPOLATIONS
    lib = _lib.load()
    for interpolation in FILTERS:
        it = INTERPOLATIONS[interpolation]
        for Hs, Ws, size, crop_pct in CASES + [(256, 256, 224, 0.875), (2048, 512, 64, 1.0)]:
            H2, W2, top, left = R.geometry(Hs, Ws, size, crop_pct)
            for C in (3, 1):
                got = lib.nvit_center_crop_ws_bytes(B, Hs, Ws, C, H2, W2, top, left, size, it)
                assert got == R.workspace_bytes(B, Hs, Ws, C, H2, W2, top, left, size, interpolation), (Hs, Ws, size, C)
        # a window in the middle of a tall source: the intermediate holds a fraction of its rows
        first, count = R.rows_read(2048, 256, 96, 64, interpolation)
        assert 0 < first and count < 2048 // 3
        # nothing is clamped: a window that leaves the resized image, a size that is no multiple of 4, a fifth filter
        for H2, W2, top, left, size, f in ((27, 38, 4, 7, 24, it), (27, 38, 2, 15, 24, it), (27, 38, -1, 7, 24, it),
                                           (27, 38, 2, 7, 22, it), (23, 38, 0, 7, 24, it), (27, 4100, 2, 7, 24, it),
                                           (27, 38, 2, 7, 24, 2)):
            assert lib.nvit_center_crop_ws_bytes(B, 37, 53, 3, H2, W2, top, left, size, f) == -1
            buf = torch.zeros(4096, dtype=torch.uint8, device=dev())
            rc = lib.nvit_center_crop_apply(buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), 4096, 1, 37, 53, 3, H2, W2,
                                            top, left, size, f, 0.5, 0.5, None)
            assert rc == _lib.HEADER["EINVAL"] and not buf.any()
