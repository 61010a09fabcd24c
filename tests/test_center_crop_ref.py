"""CPU: the numpy restatement tests/center_crop_ref.py against Pillow, bit for bit: the recorded fixture
tests/golden/center_crop_pil.npz (tools/make_golden_center_crop.py) and, where Pillow is installed, the live library
on random images - every pinned geometry, both filters, three channels and one, 256x256 -> 224 among them.  The Pillow
side is `Image.resize((W2, H2), f).crop((left, top, left + size, top + size))`."""
import numpy as np
import pytest

import center_crop_ref as R
from crop_ref import FILTERS


def test_pinned_geometries_and_the_two_roundings():
    for case, want in R.PINNED:
        assert R.geometry(*case) == want, case
    assert R.geometry(*R.STRONG_SHRINK) == (12, 8, 2, 0)
    assert R.geometry(37, 53, 24, 0.875, crop_mode="squash") == (27, 27, 2, 2)
    # the two half cases are what tell Python's round from floor(x + 1/2)
    assert R.geometry(53, 37, 24, 0.9, rounding=R.half_up) == (37, 26, 7, 1)
    assert R.geometry(37, 53, 24, 0.875, rounding=R.half_up) == (27, 38, 2, 7)


@pytest.mark.parametrize("interpolation", sorted(FILTERS))
def test_window_equals_the_pillow_fixture(interpolation):
    cases = R.golden_cases()
    assert len(cases) == 2 * (len(R.SMALL) + 1)
    assert {src.shape[2] for src, _, _ in cases} == {1, 3}
    geoms = {(src.shape[0], src.shape[1]) + g for src, g, _ in cases}
    for Hs, Ws, size, crop_pct in R.SMALL + [R.STRONG_SHRINK]:
        assert (Hs, Ws) + R.geometry(Hs, Ws, size, crop_pct) + (size,) in geoms
    for src, (H2, W2, top, left, size), want in cases:
        got = R.window(src[None], H2, W2, top, left, size, interpolation)[0]
        assert np.array_equal(got, want[interpolation]), (src.shape, H2, W2, top, left, size)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("interpolation", sorted(FILTERS))
def test_window_equals_live_pillow(interpolation, C):
    Image = pytest.importorskip("PIL.Image")
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[interpolation]
    g = np.random.default_rng(11 + C)
    for (Hs, Ws, size, crop_pct), _ in R.PINNED + [(R.STRONG_SHRINK, None)]:
        H2, W2, top, left = R.geometry(Hs, Ws, size, crop_pct)
        src = g.integers(0, 256, (Hs, Ws, C), dtype=np.uint8)
        im = Image.fromarray(src[:, :, 0] if C == 1 else src)
        want = np.asarray(im.resize((W2, H2), resample).crop((left, top, left + size, top + size))).reshape(size, size, C)
        got = R.window(src[None], H2, W2, top, left, size, interpolation)[0]
        assert np.array_equal(got, want), (Hs, Ws, size, crop_pct)


def test_rows_read_and_normalize():
    # the identity resize reads the window's rows and nothing else; a 256 -> 224 window at 16 never reads all 256
    assert R.rows_read(32, 32, 0, 32, "bilinear") == (0, 32)
    # (Pillow's support reaches one row past the last one that weighs in: row y reads y, y + 1, the second with weight 0)
    assert R.rows_read(256, 256, 16, 224, "bilinear") == (16, 225)
    assert R.rows_read(256, 256, 16, 224, "bicubic") == (15, 227)
    first, count = R.rows_read(300, 100, 18, 64, "bicubic")
    assert first > 0 and first + count < 300
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    x = R.normalize(u8, 0.5, 0.5)
    assert x.dtype == np.float32 and x.shape == (1, 1, 16, 16)
    # 0 -> exactly -1; 255 -> one ulp above 1: fp32's 1/255 is a little more than 1/255, and the fused subtraction keeps it
    assert x[0, 0, 0, 0] == -1.0 and x[0, 0, 15, 15] == np.float32(1.0) + np.float32(2.0 ** -23)
    wide = ((u8.astype(np.float64) / 255.0 - 0.45) / 0.225).transpose(0, 3, 1, 2)
    # four fp32 roundings, each at most 2^-24 relative: of 1/255 and of the fused multiply-subtract (values up to 1 and
    # 0.55, enlarged by 1/std < 4.5: 4.5 + 2.5 units of 2^-24), of 1/std and of the product (values up to 2.44 each): under
    # 12 units in all, and 8 * 2^-24 * max|value| is 19
    assert np.abs(R.normalize(u8, 0.45, 0.225).astype(np.float64) - wide).max() < 8 * 2.0 ** -24 * np.abs(wide).max()
