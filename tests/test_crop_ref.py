"""CPU: the numpy restatement tests/crop_ref.py (which the GPU tests hold the kernels to, bit for bit) against Pillow -
the committed fixture tests/golden/crop_pil.npz (tools/make_golden_crop.py) and the installed Pillow - and the
properties of both draws and of the product's two host tables."""
import math
import os

import numpy as np
import pytest

import crop_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crop_pil.npz")
FILTERS = ("bilinear", "bicubic")


golden_cases = R.golden_cases


def table_of(boxes, flip=0):
    return np.array([[*box, flip, 0, 0, 0] for box in boxes], dtype=np.int32)


def aspect(lo, hi):
    from nvit_amd.crop import aspect_table
    return aspect_table(lo, hi)


RATIO = (3 / 4, 4 / 3)


# ------------------------------------------------------------------------------------------------ the resampler
def test_the_fixture_holds_the_shapes_the_feature_is_specified_on():
    shapes = {(*src.shape, size) for src, size, _, _ in golden_cases()}
    assert {(24, 40, 3, 16), (24, 40, 1, 16), (9, 7, 3, 16), (16, 16, 3, 16), (5, 33, 3, 8), (1, 1, 3, 8), (64, 64, 3, 8),
            (256, 256, 3, 224)} <= shapes
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.mark.parametrize("interpolation", FILTERS)
def test_restatement_equals_the_pillow_fixture(interpolation):
    for src, size, boxes, want in golden_cases():
        batch = np.repeat(src[None], len(boxes), axis=0)
        got = R.crop_apply(batch, table_of(boxes), size, interpolation)
        assert np.array_equal(got, want[interpolation]), (src.shape, size, interpolation)
        flipped = R.crop_apply(batch, table_of(boxes, 1), size, interpolation)
        assert np.array_equal(flipped, want[interpolation][:, :, ::-1, :]), (src.shape, size, interpolation, "flip")
        if src.shape[:2] == (16, 16) and size == 16:
            assert np.array_equal(got[0], src), "16x16 -> 16 is the identity"


@pytest.mark.parametrize("interpolation", FILTERS)
def test_restatement_equals_the_installed_pillow_on_random_images(interpolation):
    Image = pytest.importorskip("PIL.Image")
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[interpolation]
    g = np.random.default_rng(5)
    for src, size, boxes, _ in golden_cases():
        Hs, Ws, C = src.shape
        img = g.integers(0, 256, (Hs, Ws, C), dtype=np.uint8)
        got = R.crop_apply(np.repeat(img[None], len(boxes), axis=0), table_of(boxes), size, interpolation)
        for k, (top, left, h, w) in enumerate(boxes.tolist()):
            im = Image.fromarray(img[:, :, 0] if C == 1 else img)
            want = np.asarray(im.crop((left, top, left + w, top + h)).resize((size, size), resample)).reshape(size, size, C)
            assert np.array_equal(got[k], want), (src.shape, size, (top, left, h, w), interpolation)


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("corner", [(0, 0), (10, 10), (20, 20), (0, 20)])
def test_nothing_outside_the_box_leaks_in(interpolation, corner):
    """Zeros inside a 12x12 box, 255 everywhere else: the taps clamp at the crop's edges, so the crop is all zeros."""
    img = np.full((1, 32, 32, 3), 255, np.uint8)
    top, left = corner
    img[0, top:top + 12, left:left + 12] = 0
    for size in (8, 16, 24):
        for flip in (0, 1):
            assert not R.crop_apply(img, table_of([(top, left, 12, 12)], flip), size, interpolation).any()


def test_a_box_that_leaves_the_image_is_the_whole_image():
    img = np.random.default_rng(1).integers(0, 256, (1, 9, 12, 3), dtype=np.uint8)
    whole = R.crop_apply(img, table_of([(0, 0, 9, 12)]), 8, "bilinear")
    for box in ((0, 0, 10, 12), (-1, 0, 4, 4), (6, 0, 4, 4), (0, 9, 4, 4), (0, 0, 0, 5), (0, 0, 5, 0), (2 ** 31 - 1, 0, 2, 2)):
        assert np.array_equal(R.crop_apply(img, table_of([box]), 8, "bilinear"), whole), box


# ------------------------------------------------------------------------------------------------ the crop draw
def test_every_box_lies_inside_the_image_and_the_shapes_vary():
    for Hs, Ws in ((32, 32), (24, 40), (256, 256)):
        seen = set()
        for step in range(4):
            t = R.crop_draw(3, step, 0, 64, Hs, Ws, (0.08, 1.0), RATIO, aspect(*RATIO), 0.5)
            top, left, h, w, flip = (t[:, i].astype(np.int64) for i in range(5))
            assert (h >= 1).all() and (w >= 1).all() and (top >= 0).all() and (left >= 0).all()
            assert (top + h <= Hs).all() and (left + w <= Ws).all()
            assert set(flip.tolist()) == {0, 1} and not t[:, 5:].any()
            assert (h * w >= 0.07 * Hs * Ws).all()
            asp = w / h
            assert (asp > 0.74 * (1 - 1.5 / np.minimum(h, w))).all() and (asp < 1.34 * (1 + 1.5 / np.minimum(h, w))).all()
            seen.update(zip(top.tolist(), left.tolist(), h.tolist(), w.tolist()))
        assert len(seen) > 200


def test_failed_attempts_fall_back_to_the_central_crop():
    # scale 1 at ratio 2 on a square image: w = sqrt(2) * side never fits
    t = R.crop_draw(1, 0, 0, 16, 32, 32, (1.0, 1.0), (2.0, 2.0), aspect(2.0, 2.0), 0.0)
    assert (t[:, :5] == [8, 0, 16, 32, 0]).all()      # in_ratio 1 < 2: w = Ws, h = round(Ws / 2), centred
    t = R.crop_draw(1, 0, 0, 16, 40, 10, (1.0, 1.0), (2.0, 2.0), aspect(2.0, 2.0), 0.0)
    assert (t[:, :5] == [17, 0, 5, 10, 0]).all()      # 10 wide, 40 high: in_ratio 1/4 < 2
    t = R.crop_draw(1, 0, 0, 16, 10, 40, (1.0, 1.0), (2.0, 2.0), aspect(2.0, 2.0), 0.0)
    assert (t[:, :5] == [0, 10, 10, 20, 0]).all()     # 40 wide, 10 high: in_ratio 4 > 2: h = Hs, w = round(Hs * 2)
    t = R.crop_draw(1, 0, 0, 16, 32, 32, (4.0, 4.0), (1.0, 1.0), aspect(1.0, 1.0), 0.0)
    assert (t[:, :5] == [0, 0, 32, 32, 0]).all()      # a ratio that fits, an area that does not: the whole image


def test_hflip_zero_and_one_and_the_split_invariance():
    args = (32, 32, (0.08, 1.0), RATIO, aspect(*RATIO))
    assert not R.crop_draw(9, 2, 0, 64, *args, 0.0)[:, 4].any()
    assert R.crop_draw(9, 2, 0, 64, *args, 1.0)[:, 4].all()
    whole = R.crop_draw(9, 2, 0, 8, *args, 0.5)
    halves = np.concatenate([R.crop_draw(9, 2, 0, 4, *args, 0.5), R.crop_draw(9, 2, 4, 4, *args, 0.5)])
    assert np.array_equal(whole, halves)
    assert not np.array_equal(whole, R.crop_draw(9, 3, 0, 8, *args, 0.5))
    assert not np.array_equal(whole, R.crop_draw(10, 2, 0, 8, *args, 0.5))


def test_the_aspect_table_and_its_documented_deviation():
    from nvit_amd.crop import KNOTS, aspect_table, aspect_table_deviation
    for lo, hi in (RATIO, (0.3, 1 / 0.3)):
        t = aspect_table(lo, hi)
        assert len(t) == KNOTS + 1 == R.KNOTS + 1
        assert abs(t[0] / lo - 1) < 1e-15 and abs(t[-1] / hi - 1) < 1e-14 and abs(t[KNOTS // 2] - 1) < 1e-14
        # the interpolated value against the exponential, over every 16th 24-bit uniform of a few segments
        dev = aspect_table_deviation(lo, hi)
        worst = 0.0
        for k in (0, 511, 1023):
            u = (np.arange(0, 1 << 14, 16, dtype=np.uint64) + np.uint64(k << 14)) << np.uint64(8)
            got = R.aspect_of(u, t)
            true = np.exp(math.log(lo) + (u >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 * (math.log(hi) - math.log(lo)))
            rel = got / true - 1
            assert (rel > -1e-14).all()
            worst = max(worst, rel.max())
        assert 0.99 * dev < worst <= dev * (1 + 1e-6), (lo, hi, dev, worst)
    assert 3.9e-8 < aspect_table_deviation(*RATIO) < 4.0e-8
    assert 6.8e-7 < aspect_table_deviation(0.3, 1 / 0.3) < 7.0e-7


# ------------------------------------------------------------------------------------------------ the erasing
ERASE_ASPECT = (0.3, 1 / 0.3)


def test_erasing_probability_zero_and_one_and_the_strict_bound():
    tab = aspect(*ERASE_ASPECT)
    assert not R.erase_draw(4, 0, 0, 64, 16, 16, 0.0, (0.02, 1 / 3), tab)[:, :5].any()
    ons = 0
    for H, W in ((16, 16), (8, 12), (224, 224)):
        for step in range(4):
            t = R.erase_draw(4, step, 0, 64, H, W, 1.0, (0.02, 1 / 3), tab).astype(np.int64)
            on, top, left, h, w = (t[:, i] for i in range(5))
            ons += on.sum()
            assert (h[on == 1] < H).all() and (w[on == 1] < W).all()          # timm's strict <
            assert (top >= 0).all() and (left >= 0).all() and (top + h <= H).all() and (left + w <= W).all()
            assert not t[on == 0, 1:5].any()
    assert ons >= 0.9 * 12 * 64                                               # nearly every image finds a box
    # an area that never fits: ten failed attempts, nothing erased (no fallback)
    assert not R.erase_draw(4, 0, 0, 64, 16, 16, 1.0, (1.0, 1.0), aspect(1.0, 1.0))[:, :5].any()
    # the gate is a probability; sub-keys differ per image and per step
    t = R.erase_draw(4, 0, 0, 256, 32, 32, 0.25, (0.02, 1 / 3), tab)
    assert 0.15 * 256 < t[:, 0].sum() < 0.35 * 256
    assert len({(a, b) for a, b in t[:, 5:7].tolist()}) == 256
    assert not np.array_equal(t[:, 5:7], R.erase_draw(4, 1, 0, 256, 32, 32, 0.25, (0.02, 1 / 3), tab)[:, 5:7])
    whole = R.erase_draw(4, 1, 0, 8, 32, 32, 0.5, (0.02, 1 / 3), tab)
    halves = [R.erase_draw(4, 1, f, 4, 32, 32, 0.5, (0.02, 1 / 3), tab) for f in (0, 4)]
    assert np.array_equal(whole, np.concatenate(halves))


def test_the_normal_quantile_table():
    """The conditions on the noise table, computed exactly from the knots: symmetric, finite, variance within 1 % of 1,
    kurtosis within 0.1 of 3."""
    import statistics
    from nvit_amd.crop import ERASE_KNOTS, NOISE_TAIL, normal_quantile_table
    q = np.array(normal_quantile_table(), dtype=np.float64)
    q32 = q.astype(np.float32)
    assert len(q) == ERASE_KNOTS + 1 == 1025 and np.isfinite(q32).all()
    assert np.array_equal(q32, -q32[::-1]) and q32[512] == 0 and (np.diff(q32) > 0).all()
    nd = statistics.NormalDist()
    assert q[0] == nd.inv_cdf(NOISE_TAIL) and NOISE_TAIL == 2.0 ** -15
    assert abs(q[256] - nd.inv_cdf(0.25)) < 1e-15 and abs(q[1] - nd.inv_cdf(1 / 1024)) < 1e-15
    mean, var, kurt = R.table_moments(q32)
    print(f"noise table: end knot {q32[0]!r}, mean {mean:.3e}, variance {var:.6f}, kurtosis {kurt:.6f}")
    assert abs(mean) < 1e-12 and abs(var - 1) < 0.01 and abs(kurt - 3) < 0.1
    # the generator itself: the sample moments of one image's noise are those of the table
    z = R.noise(123, 456, 1 << 18, q32).astype(np.float64)
    assert abs(z.mean()) < 0.01 and abs(z.var() - var) < 0.02 and abs((z ** 4).mean() / z.var() ** 2 - kurt) < 0.1
    assert not np.array_equal(z[:1024], R.noise(124, 456, 1024, q32))


def test_erase_apply_restatement():
    from nvit_amd.crop import normal_quantile_table
    q = np.array(normal_quantile_table()).astype(np.float32)
    x = np.random.default_rng(2).standard_normal((3, 3, 16, 16)).astype(np.float32)
    table = np.array([[1, 2, 3, 5, 7, 11, 12, 0], [0, 2, 3, 5, 7, 11, 12, 0], [1, 0, 0, 16, 16, 13, 14, 0]], np.int32)
    const = R.erase_apply(x, table, "const")
    assert not const[0, :, 2:7, 3:10].any() and not const[2].any() and np.array_equal(const[1], x[1])
    keep = np.ones((16, 16), bool)
    keep[2:7, 3:10] = False
    assert np.array_equal(const[0][:, keep], x[0][:, keep])
    pix = R.erase_apply(x, table, "pixel", q)
    assert np.array_equal(pix[0][:, keep], x[0][:, keep]) and np.array_equal(pix[1], x[1])
    assert np.array_equal(pix[2].reshape(-1), R.noise(13, 14, 3 * 256, q))
    assert not np.array_equal(pix[0, 0, 2:7, 3:10], pix[0, 1, 2:7, 3:10])   # per element, not per pixel
