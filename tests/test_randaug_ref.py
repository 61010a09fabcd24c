"""CPU: the numpy restatement of RandAugment (tests/randaug_ref.py) against Pillow - live calls and the committed fixture
tests/golden/randaug_pil.npz (tools/make_golden_randaug.py), bit for bit - its level maps against timm's table, the
distribution of its draw against 5-sigma bounds derived here, and the cos / sin table against its documented deviation.
None of it needs a GPU."""
import importlib.util
import math
import os

import numpy as np
import pytest

import randaug_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "randaug_pil.npz")
FILL = (124, 116, 104)


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_randaug",
                                                  os.path.join(os.path.dirname(HERE), "tools", "make_golden_randaug.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def twin_op(img, name, value, filt):
    H, W, _ = img.shape
    return R.apply_row(img, R.op_row(name, value, filt, H, W), FILL)


# key -> (op, raw argument, filter) without Pillow: the cases of tools/make_golden_randaug.py, restated
def fixture_cases(H, W):
    names = {R.BILINEAR: "bilinear", R.BICUBIC: "bicubic"}
    for name in R.GEOMETRIC:
        for filt in (R.BILINEAR, R.BICUBIC):
            for m in (0, 4.5, 9, 10):
                for neg in ((0,) if m == 0 else (0, 1)):
                    yield f"{name}/{names[filt]}/m{m}/{neg}", name, R.level_arg(name, m, neg, True, H, W), filt
    for filt in (R.BILINEAR, R.BICUBIC):
        for tag, name, value in (("far0", "Rotate", 77.7), ("far1", "Rotate", -98.6), ("far", "TranslateX", 0.9 * W + 0.3),
                                 ("far", "TranslateY", -(0.8 * H + 0.6))):
            yield f"{name}/{names[filt]}/{tag}", name, value, filt
    for add in (0, 99, 128):
        yield f"SolarizeAdd/{add}", "SolarizeAdd", add, R.BILINEAR
    for bits in (0, 4):
        yield f"Posterize/{bits}", "Posterize", bits, R.BILINEAR
    for th in (0, 256):
        yield f"Solarize/{th}", "Solarize", th, R.BILINEAR


@pytest.mark.parametrize("tag", ["rand_32x32", "rand_24x40", "rand_24x40x1"])
def test_restatement_equals_the_pillow_fixture_bit_for_bit(golden, tag):
    img = golden["in/" + tag]
    n = 0
    for key, name, value, filt in fixture_cases(img.shape[0], img.shape[1]):
        want = golden[f"out/{tag}/{key}"]
        got = twin_op(img, name, value, filt)
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert np.array_equal(got, want), (tag, key, int((got != want).sum()))
        n += 1
    assert n == 5 * 2 * 7 + 2 * 4 + 3 + 2 + 2
    assert sum(k.startswith(f"out/{tag}/") for k in golden.files) == n


def test_fixture_covers_the_edges_it_is_there_for(golden):
    assert sorted(k[3:] for k in golden.files if k.startswith("in/")) == ["rand_24x40", "rand_24x40x1", "rand_32x32"]
    img = golden["in/rand_24x40"]
    fill = np.array(FILL, dtype=np.uint8)
    for key in ("Rotate/bicubic/far0", "Rotate/bilinear/far1", "TranslateX/bicubic/far", "TranslateY/bilinear/far"):
        out = golden["out/rand_24x40/" + key]
        filled = (out == fill).all(axis=2).mean()
        assert (filled > 0.5) if "Translate" in key else (filled > 0.25), (key, filled)   # most of / much of the image is fill
        assert filled < 1.0
    assert (golden["out/rand_24x40x1/TranslateX/bilinear/far"] == FILL[0]).mean() > 0.5
    assert not golden["out/rand_24x40/Posterize/0"].any()
    assert np.array_equal(golden["out/rand_24x40/Solarize/256"], img) and np.array_equal(golden["out/rand_24x40/Solarize/0"], 255 - img)
    assert np.array_equal(golden["out/rand_24x40/SolarizeAdd/0"], img)
    low = img < 128
    assert np.array_equal(golden["out/rand_24x40/SolarizeAdd/128"][low], img[low] + 128)
    # m = 0: the geometric ops are the identity under both filters
    for name in R.GEOMETRIC:
        for f in ("bilinear", "bicubic"):
            assert np.array_equal(golden[f"out/rand_24x40/{name}/{f}/m0/0"], img), (name, f)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "augment_pil.npz"))


@pytest.mark.parametrize("shape", [(32, 32, 3), (24, 40, 3), (24, 40, 1), (224, 224, 3)], ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_live_pillow(shape):
    pytest.importorskip("PIL")
    G = _tool()
    H, W, C = shape
    img = np.random.default_rng(H + W + C).integers(0, 256, shape, dtype=np.uint8)
    ms = (4.5, 10) if H == 224 else (0, 4.5, 9, 10)
    n = 0
    for name in R.GEOMETRIC:
        for filt in (R.BILINEAR, R.BICUBIC):
            for m in ms:
                for neg in (0, 1):
                    v = R.level_arg(name, m, neg, True, H, W)
                    assert np.array_equal(twin_op(img, name, v, filt), G.pil_op(img, name, v, filt, FILL)), (name, filt, m, neg)
                    n += 1
            for v in ((77.7, -98.6, 0.4) if name == "Rotate" else (0.9 * W + 0.3, -(0.8 * H + 0.6)) if "Translate" in name else ()):
                assert np.array_equal(twin_op(img, name, v, filt), G.pil_op(img, name, v, filt, FILL)), (name, filt, v)
                n += 1
    assert n == 5 * 2 * len(ms) * 2 + 2 * (3 + 2 + 2)
    if H == 224:
        return
    for name, values in (("SolarizeAdd", (0, 99, 128)), ("Posterize", (0, 4)), ("Solarize", (0, 256))):
        for v in values:
            assert np.array_equal(twin_op(img, name, v, R.BILINEAR), G.pil_op(img, name, v)), (name, v)


def test_the_fill_is_per_channel():
    img = np.random.default_rng(1).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    out = twin_op(img, "TranslateX", 39.0, R.BICUBIC)   # output column 0 samples input column 39, the rest lies outside
    assert (out[:, 1:] == np.array(FILL, dtype=np.uint8)).all() and not (out[:, 0] == np.array(FILL, dtype=np.uint8)).all()
    off = R.apply_params(img[None], np.zeros((1, 3, R.ROW), dtype=np.int32), FILL)
    assert np.array_equal(off[0], img)


# ------------------------------------------------------------------------------------------------ level maps
def expected_levels(m, translate_pct, H, W):
    """timm's table, written out: op -> (increasing +, increasing -, plain +, plain -)."""
    L = m / 10
    enh_inc = (max(0.1, 1 + 0.9 * L), max(0.1, 1 - 0.9 * L))
    t = min(256, int(256 * L))
    return {
        "Rotate": (30 * L, -30 * L) * 2, "ShearX": (0.3 * L, -0.3 * L) * 2, "ShearY": (0.3 * L, -0.3 * L) * 2,
        "TranslateX": (translate_pct * L * W, -translate_pct * L * W) * 2,
        "TranslateY": (translate_pct * L * H, -translate_pct * L * H) * 2,
        **{op: enh_inc + (1.8 * L + 0.1,) * 2 for op in R.ENHANCE},
        "Posterize": (4 - int(4 * L),) * 2 + (int(4 * L),) * 2,
        "Solarize": (256 - t,) * 2 + (t,) * 2,
        "SolarizeAdd": (min(128, int(110 * L)),) * 4,
        "AutoContrast": (0,) * 4, "Equalize": (0,) * 4, "Invert": (0,) * 4,
    }


def check_level_maps(level_arg):
    H, W = 24, 40
    for m in (0, 9, 9.99, 10):
        want = expected_levels(m, 0.45, H, W)
        assert set(want) == set(R.CHOICES)
        for op, (ip, im, pp, pm) in want.items():
            got = (level_arg(op, m, 0, True, H, W, 0.45), level_arg(op, m, 1, True, H, W, 0.45),
                   level_arg(op, m, 0, False, H, W, 0.45), level_arg(op, m, 1, False, H, W, 0.45))
            for g, w in zip(got, (ip, im, pp, pm)):
                if isinstance(w, int):
                    assert isinstance(g, int) and g == w, (op, m, got)
                else:
                    assert abs(g - w) <= 4 * np.spacing(abs(w)), (op, m, got)   # the same products in another order
    # the integers at the points where truncation decides
    assert [level_arg("Posterize", m, 0, True, H, W) for m in (0, 2.49, 2.5, 9, 9.99, 10)] == [4, 4, 3, 1, 1, 0]
    assert [level_arg("Posterize", m, 0, False, H, W) for m in (0, 9, 9.99, 10)] == [0, 3, 3, 4]
    assert [level_arg("Solarize", m, 0, True, H, W) for m in (0, 9, 9.99, 10)] == [256, 26, 1, 0]
    assert [level_arg("Solarize", m, 0, False, H, W) for m in (0, 9, 9.99, 10)] == [0, 230, 255, 256]
    assert [level_arg("SolarizeAdd", m, 0, True, H, W) for m in (0, 9, 9.99, 10)] == [0, 99, 109, 110]
    assert level_arg("Color", 10, 1, True, H, W) == 0.1 and level_arg("Color", 9.99, 1, True, H, W) > 0.1
    assert level_arg("TranslateX", 10, 0, True, H, W) == 0.45 * 40 and level_arg("TranslateY", 10, 1, True, H, W) == -0.45 * 24
    assert level_arg("TranslateX", 9, 0, True, H, W) != round(level_arg("TranslateX", 9, 0, True, H, W))   # not rounded


def test_level_maps_of_the_restatement():
    check_level_maps(R.level_arg)


def test_level_maps_of_the_host_side():
    from nvit_amd import randaug as P
    check_level_maps(P.level_arg)
    assert P.CHOICES == R.CHOICES and P.OPS == R.OPS and P.ROW == R.ROW
    for m in (0, 4.5, 9, 9.99, 10):
        for op in R.CHOICES:
            for neg in (0, 1):
                for inc in (True, False):
                    assert P.level_arg(op, m, neg, inc, 24, 40, 0.3) == R.level_arg(op, m, neg, inc, 24, 40, 0.3)


def test_host_rows_equal_the_restatement():
    from nvit_amd.randaug import RandAugment
    ra = RandAugment()
    H, W = 24, 40
    entries, want = [], []
    for op in R.CHOICES:
        for m, neg, f in ((0, 0, "bilinear"), (9, 1, "bicubic"), (9.99, 0, "bicubic")):
            entries.append([(op, m, neg, f)])
            v = R.level_arg(op, m, neg, True, H, W)
            want.append(R.op_row(op, v, R.FILTERS[f], H, W))
    got = ra.params_for(entries, H, W).numpy()
    assert got.shape == (len(entries), 1, R.ROW)
    assert np.array_equal(got[:, 0], np.stack(want))
    raw = ra.params_for([[("Rotate", {"value": -98.6}, "bicubic"), None, ("SolarizeAdd", {"value": 99}), "Invert"]], H, W).numpy()
    assert np.array_equal(raw[0, 0], R.op_row("Rotate", -98.6, R.BICUBIC, H, W)) and not raw[0, 1].any()
    assert np.array_equal(raw[0, 2], R.op_row("SolarizeAdd", 99)) and np.array_equal(raw[0, 3], R.op_row("Invert"))


# ------------------------------------------------------------------------------------------------ the draw
SEED = 2024


def test_distribution_of_the_draw():
    """B = 4096 over 4 steps, two layers: n = 32768 (image, layer) draws under the defaults (m 9, mstd 0.5, prob 0.5,
    "random").  A count of n Bernoulli(p) trials has standard deviation sqrt(n p (1 - p)); the mean of n N(9, 0.5^2)
    magnitudes has 0.5 / sqrt(n), and their sample standard deviation about 0.5 / sqrt(2 n).  The interpolated quantile
    table moves neither by more than 1e-4 (its tails end at the 2^-15 quantile).  Every bound is 5 sigma."""
    det = []
    for step in range(4):
        R.draw(SEED, step, 0, 4096, 32, 32, details=det)
    n = len(det)
    assert n == 4096 * 4 * 2
    choice = np.array([d[0] for d in det])
    on = np.array([d[1] for d in det])
    raw = np.array([d[2] for d in det])
    neg = np.array([d[3] for d in det])
    fbit = np.array([d[4] for d in det])

    def binomial_ok(count, p, what):
        sigma = math.sqrt(n * p * (1 - p))
        assert abs(count - n * p) <= 5 * sigma, (what, count, n * p, sigma)
    for k in range(15):
        binomial_ok(int((choice == k).sum()), 1 / 15, f"op {R.CHOICES[k]}")
    binomial_ok(int(on.sum()), 0.5, "on")
    binomial_ok(int(neg.sum()), 0.5, "sign")
    binomial_ok(int(fbit.sum()), 0.5, "filter")
    assert abs(raw.mean() - 9.0) <= 5 * 0.5 / math.sqrt(n) + 1e-4, raw.mean()
    assert abs(raw.std() - 0.5) <= 5 * 0.5 / math.sqrt(2 * n) + 1e-4, raw.std()
    assert raw.max() > 10.0   # the clamp has work to do
    # independence of what one word does not decide: on-rate and sign rate within the ops' own counts
    for k in (3, 6, 14):
        sel = choice == k
        s = math.sqrt(sel.sum() * 0.25)
        assert abs(on[sel].sum() - sel.sum() * 0.5) <= 5 * s and abs(neg[sel].sum() - sel.sum() * 0.5) <= 5 * s


def test_draw_modes_and_the_table_it_writes():
    H, W = 24, 40
    t = R.draw(SEED, 1, 0, 64, H, W, num_layers=4)
    assert t.shape == (64, 4, R.ROW) and t.dtype == np.int32
    ids = t[:, :, 0]
    assert set(np.unique(ids)) <= {0} | {R.ID[c] for c in R.CHOICES}
    assert 0.3 < (ids == 0).mean() < 0.7
    geo = np.isin(ids, [R.ID[c] for c in R.GEOMETRIC])
    assert set(np.unique(t[geo][:, 1])) == {0, 1} and not t[~geo][:, 1].any() and not t[:, :, 14:].any()
    assert not t[ids == 0].any()
    # a function of the global index, the step and the seed
    assert np.array_equal(R.draw(SEED, 1, 40, 24, H, W, num_layers=4), t[40:])
    assert not np.array_equal(R.draw(SEED, 2, 0, 64, H, W, num_layers=4), t)
    assert not np.array_equal(R.draw(SEED + 1, 1, 0, 64, H, W, num_layers=4), t)
    # the layers draw from different keys
    assert not np.array_equal(t[:, 0], t[:, 1])
    # prob 0 and 1; fixed filters; mstd 0 and inf
    assert not R.draw(SEED, 0, 0, 32, H, W, prob=0.0).any()
    assert (R.draw(SEED, 0, 0, 32, H, W, prob=1.0)[:, :, 0] != 0).all()
    for name, code in (("bilinear", 0), ("bicubic", 1)):
        f = R.draw(SEED, 0, 0, 64, H, W, prob=1.0, interpolation=name)
        g = np.isin(f[:, :, 0], [R.ID[c] for c in R.GEOMETRIC])
        assert g.any() and (f[g][:, 1] == code).all()
    det0, deti = [], []
    R.draw(SEED, 0, 0, 256, H, W, mstd=0.0, details=det0)
    R.draw(SEED, 0, 0, 256, H, W, mstd=math.inf, magnitude=7.0, details=deti)
    assert all(d[2] == 9.0 for d in det0)
    u = np.array([d[2] for d in deti])
    assert (u >= 0).all() and (u < 7.0).all() and abs(u.mean() - 3.5) < 5 * 7.0 / math.sqrt(12 * len(u))
    # mstd 0 at m 9, increasing: the table's arguments are the level maps'
    z = R.draw(SEED, 0, 0, 256, H, W, mstd=0.0, prob=1.0)
    for row in z.reshape(-1, R.ROW):
        name = R.OPS[row[0]]
        if name == "Posterize":
            assert row[2] == 1
        if name == "Solarize":
            assert row[2] == 26
        if name == "SolarizeAdd":
            assert row[2] == 99
        if name == "ShearX":
            assert abs(abs(row[2:14].copy().view(np.float64)[1]) - 0.27) < 1e-15


def test_rotation_table_and_its_documented_deviation():
    from nvit_amd.randaug import ROT_KNOTS, rot_table, rot_table_deviation
    for mmax in (10.0, 5.0):
        t = np.array(rot_table(mmax)).reshape(2, ROT_KNOTS + 1)
        assert ROT_KNOTS == R.KNOTS and np.array_equal(t, R.rot_table(mmax))
        assert t[0, 0] == 1.0 and t[1, 0] == 0.0
        assert abs(t[0, -1] - math.cos(math.radians(3 * mmax))) < 1e-15 and abs(t[1, -1] - math.sin(math.radians(3 * mmax))) < 1e-15
        bound = rot_table_deviation(mmax)
        worst = 0.0
        for lv in np.linspace(0.0, mmax / 10.0, 20001):
            for neg in (0, 1):
                c, s = R.drawn_rotate_coef(float(lv), neg, 24, 40, t, mmax)[:2]
                a = math.radians(30.0 * lv)
                worst = max(worst, abs(c - math.cos(a)), abs(s - (math.sin(a) if neg else -math.sin(a))))
        assert 0.5 * bound < worst <= bound * (1 + 1e-6) + 1e-15, (mmax, bound, worst)
    assert 3.2e-8 < rot_table_deviation(10.0) < 3.4e-8
    # the drawn matrix against Pillow's exact one at the same angle: the documented deviation, scaled by the half-diagonal
    t = R.rot_table(10.0)
    for lv, neg in ((0.9, 0), (0.4567, 1), (1.0, 0)):
        got = np.array(R.drawn_rotate_coef(lv, neg, 24, 40, t, 10.0))
        want = np.array(R.affine_coef("Rotate", -30.0 * lv if neg else 30.0 * lv, 24, 40))
        assert np.abs(got - want).max() <= rot_table_deviation(10.0) * (1 + 20 + 12) + 1e-14
