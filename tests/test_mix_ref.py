"""CPU: the Beta quantile table of nvit_amd/mix.py against scipy (a committed fixture, and live where scipy is installed),
and the numpy restatement tests/mix_ref.py of the Mixup / CutMix draw against the distribution it claims."""
import os

import numpy as np
import pytest

import augment_ref
import mix_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_quantiles.npz")
ALPHAS = (0.1, 0.2, 0.8, 1.0, 4.0)
N_PAIRS = 100_000


def table(alpha):
    from nvit_amd.mix import beta_quantile_table
    return np.array(beta_quantile_table(alpha), dtype=np.float64)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_quantile_table_equals_the_scipy_fixture(alpha):
    g = np.load(GOLDEN)
    q = table(alpha)
    assert q.shape == (1025,)
    err = np.abs(q - g[f"q/{alpha}"]).max()
    print(f"alpha {alpha}: max |Q - scipy| = {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("alpha", ALPHAS)
def test_quantile_table_equals_scipy_live(alpha):
    special = pytest.importorskip("scipy.special")
    want = special.betaincinv(alpha, alpha, np.arange(1025) / 1024.0)
    assert np.abs(table(alpha) - want).max() <= 1e-9


@pytest.mark.parametrize("alpha", ALPHAS + (0.5, 2.0))
def test_quantile_table_is_monotone_with_exact_ends(alpha):
    q = table(alpha)
    assert q[0] == 0.0 and q[1024] == 1.0 and q[512] == 0.5
    assert (np.diff(q[:513]) > 0).all() and (np.diff(q) >= 0).all()   # 1 - 7e-28 is 1 also in fp64
    q32 = q.astype(np.float32)
    assert (np.diff(q32) >= 0).all() and q32[0] == 0.0 and q32[1024] == 1.0
    assert q32[1] >= np.finfo(np.float32).tiny   # the smallest interior knot is a normal fp32


def test_alpha_outside_the_range_is_refused():
    from nvit_amd.mix import beta_quantile_table
    for a in (0.05, 4.5, -1.0, float("nan")):
        with pytest.raises(ValueError):
            beta_quantile_table(a)


def test_vector_philox_is_the_scalar_one():
    g = np.random.default_rng(0)
    c = g.integers(0, 2 ** 32, (16, 4), dtype=np.uint64)
    for k0, k1 in ((0, 0), (0xDEADBEEF, 0x12345678)):
        got = np.stack(R.philox_vec(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k0, k1), axis=1)
        for i in range(16):
            assert got[i].tolist() == augment_ref.philox4x32_10(c[i].tolist(), (k0, k1))


@pytest.fixture(scope="module")
def pairs():
    """10^5 pairs with the defaults (mixup 0.8, cutmix 1.0, prob 1, switch 0.5) at 32x32."""
    q_mix, q_cut = table(0.8).astype(np.float32), table(1.0).astype(np.float32)
    return R.draw_pairs(0, 0, 0, N_PAIRS, 32, 32, q_mix, q_cut)


def test_cutmix_share_and_mean_lambda(pairs):
    mode, lam, box = pairs
    assert set(np.unique(mode)) == {R.MIXUP, R.CUTMIX}   # prob 1: every pair is mixed
    share = (mode == R.CUTMIX).mean()
    assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / N_PAIRS), share
    l = lam[mode == R.MIXUP].astype(np.float64)
    sigma = np.sqrt(1.0 / (4 * (2 * 0.8 + 1) * len(l)))   # Var Beta(a,a) = 1 / (4 (2a + 1))
    assert abs(l.mean() - 0.5) <= 5 * sigma, l.mean()
    assert l.min() >= 0.0 and l.max() <= 1.0


def test_boxes_are_inside_the_image_and_lambda_is_the_area(pairs):
    mode, lam, box = pairs
    H = W = 32
    b = box[mode == R.CUTMIX]
    y0, y1, x0, x1 = b.T
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
    assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    want = (1.0 - ((y1 - y0) * (x1 - x0)).astype(np.float64) / (H * W)).astype(np.float32)
    assert np.array_equal(lam[mode == R.CUTMIX], want)
    assert (box[mode != R.CUTMIX] == 0).all()
    # a rectangular image: x and y use their own side
    m, l, bx = R.draw_pairs(3, 1, 0, 2000, 24, 40, None, table(1.0).astype(np.float32))
    assert (m == R.CUTMIX).all() and (bx[:, 1] <= 24).all() and (bx[:, 3] <= 40).all() and (bx[:, 3] > 24).any()


def test_draw_is_a_pure_function_of_seed_index_and_step():
    q_mix, q_cut = table(0.8).astype(np.float32), table(1.0).astype(np.float32)
    whole = R.draw_pairs(7, 3, 0, 64, 32, 32, q_mix, q_cut, prob=0.5)
    again = R.draw_pairs(7, 3, 0, 64, 32, 32, q_mix, q_cut, prob=0.5)
    part = R.draw_pairs(7, 3, 40, 24, 32, 32, q_mix, q_cut, prob=0.5)
    far = R.draw_pairs(7, 3, 2 ** 33 + 5, 8, 32, 32, q_mix, q_cut, prob=0.5)
    for w, a, p in zip(whole, again, part):
        assert np.array_equal(w, a) and np.array_equal(w[40:], p)
    assert (whole[0] == R.NONE).any() and (whole[0] != R.NONE).any()   # prob 0.5 gates some pairs off
    assert (whole[1][whole[0] == R.NONE] == 1.0).all()
    for other in (R.draw_pairs(8, 3, 0, 64, 32, 32, q_mix, q_cut, prob=0.5),
                  R.draw_pairs(7, 4, 0, 64, 32, 32, q_mix, q_cut, prob=0.5)):
        assert not np.array_equal(other[1], whole[1])
    assert not np.array_equal(far[1], whole[1][:8])
    # the domain constant: the words are not AutoAugment's for the same seed and counter
    r = R.words(7, 3, 0, 4)
    aa = augment_ref.philox4x32_10((0, 0, 3, 0), (7, 0))
    assert [int(w[0]) for w in r] != aa
    # one alpha off: that mode never appears, the other always (prob 1)
    assert (R.draw_pairs(1, 0, 0, 500, 32, 32, q_mix, None)[0] == R.MIXUP).all()
    assert (R.draw_pairs(1, 0, 0, 500, 32, 32, None, q_cut)[0] == R.CUTMIX).all()
    assert (R.draw_pairs(1, 0, 0, 500, 32, 32, None, None)[0] == R.NONE).all()


def test_rows_of_the_table_and_the_apply():
    q_mix, q_cut = table(0.8).astype(np.float32), table(1.0).astype(np.float32)
    y = np.arange(7) * 3
    tab, lam, y2 = R.draw(5, 2, 0, y, 8, 8, q_mix, q_cut)
    assert tab.shape == (7, 8) and tab[3].tolist() == [0, np.float32(1).view(np.int32), 0, 0, 0, 0, 3, 0]
    assert tab[:, 6].tolist() == [6, 5, 4, 3, 2, 1, 0] and y2.tolist() == y[::-1].tolist()
    for p in range(3):
        assert np.array_equal(tab[p, :6], tab[6 - p, :6]) and lam[p] == lam[6 - p]
    g = np.random.default_rng(1)
    X = g.standard_normal((7, 2, 8, 8)).astype(np.float32)
    out = R.apply(X, tab)
    assert np.array_equal(out[3], X[3])
    for b in range(7):
        if tab[b, 0] == R.CUTMIX:
            y0, y1, x0, x1 = tab[b, 2:6]
            mask = np.zeros((8, 8), bool)
            mask[y0:y1, x0:x1] = True
            assert np.array_equal(out[b][:, mask], X[6 - b][:, mask]) and np.array_equal(out[b][:, ~mask], X[b][:, ~mask])
    t = R.soft_target(y % 5, y2 % 5, lam, 0.1, 5)
    assert np.allclose(t.sum(1), 1.0)
