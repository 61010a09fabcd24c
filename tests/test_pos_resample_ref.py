"""CPU: the host tap tables of the position-embedding resampling (nvit_amd/resample.py) against torch's own fp64
F.interpolate(mode="bicubic", antialias=True, align_corners=False): the per-axis weight matrix, its separability, the
transposed table the backward reads, and the packed layout the kernels read."""
import numpy as np
import pytest
import torch

import pos_resample_ref as ref
from nvit_amd import resample as R


@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_tap_table_is_torchs_weight_matrix(g, g2):
    rows = R.tap_rows(g, g2)
    W = R.dense(rows, g)
    want = ref.torch_matrix(g, g2)
    assert W.shape == want.shape == (g2, g)
    err = np.abs(W - want).max()
    print(f"[{g}->{g2}] max |W - torch| {err:.2e}, taps per row {R.max_taps(rows)}")
    assert err <= 1e-14
    assert np.abs(W.sum(axis=1) - 1.0).max() <= 1e-14
    for lo, w in zip(*rows):   # rows are clipped to the table
        assert 0 <= lo and lo + len(w) <= g and len(w) >= 1


def test_tap_counts_are_the_filters():
    """4 taps enlarging; the antialiasing filter widens with the ratio when shrinking: 6 at 7 -> 4, 8 at 14 -> 7"""
    assert R.max_taps(R.tap_rows(28, 36)) == 4 and R.max_taps(R.tap_rows(7, 10)) == 4
    assert R.max_taps(R.tap_rows(7, 4)) == 6 and R.max_taps(R.tap_rows(14, 7)) == 8


def test_it_is_not_the_plain_bicubic_filter():
    """even enlarging, torch's antialias=False filter (a = -0.75) is another matrix"""
    W = R.dense(R.tap_rows(7, 10), 7)
    assert np.abs(W - ref.torch_matrix(7, 10, antialias=False)).max() > 1e-2


@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_the_operator_is_separable(g, g2):
    """(W (x) W) p is torch's 2-D result in fp64"""
    W = R.dense(R.tap_rows(g, g2), g)
    p = torch.randn(g * g, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(g * 100 + g2))
    got = ref.apply_matrices(W, W, p.numpy(), g)
    want = ref.target(p, g, g2).numpy()
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_transposed_table_is_the_transpose(g, g2):
    fwd, bwd = R.host_tables(g, g2)
    assert np.array_equal(R.dense(bwd, g2), R.dense(fwd, g).T)   # exactly: the same fp64 values, moved
    assert len(bwd[0]) == g
    for lo, w in zip(*bwd):
        assert 0 <= lo and lo + len(w) <= g2 and len(w) >= 1


@pytest.mark.parametrize("g,g2", [(7, 4), (28, 36), (1, 3)])
def test_packed_layout(g, g2):
    fwd, bwd = R.host_tables(g, g2)
    for rows, n in ((fwd, g2), (bwd, g)):
        t = R.pack(rows)
        assert t.dtype == np.int32 and t.shape == (n, 2 + R.MAX_TAPS) and R.ROW == 2 + R.MAX_TAPS
        for o, (lo, w) in enumerate(zip(*rows)):
            assert t[o, 0] == lo and t[o, 1] == len(w)
            assert np.array_equal(t[o, 2:2 + len(w)].view(np.float32), np.asarray(w).astype(np.float32))
            assert not t[o, 2 + len(w):].any()


def test_a_ratio_over_the_tap_cap_is_refused():
    with pytest.raises(ValueError, match="taps"):
        R.host_tables(64, 7)    # shrinking: the forward rows
    with pytest.raises(ValueError, match="taps"):
        R.host_tables(4, 40)    # enlarging: the transposed rows
    R.host_tables(4, 28)        # 7x still fits
    for bad in ((0, 4), (4, 0), (4.0, 7), (True, 7)):
        with pytest.raises(ValueError):
            R.tap_rows(*bad)
    with pytest.raises(ValueError):
        R.grid_of(48)
    assert R.grid_of(49) == 7
