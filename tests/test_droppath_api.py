"""CPU: the public face of stochastic depth (nvit_amd.DropPath, ViT.attach_drop_path, the checkpoint key) and the numpy
restatement of its draw (droppath_ref.py) that the GPU tests hold the kernel to bit for bit.  No device work."""
import numpy as np
import pytest
import torch

import droppath_ref as dr
import rowops_check as rc


def test_constructor_validation():
    from nvit_amd import DropPath
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            DropPath(bad)
    for bad in ("0.1", None, True):
        with pytest.raises(TypeError):
            DropPath(bad)
    with pytest.raises(ValueError):
        DropPath(0.1, seed=-1)
    with pytest.raises(ValueError):
        DropPath(0.1, seed=2 ** 64)
    with pytest.raises(TypeError):
        DropPath(0.1, seed=1.5)
    with pytest.raises(ValueError):
        DropPath(0.1, first_index=-1)
    with pytest.raises(ValueError):
        DropPath(0.1, first_index=2 ** 62)
    with pytest.raises(TypeError):
        DropPath(0.1, scale_by_keep=1)
    dp = DropPath(0.0)
    assert dp.rate == 0.0 and dp.scale_by_keep is None and dp.step == 0
    assert DropPath(0.25, seed=2 ** 64 - 1, first_index=2 ** 62 - 1, scale_by_keep=True).scale_by_keep is True
    with pytest.raises(RuntimeError):
        DropPath(0.1).draw(2, 4)          # no device yet
    with pytest.raises(RuntimeError):
        DropPath(0.1).to("cpu")


def test_rates_are_timms_linspace():
    from nvit_amd import DropPath
    for rate in (0.0, 0.1, 0.5):
        dp = DropPath(rate)
        r = dp.rates(12)
        assert r.dtype == np.float32 and np.array_equal(r, np.linspace(0, rate, 12).astype(np.float32))
        assert np.array_equal(dp.rates(1), np.zeros(1, dtype=np.float32))
        assert np.array_equal(r, dr.rates(rate, 12))
        assert r[0] == 0.0 and r[-1] == np.float32(rate)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            DropPath(0.1).rates(bad)


def test_state_dict_round_trip(tmp_path):
    from nvit_amd import DropPath
    dp = DropPath(0.2, seed=2 ** 40 + 7)
    dp.load_state_dict({"seed": 2 ** 63 + 5, "step": 123456789012})
    assert dp.state_dict() == {"seed": 2 ** 63 + 5, "step": 123456789012}
    torch.save(dp.state_dict(), tmp_path / "dp.pt")
    other = DropPath(0.2)
    other.load_state_dict(torch.load(tmp_path / "dp.pt", weights_only=True))
    assert other.state_dict() == dp.state_dict() and other.step == 123456789012
    with pytest.raises(ValueError):
        other.load_state_dict({"seed": 1, "step": -1})


def test_restatement_statistics():
    """rate 0.5, 2 layers (p = 0, 0.5), 2^16 samples: the last block's kept fraction lies within 4 standard deviations of
    keep, its two branches differ in at least a quarter of the samples (independent draws differ in half), the first block
    never drops, and the values are exactly {0, 1/keep} or {0, 1}."""
    n = 1 << 16
    keep = 0.5
    for seed, step, first in ((0, 0, 0), (2 ** 63 + 11, 2 ** 33 + 5, 2 ** 40)):
        t = dr.draw(seed, step, first, 0.5, 2, n, True)
        assert t.shape == (4, n) and t.dtype == np.float32
        assert (t[:2] == 1.0).all()
        assert set(np.unique(t[2:])) == {np.float32(0.0), np.float32(2.0)}
        for row in (2, 3):
            f = (t[row] != 0).mean()
            assert abs(f - keep) <= 4 * np.sqrt(keep * (1 - keep) / n), (row, f)
        assert ((t[2] != 0) != (t[3] != 0)).mean() >= 0.25
        u = dr.draw(seed, step, first, 0.5, 2, n, False)
        assert np.array_equal(u != 0, t != 0) and set(np.unique(u)) == {np.float32(0.0), np.float32(1.0)}
        assert not np.array_equal(dr.draw(seed, step + 1, first, 0.5, 2, n, True), t)       # another step,
        assert not np.array_equal(dr.draw(seed + 1, step, first, 0.5, 2, n, True), t)       # another seed
    # a sample's gate depends on its global index only: a batch drawn in two halves is the batch
    whole = dr.draw(3, 9, 100, 0.5, 3, 8, True)
    halves = np.concatenate([dr.draw(3, 9, 100, 0.5, 3, 4, True), dr.draw(3, 9, 104, 0.5, 3, 4, True)], axis=1)
    assert np.array_equal(whole, halves)


def test_gated_formula_restates_the_plain_one_and_the_autograd_reference():
    """droppath_ref's gated LERP formula: with every gate 1 it is rowops_check's, value and bound; with mixed gates its
    fp64 values are those of autograd through the gated forward, and a gate table shifted by one sample is not."""
    M, C, T = 12, 260, 3
    for skip, add, accum in ((True, False, False), (False, True, True)):
        d = rc.row_case(M, C, 40, skip=skip, add=add, accum=accum)
        ones = torch.ones(M // T)
        v1, b1 = dr.gated_lerp_bounds(d, ones, T)
        v0, b0 = rc.lerp_bounds(d)
        for k in v0:
            assert torch.equal(v1[k], v0[k]) and (b1[k] >= b0[k]).all() and (b1[k] <= 1.5 * b0[k] + 1e-300).all(), k
        gate = torch.tensor([0.0, 1.0, 1.0 / 0.9, 0.0], dtype=torch.float32)
        vals, bnd = dr.gated_lerp_bounds(d, gate, T)
        ref = dr.gated_lerp_eval(d, gate, T)
        rc.close_values(vals, bnd, ref, f"gated lerp skip={skip}")
        f32 = dr.gated_lerp_formula(d, gate, T, torch.float32)
        got = {k: f32[k] for k in bnd}
        assert all(dr.within(got, ref, bnd).values())
        shifted = dr.gated_lerp_formula(d, torch.roll(gate, 1), T, torch.float32)
        ok = dr.within({k: shifted[k] for k in bnd}, ref, bnd)
        assert not ok["out"] and not ok["dh"] and not ok["dy"] and not ok["dalpha"], ok
        zero = dr.gated_lerp_eval(d, torch.zeros(M // T), T)
        assert torch.equal(zero["dy"], torch.zeros_like(zero["dy"]))
        assert torch.equal(zero["dalpha"], torch.zeros_like(zero["dalpha"]))


def test_gated_residual_formulas_restate_the_plain_ones_and_autograd():
    """the same for the plain-ViT residual kernels (z = a + gate * y, h + gate * y) and the gated copy of vit_torch_ref"""
    import vit_torch_ref
    from nvit_amd import named_config
    from nvit_amd.weights import formula_state_dict, synthetic_batch
    M, C, T = 12, 260, 3
    gate = torch.tensor([0.0, 1.0, 1.0 / 0.9, 0.0], dtype=torch.float32)
    cases = [(rc.row_case(M, C, 41, add=True, accum=acc, g_add_dtype=torch.float32), dr.gated_res_rmsnorm_formula,
              dr.gated_res_rmsnorm_eval, dr.gated_res_rmsnorm_bounds, rc.res_rmsnorm_bounds) for acc in (False, True)]
    cases.append((rc.row_case(M, C, 42), dr.gated_res_skip_formula, dr.gated_res_skip_eval, dr.gated_res_skip_bounds,
                  rc.res_skip_bounds))
    for d, formula, evalf, boundf, plain in cases:
        v1, _ = boundf(d, torch.ones(M // T), T)
        v0, _ = plain(d)
        assert all(torch.equal(v1[k], v0[k]) for k in v0)
        vals, bnd = boundf(d, gate, T)
        ref = evalf(d, gate, T)
        rc.close_values(vals, bnd, ref, "gated residual")
        f32 = formula(d, gate, T, torch.float32)
        assert all(dr.within({k: f32[k] for k in bnd}, ref, bnd).values())
        shifted = formula(d, torch.roll(gate, 1), T, torch.float32)
        ok = dr.within({k: shifted[k] for k in bnd}, ref, bnd)
        assert not ok["out"] and not ok["dy"], ok
    cfg = named_config("mini_vit")
    X, y = synthetic_batch(cfg, 4)
    sd = formula_state_dict(cfg)
    l0, _, _, g0 = vit_torch_ref.loss_and_grads(sd, cfg, X, y)
    l1, _, g1 = dr.gated_vit_loss_and_grads(sd, cfg, X, y, torch.ones(2 * cfg.n_layer, 4))
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_checkpoint_key_set():
    from nvit_amd import DropPath, ViT, named_config
    from nvit_amd.checkpoint import build_checkpoint
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    base = build_checkpoint(m, opt, 3, {"loss": 1.0})
    assert "drop_path" not in base
    dp = DropPath(0.1, seed=5)
    dp.load_state_dict({"seed": 5, "step": 42})
    ck = build_checkpoint(m, opt, 3, {"loss": 1.0}, drop_path=dp)
    assert set(ck) == set(base) | {"drop_path"} and ck["drop_path"] == {"seed": 5, "step": 42}


def test_attach_drop_path():
    from nvit_amd import DropPath, ViT, named_config
    m = ViT(named_config("micro"))
    assert m.drop_path is None
    dp = DropPath(0.1)
    assert m.attach_drop_path(dp) is m and m.drop_path is dp
    assert dp.scale_by_keep is False                      # None resolves to False for nViT
    keep = DropPath(0.1, scale_by_keep=True)
    m.attach_drop_path(keep)
    assert keep.scale_by_keep is True                     # an explicit choice stays
    assert "drop_path" not in "".join(m.state_dict().keys())
    m.attach_drop_path(None)
    assert m.drop_path is None
    with pytest.raises(TypeError):
        m.attach_drop_path(0.1)
    # the plain ViT takes timm's default: kept branches are scaled by 1 / keep
    plain = DropPath(0.1)
    ViT(named_config("micro_vit")).attach_drop_path(plain)
    assert plain.scale_by_keep is True
    from dataclasses import fields
    from nvit_amd import ViTConfig
    assert len(fields(ViTConfig)) == 26 and not any("drop_path" in f.name for f in fields(ViTConfig))
