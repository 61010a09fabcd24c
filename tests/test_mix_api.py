"""CPU: the public face of nvit_amd.mix.  Wrong arguments are refused with ValueError / TypeError before any device
work, so the refusals can be checked on CPU tensors; the state round trip works before `.to(device)`."""
import pytest
import torch


def X0(B=8, C=3, H=32, W=32, dtype=torch.float32):
    return torch.zeros(B, C, H, W, dtype=dtype)


def y0(B=8):
    return torch.zeros(B, dtype=torch.int64)


def test_exports():
    import nvit_amd
    from nvit_amd import mix
    assert nvit_amd.Mixup is mix.Mixup and nvit_amd.MixedBatch is mix.MixedBatch
    assert nvit_amd.MixedTargets is mix.MixedTargets
    m = nvit_amd.Mixup()
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.label_smoothing, m.seed, m.first_index) == \
        (0.8, 1.0, 1.0, 0.5, 0.1, 0, 0)


@pytest.mark.parametrize("kw", [dict(mixup_alpha=0.05), dict(mixup_alpha=4.5), dict(cutmix_alpha=-1.0), dict(cutmix_alpha=9),
                                dict(mixup_alpha=float("nan")), dict(prob=-0.1), dict(prob=1.5), dict(switch_prob=2.0),
                                dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(seed=-1), dict(seed=2 ** 64),
                                dict(first_index=-1), dict(first_index=2 ** 62)])
def test_constructor_refuses_values_out_of_range(kw):
    from nvit_amd.mix import Mixup
    with pytest.raises(ValueError):
        Mixup(**kw)


@pytest.mark.parametrize("kw", [dict(mixup_alpha="0.8"), dict(prob=None), dict(seed=1.0), dict(first_index=True),
                                dict(label_smoothing="x")])
def test_constructor_refuses_wrong_types(kw):
    from nvit_amd.mix import Mixup
    with pytest.raises(TypeError):
        Mixup(**kw)


def test_alpha_zero_and_the_range_ends_are_accepted():
    from nvit_amd.mix import Mixup
    for a, b in ((0, 0), (0.1, 4.0), (4, 0.1), (0, 1.0), (0.8, 0)):
        m = Mixup(a, b)
        assert m.mixes_images == (a > 0 or b > 0)


def test_batch_refuses_wrong_images_and_labels_before_device_work():
    from nvit_amd.mix import Mixup
    m = Mixup()
    for bad in (X0(dtype=torch.float64), X0().to(torch.uint8), [[1.0]], None):
        with pytest.raises(TypeError):
            m.batch(bad)
    for bad in (torch.zeros(8, 3, 32), torch.zeros(8, 3, 32, 30), torch.zeros(0, 3, 32, 32), torch.zeros(8, 3, 32, 32, 1)):
        with pytest.raises(ValueError):
            m.batch(bad)
    b = m.batch(X0())
    assert tuple(b.shape) == (8, 3, 32, 32)
    with pytest.raises(TypeError):
        b.mixed(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(TypeError):
        b.mixed([0] * 8)
    for bad in (torch.zeros(7, dtype=torch.int64), torch.zeros(8, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            b.mixed(bad)
    # the same through the direct calls
    with pytest.raises(TypeError):
        m(X0(dtype=torch.float16), y0())
    with pytest.raises(ValueError):
        m(X0(W=30), y0())
    with pytest.raises(ValueError):
        m(X0(), y0(4))
    with pytest.raises(TypeError):
        m.draw(torch.zeros(8), 32, 32)
    with pytest.raises(ValueError):
        m.draw(y0(), 0, 32)
    with pytest.raises(ValueError):
        m.apply(X0(), torch.zeros(8, 7, dtype=torch.int32))
    # right arguments, no device: refused too (there is no CPU path), not computed elsewhere
    with pytest.raises(RuntimeError):
        m(X0(), y0())
    assert m.step == 0


def test_train_step_refuses_a_bad_mixed_batch_before_device_work():
    from nvit_amd.config import named_config
    from nvit_amd.mix import Mixup
    from nvit_amd.model import ViT
    from nvit_amd.train import train_step
    cfg = named_config("micro")
    model = ViT(cfg)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    m = Mixup()
    step0 = model.step
    with pytest.raises(TypeError):
        train_step(model, opt, m.batch(X0()), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        train_step(model, opt, m.batch(X0()), y0(6))
    with pytest.raises(ValueError):
        train_step(model, opt, m.batch(X0()), y0(), accumulation_steps=3)
    assert model.step == step0 and m.step == 0


def test_state_dict_round_trip_before_the_device():
    from nvit_amd.mix import Mixup
    a = Mixup(seed=5)
    assert a.state_dict() == {"seed": 5, "step": 0} and a.step == 0
    a.load_state_dict({"seed": 2 ** 63 + 1, "step": 12})
    assert a.state_dict() == {"seed": 2 ** 63 + 1, "step": 12} and a.step == 12
    b = Mixup()
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict()
    for bad in ({"seed": -1, "step": 0}, {"seed": 0, "step": -1}, {"seed": 0, "step": 2 ** 63}):
        with pytest.raises(ValueError):
            b.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        Mixup().to("cpu")


def test_mixed_targets_slice_rows_and_check_their_arguments():
    from nvit_amd.mix import MixedTargets
    y, y2, lam = torch.arange(8), torch.arange(8).flip(0), torch.linspace(0, 1, 8)
    t = MixedTargets(y, y2, lam, 0.1)
    assert len(t) == 8 and tuple(t.shape) == (8,)
    s = t[2:6]
    assert torch.equal(s.y, y[2:6]) and torch.equal(s.y2, y2[2:6]) and torch.equal(s.lam, lam[2:6]) and s.smoothing == 0.1
    with pytest.raises(TypeError):
        t[0]
    with pytest.raises(TypeError):
        MixedTargets(y.int(), y2, lam)
    with pytest.raises(TypeError):
        MixedTargets(y, y2, lam.double())
    with pytest.raises(ValueError):
        MixedTargets(y, y2[:4], lam)
    with pytest.raises(ValueError):
        MixedTargets(y, y2, lam, 1.0)


def test_targets_for_writes_what_the_draw_would():
    from nvit_amd.mix import Mixup
    m = Mixup(label_smoothing=0.05)
    tab, t = m.targets_for([1, 2, 3, 4, 5], [("mixup", 0.3), ("cutmix", (2, 10, 4, 12))], 32, 32)
    f = lambda v: torch.tensor([v], dtype=torch.float32).view(torch.int32).item()
    assert tab.dtype == torch.int32 and tab.tolist() == [
        [1, f(0.3), 0, 0, 0, 0, 4, 0], [2, f(1 - 64 / 1024), 2, 10, 4, 12, 3, 0], [0, f(1.0), 0, 0, 0, 0, 2, 0],
        [2, f(1 - 64 / 1024), 2, 10, 4, 12, 1, 0], [1, f(0.3), 0, 0, 0, 0, 0, 0]]
    assert t.y.tolist() == [1, 2, 3, 4, 5] and t.y2.tolist() == [5, 4, 3, 2, 1] and t.smoothing == 0.05
    assert t.lam.tolist() == [torch.tensor(0.3).item(), 0.9375, 1.0, 0.9375, torch.tensor(0.3).item()]
    tab, t = m.targets_for([7, 8], [None], 8, 8)
    assert tab[:, 0].tolist() == [0, 0] and t.lam.tolist() == [1.0, 1.0] and t.y2.tolist() == [8, 7]
    for bad in ([("mixup", 1.5)], [("cutmix", (0, 9, 0, 4))], [("cutmix", (3, 2, 0, 4))], [("blend", 0.5)], []):
        with pytest.raises(ValueError):
            m.targets_for([1, 2], bad, 8, 8)
