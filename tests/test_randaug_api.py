"""CPU: RandAugment's argument checks, timm's config string, the hand-written table and the batch() plumbing - what
fires before any device work."""
import math

import pytest
import torch

from nvit_amd.randaug import MAX_LAYERS, ROW, RandAugment, parse_config


def test_defaults_are_the_deit_recipe():
    ra = RandAugment()
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.magnitude_max) == (9.0, 2, 0.5, 10.0)
    assert ra.increasing is True and ra.prob == 0.5 and ra.interpolation == "random" and ra.fill == (128, 128, 128)
    assert ra.translate_pct == 0.45 and (ra.mean, ra.std) == (0.5, 0.5)
    assert ra.state_dict() == {"seed": 0, "step": 0}
    ra.load_state_dict({"seed": 5, "step": 11})
    assert ra.state_dict() == {"seed": 5, "step": 11}
    import nvit_amd
    assert nvit_amd.RandAugment is RandAugment


def test_from_config_reads_timm_strings():
    assert parse_config("rand-m9-mstd0.5-inc1") == {"magnitude": 9, "magnitude_std": 0.5, "increasing": True}
    ra = RandAugment.from_config("rand-m9-mstd0.5-inc1", fill=(124, 116, 104), seed=3, interpolation="bicubic")
    assert (ra.magnitude, ra.magnitude_std, ra.increasing, ra.num_layers) == (9.0, 0.5, True, 2)
    assert ra.fill == (124, 116, 104) and ra.seed == 3 and ra.interpolation == "bicubic"
    rb = RandAugment.from_config("rand-m7-n3-mstd101")
    assert (rb.magnitude, rb.num_layers, rb.increasing) == (7.0, 3, True) and math.isinf(rb.magnitude_std)
    rc = RandAugment.from_config("rand-m6-mmax8-inc0-p0.7-mstd100")
    assert (rc.magnitude, rc.magnitude_max, rc.increasing, rc.prob, rc.magnitude_std) == (6.0, 8.0, False, 0.7, 100.0)
    assert RandAugment.from_config("rand-m9-n2", num_layers=4).num_layers == 4   # a keyword wins over the string
    assert RandAugment.from_config("rand").magnitude == 9.0
    for bad in ("rand-m9-w0", "rand-m9-x3", "augmix-m3", "rand-m", "rand-9", "rand-mstd", "rand-n2.5", "rand-m9--n2"):
        with pytest.raises(ValueError):
            RandAugment.from_config(bad)
    with pytest.raises(TypeError):
        RandAugment.from_config(9)
    with pytest.raises(ValueError):
        RandAugment.from_config("rand-m11")   # magnitude above the level scale
    with pytest.raises(ValueError):
        RandAugment.from_config("rand-n5")


def test_constructor_argument_errors():
    for kw in ({"num_layers": 0}, {"num_layers": MAX_LAYERS + 1}, {"magnitude": -1}, {"magnitude": 10.5},
               {"magnitude": math.nan}, {"magnitude": math.inf}, {"magnitude_std": -0.1}, {"magnitude_std": math.nan},
               {"magnitude_max": 0}, {"magnitude_max": 11}, {"magnitude_max": math.nan}, {"prob": 1.5}, {"prob": -0.1},
               {"prob": math.nan}, {"interpolation": "nearest"}, {"fill": (1, 2)}, {"fill": (0, 0, 256)}, {"fill": (-1,)},
               {"fill": ()}, {"translate_pct": 1.5}, {"translate_pct": math.nan}, {"std": 0}, {"mean": math.nan},
               {"seed": -1}, {"seed": 2 ** 64}, {"first_index": -1}, {"first_index": 2 ** 62}):
        with pytest.raises(ValueError):
            RandAugment(**kw)
    for kw in ({"num_layers": 2.0}, {"num_layers": True}, {"magnitude": "9"}, {"magnitude_std": None}, {"magnitude_max": "10"},
               {"prob": "0.5"}, {"interpolation": 1}, {"fill": 1.5}, {"fill": (1.0, 2.0, 3.0)}, {"fill": "grey"},
               {"translate_pct": "0.45"}, {"mean": "0.5"}, {"seed": 1.0}, {"first_index": "0"}, {"increasing": "yes"}):
        with pytest.raises(TypeError):
            RandAugment(**kw)
    assert RandAugment(magnitude_std=math.inf).magnitude_std == math.inf
    assert RandAugment(magnitude_std=0).magnitude_std == 0.0
    assert RandAugment(fill=7).fill == (7,) and RandAugment(fill=[1, 2, 3]).fill == (1, 2, 3)
    assert RandAugment(first_index=2 ** 33 + 5).first_index == 2 ** 33 + 5


def test_call_errors_fire_without_a_gpu():
    ra = RandAugment(seed=3)
    p = torch.zeros(2, 2, ROW, dtype=torch.int32)
    with pytest.raises(TypeError):
        ra(torch.zeros(2, 32, 32, 3))                                   # not uint8
    with pytest.raises(TypeError):
        ra.apply(torch.zeros(2, 32, 32, 3, dtype=torch.int32), p)
    with pytest.raises(ValueError):
        ra(torch.zeros(32, 32, 3, dtype=torch.uint8))                   # rank
    with pytest.raises(ValueError):
        ra(torch.zeros(2, 3, 32, 32, dtype=torch.uint8))                # C = 32
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), p[:1])   # table of another batch
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 2, 8, dtype=torch.int32))   # AutoAugment's row
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 5, ROW, dtype=torch.int32))  # five layers
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), p.to(torch.int64))
    with pytest.raises(ValueError):
        ra.apply(torch.zeros(2, 32, 30, 3, dtype=torch.uint8), p)       # W % 4 for the fp32 output
    with pytest.raises(ValueError):
        ra(torch.zeros(2, 32, 30, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        RandAugment(fill=(124, 116, 104))(torch.zeros(2, 32, 32, 1, dtype=torch.uint8))   # three colours, one channel
    with pytest.raises(RuntimeError):
        ra.draw(4, 32, 32)                                              # no device yet: no CPU path
    with pytest.raises(RuntimeError):
        ra(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ra.to("cpu")


def test_params_for_errors_and_shapes():
    ra = RandAugment()
    t = ra.params_for([["Invert", ("Rotate", 9, 1, "bicubic")], [None, ("Solarize", {"value": 0})]], 24, 40)
    assert t.shape == (2, 2, ROW) and t.dtype == torch.int32
    assert t[0, 0].tolist() == [14] + [0] * (ROW - 1) and t[0, 1, 0] == 5 and t[0, 1, 1] == 1 and not t[1, 0].any()
    assert ra.params_for([[("ShearX", 4.5, 0)]] * 3, 32, 32).shape == (3, 1, ROW)
    for bad in ([["Blur"]], [[("Rotate", 11, 0)]], [[("Rotate", -1, 0)]], [[("Rotate", 9, 2)]], [[("Rotate", 9, 0, "nearest")]],
                [[("Rotate", 9, 0, "random")]], [["Invert"], ["Invert", "Invert"]], [[]], [["Invert"] * 5], [],
                [[("Posterize", {"value": 9})]], [[("Solarize", {"value": 257})]], [[("SolarizeAdd", {"value": -1})]],
                [[("ShearX", {"value": math.nan})]], [["Identity"]]):
        with pytest.raises(ValueError):
            ra.params_for(bad, 24, 40)
    for bad in ([[5]], [[("Rotate", "9", 0)]], [[("Color", {"value": "1"})]], [[("Rotate", 9, 0, 1)]]):
        with pytest.raises(TypeError):
            ra.params_for(bad, 24, 40)
    with pytest.raises(ValueError):
        ra.params_for([["Invert"]], 0, 40)


def test_batch_plumbing_and_the_w4_rule():
    from nvit_amd.augment import AugmentedBatch
    from nvit_amd.crop import ErasedBatch, RandomErasing, RandomResizedCrop
    from nvit_amd.mix import MixedBatch, Mixup
    from nvit_amd.train import _unwrap_input, _wrap_input
    ra = RandAugment()
    u8 = torch.zeros(8, 24, 40, 3, dtype=torch.uint8)
    xb = ra.batch(u8)
    assert isinstance(xb, AugmentedBatch) and tuple(xb.shape) == (8, 24, 40, 3) and xb.device == u8.device and xb.augment is ra
    with pytest.raises(ValueError):
        ra.batch(torch.zeros(8, 24, 42, 3, dtype=torch.uint8))          # W % 4
    with pytest.raises(ValueError):
        ra.batch(torch.zeros(8, 24, 40, 4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        ra.batch(torch.zeros(8, 24, 40, 3))
    with pytest.raises(ValueError):
        RandAugment(fill=(1, 2, 3)).batch(torch.zeros(8, 24, 40, 1, dtype=torch.uint8))
    assert tuple(RandAugment(fill=9).batch(torch.zeros(8, 24, 40, 1, dtype=torch.uint8)).shape) == (8, 24, 40, 1)
    # the full chain nests and unwraps as AutoAugment's does
    rrc, erase, mix = RandomResizedCrop(32), RandomErasing(), Mixup()
    src = torch.zeros(8, 50, 60, 3, dtype=torch.uint8)
    chain = mix.batch(erase.batch(ra.batch(rrc.batch(src))))
    assert isinstance(chain, MixedBatch) and isinstance(chain.X, ErasedBatch) and tuple(chain.shape) == (8, 3, 32, 32)
    stages, x = _unwrap_input(chain)
    assert stages["augment"] is ra and stages["crop"] is rrc and stages["mix"] is mix and x is src
    again = _wrap_input(stages, src)
    assert isinstance(again, MixedBatch) and again.X.X.augment is ra


def test_train_step_refuses_a_bad_batch_before_device_work():
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import train_step
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    xb = RandAugment().batch(torch.zeros(8, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        train_step(m, opt, xb, torch.zeros(8, dtype=torch.int64), accumulation_steps=3)
    with pytest.raises(RuntimeError):   # a CPU batch: no CPU path
        train_step(m, opt, xb, torch.zeros(8, dtype=torch.int64))
    assert m.step == 0


def test_checkpoint_carries_the_stage():
    from nvit_amd.checkpoint import build_checkpoint
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    ra = RandAugment(seed=4)
    ra.load_state_dict({"seed": 4, "step": 17})
    ck = build_checkpoint(m, opt, 17, {}, rand_augment=ra)
    assert ck["rand_augment"] == {"seed": 4, "step": 17}
    assert "rand_augment" not in build_checkpoint(m, opt, 17, {})
    rb = RandAugment()
    rb.load_state_dict(ck["rand_augment"])
    assert rb.state_dict() == ra.state_dict()
