"""CPU: the numpy restatement of the AutoAugment ops (tests/augment_ref.py) against Pillow - the committed fixture
tests/golden/augment_pil.npz (tools/make_golden_augment.py) and, where PIL is importable, live calls at 224x224 - bit for
bit; the Philox4x32-10 known-answer vectors; the shipped policies; the host tables of nvit_amd/augment.py against the
restatement's; and the API's argument errors, none of which needs a GPU."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "augment_pil.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases():
    for name in R.OPS:
        if name not in R.HAS_MAGNITUDE:
            yield name, 0, 0
            continue
        for m in (0, 4, 9):
            for sign in ((0, 1) if name in R.SIGNED else (0,)):
                yield name, m, sign


@pytest.mark.parametrize("name", R.OPS)
def test_restatement_equals_the_pillow_fixture_bit_for_bit(golden, name):
    tags = [k[3:] for k in golden.files if k.startswith("in/")]
    assert sorted(tags) == ["const_32x32", "low_24x40", "low_32x32", "rand_24x40", "rand_24x40x1", "rand_32x32"]
    n = 0
    for tag in tags:
        img = golden["in/" + tag]
        for op, m, sign in _cases():
            if op != name:
                continue
            want = golden[f"out/{tag}/{op}/{m}/{sign}"]
            got = R.apply_op(img, op, R.magnitude(op, m, sign, img.shape[1]))
            assert got.dtype == np.uint8 and got.shape == img.shape
            assert np.array_equal(got, want), (tag, op, m, sign, int((got != want).sum()))
            n += 1
    assert n == 6 * (1 if name not in R.HAS_MAGNITUDE else (6 if name in R.SIGNED else 3))


def test_fixture_covers_the_edges_it_is_there_for(golden):
    const = golden["in/const_32x32"]
    assert len(np.unique(const[:, :, 1])) == 1
    for op in ("AutoContrast", "Equalize"):   # a single-valued channel is left unchanged
        assert np.array_equal(golden[f"out/const_32x32/{op}/0/0"][:, :, 1], const[:, :, 1])
    low = golden["in/low_24x40"]
    assert int(low.max()) - int(low.min()) < 100   # low contrast: AutoContrast and Equalize have work to do
    assert not np.array_equal(golden["out/low_24x40/AutoContrast/0/0"], low)
    assert os.path.getsize(GOLDEN) < 1_000_000


@pytest.mark.parametrize("name", ["Rotate", "Sharpness", "Equalize", "AutoContrast", "Contrast"])
def test_restatement_equals_live_pillow_at_224(name):
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_augment",
                                                  os.path.join(os.path.dirname(HERE), "tools", "make_golden_augment.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    g = np.random.default_rng(5)
    imgs = [g.integers(0, 256, (224, 224, 3), dtype=np.uint8), g.integers(90, 130, (224, 224, 3)).astype(np.uint8)]
    for img in imgs:
        for m in ((0, 4, 9) if name in R.HAS_MAGNITUDE else (0,)):
            for sign in ((0, 1) if name in R.SIGNED else (0,)):
                v = R.magnitude(name, m, sign, 224)
                assert np.array_equal(R.apply_op(img, name, v), G.pil_op(img, name, v)), (name, m, sign)


def test_equalize_step_zero_and_translate_out_of_the_image():
    # fewer than 255 pixels outside the last occupied bin: step == 0, unchanged
    img = np.full((16, 16, 1), 200, dtype=np.uint8)
    img[0, :8, 0] = np.arange(8)
    assert np.array_equal(R.apply_op(img, "Equalize"), img)
    rgb = np.random.default_rng(0).integers(1, 256, (8, 12, 3), dtype=np.uint8)
    assert not R.apply_op(rgb, "TranslateX", 12).any() and not R.apply_op(rgb, "TranslateY", -8).any()
    assert R.apply_op(rgb, "TranslateX", 11).any()


def test_magnitude_tables():
    assert [R.magnitude("Posterize", m, 0, 32) for m in range(10)] == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert [R.magnitude("Solarize", m, 0, 32) for m in (0, 4, 9)] == [255, 141, 0]
    assert R.magnitude("TranslateY", 9, 1, 40) == -int(150 / 331 * 40) == -18
    assert R.magnitude("ShearX", 9, 1, 32) == -0.3 and R.magnitude("Rotate", 9, 0, 32) == 30.0
    assert abs(R.magnitude("Color", 9, 1, 32) - 0.1) < 1e-12 and R.magnitude("Color", 0, 1, 32) == 1.0


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(R.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("name", ["cifar10", "imagenet"])
def test_shipped_policies_validate_and_match_the_restatement(name):
    from nvit_amd import augment as A
    pol = A.validate_policy(name)
    assert len(pol) == 25
    for sub in pol:
        assert len(sub) == 2
        for op, p, m in sub:
            assert op in A.OPS and 0.0 <= p <= 1.0 and 0 <= m <= 9
    assert [[tuple(e) for e in sub] for sub in pol] == [[tuple(e) for e in sub] for sub in R.POLICIES[name]]
    assert A.AutoAugment(name).policy == pol
    assert A.validate_policy("cifar100") == A.validate_policy("cifar10")
    assert A.OPS == R.OPS


@pytest.mark.parametrize("hw", [(32, 32), (24, 40), (224, 224)])
def test_host_argument_table_equals_the_restatement(hw):
    from nvit_amd import augment as A
    assert np.array_equal(A.arg_table(*hw).numpy(), R.arg_table(*hw))


def test_draw_restatement_is_a_function_of_the_global_index():
    pol = R.POLICIES["cifar10"]
    whole = R.draw(pol, 7, 2, 0, 40, 32, 32)
    assert np.array_equal(R.draw(pol, 7, 2, 25, 15, 32, 32), whole[25:])
    assert not np.array_equal(R.draw(pol, 7, 3, 0, 40, 32, 32), whole)
    assert not np.array_equal(R.draw(pol, 8, 2, 0, 40, 32, 32), whole)
    assert set(np.unique(whole[:, :, 0])) <= set(range(15))


def test_argument_errors_fire_without_a_gpu():
    from nvit_amd.augment import AutoAugment
    aug = AutoAugment("cifar10", seed=3)
    assert aug.state_dict() == {"seed": 3, "step": 0}
    aug.load_state_dict({"seed": 5, "step": 11})
    assert aug.state_dict() == {"seed": 5, "step": 11}
    p = torch.zeros(2, 2, 8, dtype=torch.int32)
    with pytest.raises(TypeError):
        aug(torch.zeros(2, 32, 32, 3))                              # not uint8
    with pytest.raises(TypeError):
        aug.apply(torch.zeros(2, 32, 32, 3, dtype=torch.int32), p)
    with pytest.raises(ValueError):
        aug(torch.zeros(32, 32, 3, dtype=torch.uint8))              # rank
    with pytest.raises(ValueError):
        aug(torch.zeros(2, 3, 32, 32, dtype=torch.uint8))           # C = 32
    with pytest.raises(ValueError):
        aug.apply(torch.zeros(2, 32, 32, 2, dtype=torch.uint8), p)  # C = 2
    with pytest.raises(ValueError):
        aug.batch(torch.zeros(2, 32, 32, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        aug.apply(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), p[:1])   # table of another batch
    with pytest.raises(ValueError):
        AutoAugment([(("Blur", 0.5, 1), ("Invert", 0.5, 0))])      # unknown op
    with pytest.raises(ValueError):
        AutoAugment([(("Rotate", 0.5, 10), ("Invert", 0.5, 0))])   # magnitude index
    with pytest.raises(ValueError):
        AutoAugment([(("Rotate", 0.5, -1), ("Invert", 0.5, 0))])
    with pytest.raises(ValueError):
        AutoAugment([(("Rotate", 1.5, 1), ("Invert", 0.5, 0))])    # probability
    with pytest.raises(ValueError):
        AutoAugment([(("Rotate", -0.1, 1), ("Invert", 0.5, 0))])
    with pytest.raises(ValueError):
        AutoAugment([])                                             # empty policy
    with pytest.raises(ValueError):
        AutoAugment("svhn")
    with pytest.raises(ValueError):
        AutoAugment([(("Rotate", 0.5, 1),)])                        # one op only
    with pytest.raises(ValueError):
        aug.params_for([("Blur", "Invert")], 32, 32)
    with pytest.raises(ValueError):
        aug.params_for([(("Rotate", 12, 0), "Invert")], 32, 32)
    with pytest.raises(RuntimeError):
        aug.draw(4, 32, 32)                                         # no device yet: no CPU path
    with pytest.raises(RuntimeError):
        aug(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))
    rows = aug.params_for([("Invert", ("Solarize", {"value": 0})), (("Rotate", 9, 1), "Identity")], 24, 40)
    assert rows.shape == (2, 2, 8) and rows.dtype == torch.int32
    assert np.array_equal(rows.numpy()[1, 0], R.arg_table(24, 40)[R.ID["Rotate"], 9, 1])
    assert rows[0, 1].tolist() == [R.ID["Solarize"], 0, 0, 0, 0, 0, 0, 0]


def test_train_step_refuses_a_bad_augmented_batch_before_device_work():
    from nvit_amd.augment import AugmentedBatch, AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import train_step
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    xb = AutoAugment().batch(torch.zeros(8, 32, 32, 3, dtype=torch.uint8))
    assert isinstance(xb, AugmentedBatch) and tuple(xb.shape) == (8, 32, 32, 3)
    with pytest.raises(ValueError):
        train_step(m, opt, xb, torch.zeros(8, dtype=torch.int64), accumulation_steps=3)
    with pytest.raises(RuntimeError):   # a CPU batch: no CPU path
        train_step(m, opt, xb, torch.zeros(8, dtype=torch.int64))
    assert m.step == 0
