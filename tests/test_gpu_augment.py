"""GPU: the on-device AutoAugment (nvit_augment_draw / nvit_augment_apply, nvit_amd/augment.py) against the numpy
restatement tests/augment_ref.py, which tests/test_augment_ref.py pins to Pillow.  Everything is integers, so every
comparison is exact.  The apply kernel has one code path for every image size (one workgroup per image, intermediates in
the global workspace), so there is no size threshold to straddle; 224x224x3 is there because 150 528 bytes is the size
at which an LDS-resident variant would have to change path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as R

SHAPES = [(3, 32, 32, 3), (3, 24, 40, 3), (3, 24, 40, 1), (2, 224, 224, 3)]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def aug():
    from nvit_amd.augment import AutoAugment
    return AutoAugment("cifar10", seed=0).to(dev())


def images(B, H, W, C, seed=0):
    """Image 0 random, image 1 low contrast with a channel offset, image 2 random with a constant middle channel."""
    g = np.random.default_rng(1000 * H + W + C + seed)
    x = g.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    if B > 1:
        x[1] = (g.integers(100, 140, (H, W, C)) + np.array([0, 20, -30])[:C]).astype(np.uint8)
    if B > 2:
        x[2, :, :, C // 2] = 77
    return x


def cases():
    for name in R.OPS:
        if name not in R.HAS_MAGNITUDE:
            yield name, 0, 0
            continue
        for m in (0, 4, 9):
            for sign in ((0, 1) if name in R.SIGNED else (0,)):
                yield name, m, sign


def run_u8(aug, x, params):
    """x uint8 numpy [B,H,W,C], params int numpy [B,2,8] -> the kernel's augmented uint8 batch."""
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev())
    out = aug.apply(torch.from_numpy(x).to(dev()), p, return_u8=True)
    return out.cpu().numpy()


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_op_alone_equals_the_restatement(aug, shape):
    B, H, W, C = shape
    x = images(B, H, W, C)
    n = 0
    for name, m, sign in cases():
        rows = aug.params_for([((name, m, sign), "Identity")] * B, H, W).cpu().numpy()
        assert np.array_equal(rows[0, 0], R.arg_table(H, W)[R.ID[name], m, sign])
        got = run_u8(aug, x, rows)
        same(got, R.apply_params(x, rows), (name, m, sign))
        if name == "Identity" or (name in R.SIGNED and m == 0) or (name == "Posterize" and m == 0):
            same(got, x, (name, m, sign, "is the identity"))
        n += 1
    assert n == 64   # 9 signed ops x 3 magnitudes x 2 signs + 2 unsigned x 3 + 4 without a magnitude


def test_second_slot_alone_equals_first_slot_alone(aug):
    """Identity as op 1 and the op as op 2: the same image as the other way round."""
    B, H, W, C = SHAPES[1]
    x = images(B, H, W, C)
    for name, m, sign in (("Rotate", 9, 1), ("Equalize", 0, 0), ("Sharpness", 9, 0), ("Contrast", 4, 1)):
        a = run_u8(aug, x, aug.params_for([((name, m, sign), "Identity")] * B, H, W).cpu().numpy())
        b = run_u8(aug, x, aug.params_for([("Identity", (name, m, sign))] * B, H, W).cpu().numpy())
        same(b, a, name)


def test_edge_images(aug):
    H, W = 24, 40
    g = np.random.default_rng(3)
    x = g.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    x[0, :, :, 1] = 200                          # a channel with a single value
    x[1] = 200                                   # every channel: 8 pixels off the last occupied bin -> Equalize step == 0
    x[1, 0, :8, :] = np.arange(8)[:, None]
    x[2, ::2] = 0                                # 0 and 255 only
    x[2, 1::2] = 255
    for op in ("AutoContrast", "Equalize"):
        rows = aug.params_for([(op, "Identity")] * 4, H, W).cpu().numpy()
        got = run_u8(aug, x, rows)
        same(got, R.apply_params(x, rows), op)
        same(got[0, :, :, 1], x[0, :, :, 1], op + ": single-valued channel unchanged")
        if op == "Equalize":
            same(got[1], x[1], "Equalize with step == 0 leaves the image unchanged")
    for op, value in (("Invert", None), ("Solarize", 0), ("Solarize", 255), ("Solarize", 256), ("Posterize", 0)):
        first = op if value is None else (op, {"value": value})
        rows = aug.params_for([(first, "Identity")] * 4, H, W).cpu().numpy()
        got = run_u8(aug, x, rows)
        same(got, R.apply_params(x, rows), (op, value))
        if op == "Invert" or value == 0 and op == "Solarize":
            same(got, 255 - x, (op, value, "inverts every pixel"))
        if value == 256:
            same(got, x, "Solarize above 255 changes nothing")
        if value == 255:
            assert (got[2] == 0).all()           # 255 -> 0, 0 stays
    for op, t in (("TranslateX", W), ("TranslateX", -W), ("TranslateY", H), ("TranslateY", -(H + 5)), ("TranslateX", W - 1)):
        rows = aug.params_for([((op, {"value": t}), "Identity")] * 4, H, W).cpu().numpy()
        got = run_u8(aug, x, rows)
        same(got, R.apply_params(x, rows), (op, t))
        assert got.any() == (abs(t) < (W if op == "TranslateX" else H)), (op, t)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_pairs_whose_second_op_needs_the_whole_first_result(aug, shape):
    B, H, W, C = shape
    x = images(B, H, W, C, seed=1)
    pairs = [(("Rotate", 9, 0), "Equalize"), (("ShearX", 9, 1), ("Sharpness", 9, 0)), (("Color", 9, 1), ("Contrast", 9, 0)),
             ("AutoContrast", ("Solarize", 4, 0)), ("Equalize", "Equalize"), (("TranslateY", 4, 1), "AutoContrast"),
             (("Sharpness", 9, 0), ("Rotate", 4, 1))]
    for pair in pairs:
        rows = aug.params_for([pair] * B, H, W).cpu().numpy()
        same(run_u8(aug, x, rows), R.apply_params(x, rows), pair)
    # a different pair per image in one launch
    rows = aug.params_for([pairs[i % len(pairs)] for i in range(B)], H, W).cpu().numpy()
    same(run_u8(aug, x, rows), R.apply_params(x, rows), "mixed")


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_fp32_output_has_the_bits_of_normalize_images(aug, shape):
    from nvit_amd import ops
    from nvit_amd.augment import AutoAugment
    B, H, W, C = shape
    x = torch.from_numpy(images(B, H, W, C, seed=2)).to(dev())
    rows = aug.params_for([(("Rotate", 4, 0), ("Color", 9, 0)), ("Equalize", ("Brightness", 9, 1)), ("Invert", "Identity")][:B],
                          H, W)
    u8 = aug.apply(x, rows, return_u8=True)
    assert not torch.equal(u8, x)
    f = aug.apply(x, rows)
    assert f.dtype == torch.float32 and tuple(f.shape) == (B, C, H, W)
    assert torch.equal(f, ops.normalize_images(u8))
    assert np.allclose(f.cpu().numpy(), R.normalize(u8.cpu().numpy()), atol=1e-6, rtol=0)
    other = AutoAugment("cifar10", mean=0.4, std=0.25).to(dev())
    assert torch.equal(other.apply(x, rows), ops.normalize_images(u8, 0.4, 0.25))
    # every probability 0: the deterministic pipeline alone
    off = AutoAugment([((a, 0.0, ma), (b, 0.0, mb)) for ((a, _, ma), (b, _, mb)) in R.POLICIES["imagenet"]], seed=9).to(dev())
    assert torch.equal(off(x), ops.normalize_images(x))
    assert off.step == 1


@pytest.mark.parametrize("policy", ["cifar10", "imagenet"])
def test_draw_equals_the_restatement_and_resumes(policy):
    from nvit_amd.augment import AutoAugment
    B, H, W = 1000, 32, 32
    for seed in (0, 0x1234567890ABCDEF):
        a = AutoAugment(policy, seed=seed).to(dev())
        for step in range(3):
            got = a.draw(B, H, W).cpu().numpy()
            assert np.array_equal(got, R.draw(R.POLICIES[policy], seed, step, 0, B, H, W)), (seed, step)
        assert a.step == 3 and a.state_dict() == {"seed": seed, "step": 3}
    # the probabilities are honoured roughly (the exact table is checked above): some ops on, some off
    ids = got[:, :, 0]
    assert 0.2 < (ids == 0).mean() < 0.8
    # a rank's slice of the step's batch
    whole = AutoAugment(policy, seed=5).to(dev()).draw(2 * B, H, W)
    part = AutoAugment(policy, seed=5, first_index=B).to(dev()).draw(B, H, W)
    assert torch.equal(part, whole[B:])
    # resume: a fresh object loaded with the state continues the sequence
    a = AutoAugment(policy, seed=21).to(dev())
    a.draw(64, H, W)
    a.draw(64, H, W)
    b = AutoAugment(policy, seed=0).to(dev())
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.draw(64, H, W), b.draw(64, H, W))
    assert np.array_equal(b.draw(64, H, W).cpu().numpy(), R.draw(R.POLICIES[policy], 21, 3, 0, 64, H, W))
    c = AutoAugment(policy, seed=21)
    c.load_state_dict({"seed": 21, "step": 4})   # loaded before .to(device)
    assert np.array_equal(c.to(dev()).draw(64, H, W).cpu().numpy(), R.draw(R.POLICIES[policy], 21, 4, 0, 64, H, W))


def test_call_is_draw_then_apply(aug):
    from nvit_amd.augment import AutoAugment
    B, H, W, C = 16, 32, 32, 3
    x = images(B, H, W, C, seed=4)
    a = AutoAugment("cifar10", seed=77).to(dev())
    a.load_state_dict({"seed": 77, "step": 6})
    f = a(torch.from_numpy(x).to(dev()))
    rows = R.draw(R.POLICIES["cifar10"], 77, 6, 0, B, H, W)
    assert (rows[:, :, 0] != 0).any()
    want = R.apply_params(x, rows)
    from nvit_amd import ops
    assert torch.equal(f, ops.normalize_images(torch.from_numpy(want).to(dev())))


# ------------------------------------------------------------------------------------------------ train step
def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    from nvit_amd.weights import formula_state_dict
    m = ViT(cfg)
    m.load_state_dict(formula_state_dict(cfg))
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m, m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")


def same_step(a, b, what):
    for i, (u, v) in enumerate(zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))):
        assert torch.equal(u, v), (what, ("logits", "loss", "grad_norm")[i], (u - v).abs().max().item())


def same_weights(ma, mb, what):
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), (what, n)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_with_augmentation_eager_graphed_and_plain(precision):
    """Three models from the same weights: `me` steps eagerly on aug.batch(u8), `mg` through a GraphedTrainStep that
    captured the augmentation, `mp` eagerly on the fp32 batch that a third, identically seeded augmentation produces
    outside the step.  All three agree bit for bit at every step; the three steps see three different batches."""
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro")
    B, warm = 8, 2
    g = np.random.default_rng(8)
    u8 = torch.from_numpy(g.integers(0, 256, (B, cfg.image_size, cfg.image_size, cfg.channels), dtype=np.uint8)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(dev())
    (me, oe), (mg, og), (mp, op_) = build(cfg, precision), build(cfg, precision), build(cfg, precision)
    ae, ag, ap = (AutoAugment("cifar10", seed=31).to(dev()) for _ in range(3))
    for _ in range(warm):
        train_step(me, oe, ae.batch(u8), y)
        train_step(mp, op_, ap(u8), y)
    graph = GraphedTrainStep(mg, og, ag.batch(u8), y, warmup=warm)
    assert ae.step == ag.step == ap.step == warm
    seen = []
    for i in range(3):
        xp = ap(u8)
        seen.append(xp)
        eager = train_step(me, oe, ae.batch(u8), y)
        same_step(eager, graph(u8, y), f"graphed step {i}")
        same_step(eager, train_step(mp, op_, xp, y), f"plain step {i}")
    assert not any(torch.equal(seen[i], seen[j]) for i in range(3) for j in range(i))
    assert ae.step == ag.step == warm + 3
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the plain steps")
    # eager and graphed steps alternate on one model
    same_step(train_step(me, oe, ae.batch(u8), y), train_step(mg, og, ag.batch(u8), y), "eager step on the graphed model")
    same_step(train_step(me, oe, ae.batch(u8), y), graph(ag.batch(u8), y), "replay after an eager step")
    assert ae.step == ag.step == warm + 5
    same_weights(me, mg, "after eager step and replay")
    assert me.step == mg.step == warm + 5
    with pytest.raises(ValueError):
        graph(ae.batch(u8), y)   # another augmentation's batch


def test_accumulation_augments_the_batch_once_and_a_tensor_takes_the_old_path():
    from nvit_amd import ops
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.train import train_step
    cfg = named_config("micro")
    g = np.random.default_rng(9)
    u8 = torch.from_numpy(g.integers(0, 256, (8, cfg.image_size, cfg.image_size, cfg.channels), dtype=np.uint8)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (8,))).to(dev())
    (ma, oa), (mb, ob) = build(cfg, "bf16"), build(cfg, "bf16")
    a, probe = AutoAugment("imagenet", seed=2).to(dev()), AutoAugment("imagenet", seed=2).to(dev())
    for i in range(2):
        got = train_step(ma, oa, a.batch(u8), y, accumulation_steps=2)
        assert a.step == i + 1                     # one draw for the whole batch, not one per micro-batch
        same_step(got, train_step(mb, ob, probe(u8), y, accumulation_steps=2), f"accumulated step {i}")
    same_weights(ma, mb, "accumulated")
    # every probability 0: the step on the uint8 batch is the step on normalize_images(u8)
    off = AutoAugment([(("Rotate", 0.0, 9), ("Equalize", 0.0, 0))]).to(dev())
    same_step(train_step(ma, oa, off.batch(u8), y), train_step(mb, ob, ops.normalize_images(u8), y), "augmentation off")
    same_weights(ma, mb, "augmentation off")
