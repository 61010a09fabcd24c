"""GPU, model level: evaluation from stored uint8 data.  `predict`, `validate`, `estimate_loss` and `GraphedEval` on
`ResizeCenterCrop.batch(u8)` against the same calls on the tensor `rcc(u8)`, bit for bit; the captured transform against
the eager one; batches that do not fit the graphs; another image size than the model's; the EMA's module; and the train
step's refusal.  tests/test_gpu_center_crop.py holds the transform itself to its restatement."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 8
SHAPES = {"mini": (72, 80, 56), "micro_k": (40, 40, 32)}   # config -> source Hs, Ws and the crop's size (the model's)


def build(name, precision):
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    from nvit_amd.weights import load_formula_weights
    cfg = named_config(name)
    m = ViT(cfg)
    load_formula_weights(m, cfg)
    m = m.to(DEV).set_precision(precision).train()
    normalize_matrices(m)
    return m, cfg


def stored(cfg, n, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (n, Hs, Ws, cfg.channels), generator=g, dtype=torch.uint8)
    y = torch.randint(0, cfg.num_classes, (n,), generator=g)
    return u8.to(DEV), y.to(DEV)


def loaders(rcc, cfg, Hs, Ws):
    """Three full batches and a short fourth: as `rcc.batch(u8)` objects and as the tensors `rcc(u8)`."""
    data = [stored(cfg, n, Hs, Ws, 20 + k) for k, n in enumerate((B, B, B, 5))]
    return [(rcc.batch(u), y) for u, y in data], [(rcc(u), y) for u, y in data]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_evaluation_on_the_batch_object_equals_evaluation_on_the_tensor(name, precision):
    from nvit_amd import GraphedEval, ResizeCenterCrop, evaluate
    m, cfg = build(name, precision)
    Hs, Ws, size = SHAPES[name]
    assert size == cfg.image_size
    rcc = ResizeCenterCrop(size, interpolation="bicubic", mean=0.45, std=0.225)
    objs, tens = loaders(rcc, cfg, Hs, Ws)
    assert tuple(objs[0][0].shape) == tuple(tens[0][0].shape)
    for (xo, _), (xt, _) in zip(objs, tens):
        assert torch.equal(evaluate.predict(m, xo), evaluate.predict(m, xt))
    v_want, e_want = evaluate.validate(m, tens), evaluate.estimate_loss(m, tens, 4)
    assert evaluate.validate(m, objs) == v_want
    assert evaluate.estimate_loss(m, objs, 4) == e_want
    assert evaluate.estimate_loss(m, objs, 2) == evaluate.estimate_loss(m, tens, 2)

    # the transform captured with the forward: the full batches replay, the short one runs eagerly
    ge = GraphedEval(m, *objs[0])
    assert ge.X.dtype == torch.uint8 and tuple(ge.X.shape) == (B, Hs, Ws, cfg.channels)
    assert [ge._fits(x, y) for x, y in objs] == [True, True, True, False]
    assert not ge._fits(*tens[0]), "a plain tensor does not fit graphs built on a crop"
    other = ResizeCenterCrop(size, interpolation="bicubic", mean=0.45, std=0.25)
    assert not ge._fits(other.batch(objs[0][0].u8), objs[0][1]), "nor does another transform"
    assert ge._fits(ResizeCenterCrop(*rcc.params()).batch(objs[1][0].u8), objs[1][1]), "an equal one does"
    for (xo, _), (xt, _) in zip(objs, tens):
        assert torch.equal(ge.predict(xo), evaluate.predict(m, xt))
    assert torch.equal(ge.predict(tens[1][0]), evaluate.predict(m, tens[1][0]))
    assert ge.validate(objs) == v_want and ge.validate(iter(objs)) == v_want
    assert ge.estimate_loss(objs, 4) == e_want
    # a fifth batch of another source size runs eagerly inside the same call and agrees
    u5, y5 = stored(cfg, B, Hs + 8, Ws + 4, 31)
    assert not ge._fits(rcc.batch(u5), y5)
    v5 = evaluate.validate(m, tens + [(rcc(u5), y5)])
    assert ge.validate(objs + [(rcc.batch(u5), y5)]) == v5 and v5 != v_want
    assert ge.estimate_loss(objs + [(rcc.batch(u5), y5)], 5) == evaluate.estimate_loss(m, tens + [(rcc(u5), y5)], 5)
    # the reverse: graphs built on a plain tensor take the batch object eagerly, and tensors as before
    gp = GraphedEval(m, *tens[0])
    assert gp._fits(*tens[1]) and not gp._fits(*objs[1])
    assert torch.equal(gp.predict(objs[1][0]), evaluate.predict(m, tens[1][0]))
    assert gp.validate(objs) == v_want and gp.validate(tens) == v_want
    assert m.training


def test_another_size_than_the_models_with_dynamic_img_size():
    from nvit_amd import GraphedEval, ResizeCenterCrop, evaluate
    m, cfg = build("mini", "bf16")
    rcc = ResizeCenterCrop(80)
    objs, tens = loaders(rcc, cfg, 96, 104)
    with pytest.raises(ValueError):
        evaluate.predict(m, objs[0][0])   # 80 is not the model's 56
    m.set_dynamic_img_size(True)
    assert tuple(tens[0][0].shape) == (B, cfg.channels, 80, 80)
    assert torch.equal(evaluate.predict(m, objs[0][0]), evaluate.predict(m, tens[0][0]))
    v_want = evaluate.validate(m, tens)
    assert evaluate.validate(m, objs) == v_want
    ge = GraphedEval(m, *objs[0])
    assert ge.validate(objs) == v_want
    assert torch.equal(ge.predict(objs[1][0]), evaluate.predict(m, tens[1][0]))


def test_the_ema_module_takes_the_batch_object():
    from nvit_amd import ModelEma, ResizeCenterCrop, evaluate
    from nvit_amd.train import train_step
    from nvit_amd.weights import synthetic_batch
    m, cfg = build("micro_k", "bf16")
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ema = ModelEma(m)
    opt.attach_ema(ema)
    for seed in (1, 2):
        train_step(m, opt, *(t.to(DEV) for t in synthetic_batch(cfg, B, seed=seed)))
    rcc = ResizeCenterCrop(32)
    objs, tens = loaders(rcc, cfg, 40, 40)
    want = evaluate.validate(ema.module, tens)
    assert evaluate.validate(ema.module, objs) == want
    assert want != evaluate.validate(m, tens), "the shadow is not the model"
    assert torch.equal(evaluate.predict(ema.module, objs[0][0]), evaluate.predict(ema.module, tens[0][0]))


def test_train_steps_refuse_the_batch_object():
    from nvit_amd import GraphedTrainStep, ResizeCenterCrop
    from nvit_amd.train import train_step
    m, cfg = build("micro_k", "bf16")
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    u8, y = stored(cfg, B, 40, 40, 3)
    xb = ResizeCenterCrop(32).batch(u8)
    with pytest.raises(TypeError, match="CenterCroppedBatch"):
        train_step(m, opt, xb, y)
    with pytest.raises(TypeError, match="CenterCroppedBatch"):
        GraphedTrainStep(m, opt, xb, y)
