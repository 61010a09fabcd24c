"""GPU: which calls fit a captured step (the batch-object protocol).  A GraphedTrainStep captured on the full
chain mix.batch(erase.batch(aug.batch(rrc.batch(u8)), mean, std)) takes the bare uint8 tensor, the chain of the captured
objects and any part of it, and all three are the same step; a stage that is not the captured object of its kind, or an
erase.batch with another (mean, std), is refused with the stage's word.  GraphedEval on rcc.batch(u8) replays for a second
transform of equal parameters and runs another one eagerly.  The refusals of another LRSchedule, DropPath and PatchDropout
are in test_gpu_lr_schedule.py, test_gpu_droppath.py and test_gpu_patchdrop.py, that of another ModelEma in test_gpu_ema.py.

micro at 32x32, B = 8.  Three identically seeded setups are captured once for the file: starting three calls from equal
weights, moments and counters needs three of them (a captured step cannot be wound back: the optimizer's load_state_dict
replaces the tensors whose addresses the graph holds); the refusals use the first."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 8
MEAN, STD = 0.4, 0.25


class Setup:
    """Model, optimizer and the four stages, identically seeded per instance, and the step captured on the full chain."""

    def __init__(self, u8, y, capture=True):
        from nvit_amd import AutoAugment, GraphedTrainStep, Mixup, RandomErasing, RandomResizedCrop
        from nvit_amd.config import named_config
        from nvit_amd.model import ViT
        from nvit_amd.train import normalize_matrices
        from nvit_amd.weights import load_formula_weights
        cfg = named_config("micro")
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        self.model = m.to(DEV).set_precision("bf16").train()
        normalize_matrices(self.model)
        self.opt = self.model.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
        self.rrc = RandomResizedCrop(32, interpolation="bicubic", seed=3).to(DEV)
        self.aug = AutoAugment("cifar10", seed=5).to(DEV)
        self.erase = RandomErasing(prob=0.75, seed=7).to(DEV)
        self.mix = Mixup(seed=6).to(DEV)
        self.graph = GraphedTrainStep(self.model, self.opt, self.full(u8), y, warmup=1) if capture else None

    def full(self, u8):
        return self.mix.batch(self.erase.batch(self.aug.batch(self.rrc.batch(u8)), MEAN, STD))

    def steps(self):
        return self.rrc.step, self.aug.step, self.erase.step, self.mix.step


@pytest.fixture(scope="module")
def batch():
    from nvit_amd.config import named_config
    cfg, g = named_config("micro"), np.random.default_rng(12)
    return (torch.from_numpy(g.integers(0, 256, (B, 40, 40, cfg.channels), dtype=np.uint8)).to(DEV),
            torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(DEV))


@pytest.fixture(scope="module")
def setups(batch):
    return [Setup(*batch) for _ in range(3)]


def test_the_bare_tensor_the_full_chain_and_a_part_of_it_are_the_same_step(setups, batch):
    from nvit_amd.train import train_step
    u8, y = batch
    a, b, c = setups
    assert a.steps() == b.steps() == c.steps() == (1, 1, 1, 1) and a.model.step == b.model.step == c.model.step == 1
    eager = Setup(u8, y, capture=False)   # the same steps without a graph: what the three replays must give
    train_step(eager.model, eager.opt, eager.full(u8), y)
    want = train_step(eager.model, eager.opt, eager.full(u8), y)
    outs = [a.graph(u8, y), b.graph(b.full(u8), y), c.graph(c.aug.batch(c.rrc.batch(u8)), y)]
    for what, out in zip(("the bare tensor", "the full chain", "a partial chain"), outs):
        for name, u, v in zip(("logits", "loss", "grad_norm"), (want[0], want[1], want[3]), (out[0], out[1], out[3])):
            assert torch.equal(u, v), (what, name, (u - v).abs().max().item())
    for s in setups:
        assert s.steps() == (2, 2, 2, 2) and s.model.step == 2
        for (n, p), (_, q) in zip(eager.model.named_parameters(), s.model.named_parameters()):
            assert torch.equal(p, q), n
    assert a.graph.mix is a.mix and a.graph.erase is a.erase and a.graph.augment is a.aug and a.graph.crop is a.rrc


@pytest.mark.parametrize("kind", ["Mixup", "RandomErasing", "AutoAugment", "RandAugment", "RandomResizedCrop", "mean / std"])
def test_a_stage_that_is_not_the_captured_one_is_refused_with_its_word(setups, batch, kind):
    from nvit_amd import AutoAugment, Mixup, RandAugment, RandomErasing, RandomResizedCrop
    s, (u8, y) = setups[0], batch
    before = s.steps()
    inner = s.aug.batch(s.rrc.batch(u8))
    X, word = {
        "Mixup": lambda: (Mixup(seed=6).to(DEV).batch(s.erase.batch(inner, MEAN, STD)), "another Mixup"),
        "RandomErasing": lambda: (s.mix.batch(RandomErasing(prob=0.75, seed=7).to(DEV).batch(inner, MEAN, STD)), "another RandomErasing"),
        "AutoAugment": lambda: (AutoAugment("cifar10", seed=5).to(DEV).batch(s.rrc.batch(u8)), "another augmentation"),
        "RandAugment": lambda: (s.erase.batch(RandAugment(seed=5).to(DEV).batch(s.rrc.batch(u8)), MEAN, STD), "another augmentation"),
        "RandomResizedCrop": lambda: (RandomResizedCrop(32, interpolation="bicubic", seed=3).to(DEV).batch(u8), "another RandomResizedCrop"),
        "mean / std": lambda: (s.mix.batch(s.erase.batch(inner, MEAN, 0.5)), "another mean / std of erase.batch"),
    }[kind]()
    with pytest.raises(ValueError, match="captured with " + word):
        s.graph(X, y)
    assert s.steps() == before   # refused before anything ran


def test_graphed_eval_replays_an_equal_transform_and_runs_another_one_eagerly(setups, batch):
    from nvit_amd import GraphedEval, ResizeCenterCrop, evaluate
    m, (u8, y) = setups[0].model, batch
    rcc = ResizeCenterCrop(32, interpolation="bicubic", mean=0.45, std=0.225)
    ge = GraphedEval(m, rcc.batch(u8), y)
    u2 = u8.flip(0).contiguous()
    equal, other = ResizeCenterCrop(*rcc.params()), ResizeCenterCrop(32, 0.95, interpolation="bicubic", mean=0.45, std=0.225)
    assert equal is not rcc and ge._fits_x(equal.batch(u2)) and not ge._fits_x(other.batch(u2))
    got = ge.predict(equal.batch(u2))
    assert torch.equal(ge.X, u2) and torch.equal(got, ge._logits), "replayed: the static input and output hold this call's"
    assert torch.equal(got, evaluate.predict(m, rcc(u2)))
    got = ge.predict(other.batch(u8))
    assert torch.equal(ge.X, u2), "eager: the static input was not touched"
    assert torch.equal(got, evaluate.predict(m, other(u8))) and not torch.equal(got, evaluate.predict(m, rcc(u8)))
    assert m.training
