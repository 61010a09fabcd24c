"""GPU: the train step on `ra.batch(u8)` (RandAugment inside the step, eager and captured) against the step on the tensor
that an identically seeded RandAugment builds outside it: logits, loss, gradient norm and the weights afterwards, bit
for bit; and that tensor against the numpy restatement's table and ops, so a replay is known to have drawn the table of
its step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import randaug_ref as R

FILL = (124, 116, 104)
SEED = 31


def dev():
    return torch.device("cuda:0")


def build(cfg, precision="bf16"):
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


def make(seed=SEED, **kw):
    from nvit_amd.randaug import RandAugment
    return RandAugment.from_config("rand-m9-mstd0.5-inc1", fill=FILL, seed=seed, **kw).to(dev())


def data(cfg, B, seed, side=None):
    g = np.random.default_rng(seed)
    side = side or cfg.image_size
    u8 = g.integers(0, 256, (B, side, side, cfg.channels), dtype=np.uint8)
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(dev())
    return u8, torch.from_numpy(u8).to(dev()), y


def twin_input(u8_np, step, seed=SEED):
    """What the stage makes of the batch at `step`, by the restatement: its table, its ops, then the normalise kernel."""
    from nvit_amd import ops
    H, W = u8_np.shape[1:3]
    rows = R.draw(seed, step, 0, u8_np.shape[0], H, W)
    return ops.normalize_images(torch.from_numpy(R.apply_params(u8_np, rows, FILL)).to(dev())), rows


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_eager_replayed_alternating_and_on_the_tensor_made_outside(precision):
    """Three models from the same weights: `me` steps eagerly on ra.batch(u8), `mg` through a GraphedTrainStep that
    captured the stage, `mp` eagerly on the fp32 batch that a third, identically seeded stage makes outside the step."""
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro")
    B, warm = 8, 2
    u8_np, u8, y = data(cfg, B, 8)
    (me, oe), (mg, og), (mp, op_) = build(cfg, precision), build(cfg, precision), build(cfg, precision)
    ae, ag, ap = make(), make(), make()
    for _ in range(warm):
        train_step(me, oe, ae.batch(u8), y)
        train_step(mp, op_, ap(u8), y)
    graph = GraphedTrainStep(mg, og, ag.batch(u8), y, warmup=warm)
    assert ae.step == ag.step == ap.step == warm
    tables = []
    for i in range(3):
        xp = ap(u8)
        xt, rows = twin_input(u8_np, warm + i)
        assert torch.equal(xp, xt), f"step {warm + i}: the stage's output is not the restatement's"
        tables.append(rows)
        eager = train_step(me, oe, ae.batch(u8), y)
        same_step(eager, graph(u8, y), f"replay {i}")
        same_step(eager, train_step(mp, op_, xp, y), f"step {i} on the tensor made outside")
        assert ag.step == warm + i + 1
    assert not any(np.array_equal(tables[i], tables[j]) for i in range(3) for j in range(i))   # every replay draws afresh
    assert all((t[:, :, 0] != 0).any() for t in tables)
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the steps on the tensor made outside")
    # eager and replayed steps alternate on one model
    same_step(train_step(me, oe, ae.batch(u8), y), train_step(mg, og, ag.batch(u8), y), "eager step on the graphed model")
    same_step(train_step(me, oe, ae.batch(u8), y), graph(ag.batch(u8), y), "replay after an eager step")
    assert ae.step == ag.step == warm + 5
    same_weights(me, mg, "after eager step and replay")
    assert me.step == mg.step == warm + 5
    with pytest.raises(ValueError):
        graph(ae.batch(u8), y)   # another stage's batch


def test_accumulation_draws_once_per_step_for_the_whole_batch():
    from nvit_amd.config import named_config
    from nvit_amd.train import train_step
    cfg = named_config("micro")
    u8_np, u8, y = data(cfg, 8, 9)
    (ma, oa), (mb, ob) = build(cfg), build(cfg)
    a, probe = make(seed=2), make(seed=2)
    for i in range(2):   # two steps, two draws
        got = train_step(ma, oa, a.batch(u8), y, accumulation_steps=2)
        assert a.step == i + 1                     # one draw for the whole batch, not one per micro-batch
        xp = probe(u8)
        assert torch.equal(xp, twin_input(u8_np, i, seed=2)[0])
        same_step(got, train_step(mb, ob, xp, y, accumulation_steps=2), f"accumulated step {i}")
    same_weights(ma, mb, "accumulated")
    # prob 0: the step on the uint8 batch is the step on normalize_images(u8)
    from nvit_amd import ops
    off = make(prob=0.0)
    same_step(train_step(ma, oa, off.batch(u8), y), train_step(mb, ob, ops.normalize_images(u8), y), "every layer off")
    same_weights(ma, mb, "every layer off")


class Chain:
    """The four stages, identically seeded per instance."""

    def __init__(self):
        from nvit_amd.crop import RandomErasing, RandomResizedCrop
        from nvit_amd.mix import Mixup
        self.rrc = RandomResizedCrop(32, interpolation="bicubic", seed=3).to(dev())
        self.ra = make(seed=5, interpolation="bicubic")
        self.erase = RandomErasing(prob=0.75, seed=7).to(dev())
        self.mix = Mixup(seed=6).to(dev())

    def batch(self, u8):
        return self.mix.batch(self.erase.batch(self.ra.batch(self.rrc.batch(u8))))

    def outside(self, u8, y):
        return self.mix(self.erase(self.ra(self.rrc(u8)), inplace=True), y, inplace=True)

    def steps(self):
        return (self.rrc.step, self.ra.step, self.erase.step, self.mix.step)


def test_the_full_chain_eager_and_replayed():
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro")
    B, warm = 8, 2
    _, u8, y = data(cfg, B, 12, side=40)
    u8_0 = u8.clone()
    (me, oe), (mg, og), (mp, op_) = build(cfg), build(cfg), build(cfg)
    ce, cg, cp = Chain(), Chain(), Chain()
    for _ in range(warm):
        train_step(me, oe, ce.batch(u8), y)
        train_step(mp, op_, *cp.outside(u8, y))
    graph = GraphedTrainStep(mg, og, cg.batch(u8), y, warmup=warm)
    assert ce.steps() == cg.steps() == cp.steps() == (warm,) * 4
    seen = []
    for i in range(3):
        xm, tm = cp.outside(u8, y)
        seen.append(xm.clone())
        eager = train_step(me, oe, ce.batch(u8), y)
        same_step(eager, graph(u8, y), f"replay {i}")
        same_step(eager, train_step(mp, op_, xm, tm), f"step {i} on the tensor made outside")
        assert cg.steps() == (warm + i + 1,) * 4
    assert not any(torch.equal(seen[i], seen[j]) for i in range(3) for j in range(i))
    assert torch.equal(u8, u8_0)
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the steps on the tensor made outside")
    same_step(train_step(me, oe, ce.batch(u8), y), graph(cg.batch(u8), y), "replay after an eager step")
    same_weights(me, mg, "after eager step and replay")
