"""GPU: the on-device RandomResizedCrop + flip (nvit_crop_draw / nvit_crop_apply, nvit_amd/crop.py) against the numpy
restatement tests/crop_ref.py, bit for bit, and the train step on the full input chain
mix.batch(erase.batch(aug.batch(rrc.batch(u8)))) against the step on the tensor that the four stages produce outside it,
bit for bit: eager, replayed, alternating and accumulated.  tests/test_crop_ref.py holds the restatement to Pillow."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crop_ref as R
from crop_ref import golden_cases

RATIO = (3 / 4, 4 / 3)


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("first", [0, 1000])
def test_draw_equals_the_restatement_and_the_counter_advances(first):
    from nvit_amd.crop import RandomResizedCrop, aspect_table
    for (Hs, Ws), kw in (((40, 40), {}), ((24, 40), {"scale": (0.3, 1.0), "hflip": 0.2}), ((256, 256), {"interpolation": "bicubic"}),
                         ((32, 32), {"scale": (1.0, 1.0), "ratio": (2.0, 2.0)}), ((40, 10), {"scale": (0.9, 1.0), "ratio": (2.0, 3.0)}),
                         ((10, 40), {"scale": (0.9, 1.0), "ratio": (0.25, 0.5)})):
        r = RandomResizedCrop(32, seed=2 ** 40 + 17, first_index=first, **kw).to(dev())
        scale, ratio, hflip = kw.get("scale", (0.08, 1.0)), kw.get("ratio", RATIO), kw.get("hflip", 0.5)
        for step in range(3):
            got = r.draw(33, Hs, Ws).cpu().numpy()
            want = R.crop_draw(2 ** 40 + 17, step, first, 33, Hs, Ws, scale, ratio, aspect_table(*ratio), hflip)
            assert np.array_equal(got, want), (Hs, Ws, kw, step, np.argwhere(got != want)[:4])
            assert r.step == step + 1
        assert r.state_dict() == {"seed": 2 ** 40 + 17, "step": 3}


def test_draw_resumes_from_a_state_dict_and_is_invariant_to_the_split():
    from nvit_amd.crop import RandomResizedCrop
    a = RandomResizedCrop(32, seed=21).to(dev())
    a.draw(8, 40, 40)
    a.draw(8, 40, 40)
    b = RandomResizedCrop(32, seed=0).to(dev())
    b.load_state_dict(a.state_dict())
    ta = a.draw(8, 40, 40)
    assert torch.equal(ta, b.draw(8, 40, 40))
    c = RandomResizedCrop(32, seed=21)
    c.load_state_dict({"seed": 21, "step": 2})   # loaded before .to(device)
    assert torch.equal(c.to(dev()).draw(8, 40, 40), ta)
    lo, hi = RandomResizedCrop(32, seed=21).to(dev()), RandomResizedCrop(32, seed=21, first_index=4).to(dev())
    for x in (lo, hi):
        x.load_state_dict({"seed": 21, "step": 2})
    assert torch.equal(torch.cat([lo.draw(4, 40, 40), hi.draw(4, 40, 40)]), ta)
    assert not torch.equal(a.draw(8, 40, 40), ta)


# ------------------------------------------------------------------------------------------------ apply
def boxes_for(Hs, Ws):
    """Whole image, 1x1, a single row, a single column, boxes touching each edge, one in the middle."""
    h2, w2 = max(1, Hs // 2), max(1, Ws // 2)
    return [(0, 0, Hs, Ws), (Hs // 3, Ws // 3, 1, 1), (Hs - 1, 0, 1, Ws), (0, Ws - 1, Hs, 1), (0, 0, h2, w2),
            (Hs - h2, Ws - w2, h2, w2), (0, Ws - w2, Hs, w2), (Hs - h2, 0, h2, Ws), (Hs // 4, Ws // 5, h2, w2)]


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
def test_apply_equals_the_restatement_on_every_specified_shape(interpolation):
    """One launch pair per shape and flip: the images of the batch carry different boxes, the last row is out of range
    (= the whole image)."""
    from nvit_amd.crop import RandomResizedCrop
    g = np.random.default_rng(7)
    for src, size, fixture_boxes, _ in golden_cases():
        Hs, Ws, C = src.shape
        boxes = boxes_for(Hs, Ws) if Hs < 128 else [tuple(fixture_boxes[0]), (0, 0, Hs, Ws), (100, 3, 17, 250)]
        boxes = boxes + [(0, 0, Hs + 1, Ws)]
        u8 = g.integers(0, 256, (len(boxes), Hs, Ws, C), dtype=np.uint8)
        r = RandomResizedCrop(size, interpolation=interpolation).to(dev())
        ud = torch.from_numpy(u8).to(dev())
        for flips in ([0] * len(boxes), [1] * len(boxes), [k % 2 for k in range(len(boxes))]):
            table = r.params_for(boxes, flips)
            got = r.apply(ud, table).cpu().numpy()
            want = R.crop_apply(u8, table.cpu().numpy(), size, interpolation)
            assert got.shape == want.shape == (len(boxes), size, size, C)
            bad = [k for k in range(len(boxes)) if not np.array_equal(got[k], want[k])]
            assert not bad, (src.shape, size, interpolation, flips[:2], [boxes[k] for k in bad])
        whole = r.apply(ud[-1:], r.params_for([(0, 0, Hs, Ws)], [1])).cpu().numpy()
        assert np.array_equal(got[-1:], whole)   # the out-of-range row (flipped in the last table: 9 or 3 is odd)


def test_apply_equals_the_pillow_fixture_and_leaks_nothing_across_the_crop_edge():
    from nvit_amd.crop import RandomResizedCrop
    for interpolation in ("bilinear", "bicubic"):
        for src, size, boxes, want in golden_cases():
            r = RandomResizedCrop(size, interpolation=interpolation).to(dev())
            ud = torch.from_numpy(np.repeat(src[None], len(boxes), axis=0)).to(dev())
            got = r.apply(ud, r.params_for(boxes.tolist())).cpu().numpy()
            assert np.array_equal(got, want[interpolation]), (src.shape, size, interpolation)
        img = np.full((2, 32, 32, 3), 255, np.uint8)
        img[0, :12, :12] = 0
        img[1, 10:22, 10:22] = 0
        r = RandomResizedCrop(16, interpolation=interpolation).to(dev())
        assert not r.apply(torch.from_numpy(img).to(dev()), r.params_for([(0, 0, 12, 12), (10, 10, 12, 12)], [0, 1])).any()


def test_call_is_draw_then_apply_and_other_hand_made_rows_stay_in_bounds():
    from nvit_amd.crop import RandomResizedCrop, aspect_table
    g = np.random.default_rng(3)
    u8 = g.integers(0, 256, (6, 40, 40, 3), dtype=np.uint8)
    ud = torch.from_numpy(u8).to(dev())
    r = RandomResizedCrop(32, interpolation="bicubic", seed=5).to(dev())
    r.load_state_dict({"seed": 5, "step": 4})
    want = R.crop_apply(u8, R.crop_draw(5, 4, 0, 6, 40, 40, (0.08, 1.0), RATIO, aspect_table(*RATIO), 0.5), 32, "bicubic")
    assert np.array_equal(r(ud).cpu().numpy(), want) and r.step == 5
    rows = torch.tensor([[-5, 0, 10, 10, 0, 0, 0, 0], [0, 0, 0, 0, 1, 9, 9, 9], [35, 35, 10, 10, 0, 0, 0, 0],
                         [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0, 0], [0, 0, -2 ** 31, 40, 0, 0, 0, 0],
                         [3, 4, 5, 6, 7, 0, 0, 0]], dtype=torch.int32).to(dev())
    assert np.array_equal(r.apply(ud, rows).cpu().numpy(), R.crop_apply(u8, rows.cpu().numpy(), 32, "bicubic"))


# ------------------------------------------------------------------------------------------------ through the model
def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    from nvit_amd.weights import formula_state_dict
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)   # Kohonen index buffers are not in the formula dict
    assert not res.unexpected_keys and all("kohonen" in k for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m, m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")


def same_step(a, b, what):
    for i, (u, v) in enumerate(zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))):
        assert torch.equal(u, v), (what, ("logits", "loss", "grad_norm")[i], (u - v).abs().max().item())


def same_weights(ma, mb, what):
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), (what, n)


class Chain:
    """The four stages, identically seeded per instance."""

    def __init__(self):
        from nvit_amd.augment import AutoAugment
        from nvit_amd.crop import RandomErasing, RandomResizedCrop
        from nvit_amd.mix import Mixup
        self.rrc = RandomResizedCrop(32, interpolation="bicubic", seed=3).to(dev())
        self.aug = AutoAugment("cifar10", seed=5).to(dev())
        self.erase = RandomErasing(prob=0.75, seed=7).to(dev())
        self.mix = Mixup(seed=6).to(dev())

    def batch(self, u8):
        return self.mix.batch(self.erase.batch(self.aug.batch(self.rrc.batch(u8))))

    def outside(self, u8, y):
        """(X, targets) made by running the four stages outside the step; also the crop table's draw is checked."""
        return self.mix(self.erase(self.aug(self.rrc(u8)), inplace=True), y, inplace=True)

    def steps(self):
        return (self.rrc.step, self.aug.step, self.erase.step, self.mix.step)


def data(cfg, B, seed):
    g = np.random.default_rng(seed)
    u8 = torch.from_numpy(g.integers(0, 256, (B, 40, 40, cfg.channels), dtype=np.uint8)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(dev())
    return u8, y


@pytest.mark.parametrize("config", ["micro", "micro_k"])
def test_train_step_on_the_full_chain_eager_replayed_and_alternating(config):
    """Three models from the same weights: `me` steps eagerly on the chain, `mg` through a GraphedTrainStep that captured
    it, `mp` eagerly on the tensor and targets that a third, identically seeded chain produces outside the step."""
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(config)
    assert cfg.image_size == 32
    B, warm = 8, 2
    u8, y = data(cfg, B, 12)
    u8_0 = u8.clone()
    (me, oe), (mg, og), (mp, op_) = build(cfg, "bf16"), build(cfg, "bf16"), build(cfg, "bf16")
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
        same_step(eager, graph(u8, y), f"graphed step {i}")
        same_step(eager, train_step(mp, op_, xm, tm), f"step {i} on the tensor made outside")
        assert cg.steps() == (warm + i + 1,) * 4
    assert not any(torch.equal(seen[i], seen[j]) for i in range(3) for j in range(i))   # every replay draws afresh
    assert torch.equal(u8, u8_0)
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the steps on the tensor made outside")
    # eager and replayed steps alternate on one model
    same_step(train_step(me, oe, ce.batch(u8), y), train_step(mg, og, cg.batch(u8), y), "eager step on the graphed model")
    same_step(train_step(me, oe, ce.batch(u8), y), graph(cg.batch(u8), y), "replay after an eager step")
    assert ce.steps() == cg.steps() == (warm + 5,) * 4
    same_weights(me, mg, "after eager step and replay")
    assert me.step == mg.step == warm + 5
    with pytest.raises(ValueError):
        graph(ce.batch(u8), y)   # a chain of other objects
    with pytest.raises(ValueError):
        graph(cg.mix.batch(cg.erase.batch(cg.aug.batch(ce.rrc.batch(u8)))), y)   # ... also when only the crop differs


def test_crop_then_erasing_replays_draw_the_boxes_of_their_steps():
    """erase.batch(rrc.batch(u8)): normalised in between by normalize_images' kernel.  The eager twin draws its crop
    table explicitly, so the boxes of every step are in hand: they are the restatement's for that step, differ from step
    to step, and the replay gives the bits of the step on the tensor made from exactly these boxes."""
    from nvit_amd.config import named_config
    from nvit_amd.crop import RandomErasing, RandomResizedCrop, aspect_table
    from nvit_amd.ops import normalize_images
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro")
    u8, y = data(cfg, 8, 4)
    (ma, oa), (mb, ob) = build(cfg, "bf16"), build(cfg, "bf16")
    ra, rb = (RandomResizedCrop(32, seed=9).to(dev()) for _ in range(2))
    ea, eb = (RandomErasing(prob=1.0, mode="const", seed=1).to(dev()) for _ in range(2))

    def twin_step(step):
        table = rb.draw(8, 40, 40)
        assert np.array_equal(table.cpu().numpy(), R.crop_draw(9, step, 0, 8, 40, 40, (0.08, 1.0), RATIO, aspect_table(*RATIO), 0.5))
        X = eb(normalize_images(rb.apply(u8, table), 0.4, 0.25), inplace=True)
        return table, X, train_step(mb, ob, X, y)

    graph = GraphedTrainStep(ma, oa, ea.batch(ra.batch(u8), mean=0.4, std=0.25), y, warmup=1)
    twin_step(0)
    tables, inputs = [], []
    for i in range(2):
        table, X, want = twin_step(1 + i)
        same_step(graph(u8, y), want, f"replay {i}")
        tables.append(table)
        inputs.append(X)
    assert ra.step == ea.step == rb.step == eb.step == 3
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(inputs[0], inputs[1])
    same_weights(ma, mb, "crop -> erasing")
    with pytest.raises(ValueError):
        graph(ea.batch(ra.batch(u8), mean=0.5, std=0.25), y)   # another normalisation than the captured one
    with pytest.raises(ValueError):
        graph(ea.batch(ra.batch(u8), mean=0.4, std=0.5), y)
    same_step(graph(ea.batch(ra.batch(u8), mean=0.4, std=0.25), y), twin_step(3)[2], "replay on the chain itself")


@pytest.mark.parametrize("config", ["micro", "micro_k"])
def test_a_tensor_takes_the_plain_step_eager_and_replayed(config):
    """A tensor X through the chain-resolving entries: the replayed step (whose capture wraps and resolves its input) and
    the eager step agree bit for bit, with and without accumulation, and X is left alone."""
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(config)
    g = np.random.default_rng(3)
    X = torch.from_numpy(g.standard_normal((8, cfg.channels, 32, 32)).astype(np.float32)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (8,))).to(dev())
    X0 = X.clone()
    for n in (1, 2):
        (me, oe), (mg, og) = build(cfg, "bf16"), build(cfg, "bf16")
        train_step(me, oe, X, y, accumulation_steps=n)
        graph = GraphedTrainStep(mg, og, X, y, warmup=1, accumulation_steps=n)
        assert graph.mix is None and graph.erase is None and graph.augment is None and graph.crop is None
        for i in range(2):
            same_step(train_step(me, oe, X, y, accumulation_steps=n), graph(X, y), f"step {i}, accumulation {n}")
        same_weights(me, mg, f"accumulation {n}")
    assert torch.equal(X, X0)


@pytest.mark.parametrize("config", ["micro", "micro_k"])
def test_accumulation_resolves_the_chain_once_for_the_whole_batch(config):
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(config)
    u8, y = data(cfg, 8, 9)
    (ma, oa), (mb, ob), (mg, og) = build(cfg, "bf16"), build(cfg, "bf16"), build(cfg, "bf16")
    ca, cb, cg = Chain(), Chain(), Chain()
    first = train_step(ma, oa, ca.batch(u8), y, accumulation_steps=2)
    same_step(first, train_step(mb, ob, *cb.outside(u8, y), accumulation_steps=2), "accumulated step 0")
    graph = GraphedTrainStep(mg, og, cg.batch(u8), y, warmup=1, accumulation_steps=2)   # its warm-up is step 0
    for i in (1, 2, 3):
        got = train_step(ma, oa, ca.batch(u8), y, accumulation_steps=2)
        assert ca.steps() == (i + 1,) * 4           # one draw per stage for the whole batch, not one per micro-batch
        same_step(got, train_step(mb, ob, *cb.outside(u8, y), accumulation_steps=2), f"accumulated step {i}")
        same_step(got, graph(u8, y), f"accumulated replay {i}")
        assert cg.steps() == (i + 1,) * 4
    same_weights(ma, mb, "accumulated")
    same_weights(ma, mg, "accumulated, replayed")
    assert ma.step == mg.step == 8
