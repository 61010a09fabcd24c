"""GPU: the device-resident dataset through the train step (nvit_amd/data.py, train.py).  A step on a chain around
`ld.batch()` with y=None equals, bit for bit, the step on the same chain around `images[idx]` with `labels[idx]`, idx from
the numpy twin tests/loader_ref.py: eager, replayed, alternating, accumulated, on the full chain; a replayed run covers an
epoch exactly once with no host work between the replays; a run resumed from `state_dict()` mid-epoch is the uninterrupted
one; the captured step holds the dataset tensor itself and no y; evaluation runs from `ds.eval_batches`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loader_ref as R
from nvit_amd import DeviceDataset

N, B, SEED = 37, 8, 13          # S = 4 steps per epoch, 5 images left out: a handful of steps cross an epoch border
MODELS = [("mini", "fp32"), ("mini", "bf16"), ("micro_k", "bf16")]


def dev():
    return torch.device("cuda:0")


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


def dataset(cfg, side=None, n=N, seed=0):
    """n images of side x side (default: the model's input size); the label of image i is i % classes."""
    side = side or cfg.image_size
    g = np.random.default_rng(seed)
    images = torch.from_numpy(g.integers(0, 256, (n, side, side, cfg.channels), dtype=np.uint8)).to(dev())
    return DeviceDataset(images, (torch.arange(n) % cfg.num_classes).to(dev()))


class Chain:
    """One set of identically seeded stage objects: `aug` alone, or the full mix(erase(ra(rrc(.))))."""

    def __init__(self, cfg, full):
        from nvit_amd.augment import AutoAugment
        from nvit_amd.crop import RandomErasing, RandomResizedCrop
        from nvit_amd.mix import Mixup
        from nvit_amd.randaug import RandAugment
        self.full = full
        if full:
            self.rrc, self.ra = RandomResizedCrop(cfg.image_size, seed=1).to(dev()), RandAugment(seed=2).to(dev())
            self.erase, self.mix = RandomErasing(prob=0.5, seed=3).to(dev()), Mixup(seed=4).to(dev())
        else:
            self.aug = AutoAugment("cifar10", seed=5).to(dev())

    def __call__(self, inner):
        if self.full:
            return self.mix.batch(self.erase.batch(self.ra.batch(self.rrc.batch(inner))))
        return self.aug.batch(inner)

    def counters(self):
        return [s.step for s in ((self.rrc, self.ra, self.erase, self.mix) if self.full else (self.aug,))]


def twin_idx(step, **kw):
    return torch.from_numpy(R.draw(SEED, step, N, B, **kw)).to(dev())


def same_step(a, b, what):
    for i, (u, v) in enumerate(zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))):
        assert torch.equal(u, v), (what, ("logits", "loss", "grad_norm")[i], (u - v).abs().max().item())


def same_state(ma, oa, mb, ob, what):
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), (what, n)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for k in sa:
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k][name], sb[k][name]), (what, k, name)


@pytest.mark.parametrize("full", [False, True], ids=["aug", "full_chain"])
@pytest.mark.parametrize("config,precision", MODELS, ids=lambda v: str(v))
def test_the_loader_step_is_the_step_on_the_gathered_batch(config, precision, full):
    """Three models from the same weights: `me` steps eagerly on chain(ld.batch()), `mg` through a GraphedTrainStep that
    captured its own loader, `mp` eagerly on the same chain around images[idx], labels[idx] with idx from the twin."""
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(config)
    ds = dataset(cfg, side=40 if full else None)
    (me, oe), (mg, og), (mp, op_) = (build(cfg, precision) for _ in range(3))
    ce, cg, cp = (Chain(cfg, full) for _ in range(3))
    le, lg = ds.loader(B, seed=SEED), ds.loader(B, seed=SEED)
    xe, xg = ce(le.batch()), cg(lg.batch())

    def gathered(step):
        idx = twin_idx(step)
        return train_step(mp, op_, cp(ds.images[idx]), ds.labels[idx])

    warm = 2
    for s in range(warm):
        same_step(train_step(me, oe, xe, None), gathered(s), f"eager step {s}")
    graph = GraphedTrainStep(mg, og, xg, None, warmup=warm)
    assert le.step == lg.step == warm and ce.counters() == cg.counters() == cp.counters()   # the capture pass is no step
    for s in range(warm, warm + 4):       # steps 2..5: across the border between epochs 0 and 1
        eager = train_step(me, oe, xe, None)
        same_step(eager, gathered(s), f"eager step {s}")
        same_step(eager, graph(xg, None), f"replayed step {s}")
        assert le.step == lg.step == s + 1 and lg.record.tolist() == list(divmod(s, 4))
    same_state(me, oe, mp, op_, "eager against gathered")
    same_state(me, oe, mg, og, "eager against replayed")
    # eager and replayed steps alternate on one model and one loader
    same_step(train_step(me, oe, xe, None), train_step(mg, og, xg, None), "eager step on the graphed model")
    same_step(train_step(me, oe, xe, None), graph(xg, None), "replay after an eager step")
    same_state(me, oe, mg, og, "after alternating")
    assert le.step == lg.step == warm + 6 and ce.counters() == cg.counters()
    for s in (warm + 4, warm + 5):
        gathered(s)
    same_state(me, oe, mp, op_, "gathered, after alternating")
    # the test can fail: the images of the NEXT step give other logits
    wrong = twin_idx(warm + 7)
    assert not torch.equal(wrong, twin_idx(warm + 6))
    got = train_step(me, oe, xe, None)
    assert not torch.equal(got[0], train_step(mp, op_, cp(ds.images[wrong]), ds.labels[wrong])[0])


@pytest.mark.parametrize("config,precision", [("mini", "bf16"), ("micro_k", "bf16")], ids=lambda v: str(v))
def test_accumulation_slices_the_gathered_batch_and_its_labels(config, precision):
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(config)
    ds = dataset(cfg, side=40)
    (me, oe), (mg, og), (mp, op_) = (build(cfg, precision) for _ in range(3))
    ce, cg, cp = (Chain(cfg, True) for _ in range(3))
    le, lg = ds.loader(B, seed=SEED, repeats=3), ds.loader(B, seed=SEED, repeats=3)
    graph = GraphedTrainStep(mg, og, cg(lg.batch()), None, warmup=1, accumulation_steps=2)
    for s in range(3):
        idx = twin_idx(s, repeats=3)
        assert len(set(idx.tolist())) < B          # repeated augmentation: copies of an image in one batch
        eager = train_step(me, oe, ce(le.batch()), None, accumulation_steps=2)
        assert le.step == s + 1                     # one draw per optimizer step, not one per micro-batch
        same_step(eager, train_step(mp, op_, cp(ds.images[idx]), ds.labels[idx], accumulation_steps=2), f"accumulated step {s}")
        if s >= 1:
            same_step(eager, graph(cg(lg.batch()), None), f"replayed accumulated step {s}")
    same_state(me, oe, mp, op_, "accumulated")
    same_state(me, oe, mg, og, "accumulated, replayed")


def test_replays_cover_every_epoch_exactly_once_with_no_host_work():
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep
    cfg = named_config("micro_k")       # 100 classes: the label of image i is i
    ds = dataset(cfg)
    chain_, ld = Chain(cfg, False), ds.loader(B, seed=SEED)
    S = ld.steps_per_epoch
    model, opt = build(cfg, "bf16")
    xb = chain_(ld.batch())
    step = GraphedTrainStep(model, opt, xb, None, warmup=2)
    ld.load_state_dict({**ld.state_dict(), "step": 0})      # in place: the graph holds the counter's address
    seen, records = [], []
    for _ in range(2 * S + 1):
        step(xb, None)                   # nothing else between the replays
        seen.append(step.targets.clone())
        records.append(ld.record.clone())
    labels = torch.stack(seen).cpu().numpy()
    assert torch.stack(records).tolist() == [list(divmod(s, S)) for s in range(2 * S + 1)] and ld.step == 2 * S + 1 and ld.epoch == 2
    for epoch in (0, 1):
        hist = np.bincount(labels[epoch * S:(epoch + 1) * S].ravel(), minlength=N)
        used = R.perm(np.arange(S * B), N, SEED, epoch)
        assert hist.max() == 1 and hist.sum() == S * B == 32 and set(np.flatnonzero(hist)) == set(used.tolist()), epoch
    assert np.array_equal(labels.reshape(-1), np.concatenate([R.draw(SEED, s, N, B) for s in range(2 * S + 1)]))


def test_a_run_resumed_mid_epoch_is_the_uninterrupted_run():
    from nvit_amd.config import named_config
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    ds = dataset(cfg)
    (ma, oa), (mb, ob) = build(cfg, "bf16"), build(cfg, "bf16")
    ca, cb, la, lb = Chain(cfg, False), Chain(cfg, False), ds.loader(B, seed=SEED), ds.loader(B, seed=SEED)
    whole = [train_step(ma, oa, ca(la.batch()), None) for _ in range(6)]
    for s in range(2):
        same_step(whole[s], train_step(mb, ob, cb(lb.batch()), None), f"step {s}")
    state, aug_state = lb.state_dict(), cb.aug.state_dict()
    assert state["step"] == 2 and lb.epoch == 0           # mid-epoch: S = 4
    lc, cc = ds.loader(B, seed=999), Chain(cfg, False)    # new objects: what a restarted process builds
    lc.load_state_dict(state)
    cc.aug.load_state_dict(aug_state)
    for s in range(2, 6):
        same_step(whole[s], train_step(mb, ob, cc(lc.batch()), None), f"resumed step {s}")
    same_state(ma, oa, mb, ob, "resumed")
    assert lc.state_dict() == la.state_dict() and lc.epoch == 1
    with pytest.raises(ValueError):
        ds.loader(4, seed=SEED).load_state_dict(state)    # another batch size: another sequence


def test_a_replay_copies_nothing_and_other_inputs_are_refused():
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep
    cfg = named_config("micro_k")
    ds, other = dataset(cfg), dataset(cfg, seed=1)
    chain_, ld = Chain(cfg, False), ds.loader(B, seed=SEED)
    model, opt = build(cfg, "bf16")
    xb = chain_(ld.batch())
    step = GraphedTrainStep(model, opt, xb, None, warmup=1)
    # by the code path: the static input is the dataset's own tensor (154 MB are not cloned) and there is no static y
    assert step.X is ds.images and step.X.data_ptr() == ds.images.data_ptr() and step.y is None
    assert step.targets.dtype == torch.int64 and step.targets.shape == (B,)
    step(xb, None)
    step(chain_(ld.batch()), None)       # a new batch object of the captured loader
    assert ld.step == 3
    y = torch.zeros(B, dtype=torch.int64, device=dev())
    for bad, words in ((lambda: step(chain_(ds.loader(B, seed=SEED).batch()), None), "another DeviceDataset loader"),
                       (lambda: step(chain_(other.loader(B, seed=SEED).batch()), None), "another DeviceDataset loader"),
                       (lambda: step(chain_(ds.images[:B]), y), "another dataset tensor"),
                       (lambda: step(other.images, None), "another dataset tensor"),
                       (lambda: step(xb, y), "another dataset tensor")):
        with pytest.raises(ValueError, match=words):
            bad()
    plain = GraphedTrainStep(model, opt, chain_(ds.images[:B].clone()), ds.labels[:B].clone(), warmup=1)
    with pytest.raises(ValueError, match="another DeviceDataset loader"):
        plain(xb, None)                  # a graph captured without one
    assert ld.step == 3


def test_evaluation_runs_from_eval_batches():
    from nvit_amd.config import named_config
    from nvit_amd.crop import ResizeCenterCrop
    from nvit_amd.evaluate import estimate_loss, validate
    from nvit_amd.ops import normalize_images
    cfg = named_config("micro_k")
    model, _ = build(cfg, "bf16")
    ds = dataset(cfg, side=40, n=21)
    rcc = ResizeCenterCrop(cfg.image_size)
    by_hand = [(rcc.batch(ds.images[a:a + 8]), ds.labels[a:a + 8]) for a in (0, 8, 16)]
    assert by_hand[-1][1].shape[0] == 5
    assert validate(model, ds.eval_batches(8, rcc)) == validate(model, by_hand)
    assert estimate_loss(model, ds.eval_batches(8, rcc), 3) == estimate_loss(model, by_hand, 3)
    plain = dataset(cfg, n=21)
    by_hand = [(normalize_images(plain.images[a:a + 8], 0.4, 0.2), plain.labels[a:a + 8]) for a in (0, 8, 16)]
    assert validate(model, plain.eval_batches(8, mean=0.4, std=0.2)) == validate(model, by_hand)
    ld = plain.loader(8)
    from nvit_amd.augment import AutoAugment
    with pytest.raises(TypeError, match="eval_batches"):
        validate(model, [(AutoAugment().to(dev()).batch(ld.batch()), plain.labels[:8])])
    assert ld.step == 0 and model.training
