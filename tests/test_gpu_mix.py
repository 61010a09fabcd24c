"""GPU: the on-device Mixup / CutMix (nvit_mix_draw / nvit_mix_apply, nvit_amd/mix.py) against the numpy restatement
tests/mix_ref.py, bit for bit; the soft-target loss (nvit_ce_loss_soft) against fp64 torch; and the train step with a
`mix.batch(X)` against the step on the batch mixed outside it, bit for bit, eager, replayed, accumulated and chained
behind the AutoAugment.  tests/test_mix_ref.py pins the quantile table and the restatement on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mix_ref as R


def dev():
    return torch.device("cuda:0")


def qtab(alpha):
    """The fp32 quantile table of an alpha as the product uploads it (None for alpha 0)."""
    from nvit_amd.mix import beta_quantile_table
    return None if alpha == 0 else np.array(beta_quantile_table(alpha), dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("alphas", [(0.8, 1.0), (0.2, 1.0), (0, 1.0), (0.8, 0)], ids=str)
def test_draw_equals_the_restatement(alphas):
    from nvit_amd.mix import Mixup
    q_mix, q_cut = qtab(alphas[0]), qtab(alphas[1])
    modes = set()
    for B in (1, 7, 64):
        y = np.random.default_rng(B).integers(0, 10, B)
        yd = torch.from_numpy(y).to(dev())
        for H, W in ((32, 32), (24, 40)):
            for first in (0, 2 ** 33 + 5):
                for prob in (1.0, 0.5):
                    m = Mixup(alphas[0], alphas[1], prob=prob, seed=11, first_index=first).to(dev())
                    for step in range(4):
                        table, t = m.draw(yd, H, W)
                        wt, wl, wy2 = R.draw(11, step, first, y, H, W, q_mix, q_cut, prob=prob)
                        what = (B, H, W, first, prob, step)
                        assert np.array_equal(table.cpu().numpy(), wt), what
                        assert np.array_equal(t.lam.cpu().numpy().view(np.int32), wl.view(np.int32)), what
                        assert np.array_equal(t.y2.cpu().numpy(), wy2) and torch.equal(t.y, yd), what
                        assert t.smoothing == 0.1
                        modes.update(wt[:, 0].tolist())
                    assert m.step == 4 and m.state_dict() == {"seed": 11, "step": 4}
    assert modes == {0} | ({1} if alphas[0] else set()) | ({2} if alphas[1] else set())


def test_draw_resumes_from_a_state_dict():
    from nvit_amd.mix import Mixup
    y = torch.arange(16).to(dev())
    a = Mixup(seed=21).to(dev())
    a.draw(y, 32, 32)
    a.draw(y, 32, 32)
    b = Mixup(seed=0).to(dev())
    b.load_state_dict(a.state_dict())
    (ta, a_t), (tb, b_t) = a.draw(y, 32, 32), b.draw(y, 32, 32)
    assert torch.equal(ta, tb) and torch.equal(a_t.lam, b_t.lam) and torch.equal(a_t.y2, b_t.y2)
    c = Mixup(seed=21)
    c.load_state_dict({"seed": 21, "step": 2})   # loaded before .to(device)
    assert torch.equal(c.to(dev()).draw(y, 32, 32)[0], ta)
    assert np.array_equal(ta.cpu().numpy(), R.draw(21, 2, 0, np.arange(16), 32, 32, qtab(0.8), qtab(1.0))[0])
    # the same seed does not replay on another step or with another seed
    assert not torch.equal(a.draw(y, 32, 32)[0], ta)


# ------------------------------------------------------------------------------------------------ apply
def pair_cases(H, W):
    return [("mixup", 0.0), ("mixup", 0.3), ("mixup", 1.0),
            ("cutmix", (5, 5, 3, 3)),                # empty
            ("cutmix", (0, H, 0, W)),                # the whole image
            ("cutmix", (0, 5, 4, 12)), ("cutmix", (H - 5, H, 4, 12)), ("cutmix", (3, 9, 0, 5)), ("cutmix", (3, 9, W - 6, W)),
            ("cutmix", (2, 7, 1, 6)), ("cutmix", (2, 7, 2, 7)), ("cutmix", (1, 4, 3, 11)),   # x0, x1 = 1, 2, 3 mod 4
            ("cutmix", (4, 5, 5, 6)),                # one pixel
            None]


@pytest.mark.parametrize("shape", [(7, 3, 32, 32), (4, 1, 24, 40), (2, 3, 224, 224)], ids=lambda s: "x".join(map(str, s)))
def test_apply_equals_the_restatement_out_of_place_and_in_place(shape):
    from nvit_amd.mix import Mixup
    B, C, H, W = shape
    m = Mixup().to(dev())
    x = np.random.default_rng(H + W + B).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).to(dev())
    cases, per = pair_cases(H, W), B // 2
    cases += [None] * (-len(cases) % per)
    for k in range(0, len(cases), per):
        specs = cases[k:k + per]
        table, _ = m.targets_for(list(range(B)), specs, H, W)
        want = R.apply(x, table.cpu().numpy())
        got = m.apply(xd, table)
        assert got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(x)), (specs, "input modified")
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), specs
        buf = xd.clone()
        same = m.apply(buf, table, inplace=True)
        assert same.data_ptr() == buf.data_ptr() and torch.equal(buf, got), (specs, "in place")
        for p, spec in enumerate(specs):
            i, j = p, B - 1 - p
            if spec is None or spec == ("mixup", 1.0) or spec == ("cutmix", (5, 5, 3, 3)):
                assert np.array_equal(want[i], x[i]) and np.array_equal(want[j], x[j]), spec
            if spec == ("cutmix", (0, H, 0, W)) or spec == ("mixup", 0.0):
                assert np.array_equal(want[i], x[j]) and np.array_equal(want[j], x[i]), spec
        if B % 2:
            assert np.array_equal(got[B // 2].cpu().numpy(), x[B // 2])   # the self-paired middle row


def test_call_is_draw_then_apply_and_both_alphas_off_launch_no_image_kernel():
    from nvit_amd.mix import Mixup
    B, C, H, W = 8, 3, 32, 32
    g = np.random.default_rng(4)
    x, y = g.standard_normal((B, C, H, W)).astype(np.float32), g.integers(0, 10, B)
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    m = Mixup(seed=77).to(dev())
    m.load_state_dict({"seed": 77, "step": 6})
    out, t = m(xd, yd)
    wt, wl, wy2 = R.draw(77, 6, 0, y, H, W, qtab(0.8), qtab(1.0))
    assert (wt[:, 0] != 0).all()
    assert np.array_equal(out.cpu().numpy(), R.apply(x, wt)) and np.array_equal(t.y2.cpu().numpy(), wy2)
    off = Mixup(0, 0, label_smoothing=0.1).to(dev())
    out, t = off(xd, yd)
    assert out is xd and off.step == 1
    # y2 is the partner's label also for a pair that is not mixed; at lambda = 1 it carries no weight
    assert torch.equal(t.y2, yd.flip(0)) and (t.lam == 1).all() and t.smoothing == 0.1


# ------------------------------------------------------------------------------------------------ soft loss
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ce_raw(logits, y, y2=None, lam=None, eps=0.0):
    """(rowloss, loss, dlogits) of nvit_ce_loss, or of nvit_ce_loss_soft when y2 is given."""
    from nvit_amd import ops
    B, N = logits.shape
    rowloss = torch.empty(B, device=dev())
    loss = torch.empty(1, device=dev())
    dl = torch.empty_like(logits)
    lib = ops._lib.load()
    if y2 is None:
        ops.check(lib.nvit_ce_loss(ops._p(logits), ops._p(y), ops._p(rowloss), ops._p(loss), ops._p(dl), B, N, ops._s()), "ce")
    else:
        ops.check(lib.nvit_ce_loss_soft(ops._p(logits), ops._p(y), ops._p(y2), ops._p(lam), eps, ops._p(rowloss), ops._p(loss),
                                        ops._p(dl), B, N, ops._s()), "ce_soft")
    return rowloss, loss, dl


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,N", [(3, 7), (8, 10), (33, 100), (128, 1000)])
def test_soft_loss_against_fp64(B, N, eps):
    """nvit_ce_loss_soft against fp64 F.cross_entropy with probability targets and its autograd.  Bars: those of
    test_ce_loss_fwd_bwd (2e-6 relative on the loss, 2e-7 absolute on dlogits), or four times the error that nvit_ce_loss
    itself shows against the fp64 hard-label reference on the same logits, whichever is larger (four extra rounded terms
    per element)."""
    from nvit_amd.mix import MixedTargets
    from nvit_amd.train import CrossEntropyFn
    F = torch.nn.functional
    g = torch.Generator().manual_seed(6)
    logits = rnd(B, N, seed=5, scale=3.0)
    y, y2 = torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1] = 0.0, 1.0
    l64 = logits.double().requires_grad_(True)
    target = torch.from_numpy(R.soft_target(y.numpy(), y2.numpy(), lam.numpy(), eps, N))
    ref = F.cross_entropy(l64, target)
    ref.backward()
    h64 = logits.double().requires_grad_(True)
    href = F.cross_entropy(h64, y)
    href.backward()
    ld = logits.to(dev())
    _, hloss, hdl = ce_raw(ld, y.to(dev()))
    e_hard_loss = abs(hloss.item() - href.item())
    e_hard_dl = (hdl.cpu().double() - h64.grad).abs().max().item()
    lg = logits.to(dev()).requires_grad_(True)
    out = CrossEntropyFn.apply(lg, MixedTargets(y.to(dev()), y2.to(dev()), lam.to(dev()), eps))
    out.backward()
    e_loss = abs(out.item() - ref.item())
    e_dl = (lg.grad.cpu().double() - l64.grad).abs().max().item()
    print(f"soft loss B={B} N={N} eps={eps}: loss err {e_loss:.3e} (hard {e_hard_loss:.3e}), "
          f"dlogits err {e_dl:.3e} (hard {e_hard_dl:.3e})")
    assert e_loss <= max(2e-6 * max(1.0, abs(ref.item())), 4 * e_hard_loss)
    assert e_dl <= max(2e-7, 4 * e_hard_dl)


@pytest.mark.parametrize("B,N", [(3, 7), (8, 10), (33, 100), (128, 1000)])
def test_soft_loss_at_lambda_one_without_smoothing_has_the_bits_of_the_hard_loss(B, N):
    g = torch.Generator().manual_seed(7)
    logits = rnd(B, N, seed=8, scale=3.0).to(dev())
    y, y2 = (torch.randint(0, N, (B,), generator=g).to(dev()) for _ in range(2))
    hard = ce_raw(logits, y)
    soft = ce_raw(logits, y, y2, torch.ones(B, device=dev()), 0.0)
    for h, s, what in zip(hard, soft, ("rowloss", "loss", "dlogits")):
        assert torch.equal(h, s), (what, (h - s).abs().max().item())


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


def batch(cfg, B, seed):
    g = np.random.default_rng(seed)
    X = torch.from_numpy(g.standard_normal((B, cfg.channels, cfg.image_size, cfg.image_size)).astype(np.float32)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(dev())
    return X, y


def same_step(a, b, what):
    for i, (u, v) in enumerate(zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))):
        assert torch.equal(u, v), (what, ("logits", "loss", "grad_norm")[i], (u - v).abs().max().item())


def same_weights(ma, mb, what):
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), (what, n)


def test_gradients_are_linear_in_the_target():
    """lam = 0.3 on every row, no smoothing: every parameter gradient is 0.3 g(y) + 0.7 g(y2) of two hard-label backward
    passes, within the project's fp32-mode gradient bar (2e-4 of the parameter's largest gradient element)."""
    from nvit_amd.config import named_config
    from nvit_amd.mix import MixedTargets
    from nvit_amd.train import total_loss
    cfg = named_config("micro")
    model, _ = build(cfg, "fp32")
    X, y = batch(cfg, 8, 3)
    y2 = torch.from_numpy(np.random.default_rng(4).integers(0, cfg.num_classes, (8,))).to(dev())
    assert not torch.equal(y, y2)
    lam = torch.full((8,), 0.3, device=dev())

    def grads(target):
        model.zero_grad(set_to_none=True)
        logits, aux = model(X)
        total_loss(cfg, logits, aux, target).backward()
        return {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}

    g1, g2, gs = grads(y), grads(y2), grads(MixedTargets(y, y2, lam, 0.0))
    l = float(lam[0].item())
    assert len(gs) == len(g1) > 0
    for n in gs:
        want = l * g1[n] + (1.0 - l) * g2[n]
        err, top = (gs[n] - want).abs().max().item(), want.abs().max().item()
        assert err <= 2e-4 * top, (n, err, top)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_with_mixup_eager_graphed_and_premixed(precision):
    """Three models from the same weights: `me` steps eagerly on mix.batch(X), `mg` through a GraphedTrainStep that
    captured the Mixup, `mp` eagerly on the batch and targets that a third, identically seeded Mixup produces outside the
    step.  All three agree bit for bit at every step; the steps see different mixed batches."""
    from nvit_amd.config import named_config
    from nvit_amd.mix import Mixup
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro")
    B, warm = 8, 2
    X, y = batch(cfg, B, 8)
    X0 = X.clone()
    (me, oe), (mg, og), (mp, op_) = build(cfg, precision), build(cfg, precision), build(cfg, precision)
    xe, xg, xp_ = (Mixup(seed=31).to(dev()) for _ in range(3))
    for _ in range(warm):
        train_step(me, oe, xe.batch(X), y)
        train_step(mp, op_, *xp_(X, y))
    graph = GraphedTrainStep(mg, og, xg.batch(X), y, warmup=warm)
    assert xe.step == xg.step == xp_.step == warm
    seen = []
    for i in range(3):
        xm, tm = xp_(X, y)
        seen.append(xm)
        eager = train_step(me, oe, xe.batch(X), y)
        same_step(eager, graph(X, y), f"graphed step {i}")
        same_step(eager, train_step(mp, op_, xm, tm), f"premixed step {i}")
        assert xg.step == warm + i + 1
    assert not any(torch.equal(seen[i], seen[j]) for i in range(3) for j in range(i))
    assert not any(torch.equal(s, X) for s in seen) and torch.equal(X, X0)   # the caller's batch is never modified
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the premixed steps")
    # eager and graphed steps alternate on one model
    same_step(train_step(me, oe, xe.batch(X), y), train_step(mg, og, xg.batch(X), y), "eager step on the graphed model")
    same_step(train_step(me, oe, xe.batch(X), y), graph(xg.batch(X), y), "replay after an eager step")
    assert xe.step == xg.step == warm + 5
    same_weights(me, mg, "after eager step and replay")
    with pytest.raises(ValueError):
        graph(xe.batch(X), y)   # another Mixup's batch
    plain = GraphedTrainStep(mp, op_, X, y, warmup=1)
    with pytest.raises(ValueError):
        plain(xe.batch(X), y)   # a graph captured without one


def test_accumulation_mixes_the_batch_once_and_smoothing_alone_and_off():
    from nvit_amd.config import named_config
    from nvit_amd.mix import Mixup
    from nvit_amd.train import train_step
    cfg = named_config("micro")
    X, y = batch(cfg, 8, 9)
    (ma, oa), (mb, ob) = build(cfg, "bf16"), build(cfg, "bf16")
    a, probe = Mixup(seed=2).to(dev()), Mixup(seed=2).to(dev())
    for i in range(3):
        got = train_step(ma, oa, a.batch(X), y, accumulation_steps=2)
        assert a.step == i + 1                     # one draw for the whole batch, not one per micro-batch
        same_step(got, train_step(mb, ob, *probe(X, y), accumulation_steps=2), f"accumulated step {i}")
    same_weights(ma, mb, "accumulated")
    # both alphas 0: label smoothing alone, the images untouched
    sm, sm_probe = Mixup(0, 0, label_smoothing=0.1).to(dev()), Mixup(0, 0, label_smoothing=0.1).to(dev())
    smoothed = train_step(ma, oa, sm.batch(X), y)
    same_step(smoothed, train_step(mb, ob, *sm_probe(X, y)), "smoothing alone")
    # ... and without smoothing it is the plain step, bit for bit
    off = Mixup(0, 0, label_smoothing=0.0).to(dev())
    plain = train_step(mb, ob, X, y)
    same_step(train_step(ma, oa, off.batch(X), y), plain, "everything off")
    assert not torch.equal(smoothed[1], plain[1])
    same_weights(ma, mb, "everything off")


def test_chained_behind_the_augmentation_on_the_kohonen_model():
    """mix.batch(aug.batch(u8)) on micro_k, bf16: eager and replayed against the step on the batch augmented and mixed
    outside it."""
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.mix import Mixup
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro_k")
    B, warm = 8, 2
    g = np.random.default_rng(12)
    u8 = torch.from_numpy(g.integers(0, 256, (B, cfg.image_size, cfg.image_size, cfg.channels), dtype=np.uint8)).to(dev())
    y = torch.from_numpy(g.integers(0, cfg.num_classes, (B,))).to(dev())
    (me, oe), (mg, og), (mp, op_) = build(cfg, "bf16"), build(cfg, "bf16"), build(cfg, "bf16")
    ae, ag, ap = (AutoAugment("cifar10", seed=5).to(dev()) for _ in range(3))
    xe, xg, xp_ = (Mixup(seed=6).to(dev()) for _ in range(3))

    def premixed():
        return xp_(ap(u8), y, inplace=True)

    for _ in range(warm):
        train_step(me, oe, xe.batch(ae.batch(u8)), y)
        train_step(mp, op_, *premixed())
    graph = GraphedTrainStep(mg, og, xg.batch(ag.batch(u8)), y, warmup=warm)
    assert ae.step == ag.step == xe.step == xg.step == warm
    for i in range(3):
        eager = train_step(me, oe, xe.batch(ae.batch(u8)), y)
        same_step(eager, graph(u8, y), f"graphed step {i}")
        same_step(eager, train_step(mp, op_, *premixed()), f"premixed step {i}")
    assert ag.step == xg.step == ae.step == xe.step == warm + 3
    same_weights(me, mg, "after the replays")
    same_weights(me, mp, "after the premixed steps")
    assert me.step == mg.step == warm + 3
