"""GPU: GraphedTrainStep with the Kohonen head.  The SOM schedule is host state (model.step, get_kohonen_lr); the captured
SOM updates read their rate from device scalars that every call rewrites (nvit_som_update_dev).  Two models from the same
weights, one stepped eagerly and one through the graph, must agree bit for bit at every step - with a schedule under
which every replay needs another rate, so a graph that froze its capture-time rate fails."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

AUX = ("kohonen_consistency", "kohonen_smoothness", "local_quantization", "global_quantization", "reconstruction")
SCHEDULE = dict(kohonen_alpha=0.5, kohonen_scheduler_enabled=True, kohonen_scheduler_warmup_steps=3,
                kohonen_scheduler_decay_steps=7, kohonen_scheduler_min_lr=0.05)


def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m


def _same_step(eager, graphed, what):
    le, losse, auxe, gne = eager
    lg, lossg, auxg, gng = graphed
    assert torch.equal(le, lg), (what, (le - lg).abs().max().item())
    assert torch.equal(losse, lossg), (what, losse.item(), lossg.item())
    assert set(auxe) == set(auxg) == set(AUX), (what, sorted(auxg))
    for k in AUX:
        assert torch.equal(auxe[k], auxg[k]), (what, k, auxe[k].item(), auxg[k].item())
    assert torch.equal(gne, gng), (what, gne.item(), gng.item())


def _same_state(me, mg, oe, og, steps, what):
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), (what, n)
    for km in ("local_kohonen", "global_kohonen"):
        assert torch.equal(getattr(me, km).nodes, getattr(mg, km).nodes), (what, km)
    assert me.step == mg.step == steps, (what, me.step, mg.step)
    assert oe.state_dict()["state"][0]["step"] == og.state_dict()["state"][0]["step"] == steps, what


def _compare(cfg, precision, batch=8, warm=2, steps=6):
    from nvit_amd.train import GraphedTrainStep, train_step
    data = [tuple(t.cuda() for t in synthetic_batch(cfg, batch, seed=s)) for s in (1234, 77, 5)]
    me, mg = build(cfg, precision), build(cfg, precision)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for _ in range(warm):
        train_step(me, oe, *data[0])
    g = GraphedTrainStep(mg, og, *data[0], warmup=warm)
    assert mg.step == warm and all(p.grad is None for p in mg.parameters())
    rates = set()
    for i in range(steps):
        xb, yb = data[i % 3]
        _same_step(train_step(me, oe, xb, yb), g(xb, yb), f"step {warm + 1 + i}")
        rates.add(mg.get_kohonen_lr(mg.step))
    _same_state(me, mg, oe, og, warm + steps, "after the replays")
    # an eager step on the graphed model (the rate by value again), then a replay: still the eager twin
    xb, yb = data[1]
    _same_step(train_step(me, oe, xb, yb), train_step(mg, og, xb, yb), "eager step on the graphed model")
    xb, yb = data[2]
    _same_step(train_step(me, oe, xb, yb), g(xb, yb), "replay after an eager step")
    _same_state(me, mg, oe, og, warm + steps + 2, "after eager step and replay")
    return rates


@pytest.mark.parametrize("name", ["micro_k", "micro_k_fa"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_kohonen_step_equals_eager_under_a_moving_schedule(precision, name):
    cfg = named_config(name, **SCHEDULE)
    rates = _compare(cfg, precision)
    # steps 3..8: the cosine branch (3..7, five different rates) and the floor after it (8, the rate of step 7)
    assert len(rates) == 5 and min(rates) == cfg.kohonen_scheduler_min_lr and max(rates) > 0.99 * cfg.kohonen_alpha


def test_graphed_kohonen_step_equals_eager_constant_rate_head_dim_64():
    """mini_k: head dim 64, T = 49, scheduler off - the constant rate takes the device scalar all the same."""
    cfg = named_config("mini_k")
    assert not cfg.kohonen_scheduler_enabled
    assert _compare(cfg, "bf16") == {cfg.kohonen_alpha}


def _poison_free_memory(nbytes=2 << 30):
    """Fill a large block of free HBM with NaNs and release it, so later torch.empty() buffers start as NaN."""
    t = torch.full((nbytes // 4,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    del t


def test_graphed_kohonen_step_under_nan_poison():
    """Every workspace of the Kohonen step is written before it is read, also in the captured step: with freed memory
    poisoned by NaNs the replays give the losses of a clean eager run."""
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini_k")
    X, y = (t.cuda() for t in synthetic_batch(cfg, 4))
    clean = build(cfg, "bf16")
    oc = clean.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ref = [train_step(clean, oc, X, y)[1].item() for _ in range(4)]
    m = build(cfg, "bf16")
    o = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    _poison_free_memory()
    got = [train_step(m, o, X, y)[1].item()]
    _poison_free_memory()
    g = GraphedTrainStep(m, o, X, y, warmup=1)   # its warm-up step is step 2 (not returned)
    for _ in range(2):
        _poison_free_memory()
        got.append(g(X, y)[1].item())
    assert got == [ref[0], ref[2], ref[3]], (got, ref)
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all(), n
