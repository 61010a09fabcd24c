"""GPU: gradient accumulation in the train step (`accumulation_steps`, the reference's
`training.gradient_accumulation_steps`, train.py:898-928).

The accumulated step is N training forwards on the N micro-batches, each followed by total_loss / N and backward, then
ONE fused optimizer step.  Every kernel involved is fixed-order and atomic-free, so the step must equal that sequence
written out by hand bit for bit - eagerly and as one replayed hipGraph - and, in fp32 mode, follow the CPU oracle
running the reference's loop at the bars the single step is held to."""
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

# the SOM rate moves at every model.step of the test (linear warm-up, then the cosine branch): a micro-step that took
# the rate of another one cannot pass
SCHEDULE = dict(kohonen_alpha=0.5, kohonen_scheduler_enabled=True, kohonen_scheduler_warmup_steps=3,
                kohonen_scheduler_decay_steps=40, kohonen_scheduler_min_lr=0.05)
CASES = [("mini", 2, 2), ("mini", 3, 2), ("micro_k", 2, 4)]     # name, N, rows per micro-batch
GRAPH_CASES = [("mini", 3, 2), ("micro_k", 2, 4)]


def config(name):
    return named_config(name, **SCHEDULE) if name.endswith("_k") else named_config(name)


def build(cfg, precision, renormed=True):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    if renormed:
        normalize_matrices(m)
    return m


def optimizer(m, lr=1e-3):
    return m.configure_optimizers(0.1, lr, (0.9, 0.95), "cuda")


def batches(cfg, rows, seeds=(1234, 77, 5, 901)):
    return [tuple(t.cuda() for t in synthetic_batch(cfg, rows, seed=s)) for s in seeds]


def hand_loop(m, opt, X, y, N, grad_clip=1.0):
    """The accumulated step written out: what a user had to hand-roll before `accumulation_steps` existed."""
    from nvit_amd.train import total_loss
    b = X.shape[0] // N
    logits, loss, aux = [], None, None
    for i in range(N):
        lg, ax = m(X[i * b:(i + 1) * b])
        li = total_loss(m.config, lg, ax, y[i * b:(i + 1) * b]) / N
        li.backward()
        logits.append(lg.detach())
        loss = li.detach() if loss is None else loss + li.detach()
        aux = {k: v.detach() / N for k, v in ax.items()} if aux is None else \
            {k: aux[k] + ax[k].detach() / N for k in aux}
    gnorm = opt.step_fused(m, grad_clip)[0].clone()
    opt.zero_grad(set_to_none=True)
    return torch.cat(logits), loss, aux, gnorm


def same_step(a, b, what):
    la, lossa, auxa, gna = a
    lb, lossb, auxb, gnb = b
    assert la.shape == lb.shape and torch.equal(la, lb), (what, "logits")
    assert torch.equal(lossa, lossb), (what, lossa.item(), lossb.item())
    assert set(auxa) == set(auxb) and auxa, (what, sorted(auxa), sorted(auxb))
    for k in auxa:
        assert torch.equal(auxa[k], auxb[k]), (what, k, auxa[k].item(), auxb[k].item())
    assert torch.equal(gna, gnb), (what, gna.item(), gnb.item())


def same_state(ma, mb, oa, ob, model_steps, opt_steps, what):
    n_state = 0
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):   # the SOM nodes are parameters too
        assert torch.equal(pa, pb), (what, n)
        if pa in oa.state:
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[pa][k], ob.state[pb][k]), (what, n, k)
            n_state += 1
    assert n_state > 10, n_state
    if ma.config.use_kohonen:
        for km in ("local_kohonen", "global_kohonen"):
            assert torch.equal(getattr(ma, km).nodes, getattr(mb, km).nodes), (what, km)
    assert ma.step == mb.step == model_steps, (what, ma.step, mb.step)
    assert oa.state_dict()["state"][0]["step"] == ob.state_dict()["state"][0]["step"] == opt_steps, what


@pytest.mark.parametrize("name,N,b", CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_accumulated_step_equals_the_hand_written_loop(precision, name, N, b):
    from nvit_amd.train import train_step
    cfg = config(name)
    data = batches(cfg, N * b)[:2]
    ma, mb = build(cfg, precision), build(cfg, precision)
    oa, ob = optimizer(ma), optimizer(mb)
    for k, (X, y) in enumerate(data):
        got = train_step(ma, oa, X, y, 1.0, accumulation_steps=N)
        assert got[0].shape == (N * b, cfg.num_classes) and all(p.grad is None for p in ma.parameters())
        same_step(got, hand_loop(mb, ob, X, y, N), f"step {k}")
    same_state(ma, mb, oa, ob, 2 * N, 2, "after two accumulated steps")
    if cfg.use_kohonen:
        assert len({ma.get_kohonen_lr(s) for s in range(1, 2 * N + 1)}) == 2 * N


def test_one_accumulation_step_is_the_plain_step():
    from nvit_amd.train import train_step
    cfg = config("micro_k")
    ma, mb = build(cfg, "bf16"), build(cfg, "bf16")
    oa, ob = optimizer(ma), optimizer(mb)
    for k, (X, y) in enumerate(batches(cfg, 4)[:2]):
        same_step(train_step(ma, oa, X, y, accumulation_steps=1), train_step(mb, ob, X, y), f"step {k}")
    same_state(ma, mb, oa, ob, 2, 2, "N = 1")


def test_accumulated_step_follows_the_reference_loop_on_the_oracle():
    """fp32 mode, mini, N = 2, b = 2 against the CPU oracle running the reference's loop body.  Bars: the gradient norm
    to 2e-4 relative (the bar of test_fp32_matches_reference_golden_and_one_step for the same quantity), the logits of a
    forward after the step to 2e-4 (the fp32 bar of test_training_trajectory_vs_oracle)."""
    from nvit_amd.train import train_step
    torch.set_num_threads(8)
    cfg, N, b = named_config("mini"), 2, 2
    lr, wd = 3e-3, 0.1
    X, y = synthetic_batch(cfg, N * b, seed=100)
    p = O.make_params(formula_state_dict(cfg))
    o_opt = O.make_optimizer(p, lr=lr, weight_decay=wd)
    for i in range(N):
        lg, ax = O.forward(p, cfg, X[i * b:(i + 1) * b], step=i + 1)
        (O.total_loss(cfg, lg, ax, y[i * b:(i + 1) * b]) / N).backward()     # gradients are not cleared in between
    gn_o = torch.nn.utils.clip_grad_norm_([t for t in p.values() if t.grad is not None], 1.0)
    o_opt.step()
    o_opt.zero_grad(set_to_none=True)
    O.renorm_(p, cfg)
    with torch.no_grad():
        after_o, _ = O.forward(p, cfg, X, step=N + 1)

    m = build(cfg, "fp32", renormed=False)
    opt = m.configure_optimizers(wd, lr, (0.9, 0.95), "cuda")
    _, _, _, gn = train_step(m, opt, X.cuda(), y.cuda(), 1.0, accumulation_steps=N)
    with torch.no_grad():
        after, _ = m(X.cuda())
    e_gn = abs(gn.item() - gn_o.item()) / gn_o.item()
    e_lg = (after.cpu() - after_o).abs().max().item()
    print(f"[accumulation vs oracle] gnorm {gn.item():.6f} vs {gn_o.item():.6f} (rel {e_gn:.2e}); "
          f"max|dlogit| after the step {e_lg:.2e}")
    assert gn_o.item() > 1.0          # the clipping is active
    assert e_gn < 2e-4, e_gn
    assert e_lg < 2e-4, e_lg


@pytest.mark.parametrize("name,N,b", GRAPH_CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_accumulated_step_equals_eager(precision, name, N, b):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = config(name)
    data = batches(cfg, N * b)
    me, mg = build(cfg, precision), build(cfg, precision)
    oe, og = optimizer(me), optimizer(mg)
    train_step(me, oe, *data[0], accumulation_steps=N)
    g = GraphedTrainStep(mg, og, *data[0], warmup=1, accumulation_steps=N)
    assert mg.step == N and all(p.grad is None for p in mg.parameters())
    calls = 0
    for k in (1, 2):
        same_step(train_step(me, oe, *data[k], accumulation_steps=N), g(*data[k]), f"replay {k}")
        calls += 1
    assert all(p.grad is None for p in mg.parameters())
    # one eager accumulated step on the graphed model between two replays
    same_step(train_step(me, oe, *data[3], accumulation_steps=N), train_step(mg, og, *data[3], accumulation_steps=N),
              "eager step on the graphed model")
    same_step(train_step(me, oe, *data[0], accumulation_steps=N), g(*data[0]), "replay after an eager step")
    same_state(me, mg, oe, og, 5 * N, 5, "after three replays and an eager step")


class _CountingWrapper:
    """The least a data-parallel wrapper is to the train step: .module, __call__ and no_sync()."""

    def __init__(self, module):
        self.module, self.entered, self.inside, self.forwards_inside = module, 0, False, 0

    def __call__(self, *a, **k):
        self.forwards_inside += int(self.inside)
        return self.module(*a, **k)

    @contextmanager
    def no_sync(self):
        self.entered += 1
        self.inside = True
        try:
            yield
        finally:
            self.inside = False


def test_no_sync_and_sync_grads_call_counts():
    from nvit_amd.train import train_step
    cfg, N, b = named_config("mini"), 3, 2
    X, y = batches(cfg, N * b)[0]
    m = build(cfg, "bf16")
    w = _CountingWrapper(m)
    synced = []

    def sync_grads():
        assert not w.inside and m.transformer.h[0].query.weight.grad is not None
        synced.append(m.step)

    logits, _, _, gnorm = train_step(w, optimizer(m), X, y, 1.0, sync_grads, accumulation_steps=N)
    assert w.entered == N - 1 == w.forwards_inside
    assert synced == [N]            # once, after the last backward (all N forwards have run)
    assert logits.shape[0] == N * b and torch.isfinite(gnorm)
