"""GPU tests, model level, of stochastic depth (ViT.attach_drop_path): a fixed gate table (a DropPath whose `draw` is
overridden) through the whole nViT forward and backward against the CPU oracle run with its `lerp` gated
(droppath_ref.gated_oracle), at the bars test_gpu_model.py holds the ungated model to, and through the plain ViT against
a gated fp64 copy of vit_torch_ref at the bars of test_gpu_vit_baseline.py; then what the feature must not
change (rate 0, eval, GraphedEval), fresh draws per forward that a reloaded state_dict reproduces, and the captured
train step against eager steps bit for bit.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import droppath_ref as dr
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

CASES = [("mini", 4), ("micro_k", 8)]


def build(cfg, precision, renormed=False):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    m.load_state_dict(formula_state_dict(cfg), strict=False)   # (the Kohonen index buffers are not in the formula dict)
    m = m.to("cuda:0").set_precision(precision)
    if renormed:
        normalize_matrices(m)
    return m


def fixed_table(n_layer, B):
    """dropped, kept and kept-and-scaled gates: both patterns inside the batch in every row, sample 0 loses both
    branches of the last block, sample 1 both branches of the first"""
    vals = torch.tensor([0.0, 1.0, 1.25, 1.0])
    t = torch.stack([vals[(torch.arange(B) * 3 + r * 5 + r // 2) % 4] for r in range(2 * n_layer)])
    t[2 * n_layer - 2:, 0] = 0.0
    t[:2, 1] = 0.0
    t[:, 2] = 1.0
    for r in range(2 * n_layer):
        assert (t[r] == 0).any() and (t[r] != 0).any()
    return t.contiguous()


def fixed_drop_path(table):
    from nvit_amd import DropPath

    class Fixed(DropPath):
        calls = 0

        def draw(self, n_layer, B):
            Fixed.calls += 1
            assert tuple(table.shape) == (2 * n_layer, B)
            return table.to("cuda:0")

    return Fixed(0.5), Fixed


def oracle_gated(cfg, X, y, table, renormed=False, lowp=None):
    p = O.make_params(formula_state_dict(cfg))
    if renormed:
        O.renorm_(p, cfg)
    with dr.gated_oracle(p, table):
        logits, loss, _ = O.loss_and_grads(p, cfg, X, y, lowp, step=1, want_aux=True)
    return p, logits, loss


@pytest.mark.parametrize("name,batch", CASES)
def test_fp32_gated_forward_backward_vs_gated_oracle(name, batch):
    from nvit_amd.train import total_loss
    torch.set_num_threads(8)
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, batch)
    table = fixed_table(cfg.n_layer, batch)
    p, logits_ref, loss_ref = oracle_gated(cfg, X, y, table)
    _, logits_plain, _ = oracle_gated(cfg, X, y, torch.ones_like(table))
    assert (logits_ref - logits_plain).abs().max().item() > 1e-3      # the table does change the function
    m = build(cfg, "fp32").train()
    dp, Fixed = fixed_drop_path(table)
    m.attach_drop_path(dp)
    logits, aux = m(X.cuda())
    assert Fixed.calls == 1                                            # one draw per training forward
    loss = total_loss(cfg, logits, aux, y.cuda())
    loss.backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    print(f"[fp32 gated {name}] max|dlogit|={err:.3e} loss {loss.item():.6f} vs {loss_ref.item():.6f}")
    assert err < 1e-5
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    have = {n for n, q in m.named_parameters() if q.grad is not None}
    want = {n for n, t in p.items() if t.grad is not None}
    assert have == want, have ^ want
    worst = 0.0
    for n, q in m.named_parameters():
        if q.grad is None:
            continue
        ref = p[n].grad
        e, s = (q.grad.cpu() - ref).abs().max().item(), ref.abs().max().item()
        worst = max(worst, e / (s + 1e-12))
        assert e <= 2e-4 * s + 1e-8, (n, e, s)
    print(f"   worst relative grad error {worst:.3e}")


@pytest.mark.parametrize("name,batch", CASES)
def test_bf16_gated_forward_vs_gated_oracle(name, batch):
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, batch)
    table = fixed_table(cfg.n_layer, batch)
    p, logits_ref, loss_ref = oracle_gated(cfg, X, y, table, renormed=True)
    m = build(cfg, "bf16", renormed=True).train()
    m.attach_drop_path(fixed_drop_path(table)[0])
    logits, aux = m(X.cuda())
    total_loss(cfg, logits, aux, y.cuda()).backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    print(f"[bf16 gated {name}] max|dlogit| vs the gated fp32 oracle {err:.3e}")
    assert err < 1e-3
    for n, q in m.named_parameters():
        assert q.grad is None or torch.isfinite(q.grad).all(), n


def test_plain_vit_gated_forward_backward_vs_gated_fp64_restatement():
    """mini_vit (use_nvit=False): the gated residual kernels in both directions against droppath_ref's gated copy of
    vit_torch_ref in fp64, at the bars of test_gpu_vit_baseline.py (logits 1e-5 of their largest, gradients 2e-4); bf16
    logits at that file's 1e-2."""
    cfg = named_config("mini_vit")
    batch = 4
    X, y = synthetic_batch(cfg, batch)
    sd = formula_state_dict(cfg)
    table = fixed_table(cfg.n_layer, batch)
    ref_logits, _, ref_grads = dr.gated_vit_loss_and_grads(sd, cfg, X, y, table)
    plain_logits, _, _ = dr.gated_vit_loss_and_grads(sd, cfg, X, y, torch.ones_like(table))
    assert (ref_logits - plain_logits).abs().max().item() > 1e-3
    m = build(cfg, "fp32").train()
    dp, Fixed = fixed_drop_path(table)
    m.attach_drop_path(dp)
    assert dp.scale_by_keep is True
    logits, _ = m(X.cuda())
    assert Fixed.calls == 1
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    e, s_ = (logits.detach().double().cpu() - ref_logits).abs().max().item(), ref_logits.abs().max().item()
    print(f"[fp32 gated mini_vit] max|dlogit| {e:.3e} of {s_:.3f}")
    assert e <= 1e-5 * s_ + 1e-12
    worst = 0.0
    for n, p in m.named_parameters():
        if n in ref_grads:
            r = ref_grads[n]
            err = (p.grad.double().cpu() - r).abs().max().item()
            worst = max(worst, err / (r.abs().max().item() + 1e-30))
            assert err <= 2e-4 * r.abs().max().item() + 1e-8, n
        else:
            assert p.grad is None, n
    print(f"   worst relative grad error {worst:.3e}")
    mb = build(cfg, "bf16").train()
    mb.attach_drop_path(fixed_drop_path(table)[0])
    lb, _ = mb(X.cuda())
    torch.nn.functional.cross_entropy(lb, y.cuda()).backward()
    eb = (lb.detach().double().cpu() - ref_logits).abs().max().item()
    print(f"[bf16 gated mini_vit] max|dlogit| {eb:.3e}")
    assert torch.isfinite(lb).all() and eb < 1e-2
    for n, p in mb.named_parameters():
        assert (p.grad is not None) == (n in ref_grads) and (p.grad is None or torch.isfinite(p.grad).all()), n


def test_plain_vit_graphed_step_with_drop_path_equals_eager():
    from nvit_amd import DropPath
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro_vit")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    me, mg = build(cfg, "bf16").train(), build(cfg, "bf16").train()
    de, dg = DropPath(0.3, seed=4).to("cuda:0"), DropPath(0.3, seed=4).to("cuda:0")
    me.attach_drop_path(de)
    mg.attach_drop_path(dg)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for _ in range(2):
        train_step(me, oe, X, y)
    g = GraphedTrainStep(mg, og, X, y, warmup=2)
    for _ in range(4):
        le, losse, _, _ = train_step(me, oe, X, y)
        lg, lossg, _, _ = g(X, y)
        assert torch.equal(le, lg) and torch.equal(losse, lossg)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
    assert de.step == dg.step == 6


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_inactive_drop_path_changes_no_bit(precision):
    """rate 0 attached, eval() with a live rate, predict and GraphedEval: the logits of a model with nothing attached,
    bit for bit, and no draw (the counter stays where it was)."""
    from nvit_amd import DropPath
    from nvit_amd.evaluate import GraphedEval, predict
    cfg = named_config("micro_k")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    plain = build(cfg, precision).train()
    want_train, _ = plain(X)
    plain.eval()
    with torch.no_grad():
        want_eval, _ = plain(X)
    m = build(cfg, precision).train()
    zero = DropPath(0.0).to("cuda:0")
    m.attach_drop_path(zero)
    got, _ = m(X)
    assert torch.equal(got, want_train) and zero.step == 0
    live = DropPath(0.5).to("cuda:0")
    m.attach_drop_path(live)
    m.eval()
    with torch.no_grad():
        got, _ = m(X)
    assert torch.equal(got, want_eval)
    assert torch.equal(predict(m, X), want_eval)
    ge = GraphedEval(m, X, y)
    assert torch.equal(ge.predict(X), want_eval)
    assert live.step == 0
    m.train()
    got, _ = m(X)
    assert live.step == 1 and not torch.equal(got, want_train)


def test_draws_differ_per_forward_and_resume_from_state_dict():
    from nvit_amd import DropPath
    cfg = named_config("mini")
    X, _ = synthetic_batch(cfg, 4)
    X = X.cuda()
    m = build(cfg, "fp32").train()
    dp = DropPath(0.5, seed=3).to("cuda:0")
    m.attach_drop_path(dp)
    dp.load_state_dict({"seed": 3, "step": 5})
    state = dp.state_dict()
    a1, _ = m(X)
    a2, _ = m(X)
    assert not torch.equal(a1, a2) and dp.step == 7
    dp.load_state_dict(state)
    b1, _ = m(X)
    b2, _ = m(X)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    # the gates the model used are the numpy twin's: block 1 of 2 drops with p = 0.5, unscaled for nViT
    table = torch.from_numpy(dr.draw(3, 5, 0, 0.5, cfg.n_layer, 4, False))
    assert (table == 0).any()
    fixed = build(cfg, "fp32").train()
    fixed.attach_drop_path(_fixed(table))
    c1, _ = fixed(X)
    assert torch.equal(a1, c1)


def _fixed(table):
    from nvit_amd import DropPath

    class Fixed(DropPath):
        def draw(self, n_layer, B):
            return table.to("cuda:0")

    return Fixed(0.5)


@pytest.mark.parametrize("accum", [1, 2])
def test_graphed_train_step_with_drop_path_equals_eager(accum):
    """4 replays of the captured step = 4 eager steps from the same state: weights, SOM nodes and the drop-path counter
    bit for bit; the counter advances by accumulation_steps per step; another DropPath at replay is refused."""
    from nvit_amd import DropPath
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro_k")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    X2, y2 = synthetic_batch(cfg, 8, seed=77)
    X2, y2 = X2.cuda(), y2.cuda()
    me, mg = build(cfg, "bf16", True).train(), build(cfg, "bf16", True).train()
    de, dg = DropPath(0.2, seed=11).to("cuda:0"), DropPath(0.2, seed=11).to("cuda:0")
    me.attach_drop_path(de)
    mg.attach_drop_path(dg)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    warm = 2
    for _ in range(warm):
        train_step(me, oe, X, y, accumulation_steps=accum)
    g = GraphedTrainStep(mg, og, X, y, warmup=warm, accumulation_steps=accum)
    assert de.step == dg.step == warm * accum                           # the capture pass itself drew nothing
    for (xb, yb) in ((X, y), (X2, y2), (X, y), (X2, y2)):
        le, losse, _, _ = train_step(me, oe, xb, yb, accumulation_steps=accum)
        lg, lossg, _, _ = g(xb, yb)
        assert torch.equal(le, lg) and torch.equal(losse, lossg)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
    assert torch.equal(me.local_kohonen.nodes, mg.local_kohonen.nodes)
    assert torch.equal(me.global_kohonen.nodes, mg.global_kohonen.nodes)
    assert de.step == dg.step == (warm + 4) * accum
    if accum == 2:
        assert dg.step - warm * accum == 8
    mg.attach_drop_path(DropPath(0.2, seed=11).to("cuda:0"))
    with pytest.raises(ValueError):
        g(X, y)
    mg.attach_drop_path(None)
    with pytest.raises(ValueError):
        g(X, y)
    mg.attach_drop_path(dg)
    g(X, y)
