"""GPU tests, model level, of running a ViT at another image size than it was built for: ViT.set_dynamic_img_size (the
two position tables resampled inside the forward), ViT.set_input_size (the model changed for good), and the train,
evaluate and checkpoint layers on top.  The main instrument is a twin: model A at its native size, fed size S', against
model B constructed at S' with A's weights and the kernel's own resample of A's position tables - everything behind the
embedding must then agree bit for bit, and A's position gradients must be the kernel's adjoint of B's.  The CPU oracle
(nViT) and the fp64 torch restatement (plain ViT), built at S' with tables resampled by torch in fp64, hold the result
to the bars of tests/test_gpu_droppath.py.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchdrop_ref as pr
import pos_resample_ref as ref
import vit_torch_ref as vref
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

DEV = "cuda:0"
POS = ("local_pos_embed", "global_pos_embed")
BATCH = 4


def grid(cfg):
    return cfg.image_size // cfg.local_patch_size


def build(cfg, precision, renormed=False):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    m.load_state_dict(formula_state_dict(cfg), strict=False)   # (the Kohonen index buffers are not in the formula dict)
    m = m.to(DEV).set_precision(precision)
    if renormed:
        normalize_matrices(m)
    return m


def twin_of(a, S2):
    """model B: constructed at image_size S2, A's weights, position tables = the kernel's resample of A's"""
    from nvit_amd import ops
    from nvit_amd.model import ViT
    cfg_b = named_config_like(a.config, S2)
    g, g2, C = grid(a.config), grid(cfg_b), a.config.n_embd
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    outl, outg = ops.pos_resample_fwd(sd[POS[0]].reshape(g * g, C), sd[POS[1]].reshape(g * g, C), g, g2)
    sd[POS[0]], sd[POS[1]] = outl.reshape(1, g2 * g2, C), outg.reshape(1, g2 * g2, C)
    b = ViT(cfg_b)
    b.load_state_dict(sd)
    return b.to(DEV).set_precision(a.precision)


def named_config_like(cfg, S2):
    import dataclasses
    return dataclasses.replace(cfg, image_size=S2)


def batch_at(cfg, S2, B=BATCH, seed=1234):
    X, y = synthetic_batch(named_config_like(cfg, S2), B, seed=seed)
    return X.to(DEV), y.to(DEV)


def same_weights(a, b, skip=()):
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if n not in skip:
            assert torch.equal(pa, pb), n


# ---------------------------------------------------------------------------------------------- native size: nothing changes
@pytest.mark.parametrize("name,precision", [("mini", "fp32"), ("mini", "bf16"), ("micro_k", "fp32")])
def test_native_size_with_the_flag_on_changes_no_bit(name, precision):
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    X, y = batch_at(cfg, cfg.image_size)
    res = []
    for flag in (False, True):
        m = build(cfg, precision).train().set_dynamic_img_size(flag)
        logits, aux = m(X)
        loss = total_loss(cfg, logits, aux, y)
        loss.backward()
        res.append((m, logits, loss, aux))
    (m0, l0, loss0, aux0), (m1, l1, loss1, aux1) = res
    assert torch.equal(l0, l1) and torch.equal(loss0, loss1) and set(aux0) == set(aux1)
    for k in aux0:
        assert torch.equal(aux0[k], aux1[k]), k
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert (p0.grad is None) == (p1.grad is None), n
        assert p0.grad is None or torch.equal(p0.grad, p1.grad), n
    assert m1._rt.grid is None and m1._rt.tokens is None


# ---------------------------------------------------------------------------------------------- the twin
TWINS = [("mini", 32, "fp32"), ("mini", 32, "bf16"), ("mini", 80, "fp32"), ("mini", 80, "bf16"), ("micro_k", 48, "fp32"),
         ("mini_vit", 80, "fp32"), ("mini_vit", 80, "bf16"), ("micro_fa", 48, "fp32"), ("micro_fa", 48, "bf16"),
         ("hd80", 32, "fp32"), ("hd80", 32, "bf16")]


@pytest.mark.parametrize("name,S2,precision", TWINS)
def test_dynamic_forward_backward_equals_the_model_built_at_that_size(name, S2, precision):
    from nvit_amd import ops
    from nvit_amd.evaluate import predict
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    a = build(cfg, precision).train().set_dynamic_img_size(True)
    b = twin_of(a, S2).train()
    g, g2, C = grid(cfg), grid(b.config), cfg.n_embd
    assert g2 != g and b.n_tokens == g2 * g2 and a.n_tokens == g * g
    X, y = batch_at(cfg, S2)
    la, auxa = a(X)
    lossa = total_loss(cfg, la, auxa, y)
    lossa.backward()
    lb, auxb = b(X)
    lossb = total_loss(b.config, lb, auxb, y)
    lossb.backward()
    assert tuple(la.shape) == (BATCH, cfg.num_classes)
    assert torch.equal(la, lb) and torch.equal(lossa, lossb)
    assert set(auxa) == set(auxb) and "reconstruction" in auxa
    for k in auxa:
        assert torch.equal(auxa[k], auxb[k]), k
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for n in pa:
        if n in POS:
            continue
        assert (pa[n].grad is None) == (pb[n].grad is None), n
        assert pa[n].grad is None or torch.equal(pa[n].grad, pb[n].grad), n
    # gradients land on the native-size parameters: the kernel's adjoint of B's, bit for bit
    wl, wg = ops.pos_resample_bwd(pb[POS[0]].grad.reshape(g2 * g2, C), pb[POS[1]].grad.reshape(g2 * g2, C), g, g2)
    for n, w in zip(POS, (wl, wg)):
        assert tuple(pa[n].grad.shape) == (1, g * g, C) and torch.equal(pa[n].grad.reshape(g * g, C), w), n
        assert pa[n].grad.abs().max().item() > 0
    # the forward-only route (eval, no_grad), with and without the reconstruction head
    assert torch.equal(predict(a, X), predict(b, X))
    a.eval(), b.eval()
    with torch.no_grad():
        ea, eauxa = a(X)
        eb, eauxb = b(X)
    assert torch.equal(ea, eb) and torch.equal(eauxa["reconstruction"], eauxb["reconstruction"])
    assert a._rt.grid is None and a._rt.tokens is None and a.n_tokens == g * g and a.config.image_size == cfg.image_size


def test_drop_path_and_patch_drop_at_another_size_equal_the_twin():
    """both regularisers attached, same seeds on A and B: K comes from the forward's T, the draws and the bits agree"""
    from nvit_amd import DropPath, PatchDropout
    from nvit_amd.train import total_loss
    cfg = named_config("mini")
    a = build(cfg, "bf16").train().set_dynamic_img_size(True)
    b = twin_of(a, 80).train()
    pds = []
    for m in (a, b):
        m.attach_drop_path(DropPath(0.3, seed=4).to(DEV))
        pds.append(PatchDropout(0.5, seed=9).to(DEV))
        m.attach_patch_drop(pds[-1])
    X, y = batch_at(cfg, 80)
    la, auxa = a(X)
    lb, auxb = b(X)
    assert "reconstruction" not in auxa and torch.equal(la, lb)
    total_loss(cfg, la, auxa, y).backward()
    total_loss(cfg, lb, auxb, y).backward()
    same = [n for n, p in a.named_parameters() if n not in POS]
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert all(torch.equal(pa[n].grad, pb[n].grad) for n in same if pa[n].grad is not None)
    assert pds[0].step == pds[1].step == 1 and a._rt.tokens is None and a._rt.grid is None


def test_patch_drop_draws_at_the_forwards_token_count():
    """2 train steps at 80 px (T = 100, K = 50) with the real draw = 2 steps whose tables are the numpy twin's at T = 100"""
    from nvit_amd import PatchDropout
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    T = (80 // cfg.local_patch_size) ** 2
    X, y = batch_at(cfg, 80)
    seed, first = 2 ** 40 + 9, 12
    pd = PatchDropout(0.5, seed=seed, first_index=first).to(DEV)
    K = pd.num_keep(T)
    assert (T, K) == (100, 50)
    twins = [torch.from_numpy(pr.draw(seed, s, first, BATCH, T, K)[0]) for s in range(2)]

    class Fixed(PatchDropout):
        calls = 0

        def draw(self, B, T_):
            keep = twins[Fixed.calls]
            Fixed.calls += 1
            assert (B, T_) == (BATCH, T)
            return keep.to(DEV).contiguous(), pr.slot_of(keep, T).to(DEV).contiguous()

    ma = build(cfg, "fp32").train().set_dynamic_img_size(True).attach_patch_drop(pd)
    mb = build(cfg, "fp32").train().set_dynamic_img_size(True).attach_patch_drop(Fixed(0.5))
    oa = ma.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ob = mb.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for i in range(2):
        la, lossa, _, _ = train_step(ma, oa, X, y)
        lb, lossb, _, _ = train_step(mb, ob, X, y)
        assert torch.equal(la, lb) and torch.equal(lossa, lossb), i
    assert pd.step == 2 and Fixed.calls == 2
    same_weights(ma, mb)


# ---------------------------------------------------------------------------------------------- against the CPU references
def resampled_state(cfg, S2):
    """formula weights of cfg with the two position tables resampled to S2's grid by torch in fp64 (rounded to fp32)"""
    g, g2 = grid(cfg), S2 // cfg.local_patch_size
    sd = formula_state_dict(cfg)
    for n in POS:
        sd[n] = ref.target(sd[n][0].double(), g, g2).float()[None].contiguous()
    return sd


def pulled_back(grad, cfg, S2):
    """fp64 gradient of a resampled table [1, g2*g2, C] -> gradient of the native table, by torch's fp64 autograd"""
    g, g2 = grid(cfg), S2 // cfg.local_patch_size
    p = torch.zeros(g * g, grad.shape[-1], dtype=torch.float64, requires_grad=True)
    ref.target(p, g, g2).backward(grad.double().reshape(g2 * g2, -1))
    return p.grad[None]


@pytest.mark.parametrize("name,S2", [("mini", 80), ("mini", 32), ("micro_k", 48)])
def test_fp32_vs_oracle_built_at_that_size(name, S2):
    from nvit_amd.train import total_loss
    torch.set_num_threads(8)
    cfg = named_config(name)
    cfg2 = named_config_like(cfg, S2)
    X, y = synthetic_batch(cfg2, BATCH)
    p = O.make_params(resampled_state(cfg, S2))
    logits_ref, loss_ref, _ = O.loss_and_grads(p, cfg2, X, y, None, step=1, want_aux=True)
    m = build(cfg, "fp32").train().set_dynamic_img_size(True)
    logits, aux = m(X.to(DEV))
    loss = total_loss(cfg, logits, aux, y.to(DEV))
    loss.backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    worst = 0.0
    checks = []
    for n, q in m.named_parameters():
        assert (q.grad is not None) == (p[n].grad is not None), n
        if q.grad is None:
            continue
        r = pulled_back(p[n].grad, cfg, S2) if n in POS else p[n].grad.double()
        e, s = (q.grad.double().cpu() - r).abs().max().item(), r.abs().max().item()
        worst = max(worst, e / (s + 1e-12))
        checks.append((n, e, s))
    print(f"[fp32 {name} {cfg.image_size}->{S2}] max|dlogit|={err:.3e} loss {loss.item():.6f} vs {loss_ref.item():.6f}; "
          f"worst relative grad error {worst:.3e}")
    assert err < 1e-5
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    for n, e, s in checks:
        assert e <= 2e-4 * s + 1e-8, (n, e, s)


@pytest.mark.parametrize("name,S2", [("mini", 80), ("mini", 32)])
def test_bf16_vs_oracle_built_at_that_size(name, S2):
    from nvit_amd.train import total_loss
    torch.set_num_threads(8)
    cfg = named_config(name)
    cfg2 = named_config_like(cfg, S2)
    X, y = synthetic_batch(cfg2, BATCH)
    p = O.make_params(resampled_state(cfg, S2))
    O.renorm_(p, cfg2)
    logits_ref, _, _ = O.loss_and_grads(p, cfg2, X, y, None, step=1, want_aux=True)
    m = build(cfg, "bf16", renormed=True).train().set_dynamic_img_size(True)
    logits, aux = m(X.to(DEV))
    total_loss(cfg, logits, aux, y.to(DEV)).backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    print(f"[bf16 {name} {cfg.image_size}->{S2}] max|dlogit| vs the fp32 oracle {err:.3e}")
    assert err < 1e-3
    for n, q in m.named_parameters():
        assert q.grad is None or torch.isfinite(q.grad).all(), n


def test_plain_vit_vs_fp64_restatement_built_at_that_size():
    cfg, S2 = named_config("mini_vit"), 80
    cfg2 = named_config_like(cfg, S2)
    X, y = synthetic_batch(cfg2, BATCH)
    ref_logits, _, _, ref_grads = vref.loss_and_grads(resampled_state(cfg, S2), cfg2, X, y)
    m = build(cfg, "fp32").train().set_dynamic_img_size(True)
    logits, _ = m(X.to(DEV))
    torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()
    e, s_ = (logits.detach().double().cpu() - ref_logits).abs().max().item(), ref_logits.abs().max().item()
    worst = 0.0
    checks = []
    for n, q in m.named_parameters():
        if n in ref_grads:
            r = pulled_back(ref_grads[n], cfg, S2) if n in POS else ref_grads[n]
            err = (q.grad.double().cpu() - r).abs().max().item()
            if r.abs().max().item() > 1e-6:   # (the 1e-8 floor of the bar)
                worst = max(worst, err / r.abs().max().item())
            checks.append((n, err, r.abs().max().item()))
        else:
            assert q.grad is None, n
    print(f"[fp32 mini_vit 56->{S2}] max|dlogit| {e:.3e} of {s_:.3f}; worst relative grad error {worst:.3e}")
    assert e <= 1e-5 * s_ + 1e-12
    for n, err, s in checks:
        assert err <= 2e-4 * s + 1e-8, n
    mb = build(cfg, "bf16").train().set_dynamic_img_size(True)
    lb, _ = mb(X.to(DEV))
    eb = (lb.detach().double().cpu() - ref_logits).abs().max().item()
    print(f"[bf16 mini_vit 56->{S2}] max|dlogit| {eb:.3e}")
    assert torch.isfinite(lb).all() and eb < 1e-2


# ---------------------------------------------------------------------------------------------- set_input_size, checkpoints
def test_set_input_size_and_checkpoints(tmp_path):
    from nvit_amd.checkpoint import load_checkpoint, save_checkpoint
    from nvit_amd.evaluate import GraphedEval
    from nvit_amd.train import train_step
    cfg, S2 = named_config("mini"), 80
    a = build(cfg, "bf16", renormed=True).train()
    b = twin_of(a, S2).train()
    old_opt = a.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    save_checkpoint(tmp_path / "native.pt", a, old_opt, 0, {})
    Xn, yn = batch_at(cfg, cfg.image_size)
    stale = GraphedEval(a, Xn, yn)
    old_params = (a.local_pos_embed, a.global_pos_embed)
    assert a.set_input_size(S2) is a
    assert a.config.image_size == S2 and a.n_tokens == 100 and cfg.image_size == 56   # (the caller's config is left alone)
    assert a.local_pos_embed is not old_params[0] and isinstance(a.local_pos_embed, torch.nn.Parameter)
    assert a.local_pos_embed.requires_grad and tuple(old_params[0].shape) == (1, 49, cfg.n_embd)
    sa, sb = a.state_dict(), {k: v.clone() for k, v in b.state_dict().items()}
    assert set(sa) == set(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    with pytest.raises(ValueError, match="set_input_size"):   # graphs captured on the replaced parameters are refused
        stale.predict(Xn)
    with pytest.raises(ValueError):                           # and the model now takes its new size only
        a(Xn)
    # a train step at the new size equals the twin's
    X, y = batch_at(cfg, S2)
    oa = a.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ob = b.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    la, lossa, _, _ = train_step(a, oa, X, y)
    lb, lossb, _, _ = train_step(b, ob, X, y)
    assert torch.equal(la, lb) and torch.equal(lossa, lossb)
    same_weights(a, b)
    # the resized model round-trips through a checkpoint
    save_checkpoint(tmp_path / "resized.pt", a, oa, 1, {})
    factory = lambda mm: mm.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    c, oc, ck = load_checkpoint(tmp_path / "resized.pt", DEV, optimizer_factory=factory)
    assert ck["model_args"]["image_size"] == S2 and c.config.image_size == S2 and c.n_tokens == 100
    same_weights(a, c)
    c = c.set_precision("bf16").train()
    la, _, _, _ = train_step(a, oa, X, y)
    lc, _, _, _ = train_step(c, oc, X, y)
    assert torch.equal(la, lc)
    # load_checkpoint(image_size=) of the old file = a plain load, then set_input_size
    d, od, ckd = load_checkpoint(tmp_path / "native.pt", DEV, image_size=S2)
    e, _, _ = load_checkpoint(tmp_path / "native.pt", DEV)
    assert od is None and ckd["model_args"]["image_size"] == 56 and tuple(ckd["model"][POS[0]].shape) == (1, 49, cfg.n_embd)
    assert e.config.image_size == 56 and d.config.image_size == S2
    e.set_input_size(S2)
    for k, v in d.state_dict().items():
        assert torch.equal(v, e.state_dict()[k]) and torch.equal(v, sb[k]), k   # (sb: the twin before it trained)


# ---------------------------------------------------------------------------------------------- graphs
@pytest.mark.parametrize("name,S2,precision", [("mini", 80, "bf16"), ("micro_k", 48, "fp32")])
def test_graphed_train_step_at_another_size_equals_eager(name, S2, precision):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(name)
    X, y = batch_at(cfg, S2)
    X2, y2 = batch_at(cfg, S2, seed=77)
    me = build(cfg, precision, True).train().set_dynamic_img_size(True)
    mg = build(cfg, precision, True).train().set_dynamic_img_size(True)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    warm = 2
    for _ in range(warm):
        train_step(me, oe, X, y)
    g = GraphedTrainStep(mg, og, X, y, warmup=warm)
    for i, (xb, yb) in enumerate(((X, y), (X2, y2), (X, y))):
        le, losse, auxe, gne = train_step(me, oe, xb, yb)
        lg, lossg, auxg, gng = g(xb, yb)
        assert torch.equal(le, lg) and torch.equal(losse, lossg) and torch.equal(gne, gng), i
        for k in auxe:
            assert torch.equal(auxe[k], auxg[k]), (i, k)
    same_weights(me, mg)
    for n in POS:   # the native-size tables were trained through the captured adjoint
        assert not torch.equal(dict(mg.named_parameters())[n].cpu(), formula_state_dict(cfg)[n]), n
    assert mg.step == me.step == warm + 3 and mg._rt.grid is None
    mg.set_input_size(S2)
    with pytest.raises(ValueError, match="set_input_size"):
        g(X, y)


def test_graphed_eval_at_another_size_equals_validate_and_follows_training():
    from nvit_amd.evaluate import GraphedEval, predict, validate
    from nvit_amd.train import train_step
    cfg, S2 = named_config("mini"), 80
    X, y = batch_at(cfg, S2)
    m = build(cfg, "bf16", True).train().set_dynamic_img_size(True)
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ge = GraphedEval(m, X, y)
    first = ge.validate([(X, y)])
    assert first == validate(m, [(X, y)])
    assert torch.equal(ge.predict(X), predict(m, X))
    assert ge.estimate_loss([(X, y)], 1) == pytest.approx(first["val/loss"], rel=1e-6)
    train_step(m, opt, X, y)
    second = ge.validate([(X, y)])
    assert second == validate(m, [(X, y)]) and second != first
    assert torch.equal(ge.predict(X), predict(m, X))
    assert m.training and m._rt.grid is None


# ---------------------------------------------------------------------------------------------- nothing is left behind
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_forward_at_another_size_leaves_no_state_behind(precision):
    cfg = named_config("mini")
    Xn, _ = batch_at(cfg, cfg.image_size)
    X2, _ = batch_at(cfg, 80)
    fresh = build(cfg, precision).train()
    want, want_aux = fresh(Xn)
    m = build(cfg, precision).train().set_dynamic_img_size(True)
    m(X2)
    assert m._rt.grid is None and m._rt.tokens is None
    got, aux = m(Xn)
    assert torch.equal(got, want) and torch.equal(aux["reconstruction"], want_aux["reconstruction"])
    # a stand-alone block call sees the native token count again
    h = torch.randn(2, m.n_tokens, cfg.n_embd, device=DEV)
    assert tuple(m.transformer.h[0](h).shape) == (2, m.n_tokens, cfg.n_embd)
    # a forward that fails leaves nothing behind either
    m.set_dynamic_img_size(False)
    with pytest.raises(ValueError):
        m(X2)
    assert m._rt.grid is None and m.step == 2
