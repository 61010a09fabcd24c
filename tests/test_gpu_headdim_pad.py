"""GPU: the model at head dims 72, 80, 88 and 104 (the "padded" attention route: head tensors zero-padded to the 128-wide
attention kernels).  fp32 mode against numbers recorded from the reference itself (tests/golden/hd*_b*.npz,
tools/make_golden_headdim.py) with the bars of tests/test_gpu_wide.py; bf16 mode no farther from the reference's fp32
logits than the reference's own bf16-autocast path; the forward under no_grad bit for bit the grad-enabled one; graph
replay bit for bit the eager steps; every bf16 parameter gradient of `hd80` against a float64 run of the CPU oracle."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nvit_oracle as O

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("hd80", 4), ("hd72", 2), ("hd80_k", 2), ("hd104_b", 2), ("hd88_vit", 2)]


def build(cfg, precision, renormed=True):
    from nvit_amd.model import PADDED_HEAD_DIMS, ViT
    from nvit_amd.train import normalize_matrices
    assert cfg.n_embd // cfg.n_head in PADDED_HEAD_DIMS
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)   # Kohonen index buffers are not in the formula dict
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision)
    if renormed and cfg.use_nvit:
        normalize_matrices(m)
    return m


def _assert_unit_norms(m):
    for blk in m.transformer.h:
        for n in ("att_c_proj", "mlp_c_proj"):
            assert (getattr(blk, n).weight.detach().double().norm(dim=0) - 1).abs().max().item() < 1e-5, n
        for n in ("query", "key", "value", "c_fc"):
            assert (getattr(blk, n).weight.detach().double().norm(dim=1) - 1).abs().max().item() < 1e-5, n


@pytest.mark.parametrize("name,batch", CASES)
def test_fp32_matches_reference_golden(name, batch):
    """The body and bars of test_fp32_wide_matches_reference_golden: logits 1e-5 (2e-5 with the Kohonen head), loss, aux
    losses, per-parameter gradient norms (5e-4 relative) and leading slices, the clipped global norm (2e-4), and after
    one full step (clip + AdamW, + renorm for nViT) the step-1 logits (2e-4), leading weights (2e-6) and unit row /
    column norms (the plain-ViT record has no renormalised weights)."""
    from nvit_amd.train import total_loss
    g = np.load(os.path.join(GOLD, f"{name}_b{batch}.npz"))
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, batch)
    m = build(cfg, "fp32").train()
    assert m._attn_impl() == 0
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    logits, aux = m(X.cuda())
    loss = total_loss(cfg, logits, aux, y.cuda())
    loss.backward()
    tol = 2e-5 if cfg.use_kohonen else 1e-5
    e = np.abs(logits.detach().cpu().numpy() - g["logits"]).max()
    print(f"[golden {name} B={batch}] fp32 mode vs the reference: max|dlogit| {e:.3e} (|logit|max {np.abs(g['logits']).max():.3f}), "
          f"loss {loss.item():.6f} vs {float(g['loss']):.6f}")
    assert e < tol
    assert abs(loss.item() - float(g["loss"])) < 2e-5 * max(1.0, float(g["loss"]))
    assert abs(aux["reconstruction"].item() - float(g["recon"])) < 2e-5
    if cfg.use_kohonen:
        got = np.array([aux[k].item() for k in ("kohonen_consistency", "kohonen_smoothness", "local_quantization",
                                                 "global_quantization")])
        assert np.abs(got - g["aux"]).max() < 2e-5 * max(1.0, np.abs(g["aux"]).max())
        assert np.abs(m.local_kohonen.nodes.detach().reshape(-1)[:8].cpu().numpy() - g["lnodes_head"]).max() < 5e-6
        assert np.abs(m.global_kohonen.nodes.detach().reshape(-1)[:8].cpu().numpy() - g["gnodes_head"]).max() < 5e-6
    names = [str(n) for n in g["grad_names"]]
    params = dict(m.named_parameters())
    assert {n for n, q in params.items() if q.grad is not None} == set(names)
    worst = 0.0
    for n, gn, gh in zip(names, g["grad_norms"], g["grad_heads"]):
        grad = params[n].grad
        mine = grad.double().norm().item()
        worst = max(worst, abs(mine / gn - 1) if gn > 1e-9 else 0.0)
        assert abs(mine - gn) <= 5e-4 * gn + 1e-7, (n, mine, gn)
        head = grad.reshape(-1)[:8].cpu().numpy() if grad.numel() >= 8 else np.resize(grad.reshape(-1).cpu().numpy(), 8)
        assert np.abs(head - gh).max() <= 1e-3 * max(np.abs(gh).max(), 1e-30) + 1e-6 * gn, n
    print(f"   worst relative gradient-norm error vs the reference {worst:.3e}")
    gnorm = opt.step_fused(m, 1.0)[0].item()
    opt.zero_grad(set_to_none=True)
    print(f"   clipped norm {gnorm:.6f} vs {float(g['gnorm']):.6f}")
    assert abs(gnorm - float(g["gnorm"])) < 2e-4 * float(g["gnorm"])
    with torch.no_grad():
        logits1, aux1 = m(X.cuda())
    e1 = np.abs(logits1.cpu().numpy() - g["logits1"]).max()
    print(f"   step-1 max|dlogit| {e1:.3e}")
    assert e1 < 2e-4
    if cfg.use_nvit:
        q0 = m.transformer.h[0].query.weight.detach().reshape(-1)[:8].cpu().numpy()
        assert np.abs(q0 - g["q0_head1"]).max() < 2e-6
        pl = m.transformer.h[-1].mlp_c_proj.weight.detach().reshape(-1)[:8].cpu().numpy()
        assert np.abs(pl - g["p_last_head1"]).max() < 2e-6
        _assert_unit_norms(m)


@pytest.mark.parametrize("name,batch", CASES)
def test_bf16_deviation_bounded_by_the_references_own_bf16_path(name, batch):
    """The HIP bf16 mode (MFMA attention at 128 on the padded heads) must be no farther from the reference's fp32 logits
    than the reference's own `torch.autocast("cpu", bfloat16)` path is, in max and in rms."""
    g = np.load(os.path.join(GOLD, f"{name}_b{batch}.npz"))
    cfg = named_config(name)
    X, _ = synthetic_batch(cfg, batch)
    if cfg.use_nvit:
        ref32, refbf = g["logits_fp32"], g["logits_autocast_bf16"]
        assert abs(float(g["max_abs_dev"]) - np.abs(refbf - ref32).max()) < 1e-9
    else:
        ref32, refbf = g["logits"], g["logits_autocast"]
    m = build(cfg, "bf16").train()
    assert m._attn_impl() == 1
    with torch.no_grad():
        lb, _ = m(X.cuda())
    lb = lb.float().cpu().numpy()
    rms = lambda a: float(np.sqrt(np.mean(np.square(a.astype(np.float64)))))
    hip_dev, ref_dev = np.abs(lb - ref32).max(), np.abs(refbf - ref32).max()
    hip_rms, ref_rms = rms(lb - ref32), rms(refbf - ref32)
    print(f"[autocast {name} B={batch}] |HIP_bf16 - ref_fp32| max {hip_dev:.3e} rms {hip_rms:.3e};  |ref_autocast_bf16 - ref_fp32| "
          f"max {ref_dev:.3e} rms {ref_rms:.3e};  |logit|max {np.abs(ref32).max():.3f}")
    assert hip_dev <= ref_dev, (hip_dev, ref_dev)
    assert hip_rms <= ref_rms, (hip_rms, ref_rms)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name,batch", CASES)
def test_no_grad_forward_is_the_grad_enabled_forward_bit_for_bit(name, batch, precision):
    cfg = named_config(name)
    m = build(cfg, precision).eval()
    X = synthetic_batch(cfg, batch)[0].cuda()
    logits, aux = m(X)
    assert logits.requires_grad
    with torch.no_grad():
        l0, a0 = m(X)
    assert not l0.requires_grad and torch.equal(l0, logits)
    assert set(a0) == set(aux) and "reconstruction" in a0
    for k in aux:
        assert torch.equal(a0[k], aux[k]), k
    assert m._rt.carry is None


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["hd80", "hd80_k"])
def test_graphed_train_step_equals_eager(name, precision):
    """Three replays of the captured step leave the weights (and SOM nodes) of three eager steps, bit for bit."""
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(name)
    data = [tuple(t.cuda() for t in synthetic_batch(cfg, 4, seed=s)) for s in (1234, 77, 5)]
    me, mg = build(cfg, precision).train(), build(cfg, precision).train()
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    train_step(me, oe, *data[0])
    g = GraphedTrainStep(mg, og, *data[0], warmup=1)
    for xb, yb in data:
        le, losse, _, gne = train_step(me, oe, xb, yb)
        lg, lossg, _, gng = g(xb, yb)
        assert torch.equal(le, lg) and torch.equal(losse, lossg) and torch.equal(gne, gng)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.isfinite(pe).all() and torch.equal(pe, pg), n
    if cfg.use_kohonen:
        for km in ("local_kohonen", "global_kohonen"):
            assert torch.equal(getattr(me, km).nodes, getattr(mg, km).nodes), km


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graphed_eval_predict_equals_predict(precision):
    from nvit_amd import GraphedEval, evaluate
    cfg = named_config("hd80")
    m = build(cfg, precision).train()
    batches = [tuple(t.cuda() for t in synthetic_batch(cfg, 4, seed=s)) for s in (11, 12)]
    ge = GraphedEval(m, *batches[0])
    for X, _ in batches:
        got, want = ge.predict(X).clone(), evaluate.predict(m, X)
        assert torch.isfinite(got).all() and torch.equal(got, want), (got - want).abs().max().item()


def test_bf16_gradients_of_every_parameter_vs_fp64():
    """`hd80` in bf16 (MFMA attention forward and backward at 128, the padded split and merge, dO / O padding): logits and
    every parameter gradient against a float64 run of the CPU oracle, on the pattern and bars of
    test_bf16_fused_route_vs_unfused_and_fp64 (tests/test_gpu_vit_baseline.py): logits 1e-2, each gradient within 0.1 of
    its error scale - its own norm, or for a block's q/k/v projections the norm of their stacked gradient, which one
    bf16 weight-gradient GEMM produces."""
    torch.set_num_threads(8)
    cfg = named_config("hd80")
    batch = 8
    X, y = synthetic_batch(cfg, batch)
    p = {n: t.detach().clone().double().requires_grad_(True) for n, t in formula_state_dict(cfg).items()}
    O.renorm_(p, cfg)
    ref_logits, _, _ = O.loss_and_grads(p, cfg, X.double(), y)
    ref_grads = {n: t.grad for n, t in p.items() if t.grad is not None}
    m = build(cfg, "bf16").train()
    logits, _ = m(X.cuda())
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    got = {n: q.grad.double().cpu() for n, q in m.named_parameters() if q.grad is not None}
    e_ref = (logits.detach().double().cpu() - ref_logits).abs().max().item()
    print(f"[hd80 bf16] max|dlogit| vs fp64 {e_ref:.3e}, logit max {ref_logits.abs().max().item():.3f}")
    assert e_ref < 1e-2
    assert sorted(got) == sorted(ref_grads)

    def scale_of(n):
        parts = n.split(".")
        if parts[0] == "transformer" and parts[3] in ("query", "key", "value"):
            pre, leaf = ".".join(parts[:3]), parts[4]
            return math.sqrt(sum(ref_grads[f"{pre}.{k}.{leaf}"].norm().item() ** 2 for k in ("query", "key", "value")))
        return ref_grads[n].norm().item()

    worst = 0.0
    for n, r in ref_grads.items():
        sc = scale_of(n)
        if sc < 1e-12:
            continue
        e_r = (got[n].flatten() - r.flatten()).norm().item() / sc
        worst = max(worst, e_r)
        assert e_r < 0.1, (n, e_r)
    print(f"   worst relative gradient error vs fp64 {worst:.4f}")
