"""GPU: nViT at widths over 1152 (n_embd up to 2048).

The fused optimizer step and the stand-alone renorm take column-normalised matrices of up to 2048 rows (a 16-column LDS
slab / a 32-column register panel above 1152 rows) and row-normalised matrices of up to 2048 columns.  Op level on shapes
that straddle every boundary; whole model against numbers recorded from the reference itself
(tests/golden/wide*_b2.npz, tools/make_golden_wide.py) with the bars the BASELINE sizes are held to
(tests/test_gpu_model.py); several steps against the CPU oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nvit_oracle as O

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

import vit_torch_ref
from optim_check import _fake_model  # noqa: F401  (it lives there; kept importable from here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"

# (shape, dim): 1152 rows / 1536 columns are the last sizes of the earlier paths.  (2048, 328) stands for mlp_c_proj at
# n_embd = 2048 ([2048, 8192]) cut to a width the CPU reference steps through quickly; 328 is not a multiple of the
# 16-column slab, 33 not a multiple of 4, 100 not a multiple of 32.
COL_SHAPES = [(1152, 40), (1153, 40), (1280, 100), (2048, 33), (2048, 328)]
ROW_SHAPES = [(40, 1536), (40, 1540), (24, 2048), (8 * 64, 1280)]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def build(cfg, precision, renormed=True):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)   # Kohonen index buffers are not in the formula dict
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to(DEV).set_precision(precision)
    if renormed and cfg.use_nvit:
        normalize_matrices(m)
    return m


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("grad_clip", [0.0, 0.05])
def test_fused_adamw_renorm_wide_matches_torch(grad_clip):
    """FusedAdamW.step_fused against clip_grad_norm_ -> torch.optim.AdamW.step -> x / ||x|| on CPU fp32, three steps:
    the procedure and bars of test_fused_adamw_renorm_matches_torch on the shapes around and over the earlier caps."""
    from nvit_amd.optim import FusedAdamW
    shapes = [(s, 0) for s in COL_SHAPES] + [(s, 1) for s in ROW_SHAPES] + [((517,), -1), ((8192 * 2 + 12,), -1)]
    ref = [torch.nn.Parameter(rnd(*s, seed=20 + i, scale=0.05)) for i, (s, _) in enumerate(shapes)]
    mine = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref]
    groups = lambda ps: [{"params": [p for p in ps if p.dim() >= 2], "weight_decay": 0.1},
                         {"params": [p for p in ps if p.dim() < 2], "weight_decay": 0.0}]
    o_ref = torch.optim.AdamW(groups(ref), lr=1e-2, betas=(0.9, 0.95))
    o_my = FusedAdamW(groups(mine), lr=1e-2, betas=(0.9, 0.95))
    model = _fake_model([p for p, (_, k) in zip(mine, shapes) if k == 1], [p for p, (_, k) in zip(mine, shapes) if k == 0])
    for step in range(3):
        for i, (pr, pm) in enumerate(zip(ref, mine)):
            g = rnd(*pr.shape, seed=100 + 10 * step + i, scale=0.02)
            pr.grad = g.clone()
            pm.grad = g.to(DEV)
        if grad_clip > 0:
            gn_ref = torch.nn.utils.clip_grad_norm_(ref, grad_clip)
        o_ref.step()
        with torch.no_grad():
            for pr, (_, k) in zip(ref, shapes):
                if k >= 0:
                    pr.copy_(pr / pr.norm(dim=k, keepdim=True))
        gn = o_my.step_fused(model, grad_clip)
        if grad_clip > 0:
            assert abs(gn.item() - gn_ref.item()) <= 1e-5 * gn_ref.item()
        for pr, pm in zip(ref, mine):
            err = (pm.detach().cpu() - pr.detach()).abs().max().item()
            print(f"[fused adamw clip={grad_clip} step {step}] {tuple(pr.shape)}: max|dp| {err:.3e}")
            assert err <= 2e-6 * max(1.0, pr.detach().abs().max().item()), (step, tuple(pr.shape), err)
    sd_ref, sd_my = o_ref.state_dict(), o_my.state_dict()
    assert sd_ref["state"].keys() == sd_my["state"].keys()
    for k in sd_ref["state"]:
        assert float(sd_my["state"][k]["step"]) == float(sd_ref["state"][k]["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            a, b = sd_my["state"][k][name].cpu(), sd_ref["state"][k][name]
            assert (a - b).abs().max().item() <= 1e-6 * max(1e-3, b.abs().max().item())


def _check_renormed(ws, dims, dws):
    for w, d, dw in zip(ws, dims, dws):
        w64 = w.double()
        ref = w64 / w64.norm(dim=d, keepdim=True)
        got = dw.cpu().double()
        err = (got - ref).abs().max().item()
        nerr = (got.norm(dim=d) - 1).abs().max().item()
        print(f"[renorm] {tuple(w.shape)} dim={d}: max|d| {err:.3e}, max|norm-1| {nerr:.3e}")
        assert err < 2e-7, (tuple(w.shape), d, err)
        assert nerr < 1e-5, (tuple(w.shape), d, nerr)


def test_renorm_weights_wide_vs_fp64():
    """ops.renorm_weights against fp64 x / ||x||: element error < 2e-7 absolute (the bar of test_renorm_and_shadow; the
    entries of a normalised matrix of 1153-2048 rows are of order 0.02-0.1, one fp32 rounding of the quotient is below
    1e-8), every normalised row / column norm within 1e-5 of 1.  Each matrix in a launch of its own, then all of them,
    earlier-path and new-path matrices mixed, in one launch."""
    from nvit_amd import ops
    shapes = [(s, 0) for s in COL_SHAPES] + [(s, 1) for s in ROW_SHAPES] + [((768, 100), 0), ((96, 64), 1)]
    ws = [rnd(*s, seed=40 + i) for i, (s, _) in enumerate(shapes)]
    dims = [d for _, d in shapes]
    for w, d in zip(ws, dims):
        dw = w.to(DEV).contiguous()
        table, items = ops.renorm_table([(dw, d)], torch.device(DEV))
        ops.renorm_weights(table, items)
        _check_renormed([w], [d], [dw])
    order = [9, 0, 5, 2, 10, 4, 1, 6, 3, 8, 7]   # old and new paths interleaved in one table
    dws = [ws[i].to(DEV).contiguous() for i in order]
    table, items = ops.renorm_table([(dw, dims[i]) for dw, i in zip(dws, order)], torch.device(DEV))
    ops.renorm_weights(table, items)
    _check_renormed([ws[i] for i in order], [dims[i] for i in order], dws)


def test_old_paths_unchanged_by_new_path_matrices_in_the_table():
    """A (1000, 100) column-normalised and a (40, 768) row-normalised matrix come out of the fused step bit-identical
    whether or not the table also holds matrices that take the new paths: the size dispatch did not reroute them.
    (No clipping: the clip factor depends on every gradient in the table.)"""
    from nvit_amd.optim import FusedAdamW
    outs = []
    for with_new in (False, True):
        shapes = [((1000, 100), 0), ((40, 768), 1)] + ([((1280, 100), 0), ((24, 2048), 1)] if with_new else [])
        ps = [torch.nn.Parameter(rnd(*s, seed=60 + i, scale=0.05).to(DEV)) for i, (s, _) in enumerate(shapes)]
        opt = FusedAdamW([{"params": ps, "weight_decay": 0.1}], lr=1e-2, betas=(0.9, 0.95))
        model = _fake_model([p for p, (_, k) in zip(ps, shapes) if k == 1], [p for p, (_, k) in zip(ps, shapes) if k == 0])
        for step in range(2):
            for i, p in enumerate(ps):
                p.grad = rnd(*p.shape, seed=200 + 10 * step + i, scale=0.02).to(DEV)
            opt.step_fused(model, 0.0)
        outs.append([p.detach().cpu() for p in ps[:2]] + [opt.state[p]["exp_avg_sq"].cpu() for p in ps[:2]])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ whole model
@pytest.mark.parametrize("name,batch", [("wide", 2), ("wide2k", 2), ("wide_k", 2)])
def test_fp32_wide_matches_reference_golden(name, batch):
    """The body and bars of test_fp32_full_size_matches_reference_golden (tests/test_gpu_model.py) on the wide configs,
    DIRECTLY against numbers recorded from the imported reference: fp32 mode logits 1e-5 (2e-5 with the Kohonen head),
    loss, aux losses, per-parameter gradient norms (5e-4 relative) and leading slices, the clipped global norm (2e-4),
    and after one full step (clip + AdamW + renorm) the step-1 logits (2e-4) and leading weights (2e-6)."""
    from nvit_amd.train import total_loss
    g = np.load(os.path.join(GOLD, f"{name}_b{batch}.npz"))
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, batch)
    m = build(cfg, "fp32").train()
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
    q0 = m.transformer.h[0].query.weight.detach().reshape(-1)[:8].cpu().numpy()
    assert np.abs(q0 - g["q0_head1"]).max() < 2e-6
    pl = m.transformer.h[-1].mlp_c_proj.weight.detach().reshape(-1)[:8].cpu().numpy()
    assert np.abs(pl - g["p_last_head1"]).max() < 2e-6
    _assert_unit_norms(m)


def _assert_unit_norms(m):
    for blk in m.transformer.h:
        for n in ("att_c_proj", "mlp_c_proj"):
            assert (getattr(blk, n).weight.detach().double().norm(dim=0) - 1).abs().max().item() < 1e-5, n
        for n in ("query", "key", "value", "c_fc"):
            assert (getattr(blk, n).weight.detach().double().norm(dim=1) - 1).abs().max().item() < 1e-5, n


@pytest.mark.parametrize("name,batch", [("wide", 2), ("wide2k", 2), ("wide_k", 2)])
def test_bf16_wide_deviation_bounded_by_the_references_own_bf16_path(name, batch):
    """As test_bf16_deviation_bounded_by_the_references_own_bf16_path: the HIP bf16 mode must be no farther from the
    reference's fp32 logits than the reference's own `torch.autocast("cpu", bfloat16)` path is, in max and in rms."""
    g = np.load(os.path.join(GOLD, f"{name}_b{batch}.npz"))
    cfg = named_config(name)
    X, _ = synthetic_batch(cfg, batch)
    ref32, refbf = g["logits_fp32"], g["logits_autocast_bf16"]
    m = build(cfg, "bf16").train()
    with torch.no_grad():
        lb, _ = m(X.cuda())
    lb = lb.float().cpu().numpy()
    rms = lambda a: float(np.sqrt(np.mean(np.square(a.astype(np.float64)))))
    hip_dev, ref_dev = np.abs(lb - ref32).max(), np.abs(refbf - ref32).max()
    hip_rms, ref_rms = rms(lb - ref32), rms(refbf - ref32)
    print(f"[autocast {name} B={batch}] |HIP_bf16 - ref_fp32| max {hip_dev:.3e} rms {hip_rms:.3e};  |ref_autocast_bf16 - ref_fp32| "
          f"max {ref_dev:.3e} rms {ref_rms:.3e};  |logit|max {np.abs(ref32).max():.3f}")
    assert abs(float(g["max_abs_dev"]) - ref_dev) < 1e-9
    assert hip_dev <= ref_dev, (hip_dev, ref_dev)
    assert hip_rms <= ref_rms, (hip_rms, ref_rms)


def test_wide_training_trajectory_vs_oracle():
    """Four consecutive train steps on `wide` in fp32 mode against the CPU oracle's own loop, with the bars of
    test_training_trajectory_vs_oracle; afterwards every normalised row / column norm is within 1e-5 of 1."""
    from nvit_amd.train import train_step
    torch.set_num_threads(8)
    cfg = named_config("wide")
    lr, wd, batch, steps = 3e-3, 0.1, 2, 4
    p = O.make_params(formula_state_dict(cfg))
    o_opt = O.make_optimizer(p, lr=lr, weight_decay=wd)
    m32 = build(cfg, "fp32", False).train()
    opt32 = m32.configure_optimizers(wd, lr, (0.9, 0.95), "cuda")
    worst32 = 0.0
    losses = []
    for it in range(steps):
        X, y = synthetic_batch(cfg, batch, seed=100 + it)
        lo, loss_o, _, gn_o = O.train_step(p, cfg, o_opt, X, y, 1.0)
        l32, loss32, _, gn32 = train_step(m32, opt32, X.cuda(), y.cuda(), 1.0)
        worst32 = max(worst32, (l32.detach().cpu() - lo.detach()).abs().max().item())
        losses.append((loss_o.item(), loss32.item()))
        assert abs(gn32.item() - gn_o.item()) < 1e-3 * gn_o.item(), (it, gn32.item(), gn_o.item())
    print(f"[trajectory wide] {steps} steps: max|dlogit| fp32 {worst32:.3e}; losses (oracle, fp32) "
          + " ".join(f"({a:.4f} {b:.4f})" for a, b in losses))
    assert losses[-1][0] != losses[0][0]
    assert worst32 < 2e-4, worst32
    for a, b in losses:
        assert abs(a - b) < 1e-4
    perr = 0.0
    for n, q in m32.named_parameters():
        perr = max(perr, (q.detach().cpu() - p[n].detach()).abs().max().item())
    print(f"   max parameter error after {steps} steps {perr:.3e}")
    assert perr < 2e-4, perr
    _assert_unit_norms(m32)


@pytest.mark.parametrize("name", ["wide", "wide2k"])
def test_torch_op_route_gives_the_same_weights(name):
    """clip_grad_norm_ -> torch.optim.AdamW.step -> normalize_matrices(model) (the stand-alone renorm kernel) leaves the
    weights step_fused leaves, within 2e-6."""
    from nvit_amd.train import normalize_matrices, total_loss
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, 2)
    models = []
    for fused in (True, False):
        m = build(cfg, "fp32").train()
        logits, aux = m(X.cuda())
        total_loss(cfg, logits, aux, y.cuda()).backward()
        if fused:
            m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda").step_fused(m, 1.0)
        else:
            opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")   # plain torch.optim.AdamW, same groups
            assert type(opt) is torch.optim.AdamW
            torch.nn.utils.clip_grad_norm_([q for q in m.parameters() if q.grad is not None], 1.0)
            opt.step()
            normalize_matrices(m)
        models.append(m)
    worst = 0.0
    for (n, a), (_, b) in zip(models[0].named_parameters(), models[1].named_parameters()):
        err = (a.detach() - b.detach()).abs().max().item()
        worst = max(worst, err)
        assert err <= 2e-6, (n, err)
    print(f"[torch-op route {name}] max weight difference {worst:.3e}")


def _poison_free_memory(nbytes=6 << 30):
    """Fill a large block of free HBM with NaNs and release it, so later torch.empty() buffers start as NaN."""
    t = torch.full((nbytes // 4,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    del t


def test_wide_step_under_nan_poison():
    """One train step on `wide`, B=2, with freed memory poisoned by NaNs gives the loss of a clean run and finite
    parameters: the new paths read no workspace or LDS they did not write."""
    from nvit_amd.train import train_step
    cfg = named_config("wide")
    X, y = synthetic_batch(cfg, 2)
    X, y = X.cuda(), y.cuda()
    clean = build(cfg, "bf16")
    ref = train_step(clean, clean.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda"), X, y)[1].item()
    m = build(cfg, "bf16")
    o = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    _poison_free_memory()
    got = train_step(m, o, X, y)[1].item()
    assert got == ref, (got, ref)
    for (n, a), (_, b) in zip(m.named_parameters(), clean.named_parameters()):
        assert torch.isfinite(a).all(), n
        assert torch.equal(a, b), n


def test_plain_vit_at_1280_vs_fp64():
    """The plain-ViT baseline (use_nvit=False, no renorm) at n_embd = 1280: fp32 forward / backward against the fp64
    torch restatement (tests/vit_torch_ref.py) with the bars of test_head_dims_and_bias_vs_fp64, then one fused step
    whose reported gradient norm is the fp64 one."""
    cfg = named_config("wide", use_nvit=False)
    X, y = synthetic_batch(cfg, 2)
    sd = formula_state_dict(cfg)
    ref_logits, _, _, ref_grads = vit_torch_ref.loss_and_grads(sd, cfg, X, y)
    m = build(cfg, "fp32").train()
    logits, _ = m(X.cuda())
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    e = (logits.detach().double().cpu() - ref_logits).abs().max().item()
    assert e <= 1e-5 * ref_logits.abs().max().item() + 1e-12, e
    for n, q in m.named_parameters():
        if n in ref_grads:
            r = ref_grads[n]
            assert (q.grad.double().cpu() - r).abs().max().item() <= 2e-4 * r.abs().max().item() + 1e-8, n
        else:
            assert q.grad is None, n
    gn_ref = torch.sqrt(sum(r.pow(2).sum() for r in ref_grads.values())).item()
    before = m.transformer.h[0].query.weight.detach().clone()
    gn = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda").step_fused(m, 1.0)[0].item()
    assert abs(gn - gn_ref) <= 2e-4 * gn_ref, (gn, gn_ref)
    after = m.transformer.h[0].query.weight.detach()
    assert torch.isfinite(after).all() and not torch.equal(after, before)


def test_width_1408_takes_the_unfused_qk_route():
    """n_embd = 1408 is a multiple of 64 but not of 256, which the q/k-normalising GEMM epilogue needs: at a token
    count where 2 * 1408 columns would otherwise qualify for the fused GEMM the bf16 mode must run forward and backward
    (on the split route) to finite values; the fp32 mode is held to the CPU oracle at the 1e-5 bar."""
    cfg = named_config("mini", n_embd=1408, n_head=22, n_layer=1)
    X, y = synthetic_batch(cfg, 32)   # 32 x 49 tokens
    p = O.make_params(formula_state_dict(cfg))
    O.renorm_(p, cfg)
    with torch.no_grad():
        lo, _ = O.forward(p, cfg, X)
    m32 = build(cfg, "fp32").train()
    with torch.no_grad():
        l32, _ = m32(X.cuda())
    assert (l32.cpu() - lo).abs().max().item() < 1e-5
    mbf = build(cfg, "bf16").train()
    lb, _ = mbf(X.cuda())
    torch.nn.functional.cross_entropy(lb.float(), y.cuda()).backward()
    assert torch.isfinite(lb).all()
    for n, q in mbf.named_parameters():
        assert q.grad is None or torch.isfinite(q.grad).all(), n
