"""GPU: the plain-ViT baseline (use_nvit=False) on the HIP kernels.

fp32 mode against numbers recorded from the reference itself (tests/golden/vit_*.npz, tools/make_golden_vit.py):
logits / losses <= 1e-5, gradients and the one-step result <= 2e-4 relative (the nViT bars).  bf16 mode: its distance
to the reference's fp32 logits may not exceed that of the reference's own bf16-autocast path.  The new row kernels
(residual + RMSNorm, residual + norm_skip, head split / merge) against float64 torch math on random data."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd import ops
from nvit_amd._lib import BF16, BF16_F32IN, F32
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

import vit_torch_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("micro", 8), ("mini", 4), ("tiny", 32)]
EPS = 1e-6


def _gold(name, batch):
    return np.load(os.path.join(GOLD, f"vit_{name}_b{batch}.npz"))


def build(cfg, precision):
    from nvit_amd.model import ViT
    m = ViT(cfg)
    m.load_state_dict(formula_state_dict(cfg), strict=True)
    return m.to("cuda:0").set_precision(precision).train()


def _close(got, ref, rel, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    e = (got - ref).abs().max().item()
    s = ref.abs().max().item()
    assert e <= rel * s + 1e-12, (what, e, s)


# ------------------------------------------------------------------------------------------------ row kernels
def _rand(M, C, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((M, C), device="cuda", generator=g) * scale).to(dtype)


def _rms64(z, w):
    rs = torch.rsqrt((z * z).mean(-1, keepdim=True) + EPS)
    return z * rs * w, rs


ROW_C = [64, 192, 768, 1024]
ROW_M = [37, 1001]        # ragged: not a multiple of the 4 rows of a workgroup


@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("M", ROW_M)
@pytest.mark.parametrize("ydt", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_res_rmsnorm_fwd_vs_fp64(C, M, ydt, dt):
    a = _rand(M, C, seed=1)
    y = _rand(M, C, ydt, 0.5, seed=2) if ydt is not None else None
    w = 1.0 + 0.1 * _rand(1, C, seed=3).reshape(C)
    out, out_lo, rstd = ops.res_rmsnorm_fwd(dt, a, y, w, EPS)
    z = a.double() + (y.double() if y is not None else 0.0)
    ref, rs = _rms64(z, w.double())
    _close(out, ref, 2e-6, "out")
    _close(rstd, rs.reshape(-1), 2e-6, "rstd")
    assert torch.equal(out_lo, out.to(ops.tdtype(dt)))


@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("M", ROW_M)
@pytest.mark.parametrize("ydt", [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("add", [False, True])
def test_res_rmsnorm_bwd_vs_fp64(C, M, ydt, dt, add):
    a = _rand(M, C, seed=4)
    y = _rand(M, C, ydt, 0.5, seed=5) if ydt is not None else None
    w = 1.0 + 0.1 * _rand(1, C, seed=6).reshape(C)
    g = _rand(M, C, seed=7)
    g_add = _rand(M, C, ops.tdtype(dt), 0.3, seed=8) if add else None
    prev = _rand(M, C, seed=9) if add else None        # exercise the accumulate mode with the addend variants
    _, _, rstd = ops.res_rmsnorm_fwd(dt, a, y, w, EPS, want_lo=False)
    dz, dz_lo, part = ops.res_rmsnorm_bwd(dt, g, a, y, w, rstd, g_add=g_add, dz=(prev.clone() if add else None),
                                          want_lo=True)
    z = (a.double() + (y.double() if y is not None else 0.0)).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    out, _ = _rms64(z, w64)
    gt = g.double() + (g_add.double() if add else 0.0)
    out.backward(gt)
    ref = z.grad + (prev.double() if add else 0.0)
    _close(dz, ref, 2e-5, "dz")
    assert torch.equal(dz_lo, dz.to(ops.tdtype(dt)))
    assert part.shape[0] % 4 == 0 and part.shape[1] == C
    _close(part.double().sum(0), w64.grad, 2e-5, "dw")


@pytest.mark.parametrize("C", ROW_C)
@pytest.mark.parametrize("M", ROW_M)
@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_res_skip_fwd_bwd_vs_fp64(C, M, ydt, dt):
    h = _rand(M, C, seed=10)
    y = _rand(M, C, ydt, 0.5, seed=11)
    x = _rand(M, C, seed=12)
    x = x / x.norm(dim=-1, keepdim=True)
    skip = torch.tensor([0.9], device="cuda")
    out, out_lo = ops.res_skip_fwd(dt, h, y, skip, x)
    h64 = h.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    s64 = skip.double().requires_grad_(True)
    r = (h64 + y.double()) * s64 + x64
    ref = r / r.norm(dim=-1, keepdim=True)
    _close(out, ref.detach(), 2e-6, "out")
    assert torch.equal(out_lo, out.to(ops.tdtype(dt)))
    g = _rand(M, C, seed=13)
    dh, dh_lo, dx, part = ops.res_skip_bwd(dt, g, h, y, skip, x)
    ref.backward(g.double())
    _close(dh, h64.grad, 2e-5, "dh")
    _close(dx, x64.grad, 2e-5, "dx")
    assert torch.equal(dh_lo, dh.to(ops.tdtype(dt)))
    _close(part.double().sum().reshape(1), s64.grad, 2e-5, "dskip")


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dt", [F32, BF16, BF16_F32IN])
def test_head_split_and_merge(d, dt):
    B, T, H = 3, 37, 4
    C, M = H * d, B * T
    tin = torch.float32 if dt in (F32, BF16_F32IN) else torch.bfloat16
    tout = torch.float32 if dt == F32 else torch.bfloat16
    qkv = _rand(M, 3 * C, tin, seed=14)
    qh, kh, vh, _, _ = ops.qknorm_fwd(dt, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, None, 0.0, B, T, H, d)
    heads = lambda t: t.reshape(B, T, H, d).transpose(1, 2).to(tout)
    assert torch.equal(qh, heads(qkv[:, :C])) and torch.equal(kh, heads(qkv[:, C:2 * C]))
    assert torch.equal(vh, heads(qkv[:, 2 * C:]))
    mdt = F32 if dt == F32 else BF16
    dq = torch.empty((M, 3 * C), device="cuda", dtype=tout)
    part = ops.qknorm_bwd(mdt, qh, kh, vh, None, None, None, None, None, 0.0, dq, 3 * C, dq[:, C:], 3 * C,
                          dq[:, 2 * C:], 3 * C, B, T, H, d)
    assert part is None
    assert torch.equal(dq, qkv.to(tout))


def test_fused_split_route_matches_unfused_ops():
    """Split-only q/k/v epilogue (EPI 4 with sqk = NULL, q pre-scaled), running-max attention on the pre-scaled q, and the
    MFMA backward's plain token-major store, against fp32 GEMM + split + attention + merge (bf16, d = 64)."""
    B, T, H, d = 112, 49, 4, 64
    C, M = H * d, B * T
    assert ops.fusable(BF16, M, 3 * C, C)
    A = _rand(M, C, torch.bfloat16, seed=30)
    W = _rand(3 * C, C, torch.bfloat16, 0.06, seed=31)
    qpre = ops.LOG2E / math.sqrt(d)
    scale = 1.0 / math.sqrt(d)
    qh, kh, vh, rq, rk = ops.gemm_nt_qknorm(A, W, M, C, 3, 0, None, 0.0, B, T, H, d, q_prescale=qpre)
    assert rq is None and rk is None
    qkv = ops.gemm_nt(A, W, M, 3 * C, C, out_dtype=torch.float32)
    q2, k2, v2, rq2, rk2 = ops.qknorm_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, None, 0.0,
                                          B, T, H, d)
    assert rq2 is None and rk2 is None
    _close(qh, q2.float() * qpre, 8e-3, "q")
    _close(kh, k2, 8e-3, "k")
    _close(vh, v2, 8e-3, "v")
    o1, lse1 = ops.attn_fwd(BF16, 1, qh, kh, vh, scale, q_prescale=qpre)
    o2, lse2 = ops.attn_fwd(BF16, 1, q2, k2, v2, scale)
    _close(o1, o2, 2e-2, "o")
    _close(lse1, lse2, 1e-3, "lse")
    do = _rand(M, C, torch.bfloat16, seed=32)
    d1 = torch.empty((M, 3 * C), device="cuda", dtype=torch.bfloat16)
    pq, pk = ops.attn_bwd_qknorm(do, qh, kh, vh, o1, lse1, scale, None, None, None, 0.0, d1, 3 * C, d1[:, C:],
                                 d1[:, 2 * C:], 3 * C, q_prescale=qpre)
    assert pq is None and pk is None
    dqh, dkh, dvh = ops.attn_bwd(BF16, 1, do, q2, k2, v2, o2, lse2, scale)
    d2 = torch.empty_like(d1)
    ops.qknorm_bwd(BF16, dqh, dkh, dvh, None, None, None, None, None, 0.0, d2, 3 * C, d2[:, C:], 3 * C, d2[:, 2 * C:],
                   3 * C, B, T, H, d)
    for i, n in enumerate("qkv"):
        _close(d1[:, i * C:(i + 1) * C], d2[:, i * C:(i + 1) * C], 3e-2, "d" + n)


def test_row_wrappers_reject_bad_operands():
    a = _rand(16, 64)
    w = torch.ones(64, device="cuda")
    _, _, rstd = ops.res_rmsnorm_fwd(F32, a, None, w, EPS)
    with pytest.raises(ValueError):
        ops.res_rmsnorm_bwd(F32, _rand(16, 128)[:, ::2], a, None, w, rstd)     # strided gradient
    with pytest.raises(ValueError):
        ops.res_rmsnorm_bwd(F32, a, a, _rand(16, 32), w, rstd)                 # y of the wrong shape
    with pytest.raises(ValueError):
        ops.res_rmsnorm_bwd(F32, a, a, None, w, rstd, dz=a.to(torch.bfloat16))  # dz not fp32
    with pytest.raises(ValueError):
        ops.res_skip_bwd(F32, a.t(), a, a, torch.ones(1, device="cuda"), a)   # non-contiguous dout
    with pytest.raises(RuntimeError):
        ops.res_skip_fwd(F32, a.cpu(), a, torch.ones(1, device="cuda"), a)    # host tensor


# ------------------------------------------------------------------------------------------------ whole model
@pytest.mark.parametrize("name,batch", CASES)
def test_fp32_matches_reference_golden_and_one_step(name, batch):
    from nvit_amd.train import train_step
    g = _gold(name, batch)
    cfg = named_config(name + "_vit")
    X, y = synthetic_batch(cfg, batch)
    m = build(cfg, "fp32")
    logits, aux = m(X.cuda())
    loss = torch.nn.functional.cross_entropy(logits, y.cuda())
    loss.backward()
    err = np.abs(logits.detach().cpu().numpy() - g["logits"]).max()
    print(f"[vit fp32 {name}] max|dlogit| = {err:.3e}")
    assert err <= 1e-5
    assert abs(loss.item() - float(g["loss"])) <= 1e-5
    assert abs(aux["reconstruction"].item() - float(g["recon"])) <= 1e-5
    params = dict(m.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(g["grad_names"])
    for n, gn, head in zip(g["grad_names"], g["grad_norms"], g["grad_heads"]):
        gr = params[n].grad.reshape(-1).double().cpu()
        assert abs(gr.norm().item() - gn) <= 2e-4 * gn + 1e-8, n
        k = min(8, gr.numel())
        assert np.abs(gr[:k].numpy() - head[:k]).max() <= 2e-4 * gr.abs().max().item() + 1e-8, n
    m.zero_grad(set_to_none=True)
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    assert len(opt.param_groups) == 2
    _, _, _, gnorm = train_step(m, opt, X.cuda(), y.cuda(), 1.0)
    assert abs(gnorm.item() - float(g["gnorm"])) <= 2e-4 * float(g["gnorm"])
    with torch.no_grad():
        logits1, aux1 = m(X.cuda())
    e1 = np.abs(logits1.cpu().numpy() - g["logits1"]).max()
    print(f"[vit fp32 {name}] step-1 max|dlogit| = {e1:.3e}")
    assert e1 <= 2e-4 * max(1.0, np.abs(g["logits1"]).max())
    assert abs(aux1["reconstruction"].item() - float(g["recon1"])) <= 2e-4 * float(g["recon1"])


@pytest.mark.parametrize("name,batch", CASES + [("base", 2)])
def test_bf16_deviation_bounded_by_the_references_own_bf16_path(name, batch):
    g = _gold(name, batch)
    cfg = named_config(name + "_vit")
    X, _ = synthetic_batch(cfg, batch)
    m = build(cfg, "bf16")
    with torch.no_grad():
        logits, _ = m(X.cuda())
    d = np.abs(logits.cpu().numpy().astype(np.float64) - g["logits"])
    da = np.abs(g["logits_autocast"].astype(np.float64) - g["logits"])
    rms, rms_a = math.sqrt((d ** 2).mean()), math.sqrt((da ** 2).mean())
    print(f"[vit bf16 {name}] max {d.max():.3e} (autocast {da.max():.3e})  rms {rms:.3e} (autocast {rms_a:.3e})")
    assert d.max() <= da.max() and rms <= rms_a


@pytest.mark.parametrize("n_head", [4, 2, 1])      # head dims 32, 64, 128
@pytest.mark.parametrize("bias", [False, True])
def test_head_dims_and_bias_vs_fp64(n_head, bias):
    cfg = named_config("mini_vit", n_head=n_head, bias=bias)
    X, y = synthetic_batch(cfg, 4)
    sd = formula_state_dict(cfg)
    ref_logits, ref_loss, _, ref_grads = vit_torch_ref.loss_and_grads(sd, cfg, X, y)
    m = build(cfg, "fp32")
    logits, _ = m(X.cuda())
    torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
    _close(logits.detach(), ref_logits, 1e-5, "logits")
    for n, p in m.named_parameters():
        if n in ref_grads:
            r = ref_grads[n]
            assert (p.grad.double().cpu() - r).abs().max().item() <= 2e-4 * r.abs().max().item() + 1e-8, n
        else:
            assert p.grad is None, n
    mb = build(cfg, "bf16")
    with torch.no_grad():
        lb, _ = mb(X.cuda())
    e = (lb.double().cpu() - ref_logits).abs().max().item()
    print(f"[vit d={cfg.n_embd // n_head} bias={bias}] bf16 max|dlogit| {e:.3e}")
    assert torch.isfinite(lb).all() and e < 1e-2


def test_standalone_block_and_cross_attention_forward():
    """Block.forward (output before norm_skip) and CrossAttentionBlock.forward on their own, fp32, against float64."""
    cfg = named_config("mini_vit")
    m = build(cfg, "fp32")
    sd = {n: t.double() for n, t in formula_state_dict(cfg).items()}
    B, T, C = 2, m.n_tokens, cfg.n_embd
    h = _rand(B * T, C, seed=20).reshape(B, T, C)
    h2 = _rand(B * T, C, seed=21).reshape(B, T, C)
    with torch.no_grad():
        out = m.transformer.h[1](h)
        xo = m.cross_attention(h, h2)
    # float64: a one-block / cross-only model through the restatement, by zeroing what is not under test
    import torch.nn.functional as F
    p = "transformer.h.1."

    def rms(x, w):
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w

    def attn(q, k, v):
        H, d = cfg.n_head, C // cfg.n_head
        hs = lambda t: t.reshape(B, T, H, d).transpose(1, 2)
        return ((hs(q) @ hs(k).transpose(-1, -2) / math.sqrt(d)).softmax(-1) @ hs(v)).transpose(1, 2).reshape(B, T, C)

    hh = h.double().cpu()
    a = rms(hh, sd[p + "rmsnorm_att.weight"])
    h1 = a + F.linear(attn(F.linear(a, sd[p + "query.weight"]), F.linear(a, sd[p + "key.weight"]),
                           F.linear(a, sd[p + "value.weight"])), sd[p + "att_c_proj.weight"])
    bm = rms(h1, sd[p + "rmsnorm_mlp.weight"])
    u, v = F.linear(bm, sd[p + "c_fc.weight"]).chunk(2, dim=-1)
    _close(out, bm + F.linear(u * F.silu(v), sd[p + "mlp_c_proj.weight"]), 1e-5, "block")
    q = "cross_attention."
    ln, gn = rms(hh, sd[q + "local_norm.weight"]), rms(h2.double().cpu(), sd[q + "global_norm.weight"])
    o = attn(F.linear(ln, sd[q + "q_local.weight"]), F.linear(gn, sd[q + "k_global.weight"]),
             F.linear(gn, sd[q + "v_global.weight"]))
    u, v = F.linear(o, sd[q + "proj.weight"]).chunk(2, dim=-1)
    _close(xo, F.linear(u * F.silu(v), sd[q + "out_proj.weight"]), 1e-5, "cross")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_train_step_equals_eager(precision):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro_vit")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    X2, y2 = synthetic_batch(cfg, 8, seed=77)
    X2, y2 = X2.cuda(), y2.cuda()
    me, mg = build(cfg, precision), build(cfg, precision)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for _ in range(2):
        train_step(me, oe, X, y)
    g = GraphedTrainStep(mg, og, X, y, warmup=2)
    for xb, yb in ((X, y), (X2, y2), (X, y)):
        le, losse, _, gne = train_step(me, oe, xb, yb)
        lg, lossg, _, gng = g(xb, yb)
        assert torch.equal(le, lg) and torch.equal(losse, lossg) and torch.equal(gne, gng)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n


def _poison_free_memory(nbytes=6 << 30):
    t = torch.full((nbytes // 4,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize("name,batch", [("micro", 8), ("tiny", 32)])
def test_no_uninitialised_reads_under_nan_poison(name, batch):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(name + "_vit")
    X, y = synthetic_batch(cfg, batch)
    X, y = X.cuda(), y.cuda()
    clean = build(cfg, "bf16")
    oc = clean.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ref = [train_step(clean, oc, X, y)[1].item() for _ in range(5)]
    m = build(cfg, "bf16")
    o = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    got = []
    for _ in range(2):
        _poison_free_memory()
        got.append(train_step(m, o, X, y)[1].item())
    _poison_free_memory()
    g = GraphedTrainStep(m, o, X, y, warmup=1)
    got.append(float("nan"))           # the warm-up step inside GraphedTrainStep
    for _ in range(2):
        _poison_free_memory()
        got.append(g(X, y)[1].item())
    assert got[0] == ref[0] and got[1] == ref[1] and got[3] == ref[3] and got[4] == ref[4], (got, ref)
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all(), n


def test_checkpoint_resume_is_exact(tmp_path):
    from nvit_amd.checkpoint import load_checkpoint, save_checkpoint
    from nvit_amd.train import train_step
    cfg = named_config("micro_vit")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    mk_opt = lambda mm: mm.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    a = build(cfg, "bf16")
    oa = mk_opt(a)
    for _ in range(3):
        train_step(a, oa, X, y)
    b = build(cfg, "bf16")
    ob = mk_opt(b)
    for _ in range(2):
        train_step(b, ob, X, y)
    path = save_checkpoint(tmp_path / "checkpoint_latest.pt", b, ob, 2, {"val/loss": 0.0, "train/loss": 0.0})
    c, oc, ck = load_checkpoint(path, device="cuda", optimizer_factory=mk_opt, trusted=True)
    assert not c.config.use_nvit and ck["iter_num"] == 2
    c.set_precision("bf16").train()
    train_step(c, oc, X, y)
    for (n, pa), (_, pc) in zip(a.named_parameters(), c.named_parameters()):
        assert torch.equal(pa, pc), n
    sa, sc = oa.state_dict()["state"], oc.state_dict()["state"]
    assert sa.keys() == sc.keys()
    for k in sa:
        assert torch.equal(sa[k]["exp_avg"], sc[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sc[k]["exp_avg_sq"])


def test_training_learns_in_bf16():
    """A few dozen fused steps on a fixed batch drive the loss down (end to end as a learner)."""
    from nvit_amd.train import train_step
    cfg = named_config("mini_vit")
    X, y = synthetic_batch(cfg, 16)
    X, y = X.cuda(), y.cuda()
    m = build(cfg, "bf16")
    opt = m.configure_optimizers(0.0, 3e-3, (0.9, 0.95), "cuda")
    first = train_step(m, opt, X, y)[1].item()
    for _ in range(40):
        last = train_step(m, opt, X, y)[1].item()
    print(f"[vit learn] loss {first:.3f} -> {last:.3f}")
    assert math.isfinite(last) and last < 0.5 * first


@pytest.mark.parametrize("bias", [False, True])
def test_bf16_fused_route_vs_unfused_and_fp64(bias):
    """A shape that takes the fused epilogues (split-only q/k/v, SwiGLU forward and backward with gate scale 1, the
    MFMA attention backward's plain store) in bf16: logits and every parameter gradient against the float64
    restatement, and against the same model with the fusions switched off.  With bias the fused q/k/v and c_fc GEMMs
    add it inside their head-split and SwiGLU epilogues (the same fused kernels as without); the SwiGLU backward
    epilogue runs as well."""
    cfg = named_config("mini_vit", n_embd=256, n_head=4, bias=bias)
    batch = 112
    X, y = synthetic_batch(cfg, batch)
    T = (cfg.image_size // cfg.local_patch_size) ** 2
    assert ops.fusable(BF16, batch * T, 3 * cfg.n_embd, cfg.n_embd), "test config no longer reaches the fused path"
    torch.set_num_threads(8)
    ref_logits, _, _, ref_grads = vit_torch_ref.loss_and_grads(formula_state_dict(cfg), cfg, X, y)   # float64, CPU

    def run(fuse_min):
        old = ops.FUSE_MIN_ELEMS
        ops.FUSE_MIN_ELEMS = fuse_min
        try:
            m = build(cfg, "bf16")
            logits, _ = m(X.cuda())
            torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
            return logits.detach().double().cpu(), {n: q.grad.double().cpu() for n, q in m.named_parameters()
                                                     if q.grad is not None}
        finally:
            ops.FUSE_MIN_ELEMS = old

    lf, gf = run(ops.FUSE_MIN_ELEMS)
    lu, gu = run(1 << 62)
    e_ref = (lf - ref_logits).abs().max().item()
    e_fu = (lf - lu).abs().max().item()
    print(f"[vit fused bias={bias}] max|dlogit| vs fp64 {e_ref:.3e} (unfused {(lu - ref_logits).abs().max().item():.3e}),"
          f" fused vs unfused {e_fu:.3e}, logit max {ref_logits.abs().max().item():.3f}")
    assert e_ref < 1e-2 and e_fu < 5e-3
    assert sorted(gf) == sorted(gu) == sorted(ref_grads)

    def scale_of(n):
        """Error scale of a gradient: its own norm, or for the q/k/v projections of a block the norm of the stacked
        q/k/v gradient that one bf16 weight-gradient GEMM produces.  At these weights block attention is nearly uniform
        and the q / k gradients are 1e-7 .. 1e-9 of the v gradient (softmax: sum over keys of dS = 0), so relative to
        their own size they are cancellation noise in any bf16 computation (a float32 CPU emulation that rounds the
        linear operands and output gradients to bf16 misses them by 2 % .. 550 %)."""
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
        a, b = gf[n].flatten(), gu[n].flatten()
        e_r = (a - r.flatten()).norm().item() / sc
        e_u = (a - b).norm().item() / sc
        worst = max(worst, e_r)
        assert e_r < 0.1 and e_u < 0.05, (n, e_r, e_u)
    print(f"   worst relative gradient error vs fp64 {worst:.4f}")
