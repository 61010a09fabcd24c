"""GPU: flash_attn=True, the reference's head-axis attention (softmax over the H heads of each token).

1. nvit_attn_heads_fwd / _bwd against a float64 restatement: head dims 32 / 64 / 128 x 2..32 heads, ragged row counts,
   nViT (normalised, sqk) and plain heads, self- and cross-attention buffer layouts, fp32 and bf16 outputs; two backward
   runs are bitwise identical.
2. The fp32 mode against the numbers recorded from the reference itself (tests/golden/fa_*.npz, tools/make_golden_flash.py).
3. The bf16 mode no farther from the reference's fp32 logits than the reference's own bf16-autocast path.
4. GraphedTrainStep with micro_fa replays the eager step bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd import ops
from nvit_amd._lib import BF16, F32
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BF16_REL = 2.0 ** -8   # one bf16 rounding of a stored value (half an ulp is 2^-9 relative; margin for the fp32 part)


def _ref(q, k, v, sqk, c_q, scale, H, d, dout):
    """float64: O, and (dq, dk, dv, d sqk) for the upstream gradient dout; q [M, C] etc."""
    M, C = q.shape
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = sqk.detach().double().requires_grad_(True) if sqk is not None else None
    sp = lambda t: t.reshape(M, H, d)
    if s is not None:
        nrm = lambda t: t / t.norm(dim=-1, keepdim=True)
        se = (s * c_q).reshape(H, d)
        qt, kt = se * nrm(sp(q)), se * nrm(sp(k))
    else:
        qt, kt = sp(q), sp(k)
    p = torch.softmax(qt @ kt.transpose(-1, -2) * scale, dim=-1)
    o = (p @ sp(v)).reshape(M, C)
    o.backward(dout.double())
    return o.detach(), q.grad, k.grad, v.grad, (s.grad if s is not None else None)


def _close(got, want, dt, what):
    got, want = got.double(), want.double()
    big = want.abs().max().item()
    err = (got - want).abs()
    if dt == F32:
        assert err.max().item() <= 1e-5 * big, (what, err.max().item(), big)
    else:
        bound = BF16_REL * want.abs() + 1e-5 * big
        assert bool((err <= bound).all()), (what, (err - bound).max().item(), big)


def _run(dt, d, H, M, norm, cross, seed=0):
    dev = "cuda"
    C = H * d
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * H + d)
    if cross:
        qbuf = torch.randn(M, C, generator=g).to(dev)
        kvbuf = torch.randn(M, 2 * C, generator=g).to(dev)
        q, k, v, ldq, ldkv = qbuf, kvbuf, kvbuf[:, C:], C, 2 * C
    else:
        qkv = torch.randn(M, 3 * C, generator=g).to(dev)
        q, k, v, ldq, ldkv = qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, 3 * C
    if norm:
        c_q = 1.0 / (1.0 / math.sqrt(C))
        # sqk * c_q around 1, as the model holds it (exactly 1 at initialisation): scores up to about sqrt(d)
        sqk = ((1.0 + 0.2 * torch.randn(C, generator=g)) / c_q).to(dev)
        scale = math.sqrt(d)
    else:
        c_q, sqk, scale = 0.0, None, 1.0 / math.sqrt(d)
    td = ops.tdtype(dt)
    dout = torch.randn(M, C, generator=g).to(dev).to(td)
    o, lse = ops.attn_heads_fwd(dt, q, ldq, k, v, ldkv, sqk, c_q, scale, M, H, d)

    def bwd():
        if cross:
            dq = torch.full((M, C), float("nan"), device=dev, dtype=td)
            dkv = torch.full((M, 2 * C), float("nan"), device=dev, dtype=td)
            dk, dv, lddq, lddkv = dkv, dkv[:, C:], C, 2 * C
        else:
            dqkv = torch.full((M, 3 * C), float("nan"), device=dev, dtype=td)
            dq, dk, dv, lddq, lddkv = dqkv, dqkv[:, C:], dqkv[:, 2 * C:], 3 * C, 3 * C
        part = ops.attn_heads_bwd(dt, dout, q, ldq, k, v, ldkv, sqk, c_q, scale, lse, dq, lddq, dk, dv, lddkv, M, H, d)
        return dq[:, :C].clone(), dk[:, :C].clone(), dv[:, :C].clone(), part

    dq, dk, dv, part = bwd()
    dq2, dk2, dv2, part2 = bwd()
    torch.cuda.synchronize()
    for a, b in ((dq, dq2), (dk, dk2), (dv, dv2), (part, part2)):
        if a is not None:
            assert torch.equal(a, b), "backward is not deterministic"
    ro, rdq, rdk, rdv, rds = _ref(q[:, :C], k[:, :C], v[:, :C], sqk, c_q, scale, H, d, dout.float())
    tag = f"dt={dt} d={d} H={H} M={M} norm={norm} cross={cross}"
    _close(o, ro, dt, "O " + tag)
    _close(dq, rdq, dt, "dq " + tag)
    _close(dk, rdk, dt, "dk " + tag)
    _close(dv, rdv, dt, "dv " + tag)
    if norm:
        ds = part.double().sum(0) * c_q
        big = rds.abs().max().item()
        assert (ds - rds).abs().max().item() <= (1e-5 if dt == F32 else 1e-4) * big, ("dsqk " + tag)
    # lse: natural log of each softmax denominator (the backward's only saved state besides the inputs)
    assert torch.isfinite(lse).all()


SHAPES = [(d, H) for d in (32, 64, 128) for H in (2, 3, 12, 16, 32) if (H * d) % 64 == 0]


@pytest.mark.parametrize("d,H", SHAPES)
def test_kernels_against_float64(d, H):
    for dt in (F32, BF16):
        for norm in (True, False):
            for cross in (False, True):
                for M in (1, 37):
                    _run(dt, d, H, M, norm, cross)


def test_kernels_many_rows_per_workgroup():
    """More rows than workgroups: each workgroup loops over tokens (LDS stage reuse, d(sqk) partials over several rows)."""
    for dt in (F32, BF16):
        _run(dt, 64, 12, 10001, True, False)
        _run(dt, 32, 32, 9000, False, True)


def test_head_count_beyond_the_build_is_rejected():
    q = torch.zeros(4, 3 * 33 * 32, device="cuda")
    with pytest.raises(RuntimeError, match="at most 32"):
        ops.attn_heads_fwd(F32, q, q.shape[1], q, q, q.shape[1], None, 0.0, 1.0, 4, 33, 32)


# ---------------------------------------------------------------------------------------------- whole model
def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision)
    if cfg.use_nvit:
        normalize_matrices(m)   # the renormed weight state the fixtures were recorded in
    return m


FA_CASES = [("micro", 8), ("micro_k", 8), ("mini", 4), ("tiny", 32), ("micro_vit", 8)]
AUX_KEYS = ("kohonen_consistency", "kohonen_smoothness", "local_quantization", "global_quantization")


@pytest.mark.parametrize("name,batch", FA_CASES)
def test_fp32_matches_reference_golden_and_one_step(name, batch):
    from nvit_amd.train import total_loss, train_step
    g = np.load(os.path.join(GOLD, f"fa_{name}_b{batch}.npz"))
    cfg = named_config(name + "_fa")
    X, y = synthetic_batch(cfg, batch)
    m = build(cfg, "fp32").train()
    logits, aux = m(X.cuda())
    loss = total_loss(cfg, logits, aux, y.cuda())
    loss.backward()
    tol = 2e-5 if cfg.use_kohonen else 1e-5
    e = np.abs(logits.detach().cpu().numpy() - g["logits"]).max()
    print(f"[fa golden {name} B={batch}] fp32 max|dlogit| {e:.3e} (|logit|max {np.abs(g['logits']).max():.3f})")
    assert e <= tol
    assert abs(loss.item() - float(g["loss"])) <= tol
    assert abs(aux["reconstruction"].item() - float(g["recon"])) <= 1e-5
    if cfg.use_kohonen:
        for i, k in enumerate(AUX_KEYS):
            assert abs(aux[k].item() - float(g["aux"][i])) < 2e-5 * max(1.0, abs(float(g["aux"][i]))), k
    params = dict(m.named_parameters())
    for n, gn in zip(g["grad_names"], g["grad_norms"]):
        gr = params[n].grad
        assert gr is not None, n
        assert abs(gr.double().norm().item() - gn) <= 2e-4 * gn + 1e-8, (n, gr.double().norm().item(), gn)
    # one full step (clip + AdamW + renorm) from a fresh model, then the step-1 logits
    m = build(cfg, "fp32").train()
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    _, _, _, gnorm = train_step(m, opt, X.cuda(), y.cuda(), 1.0)
    assert abs(gnorm.item() - float(g["gnorm"])) <= 2e-4 * float(g["gnorm"])
    with torch.no_grad():
        logits1, _ = m(X.cuda())
    e1 = np.abs(logits1.cpu().numpy() - g["logits1"]).max()
    print(f"   step-1 max|dlogit| {e1:.3e}")
    assert e1 <= 2e-4


@pytest.mark.parametrize("name,batch", [("mini", 4), ("tiny", 32), ("micro_vit", 8), ("base", 2)])
def test_bf16_deviation_bounded_by_the_references_own_bf16_path(name, batch):
    g = np.load(os.path.join(GOLD, f"fa_{name}_b{batch}.npz"))
    cfg = named_config(name + "_fa")
    X, _ = synthetic_batch(cfg, batch)
    ref32, refbf = g["logits"].astype(np.float64), g["logits_autocast"].astype(np.float64)
    m = build(cfg, "bf16").train()
    with torch.no_grad():
        lb, _ = m(X.cuda())
    lb = lb.float().cpu().numpy().astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean(np.square(a))))
    hip_dev, ref_dev = np.abs(lb - ref32).max(), np.abs(refbf - ref32).max()
    hip_rms, ref_rms = rms(lb - ref32), rms(refbf - ref32)
    print(f"[fa autocast {name} B={batch}] |HIP_bf16 - ref_fp32| max {hip_dev:.3e} rms {hip_rms:.3e};  "
          f"|ref_autocast_bf16 - ref_fp32| max {ref_dev:.3e} rms {ref_rms:.3e}")
    assert hip_dev <= ref_dev, (hip_dev, ref_dev)
    assert hip_rms <= ref_rms, (hip_rms, ref_rms)


def test_base_fp32_logits_match_reference_golden():
    g = np.load(os.path.join(GOLD, "fa_base_b2.npz"))
    cfg = named_config("base_fa")
    X, _ = synthetic_batch(cfg, 2)
    m = build(cfg, "fp32").train()
    with torch.no_grad():
        logits, _ = m(X.cuda())
    e = np.abs(logits.cpu().numpy() - g["logits"]).max()
    print(f"[fa golden base B=2] fp32 max|dlogit| {e:.3e}")
    assert e <= 2e-5


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_train_step_equals_eager(precision):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("micro_fa")
    X, y = synthetic_batch(cfg, 8)
    X, y = X.cuda(), y.cuda()
    X2, y2 = synthetic_batch(cfg, 8, seed=77)
    X2, y2 = X2.cuda(), y2.cuda()
    me, mg = build(cfg, precision), build(cfg, precision)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    warm = 2
    for _ in range(warm):
        train_step(me, oe, X, y)
    gs = GraphedTrainStep(mg, og, X, y, warmup=warm)
    for (xb, yb) in ((X, y), (X2, y2), (X, y)):
        le, losse, _, gne = train_step(me, oe, xb, yb)
        lg, lossg, _, gng = gs(xb, yb)
        assert torch.equal(le, lg), (le - lg).abs().max().item()
        assert torch.equal(losse, lossg)
        assert torch.equal(gne, gng)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
    for grp in oe.param_groups:
        grp["lr"] = 5e-4
    gs.set_lr(5e-4)
    train_step(me, oe, X2, y2)
    gs(X2, y2)
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n
