"""Attention at head dims 32 and 128: the MFMA kernels (impl 1) and the scalar-FMA kernels (impl 0, d = 128) against
fp32 SDPA math with the bars of test_gpu_ops.py::test_attention / test_attention_bounded_scores, on ragged and degenerate
lengths (impl 0 also with Tq != Tk, at every head dim), with operands inside NaN padding and outputs inside sentinel
padding; bitwise run-to-run reproducibility (also at d = 64); and the model at d = 128 and d = 32 against the CPU oracle
with the bars of test_gpu_model.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch
from oracle import nvit_oracle as O

# the padding harness (NaN operand margins, sentinel output margins); test_gpu_heads_pad.py takes it from here
from attn_check import PAD, SENTINEL, Padded, operand, output, run_bwd, run_fwd   # noqa: F401


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _sdpa_ref(qh, kh, vh, scale):
    s = (qh @ kh.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    return p @ vh, torch.logsumexp(s, dim=-1)


def _inputs(dtype, B, H, T, d, Tk=None):
    # |q|=|k|=1.3 per head: logits up to sqrt(d)*1.69 (as test_attention)
    Tk = T if Tk is None else Tk
    q = (1.3 * torch.nn.functional.normalize(rnd(B, H, T, d, seed=1), dim=-1)).to(dtype)
    k = (1.3 * torch.nn.functional.normalize(rnd(B, H, Tk, d, seed=2), dim=-1)).to(dtype)
    v = rnd(B, H, Tk, d, seed=3).to(dtype)
    g = rnd(B, H, T, d, seed=4).to(dtype)
    return q, k, v, g


SHAPES = [(2, 2, 1), (2, 3, 16), (3, 2, 49), (2, 2, 130), (2, 3, 257), (2, 2, 784)]
CASES = ([(torch.bfloat16, 1, d, B, H, T) for d in (32, 128) for (B, H, T) in SHAPES] +
         [(dt, 0, 128, B, H, T) for dt in (torch.float32, torch.bfloat16) for (B, H, T) in SHAPES])


@pytest.mark.parametrize("dtype,impl,d,B,H,T", CASES)
def test_attention_head_dim(dtype, impl, d, B, H, T):
    _check_head_dim(dtype, impl, d, B, H, T, math.sqrt(d))


@pytest.mark.parametrize("d", [32, 128])
def test_attention_head_dim_unit_scale(d):
    """scale * log2(e) == 1 with q not pre-scaled: the backward kernels take their UNIT variant (-lse as the initial
    accumulator of the score product), which the generic entry reaches at no other scale.  Same reference and bars."""
    _check_head_dim(torch.bfloat16, 1, d, 2, 2, 130, math.log(2.0))


# Tk = 33: a full 32-key LDS tile and a one-key tile.  Tq = 65: a full 64-row workgroup and one with a single live row (at
# d = 128, four lanes per row, five workgroups of 16 rows).  Tq = 1: the single query.  B, H > 1: the b / h indexing.
UNEQUAL = [(dt, d, B, H, Tq, Tk) for d in (32, 64, 128) for dt in (torch.float32, torch.bfloat16)
           for (B, H, Tq, Tk) in [(2, 2, 17, 33), (2, 2, 65, 32), (2, 3, 1, 40)]]


@pytest.mark.parametrize("dtype,d,B,H,Tq,Tk", UNEQUAL)
def test_attention_scalar_unequal_lengths(dtype, d, B, H, Tq, Tk):
    """impl 0 forward and backward with Tq != Tk: same fp64 reference, padding harness and bars as above."""
    _check_head_dim(dtype, 0, d, B, H, Tq, math.sqrt(d), Tk=Tk)


def _check_head_dim(dtype, impl, d, B, H, T, scale, Tk=None):
    from nvit_amd.ops import dt_of
    q, k, v, g = _inputs(dtype, B, H, T, d, Tk)
    # (the reference runs in fp64 on the same operands: at d = 128 an fp32 evaluation of the same formula is itself
    #  1.8e-6 - 3.3e-6 away from the exact result on these inputs, at or above the fp32 bar of 2e-6)
    qf, kf, vf = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, lse_ref = _sdpa_ref(qf, kf, vf, scale)
    o_ref.backward(g.double())
    dt = dt_of(q)
    o, lse = run_fwd(dt, impl, q, k, v, scale)
    o_bhtd = o.float().cpu().reshape(B, T, H, d).permute(0, 2, 1, 3)
    tol = 2e-6 if dtype == torch.float32 else 1e-2
    assert (o_bhtd.double() - o_ref.detach()).abs().max().item() < tol
    assert (lse.cpu().double() - lse_ref.detach()).abs().max().item() < 1e-4
    g_tok = g.permute(0, 2, 1, 3).reshape(B * T, H * d).contiguous()
    dq, dk, dv = run_bwd(dt, impl, g_tok, q, k, v, o, lse, scale)
    tolg = 5e-5 if dtype == torch.float32 else 3e-2
    for name, got, ref in (("dq", dq, qf.grad), ("dk", dk, kf.grad), ("dv", dv, vf.grad)):
        e = (got.double().cpu() - ref).abs().max().item()
        lim = tolg * max(1.0, ref.abs().max().item())
        assert e < lim, f"{name}: err {e:.3e} >= {lim:.3e}"


# smul: scale of the learned per-channel factor.  The score bound grows with sqrt(d): 1.0 and 1.6 (1.4 at d = 128) stay
# within the fast path's range, 3.0 exceeds it and takes the online-softmax fallback.
BOUNDED = [(d, B, H, T, smul, pre) for d, smuls in ((32, (1.0, 1.6, 3.0)), (128, (1.0, 1.4, 3.0)))
           for (B, H, T) in [(2, 3, 784), (1, 2, 130), (1, 1, 16), (2, 2, 64), (2, 2, 49)]
           for smul in smuls for pre in (False, True)]


@pytest.mark.parametrize("d,B,H,T,smul,prescale", BOUNDED)
def test_attention_bounded_scores_head_dim(d, B, H, T, smul, prescale):
    """nvit_attn_fwd_bounded at d = 32 / 128 with the structure and bars of test_attention_bounded_scores; prescale: qh
    holds attn_q_prescale(d) * q_hat (the UNIT branch)."""
    from nvit_amd import ops
    from nvit_amd._lib import BF16
    C = H * d
    c_q = 32.0
    sqk = (smul / 32.0) * (1.0 + 0.3 * torch.tanh(rnd(C, seed=7)))
    s_eff = (sqk * c_q).reshape(1, H, 1, d)
    qpre = ops.attn_q_prescale(d) if prescale else 1.0
    q_in = (qpre * s_eff * torch.nn.functional.normalize(rnd(B, H, T, d, seed=1), dim=-1)).bfloat16()
    k = (s_eff * torch.nn.functional.normalize(rnd(B, H, T, d, seed=2), dim=-1)).bfloat16()
    v = rnd(B, H, T, d, seed=3).bfloat16()
    q = q_in.float() / qpre
    scale = math.sqrt(d)
    tb = scale * 1.4426950408889634 * (sqk * c_q).reshape(H, d).abs().max(dim=-1).values.max().item() ** 2
    fast = tb <= 60.0
    assert fast == (smul < 3.0)
    o_ref, lse_ref = _sdpa_ref(q, k.float(), v.float(), scale)
    o, lse = run_fwd(BF16, 1, q_in, k, v, scale, sqk, c_q, qpre)
    o2, lse2 = run_fwd(BF16, 1, q.bfloat16(), k, v, scale)
    o_bhtd = o.float().cpu().reshape(B, T, H, d).permute(0, 2, 1, 3)
    lse_tol = 4e-3 if fast else 1e-4 * max(1.0, lse_ref.abs().max().item())
    o_tol = 1e-2 + 2.0 ** -7 * o_ref.abs().max().item()
    assert (o_bhtd - o_ref).abs().max().item() < o_tol
    assert (lse.cpu() - lse_ref).abs().max().item() < lse_tol
    if not prescale:   # (with the pre-scale, q.bfloat16() is a second rounding of q_in / qpre)
        assert (o.float() - o2.float()).abs().max().item() < o_tol
        assert (lse - lse2).abs().max().item() < lse_tol
    # spike: one key aligned with one query at the largest possible score must not overflow
    q2, k2 = q_in.clone(), k.clone()
    k2[0, 0, T // 2] = (q2[0, 0, 0].float() / qpre).bfloat16()
    o3, lse3 = run_fwd(BF16, 1, q2, k2, v, scale, sqk, c_q, qpre)
    o3_ref, lse3_ref = _sdpa_ref(q2.float() / qpre, k2.float(), v.float(), scale)
    assert torch.isfinite(o3.float()).all() and torch.isfinite(lse3).all()
    o3_bhtd = o3.float().cpu().reshape(B, T, H, d).permute(0, 2, 1, 3)
    assert (o3_bhtd - o3_ref).abs().max().item() < 1e-2 + 2.0 ** -7 * o3_ref.abs().max().item()
    assert (lse3.cpu() - lse3_ref).abs().max().item() < lse_tol


@pytest.mark.parametrize("d", [32, 64, 128])
def test_attention_head_dim_bitwise_reproducible(d):
    from nvit_amd import ops
    from nvit_amd._lib import BF16
    B, H, T = 2, 3, 784
    q, k, v, g = (x.to(dev()) for x in _inputs(torch.bfloat16, B, H, T, d))
    g_tok = g.permute(0, 2, 1, 3).reshape(B * T, H * d).contiguous()
    scale = math.sqrt(d)
    sqk = ((1.0 / 32.0) * (1.0 + 0.3 * torch.tanh(rnd(H * d, seed=7)))).to(dev())
    runs = []
    for _ in range(2):
        o, lse = ops.attn_fwd(BF16, 1, q, k, v, scale)
        ob, lseb = ops.attn_fwd(BF16, 1, q, k, v, scale, sqk, 32.0, q_prescale=ops.attn_q_prescale(d))
        runs.append((o, lse, ob, lseb) + tuple(ops.attn_bwd(BF16, 1, g_tok, q, k, v, o, lse, scale)))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- model level
def build(cfg, precision, renormed):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision)
    if renormed:
        normalize_matrices(m)
    return m


def oracle_run(cfg, X, y, renormed, lowp=None):
    p = O.make_params(formula_state_dict(cfg))
    if renormed:
        O.renorm_(p, cfg)
    logits, loss, recon = O.loss_and_grads(p, cfg, X, y, lowp)
    return p, logits, loss, recon


MODEL_CASES = [("d128", dict(n_embd=256, n_head=2), 4), ("d32", dict(n_embd=128, n_head=4), 4)]


@pytest.mark.parametrize("tag,over,batch", MODEL_CASES)
def test_fp32_model_head_dim_vs_oracle(tag, over, batch):
    torch.set_num_threads(8)
    cfg = named_config("mini", **over)
    assert not cfg.bias
    X, y = synthetic_batch(cfg, batch)
    p, logits_ref, loss_ref, recon_ref = oracle_run(cfg, X, y, True)
    m = build(cfg, "fp32", True).train()
    assert m._attn_impl() == 0
    logits, aux = m(X.cuda())
    loss = torch.nn.functional.cross_entropy(logits, y.cuda())
    loss.backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    print(f"[fp32 mini {tag}] max|dlogit|={err:.3e}")
    assert err < 1e-5
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    assert abs(aux["reconstruction"].item() - recon_ref.item()) < 1e-5
    have = {n for n, q in m.named_parameters() if q.grad is not None}
    want = {n for n, t in p.items() if t.grad is not None}
    assert have == want
    for n, q in m.named_parameters():
        if q.grad is None:
            continue
        ref = p[n].grad
        e = (q.grad.cpu() - ref).abs().max().item()
        s = ref.abs().max().item()
        assert e <= 2e-4 * s + 1e-8, (n, e, s)


@pytest.mark.parametrize("tag,over,batch", MODEL_CASES)
def test_bf16_model_head_dim_vs_oracle(tag, over, batch):
    cfg = named_config("mini", **over)
    X, y = synthetic_batch(cfg, batch)
    p, logits_ref, loss_ref, _ = oracle_run(cfg, X, y, True)
    pe, logits_emu, _, _ = oracle_run(cfg, X, y, True, lowp=O.bf16_round)
    m = build(cfg, "bf16", True).train()
    assert m._attn_impl() == 1
    logits, aux = m(X.cuda())
    loss = torch.nn.functional.cross_entropy(logits, y.cuda())
    loss.backward()
    err = (logits.detach().cpu() - logits_ref).abs().max().item()
    err_emu = (logits.detach().cpu() - logits_emu).abs().max().item()
    d_emu = (logits_emu - logits_ref).abs().max().item()
    print(f"[bf16 mini {tag}] max|dlogit| vs fp32 oracle {err:.3e}, vs bf16-operand oracle {err_emu:.3e} (d_emu {d_emu:.3e})")
    assert err_emu < 1e-3, (err_emu, d_emu)
    assert err < d_emu + 5e-4, (err, d_emu)
    for n, q in m.named_parameters():
        if q.grad is None:
            continue
        a, b = q.grad.cpu().flatten().double(), p[n].grad.flatten().double()
        if b.norm() < 1e-12:
            continue
        cos = (a @ b / (a.norm() * b.norm() + 1e-30)).item()
        assert cos > 0.98, (n, cos)


def test_bf16_train_step_head_dim_128():
    from nvit_amd.train import train_step
    cfg = named_config("mini", n_embd=256, n_head=2)
    X, y = synthetic_batch(cfg, 4)
    m = build(cfg, "bf16", True).train()
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    _, loss, _, gnorm = train_step(m, opt, X.cuda(), y.cuda(), 1.0)
    assert torch.isfinite(loss).item() and torch.isfinite(gnorm).item()
    for blk in m.transformer.h:
        for lin, dim in ((blk.query, 1), (blk.key, 1), (blk.value, 1), (blk.c_fc, 1), (blk.att_c_proj, 0),
                         (blk.mlp_c_proj, 0)):
            assert (lin.weight.detach().norm(dim=dim) - 1).abs().max().item() < 1e-5
