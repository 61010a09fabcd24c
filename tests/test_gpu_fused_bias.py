"""GPU: the bias of the fused GEMM epilogues (SwiGLU, gate-only SwiGLU, q/k/v normalise + head split) and the model
routes it opens (ViTConfig.bias=True on the fused forward paths).

Op level, at the smallest shapes at which the bias index can go wrong:
  SwiGLU   M=300, F=256 (N=2F=512), K=128: one full and one 44-row ragged row tile, two column tiles (n_base != 0);
  q/k/v    C=256, H=4, d=64, T=49, Bsz=6 (M=294), K=256: a tile's rows cross batch boundaries; as one stacked launch
           (nparts=3) and as the cross-attention pair (q alone, then k|v with part0=1), with sqk and split-only, always with
           a q_prescale other than 1.
Exact data: the launch with a bias against the bias-free launch on operands with the bias appended as 64 more K columns
(A' = [A | 1 0..0], B' = [B | b 0..0]) - both accumulators hold the same integers, so every output must be the same
bits - and against the fp64 result.  Gaussian data: against fp64 with the bars of the bias-free tests of these
epilogues (test_gpu_ops.py::test_fused_gemm_swiglu_and_qknorm_match_unfused, gemm_check.check_gauss).
Model level: mini / mini_vit at n_embd=256, bf16, B=336 with non-zero biases: the bias=True model launches the GEMM
families its bias=False twin launches, and agrees with the unfused route and with the CPU references."""
import math

import pytest
import torch

import gemm_check as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16T = torch.bfloat16
NAN = float("nan")


def ops_():
    from nvit_amd import ops
    return ops


def _dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _augment(A, B, bias):
    """[A | 1 0..0], [B | bias 0..0]: 64 more K columns (one K slab of the kernel) that add bias[n] to every sum."""
    ea = torch.zeros(A.shape[0], 64)
    ea[:, 0] = 1.0
    eb = torch.zeros(B.shape[0], 64)
    eb[:, 0] = bias
    return torch.cat([A, ea], 1), torch.cat([B, eb], 1)


def _swiglu_gate64(z, F):
    """fp64 gate of interleaved pre-activations z [M, 2F] (already scaled): u16|v16 column groups -> [M, F]."""
    zz = z.reshape(z.shape[0], F // 16, 2, 16)
    return (zz[:, :, 0] * (zz[:, :, 1] * torch.sigmoid(zz[:, :, 1]))).reshape(z.shape[0], F)


# ------------------------------------------------------------------------------------------------ SwiGLU (EPI 3 / 6)
SW_M, SW_F, SW_K = 300, 256, 128


def _swiglu_gauss(seed=0):
    """bf16-rounded Gaussian operands, a gate scale, and a Gaussian bias of the pre-activations' own scale
    (std sqrt(K) * 0.05)."""
    A = gc.gauss_data((SW_M, SW_K), seed + 1).to(BF16T)
    W = (gc.gauss_data((2 * SW_F, SW_K), seed + 2) * 0.05).to(BF16T)
    gs = 1 + 0.1 * gc.gauss_data((2 * SW_F,), seed + 3)
    b = gc.gauss_data((2 * SW_F,), seed + 4) * (math.sqrt(SW_K) * 0.05)
    return A, W, gs, b


@pytest.mark.parametrize("use_gs", [True, False])
def test_swiglu_bias_exact_vs_k_augmented_bias_free(use_gs):
    """FAILS WITHOUT THE FEATURE.  No tolerance: uv, xm (EPI 3) and xm (EPI 6) with bias=b are the bits of the bias-free
    launch on the K-augmented operands, and uv is the single bf16 rounding of the exact fp64 A B^T + b."""
    ops = ops_()
    M, F, K = SW_M, SW_F, SW_K
    d = gc.nt_exact(M, 2 * F, K, 40, bias=True)          # require_exact: |sum| + |bias| < 2^24
    gc.require_exact(K + 64, 4, 8)                       # ... and the augmented sum (|b| <= 8 in the B' column)
    A2, B2 = _augment(d["A"], d["B"], d["bias"])
    A, B, A2, B2 = (_dev(t, BF16T) for t in (d["A"], d["B"], A2, B2))
    b = _dev(d["bias"])
    gs = _dev(1 + 0.1 * gc.gauss_data((2 * F,), 41)) if use_gs else None
    gscale = 1.5 if use_gs else 1.0
    uv, xm = ops.gemm_nt_swiglu(A, B, M, F, K, gs, gscale, bias=b)
    xa = ops.gemm_nt_swiglu_act(A, B, M, F, K, gs, gscale, bias=b)
    uv2, xm2 = ops.gemm_nt_swiglu(A2, B2, M, F, K + 64, gs, gscale)
    xa2 = ops.gemm_nt_swiglu_act(A2, B2, M, F, K + 64, gs, gscale)
    uv0, _ = ops.gemm_nt_swiglu(A, B, M, F, K, gs, gscale)
    torch.cuda.synchronize()
    assert torch.equal(uv, uv2) and torch.equal(xm, xm2) and torch.equal(xa, xa2)
    assert not torch.equal(uv, uv0), "the bias changed nothing: the case shows nothing"
    ref, _ = gc.nt_ref(d["A"], d["B"], bias=d["bias"])
    gc.assert_exact(uv.cpu(), ref, "uv = A B^T + bias")
    assert torch.isfinite(xm.float()).all()


def test_swiglu_zero_bias_is_no_bias_and_act_matches_full():
    """bias=zeros gives the bits of bias=None; with a bias the gate-only epilogue (EPI 6) writes the xm of the full one
    (EPI 3)."""
    ops = ops_()
    M, F, K = SW_M, SW_F, SW_K
    A, W, gs, b = _swiglu_gauss()
    A, W, gs, b = _dev(A), _dev(W), _dev(gs), _dev(b)
    z = torch.zeros_like(b)
    uv0, xm0 = ops.gemm_nt_swiglu(A, W, M, F, K, gs, 3.0)
    uvz, xmz = ops.gemm_nt_swiglu(A, W, M, F, K, gs, 3.0, bias=z)
    assert torch.equal(uvz, uv0) and torch.equal(xmz, xm0)
    assert torch.equal(ops.gemm_nt_swiglu_act(A, W, M, F, K, gs, 3.0, bias=z), xm0)
    assert torch.equal(ops.gemm_nt_swiglu_act(A, W, M, F, K, gs, 3.0), xm0)
    uvb, xmb = ops.gemm_nt_swiglu(A, W, M, F, K, gs, 3.0, bias=b)
    assert torch.equal(ops.gemm_nt_swiglu_act(A, W, M, F, K, gs, 3.0, bias=b), xmb)
    assert not torch.equal(xmb, xm0)


def test_swiglu_bias_gauss_vs_fp64():
    """Gaussian data against fp64 (A B^T + b, then the gate) from the bf16-rounded operands.  uv is a bf16 store of the
    biased accumulator: gemm_check's bound with the bias in the magnitude (what holds the plain GEMM's bias epilogue, which
    the bias-free test compares uv to).  xm: the bias-free test's bar, 2e-2 * max(1, |x|max)."""
    ops = ops_()
    M, F, K = SW_M, SW_F, SW_K
    A, W, gs, b = _swiglu_gauss()
    Ad, Wd, gsd, bd = _dev(A), _dev(W), _dev(gs), _dev(b)
    uv, xm = ops.gemm_nt_swiglu(Ad, Wd, M, F, K, gsd, 3.0, bias=bd)
    ref, mag = gc.nt_ref(A.float(), W.float(), bias=b)
    gc.check_gauss(uv.cpu(), ref, mag, K, "swiglu uv with bias")
    want = _swiglu_gate64(ref * (gs.double() * 3.0), F)
    err = (xm.cpu().double() - want).abs().max().item()
    print(f"   swiglu xm with bias: max err {err:.3e}, |x|max {want.abs().max().item():.3f}")
    assert err < 2e-2 * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------------ q/k/v (EPI 4)
QK_C, QK_H, QK_D, QK_T, QK_B, QK_K = 256, 4, 64, 49, 6, 256
QK_M = QK_T * QK_B
FORMS = {"stacked": ((3, 0),), "pair": ((1, 0), (2, 1))}   # (nparts, part0) per launch


def _qkv(ops, X, W, bias, sqk, c_q, form, qp, K=QK_K):
    """The q/k/v head tensors of one stacked launch or of the cross-attention pair, into NaN-filled buffers."""
    C = QK_C
    bufs = ops.qk_buffers(1, QK_B, QK_T, QK_H, QK_D, X.device, norm=sqk is not None)
    for t in bufs:
        if t is not None:
            t.fill_(NAN)
    for n, p0 in FORMS[form]:
        rows = slice(p0 * C, (p0 + n) * C)
        ops.gemm_nt_qknorm(X, W[rows], QK_M, K, n, p0, sqk, c_q, QK_B, QK_T, QK_H, QK_D, bufs,
                           q_prescale=(qp if p0 == 0 else 1.0), bias=(None if bias is None else bias[rows]))
    torch.cuda.synchronize()
    return bufs


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _heads64(t):
    """[M, C] token-major (CPU) -> [B, H, T, d]"""
    return t.reshape(QK_B, QK_T, QK_H, QK_D).permute(0, 2, 1, 3)


@pytest.mark.parametrize("norm", [True, False], ids=["sqk", "split"])
@pytest.mark.parametrize("form", list(FORMS))
def test_qkv_bias_exact_vs_k_augmented_bias_free(form, norm):
    """FAILS WITHOUT THE FEATURE.  No tolerance: qh, kh, vh, rq, rk with the stacked bias are the bits of the bias-free
    launch on the K-augmented operands (the normalise runs on the same exact sums in both).  Split-only, k and v are
    also the single bf16 rounding of the exact fp64 result."""
    ops = ops_()
    C, K = QK_C, QK_K
    d = gc.nt_exact(QK_M, 3 * C, K, 50, bias=True)
    gc.require_exact(K + 64, 4, 8)
    X2, W2 = _augment(d["A"], d["B"], d["bias"])
    X, W, X2, W2 = (_dev(t, BF16T) for t in (d["A"], d["B"], X2, W2))
    b = _dev(d["bias"])
    sqk = _dev(1 / 32 + 0.003 * gc.gauss_data((C,), 51)) if norm else None
    c_q = 32.0 if norm else 0.0
    qp = ops.attn_q_prescale(QK_D) if norm else ops.LOG2E / math.sqrt(QK_D)
    got = _qkv(ops, X, W, b, sqk, c_q, form, qp)
    want = _qkv(ops, X2, W2, None, sqk, c_q, form, qp, K=K + 64)
    free = _qkv(ops, X, W, None, sqk, c_q, form, qp)
    for t in got:
        assert t is None or torch.isfinite(t.float()).all()
    assert _same(got, want)
    assert not any(torch.equal(x, y) for x, y in zip(got[:3], free[:3])), "the bias left a part unchanged"
    assert (got[3] is None) == (not norm)
    if not norm:
        ref, _ = gc.nt_ref(d["A"], d["B"], bias=d["bias"])
        gc.assert_exact(got[1].cpu(), _heads64(ref[:, C:2 * C]).contiguous(), "kh = heads(A B^T + bias)")
        gc.assert_exact(got[2].cpu(), _heads64(ref[:, 2 * C:]).contiguous(), "vh = heads(A B^T + bias)")


@pytest.mark.parametrize("norm", [True, False], ids=["sqk", "split"])
@pytest.mark.parametrize("form", list(FORMS))
def test_qkv_bias_zero_and_gauss_vs_fp64(form, norm):
    """bias=zeros gives the bits of bias=None.  Gaussian data and a Gaussian bias of the projections' own scale (std
    sqrt(K) * 0.05) against fp64 (A B^T + b, normalise, sqk * c_q, head split) from the bf16-rounded operands, with the
    bias-free test's bars: normalised q, k 1e-2; raw parts 2e-2 of their largest value; rq, rk 1e-3 of theirs.  q leaves
    multiplied by q_prescale (one rounding of the product), so its bar is that of the unscaled q times q_prescale:
    it is compared after division by q_prescale.  Raw k, v (bf16 stores of the biased accumulator) also hold gemm_check's
    bound with the bias in the magnitude."""
    ops = ops_()
    C, K, M = QK_C, QK_K, QK_M
    X = gc.gauss_data((M, K), 60).to(BF16T)
    W = (gc.gauss_data((3 * C, K), 61) * 0.05).to(BF16T)
    b = gc.gauss_data((3 * C,), 62) * (math.sqrt(K) * 0.05)
    sqk = (1 / 32 + 0.003 * gc.gauss_data((C,), 63)) if norm else None
    c_q = 32.0 if norm else 0.0
    qp = ops.attn_q_prescale(QK_D) if norm else ops.LOG2E / math.sqrt(QK_D)
    Xd, Wd, bd, sd = _dev(X), _dev(W), _dev(b), (None if sqk is None else _dev(sqk))
    assert _same(_qkv(ops, Xd, Wd, torch.zeros_like(bd), sd, c_q, form, qp), _qkv(ops, Xd, Wd, None, sd, c_q, form, qp))
    qh, kh, vh, rq, rk = (None if t is None else t.cpu() for t in _qkv(ops, Xd, Wd, bd, sd, c_q, form, qp))
    ref, mag = gc.nt_ref(X.float(), W.float(), bias=b)
    acc = [_heads64(ref[:, i * C:(i + 1) * C]) for i in range(3)]
    amag = [_heads64(mag[:, i * C:(i + 1) * C]) for i in range(3)]
    e = lambda got, want: (got.double() - want).abs().max().item()
    raw_bar = lambda i: 2e-2 * acc[i].abs().max().item()
    if norm:
        s = (sqk.double() * c_q).reshape(1, QK_H, 1, QK_D)
        nrm = [a.norm(dim=-1, keepdim=True) for a in acc[:2]]
        errs = {"q": e(qh.double() / qp, acc[0] / nrm[0] * s), "k": e(kh, acc[1] / nrm[1] * s)}
        print(f"   qknorm[{form}] with bias: {errs}")
        assert errs["q"] < 1e-2 and errs["k"] < 1e-2
        for got, n_ in ((rq, nrm[0]), (rk, nrm[1])):
            want = (1.0 / n_.squeeze(-1)).permute(0, 2, 1).reshape(M, QK_H)
            assert e(got, want) < 1e-3 * want.abs().max().item()
    else:
        assert rq is None and rk is None
        assert e(qh.double() / qp, acc[0]) < raw_bar(0)
        assert e(kh, acc[1]) < raw_bar(1)
        gc.check_gauss(kh, acc[1].contiguous(), amag[1].contiguous(), K, f"split[{form}] kh with bias")
    assert e(vh, acc[2]) < raw_bar(2)
    gc.check_gauss(vh, acc[2].contiguous(), amag[2].contiguous(), K, f"qkv[{form}] vh with bias")


# ------------------------------------------------------------------------------------------------ wrong bias
def test_wrong_bias_raises_and_launches_nothing():
    ops = ops_()
    A, W, gs, b = _swiglu_gauss()
    A, W, gs, b = _dev(A), _dev(W), _dev(gs), _dev(b)
    X = _dev(gc.gauss_data((QK_M, QK_K), 70), BF16T)
    Wq = _dev(gc.gauss_data((3 * QK_C, QK_K), 71) * 0.05, BF16T)
    bq = _dev(gc.gauss_data((3 * QK_C,), 72))

    def bad(good):
        n = good.numel()
        return {"bf16": good.to(BF16T), "fp64": good.double(), "short": good[:n - 4].contiguous(),
                "long": torch.cat([good, good[:4]]), "strided": torch.cat([good, good])[::2], "2-d": good.reshape(2, -1),
                "host": good.cpu()}

    calls = [(lambda x: ops.gemm_nt_swiglu(A, W, SW_M, SW_F, SW_K, gs, 3.0, bias=x), b),
             (lambda x: ops.gemm_nt_swiglu_act(A, W, SW_M, SW_F, SW_K, gs, 3.0, bias=x), b),
             (lambda x: ops.gemm_nt_qknorm(X, Wq, QK_M, QK_K, 3, 0, None, 0.0, QK_B, QK_T, QK_H, QK_D, bias=x), bq),
             (lambda x: ops.gemm_nt_qknorm(X, Wq[QK_C:], QK_M, QK_K, 2, 1, None, 0.0, QK_B, QK_T, QK_H, QK_D, bias=x),
              bq[QK_C:])]
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_collect()
    try:
        for call, good in calls:
            assert bad(good)["strided"].numel() == good.numel() and not bad(good)["strided"].is_contiguous()
            for what, x in bad(good).items():
                with pytest.raises(ValueError):
                    call(x)
        call, _ = calls[3]
        with pytest.raises(ValueError):
            call(bq)          # the whole stacked bias for a two-part launch
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    launched = {k: v["launches"] for k, v in ops.prof_collect().items() if v["launches"]}
    assert not launched, launched


# ------------------------------------------------------------------------------------------------ model level
MODEL_B = 336
FAMILIES = ("gemm_swiglu", "gemm_qknorm", "gemm_swiglu_act")


def _cfg(kind, bias):
    from nvit_amd.config import named_config
    return named_config(kind, n_embd=256, n_head=4, bias=bias)


def _state(cfg):
    """The formula weights with every block / cross-attention linear bias drawn N(0, 0.02) from a seeded generator."""
    from nvit_amd.weights import formula_state_dict
    sd = formula_state_dict(cfg)
    g = torch.Generator().manual_seed(20240)
    n = 0
    for k in sorted(sd):
        if k.endswith(".bias") and k.startswith(("transformer.h.", "cross_attention.")):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.02
            n += 1
    assert n == (6 * cfg.n_layer + 5 if cfg.bias else 0)
    return sd


def _build(cfg, train=True):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    m.load_state_dict(_state(cfg), strict=True)
    m = m.to(DEV).set_precision("bf16")
    if cfg.use_nvit:
        normalize_matrices(m)
    return m.train() if train else m.eval()


def _batch(cfg):
    from nvit_amd.weights import synthetic_batch
    return synthetic_batch(cfg, MODEL_B)


def _assert_fusable_shape(cfg):
    """The smallest fused candidate, the cross-attention q projection (M x C), clears the size threshold."""
    ops = ops_()
    T = (cfg.image_size // cfg.local_patch_size) ** 2
    assert MODEL_B * T == 16464 and MODEL_B * T * cfg.n_embd >= ops.FUSE_MIN_ELEMS
    assert ops.fusable(1, MODEL_B * T, cfg.n_embd, cfg.n_embd), "test config no longer reaches the fused path"


def _launches(m, X, no_grad):
    ops = ops_()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_collect()
    try:
        if no_grad:
            with torch.no_grad():
                m(X)
        else:
            m(X)
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    prof = ops.prof_collect()
    return {f: prof[f]["launches"] for f in FAMILIES}


@pytest.mark.parametrize("kind", ["mini", "mini_vit"])
def test_bias_model_takes_the_fused_routes_of_its_bias_free_twin(kind):
    """FAILS WITHOUT THE FEATURE.  Launch counts of the fused GEMM families, bias=True against bias=False at the same
    shape: equal and non-zero, in a grad-enabled forward (SwiGLU with the raw store, q/k/v) and under no_grad (gate-only
    SwiGLU, q/k/v).  Under no_grad the logits and aux of the bias=True model are the bits of its grad-enabled forward."""
    counts = {}
    for bias in (True, False):
        cfg = _cfg(kind, bias)
        _assert_fusable_shape(cfg)
        m = _build(cfg, train=False)
        X = _batch(cfg)[0].to(DEV)
        logits, aux = m(X)   # warm-up: shadow tables, LDS attributes
        counts[bias] = (_launches(m, X, no_grad=False), _launches(m, X, no_grad=True))
        if bias:
            with torch.no_grad():
                l0, a0 = m(X)
            assert torch.equal(l0, logits) and set(a0) == set(aux)
            for k in aux:
                assert torch.equal(a0[k], aux[k]), k
    print(f"   [{kind}] fused launches (grad, no_grad): bias {counts[True]}, no bias {counts[False]}")
    assert counts[True] == counts[False]
    grad, lean = counts[False]
    n = _cfg(kind, False).n_layer + 1          # one per block and one for the cross-attention call
    assert grad == {"gemm_swiglu": n, "gemm_qknorm": n + 1, "gemm_swiglu_act": 0}   # cross-attention: q and k|v launches
    assert lean == {"gemm_swiglu": 0, "gemm_qknorm": n + 1, "gemm_swiglu_act": n}


def _reference(cfg, X, y):
    """(logits, {name: grad}) of the CPU reference on the same state: float64 torch restatement (plain ViT); the oracle
    as test_gpu_model.py runs it, matrices renormalised (nViT)."""
    torch.set_num_threads(8)
    if not cfg.use_nvit:
        import vit_torch_ref
        logits, _, _, grads = vit_torch_ref.loss_and_grads(_state(cfg), cfg, X, y)
        return logits.double(), {n: g.double() for n, g in grads.items()}
    from oracle import nvit_oracle as O
    p = O.make_params(_state(cfg))
    O.renorm_(p, cfg)
    logits, _, _ = O.loss_and_grads(p, cfg, X, y, None)
    return logits.detach().double(), {n: t.grad.double() for n, t in p.items() if t.grad is not None}


@pytest.mark.parametrize("kind", ["mini", "mini_vit"])
def test_bias_model_fused_vs_unfused_and_reference(kind):
    """bias=True with non-zero biases on the fused routes: logits and every parameter gradient (all bias gradients
    included) against the same model with the fusions off - the bars of
    test_gpu_vit_baseline.py::test_bf16_fused_route_vs_unfused_and_fp64: logits 5e-3, gradients 5 % of their error scale
    (the stacked q/k/v gradient for a block's q, k, v) - and against the CPU reference with that reference's own test's
    bars: plain ViT (float64) logits 1e-2, gradients 10 % of the same scale; nViT (oracle,
    test_gpu_model.py::test_bf16_fused_epilogues_match_unfused_and_oracle) logits 1.5e-3, gradient cosine > 0.98."""
    ops = ops_()
    cfg = _cfg(kind, True)
    _assert_fusable_shape(cfg)
    X, y = _batch(cfg)
    ref_logits, ref_grads = _reference(cfg, X, y)

    def run(fuse_min):
        old = ops.FUSE_MIN_ELEMS
        ops.FUSE_MIN_ELEMS = fuse_min
        try:
            m = _build(cfg)
            logits, _ = m(X.to(DEV))
            torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()
            return logits.detach().double().cpu(), {n: q.grad.double().cpu() for n, q in m.named_parameters()
                                                     if q.grad is not None}
        finally:
            ops.FUSE_MIN_ELEMS = old

    lf, gf = run(ops.FUSE_MIN_ELEMS)
    lu, gu = run(1 << 62)
    e_ref = (lf - ref_logits).abs().max().item()
    e_fu = (lf - lu).abs().max().item()
    print(f"   [{kind} bias] max|dlogit| vs reference {e_ref:.3e} (unfused {(lu - ref_logits).abs().max().item():.3e}), "
          f"fused vs unfused {e_fu:.3e}, logit max {ref_logits.abs().max().item():.3f}")
    assert e_fu < 5e-3
    assert e_ref < (1.5e-3 if cfg.use_nvit else 1e-2)
    assert sorted(gf) == sorted(gu) == sorted(ref_grads)
    nbias = [n for n in gf if n.endswith(".bias") and n.startswith(("transformer.h.", "cross_attention."))]
    assert len(nbias) == 6 * cfg.n_layer + 5

    def scale_of(n):
        parts = n.split(".")
        if parts[0] == "transformer" and parts[3] in ("query", "key", "value"):
            pre, leaf = ".".join(parts[:3]), parts[4]
            return math.sqrt(sum(ref_grads[f"{pre}.{k}.{leaf}"].norm().item() ** 2 for k in ("query", "key", "value")))
        return ref_grads[n].norm().item()

    worst_r, worst_u, worst_cos = 0.0, 0.0, 1.0
    fails = []
    for n, r in ref_grads.items():
        sc = scale_of(n)
        if sc < 1e-12:
            continue
        a, b, r = gf[n].flatten(), gu[n].flatten(), r.flatten()
        e_r = (a - r).norm().item() / sc
        e_u = (a - b).norm().item() / sc
        cos = (a @ r / (a.norm() * r.norm() + 1e-30)).item() if r.norm() >= 1e-12 else 1.0
        worst_r, worst_u, worst_cos = max(worst_r, e_r), max(worst_u, e_u), min(worst_cos, cos)
        ok = e_u < 0.05 and (cos > 0.98 if cfg.use_nvit else e_r < 0.1)
        if not ok:
            fails.append((n, e_r, e_u, cos))
    print(f"   worst relative gradient error vs reference {worst_r:.4f}, fused vs unfused {worst_u:.4f}"
          + (f", worst cosine vs reference {worst_cos:.5f}" if cfg.use_nvit else ""))
    assert not fails, fails
