"""GPU, op level: the zero-padded-head row kernels (heads_pad_fwd / heads_pad_bwd / pad_cols / unpad_cols) that let head
dims 72, 80, 88 and 104 run on the 128-wide attention kernels, and those attention kernels on the padded tensors.

Row kernels: against the fp64 references and per-element bounds that tests/rowops_check.py gives the qknorm cases (the
formulas are the same; only the memory layout differs), operands inside NaN margins, outputs inside sentinel margins
and pre-filled with NaN: afterwards every pad column is exactly zero and every real column finite.
Attention: nvit_attn_fwd / _fwd_bounded / _bwd at D = 128 on tensors the split kernel wrote, against SDPA math on the
compact d-wide tensors at the softmax scale of the REAL d, with the bars of tests/test_gpu_attn_headdim.py; a reference
at the scale of the padded width is rejected by the same bars."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_check as rc
import test_gpu_attn_headdim as AH
from test_gpu_attn_headdim import Padded

F32T, F64T, BF16T = torch.float32, torch.float64, torch.bfloat16
NAN = float("nan")
DP = 128
# (d, H): a head of 20 float4 lanes straddles the 64-lane boundary of the compact row; a ragged last vector; 88; C = 1664;
# C = 1920, the widest
HEADS = [(80, 4), (72, 8), (88, 8), (104, 16), (80, 24)]
BT = [(1, 1), (2, 49), (3, 16)]


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def modes():
    from nvit_amd import _lib
    return _lib.F32, _lib.BF16, _lib.BF16_F32IN


def D(t):
    return None if t is None else t.to(dev())


def nan_filled(shape, dtype):
    """an output buffer inside sentinel margins whose own elements are NaN before the call"""
    p = Padded(shape, dtype, AH.SENTINEL)
    p.t.fill_(NAN)
    return p


def projections(c, layout):
    """q | k | v [M, C] fp32 inside NaN margins: one stacked [M, 3C] buffer, or the cross-attention pair [M, C] / [M, 2C].
    -> (q, ldq, k, v, ldkv, keep-alive)"""
    C = c["H"] * c["d"]
    if layout == "stacked":
        p = Padded((c["q"].shape[0], 3 * C), F32T, NAN, torch.cat([c["q"], c["k"], c["v"]], dim=1))
        return p.t, 3 * C, p.t[:, C:], p.t[:, 2 * C:], 3 * C, (p,)
    pq = Padded(tuple(c["q"].shape), F32T, NAN, c["q"])
    pkv = Padded((c["q"].shape[0], 2 * C), F32T, NAN, torch.cat([c["k"], c["v"]], dim=1))
    return pq.t, C, pkv.t, pkv.t[:, C:], 2 * C, (pq, pkv)


def grad_outputs(M, C, layout, dtype):
    """dq | dk | dv destinations, NaN-filled inside sentinel margins, laid out like the projections"""
    if layout == "stacked":
        p = nan_filled((M, 3 * C), dtype)
        return p.t, 3 * C, p.t[:, C:], p.t[:, 2 * C:], 3 * C, (p,)
    pq, pkv = nan_filled((M, C), dtype), nan_filled((M, 2 * C), dtype)
    return pq.t, C, pkv.t, pkv.t[:, C:], 2 * C, (pq, pkv)


def split(c, mode, layout, norm):
    """heads_pad_fwd into NaN-filled buffers -> dict of the Padded outputs (None where the call has none)"""
    ops = ops_()
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    out_dt = F32T if mode == modes()[0] else BF16T
    q, ldq, k, v, ldkv, keep = projections(c, layout)
    bufs = {n: nan_filled((B, H, T, DP), out_dt) for n in ("qh", "kh", "vh")}
    if norm:
        bufs.update(rq=nan_filled((B * T, H), F32T), rk=nan_filled((B * T, H), F32T), sqk_pad=nan_filled((H * DP,), F32T))
    out = tuple(bufs[n].t if n in bufs else None for n in ("qh", "kh", "vh", "rq", "rk", "sqk_pad"))
    res = ops.heads_pad_fwd(mode, q, ldq, k, ldkv, v, ldkv, D(c["sqk"]) if norm else None, c["c_q"], B, T, H, d, out=out)
    torch.cuda.synchronize()
    for a, b in zip(res, out):
        assert (a is None and b is None) or a.data_ptr() == b.data_ptr()
    for n, p in bufs.items():
        assert p.margins_intact(), f"{n}: wrote outside its buffer"
    return bufs


def assert_pads_zero(bufs, d, label):
    for n in ("qh", "kh", "vh"):
        t = bufs[n].t
        assert (t[..., d:] == 0).all(), f"{label}: pad columns of {n} are not all zero"
        assert torch.isfinite(t[..., :d].float()).all(), f"{label}: {n} has a non-finite real column"
    if "sqk_pad" in bufs:
        s = bufs["sqk_pad"].t.reshape(-1, DP)
        assert (s[:, d:] == 0).all(), f"{label}: pad entries of the padded sqk are not zero"


def run_case(c, mode, layout, norm, nblk, label):
    """Forward and backward of one case.  mode F32: fp32 head tensors, backward in F32 against both references;
    BF16_F32IN: bf16 head tensors, the backward runs in BF16 from the forward's own outputs."""
    ops = ops_()
    F32, BF16, _ = modes()
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    M, C = B * T, H * d
    out_dt = F32T if mode == F32 else BF16T
    c = dict(c, **{n: c[n].to(out_dt) for n in ("gq", "gk", "gv")})   # the incoming gradients are exact inputs too
    bufs = split(c, mode, layout, norm)
    assert_pads_zero(bufs, d, label)
    qh, kh, vh = (bufs[n].t for n in ("qh", "kh", "vh"))
    heads_of = lambda x: rc.to_heads(x, B, T, H, d).to(out_dt).contiguous()
    assert rc.bits_equal(vh[..., :d].cpu().contiguous(), heads_of(c["v"])), f"{label}: vh is not a copy of v"
    if norm:
        ref = rc.qknorm_eval(c)
        _, bnd = rc.qknorm_bounds(c)
        got = {"qh": qh[..., :d], "kh": kh[..., :d], "rq": bufs["rq"].t, "rk": bufs["rk"].t}
        rc.check_all(got, ref, {n: bnd[n] for n in got}, label + " fwd")
        want = torch.zeros(H, DP)
        want[:, :d] = c["sqk"].reshape(H, d)
        assert rc.bits_equal(bufs["sqk_pad"].t.cpu().reshape(H, DP), want), f"{label}: padded sqk"
    else:
        assert rc.bits_equal(qh[..., :d].cpu().contiguous(), heads_of(c["q"])), f"{label}: qh is not a copy of q"
        assert rc.bits_equal(kh[..., :d].cpu().contiguous(), heads_of(c["k"])), f"{label}: kh is not a copy of k"
    # ---- backward: gradients whose pad columns hold NaN (the merge reads the first d columns only)
    grads = {}
    for n in ("gq", "gk", "gv"):
        p = Padded((B, H, T, DP), out_dt, NAN)
        p.t.fill_(NAN)
        p.t[..., :d] = D(c[n])
        grads[n] = p
    bdt = F32 if mode == F32 else BF16
    dq, lddq, dk, dv, lddkv, outs = grad_outputs(M, C, layout, out_dt)
    part_buf = nan_filled((nblk if nblk is not None else min(1024, math.ceil(M / 4)), C), F32T) if norm else None
    part = ops.heads_pad_bwd(bdt, grads["gq"].t, grads["gk"].t, grads["gv"].t, qh, kh, bufs["rq"].t if norm else None,
                             bufs["rk"].t if norm else None, D(c["sqk"]) if norm else None, c["c_q"], dq, lddq, dk,
                             lddkv, dv, lddkv, B, T, H, d, nblk=nblk, out=part_buf.t if norm else None)
    torch.cuda.synchronize()
    for p in outs + ((part_buf,) if norm else ()):
        assert p.margins_intact(), f"{label}: the backward wrote outside its buffers"
    dq, dk, dv = dq[:, :C], dk[:, :C], dv[:, :C]
    assert rc.bits_equal(dv.cpu().contiguous(), rc.from_heads(c["gv"], B, T, H, d).contiguous()), f"{label}: dv is not a copy of dvh"
    if not norm:
        assert part is None
        assert rc.bits_equal(dq.cpu().contiguous(), rc.from_heads(c["gq"], B, T, H, d).contiguous()), f"{label}: dq"
        assert rc.bits_equal(dk.cpu().contiguous(), rc.from_heads(c["gk"], B, T, H, d).contiguous()), f"{label}: dk"
        return
    assert part.data_ptr() == part_buf.t.data_ptr()
    dsqk = torch.full((C,), NAN, device=dev())
    ops.colsum_reduce(part, dsqk, False, kind=0, scale=c["c_q"])
    got = {"dq": dq, "dk": dk, "dsqk": dsqk}
    given = {"qh": qh[..., :d].cpu().contiguous(), "kh": kh[..., :d].cpu().contiguous(), "rq": bufs["rq"].t.cpu(),
             "rk": bufs["rk"].t.cpu()}
    _, bnd2 = rc.qknorm_bounds(c, given)
    rc.check_all(got, rc.qknorm_bwd_formula(c, given, F64T), bnd2, label + " bwd (formula on the kernel's tensors)")
    if mode == F32:
        rc.check_all(got, ref, {n: bnd[n] for n in got}, label + " bwd (autograd)")


@pytest.mark.parametrize("d,H", HEADS)
def test_heads_pad_fwd_bwd_types_strides_rows(d, H):
    F32, _, BF16_F32IN = modes()
    for (B, T), layout in zip(BT, ("stacked", "cross", "stacked")):
        c = rc.qk_case(B, T, H, d, 300 + d + H)
        for mode in (F32, BF16_F32IN):
            for norm in (True, False):
                run_case(c, mode, layout, norm, None, f"heads_pad d{d} H{H} B{B} T{T} mode={mode} {layout} norm={norm}")
    # the other layout at the ragged row count, and 12 waves that walk 8 or 9 rows each (98 rows, 3 workgroups)
    c = rc.qk_case(2, 49, H, d, 310 + d + H)
    run_case(c, BF16_F32IN, "cross", True, 3, f"heads_pad d{d} H{H} M98 cross nblk=3")
    run_case(c, F32, "stacked", True, 3, f"heads_pad d{d} H{H} M98 stacked nblk=3")


@pytest.mark.parametrize("d,H", [(80, 4), (104, 16)])
def test_heads_pad_calls_are_bitwise_reproducible(d, H):
    F32, BF16, BF16_F32IN = modes()
    ops = ops_()
    B, T = 2, 49
    c = rc.qk_case(B, T, H, d, 77)
    M, C = B * T, H * d
    runs = []
    for _ in range(2):
        bufs = split(c, BF16_F32IN, "stacked", True)
        qh, kh, vh = (bufs[n].t for n in ("qh", "kh", "vh"))
        g = [torch.zeros((B, H, T, DP), dtype=BF16T, device=dev()) for _ in range(3)]
        for t, n in zip(g, ("gq", "gk", "gv")):
            t[..., :d] = D(c[n]).bfloat16()
        dqkv = torch.full((M, 3 * C), NAN, dtype=BF16T, device=dev())
        part = ops.heads_pad_bwd(BF16, g[0], g[1], g[2], qh, kh, bufs["rq"].t, bufs["rk"].t, D(c["sqk"]), c["c_q"], dqkv,
                                 3 * C, dqkv[:, C:], 3 * C, dqkv[:, 2 * C:], 3 * C, B, T, H, d)
        o = ops.unpad_cols(vh.permute(0, 2, 1, 3).reshape(M, H * DP).contiguous(), M, H, d)
        runs.append([bufs[n].t.clone() for n in ("qh", "kh", "vh", "rq", "rk", "sqk_pad")] + [dqkv, part, o,
                                                                                               ops.pad_cols(o, M, H, d)])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("dtype", [F32T, BF16T])
@pytest.mark.parametrize("d,H,M", [(80, 4, 1), (72, 8, 98), (104, 16, 48), (80, 24, 37)])
def test_unpad_then_pad_is_the_identity_on_real_columns(d, H, M, dtype):
    """O unpad [M, H*128] -> [M, C], then dO pad of the same data back: the real columns come back bit for bit, every
    pad column is exactly zero whatever the source held there (NaN here) and whatever the destination held before."""
    ops = ops_()
    src = Padded((M, H * DP), dtype, NAN)
    src.t.fill_(NAN)
    data = AH.rnd(M, H, d, seed=d + H + M).to(dtype)
    src.t.view(M, H, DP)[..., :d] = data.to(dev())
    mid, back = nan_filled((M, H * d), dtype), nan_filled((M, H * DP), dtype)
    assert ops.unpad_cols(src.t, M, H, d, out=mid.t).data_ptr() == mid.t.data_ptr()
    assert ops.pad_cols(mid.t, M, H, d, out=back.t).data_ptr() == back.t.data_ptr()
    torch.cuda.synchronize()
    assert mid.margins_intact() and back.margins_intact()
    assert rc.bits_equal(mid.t.cpu(), data.reshape(M, H * d))
    b = back.t.view(M, H, DP)
    assert rc.bits_equal(b[..., :d].cpu().contiguous(), data) and (b[..., d:] == 0).all()


def test_wrappers_reject_what_the_kernels_do_not_cover():
    ops = ops_()
    F32, BF16, BF16_F32IN = modes()
    x = torch.zeros((4, 3 * 96), device=dev())
    with pytest.raises(RuntimeError, match="heads_pad_fwd"):   # d = 12: no multiple of 8
        ops.heads_pad_fwd(F32, x, 36, x, 36, x, 36, None, 0.0, 1, 4, 1, 12)
    with pytest.raises(RuntimeError, match="heads_pad_fwd"):   # d = 128: nothing to pad
        ops.heads_pad_fwd(F32, x, 288, x, 288, x, 288, None, 0.0, 1, 4, 1, 128)
    with pytest.raises(RuntimeError, match="heads_pad_fwd"):   # bf16 projections are not an input type
        ops.heads_pad_fwd(BF16, x, 288, x, 288, x, 288, None, 0.0, 1, 4, 1, 96)
    with pytest.raises(TypeError):
        ops.heads_pad_fwd(BF16_F32IN, x.bfloat16(), 288, x, 288, x, 288, None, 0.0, 1, 4, 1, 96)
    with pytest.raises(ValueError):
        ops.pad_cols(x, 4, 3, 80)
    with pytest.raises(ValueError):
        ops.unpad_cols(x, 4, 3, 96, out=torch.zeros((4, 288), device=dev()))


# ------------------------------------------------------------------------------------------------ attention on padded tensors
def _compact_inputs(B, H, T, d):
    """|q| = |k| = 1.3 per head (logits up to sqrt(d) * 1.69), as test_gpu_attn_headdim._inputs, token-major fp32"""
    tok = lambda x: x.permute(0, 2, 1, 3).reshape(B * T, H * d).contiguous()
    q = 1.3 * torch.nn.functional.normalize(AH.rnd(B, H, T, d, seed=1), dim=-1)
    k = 1.3 * torch.nn.functional.normalize(AH.rnd(B, H, T, d, seed=2), dim=-1)
    return tok(q), tok(k), tok(AH.rnd(B, H, T, d, seed=3)), AH.rnd(B, H, T, d, seed=4)


ATTN_CASES = [(dtype, impl, d, H, T) for dtype, impl in ((BF16T, 1), (F32T, 0)) for d, H in ((80, 3), (104, 2))
              for T in (1, 49, 130, 257)]


@pytest.mark.parametrize("dtype,impl,d,H,T", ATTN_CASES)
def test_attention_on_padded_heads(dtype, impl, d, H, T):
    """nvit_attn_fwd and nvit_attn_bwd at D = 128 on the split kernel's padded tensors against fp64 SDPA math on the
    compact tensors (scale sqrt(d) of the real d; bars of test_gpu_attn_headdim._check_head_dim); the merged gradients are
    the same bits with NaN written into the gradient pads first; at T > 1 the same bar rejects scale = sqrt(128)."""
    ops = ops_()
    F32, BF16, BF16_F32IN = modes()
    B = 2
    M, C = B * T, H * d
    dt = F32 if dtype == F32T else BF16
    qt, kt, vt, g = _compact_inputs(B, H, T, d)
    c = {"q": qt, "k": kt, "v": vt, "sqk": None, "c_q": 0.0, "B": B, "T": T, "H": H, "d": d}
    bufs = split(c, F32 if dtype == F32T else BF16_F32IN, "stacked", False)
    assert_pads_zero(bufs, d, "attention inputs")
    qh, kh, vh = (bufs[n].t for n in ("qh", "kh", "vh"))
    g = g.to(dtype)
    scale = math.sqrt(d)

    def reference(s):
        leaves = [t[..., :d].cpu().double().requires_grad_(True) for t in (qh, kh, vh)]
        o_ref, lse_ref = AH._sdpa_ref(*leaves, s)
        o_ref.backward(g.double())
        return o_ref.detach(), lse_ref.detach(), [t.grad for t in leaves]

    o_ref, lse_ref, g_ref = reference(scale)
    o_pad, lse = AH.run_fwd(dt, impl, qh, kh, vh, scale)
    assert (o_pad.view(M, H, DP)[..., d:] == 0).all(), "pad columns of O are not zero"
    o = ops.unpad_cols(o_pad, M, H, d)
    o_bhtd = o.float().cpu().reshape(B, T, H, d).permute(0, 2, 1, 3).double()
    tol = 2e-6 if dtype == F32T else 1e-2
    err = (o_bhtd - o_ref).abs().max().item()
    assert err < tol, err
    assert (lse.cpu().double() - lse_ref).abs().max().item() < 1e-4
    if T > 1:   # (one key: the softmax is 1 at any scale)
        o_wrong, _, _ = reference(math.sqrt(DP))
        assert (o_bhtd - o_wrong).abs().max().item() >= tol, "the bar does not tell sqrt(d) from sqrt(128)"
    g_tok = g.permute(0, 2, 1, 3).reshape(M, C).contiguous().to(dev())
    g_pad = ops.pad_cols(g_tok, M, H, d)
    dqh, dkh, dvh = AH.run_bwd(dt, impl, g_pad, qh, kh, vh, ops.pad_cols(o, M, H, d), lse, scale)
    merged = []
    for poison in (False, True):
        if poison:
            for t in (dqh, dkh, dvh):
                t[..., d:] = NAN
        dqkv = torch.full((M, 3 * C), NAN, dtype=dtype, device=dev())
        ops.heads_pad_bwd(dt, dqh, dkh, dvh, None, None, None, None, None, 0.0, dqkv, 3 * C, dqkv[:, C:], 3 * C,
                          dqkv[:, 2 * C:], 3 * C, B, T, H, d)
        merged.append(dqkv)
    assert torch.isfinite(merged[1].float()).all() and torch.equal(merged[0], merged[1]), "gradient pads leaked"
    tolg = 5e-5 if dtype == F32T else 3e-2
    for i, (name, ref) in enumerate(zip(("dq", "dk", "dv"), g_ref)):
        got = merged[0][:, i * C:(i + 1) * C].cpu().double().reshape(B, T, H, d).permute(0, 2, 1, 3)
        e = (got - ref).abs().max().item()
        lim = tolg * max(1.0, ref.abs().max().item())
        assert e < lim, f"{name}: err {e:.3e} >= {lim:.3e}"


@pytest.mark.parametrize("dtype,impl,d,H,T", ATTN_CASES)
def test_bounded_attention_on_padded_heads(dtype, impl, d, H, T):
    """nvit_attn_fwd_bounded at D = 128 with the padded sqk the split kernel wrote (indexed sqk[h*128 + lane]), on its
    normalised q and k, against SDPA math on the compact tensors.  Bars: bf16 those of
    test_attention_bounded_scores_head_dim (the bound, 1.44 * sqrt(d) * 1.3^2 < 60, keeps the fast path), fp32 those of
    _check_head_dim."""
    ops = ops_()
    F32, BF16, BF16_F32IN = modes()
    B = 2
    M = B * T
    dt = F32 if dtype == F32T else BF16
    c = rc.qk_case(B, T, H, d, 500 + d + T)
    c["sqk"] = (1.0 / 32.0) * (1.0 + 0.3 * torch.tanh(AH.rnd(H * d, seed=7)))
    bufs = split(c, F32 if dtype == F32T else BF16_F32IN, "stacked", True)
    assert_pads_zero(bufs, d, "bounded attention inputs")
    qh, kh, vh, sqk_pad = (bufs[n].t for n in ("qh", "kh", "vh", "sqk_pad"))
    scale = math.sqrt(d)
    assert scale * 1.4426950408889634 * (c["sqk"] * c["c_q"]).abs().max().item() ** 2 <= 60.0
    leaves = [t[..., :d].cpu().double() for t in (qh, kh, vh)]
    o_ref, lse_ref = AH._sdpa_ref(*leaves, scale)
    o_pad, lse = AH.run_fwd(dt, impl, qh, kh, vh, scale, sqk_pad, c["c_q"], 1.0)
    o = ops.unpad_cols(o_pad, M, H, d).float().cpu().reshape(B, T, H, d).permute(0, 2, 1, 3).double()
    if dtype == F32T:
        o_tol, lse_tol = 2e-6, 1e-4
    else:
        o_tol, lse_tol = 1e-2 + 2.0 ** -7 * o_ref.abs().max().item(), 4e-3
    assert (o - o_ref).abs().max().item() < o_tol
    assert (lse.cpu().double() - lse_ref).abs().max().item() < lse_tol


def test_reference_mutants_normalise_over_dp_is_the_same_scale_by_dp_is_not():
    """What zero padding leaves alone and what it does not, on the reference side: normalising over groups of 128 columns
    of zero-padded data gives the head tensors of the d-wide normalise exactly; the softmax scale of the padded width,
    sqrt(128) in place of sqrt(80), moves the attention output by far more than any bar of the tests above."""
    B, T, H, d = 2, 49, 4, 80
    c = rc.qk_case(B, T, H, d, 9)
    padc = lambda x: torch.nn.functional.pad(x.reshape(-1, H, d), (0, DP - d)).reshape(x.shape[0], H * DP)
    cp = dict(c, q=padc(c["q"]), k=padc(c["k"]), v=padc(c["v"]), sqk=padc(c["sqk"][None])[0], d=DP,
              gq=torch.nn.functional.pad(c["gq"], (0, DP - d)), gk=torch.nn.functional.pad(c["gk"], (0, DP - d)),
              gv=torch.nn.functional.pad(c["gv"], (0, DP - d)))
    a, b = rc.qknorm_eval(c), rc.qknorm_eval(cp)
    for n in ("qh", "kh", "vh"):
        assert (b[n][..., :d] - a[n]).abs().max().item() < 1e-12 and (b[n][..., d:] == 0).all(), n
    for n in ("dq", "dk", "dv"):
        assert (b[n].reshape(-1, H, DP)[..., :d].reshape(-1, H * d) - a[n]).abs().max().item() < 1e-12, n
    o_d, _ = AH._sdpa_ref(a["qh"], a["kh"], a["vh"], math.sqrt(d))
    o_dp, _ = AH._sdpa_ref(b["qh"], b["kh"], b["vh"], math.sqrt(d))
    o_bad, _ = AH._sdpa_ref(b["qh"], b["kh"], b["vh"], math.sqrt(DP))
    assert (o_dp[..., :d] - o_d).abs().max().item() < 1e-12 and (o_dp[..., d:] == 0).all()
    assert (o_bad[..., :d] - o_d).abs().max().item() > 1e-2
