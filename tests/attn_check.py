"""Oracles of the MFMA attention tests (a plain helper module; test_attn_check.py checks it on the CPU,
test_gpu_attn_bounds.py uses it against the kernels of attn_mfma.hip; test_gpu_attn_headdim.py takes the padding harness).

Reference (`attn_ref`): softmax(scale q k^T) v, lse and, from autograd of that forward, dq, dk, dv, in fp64 on the CPU from
the exact bf16 operands the kernel is handed; a pre-scaled q is divided by q_prescale in fp64 (dq is the gradient of that
quotient, as the kernels return it).  Tq != Tk is supported.  `attn_grads_formula` restates the gradients with the
explicit dS = P (dP - delta).

Data families (dicts of operands [B, H, T, d] in bf16): `counting_case` (all scores equal, integer v and dO: every key
and every query row shows in every sum, and the result is exact up to one division and one rounding), `two_level_case`
(one-hot q and k: a score is 0 or scale a^2, v different for every key), `gauss_case` / `bounded_gauss_case` (the data of
test_gpu_ops.py / test_gpu_attn_headdim.py).

Bounds (`fwd_bounds`, `bwd_bounds`): per element, first order, operation by operation, from the fp64 quantities.
U32 = 2^-24 is the unit roundoff of fp32.  pack8 / pack4 and the stores round to nearest even to bf16, which has 8
significant bits: the error of one rounding is at most half an ulp, 2^(e - 8) for 2^e <= |x| < 2^(e + 1), i.e. between
2^-9 |x| and U16 |x| with U16 = 2^-8.  (2^-9 is the value at the top of a binade only: 1 + 2^-8 rounds to 1.  The lse bar
of 4e-3 of the older tests is ln(1 + 2^-8), and the emulator below, which is correct arithmetic, exceeds bounds written
with 2^-9 by up to 1.5.)  Where the rounded value is known in fp64 (P and dS of the backward, p relative to the score
bound on the FAST paths) the bound takes half an ulp at that value, `half_ulp_bf16`; where it is not (p relative to the
running maximum of the online path) it takes U16 |x|.

* raw score r = sum over d of q k (fp32, in the MFMA): red(d + 1, sum |q| |k|) (+ 1: the seed of the UNIT variants).
* exponent a = r c2 - off in log2 units, c2 = scale log2(e) / q_prescale, off = the running maximum (online), the score
  bound (FAST) or lse log2(e) (backward): c2 e_r + (LIB + 4) U32 (|r c2| + |off|) (c2: two conversions, a mul, a
  division; the mul; the subtraction; off likewise).  p = v_exp_f32(a): relative error ln 2 e_a + LIB U32.
* P is rounded to bf16 for P V and for dV: a single rounding of every term, so the worst case, the sum of the terms' half
  ulps, holds and is what the bound takes (the LAMBDA sqrt(n) u rule for n independent roundings is never below it).  Terms whose
  rounded values are bit-identical share ONE error: keys (or query rows) are grouped where the raw score has at most one
  nonzero product (exact in fp32 in any order) and equals another's - and, across query rows, where the handed lse is
  bit-identical and the true lse equal - and a group contributes its relative half ulp times |signed sum of the group|.  On the online path
  the row sum comes from the fp32 p, so the groups are per KV tile (the running maximum may move between tiles), except
  that a row whose scores are all equal has p = exp2(0) = 1 exactly at every tile: no error.  On the FAST paths the row
  sum is taken from the same bf16 values, so a group's error enters as its half ulp times |sum_G p (v - o)|: with one group (counting
  data) it cancels, the output is the exact mean up to the division and the final rounding.
* accumulation in fp32: red(n, sum |terms|) for P V, the row sum, dQ, dK, dV; the online rescale costs (LIB + 2) U32 per
  tile; the final 1 / l and multiply (LIB + 1) U32 |o|.
* lse, online: the errors of l relative to l, LIB U32 |ln l| for logf, (LIB + 5) U32 |m| for m c2 / log2(e), one add.
  lse, FAST: as above with -ln(1 - r), r = the p-weighted mean of the relative half ulps (at most U16), for the bf16 values the
  row sum is taken from (this is what the 4e-3 of the older tests stands for), and (LIB + 3) U32 (|bound| + |log2 l|) / log2(e).
* backward: the kernels are handed o (bf16) and lse (fp32); their ACTUAL deviations from the reference enter to first
  order (lse: relative error of every p of the row; o: through delta).  delta = fp32 sum over d of dO o:
  red(d, sum |dO o|) + sum |dO| |o_handed - o|.  w = dP - delta with -delta as the MFMA seed: red(d + 1, sum |dO| |v| +
  |delta|) + e_delta.  dS = p w (one rounding) is rounded to bf16 (half an ulp at |dS|, worst case) for dQ and dK; the scale is
  applied to the accumulators ((LIB + 3) U32).
* a bf16 output adds half a bf16 ulp (`check`).

No constant is fitted to a kernel's output; LAMBDA stays 8.

Emulator (`emulate`): the arithmetic above in torch on the CPU, written from the header comments of attn_mfma.hip, with
fp32 / bf16 tensors at the rounding points; switches for the path (online / fast / unit), the summation order (whole
rows, or tiles of TKV keys / queries in ascending order) and the mutants of MUTANTS.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from gemm_check import LAMBDA, U32, bits_equal, gauss_data, half_ulp_bf16, int_data   # noqa: F401
from kohonen_check import F64, LIB, check, check_all, red                               # noqa: F401
from rowops_check import Ev, from_heads, qknorm_bounds, qknorm_bwd_formula, to_heads     # noqa: F401

U16 = 2.0 ** -8          # unit roundoff of bf16: 8 significant bits, half an ulp at the bottom of a binade
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
BOUND_MAX = 60.0         # FAST path: score bound in log2 units
BF16T, F32T = torch.bfloat16, torch.float32
MAX_GROUPS = 64

# ------------------------------------------------------------------------------------------------ shapes
HEAD_DIMS = [32, 64, 128]
EQUAL_T = [1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 193, 257]
GAUSS_T = [17, 65, 129, 257]
UNEQUAL = [(1, 65), (17, 193), (129, 33), (33, 129), (200, 1)]     # (Tq, Tk)
FUSED_T = [16, 49, 129, 200, 257]
# Gaussian data also runs where two-level data leaves every query row with the same number of matching keys (all row
# statistics equal: MUTANT d_fragment_stats would pass unseen)
GAUSS_EXTRA = [(64, 64), (17, 193), (33, 129)]


def gauss_runs(Tq: int, Tk: int) -> bool:
    return (Tq == Tk and Tq in GAUSS_T) or (Tq, Tk) in GAUSS_EXTRA


def tkv_of(d: int) -> int:
    """keys per staged KV tile (and queries per tile of the dK/dV kernel)"""
    return 32 if d == 128 else 64


def equal_lengths(d: int):
    return EQUAL_T + ([97] if d == 128 else [])


# ------------------------------------------------------------------------------------------------ padding harness
PAD = 4096          # elements of padding on each side (a multiple of 8: keeps 16-byte alignment)
SENTINEL = -12288.0   # exact in bf16 and fp32


def dev():
    return torch.device("cuda:0")


class Padded:
    """A tensor placed in the middle of a larger device buffer whose margins hold `fill`."""

    def __init__(self, shape, dtype, fill, data=None):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev())
        self.t = self.buf[PAD:PAD + n].view(shape)
        if data is not None:
            self.t.copy_(data)
        self.fill = fill

    def ptr(self):
        return self.t.data_ptr()

    def margins_intact(self):
        m = torch.cat([self.buf[:PAD], self.buf[-PAD:]]).float()
        return bool(torch.isnan(m).all()) if math.isnan(self.fill) else bool((m == self.fill).all())


def operand(x):
    return Padded(tuple(x.shape), x.dtype, float("nan"), x.to(dev()))


def output(shape, dtype):
    return Padded(shape, dtype, SENTINEL)


def run_fwd(dt, impl, q, k, v, scale, sqk=None, c_q=0.0, q_prescale=1.0):
    """nvit_attn_fwd / nvit_attn_fwd_bounded on padded operands and outputs; returns (o, lse) as plain tensors."""
    from nvit_amd import _lib, ops
    (B, H, Tq, d), Tk = q.shape, k.shape[2]
    qp, kp, vp = operand(q), operand(k), operand(v)
    o, lse = output((B * Tq, H * d), q.dtype), output((B, H, Tq), torch.float32)
    lib = _lib.load()
    if sqk is None:
        rc = lib.nvit_attn_fwd(dt, impl, qp.ptr(), kp.ptr(), vp.ptr(), scale, o.ptr(), lse.ptr(), B, H, Tq, Tk, d, ops._s())
    else:
        sp = operand(sqk)
        rc = lib.nvit_attn_fwd_bounded(dt, impl, qp.ptr(), kp.ptr(), vp.ptr(), scale, sp.ptr(), c_q, q_prescale, o.ptr(),
                                       lse.ptr(), B, H, Tq, Tk, d, ops._s())
    ops.check(rc, "nvit_attn_fwd")
    torch.cuda.synchronize()
    assert o.margins_intact() and lse.margins_intact()
    return o.t.clone(), lse.t.clone()


def run_bwd(dt, impl, g_tok, q, k, v, o, lse, scale):
    from nvit_amd import _lib, ops
    (B, H, Tq, d), Tk = q.shape, k.shape[2]
    gp, qp, kp, vp, op, lp = (operand(x) for x in (g_tok, q, k, v, o, lse))
    dq, dk, dv = (output((B, H, T, d), q.dtype) for T in (Tq, Tk, Tk))
    delta = Padded((2, B, H, Tq), torch.float32, float("nan"))   # workspace: written before it is read
    rc = _lib.load().nvit_attn_bwd(dt, impl, gp.ptr(), qp.ptr(), kp.ptr(), vp.ptr(), op.ptr(), lp.ptr(), scale, dq.ptr(),
                                   dk.ptr(), dv.ptr(), delta.ptr(), B, H, Tq, Tk, d, ops._s())
    ops.check(rc, "nvit_attn_bwd")
    torch.cuda.synchronize()
    for x in (dq, dk, dv):
        assert x.margins_intact()
    return dq.t.clone(), dk.t.clone(), dv.t.clone()


def tok(x: torch.Tensor) -> torch.Tensor:
    """[B, H, T, d] -> token-major [B * T, H * d]"""
    B, H, T, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * d).contiguous()


def untok(x: torch.Tensor, B: int, H: int) -> torch.Tensor:
    """token-major [B * T, H * d] -> [B, H, T, d]"""
    M, C = x.shape
    return x.reshape(B, M // B, H, C // H).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------------ data
def _case(q, k, v, g, scale, family, qpre=1.0, sqk=None, c_q=0.0) -> Dict:
    return {"q": q.to(BF16T), "k": k.to(BF16T), "v": v.to(BF16T), "g": g.to(BF16T), "scale": float(scale),
            "qpre": float(qpre), "sqk": sqk, "c_q": float(c_q), "family": family}


def nonzero_ints(shape, amax: int, seed: int) -> torch.Tensor:
    """integers in +-{1 .. amax}, never 0"""
    mag = torch.randint(1, amax + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()
    sgn = torch.randint(0, 2, tuple(shape), generator=torch.Generator().manual_seed(seed + 1)).float() * 2 - 1
    return mag * sgn


def require_counting_exact(Tq: int, Tk: int, d: int, amax: int) -> None:
    """Refuse a counting case whose sums could leave the exact range.  sum_j v_j and sum_i dO_i are integers up to
    max(Tq, Tk) amax, multiplied by ONE bf16 value p (8 significant bits): exact in fp32 while the integer stays below
    2^16.  dP and delta's integer part are sums over d of products up to amax^2: below 2^24."""
    if max(Tq, Tk) * amax >= 2 ** 16 or d * amax * amax >= 2 ** 24:
        raise ValueError(f"counting case out of range: sums up to {max(Tq, Tk) * amax} (limit 2^16) and "
                         f"{d * amax * amax} (limit 2^24)")


def counting_case(B, H, Tq, Tk, d, seed, zero="q", scale=None, qpre=1.0, bound=None, amax=4) -> Dict:
    """zero = "q": q = 0, k small integers (dq is exercised, dk = 0); zero = "k": the other way round.
    bound: the value of sqk * c_q handed to the bounded entry (None: the generic entry)."""
    require_counting_exact(Tq, Tk, d, amax)
    scale = math.sqrt(d) if scale is None else scale
    other = nonzero_ints((B, H, Tk if zero == "q" else Tq, d), 2, seed)
    q = torch.zeros(B, H, Tq, d) if zero == "q" else other
    k = other if zero == "q" else torch.zeros(B, H, Tk, d)
    sqk, c_q = (None, 0.0) if bound is None else (torch.full((H * d,), bound / 32.0), 32.0)
    return _case(q, k, nonzero_ints((B, H, Tk, d), amax, seed + 2), nonzero_ints((B, H, Tq, d), amax, seed + 4), scale,
                 "counting_" + zero, qpre, sqk, c_q)


def two_level_a(Tk: int, d: int, scale: float, h: int) -> float:
    """a (a bf16 number: a^2 is exact in fp32) such that the matching keys - about one in min(d, Tk) - carry about half
    of a row's weight at head 0: exp(scale a^2) = min(d, Tk) - 1; every head has its own a (x 1, 1.125, 1.25, ...)."""
    ratio = max(min(d, Tk) - 1, 2)
    a = math.sqrt(math.log(ratio) / scale) * (1.0 + 0.125 * (h % 4))
    return float(torch.tensor(a).to(BF16T))


def two_level_case(B, H, Tq, Tk, d, seed, scale=None, qpre=1.0, bounded=False, over=False) -> Dict:
    """k_j = a e_{j mod d}, q_i = a e_{(7 i + 3) mod d} (handed as bf16(qpre a) e): a score is 0 or scale a^2.  v is a
    different dyadic row for every key; dO integers.  bounded: sqk * c_q = a per channel (the bound is attained);
    over: sqk * c_q = 8 a (a bound beyond BOUND_MAX: the entry falls back to the online path)."""
    scale = math.sqrt(d) if scale is None else scale
    q, k = torch.zeros(B, H, Tq, d), torch.zeros(B, H, Tk, d)
    sq = torch.zeros(H, d)
    i, j = torch.arange(Tq), torch.arange(Tk)
    for h in range(H):
        a = two_level_a(Tk, d, scale, h)
        q[:, h, i, (7 * i + 3) % d] = float((torch.tensor(a * qpre)).to(BF16T))
        k[:, h, j, j % d] = a
        sq[h] = a * (8.0 if over else 1.0)
    c = torch.arange(d)
    v = (((j[:, None] * 31 + c[None, :] * 17) % 61) - 30).float() / 8.0          # |v| <= 3.75, 6 bits
    v = v[None, None] + torch.arange(B * H).reshape(B, H, 1, 1).float() / 4.0
    sqk, c_q = (sq.reshape(-1) / 32.0, 32.0) if (bounded or over) else (None, 0.0)
    return _case(q, k, v.expand(B, H, Tk, d), nonzero_ints((B, H, Tq, d), 4, seed), scale, "two_level", qpre, sqk, c_q)


def gauss_case(B, H, Tq, Tk, d, seed, scale=None) -> Dict:
    """|q| = |k| = 1.3 per head (test_attention)"""
    unit = lambda T, s: 1.3 * torch.nn.functional.normalize(gauss_data((B, H, T, d), s), dim=-1)
    return _case(unit(Tq, seed), unit(Tk, seed + 1), gauss_data((B, H, Tk, d), seed + 2),
                 gauss_data((B, H, Tq, d), seed + 3), math.sqrt(d) if scale is None else scale, "gauss")


def bounded_gauss_case(B, H, Tq, Tk, d, seed, qpre=1.0, smul=1.0) -> Dict:
    """(sqk * c_q) * unit vectors (test_attention_bounded_scores); qpre: q is handed as qpre * q_hat"""
    sqk = (smul / 32.0) * (1.0 + 0.3 * torch.tanh(gauss_data((H * d,), seed + 7)))
    s_eff = (sqk * 32.0).reshape(1, H, 1, d)
    unit = lambda T, s: s_eff * torch.nn.functional.normalize(gauss_data((B, H, T, d), s), dim=-1)
    return _case(qpre * unit(Tq, seed), unit(Tk, seed + 1), gauss_data((B, H, Tk, d), seed + 2),
                 gauss_data((B, H, Tq, d), seed + 3), math.sqrt(d), "gauss_bounded", qpre, sqk, 32.0)


def score_bound(c: Dict) -> Optional[torch.Tensor]:
    """the FAST path's score bound in log2 units per head [1, H, 1, 1] (None without sqk)"""
    if c["sqk"] is None:
        return None
    H, d = c["q"].shape[1], c["q"].shape[3]
    sm = (c["sqk"].double() * c["c_q"]).abs().reshape(H, d).max(dim=-1).values
    return (c["scale"] * LOG2E * sm * sm).reshape(1, H, 1, 1)


def path_of(c: Dict) -> str:
    """the forward path the bounded / generic entry takes on this case"""
    tb = score_bound(c)
    if tb is None or tb.max().item() > BOUND_MAX:
        return "online"
    return "unit" if abs(c["scale"] * LOG2E / c["qpre"] - 1.0) < 1e-6 else "fast"


# ------------------------------------------------------------------------------------------------ reference
def attn_ref(c: Dict, backward: bool = True) -> Dict[str, torch.Tensor]:
    q = (c["q"].double() / c["qpre"]).requires_grad_(backward)
    k, v = c["k"].double().requires_grad_(backward), c["v"].double().requires_grad_(backward)
    s = (q @ k.transpose(-1, -2)) * c["scale"]
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ v
    res = {"o": o.detach(), "lse": lse.detach()}
    if backward:
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), c["g"].double())
        res.update(dq=dq, dk=dk, dv=dv)
    return res


def attn_grads_formula(c: Dict) -> Dict[str, torch.Tensor]:
    """the gradients restated: P from lse, dP = dO v^T, delta = <dO, o>, dS = P (dP - delta)"""
    q, k, v, g = c["q"].double() / c["qpre"], c["k"].double(), c["v"].double(), c["g"].double()
    s = (q @ k.transpose(-1, -2)) * c["scale"]
    m = s.max(dim=-1, keepdim=True).values
    lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
    P = torch.exp(s - lse)
    o = P @ v
    dS = P * (g @ v.transpose(-1, -2) - (g * o).sum(-1, keepdim=True))
    return {"o": o, "lse": lse[..., 0], "dq": c["scale"] * dS @ k, "dk": c["scale"] * dS.transpose(-1, -2) @ q,
            "dv": P.transpose(-1, -2) @ g}


# ------------------------------------------------------------------------------------------------ bounds
def _scores(c: Dict):
    qh, k = c["q"].double(), c["k"].double()
    d = qh.shape[-1]
    c2 = c["scale"] * LOG2E / c["qpre"]
    raw = qh @ k.transpose(-1, -2)
    e_raw = red(d + 1, qh.abs() @ k.abs().transpose(-1, -2))
    exact = ((qh != 0).double() @ (k != 0).double().transpose(-1, -2)) <= 1
    lv = torch.unique(raw[exact])
    if lv.numel() == 0 or lv.numel() > 8:
        level = torch.full(raw.shape, -1, dtype=torch.long)
    else:
        level = torch.where(exact, torch.searchsorted(lv, raw.contiguous()).clamp(max=lv.numel() - 1), -1)
        level = torch.where(exact & (lv[level.clamp(min=0)] == raw), level, -1)
    return raw, raw * c2, c2, e_raw, level


def rel16(x: torch.Tensor) -> torch.Tensor:
    """half a bf16 ulp at |x|, relative to |x|: between U16 / 2 and U16 (0 where x == 0)"""
    ax = x.abs().double()
    return torch.where(ax > 0, half_ulp_bf16(ax) / ax.clamp(min=1e-300), torch.zeros_like(ax))


def grouped_abs(P: torch.Tensor, X: torch.Tensor, key: torch.Tensor, o: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum over the groups G of |sum_{j in G} P[.., i, j] (X[.., j, :] - o[.., i, :])| (o None: 0); key [.., i, j] >= 0
    names the group, key < 0 is a group of its own.  More than MAX_GROUPS groups: every term on its own (never smaller)."""
    ids = torch.unique(key[key >= 0])
    if ids.numel() > MAX_GROUPS:
        ids, key = ids[:0], torch.full_like(key, -1)
    single = P.abs() * (key < 0)
    acc = single @ X.abs() + (single.sum(-1, keepdim=True) * o.abs() if o is not None else 0.0)
    for u in ids.tolist():
        Pm = P * (key == u)
        t = Pm @ X
        if o is not None:
            t = t - Pm.sum(-1, keepdim=True) * o
        acc = acc + t.abs()
    return acc


def fwd_bounds(c: Dict, ref: Dict, path: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Bounds of o [B, H, Tq, d] (without the output's own rounding) and lse [B, H, Tq] on `path` (None: the path the
    entry takes on this case)."""
    path = path_of(c) if path is None else path
    v = c["v"].double()
    Tk, d = v.shape[2], v.shape[3]
    tkv = tkv_of(d)
    nt = -(-Tk // tkv)
    raw, x, c2, e_raw, level = _scores(c)
    o, lse = ref["o"], ref["lse"][..., None]
    P = torch.exp(raw * (c["scale"] / c["qpre"]) - lse)
    smax = x.max(dim=-1, keepdim=True).values
    if path == "online":
        off = x.abs().max(dim=-1, keepdim=True).values
    else:
        off = score_bound(c).expand(-1, -1, x.shape[2], 1)
        r16 = rel16(torch.exp2(x - off))          # the rounded value is p relative to the bound
    e_p = LN2 * (c2 * e_raw + (LIB + 4) * U32 * (x.abs() + off.abs())) + LIB * U32
    PV = P @ v.abs()
    indep = (e_p * P) @ v.abs() + o.abs() * (e_p * P).sum(-1, keepdim=True)
    tile = (torch.arange(Tk) // tkv).expand(level.shape)
    if path == "online":
        flat = (level >= 0).all(-1, keepdim=True) & (raw.max(-1, keepdim=True).values == raw.min(-1, keepdim=True).values)
        dlt = torch.where(flat, 0.0, U16).expand(P.shape)
        rounding = grouped_abs(P * dlt, v, torch.where(level >= 0, level * nt + tile, -1))
    else:
        rounding = grouped_abs(P * r16, v, level, o) / (1.0 - U16)     # (the row sum itself is off by up to U16)
    acc = red(Tk, PV) + red(Tk, torch.ones(())) * o.abs()
    resc = nt * (LIB + 2) * U32 * (PV + o.abs()) if path == "online" else 0.0
    b_o = indep + rounding + acc + resc + (LIB + 1) * U32 * o.abs()
    rel_l = (e_p * P).sum(-1, keepdim=True) + red(Tk, torch.ones(()))
    if path == "online":
        m_nat = smax / LOG2E
        b_l = rel_l + nt * (LIB + 2) * U32 + U32 * ((LIB + 5) * m_nat.abs() + LIB * (lse - m_nat).abs() + lse.abs())
    else:
        b_l = rel_l - torch.log1p(-(P * r16).sum(-1, keepdim=True)) + (LIB + 3) * U32 * (off.abs() + (lse * LOG2E - off).abs()) / LOG2E
    return {"o": b_o, "lse": b_l[..., 0]}


def bwd_bounds(c: Dict, ref: Dict, o_h: torch.Tensor, lse_h: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Bounds of dq (the gradient of q / qpre), dk, dv [B, H, T, d] WITHOUT the output's own rounding (`check` adds half a
    bf16 ulp).  o_h [B, H, Tq, d], lse_h [B, H, Tq]: what the backward kernels are handed."""
    qhat, k, v, g = c["q"].double() / c["qpre"], c["k"].double(), c["v"].double(), c["g"].double()
    Tq, Tk, d = qhat.shape[2], k.shape[2], k.shape[3]
    scale = abs(c["scale"])
    raw, x, c2, e_raw, level = _scores(c)
    o, lse = ref["o"], ref["lse"][..., None]
    lse_h = lse_h.detach().cpu().to(F32T)
    e_lse = torch.expm1((lse_h.double()[..., None] - lse).abs())      # |exp(+-e) - 1| <= expm1(e)
    e_o = (o_h.detach().cpu().double() - o).abs()
    P = torch.exp(raw * (c["scale"] / c["qpre"]) - lse)
    e_pi = LN2 * (c2 * e_raw + (LIB + 4) * U32 * (x.abs() + (lse_h.double()[..., None] * LOG2E).abs())) + (LIB + 1) * U32
    delta = (g * o).sum(-1, keepdim=True)
    e_delta = (g.abs() * e_o).sum(-1, keepdim=True) + red(d, (g * o).abs().sum(-1, keepdim=True))
    e_w = red(d + 1, g.abs() @ v.abs().transpose(-1, -2) + delta.abs()) + e_delta
    dS = P * (g @ v.transpose(-1, -2) - delta)
    e_dS = dS.abs() * (e_pi + e_lse + U32) + half_ulp_bf16(dS) + P * e_w
    b_dq = scale * (e_dS @ k.abs() + red(Tk, dS.abs() @ k.abs())) + (LIB + 3) * U32 * ref["dq"].abs()
    dST, e_dST = dS.transpose(-1, -2), e_dS.transpose(-1, -2)
    b_dk = scale * (e_dST @ qhat.abs() + red(Tq, dST.abs() @ qhat.abs())) + (2 * LIB + 3) * U32 * ref["dk"].abs()
    # dV: rows with bit-identical handed lse and equal true lse share the error of lse and, at equal exact scores, the
    # rounding of p
    rows = torch.stack([lse_h.double().reshape(-1), lse.reshape(-1)], dim=1)
    _, inv = torch.unique(rows, dim=0, return_inverse=True)
    nu = int(inv.max().item()) + 1
    key = torch.where(level >= 0, level * nu + inv.reshape(lse.shape), -1)
    PT = P.transpose(-1, -2)
    b_dv = ((e_pi * P).transpose(-1, -2) @ g.abs() + grouped_abs((P * (rel16(P) + e_lse)).transpose(-1, -2), g, key.transpose(-1, -2))
            + red(Tq, PT @ g.abs()))
    return {"dq": b_dq, "dk": b_dk, "dv": b_dv}


def margin(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """largest err / bound (+ half a bf16 ulp for a bf16 output, as `check`), without asserting; inf where a non-zero
    error meets a zero bound or the output is not finite"""
    out = out.detach().cpu()
    ref = ref.detach().to(F64)
    bound = torch.as_tensor(bound, dtype=F64).expand(ref.shape)
    if out.dtype == BF16T:
        bound = bound + half_ulp_bf16(ref.abs() + bound)
    if not torch.isfinite(out.float()).all():
        return math.inf
    err = (out.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0))
    return r.max().item()


# ------------------------------------------------------------------------------------------------ emulator
# name: what the kernel would do wrong
MUTANTS = {
    "a_last_key_dropped": "the last key left out (forward and dQ)",
    "b_last_key_twice": "key Tk - 1 counted twice in the ragged tile (forward and dQ)",
    "c_v_keys_swapped": "keys 2 and 3 of every 32-key step swapped in V (dQ: in the transposed K) while P is unchanged",
    "d_fragment_stats": "query fragment 16..31 of a wave uses fragment 0..15's row sum / lse",
    "e_tile3_reads_tile0": "the fourth KV tile reads the first tile's K and V again",
    "f_last_query_twice": "query row Tq - 1 counted twice in dK / dV",
    "g_delta_sign": "delta added where it is subtracted",
    "g_delta_neighbour": "delta of row i ^ 1",
    "h_dk_scale": "dK scaled by scale where scale / q_prescale is due",
    "i_lse_other_head": "head h reads the lse of head h ^ 1 (backward)",
}


def mutant_applies(name: str, H: int, Tq: int, Tk: int, d: int, qpre: float = 1.0) -> bool:
    tkv = tkv_of(d)
    return {"a_last_key_dropped": Tk >= 2, "b_last_key_twice": Tk % tkv != 0, "c_v_keys_swapped": Tk >= 4,
            "d_fragment_stats": Tq > 16, "e_tile3_reads_tile0": Tk > 3 * tkv, "f_last_query_twice": Tq % tkv != 0,
            "g_delta_sign": True, "g_delta_neighbour": Tq >= 2,
            "h_dk_scale": qpre != 1.0 and Tk >= 2,   # (one key: dS = 0, dK is identically 0)
            "i_lse_other_head": H >= 2}[name]


def _f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=F32T)


def _key_tiles(T: int, tkv: int, tiled: bool, mutant: Optional[str]):
    """[(indices of the K rows, indices of the V rows)] per tile"""
    step = tkv if tiled else max(T, 1)
    tiles = [torch.arange(t, min(t + step, T)) for t in range(0, T, step)]
    if mutant == "a_last_key_dropped":
        tiles[-1] = tiles[-1][:-1]
    if mutant == "b_last_key_twice":
        tiles[-1] = torch.cat([tiles[-1], tiles[-1][-1:]])
    if mutant == "e_tile3_reads_tile0":
        tiles[3] = tiles[0][:tiles[3].numel()]
    out = []
    for idx in tiles:
        vidx = idx.clone()
        if mutant == "c_v_keys_swapped":
            for s0 in range(0, idx.numel() - 3, 32):
                vidx[s0 + 2], vidx[s0 + 3] = idx[s0 + 3], idx[s0 + 2]
        if idx.numel():
            out.append((idx, vidx))
    return out


def _frag_shift(x: torch.Tensor, dim: int) -> torch.Tensor:
    """rows 16..31 of every 32 take the value of the row 16 above"""
    i = torch.arange(x.shape[dim])
    return x.index_select(dim, torch.where(i % 32 >= 16, i - 16, i))


def _other_head(x: torch.Tensor) -> torch.Tensor:
    H = x.shape[1]
    h = torch.arange(H)
    return x[:, torch.where((h ^ 1) < H, h ^ 1, h)]


def emulate_fwd(c: Dict, path: Optional[str] = None, tiled: bool = True, mutant: Optional[str] = None):
    """(o bf16 [B, H, Tq, d], lse fp32 [B, H, Tq]) as the forward kernel computes them"""
    path = path_of(c) if path is None else path
    qf, kf, vf = c["q"].float(), c["k"].float(), c["v"].float()
    B, H, Tq, d = qf.shape
    c2t = _f32(c["scale"]) * _f32(LOG2E)
    c2 = c2t / _f32(c["qpre"])
    tiles = _key_tiles(kf.shape[2], tkv_of(d), tiled or mutant is not None, mutant)
    acc = torch.zeros(B, H, Tq, d)
    l = torch.zeros(B, H, Tq, 1)
    if path == "online":
        m = torch.full((B, H, Tq, 1), -math.inf)
        for idx, vidx in tiles:
            s = qf @ kf[:, :, idx].transpose(-1, -2)
            mn = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
            corr = torch.exp2((m - mn) * c2)
            p = torch.exp2(s * c2 - mn * c2)
            l = l * corr + p.sum(-1, keepdim=True)
            acc = acc * corr + p.to(BF16T).float() @ vf[:, :, vidx]
            m = mn
        lse = m * (c2 * _f32(1.0 / LOG2E)) + torch.log(l)
    else:
        sm = (c["sqk"].float() * _f32(c["c_q"])).abs().reshape(H, d).max(dim=-1).values.reshape(1, H, 1, 1)
        tb = c2t * sm * sm
        for idx, vidx in tiles:
            s = qf @ kf[:, :, idx].transpose(-1, -2)
            p = torch.exp2(s - tb if path == "unit" else s * c2 - tb).to(BF16T).float()
            l = l + p.sum(-1, keepdim=True)
            acc = acc + p @ vf[:, :, vidx]
        lse = (tb + torch.log2(l)) * _f32(1.0 / LOG2E)
    if mutant == "d_fragment_stats":
        l, lse = _frag_shift(l, 2), _frag_shift(lse, 2)
    return (acc * (1.0 / l)).to(BF16T), lse[..., 0].to(F32T)


def emulate_bwd(c: Dict, o: torch.Tensor, lse: torch.Tensor, tiled: bool = True, mutant: Optional[str] = None,
                raw: bool = False):
    """(dq, dk, dv) bf16 as the dQ and dK/dV kernels compute them from the handed o (bf16 [B, H, Tq, d]) and lse; the
    UNIT variants (c2 == 1) seed the score product with -lse in log2 units.  raw: the fp32 accumulators (what the fused
    q/k-normalise epilogue starts from)."""
    qf, kf, vf, gf = c["q"].float(), c["k"].float(), c["v"].float(), c["g"].float()
    B, H, Tq, d = qf.shape
    Tk = kf.shape[2]
    tkv = tkv_of(d)
    c2 = _f32(c["scale"]) * _f32(LOG2E) / _f32(c["qpre"])
    unit = abs(float(c2) - 1.0) < 1e-6
    delta = (gf * o.float()).sum(-1, keepdim=True)
    lse2 = (lse.float() * _f32(LOG2E))[..., None]
    if mutant == "i_lse_other_head":
        lse2 = _other_head(lse2)
    if mutant == "g_delta_neighbour":
        i = torch.arange(Tq)
        delta = delta[:, :, torch.where((i ^ 1) < Tq, i ^ 1, i)]
    sgn = -1.0 if mutant == "g_delta_sign" else 1.0

    def ds_p(qs, ks, vs, gs, l2, dl):
        s = qs @ ks.transpose(-1, -2)
        p = torch.exp2(s - l2 if unit else s * c2 - l2)
        w = gs @ vs.transpose(-1, -2) - sgn * dl
        return (p * w).to(BF16T).float(), p.to(BF16T).float()

    force = tiled or mutant is not None
    l2q = _frag_shift(lse2, 2) if mutant == "d_fragment_stats" else lse2
    dq = torch.zeros(B, H, Tq, d)
    for idx, vidx in _key_tiles(Tk, tkv, force, mutant):
        ds, _ = ds_p(qf, kf[:, :, idx], vf[:, :, idx], gf, l2q, delta)
        dq = dq + ds @ kf[:, :, vidx]
    dq = dq * _f32(c["scale"])
    qtiles = _key_tiles(Tq, tkv, force, None)
    if mutant == "f_last_query_twice":
        qtiles[-1] = (torch.cat([qtiles[-1][0], qtiles[-1][0][-1:]]),) * 2
    dk, dv = torch.zeros(B, H, Tk, d), torch.zeros(B, H, Tk, d)
    for qi, _ in qtiles:
        ds, p = ds_p(qf[:, :, qi], kf, vf, gf[:, :, qi], lse2[:, :, qi], delta[:, :, qi])
        dv = dv + p.transpose(-1, -2) @ gf[:, :, qi]
        dk = dk + ds.transpose(-1, -2) @ qf[:, :, qi]
    dk = dk * (_f32(c["scale"]) if mutant == "h_dk_scale" else _f32(c["scale"]) / _f32(c["qpre"]))
    return (dq, dk, dv) if raw else (dq.to(BF16T), dk.to(BF16T), dv.to(BF16T))


def emulate(c: Dict, path: Optional[str] = None, tiled: bool = True, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Forward and backward.  A mutant's backward is handed the correct forward's o and lse (a wrong forward is seen in
    o and lse themselves)."""
    o, lse = emulate_fwd(c, path, tiled, mutant)
    o_h, lse_h = (o, lse) if mutant is None else emulate_fwd(c, path, tiled, None)
    dq, dk, dv = emulate_bwd(c, o_h, lse_h, tiled, mutant)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "o_h": o_h, "lse_h": lse_h}


def all_bounds(c: Dict, ref: Dict, o_h: torch.Tensor, lse_h: torch.Tensor, path: Optional[str] = None) -> Dict:
    b = fwd_bounds(c, ref, path)
    b.update(bwd_bounds(c, ref, o_h, lse_h))
    return b


OUTS = ("o", "lse", "dq", "dk", "dv")


def margins(got: Dict, ref: Dict, bound: Dict) -> Dict[str, float]:
    return {n: margin(got[n], ref[n], bound[n]) for n in OUTS if n in got and n in bound}


# ------------------------------------------------------------------------------------------------ cases
CONFIGS = ("online", "unit_bwd", "fast", "fast_unit", "over")   # the entry and path a case is built for
FAMILIES = ("counting_q", "counting_k", "two_level", "gauss")


def q_prescale(d: int) -> float:
    """ops.attn_q_prescale (the GPU test asserts the two agree)"""
    return math.sqrt(d) * LOG2E


def make_case(family: str, config: str, B: int, H: int, Tq: int, Tk: int, d: int, seed: int = 11) -> Dict:
    """online: the generic entry at scale sqrt(d).  unit_bwd: the generic entry at scale ln 2 (online forward, UNIT
    backward).  fast / fast_unit / over: the bounded entry within the bound, with q pre-scaled, and with a bound beyond
    BOUND_MAX (online fallback)."""
    bounded = config in ("fast", "fast_unit", "over")
    qpre = q_prescale(d) if config == "fast_unit" else 1.0
    scale = LN2 if config == "unit_bwd" else math.sqrt(d)
    if family in ("counting_q", "counting_k"):
        bound = {"fast": 1.0, "fast_unit": 1.0, "over": 3.0}.get(config)
        return counting_case(B, H, Tq, Tk, d, seed, family[-1], scale, qpre, bound)
    if family == "two_level":
        return two_level_case(B, H, Tq, Tk, d, seed, scale, qpre, bounded, config == "over")
    if bounded:
        return bounded_gauss_case(B, H, Tq, Tk, d, seed, qpre, 3.0 if config == "over" else 1.0)
    return gauss_case(B, H, Tq, Tk, d, seed, scale)


# The families a mutant is shown on (test_attn_check.py: err / bound >= 2 on at least one of them, at every shape of the
# GPU list the mutant applies to and the family runs at).  Counting data shows what changes WHICH terms enter a sum;
# where all rows or heads are alike (counting: every lse is ln Tk) a mixed-up row statistic needs two-level or Gaussian
# data.
MUTANT_FAMILIES = {
    "a_last_key_dropped": ("counting_q", "counting_k", "two_level"),
    "b_last_key_twice": ("counting_q", "counting_k", "two_level"),
    "c_v_keys_swapped": ("two_level", "gauss"),
    "d_fragment_stats": ("two_level", "gauss"),
    "e_tile3_reads_tile0": ("counting_q", "counting_k", "two_level"),
    "f_last_query_twice": ("counting_q", "counting_k", "two_level"),
    "g_delta_sign": ("counting_q", "counting_k", "two_level", "gauss"),
    "g_delta_neighbour": ("counting_q", "counting_k", "two_level", "gauss"),
    "h_dk_scale": ("counting_k", "two_level", "gauss"),
    "i_lse_other_head": ("two_level", "gauss"),
}

# (mutant, Tq, Tk) that no family running at that shape can show, at any head dim: with one query and one key every head
# of every family has lse = the one score and P = 1, and dS = 0; Gaussian data does not run there.
NOT_SHOWN = {("i_lse_other_head", 1, 1): "P = 1 whatever lse is read when it equals the own one: all heads' only score is 0"}


# ------------------------------------------------------------------------------------------------ fused backward, d = 64
def fused_case(B: int, H: int, T: int, seed: int, qpre: float, with_sqk: bool) -> Dict:
    """The operands of nvit_attn_bwd_qknorm: (sqk c_q) * unit vectors (q handed as qpre * q_hat) and positive saved
    inverse norms rq, rk [M, H]; without sqk plain heads with |q_hat| = |k| = 1.3."""
    if with_sqk:
        c = bounded_gauss_case(B, H, T, T, 64, seed, qpre)
        c["rq"] = 1.0 + 0.1 * gauss_data((B * T, H), seed + 8).abs()
        c["rk"] = 1.0 + 0.1 * gauss_data((B * T, H), seed + 9).abs()
    else:
        c = gauss_case(B, H, T, T, 64, seed)
        c["q"] = (qpre * c["q"].float()).to(BF16T)
        c["qpre"] = float(qpre)
        c["rq"] = c["rk"] = None
    return c


def fused_ref_bounds(c: Dict, ref: Dict, hb: Dict):
    """(values, bounds) of the fused backward's outputs, token-major [M, C] (+ dsqk [C] with sqk): the fp64 head-major
    gradients `ref` pushed through rowops_check.qknorm_bwd_formula from the handed qh / qpre, kh, rq, rk, run on Ev with
    the head-major attention bounds `hb` as the input error of gq, gk (the kernels hand the fp32 accumulators over: no
    rounding in between).  qh / qpre: the kernel multiplies by 1 / (s qpre): (LIB + 2) U32.  dsqk: the formula's one sum
    over the rows covers the partial rows and their reduction in any order; part_q and part_k are scaled and added
    separately: 4 U32 of the magnitude more."""
    B, H, T, d = c["q"].shape
    fh = lambda t: from_heads(t, B, T, H, d)
    if c["sqk"] is None:
        return {n: fh(ref[n]) for n in ("dq", "dk", "dv")}, {n: fh(hb[n]) for n in ("dq", "dk", "dv")}
    qhat = c["q"].double() / c["qpre"]
    cc = {"sqk": c["sqk"], "c_q": c["c_q"], "B": B, "T": T, "H": H, "d": d, "gq": Ev(ref["dq"], hb["dq"]),
          "gk": Ev(ref["dk"], hb["dk"])}
    fwd = {"qh": Ev(qhat, (LIB + 2) * U32 * qhat.abs()), "kh": Ev(c["k"].double()), "rq": c["rq"], "rk": c["rk"]}
    res = qknorm_bwd_formula(cc, fwd, "ev")
    vals = {"dq": res["dq"].v, "dk": res["dk"].v, "dv": fh(ref["dv"]), "dsqk": res["dsqk"].v}
    bounds = {"dq": res["dq"].e, "dk": res["dk"].e, "dv": fh(hb["dv"]),
              "dsqk": res["dsqk"].e + 4 * U32 * abs(c["c_q"]) * res["dsqk_rows"].v.abs().sum(0)}
    return vals, bounds


def fused_values_f64(c: Dict, ref: Dict) -> Dict[str, torch.Tensor]:
    """the reference itself: qknorm_bwd_formula at float64"""
    B, H, T, d = c["q"].shape
    cc = {"sqk": c["sqk"], "c_q": c["c_q"], "B": B, "T": T, "H": H, "d": d, "gq": ref["dq"], "gk": ref["dk"]}
    fwd = {"qh": c["q"].double() / c["qpre"], "kh": c["k"].double(), "rq": c["rq"], "rk": c["rk"]}
    res = qknorm_bwd_formula(cc, fwd, F64)
    return {"dq": res["dq"], "dk": res["dk"], "dsqk": res["dsqk"]}
