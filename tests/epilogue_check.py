"""Oracles of the fused-epilogue GEMM tests (a plain helper module; test_epilogue_check.py checks it on the CPU,
test_gpu_epilogue_bounds.py uses it against the four fused launches of the persistent 256x256 NT GEMM:
nvit_gemm_nt_swiglu (EPI 3), nvit_gemm_nt_swiglu_act (EPI 6), nvit_gemm_nt_qknorm (EPI 4), each with and without a bias, and
nvit_gemm_nt_swiglu_bwd (EPI 5)).

The composition of two oracles that exist: A and B are the bf16 integers of gemm_check.nt_exact (|a|, |b| <= 2; a case
that could leave the exact range is refused by require_exact), so acc = A B^T (+ an integer bias) is exact in fp32 in any
summation order.  acc is the INPUT of the epilogue reference: a raw output (uv, vh, split-only kh) must be ONE bf16
rounding of it, bit for bit, and everything the epilogue computes is held to the row-kernel references and Ev bounds
of rowops_check.py (swiglu_eval / swiglu_formula / swiglu_bounds, qknorm_eval / qknorm_fwd_formula) with no GEMM
tolerance in them.  Nothing of those oracles is restated here; this module builds their case dicts from acc, slices
their results the way the kernels lay them out, and carries the mutants.

The exponential of these epilogues
----------------------------------
The row kernels call expf and divide; `rc._exp` allows LIB = 4 roundings for that.  The fused epilogues evaluate
sigmoid(v) as v_rcp_f32(1 + __expf(-v)), and __expf(x) is v_exp_f32(fl(x * c)) with c = fl(log2 e) = 0x1.715476p+0
(the compiler's header; no range reduction, no compensation).  Its error, relative to exp(x), to first order:

* c = log2(e) (1 + dc), |dc| <= U32                 (the constant rounded to fp32)
* y = fl(x c) = x c (1 + dm), |dm| <= U32            (the product)
  exp2(y) = exp(x (1 + dc)(1 + dm)) = exp(x) (1 + x (dc + dm)):   2 |x| U32
* v_exp_f32 is specified to 1 ulp = 2^-23 relative to its result:   2 U32

so FAST_EXP(x) = (2 |x| + 2) U32 on top of what the argument carries, against 4 U32 for expf: at |x| = 7 that is 16
roundings.  v_rcp_f32 is specified to 1 ulp (2 U32), inside the LIB = 4 that `rc._recip` allows for a division.  Neither
instruction keeps denormals, exp overflows to inf beyond |x| = 88.7 (then rcp gives 0 where the truth is below the
smallest normal), so both results also carry an ABSOLUTE error of FTZ = 2^-126.  That term matters with `gs` off,
where the pre-activations are the raw integers (|v| up to a few hundred); no other operation can underflow at the data
used here: with gs off u and v are integers (0, where the result and its bound are exactly 0, or >= 1 in magnitude),
with gs on |v| < 80 (asserted by the case builders).
`fast_math()` swaps these two rules into rowops_check for the duration of a bounds (or fp32 emulation) call; nothing
else uses them.  The allowance is derived, not tuned: a GPU margin above 1 under it is a finding to explain.

Layouts (from the launches' contracts in include/nvit_hip.h)
-----------------------------------------------------------
* EPI 3 / 6: B is the perm=1 shadow, so the output column order is interleaved (16 u | 16 v); gs and bias are read in
  that order; uv [M, 2F] leaves interleaved, xm [M, F] in natural order.
* EPI 5: N = F; uv and duv [M, 2F] are interleaved, gs and `part` are in natural (u | v) order.  part holds one fp32
  row per 128 rows of whole 256-row tiles: round_up(M, 256) / 128 rows, all written, the dead ones zero.
* EPI 4: columns are nparts stacked [C]-wide projections starting at part0 (0 = q, 1 = k, 2 = v); outputs are
  [B, H, T, 64] head tensors and rq, rk [M, H].
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional

import torch

import gemm_check as gc
import rowops_check as rc
from rowops_check import BF16T, F32T, F64, LIB, U32, Ev, deinterleave, interleave   # noqa: F401  (for the tests)

FTZ = 2.0 ** -126                       # smallest normal fp32: the absolute error of a flushed result
LOG2E_F32 = float.fromhex("0x1.715476p+0")
TILE, WAVE_ROWS, PART_ROWS, HEAD = 256, 128, 128, 64

# ------------------------------------------------------------------------------------------------ shapes
EDGE_M = [1, 129, 255, 257, 300]
SWIGLU_FK = [(128, 64), (384, 320)]     # (F, K): one column tile and one stage; three column tiles and five stages
SWIGLU_BIAS = {3: (300, 384, 320, True), 6: (129, 128, 64, False)}    # launch -> (M, F, K, gs): the one biased shape
BWD_FK = [(256, 64), (768, 320)]
# (Bsz, T, H, K, nparts, part0, sqk, bias): every (Bsz, T) with H = 12, every value of the other axes at least once
QK_CASES = [(1, 1, 12, 64, 3, 0, True, False), (300, 1, 12, 320, 1, 0, True, False), (300, 1, 4, 64, 3, 0, False, False),
            (37, 7, 12, 64, 2, 1, True, True), (37, 7, 4, 320, 3, 0, True, False), (6, 49, 12, 320, 1, 2, True, False),
            (6, 49, 4, 64, 2, 1, False, False), (3, 197, 12, 64, 3, 0, True, True),
            (3, 197, 12, 320, 3, 0, False, True), (2, 300, 12, 320, 3, 0, True, False),
            (2, 300, 4, 64, 1, 0, False, False)]
ROUNDS_K = [(128, 0), (384, 0), (384, 1)]           # (K, dynamic scheduling); dynamic engages from K = 384
ROUNDS_QK_T = 37                                    # the ragged many-round q/k case (see rounds_shape)


def qk_id(case) -> str:
    Bsz, T, H, K, nparts, part0, norm, bias = case
    return f"B{Bsz}T{T}H{H}K{K}p{part0}+{nparts}{'' if norm else '-split'}{'-bias' if bias else ''}"


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def rounds_shape(n_cu: int, T: Optional[int] = None):
    """(M, slice rows) of the many-rounds case for a grid of n_cu workgroups (a multiple of 8) and four column tiles:
    about 2.25 n_cu tiles, a ragged last row tile, and row slices of whole 256-row tiles with at most n_cu tiles each.
    T (EPI 4): M and the slices are multiples of T as well.  M = 144 * 256 + 37 at n_cu = 256.
    (T = 256 cannot have a ragged last tile, M being a multiple of T; the ragged q/k case takes T = 37.)"""
    tiles_m = (9 * n_cu // 4) // 4
    M = tiles_m * TILE + 37
    step = TILE if T is None else TILE * T // math.gcd(TILE, T)
    sl = (n_cu // 4) * TILE // step * step
    assert sl > 0, "grid too small for a slice of whole tiles and whole batches"
    if T is not None:
        M = M // T * T
        if M % TILE == 0 and T % TILE:
            M -= T
    return M, sl


# ------------------------------------------------------------------------------------------------ the fast rules
def _fast_exp(x):
    if isinstance(x, Ev):
        v = torch.exp(x.v.clamp(max=700.0))   # (fp64 stays finite; beyond, 1 / (1 + v) is far below FTZ either way)
        return Ev(v, v * (x.e + (2.0 * x.v.abs() + 2.0) * U32) + FTZ)
    if x.dtype == F32T:
        return torch.exp2(x * LOG2E_F32)      # the fp32 emulation: the constant and the product rounded as on the GPU
    return torch.exp(x)


def _fast_recip(x):
    if isinstance(x, Ev):
        v = 1.0 / x.v
        return Ev(v, v.abs() * (x.e / x.v.abs() + LIB * U32) + FTZ)
    return 1.0 / x


@contextlib.contextmanager
def swapped(**fns):
    """rowops_check's rules `name=fn` replaced for the duration (the formulas look them up at call time)"""
    old = {k: getattr(rc, k) for k in fns}
    try:
        for k, f in fns.items():
            setattr(rc, k, f)
        yield
    finally:
        for k, f in old.items():
            setattr(rc, k, f)


def fast_math():
    return swapped(_exp=_fast_exp, _recip=_fast_recip)


# ------------------------------------------------------------------------------------------------ data
def acc_of(d: Dict, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the exact fp32 accumulator entering the epilogue, in fp64: A B^T (+ bias) on `rows` (all when None)"""
    acc, _ = gc.nt_ref(d["A"], d["B"], rows, d["bias"])
    assert torch.equal(acc.float().double(), acc)
    return acc


def take_rows(t: Optional[torch.Tensor], rows: Optional[torch.Tensor]):
    return t if t is None or rows is None else t[rows]


def exact_operands(M: int, N: int, K: int, seed: int, bias: bool = False) -> Dict:
    """nt_exact with amax = 2, and every third row of A replaced by a row of B (negated for every sixth).  Random
    sums have a standard deviation of sqrt(4 K) <= 40 and never leave the 8 bits that bf16 holds exactly; an aligned
    pair sums its squares, about 2 K: from K = 320 on those accumulators (one per planted row) lie in [512, 1024),
    where bf16 steps by 4, so round-to-nearest-even, ties and truncation all differ.  Still integers of magnitude
    <= 2: the worst case that require_exact refused is unchanged."""
    d = gc.nt_exact(M, N, K, seed, amax=2, bias=bias)
    r = torch.arange(0, M, 3)
    d["A"][r] = d["B"][(5 * r + 1) % N] * (1.0 - 2.0 * (r % 2))[:, None]
    return d


def swiglu_fwd_case(M: int, F: int, K: int, seed: int, use_gs: bool = True, bias: bool = False) -> Dict:
    """Operands of EPI 3 / 6.  gs (natural order; the kernel takes interleave(gs)) is Gaussian around 1; gscale brings
    the integer sums (standard deviation sqrt(4 K): operands uniform in [-2, 2]) to swiglu_case's 1.5."""
    d = exact_operands(M, 2 * F, K, seed, bias)
    d.update(M=M, F=F, K=K, gs=gc.gauss_data((2 * F,), seed + 7) * 0.1 + 1.0 if use_gs else None,
             gscale=1.5 / math.sqrt(4.0 * K) if use_gs else 1.0)
    return d


def swiglu_fwd_c(d: Dict, rows: Optional[torch.Tensor] = None) -> Dict:
    """the swiglu_case dict of rowops_check for this launch: uv = the accumulator in natural order"""
    acc = acc_of(d, rows)
    c = {"acc": acc, "uv": deinterleave(acc, d["F"]), "suv": d["gs"], "gscale": d["gscale"],
         "dx": torch.ones((acc.shape[0], d["F"]), dtype=F64)}
    if d["gs"] is not None:
        assert (c["uv"] * d["gs"].double() * d["gscale"]).abs().max() < 80.0
    return c


def swiglu_bwd_case(M: int, F: int, K: int, seed: int, use_gs: bool = True) -> Dict:
    """Operands of EPI 5: acc = dx [M, F]; the saved uv (natural order here, the kernel reads interleave(uv)) is
    Gaussian bf16, an exact input; with gs the scaled pre-activations have swiglu_case's 1.5."""
    d = exact_operands(M, F, K, seed)
    d.update(M=M, F=F, K=K, uv=(gc.gauss_data((M, 2 * F), seed + 6) * 0.5).bfloat16(),
             gs=gc.gauss_data((2 * F,), seed + 7) * 0.1 + 1.0 if use_gs else None, gscale=3.0 if use_gs else 1.0)
    return d


def round_bf16(acc: torch.Tensor) -> torch.Tensor:
    """ONE round-to-nearest-even of the exact accumulator"""
    return acc.float().bfloat16()


def trunc_bf16(acc: torch.Tensor) -> torch.Tensor:
    """mutant: the low 16 bits dropped"""
    return (acc.float().view(torch.int32) & -65536).view(F32T).bfloat16()


def swiglu_bwd_c(d: Dict, rows: Optional[torch.Tensor] = None, dx_of=round_bf16) -> Dict:
    acc = acc_of(d, rows)
    c = {"acc": acc, "uv": take_rows(d["uv"], rows), "suv": d["gs"], "gscale": d["gscale"], "dx": dx_of(acc)}
    assert (c["uv"].double() * (1.0 if d["gs"] is None else d["gs"].double() * d["gscale"])).abs().max() < 80.0
    return c


def qk_fused_case(Bsz: int, T: int, H: int, K: int, nparts: int, part0: int, seed: int, norm: bool = True,
                  bias: bool = False) -> Dict:
    d = exact_operands(Bsz * T, nparts * H * HEAD, K, seed, bias)
    d.update(M=Bsz * T, K=K, Bsz=Bsz, T=T, H=H, nparts=nparts, part0=part0, c_q=32.0,
             sqk=rc.signed(gc.gauss_data((H * HEAD,), seed + 7) * 0.003 + 1 / 32) if norm else None)
    return d


def qk_fused_c(d: Dict, rows: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None) -> Dict:
    """The qk_case dict of rowops_check for this launch: q, k, v = the accumulator's parts (a part the launch does not
    compute is absent from c["parts"] and stands in as ones).  With `rows` the rows form one batch of len(rows) tokens:
    the head layout of sampled rows is the caller's business.  No q or k head row may have a zero sum of squares."""
    acc = acc_of(d, rows) if acc is None else acc
    R, C, H = acc.shape[0], d["H"] * HEAD, d["H"]
    parts = {d["part0"] + i: acc[:, i * C:(i + 1) * C] for i in range(d["nparts"])}
    if d["sqk"] is not None:
        for p in (0, 1):
            if p in parts:
                assert (parts[p].reshape(R, H, HEAD) ** 2).sum(-1).min() > 0, "a head row with a zero sum of squares"
    B, T = (d["Bsz"], d["T"]) if rows is None else (1, R)
    one = torch.ones((R, C), dtype=F64)
    zero = torch.zeros((B, H, T, HEAD), dtype=F64)
    return {"acc": acc, "parts": parts, "q": parts.get(0, one), "k": parts.get(1, one), "v": parts.get(2, one),
            "sqk": d["sqk"], "c_q": d["c_q"], "B": B, "T": T, "H": H, "d": HEAD, "gq": zero, "gk": zero, "gv": zero}


# ------------------------------------------------------------------------------------------------ EPI 3 / 6
def swiglu_fwd_ref(c: Dict):
    """(reference, bound) of xm [M, F]; the raw uv is round_bf16(c["acc"]), checked with assert_exact"""
    with fast_math():
        _, bnd = rc.swiglu_bounds(c)
    return rc.swiglu_eval(c)["x"], bnd["x"]


def swiglu_fwd_f32(c: Dict, fast: bool) -> torch.Tensor:
    """an fp32 evaluation of the formula, with expf and a division or with the epilogue's fast pair"""
    with (fast_math() if fast else contextlib.nullcontext()):
        return rc.swiglu_formula(c, F32T)["x"]


def swiglu_fwd_mutant(c: Dict, kind: str) -> torch.Tensor:
    F = c["uv"].shape[1] // 2
    if kind == "partner":       # u gated by the v of the neighbouring 16-column group
        return rc.swiglu_eval(dict(c, uv=torch.cat([c["uv"][:, :F], torch.roll(c["uv"][:, F:], 16, 1)], 1)))["x"]
    if kind == "sign":          # rcp(1 + exp(v)) in place of exp(-v)
        with swapped(_exp=lambda x: torch.exp(-x)):
            return rc.swiglu_formula(c, F64)["x"]
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ EPI 5
def _blocks(x: Ev, nblk: int, fill: Optional[int] = None) -> Ev:
    """[R, N] -> [nblk, 128, N]; rows past R are zero terms (fill: that row repeated - the clamped dead rows, counted)"""
    def pad(t):
        tail = torch.zeros((nblk * PART_ROWS - t.shape[0], t.shape[1]), dtype=t.dtype)
        if fill is not None:
            tail = tail + t[fill]
        return torch.cat([t, tail]).reshape(nblk, PART_ROWS, t.shape[1])
    return x.map(pad)


def part_blocks(M: int) -> int:
    return round_up(M, TILE) // PART_ROWS


def swiglu_bwd_ref(c: Dict, nblk: Optional[int] = None, mutant: Optional[str] = None):
    """(reference, bound) dicts: duv [R, 2F] natural order, and with gs: part [nblk, 2F] (row r = the sum of the
    d(suv) row terms over rows [128 r, 128 r + 128) that exist, times gscale: the rows' own bounds + red(128, .); a row
    without a live row is 0 with bound 0) and dsuv [2F].  c holds whole 128-row blocks from a block boundary on.
    mutant "dead": the clamped dead rows counted; "shift": row r holds block r + 1."""
    ref = rc.swiglu_eval(c)
    with fast_math():
        f = rc.swiglu_formula(c, "ev")
    out, bnd = {"duv": ref["duv"]}, {"duv": f["duv"].e}
    if c["suv"] is not None:
        R = c["uv"].shape[0]
        nblk = part_blocks(R) if nblk is None else nblk
        rows = _blocks(f["dsuv_rows"], nblk, R - 1 if mutant == "dead" else None)
        part = rc._view(rc._sum(rows, 1) * c["gscale"], lambda t: t.reshape(nblk, -1))
        if mutant == "shift":
            part = part.map(lambda t: torch.roll(t, -1, 0))
        out.update(part=part.v, dsuv=ref["dsuv"])
        bnd.update(part=part.e, dsuv=f["dsuv"].e)
    return out, bnd


def swiglu_bwd_f32(c: Dict, fast: bool) -> Dict[str, torch.Tensor]:
    """an fp32 evaluation: duv, and part summed in fp32 block by block"""
    with (fast_math() if fast else contextlib.nullcontext()):
        f = rc.swiglu_formula(c, F32T)
    got = {"duv": f["duv"]}
    if c["suv"] is not None:
        nblk = part_blocks(c["uv"].shape[0])
        rows = _blocks(Ev(f["dsuv_rows"]), nblk).v.float()
        got["part"] = rows.sum(1) * torch.tensor(c["gscale"], dtype=F32T)
        got["dsuv"] = got["part"].sum(0)
    return got


# ------------------------------------------------------------------------------------------------ EPI 4
def qk_fused_ref(c: Dict, q_prescale: float):
    """(reference, bound) dicts over the parts of the launch, [B, H, T, 64] and [M, H].  A bound of None: the output is
    one bf16 rounding of the reference, bit for bit (vh; split-only kh).
    q's constant is folded the way the kernel folds it, sqk * fl(c_q * q_prescale): the two constants rounded to fp32
    and their product rounded once more, carried through Ev; q is compared as stored."""
    parts, norm = c["parts"], c["sqk"] is not None
    ref, bnd = {}, {}
    hd = lambda x: rc.to_heads(x, c["B"], c["T"], c["H"], HEAD)
    if 2 in parts:
        ref["vh"], bnd["vh"] = hd(parts[2]), None
    if not norm:
        if 1 in parts:
            ref["kh"], bnd["kh"] = hd(parts[1]), None
        if 0 in parts:
            q = Ev(parts[0]) * Ev.lift(q_prescale)
            ref["qh"], bnd["qh"] = hd(q.v), hd(q.e)
        return ref, bnd
    if 1 in parts:
        r, f = rc.qknorm_eval(c), rc.qknorm_fwd_formula(c, "ev")
        ref.update(kh=r["kh"], rk=r["rk"])
        bnd.update(kh=f["kh"].e, rk=f["rk"].e)
    if 0 in parts:
        r = rc.qknorm_eval(dict(c, c_q=c["c_q"] * q_prescale))
        f = rc.qknorm_fwd_formula(dict(c, c_q=Ev.lift(c["c_q"]) * Ev.lift(q_prescale)), "ev")
        ref.update(qh=r["qh"], rq=r["rq"])
        bnd.update(qh=f["qh"].e, rq=f["rq"].e)
    return ref, bnd


def qk_fused_f32(c: Dict, q_prescale: float) -> Dict[str, torch.Tensor]:
    """an fp32 evaluation of the outputs that have a bound"""
    parts, got = c["parts"], {}
    f32 = lambda x: torch.tensor(x, dtype=F32T)
    if c["sqk"] is None:
        if 0 in parts:
            got["qh"] = rc.to_heads(parts[0].float() * f32(q_prescale), c["B"], c["T"], c["H"], HEAD)
        return got
    if 1 in parts:
        f = rc.qknorm_fwd_formula(c, F32T)
        got.update(kh=f["kh"], rk=f["rk"])
    if 0 in parts:
        f = rc.qknorm_fwd_formula(dict(c, c_q=float(f32(c["c_q"]) * f32(q_prescale))), F32T)
        got.update(qh=f["qh"], rq=f["rq"])
    return got


def qk_fused_mutant(c: Dict, q_prescale: float, kind: str, bias: Optional[torch.Tensor] = None,
                    part0: int = 0) -> Dict[str, torch.Tensor]:
    """group32 / group128: normalised over 32 or 128 columns; prescale_k: q_prescale on k as well; bias_late: the bias
    joins after the sum of squares (bias: the launch's, stacked from part0 on)."""
    qc = dict(c, c_q=c["c_q"] * q_prescale)
    if kind in ("group32", "group128"):
        g = int(kind[5:])
        return {"qh": rc.qknorm_eval(qc, group=g)["qh"], "kh": rc.qknorm_eval(c, group=g)["kh"]}
    if kind == "prescale_k":
        return {"kh": rc.qknorm_eval(qc)["kh"]}
    if kind == "bias_late":
        C = c["H"] * HEAD
        out = {}
        for p, n, cc in ((0, "q", qc), (1, "k", c)):
            if p in c["parts"]:
                b = bias[(p - part0) * C:(p - part0 + 1) * C].double()
                x = c["parts"][p]
                ratio = ((x ** 2).reshape(-1, c["H"], HEAD).sum(-1) / ((x - b) ** 2).reshape(-1, c["H"], HEAD).sum(-1)).sqrt()
                scale = rc.to_heads(ratio[:, :, None].expand(-1, -1, HEAD).reshape(-1, C), c["B"], c["T"], c["H"], HEAD)
                out[n + "h"] = rc.qknorm_eval(cc)[n + "h"] * scale
        return out
    raise ValueError(kind)


def head_scatter(x: torch.Tensor, B: int, T: int, H: int, wraps: Optional[int] = None) -> torch.Tensor:
    """[M, C] rows placed into [B, H, T, 64] the way the epilogue addresses them: the (batch, token) of a wave tile's
    first row (128 rows per wave tile) from one division, then a step per row, wrapping into the next batch while the
    token is >= T.  wraps None: as often as needed (= to_heads).  The mutants wrap at most `wraps` times: 0 = the row
    lands at (b, t) of the wave tile's batch unwrapped, 1 = the `if` that is enough from T = 128 on.  A row whose
    address falls outside the tensor is dropped; what no row reaches keeps the correct value."""
    M = x.shape[0]
    out = rc.to_heads(x, B, T, H, HEAD).clone().reshape(B * H * T, HEAD)
    if wraps is None:
        return out.reshape(B, H, T, HEAD)
    m = torch.arange(M)
    b = (m // WAVE_ROWS * WAVE_ROWS) // T
    t = m - b * T
    for _ in range(wraps):
        over = (t >= T).long()
        t, b = t - over * T, b + over
    for h in range(H):
        dst = (b * H + h) * T + t
        ok = dst < B * H * T
        out[dst[ok]] = x[:, h * HEAD:(h + 1) * HEAD][ok]
    return out.reshape(B, H, T, HEAD)


# ------------------------------------------------------------------------------------------------ checks
def check_or_exact(out: torch.Tensor, ref: torch.Tensor, bound: Optional[torch.Tensor], label: str,
                   verbose: bool = True) -> Optional[float]:
    """bound None: bit-identical to one rounding of the exact reference (returns None); otherwise kohonen_check.check
    (+ half a bf16 ulp for a bf16 output), returning the largest err / bound"""
    if bound is None:
        gc.assert_exact(out.detach().cpu(), ref, label)
        if verbose:
            print(f"   {label}: exact bits")
        return None
    return rc.check(out, ref, bound, label, verbose)


def margin(out: torch.Tensor, ref: torch.Tensor, bound: Optional[torch.Tensor]) -> float:
    """the largest err / bound that check_or_exact would judge, without judging it (the mutants' figures): inf for a
    non-finite output, an error where the bound is 0, or other bits than the exact ones"""
    out = out.detach().cpu()
    if bound is None:
        return 0.0 if gc.bits_equal(gc._plus_zero(out), gc._plus_zero(gc.expected_exact(ref, out.dtype))) else math.inf
    if not torch.isfinite(out.float()).all():
        return math.inf
    ref = ref.detach().to(F64)
    b = torch.as_tensor(bound, dtype=F64).expand(ref.shape)
    if out.dtype == BF16T:
        b = b + gc.half_ulp_bf16(ref.abs() + b)
    err = (out.double() - ref).abs()
    ratio = torch.where(b > 0, err / b, torch.where(err > 0, math.inf, 0.0))
    return ratio.max().item()


def misrounded(out: torch.Tensor, ref: torch.Tensor) -> float:
    """share of a bf16 output's elements that are not the fp64 reference rounded to nearest even: what the epilogue's
    fp32 arithmetic moved across a rounding boundary (the margin of a bf16 output is about 1 whenever it rounds right)"""
    return (out.detach().cpu() != ref.float().bfloat16()).double().mean().item()


def crossed(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """A bf16 output's fp32 error that shows through its rounding, over its fp32 bound (without the half ulp): where
    the output is not the rounded reference, the value before rounding lay beyond the midpoint between the two, so its
    error was at least the reference's distance to that midpoint.  The largest such ratio: a lower estimate of the
    margin the fp32 arithmetic has under the Ev bound (0 when every element rounds like the reference)."""
    out, ref = out.detach().cpu(), ref.detach().to(F64)
    want = ref.float().bfloat16()
    off = out != want
    if not off.any():
        return 0.0
    mid = (out.double() + want.double()) / 2
    b = torch.as_tensor(bound, dtype=F64).expand(ref.shape)[off]
    return ((ref - mid).abs()[off] / b.clamp(min=FTZ)).max().item()
