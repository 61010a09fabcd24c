"""Oracles of the GEMM tests (a plain helper module; test_gemm_bounds.py checks it on the CPU, test_gpu_gemm.py and
test_gpu_ops.py use it against the HIP kernels).

Two oracles, both with an fp64 reference computed on the CPU from the exact operands the kernel saw:

* exact data (the main one): operands, bias, rowadd and an accumulated old C are small integers, colscale is a
  power of two.  `require_exact` refuses any case in which a partial sum could reach 2^24, so every fp32
  intermediate is exact whatever the summation order (MFMA internal order, K slabs, TN splits).  Then an fp32
  output must be bit-identical to the reference and a bf16 output bit-identical to ONE round-to-nearest-even of it.
  A dropped or doubled slab / row / column, a wrong epilogue order, truncation instead of rounding, a second rounding
  or a bf16 intermediate all fail; no tolerance is involved.
* Gaussian data (for fp32 operands, where integers cannot show an operand rounded to bf16): per element
  |out - ref| <= LAMBDA * sqrt(K_eff) * 2^-24 * mag (+ half a bf16 ulp of the reference for bf16 output), with
  mag = (|A| |B|^T + |bias|) * |colscale| + |rowadd| + |old C| and LAMBDA = 8 (the probabilistic bound of
  Higham and Mary for mean-zero data).  K_eff = K for NT, Mred + splits for TN.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

U32 = 2.0 ** -24        # unit roundoff of fp32
LAMBDA = 8.0
EXACT_LIMIT = 2 ** 24   # integers below this are exact in fp32
POW2_SCALES = (-2.0, -1.0, 1.0, 2.0, 4.0)


# ---------------------------------------------------------------------------------------------- data
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def int_data(shape, amax: int, seed: int) -> torch.Tensor:
    """fp32 tensor of integers in [-amax, amax]."""
    return torch.randint(-amax, amax + 1, tuple(shape), generator=_gen(seed)).float()


def gauss_data(shape, seed: int) -> torch.Tensor:
    return torch.randn(tuple(shape), generator=_gen(seed))


def pow2_data(n: int, seed: int) -> torch.Tensor:
    s = torch.tensor(POW2_SCALES)
    return s[torch.randint(0, len(POW2_SCALES), (n,), generator=_gen(seed))]


def require_exact(k_eff: int, amax_a: float, amax_b: float, addend: float = 0.0, scale: float = 1.0,
                  pre_scale: float = 0.0) -> None:
    """Refuse a case whose fp32 partial sums could reach 2^24: |sum| <= k_eff * amax_a * amax_b, then
    (sum + pre_scale) * scale + addend.  Every value is an integer, so below the limit every one is exact."""
    worst = (k_eff * amax_a * amax_b + pre_scale) * scale + addend
    if worst >= EXACT_LIMIT:
        raise ValueError(f"exact-data case out of range: partial sums up to {worst:.0f} >= 2^24 "
                         f"(K_eff={k_eff}, |a|<={amax_a}, |b|<={amax_b}, addends {addend}, scale {scale})")


def nt_exact(M: int, N: int, K: int, seed: int, *, amax: int = 4, bias: bool = False, colscale: bool = False,
             period: int = 0, old_amax: float = 0.0) -> dict:
    """Integer operands (and epilogue vectors) of C[M,N] = A[M,K] B[N,K]^T; old_amax bounds an accumulated old C."""
    bmax, rmax = 8, 16
    smax = max(abs(s) for s in POW2_SCALES) if colscale else 1.0
    require_exact(K, amax, amax, addend=(rmax if period else 0) + old_amax, scale=smax,
                  pre_scale=bmax if bias else 0)
    d = {"A": int_data((M, K), amax, seed), "B": int_data((N, K), amax, seed + 1), "bias": None, "colscale": None,
         "rowadd": None, "period": period}
    if bias:
        d["bias"] = int_data((N,), bmax, seed + 2)
    if colscale:
        d["colscale"] = pow2_data(N, seed + 3)
    if period:
        d["rowadd"] = int_data((period, N), rmax, seed + 4)
    return d


def tn_exact(Mred: int, N: int, K: int, seed: int, *, amax: int = 4, old_amax: float = 0.0) -> dict:
    """Integer operands of G[N,K] = sum_m A[m,N] B[m,K] over Mred rows."""
    require_exact(Mred, amax, amax, addend=old_amax)
    return {"A": int_data((Mred, N), amax, seed), "B": int_data((Mred, K), amax, seed + 1)}


def cancelling_old(ref: torch.Tensor, seed: int, rel: float = 2.0 ** -5) -> torch.Tensor:
    """An old C of about -ref * (1 + small noise), rounded to integers (exact in bf16 below 256, and an integer
    whatever bf16 rounds it to above): the "+=" result is then small and a second rounding shows in full."""
    noise = (torch.rand(ref.shape, generator=_gen(seed), dtype=torch.float64) * 2 - 1) * rel
    return torch.round(-ref * (1 + noise)).float()


def sample_rows(M: int, tile: int = 256, nrand: int = 64, seed: int = 0) -> Optional[torch.Tensor]:
    """Rows of a large output checked against the fp64 reference: the first and the last tile in full, the first and
    last row of every tile, and some random rows.  None = all rows (small shapes are checked in full)."""
    if M <= 4 * tile:
        return None
    rows = set(range(0, tile)) | set(range((M - 1) // tile * tile, M))
    for t0 in range(0, M, tile):
        rows.add(t0)
        rows.add(min(t0 + tile, M) - 1)
    rows |= set(torch.randint(0, M, (nrand,), generator=_gen(seed)).tolist())
    return torch.tensor(sorted(rows), dtype=torch.long)


# ---------------------------------------------------------------------------------------------- references
def nt_ref(A, B, rows=None, bias=None, colscale=None, rowadd=None, period=0, old=None):
    """fp64 reference and magnitude of out[m] = ((A B^T + bias) * colscale + rowadd[m % period]) + old[m] on the
    rows `rows` (all when None).  `old` is given for the same rows.  Tensors are CPU; returns (ref, mag)."""
    M = A.shape[0]
    idx = torch.arange(M) if rows is None else rows
    a = A[idx].double()
    b = B.double()
    ref = a @ b.t()
    mag = a.abs() @ b.abs().t()
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if colscale is not None:
        ref = ref * colscale.double()
        mag = mag * colscale.double().abs()
    if rowadd is not None:
        r = rowadd.double()[idx % period]
        ref = ref + r
        mag = mag + r.abs()
    if old is not None:
        ref = ref + old.double()
        mag = mag + old.double().abs()
    return ref, mag


def perm_rows(N: int) -> torch.Tensor:
    """Master row of shadow row s for perm=1 (the SwiGLU u16|v16 interleave, nvit_shadow_weights)."""
    s = torch.arange(N)
    q, w = s // 32, s % 32
    return torch.where(w < 16, q * 16 + w, N // 2 + q * 16 + (w - 16))


def tn_ref(A, B, Mred, perm=0, old=None):
    """fp64 reference and magnitude of G[perm(n), k] = sum_{m < Mred} A[m, n] B[m, k] (+ old, in master order)."""
    a, b = A[:Mred].double(), B[:Mred].double()
    ref, mag = a.t() @ b, a.abs().t() @ b.abs()
    if perm:
        p = perm_rows(ref.shape[0])
        r2, m2 = torch.empty_like(ref), torch.empty_like(mag)
        r2[p], m2[p] = ref, mag
        ref, mag = r2, m2
    if old is not None:
        ref = ref + old.double()
        mag = mag + old.double().abs()
    return ref, mag


# ---------------------------------------------------------------------------------------------- checks
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality (NaN payloads included)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def expected_exact(ref: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """The only acceptable output for an exact reference: fp32 itself, or one round-to-nearest-even to bf16."""
    want = ref.float()
    assert torch.equal(want.double(), ref), "reference is not exact in fp32: the case is out of range"
    return want if out_dtype == torch.float32 else want.bfloat16()


def _plus_zero(t: torch.Tensor) -> torch.Tensor:
    return torch.where(t == 0, torch.zeros_like(t), t)


def assert_exact(out: torch.Tensor, ref: torch.Tensor, label: str = "") -> None:
    """out (CPU, fp32 or bf16) must be bit-identical to the single rounding of the exact fp64 reference.  The one
    freedom: the sign of an exact zero (a kernel's accumulator starts at +0, so +0 + (-0) = +0 where the fp64 product
    of a single term is -0)."""
    want = _plus_zero(expected_exact(ref, out.dtype))
    out = _plus_zero(out)
    if bits_equal(out, want):
        return
    bad = (_bits(out.contiguous()) != _bits(want)).nonzero()
    i = tuple(bad[0].tolist())
    raise AssertionError(f"{label}: {bad.shape[0]} of {out.numel()} elements differ from the exact result; first at "
                         f"{i}: got {out[i].item()!r}, want {want[i].item()!r} (exact {ref[i].item()!r})")


def half_ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Half a bf16 ulp at |x| (8 significant bits), 0 where x == 0."""
    ax = x.abs().double()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    return torch.where(ax > 0, torch.exp2(e - 8), torch.zeros_like(ax))


def gauss_bound(ref: torch.Tensor, mag: torch.Tensor, k_eff: int, out_dtype: torch.dtype,
                lam: float = LAMBDA) -> torch.Tensor:
    b = lam * math.sqrt(k_eff) * U32 * mag
    if out_dtype == torch.bfloat16:
        b = b + half_ulp_bf16(ref.abs() + b)
    return b


def check_gauss(out: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, k_eff: int, label: str = "",
                verbose: bool = True) -> float:
    """Assert |out - ref| <= bound element-wise; returns max(err / bound) (printed: margins stay visible).  For bf16
    output the half-ulp term dominates and a correctly rounded result reaches it: margins close to 1 are expected
    there; the fp32-output margins show the accumulation headroom."""
    assert torch.isfinite(out).all(), f"{label}: non-finite output"
    err = (out.double() - ref).abs()
    b = gauss_bound(ref, mag, k_eff, out.dtype)
    zero = b == 0
    assert not (err[zero] > 0).any(), f"{label}: nonzero error where the result must be exact"
    margin = (err[~zero] / b[~zero]).max().item() if (~zero).any() else 0.0
    if verbose:
        print(f"   {label}: max err/bound {margin:.3f} (K_eff {k_eff})")
    assert margin <= 1.0, f"{label}: max err/bound {margin:.3f} > 1"
    return margin


def old_tol_or_bound(old_tol: float, ref, mag, k_eff, out_dtype) -> torch.Tensor:
    """Element-wise min(old tolerance, Gaussian bound): a tightened assertion that can never be looser than before."""
    return torch.clamp(gauss_bound(ref, mag, k_eff, out_dtype), max=old_tol)
