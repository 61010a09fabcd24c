"""Thin Python wrappers over the C ABI (include/nvit_hip.h).

PyTorch is used here only as plumbing: device memory (caching allocator), the current HIP
stream, and dtype bookkeeping.  Every function enqueues hand-written HIP kernels on
`torch.cuda.current_stream()`; nothing falls back to torch operators.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib, resample
from ._lib import BF16, F32, call, check  # noqa: F401 (check: tests make raw calls through ops.check)

Tensor = torch.Tensor
# layout numbers shared with the kernels: each is written once, in include/nvit_hip.h
MAX_PART_BLOCKS = _lib.const("MAX_PART_BLOCKS")   # the most workgroups a backward row kernel accepts
ROW_WAVES = _lib.const("ROW_WAVES")   # rows in flight per workgroup; per-wave partial arrays hold ROW_WAVES * nblk rows
ROW_GRID_MAX = _lib.const("ROW_GRID_MAX")   # workgroups of a forward row kernel's grid; more rows are walked with a stride
PAD_HEAD_DIM = _lib.const("PAD_HEAD_DIM")   # dp: the attention head dim the zero-padded head tensors run at
REDUCE_MAX_ITEMS = _lib.const("COLSUM_REDUCE_MAX_ITEMS")   # reductions nvit_colsum_reduce_multi takes in one launch
ATTN_BWD_PART_ROWS = _lib.const("ATTN_BWD_PART_ROWS")   # tokens per row of nvit_attn_bwd_qknorm's d(sqk) partials
SWIGLU_BWD_TILE_ROWS = _lib.const("SWIGLU_BWD_TILE_ROWS")   # nvit_gemm_nt_swiglu_bwd: d(suv) partials, one row per
SWIGLU_BWD_PART_ROWS = _lib.const("SWIGLU_BWD_PART_ROWS")   #   PART_ROWS rows of whole TILE_ROWS-row tiles
PATCH_K_STEP = _lib.const("PATCH_EMBED_K_STEP")   # nvit_patch_embed_fwd: patch length padded to whole stages,
PATCH_TILE_ROWS = _lib.const("PATCH_EMBED_TILE_ROWS")   #   saved patch rows to whole row tiles
SHADOW_TILE = _lib.const("SHADOW_TILE")   # nvit_shadow_weights: edge of a work item


def tdtype(dt: int) -> torch.dtype:
    return torch.float32 if dt == F32 else torch.bfloat16


def dt_of(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("nvit_amd ops need device tensors: the nViT hot path has no CPU fallback")


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def bk_of(dt: int) -> int:
    return 32 if dt == F32 else 64


# ----------------------------------------------------------------------------- GEMMs
def gemm_nt(A: Tensor, B: Tensor, M: int, N: int, K: int, out: Optional[Tensor] = None,
            out_dtype: torch.dtype = torch.float32, bias: Optional[Tensor] = None,
            colscale: Optional[Tensor] = None, rowadd: Optional[Tensor] = None, rowadd_period: int = 0,
            accumulate: bool = False, lda: Optional[int] = None, ldb: Optional[int] = None,
            ldc: Optional[int] = None) -> Tensor:
    """out[M,N] = A[M,K] @ B[N,K]^T (+epilogue). A,B same dtype (fp32 or bf16)."""
    _chk_dev(A, B)
    dt = dt_of(A)
    assert dt_of(B) == dt
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=out_dtype)
    ldc = out.stride(0) if ldc is None else ldc
    call("nvit_gemm_nt", dt, A, lda, B, ldb, out, ldc, dt_of(out), M, N, K, bias, colscale, rowadd, rowadd_period,
         int(accumulate), _s())
    return out


FUSE_MIN_ELEMS = 256 * 256 * 64   # below this output size the fused persistent kernel is not worth a launch


def fusable(dt: int, M: int, N: int, K: int) -> bool:
    """True when the fused-epilogue persistent GEMM (nvit_gemm_nt_swiglu / _swiglu_act / _qknorm, each with or without a
    bias) can and should be used."""
    return bool(_lib.load().nvit_gemm_nt_fusable(dt, M, N, K)) and M * N >= FUSE_MIN_ELEMS


def _chk_fused_bias(bias: Optional[Tensor], n: int, ref: Tensor, what: str) -> None:
    """The bias of a fused-epilogue GEMM: contiguous fp32 [n] on the operands' device (the kernel reads it unchecked)."""
    if bias is None:
        return
    if (bias.dtype != torch.float32 or bias.dim() != 1 or bias.numel() != n or not bias.is_contiguous()
            or bias.device != ref.device):
        raise ValueError(f"{what}: bias must be a contiguous fp32 tensor of {n} elements on {ref.device}, got "
                         f"{bias.dtype} {tuple(bias.shape)} stride {bias.stride()} on {bias.device}")


def gemm_nt_swiglu(A: Tensor, B: Tensor, M: int, F: int, K: int, gs: Optional[Tensor], gscale: float, *,
                   bias: Optional[Tensor] = None):
    """uv [M,2F] (raw, interleaved) and xm [M,F] = swiglu(uv) in one launch (bf16).
    bias: fp32 [2F] in the interleaved column order of B (like gs), part of uv."""
    _chk_dev(A, B)
    _chk_fused_bias(bias, 2 * F, A, "gemm_nt_swiglu")
    uv = torch.empty((M, 2 * F), device=A.device, dtype=torch.bfloat16)
    xm = torch.empty((M, F), device=A.device, dtype=torch.bfloat16)
    call("nvit_gemm_nt_swiglu", dt_of(A), A, A.stride(0), B, B.stride(0), uv, xm, M, F, K, gs, gscale, bias, _s())
    return uv, xm


def gemm_nt_swiglu_act(A: Tensor, B: Tensor, M: int, F: int, K: int, gs: Optional[Tensor], gscale: float, *,
                       bias: Optional[Tensor] = None) -> Tensor:
    """xm [M,F] of gemm_nt_swiglu, bit for bit, without the raw uv store (forward-only calls; bf16)."""
    _chk_dev(A, B)
    _chk_fused_bias(bias, 2 * F, A, "gemm_nt_swiglu_act")
    xm = torch.empty((M, F), device=A.device, dtype=torch.bfloat16)
    call("nvit_gemm_nt_swiglu_act", dt_of(A), A, A.stride(0), B, B.stride(0), xm, M, F, K, gs, gscale, bias, _s())
    return xm


def gemm_nt_swiglu_bwd(A: Tensor, B: Tensor, uv: Tensor, M: int, F: int, K: int, gs: Optional[Tensor], gscale: float):
    """duv [M,2F] (interleaved) and the d(suv) partials from dy [M,K] and W^T [F,K] in one launch (bf16)."""
    _chk_dev(A, B, uv)
    duv = torch.empty((M, 2 * F), device=A.device, dtype=torch.bfloat16)
    part = (torch.empty((round_up(M, SWIGLU_BWD_TILE_ROWS) // SWIGLU_BWD_PART_ROWS, 2 * F), device=A.device,
                        dtype=torch.float32) if gs is not None else None)
    call("nvit_gemm_nt_swiglu_bwd", dt_of(A), A, A.stride(0), B, B.stride(0), uv, duv, part, M, F, K, gs, gscale, _s())
    return duv, part


def qk_buffers(dt: int, B: int, T: int, H: int, d: int, device, norm: bool = True):
    """qh, kh, vh [B,H,T,d] and (norm) rq, rk [B*T,H]; without the normalise rq, rk are None."""
    td = tdtype(dt)
    qh = torch.empty((B, H, T, d), device=device, dtype=td)
    if not norm:
        return qh, torch.empty_like(qh), torch.empty_like(qh), None, None
    return (qh, torch.empty_like(qh), torch.empty_like(qh),
            torch.empty((B * T, H), device=device, dtype=torch.float32),
            torch.empty((B * T, H), device=device, dtype=torch.float32))


LOG2E = 1.4426950408889634


def attn_q_prescale(d: int) -> float:
    """The factor that, folded into q_hat by its producer, turns the MFMA result into the score in log2 units:
    sqrt(d) * log2(e) - the exponent of the attention kernels then needs no multiply (nvit_attn_fwd_bounded)."""
    return math.sqrt(d) * LOG2E


def gemm_nt_qknorm(A: Tensor, B: Tensor, M: int, K: int, nparts: int, part0: int, sqk: Optional[Tensor], c_q: float,
                   Bsz: int, T: int, H: int, d: int, bufs=None, q_prescale: float = 1.0, *,
                   bias: Optional[Tensor] = None):
    """q/k/v projection(s) with the per-head normalise, sqk scale and head split fused (bf16, d=64).
    sqk None: the head split alone (plain-ViT attention; rq, rk None).
    q_prescale: extra factor folded into the q part (pass the same value to attn_fwd / attn_bwd_qknorm).
    bias: fp32 [nparts*H*d], the stacked biases of this launch's projections, added before the normalise."""
    _chk_dev(A, B)
    _chk_fused_bias(bias, nparts * H * d, A, "gemm_nt_qknorm")
    if bufs is None:
        bufs = qk_buffers(dt_of(A), Bsz, T, H, d, A.device, norm=sqk is not None)
    qh, kh, vh, rq, rk = bufs
    call("nvit_gemm_nt_qknorm", dt_of(A), A, A.stride(0), B, B.stride(0), M, K, nparts, part0, sqk, c_q, q_prescale, qh, kh,
         vh, rq, rk, T, H, d, bias, _s())
    return bufs


_ws_cache = {}


def _workspace(nbytes: int, device) -> Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(max(nbytes // 4 + 1, 1 << 20), device=device, dtype=torch.float32)
        _ws_cache[key] = ws
    return ws


def tn_splits(Mred: int, N: int, K: int, dt: int) -> int:
    if N % 256 == 0 and K % 256 == 0 and Mred >= 4096:
        # persistent 256x256 kernel: (tiles x splits) work items dealt over 256 workgroups; pick the
        # split count that fills whole rounds best (fewest splits on ties: less slab traffic)
        tiles = (N // 256) * (K // 256)
        flops = 2.0 * Mred * N * K
        best, best_t = 1, float("inf")
        for s in range(1, 65):
            if Mred // s < 1024:
                break
            items = tiles * s
            eff = items / (math.ceil(items / 256) * 256)
            t = flops / (1.0e15 * eff) + 2.0 * s * N * K * 4 / 4.0e12  # MFMA time + slab write/read
            if t < best_t:
                best, best_t = s, t
        return best
    tiles = math.ceil(N / 128) * math.ceil(K / 128)
    rb = bk_of(dt)
    want = max(1, math.ceil(1024 / tiles))
    return max(1, min(want, math.ceil(Mred / (4 * rb)), 64))


def gemm_tn(A: Tensor, B: Tensor, G: Tensor, Mred: int, N: int, K: int, perm: int = 0, accumulate: bool = False,
            lda: Optional[int] = None, ldb: Optional[int] = None, ldg: Optional[int] = None) -> Tensor:
    """G[N,K] (+)= A[Mred,N]^T @ B[Mred,K]; G fp32."""
    _chk_dev(A, B, G)
    dt = dt_of(A)
    assert dt_of(B) == dt and G.dtype == torch.float32
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldg = G.stride(0) if ldg is None else ldg
    splits = tn_splits(Mred, N, K, dt)
    nbytes = splits * N * K * 4 + 256
    ws = _workspace(nbytes, A.device)
    call("nvit_gemm_tn", dt, A, lda, B, ldb, G, ldg, Mred, N, K, splits, ws, ws.numel() * 4, perm, int(accumulate), _s())
    return G


# ----------------------------------------------------------------------------- row ops
_LERP_BWD_BLOCKS: dict = {}
PART_BLOCKS = 1024   # workgroups of the backward row kernels
assert PART_BLOCKS <= MAX_PART_BLOCKS


def _row_part_blocks(M: int) -> int:
    return min(PART_BLOCKS, math.ceil(M / ROW_WAVES))


def _part_blocks(nblk: Optional[int], default: int, name: str) -> int:
    """Workgroups of a backward row kernel: the wrapper's own choice, or the caller's `nblk` as given (tests use it to
    make a wave walk several rows at a small M; the partial arrays are sized from it)."""
    if nblk is None:
        return default
    if isinstance(nblk, bool) or not isinstance(nblk, int) or not 1 <= nblk <= MAX_PART_BLOCKS:
        raise ValueError(f"{name}: nblk must be an integer in 1..{MAX_PART_BLOCKS}, got {nblk!r}")
    return nblk


def _chk_gate(gate: Optional[Tensor], M: int, ref: Tensor, what: str) -> int:
    """-> rows_per_sample of a row kernel's optional gate (1 without one): `gate` holds one fp32 gate per sample (a row of
    DropPath's table), the [M, C] operands hold M / gate.numel() consecutive rows per sample.  The kernel indexes it
    unchecked."""
    if gate is None:
        return 1
    if (not isinstance(gate, Tensor) or gate.dtype != torch.float32 or gate.dim() != 1 or not gate.is_contiguous()
            or gate.device != ref.device or gate.numel() < 1 or M % gate.numel()):
        raise ValueError(f"{what}: gate must be a contiguous fp32 vector on {ref.device} whose length divides M={M}")
    return M // gate.numel()


def lerp_fwd(dt: int, h: Tensor, y: Tensor, alpha: Tensor, c_a: float, skip_x: Optional[Tensor] = None,
             skip: Optional[Tensor] = None, want_lo: bool = True, *,
             gate: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """gate (fp32 [B], M = B * rows per sample; stochastic depth): the gated kernel, out = nrm(a + gate * lam * (b - a))."""
    M, Cc = h.shape
    out = torch.empty_like(h)
    out_lo = torch.empty((M, Cc), device=h.device, dtype=tdtype(dt)) if want_lo else None
    T = _chk_gate(gate, M, h, "lerp_fwd")
    call("nvit_lerp_fwd", dt, h, y, dt_of(y), alpha, c_a, skip_x, skip, gate, T, out, out_lo, M, Cc, _s())
    return out, out_lo


def lerp_bwd(dt: int, dout: Tensor, h: Tensor, y: Tensor, alpha: Tensor, c_a: float, skip_x: Optional[Tensor],
             skip: Optional[Tensor], dh: Optional[Tensor], accum_dh: bool, want_dy_f32: bool, want_dy_lo: bool,
             dout_add: Optional[Tensor] = None, *, nblk: Optional[int] = None, gate: Optional[Tensor] = None):
    """-> dh, dy_f32|None, dy_lo|None, dskip_x|None, part_dlam [ROW_WAVES*nblk,C], part_dskip|None.
    dout_add: optional bf16 [M,C] added to dout inside the kernel (a data-gradient GEMM's output).
    nblk: workgroups to launch instead of the resident count (1..MAX_PART_BLOCKS).
    gate: as in lerp_fwd; the gated kernel is built for the block chain's two calls only (skip_x without accum_dh, or
    accum_dh without skip_x)."""
    if dout_add is not None and (dout_add.dtype != torch.bfloat16 or dout_add.shape != h.shape or not dout_add.is_contiguous()):
        raise ValueError("lerp_bwd: dout_add must be a contiguous bf16 [M,C] tensor")
    M, Cc = h.shape
    dev = h.device
    if dh is None:
        dh = torch.empty_like(h)
        accum_dh = False
    gated = gate is not None
    T = _chk_gate(gate, M, h, "lerp_bwd")
    if gated and (skip_x is not None) == bool(accum_dh):
        raise ValueError("lerp_bwd: the gated kernel takes skip_x without accum_dh, or accum_dh without skip_x")
    # grid = the workgroups resident at once for this kernel variant (a second, partly filled round of a 1024-block
    # grid cost 1.8 ms per Base step)
    key = (dt, dt_of(y), Cc, dout_add is not None, skip_x is not None, bool(accum_dh), gated)
    nres = _LERP_BWD_BLOCKS.get(key)
    if nres is None:
        nres = int(_lib.load().nvit_lerp_bwd_blocks(dt, dt_of(y), Cc, int(key[3]), int(key[4]), int(key[5]),
                                                    int(gated))) or PART_BLOCKS
        _LERP_BWD_BLOCKS[key] = nres
    nblk = _part_blocks(nblk, min(nres, math.ceil(M / ROW_WAVES)), "lerp_bwd")
    dy = torch.empty_like(h) if want_dy_f32 else None
    dy_lo = torch.empty((M, Cc), device=dev, dtype=tdtype(dt)) if want_dy_lo else None
    dskip_x = torch.empty_like(h) if skip_x is not None else None
    part = torch.empty((ROW_WAVES * nblk, Cc), device=dev, dtype=torch.float32)   # one row of column partials per wave
    pskip = torch.empty((ROW_WAVES * nblk,), device=dev, dtype=torch.float32) if skip_x is not None else None
    call("nvit_lerp_bwd", dt, dout, dout_add, h, y, dt_of(y), alpha, c_a, skip_x, skip, gate, T, dh, int(accum_dh), dy,
         dy_lo, dskip_x, part, pskip, nblk, M, Cc, _s())
    return dh, dy, dy_lo, dskip_x, part, pskip


def rmsnorm_fwd(x: Tensor, w: Tensor, eps: float):
    M, Cc = x.shape
    out = torch.empty_like(x)
    rstd = torch.empty((M,), device=x.device, dtype=torch.float32)
    call("nvit_rmsnorm_fwd", x, w, eps, out, rstd, M, Cc, _s())
    return out, rstd


def rmsnorm_bwd(dout: Tensor, x: Tensor, w: Tensor, rstd: Tensor, *, nblk: Optional[int] = None):
    """-> dx [M,C], dw [C]"""
    M, Cc = x.shape
    nblk = _part_blocks(nblk, _row_part_blocks(M), "rmsnorm_bwd")
    dx = torch.empty_like(x)
    part = torch.empty((nblk, Cc), device=x.device, dtype=torch.float32)
    call("nvit_rmsnorm_bwd", dout, x, w, rstd, dx, part, nblk, M, Cc, _s())
    dw = torch.empty((Cc,), device=x.device, dtype=torch.float32)
    colsum_reduce(part, dw, False)
    return dx, dw


def _chk_rows(shape, *ts, f32=(), name=""):
    """Row-kernel operands: device tensors, contiguous, of the [M,C] (or [C]) shape the kernel indexes; `f32` must be
    fp32, the others fp32 or bf16."""
    for t in ts + tuple(f32):
        if t is None:
            continue
        _chk_dev(t)
        if not t.is_contiguous():
            raise ValueError(f"{name}: operands must be contiguous")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{name}: fp32 or bf16 operands expected, got {t.dtype}")
    for t in f32:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{name}: fp32 operand expected, got {t.dtype}")
    for t in ts + tuple(f32):
        if t is not None and t.dim() == 2 and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: operand of shape {tuple(t.shape)}, expected {tuple(shape)}")


def _chk_vec(C: int, *vs, name=""):
    for v in vs:
        _chk_dev(v)
        if v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != C:
            raise ValueError(f"{name}: contiguous fp32 vector of {C} elements expected")


def res_rmsnorm_fwd(dt: int, a: Tensor, y: Optional[Tensor], w: Tensor, eps: float, want_lo: bool = True, *,
                    gate: Optional[Tensor] = None):
    """out = rms(a + y) * w (y None: rms(a) * w) -> out fp32, out_lo (type dt) | None, rstd [M].
    gate (fp32 [B], M = B * rows per sample; stochastic depth, needs y): rms(a + gate * y) * w."""
    M, Cc = a.shape
    _chk_rows((M, Cc), y, f32=(a,), name="res_rmsnorm_fwd")
    _chk_vec(Cc, w, name="res_rmsnorm_fwd")
    out = torch.empty_like(a)
    out_lo = torch.empty((M, Cc), device=a.device, dtype=tdtype(dt)) if want_lo else None
    rstd = torch.empty((M,), device=a.device, dtype=torch.float32)
    if gate is not None and y is None:
        raise ValueError("res_rmsnorm_fwd: a gate needs the branch output y")
    T = _chk_gate(gate, M, a, "res_rmsnorm_fwd")
    call("nvit_res_rmsnorm_fwd", dt, a, y, dt_of(y) if y is not None else F32, w, eps, gate, T, out, out_lo, rstd, M, Cc,
         _s())
    return out, out_lo, rstd


def res_rmsnorm_bwd(dt: int, g: Tensor, a: Tensor, y: Optional[Tensor], w: Tensor, rstd: Tensor,
                    g_add: Optional[Tensor] = None, dz: Optional[Tensor] = None, want_lo: bool = False, *,
                    nblk: Optional[int] = None, gate: Optional[Tensor] = None):
    """Backward of res_rmsnorm_fwd -> dz fp32 (added to `dz` when given), dz_lo (type dt) | None, part_dw [ROW_WAVES*nblk, C].
    g_add: optional type-dt [M,C] addend of the incoming gradient (a data-gradient GEMM's output).
    gate: as in res_rmsnorm_fwd (needs y and g_add); dz stays d(a + gate * y), dz_lo becomes gate * dz = d(y)."""
    M, Cc = a.shape
    _chk_rows((M, Cc), y, g_add, f32=(a, g, dz), name="res_rmsnorm_bwd")
    _chk_vec(Cc, w, name="res_rmsnorm_bwd")
    _chk_vec(M, rstd, name="res_rmsnorm_bwd")
    if g_add is not None and g_add.dtype != tdtype(dt):
        raise ValueError("res_rmsnorm_bwd: g_add must be a contiguous [M,C] tensor of the mode's operand type")
    accum = dz is not None
    if dz is None:
        dz = torch.empty_like(a)
    nblk = _part_blocks(nblk, _row_part_blocks(M), "res_rmsnorm_bwd")
    dz_lo = torch.empty((M, Cc), device=a.device, dtype=tdtype(dt)) if want_lo else None
    part = torch.empty((ROW_WAVES * nblk, Cc), device=a.device, dtype=torch.float32)
    if gate is not None and (y is None or g_add is None):
        raise ValueError("res_rmsnorm_bwd: the gated kernel needs the branch output y and the addend g_add")
    T = _chk_gate(gate, M, a, "res_rmsnorm_bwd")
    call("nvit_res_rmsnorm_bwd", dt, g, g_add, a, y, dt_of(y) if y is not None else F32, w, rstd, gate, T, dz, int(accum),
         dz_lo, part, nblk, M, Cc, _s())
    return dz, dz_lo, part


def res_skip_fwd(dt: int, h: Tensor, y: Tensor, skip: Tensor, x: Tensor, want_lo: bool = True, *,
                 gate: Optional[Tensor] = None):
    """out = nrm((h + y) * skip + x) -> out fp32, out_lo (type dt) | None.
    gate (fp32 [B], M = B * rows per sample; stochastic depth): nrm((h + gate * y) * skip + x)."""
    M, Cc = h.shape
    _chk_rows((M, Cc), y, f32=(h, x), name="res_skip_fwd")
    _chk_vec(1, skip, name="res_skip_fwd")
    out = torch.empty_like(h)
    out_lo = torch.empty((M, Cc), device=h.device, dtype=tdtype(dt)) if want_lo else None
    T = _chk_gate(gate, M, h, "res_skip_fwd")
    call("nvit_res_skip_fwd", dt, h, y, dt_of(y), skip, x, gate, T, out, out_lo, M, Cc, _s())
    return out, out_lo


def res_skip_bwd(dt: int, dout: Tensor, h: Tensor, y: Tensor, skip: Tensor, x: Tensor, want_lo: bool = True, *,
                 nblk: Optional[int] = None, gate: Optional[Tensor] = None):
    """Backward of res_skip_fwd -> dh = d(h + y) fp32, dh_lo (type dt) | None, dx fp32, part_dskip [ROW_WAVES*nblk].
    gate: as in res_skip_fwd; dh stays d(h + gate * y), dh_lo becomes gate * dh = d(y)."""
    M, Cc = h.shape
    _chk_rows((M, Cc), y, f32=(dout, h, x), name="res_skip_bwd")
    _chk_vec(1, skip, name="res_skip_bwd")
    nblk = _part_blocks(nblk, _row_part_blocks(M), "res_skip_bwd")
    dh = torch.empty_like(h)
    dx = torch.empty_like(h)
    dh_lo = torch.empty((M, Cc), device=h.device, dtype=tdtype(dt)) if want_lo else None
    part = torch.empty((ROW_WAVES * nblk,), device=h.device, dtype=torch.float32)
    T = _chk_gate(gate, M, h, "res_skip_bwd")
    call("nvit_res_skip_bwd", dt, dout, h, y, dt_of(y), skip, x, gate, T, dh, dh_lo, dx, part, nblk, M, Cc, _s())
    return dh, dh_lo, dx, part


def norm_skip_fwd(src: Tensor, tgt: Optional[Tensor], skip: Tensor) -> Tensor:
    """nrm(src*skip + tgt); tgt None = justnorm(src*skip)."""
    M, Cc = src.shape
    out = torch.empty_like(src)
    call("nvit_norm_skip_fwd", src, tgt, skip, out, M, Cc, _s())
    return out


def norm_skip_bwd(dout: Tensor, src: Tensor, tgt: Optional[Tensor], skip: Tensor, *, nblk: Optional[int] = None):
    M, Cc = src.shape
    nblk = _part_blocks(nblk, _row_part_blocks(M), "norm_skip_bwd")
    dsrc = torch.empty_like(src)
    dtgt = torch.empty_like(src) if tgt is not None else None
    part = torch.empty((nblk,), device=src.device, dtype=torch.float32)
    call("nvit_norm_skip_bwd", dout, src, tgt, skip, dsrc, dtgt, part, nblk, M, Cc, _s())
    dskip = torch.empty_like(skip)
    colsum_reduce(part, dskip, False)
    return dsrc, dtgt, dskip


def _pad_out(out, shape, dtype, device, name: str) -> Tensor:
    """An `out=` buffer of the padded-head ops (tests hand in pre-filled ones), checked, or a fresh torch.empty."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}")
    return out


def _heads_split(name: str, dp: int, dt: int, q, ldq, k, ldk, v, ldv, sqk, c_q, B, T, H, d, out, mid=(), post=()):
    """nvit_<name>: the head split (+ q/k normalise when sqk is given) into head tensors [B,H,T,dp] (out: optional buffers,
    or None).  mid / post: what this entry point takes before B and behind d.  -> qh, kh, vh, rq, rk."""
    dev = q.device
    td = tdtype(BF16 if dt == _lib.BF16_F32IN else dt)   # BF16_F32IN: fp32 projection outputs in, bf16 head tensors out
    o = tuple(out) if out is not None else (None,) * 5
    qh, kh, vh = (_pad_out(o[i], (B, H, T, dp), td, dev, name) for i in range(3))
    rq, rk = (_pad_out(o[i], (B * T, H), torch.float32, dev, name) for i in (3, 4)) if sqk is not None else (None, None)
    call("nvit_" + name, dt, q, ldq, k, ldk, v, ldv, sqk, c_q, qh, kh, vh, rq, rk, *mid, B, T, H, d, *post, _s())
    return qh, kh, vh, rq, rk


def _heads_merge(name: str, dt: int, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, ldq, dk, ldk, dv, ldv, B, T, H, d, nblk,
                 out, post=()) -> Optional[Tensor]:
    """nvit_<name>: the backward of _heads_split into token-major dq/dk/dv (type dt) -> the d(sqk*c_q) partials
    [nblk, H*d] (out: optional buffer), or None for the head merge alone (sqk None).  post: what it takes behind d."""
    nblk = _part_blocks(nblk, _row_part_blocks(B * T), name)
    part = _pad_out(out, (nblk, H * d), torch.float32, dq.device, name) if sqk is not None else None
    call("nvit_" + name, dt, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, ldq, dk, ldk, dv, ldv, part, nblk, B, T, H, d,
         *post, _s())
    return part


def qknorm_fwd(dt: int, q: Tensor, ldq: int, k: Tensor, ldk: int, v: Tensor, ldv: int, sqk: Optional[Tensor], c_q: float,
               B: int, T: int, H: int, d: int):
    """sqk None: the head split alone (plain-ViT attention); rq, rk are then None."""
    return _heads_split("qknorm_fwd", d, dt, q, ldq, k, ldk, v, ldv, sqk, c_q, B, T, H, d, None)


def qknorm_bwd(dt: int, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q: float, dq: Tensor, ldq: int, dk: Tensor, ldk: int,
               dv: Tensor, ldv: int, B: int, T: int, H: int, d: int, *, nblk: Optional[int] = None) -> Optional[Tensor]:
    """sqk None: the head merge alone (backward of the plain split); returns None instead of the d(sqk) partials."""
    return _heads_merge("qknorm_bwd", dt, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, ldq, dk, ldk, dv, ldv, B, T, H, d,
                        nblk, None)


def heads_pad_fwd(dt: int, q: Tensor, ldq: int, k: Tensor, ldk: int, v: Tensor, ldv: int, sqk: Optional[Tensor],
                  c_q: float, B: int, T: int, H: int, d: int, *, out=None):
    """qknorm_fwd from fp32 projections (dt F32 or BF16_F32IN) into zero-padded head tensors [B,H,T,PAD_HEAD_DIM]: every
    pad column is stored as zero on every call.  -> qh, kh, vh, rq, rk, sqk_pad ([H*PAD_HEAD_DIM], sqk with zero pads);
    sqk None: the split alone, rq = rk = sqk_pad = None.  out: optional (qh, kh, vh, rq, rk, sqk_pad) buffers."""
    _chk_dev(q, k, v, sqk)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32:
        raise TypeError("heads_pad_fwd: the projections are fp32")
    dp = PAD_HEAD_DIM
    o = tuple(out) if out is not None else (None,) * 6
    sqk_pad = _pad_out(o[5], (H * dp,), torch.float32, q.device, "heads_pad_fwd") if sqk is not None else None
    return (*_heads_split("heads_pad_fwd", dp, dt, q, ldq, k, ldk, v, ldv, sqk, c_q, B, T, H, d, o, (sqk_pad,), (dp,)),
            sqk_pad)


def heads_pad_bwd(dt: int, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q: float, dq: Tensor, ldq: int, dk: Tensor, ldk: int,
                  dv: Tensor, ldv: int, B: int, T: int, H: int, d: int, *, nblk: Optional[int] = None,
                  out: Optional[Tensor] = None) -> Optional[Tensor]:
    """qknorm_bwd from the first d columns of zero-padded dqh, dkh, dvh [B,H,T,PAD_HEAD_DIM] into token-major dq/dk/dv
    (type dt) -> the d(sqk*c_q) partials [nblk, H*d] in compact channel order (out: optional buffer for them); sqk None:
    the head merge alone, returns None."""
    _chk_dev(dqh, dkh, dvh, dq, dk, dv)
    return _heads_merge("heads_pad_bwd", dt, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, ldq, dk, ldk, dv, ldv, B, T, H, d,
                        nblk, out, (PAD_HEAD_DIM,))


def pad_cols(src: Tensor, M: int, H: int, d: int, *, out: Optional[Tensor] = None) -> Tensor:
    """[M, H*d] -> [M, H*PAD_HEAD_DIM] with zero pads (dO, and O rebuilt for the attention backward)."""
    _chk_dev(src)
    if tuple(src.shape) != (M, H * d) or not src.is_contiguous():
        raise ValueError(f"pad_cols: src must be a contiguous [{M}, {H * d}] tensor, got {tuple(src.shape)}")
    dst = _pad_out(out, (M, H * PAD_HEAD_DIM), src.dtype, src.device, "pad_cols")
    call("nvit_pad_cols", dt_of(src), src, dst, M, H, d, PAD_HEAD_DIM, _s())
    return dst


def unpad_cols(src: Tensor, M: int, H: int, d: int, *, out: Optional[Tensor] = None) -> Tensor:
    """[M, H*PAD_HEAD_DIM] -> [M, H*d]: the first d columns of every head (O for the output projection)."""
    _chk_dev(src)
    if tuple(src.shape) != (M, H * PAD_HEAD_DIM) or not src.is_contiguous():
        raise ValueError(f"unpad_cols: src must be a contiguous [{M}, {H * PAD_HEAD_DIM}] tensor, got {tuple(src.shape)}")
    dst = _pad_out(out, (M, H * d), src.dtype, src.device, "unpad_cols")
    call("nvit_unpad_cols", dt_of(src), src, dst, M, H, d, PAD_HEAD_DIM, _s())
    return dst


def swiglu_fwd(dt: int, uv: Tensor, suv: Optional[Tensor], gscale: float, M: int, F: int) -> Tensor:
    """dt = BF16_F32IN: fp32 pre-activations in, bf16 gated output."""
    x = torch.empty((M, F), device=uv.device, dtype=tdtype(BF16 if dt == _lib.BF16_F32IN else dt))
    call("nvit_swiglu_fwd", dt, uv, suv, gscale, x, M, F, _s())
    return x


def swiglu_bwd(dt: int, dx: Tensor, uv: Tensor, suv: Optional[Tensor], gscale: float, M: int, F: int):
    duv = torch.empty((M, 2 * F), device=uv.device, dtype=tdtype(dt))
    colblocks = math.ceil(F / 1024)
    rowblocks = max(1, min(M, math.ceil(2048 / colblocks)))
    rpb = math.ceil(M / rowblocks)
    nrb = math.ceil(M / rpb)
    part = torch.empty((nrb, 2 * F), device=uv.device, dtype=torch.float32) if suv is not None else None
    call("nvit_swiglu_bwd", dt, dx, uv, suv, gscale, duv, part, rpb, M, F, _s())
    return duv, part


def colsum_reduce(part: Tensor, out: Tensor, accumulate: bool, kind: int = 0, ref: Optional[Tensor] = None,
                  scale: float = 1.0) -> None:
    nblk, N = part.shape if part.dim() == 2 else (part.shape[0], 1)
    call("nvit_colsum_reduce", part, nblk, N, out, int(accumulate), kind, ref, scale, _s())


class ReduceBatch:
    """Column-partial reductions collected during one backward node and issued as ONE launch (`flush`): items are
    (part [rows, N], out [N], accumulate, kind, ref, scale) as for `colsum_reduce`, optionally with a second partial
    array that is reduced, scaled and added after the first (`part_b`)."""

    def __init__(self) -> None:
        self.items = []

    def add(self, part: Tensor, out: Tensor, accumulate: bool = False, kind: int = 0, ref: Optional[Tensor] = None,
            scale: float = 1.0, part_b: Optional[Tensor] = None) -> None:
        self.items.append((part, out, accumulate, kind, ref, scale, part_b))
        if len(self.items) == REDUCE_MAX_ITEMS:
            self.flush()

    def flush(self) -> None:
        items, self.items = self.items, []
        n = len(items)
        if n == 0:
            return
        if n == 1 and items[0][6] is None:
            part, out, acc, kind, ref, scale, _ = items[0]
            colsum_reduce(part, out, acc, kind, ref, scale)
            return
        I64, I32, F32_ = C.c_int64 * n, C.c_int * n, C.c_float * n
        rows = lambda t: t.shape[0]
        cols = lambda t: t.shape[1] if t.dim() == 2 else 1
        call("nvit_colsum_reduce_multi", I64(*[it[0].data_ptr() for it in items]), I32(*[rows(it[0]) for it in items]),
             I64(*[(it[6].data_ptr() if it[6] is not None else 0) for it in items]),
             I32(*[(rows(it[6]) if it[6] is not None else 0) for it in items]), I32(*[cols(it[0]) for it in items]),
             I64(*[it[1].data_ptr() for it in items]), I32(*[int(it[2]) for it in items]), I32(*[it[3] for it in items]),
             I64(*[(it[4].data_ptr() if it[4] is not None else 0) for it in items]), F32_(*[float(it[5]) for it in items]),
             n, _s())


def colsum(a: Tensor, R: int, N: int, out: Tensor, accumulate: bool, b: Optional[Tensor] = None, period: int = 0,
           scale: float = 1.0, lda: Optional[int] = None, ldb: Optional[int] = None) -> None:
    lda = a.stride(0) if lda is None else lda
    ldb = (b.stride(0) if ldb is None else ldb) if b is not None else 0
    call("nvit_colsum", a, dt_of(a), lda, b, dt_of(b) if b is not None else F32, ldb, R, N, period, out, int(accumulate),
         scale, _s())


def colsum_big(a: Tensor, R: int, N: int, out: Tensor, accumulate: bool, lda: Optional[int] = None) -> None:
    """column sums over many rows: fold rows modulo 512 first, then reduce the 512 partial rows."""
    if R <= 1024:
        colsum(a, R, N, out, accumulate, lda=lda)
        return
    part = torch.empty((512, N), device=a.device, dtype=torch.float32)
    colsum(a, R, N, part, False, period=512, lda=lda)
    colsum(part, 512, N, out, accumulate)


def cast(src: Tensor, dt: int) -> Tensor:
    dst = torch.empty(src.shape, device=src.device, dtype=tdtype(dt))
    call("nvit_cast", src, dst, dt, src.numel(), _s())
    return dst


def _chk_token_rows(name: str, table: Tensor, what: str, B: int, n: int, rows: int, s0: Tensor, s1: Optional[Tensor]):
    """Operands of rows_gather / rows_scatter: fp32 [B*rows, C] row tensors, C a multiple of 4, and the int32 [B, n] index
    table on their device.  -> C."""
    if isinstance(B, bool) or not isinstance(B, int) or B < 1:
        raise ValueError(f"{name}: B must be an int >= 1 (got {B!r})")
    if not isinstance(s0, Tensor) or s0.dim() != 2 or s0.shape[1] % 4:
        raise ValueError(f"{name}: [rows, C] operands with C a multiple of 4 expected")
    _chk_rows((B * rows, s0.shape[1]), f32=(s0, s1), name=name)
    if s1 is not None and (s1.dim() != 2 or s1.device != s0.device):
        raise ValueError(f"{name}: the second stream must be a [rows, C] tensor on {s0.device}")
    if (not isinstance(table, Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (B, n)
            or not table.is_contiguous() or table.device != s0.device):
        raise ValueError(f"{name}: {what} must be a contiguous int32 [{B}, {n}] tensor on {s0.device}")
    return s0.shape[1]


def rows_gather(src0: Tensor, src1: Optional[Tensor], keep: Tensor, B: int, T: int, lo_dt: Optional[int] = None):
    """Token gather of patch dropout (nvit_rows_gather): src fp32 [B*T, C], keep int32 [B, K] -> dst fp32 [B*K, C] with
    dst[b*K + j] = src[b*T + keep[b, j]]; src1 None: one stream.  lo_dt BF16: also the bf16 twins of the gathered rows
    (the bits of ops.cast).  -> (dst0, dst1, lo0, lo1), None where absent.  keep's values are the caller's: an index
    outside [0, T) gathers a row of zeros."""
    if not isinstance(keep, Tensor) or keep.dim() != 2:
        raise ValueError("rows_gather: keep must be an int32 [B, K] tensor")
    K = keep.shape[1]
    if isinstance(T, bool) or not isinstance(T, int) or not 1 <= K <= T:
        raise ValueError(f"rows_gather: 1 <= K <= T expected (K={K}, T={T!r})")
    if lo_dt not in (None, BF16):
        raise ValueError("rows_gather: the twins are bf16 (lo_dt None or BF16)")
    Cc = _chk_token_rows("rows_gather", keep, "keep", B, K, T, src0, src1)
    dev = src0.device
    dst0 = torch.empty((B * K, Cc), device=dev, dtype=torch.float32)
    dst1 = torch.empty_like(dst0) if src1 is not None else None
    lo0 = torch.empty((B * K, Cc), device=dev, dtype=torch.bfloat16) if lo_dt is not None else None
    lo1 = torch.empty_like(lo0) if lo_dt is not None and src1 is not None else None
    call("nvit_rows_gather", src0, src1, keep, dst0, dst1, lo0, lo1, BF16 if lo_dt is not None else 0, B, T, K, Cc, _s())
    return dst0, dst1, lo0, lo1


def rows_scatter(d0: Tensor, d1: Optional[Tensor], slot: Tensor, B: int, K: int):
    """Backward of rows_gather (nvit_rows_scatter): d fp32 [B*K, C], slot int32 [B, T] -> g fp32 [B*T, C] with g[b*T + t] =
    d[b*K + slot[b, t]] where 0 <= slot[b, t] < K, else zeros; every element of g is written by the one launch.
    -> (g0, g1), g1 None without d1."""
    if not isinstance(slot, Tensor) or slot.dim() != 2:
        raise ValueError("rows_scatter: slot must be an int32 [B, T] tensor")
    T = slot.shape[1]
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= T:
        raise ValueError(f"rows_scatter: 1 <= K <= T expected (K={K!r}, T={T})")
    Cc = _chk_token_rows("rows_scatter", slot, "slot", B, T, K, d0, d1)
    g0 = torch.empty((B * T, Cc), device=d0.device, dtype=torch.float32)
    g1 = torch.empty_like(g0) if d1 is not None else None
    call("nvit_rows_scatter", d0, d1, slot, g0, g1, B, T, K, Cc, _s())
    return g0, g1


def _pos_resample(name: str, s0: Tensor, s1: Optional[Tensor], n_src: int, n_dst: int, g: int, g2: int, table: Tensor):
    """Operands of pos_resample_fwd / bwd: fp32 [n_src^2, C] tables, C a multiple of 4 up to MAX_EMBD, and the packed tap
    table int32 [n_dst, 2 + MAX_TAPS] on their device.  One launch for both tables."""
    if not isinstance(s0, Tensor) or s0.dim() != 2 or s0.shape[1] % 4 or not 0 < s0.shape[1] <= _lib.MAX_EMBD:
        raise ValueError(f"{name}: [rows, C] operands with C a multiple of 4, at most {_lib.MAX_EMBD}, expected")
    _chk_rows((n_src * n_src, s0.shape[1]), f32=(s0, s1), name=name)
    if s1 is not None and (s1.dim() != 2 or s1.device != s0.device):
        raise ValueError(f"{name}: the second table must be a [rows, C] tensor on {s0.device}")
    if (not isinstance(table, Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (n_dst, resample.ROW)
            or not table.is_contiguous() or table.device != s0.device):
        raise ValueError(f"{name}: the tap table must be a contiguous int32 [{n_dst}, {resample.ROW}] tensor on {s0.device}")
    d0 = torch.empty((n_dst * n_dst, s0.shape[1]), device=s0.device, dtype=torch.float32)
    d1 = torch.empty_like(d0) if s1 is not None else None
    call("nvit_" + name, s0, s1, table, d0, d1, g, g2, s0.shape[1], _s())
    return d0, d1


def pos_resample_fwd(p0: Tensor, p1: Optional[Tensor], g: int, g2: int):
    """Position tables p fp32 [g*g, C] resampled to the grid g2 x g2 (nvit_pos_resample_fwd): what F.interpolate(...,
    mode="bicubic", align_corners=False, antialias=True) computes on the [C, g, g] image, in fp32.  p1 None: one table,
    else both in one launch.  -> (out0, out1) fp32 [g2*g2, C], out1 None without p1.  Equal grids launch nothing and
    return the operands themselves.  ValueError for a grid ratio beyond the kernels' taps per row (resample.MAX_TAPS).
    The first call for (g, g2) on a device sends the tap tables: not under graph capture."""
    _chk_dev(p0)
    resample.check_grids(g, g2)
    if g == g2:
        _chk_rows((g * g, p0.shape[1]), f32=(p0, p1), name="pos_resample_fwd")
        return p0, p1
    taps, _ = resample.tap_tables(g, g2, p0.device)
    return _pos_resample("pos_resample_fwd", p0, p1, g, g2, g, g2, taps)


def pos_resample_bwd(d0: Tensor, d1: Optional[Tensor], g: int, g2: int):
    """The exact adjoint of pos_resample_fwd (nvit_pos_resample_bwd): d fp32 [g2*g2, C] -> gradients fp32 [g*g, C], every
    element written once in a fixed order.  Equal grids return the operands themselves."""
    _chk_dev(d0)
    resample.check_grids(g, g2)
    if g == g2:
        _chk_rows((g * g, d0.shape[1]), f32=(d0, d1), name="pos_resample_bwd")
        return d0, d1
    _, taps_t = resample.tap_tables(g, g2, d0.device)
    return _pos_resample("pos_resample_bwd", d0, d1, g2, g, g, g2, taps_t)


def normalize_images(x: Tensor, mean: float = 0.5, std: float = 0.5) -> Tensor:
    """ToTensor + Normalize(mean, std) on the device (reference train.py:1084-1090, the deterministic part of its input
    pipeline): uint8 [B,H,W,C] (scaled by 1/255) or fp32 [B,C,H,W] in [0,1] -> fp32 [B,C,H,W]."""
    _chk_dev(x)
    x = x.contiguous()
    if x.dtype == torch.uint8:
        B, H, W, Cc = x.shape
        u8 = 1
    elif x.dtype == torch.float32:
        B, Cc, H, W = x.shape
        u8 = 0
    else:
        raise TypeError("normalize_images: uint8 [B,H,W,C] or float32 [B,C,H,W]")
    out = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32)
    call("nvit_normalize_images", x, u8, out, B, Cc, H, W, mean, std, _s())
    return out


def scale_cols(a: Tensor, s: Tensor, c: float, R: int, N: int, out: Tensor, lda: Optional[int] = None,
               ldo: Optional[int] = None) -> Tensor:
    lda = a.stride(0) if lda is None else lda
    ldo = out.stride(0) if ldo is None else ldo
    call("nvit_scale_cols", a, lda, s, c, out, dt_of(out), ldo, R, N, _s())
    return out


def eval_metrics(logits: Tensor, y: Tensor, acc: Tensor) -> None:
    """acc[0..3] (fp32, device) += batch-mean cross-entropy, top-1 %, top-min(5,N) %, 1 - one launch, nothing read back."""
    _chk_dev(logits, y, acc)
    if logits.dtype != torch.float32 or y.dtype != torch.int64 or acc.dtype != torch.float32 or acc.numel() < 4:
        raise RuntimeError("eval_metrics: fp32 logits [B,N], int64 labels [B] and an fp32 accumulator of 4 values")
    logits, y = logits.contiguous(), y.contiguous()
    B, N = logits.shape
    if y.numel() != B or not acc.is_contiguous():
        raise RuntimeError("eval_metrics: one label per row and a contiguous accumulator")
    call("nvit_eval_metrics", logits, y, acc, B, N, _s())


# ----------------------------------------------------------------------------- attention
def attn_fwd(dt: int, impl: int, qh: Tensor, kh: Tensor, vh: Tensor, scale: float, sqk: Optional[Tensor] = None,
             c_q: float = 0.0, q_prescale: float = 1.0):
    """sqk/c_q given: q and k are (sqk*c_q) * unit vectors per head (the nViT call sites) -> bounded-score kernel path;
    q_prescale: qh holds q_prescale * q_hat (without sqk: the running-maximum kernel on a pre-scaled q)."""
    B, H, Tq, d = qh.shape
    Tk = kh.shape[2]
    o = torch.empty((B * Tq, H * d), device=qh.device, dtype=tdtype(dt))
    lse = torch.empty((B, H, Tq), device=qh.device, dtype=torch.float32)
    if sqk is not None or q_prescale != 1.0:
        call("nvit_attn_fwd_bounded", dt, impl, qh, kh, vh, scale, sqk, c_q, q_prescale, o, lse, B, H, Tq, Tk, d, _s())
    else:
        call("nvit_attn_fwd", dt, impl, qh, kh, vh, scale, o, lse, B, H, Tq, Tk, d, _s())
    return o, lse


def attn_bwd(dt: int, impl: int, dout: Tensor, qh: Tensor, kh: Tensor, vh: Tensor, o: Tensor, lse: Tensor,
             scale: float):
    B, H, Tq, d = qh.shape
    Tk = kh.shape[2]
    dqh = torch.empty_like(qh)
    dkh = torch.empty_like(kh)
    dvh = torch.empty_like(vh)
    delta = torch.empty((2, B, H, Tq), device=qh.device, dtype=torch.float32)   # workspace: -delta | -lse*log2(e)
    call("nvit_attn_bwd", dt, impl, dout, qh, kh, vh, o, lse, scale, dqh, dkh, dvh, delta, B, H, Tq, Tk, d, _s())
    return dqh, dkh, dvh


def attn_bwd_qknorm(dout: Tensor, qh: Tensor, kh: Tensor, vh: Tensor, o: Tensor, lse: Tensor, scale: float,
                    rq: Tensor, rk: Tensor, sqk: Tensor, c_q: float, dq: Tensor, ldq: int, dk: Tensor, dv: Tensor,
                    ldkv: int, q_prescale: float = 1.0):
    """MFMA attention backward + q/k-normalise backward in one pass (bf16, d=64).
    Writes dq/dk/dv token-major; returns the partial sums (part_q, part_k) of d/d(sqk*c_q).
    sqk None (plain-ViT heads; rq, rk None): dq/dk/dv stored as they are, returns (None, None)."""
    B, H, Tq, d = qh.shape
    Tk = kh.shape[2]
    dev = qh.device
    if sqk is None:
        part_q = part_k = None
    else:
        part_q = torch.empty((B * math.ceil(Tq / ATTN_BWD_PART_ROWS), H * d), device=dev, dtype=torch.float32)
        part_k = torch.empty((B * math.ceil(Tk / ATTN_BWD_PART_ROWS), H * d), device=dev, dtype=torch.float32)
    delta = torch.empty((2, B, H, Tq), device=dev, dtype=torch.float32)   # workspace: -delta | -lse*log2(e)
    call("nvit_attn_bwd_qknorm", BF16, dout, qh, kh, vh, o, lse, scale, rq, rk, sqk, c_q, q_prescale, dq, ldq, dk, dv, ldkv,
         part_q, part_k, delta, B, H, Tq, Tk, d, _s())
    return part_q, part_k


def attn_heads_fwd(dt: int, q: Tensor, ldq: int, k: Tensor, v: Tensor, ldkv: int, sqk: Optional[Tensor], c_q: float,
                   scale: float, M: int, H: int, d: int):
    """Head-axis attention of the reference's flash_attn=True branch (softmax over the H heads of each token) from the
    fp32 token-major projection outputs.  sqk None: plain heads.  -> O [M, C] (type dt), lse [M, H] fp32."""
    _chk_dev(q, k, v)
    o = torch.empty((M, H * d), device=q.device, dtype=tdtype(dt))
    lse = torch.empty((M, H), device=q.device, dtype=torch.float32)
    call("nvit_attn_heads_fwd", dt, q, ldq, k, v, ldkv, sqk, c_q, scale, o, lse, M, H, d, _s())
    return o, lse


ATTN_HEADS_BWD_BLOCKS = 4096   # one-wave workgroups of the head-axis backward (rows of its d(sqk) partials)
assert ATTN_HEADS_BWD_BLOCKS <= _lib.const("ATTN_HEADS_BWD_MAX_BLOCKS")


def attn_heads_bwd(dt: int, dout: Tensor, q: Tensor, ldq: int, k: Tensor, v: Tensor, ldkv: int, sqk: Optional[Tensor],
                   c_q: float, scale: float, lse: Tensor, dq: Tensor, lddq: int, dk: Tensor, dv: Tensor, lddkv: int,
                   M: int, H: int, d: int) -> Optional[Tensor]:
    """Backward of attn_heads_fwd into token-major dq / dk / dv (type dt).  Returns the [nblk, C] partial sums of
    d/d(sqk*c_q) (None without sqk)."""
    _chk_dev(dout, q, k, v, lse, dq, dk, dv)
    nblk = max(1, min(ATTN_HEADS_BWD_BLOCKS, M))
    part = torch.empty((nblk, H * d), device=q.device, dtype=torch.float32) if sqk is not None else None
    call("nvit_attn_heads_bwd", dt, dout, q, ldq, k, v, ldkv, sqk, c_q, scale, lse, dq, lddq, dk, dv, lddkv, part, nblk, M,
         H, d, _s())
    return part


# ----------------------------------------------------------------------------- embed / head
def im2col(dt: int, img: Tensor, Pl: int, Pg: int):
    B, ch, S, _ = img.shape
    T = (S // Pl) ** 2
    td = tdtype(dt)
    A_l = torch.empty((B * T, ch * Pl * Pl), device=img.device, dtype=td)
    A_g = torch.empty((B * T, ch * Pg * Pg), device=img.device, dtype=td)
    call("nvit_im2col", dt, img, A_l, A_g, B, ch, S, Pl, Pg, _s())
    return A_l, A_g


def patch_kp(K: int) -> int:
    """patch length padded to whole stages of nvit_patch_embed_fwd (what nvit_patch_embed_kp returns)"""
    return round_up(K, PATCH_K_STEP)


def patch_embed_fwd(img: Tensor, w_l: Tensor, b_l: Optional[Tensor], pos_l: Tensor, w_g: Tensor, b_g: Optional[Tensor],
                    pos_g: Tensor, Pl: int, Pg: int, Cc: int, save_rows: bool = True, twins: bool = False):
    """Fused dual patch embedding of the bf16 mode -> loc, glo fp32 [M, C], (twins) their bf16 copies, and (save_rows)
    the bf16 patch rows a_l [Mpad, Kp_l], a_g [Mpad, Kp_g] for the weight gradients.
    w_l / w_g: split images [C, 2*Kp] (shadow perm 2).  Returns (loc, glo, a_l, a_g, loc_lo, glo_lo)."""
    B, ch, S, _ = img.shape
    T = (S // Pl) ** 2
    M = B * T
    Kpl, Kpg = patch_kp(ch * Pl * Pl), patch_kp(ch * Pg * Pg)
    assert w_l.shape == (Cc, 2 * Kpl) and w_g.shape == (Cc, 2 * Kpg) and w_l.dtype == torch.bfloat16
    assert pos_l.shape == (T, Cc) and pos_g.shape == (T, Cc) and img.dtype == torch.float32 and img.is_contiguous()
    _chk_dev(img, w_l, w_g, pos_l, pos_g)
    dev = img.device
    loc = torch.empty((M, Cc), device=dev, dtype=torch.float32)
    glo = torch.empty((M, Cc), device=dev, dtype=torch.float32)
    a_l = a_g = lo_l = lo_g = None
    if save_rows:
        Mpad = round_up(M, PATCH_TILE_ROWS)
        a_l = torch.empty((Mpad, Kpl), device=dev, dtype=torch.bfloat16)
        a_g = torch.empty((Mpad, Kpg), device=dev, dtype=torch.bfloat16)
    if twins:
        lo_l = torch.empty((M, Cc), device=dev, dtype=torch.bfloat16)
        lo_g = torch.empty((M, Cc), device=dev, dtype=torch.bfloat16)
    call("nvit_patch_embed_fwd", img, w_l, b_l, pos_l, loc, lo_l, a_l, w_g, b_g, pos_g, glo, lo_g, a_g, B, ch, S, Pl, Pg, Cc,
         _s())
    return loc, glo, a_l, a_g, lo_l, lo_g


def pool_ln_fwd(dt: int, x: Tensor, w: Tensor, b: Tensor, eps: float, B: int, T: int, Cc: int):
    dev = x.device
    nchunk = max(1, min(T, math.ceil(1024 / B)))
    pooled = torch.empty((B, Cc), device=dev, dtype=torch.float32)
    ln = torch.empty_like(pooled)
    ln_lo = torch.empty((B, Cc), device=dev, dtype=tdtype(dt))
    stats = torch.empty((B, 2), device=dev, dtype=torch.float32)
    ws = torch.empty((B, nchunk, Cc), device=dev, dtype=torch.float32)
    call("nvit_pool_ln_fwd", dt, x, w, b, eps, pooled, ln, ln_lo, stats, ws, nchunk, B, T, Cc, _s())
    return pooled, ln, ln_lo, stats


def pool_ln_bwd(dln: Tensor, pooled: Tensor, w: Tensor, stats: Tensor, dw: Tensor, db: Tensor, accumulate: bool,
                B: int, T: int, Cc: int) -> Tensor:
    dx = torch.empty((B * T, Cc), device=dln.device, dtype=torch.float32)
    call("nvit_pool_ln_bwd", dln, pooled, w, stats, dx, dw, db, int(accumulate), B, T, Cc, _s())
    return dx


def recon_loss(raw: Tensor, img: Tensor, P: int) -> Tensor:
    B, ch, S, _ = img.shape
    nblk = PART_BLOCKS
    part = torch.empty((nblk,), device=img.device, dtype=torch.float32)
    loss = torch.empty((1,), device=img.device, dtype=torch.float32)
    call("nvit_recon_loss", raw, img, part, nblk, loss, B, ch, S, P, _s())
    return loss.reshape(())


# ----------------------------------------------------------------------------- Kohonen head (config C5)
def som_bmu(x: Tensor, nodes: Tensor) -> Tensor:
    """x [M,C] fp32, nodes [N,C] fp32 -> idx [M] int64 (exact-f32 MFMA score GEMM + argmin kernel)."""
    M, Cc = x.shape
    N = nodes.shape[0]
    Kp = round_up(Cc, bk_of(F32))
    xs, ns = x, nodes
    if Kp != Cc:   # the GEMM takes K in whole LDS rows of 32 floats: zero columns add nothing to x . node
        xs = torch.nn.functional.pad(x, (0, Kp - Cc))
        ns = torch.nn.functional.pad(nodes, (0, Kp - Cc))
    scores = gemm_nt(xs, ns, M, N, Kp)                        # fp32 operands -> v_mfma_f32_16x16x4_f32
    nn_ws = torch.empty((N,), device=x.device, dtype=torch.float32)
    idx = torch.empty((M,), device=x.device, dtype=torch.int64)
    call("nvit_som_bmu", scores, nodes, nn_ws, M, N, Cc, idx, _s())
    return idx


def gather_rows(nodes: Tensor, idx: Tensor) -> Tensor:
    M, Cc = idx.numel(), nodes.shape[1]
    out = torch.empty((M, Cc), device=nodes.device, dtype=torch.float32)
    call("nvit_gather_rows", nodes, idx, out, M, Cc, _s())
    return out


def onehot(idx: Tensor, N: int) -> Tensor:
    """fp32 [M, N] rows with a single 1 at idx[m] (N a multiple of 4)."""
    M = idx.numel()
    oh = torch.empty((M, N), device=idx.device, dtype=torch.float32)
    call("nvit_onehot", idx, oh, M, N, _s())
    return oh


def scatter_rows(dout: Tensor, idx: Tensor, N: int) -> Tensor:
    """dnodes[n] = sum of dout rows with idx == n.  All tokens may pick the same node (they do at init: the BMU of a
    small-norm patch is the smallest-norm node), so instead of a per-node loop this is onehot(idx)^T . dout on the
    exact-f32 weight-gradient GEMM: load balanced and deterministic whatever the histogram."""
    M, Cc = dout.shape
    dn = torch.empty((N, Cc), device=dout.device, dtype=torch.float32)
    if N % 4 != 0 or Cc % 4 != 0:
        call("nvit_scatter_rows", dout, idx, dn, M, N, Cc, _s())
        return dn
    return gemm_tn(onehot(idx, N), dout.float().contiguous(), dn, M, N, Cc)


def som_update(nodes: Tensor, x: Tensor, idx: Tensor, lr_alpha, sigma: float, gm: int, gn: int, B: int,
               T: int, periodic: bool = True) -> None:
    """KohonenMap.update_nodes for the whole batch, in place on nodes.  lr_alpha (learning rate x the map's alpha): a
    Python float, passed by value (nvit_som_update), or a 1-element fp32 tensor on the nodes' device that the kernel reads
    when it runs (nvit_som_update_dev: a captured step whose host rewrites the rate between replays).  Equal values
    give equal bits."""
    dev_rate = isinstance(lr_alpha, Tensor)
    if dev_rate and (lr_alpha.dtype != torch.float32 or lr_alpha.numel() != 1 or not lr_alpha.is_cuda
                     or lr_alpha.device != nodes.device):
        raise ValueError(f"som_update: a tensor lr_alpha must be one fp32 element on the nodes' device ({nodes.device}), "
                         f"got {lr_alpha.dtype} {tuple(lr_alpha.shape)} on {lr_alpha.device}")
    Cc = nodes.shape[1]
    v_ws = torch.empty((B, Cc), device=nodes.device, dtype=torch.float32)
    s_ws = torch.empty((B, gm * gn), device=nodes.device, dtype=torch.float32)
    if dev_rate:
        call("nvit_som_update_dev", nodes, x, idx, lr_alpha, sigma, gm, gn, int(periodic), v_ws, s_ws, B, T, Cc, _s())
        return
    call("nvit_som_update", nodes, x, idx, lr_alpha, sigma, gm, gn, int(periodic), v_ws, s_ws, B, T, Cc, _s())


def cos_consistency_fwd(a: Tensor, b: Tensor):
    M, Cc = a.shape
    nblk = min(PART_BLOCKS, math.ceil(M / 4))
    stats = torch.empty((M, 3), device=a.device, dtype=torch.float32)
    part = torch.empty((nblk,), device=a.device, dtype=torch.float32)
    loss = torch.empty((1,), device=a.device, dtype=torch.float32)
    call("nvit_cos_consistency_fwd", a, b, stats, part, nblk, loss, M, Cc, _s())
    return loss.reshape(()), stats


def cos_consistency_bwd(a: Tensor, b: Tensor, stats: Tensor, g: Tensor):
    M, Cc = a.shape
    da, db = torch.empty_like(a), torch.empty_like(b)
    call("nvit_cos_consistency_bwd", a, b, stats, g, da, db, M, Cc, _s())
    return da, db


def huber_fwd(a: Tensor, b: Tensor) -> Tensor:
    nblk = PART_BLOCKS
    part = torch.empty((nblk,), device=a.device, dtype=torch.float32)
    loss = torch.empty((1,), device=a.device, dtype=torch.float32)
    call("nvit_huber_fwd", a, b, part, nblk, loss, a.numel(), _s())
    return loss.reshape(())


def huber_bwd(a: Tensor, b: Tensor, g: Tensor):
    da, db = torch.empty_like(a), torch.empty_like(b)
    call("nvit_huber_bwd", a, b, g, da, db, a.numel(), _s())
    return da, db


def som_smooth_fwd(nodes: Tensor, idx: Tensor, map_size: int):
    Nn, Cc = nodes.shape
    cnt = torch.empty((Nn,), device=nodes.device, dtype=torch.int32)
    D = torch.empty((Nn, 8), device=nodes.device, dtype=torch.float32)
    loss = torch.empty((1,), device=nodes.device, dtype=torch.float32)
    call("nvit_som_smooth_fwd", nodes, idx, cnt, D, loss, idx.numel(), Nn, Cc, map_size, _s())
    return loss.reshape(()), cnt, D


def som_smooth_bwd(nodes: Tensor, D: Tensor, cnt: Tensor, g: Tensor, M: int, map_size: int) -> Tensor:
    Nn, Cc = nodes.shape
    dn = torch.empty_like(nodes)
    call("nvit_som_smooth_bwd", nodes, D, cnt, g, dn, 0, M, Nn, Cc, map_size, _s())
    return dn


def recon_bwd(dt: int, raw: Tensor, img: Tensor, g: Tensor, P: int) -> Tensor:
    B, ch, S, _ = img.shape
    draw = torch.empty(raw.shape, device=raw.device, dtype=tdtype(dt))
    call("nvit_recon_bwd", dt, raw, img, g, draw, B, ch, S, P, _s())
    return draw


# ----------------------------------------------------------------------------- weights
def renorm_table(mats, device) -> Tuple[Tensor, int]:
    """mats: list of (tensor fp32 [rows, cols] contiguous, dim). -> device table, total_items"""
    rows_, first = [], 0
    for w, dim in mats:
        assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2
        r, c = w.shape
        if dim == 0 and r > _lib.RENORM_MAX_ROWS_DIM0:
            raise RuntimeError(f"renorm: column-normalised matrix with {r} rows exceeds the register panel "
                               f"({_lib.RENORM_MAX_ROWS_DIM0})")
        if dim == 1:
            items = math.ceil(r / _lib.RENORM_ROWS_PER_ITEM)
        else:   # the panel width follows the kernel's choice by row count
            items = math.ceil(c / (_lib.RENORM_COLS_PER_ITEM if r <= _lib.RENORM_TALL_ROWS
                                   else _lib.RENORM_TALL_COLS_PER_ITEM))
        rows_.append([w.data_ptr(), r, c, dim, first])
        first += items
    return torch.tensor(rows_, dtype=torch.int64).to(device), first


def renorm_weights(table: Tensor, total_items: int) -> None:
    call("nvit_renorm_weights", table, table.shape[0], total_items, _s())


def lr_schedule(table: Optional[Tensor], n: int, lr_scale: Optional[Tensor], step: Tensor, kind: int, lr: float,
                min_lr: float, warmup_init: float, warmup_iters: int, decay_iters: int, last_lr: Tensor,
                last_lr64: Tensor) -> None:
    """One step of a learning-rate schedule (nvit_lr_schedule): L(step[0]) in fp64 -> last_lr / last_lr64, (float)(L *
    lr_scale[i]) into the lr half of the last column of table row i < n, step[0] += 1.  n == 0: no table is touched."""
    _chk_dev(table, lr_scale, step, last_lr, last_lr64)
    if step.dtype != torch.int64 or last_lr.dtype != torch.float32 or last_lr64.dtype != torch.float64:
        raise ValueError("lr_schedule: step int64[1], last_lr fp32[1], last_lr64 fp64[1]")
    if n:
        if table.dtype != torch.int64 or lr_scale.dtype != torch.float32 or not table.is_contiguous() \
                or not lr_scale.is_contiguous() or table.numel() < n * _lib.const("OPT_TABLE_COLS") or lr_scale.numel() < n:
            raise ValueError("lr_schedule: table must be contiguous int64 [n, cols] and lr_scale contiguous fp32 [n]")
        if table.device != step.device or lr_scale.device != step.device:
            raise RuntimeError("lr_schedule: the table lives on another device than the schedule")
    call("nvit_lr_schedule", table if n else None, n, lr_scale if n else None, step, kind, lr, min_lr, warmup_init,
         warmup_iters, decay_iters, last_lr, last_lr64, _s())


def shadow_table(entries, device) -> Tuple[Tensor, int]:
    """entries: list of (src fp32 2-D view, dst|None, dst_ld, dst_cols, dstT|None, dstT_ld, dstT_cols, perm)."""
    rows_, first = [], 0
    for src, dst, dst_ld, dst_cols, dstT, dstT_ld, dstT_cols, perm in entries:
        assert src.dtype == torch.float32 and src.is_contiguous()
        r, c = src.shape[0], src.numel() // src.shape[0]
        tiles_c = math.ceil(max(c, dst_cols if dst is not None else 0) / SHADOW_TILE)
        tiles_r = math.ceil(max(r, dstT_cols if dstT is not None else 0) / SHADOW_TILE)
        rows_.append([src.data_ptr(), r, c, dst.data_ptr() if dst is not None else 0, dst_ld, dst_cols,
                      dstT.data_ptr() if dstT is not None else 0, dstT_ld, dstT_cols, perm, first, tiles_c])
        first += tiles_c * tiles_r
    return torch.tensor(rows_, dtype=torch.int64).to(device), first


def shadow_weights(table: Tensor, total_items: int, dt: int) -> None:
    call("nvit_shadow_weights", table, table.shape[0], total_items, dt, _s())


# ----------------------------------------------------------------------------- weight EMA
EMA_TABLE_COLS = _lib.const("EMA_TABLE_COLS")
EMA_CHUNK = _lib.const("EMA_CHUNK")          # elements per work item of nvit_ema_update
EMA_MAX_GRID = _lib.const("EMA_MAX_GRID")    # its workgroups: a table of more chunks takes several sweeps
EMA_FLAG_COPY = _lib.const("EMA_FLAG_COPY")
EMA_FLAG_SCALAR = _lib.const("EMA_FLAG_SCALAR")


def ema_table(pairs, device) -> Tuple[Tensor, int]:
    """pairs: list of (src, dst) or (src, dst, copy) with src, dst contiguous fp32 device tensors of equal, non-zero
    numel -> (device table of nvit_ema_update, total_chunks).  copy=True flags a row that stores src unchanged.  A row
    of numel % 4 != 0, or with a pointer that is not 16-byte aligned, is flagged for the element-wise path here.
    ValueError when a dst range overlaps any other range of the table (its own src included); sources may repeat.
    The host image is pinned, so do not call this during a stream capture."""
    rows_, spans, first = [], [], 0
    for pair in pairs:
        src, dst = pair[0], pair[1]
        copy = bool(pair[2]) if len(pair) > 2 else False
        _chk_dev(src, dst)
        for t in (src, dst):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("ema_table: contiguous fp32 tensors expected")
        n = src.numel()
        if n == 0 or dst.numel() != n:
            raise ValueError(f"ema_table: src and dst need the same non-zero numel (got {n} and {dst.numel()})")
        sp, dp = src.data_ptr(), dst.data_ptr()
        flags = (EMA_FLAG_COPY if copy else 0) | (EMA_FLAG_SCALAR if (n % 4 or sp % 16 or dp % 16) else 0)
        rows_.append([sp, dp, n, first, flags])
        spans += [(sp, sp + 4 * n, False), (dp, dp + 4 * n, True)]
        first += math.ceil(n / EMA_CHUNK)
    if not rows_:
        raise ValueError("ema_table: no rows")
    if first >= 2 ** 31:
        raise ValueError("ema_table: too many chunks for one table")
    end_any = end_dst = 0   # sweep over the ranges by start address: a dst may meet nothing, a src no dst
    for lo, hi, is_dst in sorted(spans):
        if lo < (end_any if is_dst else end_dst):
            raise ValueError("ema_table: a destination overlaps another range of the table (src == dst included)")
        end_any = max(end_any, hi)
        if is_dst:
            end_dst = max(end_dst, hi)
    host = torch.tensor(rows_, dtype=torch.int64).pin_memory()
    return host.to(device, non_blocking=True), first


def ema_tick(state: Tensor, decay: float, warmup: bool, skip_state: Optional[Tensor] = None) -> None:
    """state (fp32 device [4]: updates applied, omd, spare, spare): omd = 1 - d for the update about to run, d =
    min(decay, (1 + t) / (10 + t)) with warmup and decay without, computed in fp64 on the device, and t += 1.  The count
    is a float, exact up to 2^24 updates (like the optimizer's hyper[0]).  With skip_state (the optimizer's) and
    skip_state[0] != 0 the count stays and omd = 0."""
    _chk_dev(state, skip_state)
    if state.dtype != torch.float32 or state.numel() < 4 or not state.is_contiguous():
        raise RuntimeError("ema_tick: state must be a contiguous fp32 tensor of 4 elements")
    call("nvit_ema_tick", state, float(decay), int(bool(warmup)), skip_state, _s())


def ema_update(table: Tensor, total_chunks: int, state: Optional[Tensor] = None) -> None:
    """dst = fma(omd, src - dst, dst) over the table's rows with omd = state[1] (nothing is touched when it is 0); copy
    rows store src.  state=None: only the copy rows run."""
    _chk_dev(table, state)
    call("nvit_ema_update", table, table.shape[0], total_chunks, state, _s())


# ----------------------------------------------------------------------------- profiling
def prof_enable(on: bool) -> None:
    _lib.load().nvit_prof_enable(int(on))


def prof_select(*families: str) -> None:
    """time only the launches of the named kernel families (names: _lib.KID_NAMES)"""
    mask = 0
    for f in families:
        mask |= 1 << _lib.KID_NAMES.index(f)
    _lib.load().nvit_prof_select(mask)


def prof_collect():
    n = len(_lib.KID_NAMES)
    ms = (C.c_double * n)()
    fl = (C.c_double * n)()
    by = (C.c_double * n)()
    ln = (C.c_int64 * n)()
    call("nvit_prof_collect", ms, fl, by, ln)
    return {_lib.KID_NAMES[i]: {"ms": ms[i], "flops": fl[i], "bytes": by[i], "launches": ln[i]} for i in range(n)}
