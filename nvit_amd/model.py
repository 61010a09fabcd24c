"""nViT model whose forward/backward run on hand-written gfx950 HIP kernels.

Drop-in mirror of the reference module tree (/root/reference/nvit/model.py): same class
names, constructor and forward() signatures, parameter names and shapes (SURVEY.md §8b,
§9.5), so `ViT(ViTConfig(**model_args))`, `state_dict()/load_state_dict()`,
`configure_optimizers()` and the attribute accesses of the reference trainer
(train.py:422,474-480,1045-1054) work unchanged.  The nn.Conv2d / nn.Linear / nn.LayerNorm
sub-modules are parameter containers only: their torch forward is never called.  All
compute goes through the C ABI in include/nvit_hip.h (nvit_amd/ops.py); there is no CPU
or torch-operator fallback — without the HIP library or a GPU, forward() raises.

Both paths are implemented: nViT (`use_nvit=True`) and the plain-ViT baseline (`use_nvit=False`, without the Kohonen head),
each with both attention forms the reference selects by `flash_attn`.  `flash_attn=False` is SDPA over the tokens.
`flash_attn=True` computes what the reference's flash_attn_func call computes on its [B,H,T,d] tensors, which
flash-attn reads as [batch, seqlen, nheads, headdim]: a softmax over the H heads of each token, with no token mixing
(nvit_attn_heads_fwd/bwd, at most 32 heads).  The plain-ViT baseline's reference construction bug
(the RMSNorm modules its forward calls are built only for nViT) is repaired by building
`rmsnorm_att` / `rmsnorm_mlp` in both modes.

Precision modes (model.precision): "bf16" = bf16 MFMA operands, fp32 accumulate, fp32
residual stream/norms/params/grads (the performance mode); "fp32" = exact-f32 MFMA
everywhere (parity mode, <=1e-5 against the CPU oracle).
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from . import ops, resample
from ._lib import ATTN_HEADS_MAX_H, BF16, BF16_F32IN, F32, MAX_EMBD
from .config import ViTConfig
from .kohonen import CosConsistencyFn, HuberFn, KohonenMap, MapSmoothnessFn

Tensor = torch.Tensor
HEAD_DIMS = (32, 64, 128)   # attention head dims n_embd // n_head the kernels cover
# head dims that run on the 128-wide kernels with head tensors whose columns d..127 are stored zeros (_attn_fwd, "split")
PADDED_HEAD_DIMS = (72, 80, 88, 104)


def _dt_from_precision(p: str) -> int:
    if p == "fp32":
        return F32
    if p == "bf16":
        return BF16
    raise ValueError(f"precision must be 'fp32' or 'bf16', got {p!r}")


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        x2 = x.reshape(-1, x.shape[-1]).contiguous().float()
        out, rstd = ops.rmsnorm_fwd(x2, w.detach().contiguous().float(), eps)
        ctx.save_for_backward(x2, w, rstd)
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        x2, w, rstd = ctx.saved_tensors
        dx, dw = ops.rmsnorm_bwd(g.reshape(x2.shape).contiguous().float(), x2, w.detach().contiguous().float(), rstd)
        return dx.reshape(g.shape), dw, None


class RMSNorm(nn.Module):
    """reference model.py:170-182: x * rsqrt(mean(x^2) + eps) * weight, as one row kernel each way.  Dead in nViT mode
    (no Block calls it; its parameters exist for state_dict parity) but a working public module."""

    def __init__(self, embdim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(embdim))
        self.eps = eps

    def forward(self, x: Tensor) -> Tensor:
        if not x.is_cuda:
            raise RuntimeError("RMSNorm runs only on the HIP device (no CPU fallback)")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise RuntimeError(f"RMSNorm: floating-point input expected, got {x.dtype}")
        if x.dtype == torch.float32:
            return _RMSNormFn.apply(x, self.weight, self.eps)
        # reference model.py:176-182: computed in fp32, the normalised value cast back to the input dtype BEFORE the
        # weight multiply (torch type promotion then decides the output dtype)
        ones = torch.ones_like(self.weight)
        return self.weight * _RMSNormFn.apply(x, ones, self.eps).to(x.dtype)


# --------------------------------------------------------------------------------------------
# Runtime: precision, shadows (MFMA-operand copies of the fp32 master weights)
# --------------------------------------------------------------------------------------------
class _Runtime:
    """Per-model device state that is NOT part of the state_dict: bf16 (or fp32) weight shadows in
    the layouts the GEMMs want, rebuilt from the fp32 masters at the start of every forward."""

    def __init__(self, model: "ViT") -> None:
        self.model = model
        self.dt = F32
        self.device = None
        self.key = None
        self.sh: Dict[str, Tensor] = {}
        self.table = None
        self.items = 0
        self.btable = None
        self.bitems = 0
        # bf16 mode: the two data-gradient GEMMs that used to accumulate into the fp32 residual-stream gradient (c_fc
        # and q/k/v) store bf16 once and the next lerp_bwd adds it while it reads its incoming gradient anyway
        # (nvit_lerp_bwd dout_add).  `carry` hands the q/k/v addend to the backward of the PREVIOUS block of the chain
        # built by ViT.forward: (index of the consumer, tensor); -1 = the cross-attention block.
        self.carry = None
        # tokens per sample of the forward that is running: None = model.n_tokens; a forward that drops patches
        # (ViT.attach_patch_drop) sets the K it kept for the calls behind its gather and clears it when it returns.  A
        # backward reads the count its own forward saw from ctx.dims, never from here.
        self.tokens = None
        # side of the token grid of the forward that is running: None = the native one (config.image_size); a forward on
        # an image of another size (ViT.set_dynamic_img_size) sets it for the whole call and clears it when it returns.
        # Kept apart from `tokens`: patch dropout needs both, the T it draws from and the K it keeps.
        self.grid = None

    @property
    def grid_tokens(self) -> int:
        """Tokens per sample the running forward embeds (before any patch dropout)."""
        return self.model.n_tokens if self.grid is None else self.grid * self.grid

    @property
    def n_tokens(self) -> int:
        return self.grid_tokens if self.tokens is None else self.tokens

    def y_dtype(self) -> torch.dtype:
        """Storage type of the branch outputs y (att_c_proj / mlp_c_proj / out_proj results, the second LERP input).
        bf16 mode stores them in bf16, as the reference's own autocast path does (every nn.Linear returns
        bf16).  y only enters the stream through lam * (nrm(y) - nrm(h)) with lam ~ 0.05, so its rounding adds ~5e-6 rms
        to a stream error of ~2e-5; the matched CPU emulation rounds y at the same point."""
        return torch.bfloat16 if self.dt != F32 else torch.float32

    def grad_buf(self, params, shape) -> Tensor:
        """Destination of a parameter gradient: the data-parallel wrapper's flat bucket slice when it offers one
        (`model._grad_sink`, parallel.py: gradients are produced in place, nothing is copied), else a fresh tensor.
        `params`: the parameter, or the parameters whose gradients one GEMM writes stacked along dim 0."""
        sink = self.model._grad_sink
        if sink is not None:
            t = sink(params, shape)
            if t is not None:
                return t
        return torch.empty(shape, device=params[0].device, dtype=torch.float32)

    def _build(self, device, dt: int) -> None:
        m, cfg = self.model, self.model.config
        C, L = cfg.n_embd, cfg.n_layer
        td = ops.tdtype(dt)
        bk = ops.bk_of(dt)
        sh: Dict[str, Tensor] = {}
        ent = []   # weight shadows (type dt)
        bent = []  # bias shadows (fp32)

        def new(name, r, c):
            t = torch.empty((r, c), device=device, dtype=td)
            sh[name] = t
            return t

        def newb(name, n):
            t = torch.empty((n,), device=device, dtype=torch.float32)
            sh[name] = t
            return t

        def w2(p):  # 2-D view of a parameter
            return p.detach().reshape(p.shape[0], -1)

        Kl = cfg.channels * cfg.local_patch_size ** 2
        Kg = cfg.channels * cfg.global_patch_size ** 2
        if dt == F32:
            ent.append((w2(m.local_patch_embed.weight), new("pe_l", C, Kl), Kl, Kl, None, 0, 0, 0))
            ent.append((w2(m.global_patch_embed[1].weight), new("pe_g", C, Kg), Kg, Kg, None, 0, 0, 0))
        else:   # split-precision images, one [hi32 | lo32] slice per 32 patch elements (see _EmbedFn); padding stays zero
            for name, w, K in (("pe_l", m.local_patch_embed.weight, Kl), ("pe_g", m.global_patch_embed[1].weight, Kg)):
                Kp = ops.patch_kp(K)
                sh[name] = torch.zeros((C, 2 * Kp), device=device, dtype=td)
                ent.append((w2(w), sh[name], 2 * Kp, K, None, 0, 0, 2))

        def stack(prefix, lins, perm=0):
            """shadow of row-stacked Linear weights [sum rows, K] and its transpose [K, sum rows]."""
            rows = sum(l.weight.shape[0] for l in lins)
            K = lins[0].weight.shape[1]
            W = new(prefix + ".W", rows, K)
            Wt = new(prefix + ".Wt", K, rows)
            off = 0
            for l in lins:
                r = l.weight.shape[0]
                ent.append((w2(l.weight), W[off:], K, K, Wt[:, off:], rows, r, perm))
                off += r
            if lins[0].bias is not None:
                bsh = newb(prefix + ".b", rows)
                off = 0
                for l in lins:
                    r = l.weight.shape[0]
                    bent.append((l.bias.detach().reshape(r, 1), bsh[off:], 1, 1, None, 0, 0, perm))
                    off += r

        ca = m.cross_attention
        stack("x.q", [ca.q_local])
        stack("x.kv", [ca.k_global, ca.v_global])
        stack("x.proj", [ca.proj], perm=1)
        stack("x.out", [ca.out_proj])
        for i, blk in enumerate(m.transformer.h):
            stack(f"h{i}.qkv", [blk.query, blk.key, blk.value])
            stack(f"h{i}.o", [blk.att_c_proj])
            stack(f"h{i}.fc", [blk.c_fc], perm=1)
            stack(f"h{i}.p", [blk.mlp_c_proj])
            # suv in the interleaved (perm=1) column order of the c_fc shadow, for the fused SwiGLU epilogue
            if cfg.use_nvit:
                bent.append((blk.suv.detach().reshape(8 * C, 1), newb(f"h{i}.suv_i", 8 * C), 1, 1, None, 0, 0, 1))
        # classifier head: transposed shadow zero-padded along classes to a multiple of the K stage
        ncls = cfg.num_classes
        Kp = ops.round_up(ncls, bk)
        ent.append((w2(m.mlp_head[1].weight), new("head.W", ncls, C), C, C, new("head.Wt", C, Kp), Kp, Kp, 0))
        ent.append((w2(m.reconstruction_head[0].weight), new("rec.W", Kl, C), C, C, new("rec.Wt", C, Kl), Kl, Kl, 0))
        self.sh = sh
        self.table, self.items = ops.shadow_table(ent, device)
        if bent:
            self.btable, self.bitems = ops.shadow_table(bent, device)
        else:
            self.btable, self.bitems = None, 0

    def refresh(self, device, dt: int) -> None:
        key = (str(device), dt) + tuple(p.data_ptr() for p in self.model.parameters())
        if key != self.key:
            self._build(device, dt)
            self.key, self.device, self.dt = key, device, dt
        ops.shadow_weights(self.table, self.items, dt)
        if self.btable is not None:
            ops.shadow_weights(self.btable, self.bitems, F32)


# --------------------------------------------------------------------------------------------
# Functional forward / backward pieces (all compute through ops.*)
# --------------------------------------------------------------------------------------------
def _param_grad_alpha(rt, part: Tensor, alpha: Tensor, c_a: float, batch: "ops.ReduceBatch") -> Tensor:
    g = rt.grad_buf((alpha,), alpha.shape)
    batch.add(part, g, False, kind=1, ref=alpha, scale=c_a)
    return g


def _param_grad_scaled(rt, part: Tensor, like: Tensor, scale: float, batch: "ops.ReduceBatch",
                       part_b: Optional[Tensor] = None) -> Tensor:
    g = rt.grad_buf((like,), like.shape)
    batch.add(part, g, False, kind=0, scale=scale, part_b=part_b)
    return g


def _bias_grad(dy_lo: Tensor, M: int, N: int, perm: int = 0) -> Tensor:
    g = torch.empty((N,), device=dy_lo.device, dtype=torch.float32)
    if perm == 0:
        ops.colsum_big(dy_lo, M, N, g, False)
    else:
        part = torch.empty((512, N), device=dy_lo.device, dtype=torch.float32)
        ops.colsum(dy_lo, M, N, part, False, period=512)
        ops.colsum_reduce(part, g, False, kind=2)
    return g


def _lo(rt: _Runtime, x: Tensor, x_lo: Tensor) -> Tensor:
    """MFMA-operand copy of the residual stream: the bf16 twin written by the producing kernel, or
    (fp32 mode) the fp32 tensor itself, detached."""
    return x.detach() if rt.dt == F32 else x_lo


def _take_carry(rt: "_Runtime", idx: int, chained: bool, dout: Tensor):
    """(dout, addend): the bf16 addend the backward of block idx+1 left for this node (see _Runtime.carry), or None.  It is
    only valid for the very gradient tensor that node returned: anything else (a hook that replaced the gradient, a second
    consumer whose gradient autograd summed in) would silently drop or misplace it, so it is checked, not assumed.

    RESTRICTION of the chained bf16 mode: the gradient a chained block's backward RETURNS
    for its input lacks the q/k/v data-gradient part, which travels through `rt.carry` to the next backward node of
    ViT.forward's chain.  A tensor hook on a block input inside ViT.forward, or `autograd.grad` that stops at one, sees
    that incomplete gradient; an early stop leaves the addend dangling, which the NEXT forward reports (it raises).
    Stand-alone `Block.forward` calls are not chained and return complete gradients."""
    c, rt.carry = rt.carry, None
    if c is None:
        return dout, None
    want, dx, add = c
    if not chained or want != idx:
        raise RuntimeError("nvit_amd: pending q/k/v data gradient was not consumed by the block it was produced for")
    if dout.data_ptr() != dx.data_ptr():
        # autograd handed this node a different tensor (gradient hook / extra consumer of the block input): fold the
        # addend in explicitly - out of place, the gradient tensor belongs to autograd and may be shared with another
        # consumer - and carry on with the plain path
        return dout + add.float(), None
    return dout, add


RMS_EPS = 1e-6   # reference RMSNorm default (model.py:171)


def _lean() -> bool:
    """True when no backward can follow the forward being built (torch.no_grad / inference_mode: estimate_loss, validate
    and serving in the reference, train.py:482-506,577-627).  The block functions then store nothing that only their
    backward reads and save nothing; every value they return is the same bits.  Asked where a block function is APPLIED:
    inside an autograd.Function's forward grad mode is always off."""
    return not torch.is_grad_enabled()


def _dims(rt: _Runtime, M: int):
    """(B, T, C, H, d, M) of a block call over M = B*T token rows, T the running forward's count (_Runtime.tokens)."""
    cfg = rt.model.config
    T = rt.n_tokens
    return M // T, T, cfg.n_embd, cfg.n_head, cfg.n_embd // cfg.n_head, M


def _qkv_cols(ts, C: int):
    """(q, ldq, k, v, ldkv): q, k, v as column views of the stacked projection outputs, or of their gradients, `ts`:
    one [M, 3C] tensor (self-attention) or [M, C] and [M, 2C] (cross-attention)."""
    if len(ts) == 1:
        qkv, = ts
        return qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C
    q, kv = ts
    return q, C, kv, kv[:, C:], 2 * C


def _attn_fwd(rt: _Runtime, impl: int, srcs, sqk: Optional[Tensor], c_q: float, scale: float, dims,
              lean: bool = False):
    """The attention of every block function, from its q/k/v projection sources to O [M, C] (the output projection's A
    operand).  srcs: ((A, shadow prefix, parts), ...), one projection GEMM each, their output columns q | k | v in
    order.  sqk None (c_q 0.0): plain-ViT heads, else the nViT normalise + sqk scale.  One of three routes:
      heads  flash_attn=True: the reference's flash_attn_func reads its [B,H,T,d] arguments as [batch, seqlen, nheads,
             headdim], so the softmax runs over the H heads of each token of the fp32 token-major
             projections;
      fused  d = 64, C % 256 == 0 and a shape the fused GEMM takes (bf16 only; N of the FIRST projection decides): the
             bias (if any), the normalise (nViT) and the head split in the projection GEMM's epilogue, q pre-scaled so
             that the attention kernels' exponent needs no multiply;
      split  otherwise (small problems: 128x128 GEMM kernel): the projections leave the GEMM in fp32 and are normalised
             from the unrounded values, like the fused epilogue (one rounding, at the head tensors).  The head tensors
             are [B,H,T,dp]: dp = d, or for d in PADDED_HEAD_DIMS dp = 128 with columns d..127 stored zeros
             (heads_pad_fwd, which also pads sqk for the score bound): the attention kernels then run at head dim 128
             with the scale of the real d, and O [M, H*128] is compacted to [M, C].  Zero columns change no score, no
             output column < d and no gradient column < d.
    -> o, lse, att (route, impl, q pre-scale, scale) for _attn_bwd, and the tensors it reads: the fp32 projections
    (heads) or qh, kh, vh, rq, rk.
    lean (a forward no backward follows): the same launches - no attention kernel takes a NULL lse, rq or rk, so those
    small stores stay - but nothing is handed back for saving: the projections / head tensors are released here, before
    the caller allocates the MLP's tensors, not at the end of the block."""
    B, T, C, H, d, M = dims
    dt, sh = rt.dt, rt.sh
    heads = rt.model.config.flash_attn
    dp = ops.PAD_HEAD_DIM if d in PADDED_HEAD_DIMS else d   # (padded never with flash_attn: refused at construction)
    sqk_a = sqk   # as the attention kernel's score bound reads it
    if not heads and impl == 1 and d == 64 and C % 256 == 0 and ops.fusable(dt, M, srcs[0][2] * C, C):
        route = "fused"
        # the softmax scale (nViT: sqrt(d) on unit q, k) times log2(e); with sqk absent the running-maximum kernel runs
        # on the pre-scaled q (and the dK/dV backward takes its generated loop)
        qpre = ops.attn_q_prescale(d) if sqk is not None else ops.LOG2E / math.sqrt(d)
        bufs = ops.qk_buffers(dt, B, T, H, d, srcs[0][0].device, norm=sqk is not None)
        part0 = 0
        for A, w, n in srcs:
            ops.gemm_nt_qknorm(A, sh[w + ".W"], M, C, n, part0, sqk, c_q, B, T, H, d, bufs,
                               q_prescale=(qpre if part0 == 0 else 1.0), bias=sh.get(w + ".b"))
            part0 += n
    else:
        projs = [ops.gemm_nt(A, sh[w + ".W"], M, n * C, C, out_dtype=torch.float32, bias=sh.get(w + ".b"))
                 for A, w, n in srcs]
        q, ldq, k, v, ldkv = _qkv_cols(projs, C)
        if heads:
            o, lse = ops.attn_heads_fwd(dt, q, ldq, k, v, ldkv, sqk, c_q, scale, M, H, d)
            return o, lse, ("heads", impl, 1.0, scale), (() if lean else tuple(projs))
        route, qpre = "split", 1.0
        dt_in = dt if dt == F32 else BF16_F32IN   # the projection outputs are fp32 in both modes
        if dp != d:
            *bufs, sqk_a = ops.heads_pad_fwd(dt_in, q, ldq, k, ldkv, v, ldkv, sqk, c_q, B, T, H, d)
        else:
            bufs = ops.qknorm_fwd(dt_in, q, ldq, k, ldkv, v, ldkv, sqk, c_q, B, T, H, d)
        # plain and padded heads free the projections before O is allocated, compact nViT after attn_fwd (at return)
        if sqk is None or dp != d:
            del projs, q, k, v
    qh, kh, vh, _, _ = bufs
    o, lse = ops.attn_fwd(dt, impl, qh, kh, vh, scale, sqk_a, c_q, q_prescale=qpre)
    if dp != d:
        o = ops.unpad_cols(o, M, H, d)
    return o, lse, (route, impl, qpre, scale), (() if lean else tuple(bufs))


def _attn_bwd(rt: _Runtime, att, saved, do: Tensor, o: Tensor, lse: Tensor, grads, sqk: Optional[Tensor], c_q: float,
              dims):
    """Backward of _attn_fwd (att, saved: what it returned) into the token-major projection gradients `grads`, stacked
    like the projection outputs.  -> (part, part_k): the d(sqk*c_q) partials for the block's ReduceBatch (part_k: the k
    side of the fused backward, else None); (None, None) for plain heads."""
    B, T, C, H, d, M = dims
    dt = rt.dt
    route, impl, qpre, scale = att
    dq, lddq, dk, dv, lddkv = _qkv_cols(grads, C)
    if route == "heads":
        q, ldq, k, v, ldkv = _qkv_cols(saved, C)
        return ops.attn_heads_bwd(dt, do, q, ldq, k, v, ldkv, sqk, c_q, scale, lse, dq, lddq, dk, dv, lddkv, M, H,
                                  d), None
    qh, kh, vh, rq, rk = saved
    # attention backward with the q/k-normalise backward (nViT) fused into its epilogues, dq/dk/dv stored token-major:
    # nViT after either forward route (the split one leaves q unscaled, qpre 1); plain heads after the fused one only
    fused_bwd = (dt != F32 and d == 64) if sqk is not None else route == "fused"
    if fused_bwd:
        return ops.attn_bwd_qknorm(do, qh, kh, vh, o, lse, scale, rq, rk, sqk, c_q, dq, lddq, dk, dv, lddkv,
                                   q_prescale=qpre)
    dp = ops.PAD_HEAD_DIM if d in PADDED_HEAD_DIMS else d
    if dp != d:
        # dO and O zero-padded to the head tensors' width (the dQ kernel's delta = rowsum(dO*O) runs over all 128
        # columns; the padded O is rebuilt from the compact one, not kept from the forward), attn_bwd at 128, then the
        # merge, which reads the first d columns of each gradient only
        do, o = ops.pad_cols(do, M, H, d), ops.pad_cols(o, M, H, d)
    dqh, dkh, dvh = ops.attn_bwd(dt, impl, do, qh, kh, vh, o, lse, scale)
    del do, o   # (padded: the two copies are released before the merge)
    merge = ops.heads_pad_bwd if dp != d else ops.qknorm_bwd
    return merge(dt, dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, lddq, dk, lddkv, dv, lddkv, B, T, H, d), None


def _swiglu_fwd(rt: _Runtime, A: Tensor, w: str, M: int, F: int, K: int, gs: Optional[Tensor],
                gs_fused: Optional[Tensor], gscale: float, lean: bool = False):
    """Gated MLP input: uv = A W^T (+ bias) [M, 2F] (shadow `w`, interleaved columns) and x = swiglu(uv) [M, F] with the
    gate scale gs * gscale (gs None: 1).  -> (uv as backward reads it, x).  The fused GEMM epilogue takes gs in the
    shadow's interleaved column order (gs_fused), the row kernel in natural order (gs); the bias shadow is interleaved
    for both and joins the sums in either route's GEMM epilogue, so the saved uv includes it.
    lean (a forward no backward follows): uv is None - the fused GEMM does not store it (the gate-only epilogue, same
    x bit for bit), the unfused route does not make the bf16 copy."""
    dt, sh = rt.dt, rt.sh
    bias = sh.get(w + ".b")   # in the shadow's interleaved column order
    if ops.fusable(dt, M, 2 * F, K):
        if lean:
            return None, ops.gemm_nt_swiglu_act(A, sh[w + ".W"], M, F, K, gs_fused, gscale, bias=bias)
        return ops.gemm_nt_swiglu(A, sh[w + ".W"], M, F, K, gs_fused, gscale, bias=bias)
    uv32 = ops.gemm_nt(A, sh[w + ".W"], M, 2 * F, K, out_dtype=torch.float32, bias=bias)
    # bf16: the gate from the unrounded pre-activations; the bf16 copy is what backward reads
    x = ops.swiglu_fwd(dt if dt == F32 else BF16_F32IN, uv32, gs, gscale, M, F)
    if lean:
        return None, x
    return (uv32 if dt == F32 else ops.cast(uv32, dt)), x


def _swiglu_bwd(rt: _Runtime, dy: Tensor, w: str, uv: Tensor, M: int, F: int, K: int, gs: Optional[Tensor],
                gscale: float):
    """dy [M, K] through the following projection (transposed shadow `w`, [F, K]) and the SwiGLU backward: fused, the
    gate backward runs in the GEMM epilogue (dx never reaches HBM).  -> duv [M, 2F], d(gs) partials (None without gs)."""
    dt, sh = rt.dt, rt.sh
    if ops.fusable(dt, M, F, K):
        return ops.gemm_nt_swiglu_bwd(dy, sh[w + ".Wt"], uv, M, F, K, gs, gscale)
    dx = ops.gemm_nt(dy, sh[w + ".Wt"], M, F, K, out_dtype=ops.tdtype(dt))
    return ops.swiglu_bwd(dt, dx, uv, gs, gscale, M, F)


def _wgrad(rt: _Runtime, dy: Tensor, a: Tensor, params, M: int, N: int, K: int, has_b: bool, perm: int = 0):
    """Weight gradient dy^T a [N, K] of a linear into its destination (see _Runtime.grad_buf) and its bias gradient (None
    without bias).  perm 1: the rows of an interleaved (SwiGLU) shadow."""
    g = ops.gemm_tn(dy, a, rt.grad_buf(params, (N, K)), M, N, K, perm=perm)
    return g, (_bias_grad(dy, M, N, perm) if has_b else None)


class _BlockFn(torch.autograd.Function):
    """One nGPT block (+ norm_skip): reference Block.forward (model.py:92-169) followed by
    Block.norm_skip (model.py:84-87) as called at model.py:450-452."""

    @staticmethod
    def forward(ctx, x, x_lo, rt, idx, with_skip, impl, skip_param, attn_alpha, mlp_alpha, sqk, suv, wq, wk, wv, wo,
                wfc, wp, bq, bk_, bv, bo, bfc, bp, chained=False, lean=False, gates=None):
        # gates: None, or (attention, MLP) fp32 [B] each, this block's two rows of the DropPath table: the gated LERP
        # kernels then run in both directions (a dropped branch is still computed and discarded, as in timm)
        cfg = rt.model.config
        dims = _dims(rt, x.shape[0])
        B, T, C, H, d, M = dims
        dt = rt.dt
        sh = rt.sh
        c_q, c_a = 1.0 / cfg.base_scale, 0.05 / cfg.base_scale
        pre = f"h{idx}."
        has_b = bq is not None
        o, lse, att, att_saved = _attn_fwd(rt, impl, ((x_lo, pre + "qkv", 3),), sqk, c_q, math.sqrt(d), dims,
                                           lean)
        y = ops.gemm_nt(o, sh[pre + "o.W"], M, C, C, out_dtype=rt.y_dtype(), bias=sh.get(pre + "o.b"))
        g_att, g_mlp = gates if gates is not None else (None, None)
        h1, h1_lo = ops.lerp_fwd(dt, x, y, attn_alpha, c_a, want_lo=(dt != F32), gate=g_att)
        if dt == F32:
            h1_lo = h1
        # c_fc GEMM with the suv scale + SwiGLU gate (writes raw uv for backward and x_mlp)
        uv, xm = _swiglu_fwd(rt, h1_lo, pre + "fc", M, 4 * C, C, suv, sh[pre + "suv_i"], math.sqrt(C), lean)
        y2 = ops.gemm_nt(xm, sh[pre + "p.W"], M, C, 4 * C, out_dtype=rt.y_dtype(), bias=sh.get(pre + "p.b"))
        if with_skip:
            xn, xn_lo = ops.lerp_fwd(dt, h1, y2, mlp_alpha, c_a, skip_x=x, skip=skip_param, want_lo=(dt != F32),
                                     gate=g_mlp)
        else:
            xn, xn_lo = ops.lerp_fwd(dt, h1, y2, mlp_alpha, c_a, want_lo=(dt != F32), gate=g_mlp)
        if dt == F32:
            xn_lo = xn.new_empty(0)  # placeholder: callers alias x itself in fp32 mode (see _lo())
        if lean:   # no backward follows (see _lean()): nothing to save
            return xn, xn_lo
        ctx.rt, ctx.idx, ctx.with_skip, ctx.has_b, ctx.attn = rt, idx, with_skip, has_b, att
        ctx.chained = bool(chained)   # called from ViT.forward's block chain: the consumer of dx is our own backward node
        ctx.gates = (g_att, g_mlp)    # (rows of the step's gate table: B floats each, no gradient)
        ctx.dims = dims
        ctx.par = (skip_param, attn_alpha, mlp_alpha, sqk, suv, wq, wk, wv, wo, wfc, wp)   # gradient destinations
        ctx.save_for_backward(x, x_lo, o, lse, y, h1, h1_lo, uv, xm, y2, skip_param, attn_alpha, mlp_alpha, sqk, suv,
                              *att_saved)
        ctx.mark_non_differentiable(xn_lo)
        ctx.set_materialize_grads(False)  # no zero-filled [M,C] gradient for the bf16 twin on every backward
        return xn, xn_lo

    @staticmethod
    def backward(ctx, dxn, _unused):
        (x, x_lo, o, lse, y, h1, h1_lo, uv, xm, y2, skip_param, attn_alpha, mlp_alpha, sqk, suv,
         *att_saved) = ctx.saved_tensors
        rt, idx = ctx.rt, ctx.idx
        B, T, C, H, d, M = ctx.dims
        p_skip, p_aalpha, p_malpha, p_sqk, p_suv, p_wq, p_wk, p_wv, p_wo, p_wfc, p_wp = ctx.par
        cfg = rt.model.config
        dt, td = rt.dt, ops.tdtype(rt.dt)
        sh = rt.sh
        c_q, c_a = 1.0 / cfg.base_scale, 0.05 / cfg.base_scale
        pre = f"h{idx}."
        if dxn is None:
            return (None,) * 26
        dxn = dxn.contiguous()
        g_att, g_mlp = ctx.gates
        lo_dgrad = dt != F32
        red = ops.ReduceBatch()   # the block's six parameter-gradient reductions go out as one launch at the end
        dxn, carry_in = _take_carry(rt, idx, ctx.chained, dxn)   # q/k/v data gradient of the block after this one (bf16), or None
        # ---- MLP half + norm_skip
        if ctx.with_skip:
            dh1, _, dy2_lo, dx, part_lam, part_skip = ops.lerp_bwd(dt, dxn, h1, y2, mlp_alpha, c_a, x, skip_param,
                                                                   None, False, False, True, dout_add=carry_in,
                                                                   gate=g_mlp)
            dskip = rt.grad_buf((p_skip,), p_skip.shape)
            red.add(part_skip, dskip, False)
        else:
            # (never gated: ViT.forward's chain, the only gated caller, always runs with_skip)
            dh1, _, dy2_lo, _, part_lam, _ = ops.lerp_bwd(dt, dxn, h1, y2, mlp_alpha, c_a, None, None, None, False,
                                                          False, True, dout_add=carry_in)
            dx, dskip = None, None
        d_mlp_alpha = _param_grad_alpha(rt, part_lam, p_malpha, c_a, red)
        duv, part_suv = _swiglu_bwd(rt, dy2_lo, pre + "p", uv, M, 4 * C, C, suv, math.sqrt(C))
        g_wp, g_bp = _wgrad(rt, dy2_lo, xm, (p_wp,), M, C, 4 * C, ctx.has_b)
        d_suv = _param_grad_scaled(rt, part_suv, p_suv, 1.0, red)
        if lo_dgrad:
            dh1_add = ops.gemm_nt(duv, sh[pre + "fc.Wt"], M, C, 8 * C, out_dtype=td)   # bf16, added by the next lerp_bwd
        else:
            dh1_add = None
            ops.gemm_nt(duv, sh[pre + "fc.Wt"], M, C, 8 * C, out=dh1, accumulate=True)
        g_wfc, g_bfc = _wgrad(rt, duv, h1_lo, (p_wfc,), M, 8 * C, C, ctx.has_b, perm=1)
        # ---- attention half
        if dx is None:
            dx, _, dy_lo, _, part_lam, _ = ops.lerp_bwd(dt, dh1, x, y, attn_alpha, c_a, None, None, None, False,
                                                        False, True, dout_add=dh1_add)
        else:
            dx, _, dy_lo, _, part_lam, _ = ops.lerp_bwd(dt, dh1, x, y, attn_alpha, c_a, None, None, dx, True, False,
                                                        True, dout_add=dh1_add, gate=g_att)
        d_attn_alpha = _param_grad_alpha(rt, part_lam, p_aalpha, c_a, red)
        do = ops.gemm_nt(dy_lo, sh[pre + "o.Wt"], M, C, C, out_dtype=td)
        g_wo, g_bo = _wgrad(rt, dy_lo, o, (p_wo,), M, C, C, ctx.has_b)
        dqkv = torch.empty((M, 3 * C), device=x.device, dtype=td)
        part_q, part_k = _attn_bwd(rt, ctx.attn, att_saved, do, o, lse, (dqkv,), sqk, c_q, ctx.dims)
        d_sqk = _param_grad_scaled(rt, part_q, p_sqk, c_q, red, part_b=part_k)
        if lo_dgrad and ctx.chained:
            # the consumer of dx is the backward node of the previous block (or of the cross-attention block): hand it
            # the q/k/v data gradient as a separate bf16 addend instead of read-modify-writing dx
            rt.carry = (idx - 1, dx, ops.gemm_nt(dqkv, sh[pre + "qkv.Wt"], M, C, 3 * C, out_dtype=td))
        else:
            ops.gemm_nt(dqkv, sh[pre + "qkv.Wt"], M, C, 3 * C, out=dx, accumulate=True)
        # one stacked GEMM output = three adjacent bucket slices
        g_qkv, g_bqkv = _wgrad(rt, dqkv, x_lo, (p_wq, p_wk, p_wv), M, 3 * C, C, ctx.has_b)
        red.flush()
        gq, gk, gv = g_qkv[:C], g_qkv[C:2 * C], g_qkv[2 * C:]
        if ctx.has_b:
            gbq, gbk, gbv = g_bqkv[:C], g_bqkv[C:2 * C], g_bqkv[2 * C:]
        else:
            gbq = gbk = gbv = None
        return (dx, None, None, None, None, None, dskip, d_attn_alpha, d_mlp_alpha, d_sqk, d_suv, gq, gk, gv, g_wo,
                g_wfc, g_wp, gbq, gbk, gbv, g_bo, g_bfc, g_bp, None, None, None)


class _CrossFn(torch.autograd.Function):
    """CrossAttentionBlock.forward (reference model.py:219-275), nViT branch."""

    @staticmethod
    def forward(ctx, loc, glo, loc_lo, glo_lo, rt, impl, attn_alpha, sqk, wq, wk, wv, wproj, wout, bq, bk_, bv, bproj, bout,
                chained=False, lean=False):
        cfg = rt.model.config
        dims = _dims(rt, loc.shape[0])
        B, T, C, H, d, M = dims
        dt = rt.dt
        sh = rt.sh
        c_q, c_a = 1.0 / cfg.base_scale, 0.05 / cfg.base_scale
        has_b = bq is not None
        if dt == F32:
            loc_lo, glo_lo = loc, glo
        else:   # bf16 operand copies: handed in by the producer (patch-embedding epilogue) or cast here
            loc_lo = ops.cast(loc, dt) if loc_lo is None else loc_lo
            glo_lo = ops.cast(glo, dt) if glo_lo is None else glo_lo
        # q from the local stream, k/v from the global stream
        o, lse, att, att_saved = _attn_fwd(rt, impl, ((loc_lo, "x.q", 1), (glo_lo, "x.kv", 2)), sqk, c_q,
                                           math.sqrt(d), dims, lean)
        pr, g = _swiglu_fwd(rt, o, "x.proj", M, C, C, None, None, 1.0, lean)
        y = ops.gemm_nt(g, sh["x.out.W"], M, C, C, out_dtype=rt.y_dtype(), bias=sh.get("x.out.b"))
        x, x_lo = ops.lerp_fwd(dt, loc, y, attn_alpha, c_a, want_lo=(dt != F32))
        if dt == F32:
            x_lo = x.new_empty(0)
        if lean:
            return x, x_lo
        ctx.rt, ctx.has_b, ctx.attn = rt, has_b, att
        ctx.chained = bool(chained)
        ctx.dims = dims
        ctx.par = (attn_alpha, sqk, wq, wk, wv, wproj, wout)
        ctx.save_for_backward(loc, glo, loc_lo, glo_lo, o, lse, pr, g, y, attn_alpha, sqk, *att_saved)
        ctx.mark_non_differentiable(x_lo)
        ctx.set_materialize_grads(False)
        return x, x_lo

    @staticmethod
    def backward(ctx, dx, _unused):
        if dx is None:
            return (None,) * 20
        loc, glo, loc_lo, glo_lo, o, lse, pr, g, y, attn_alpha, sqk, *att_saved = ctx.saved_tensors
        rt = ctx.rt
        B, T, C, H, d, M = ctx.dims
        p_alpha, p_sqk, p_wq, p_wk, p_wv, p_wproj, p_wout = ctx.par
        cfg = rt.model.config
        dt, td = rt.dt, ops.tdtype(rt.dt)
        sh = rt.sh
        dev = loc.device
        c_q, c_a = 1.0 / cfg.base_scale, 0.05 / cfg.base_scale
        dx = dx.contiguous()
        red = ops.ReduceBatch()
        dx, carry_in = _take_carry(rt, -1, ctx.chained, dx)
        dloc, _, dy_lo, _, part_lam, _ = ops.lerp_bwd(dt, dx, loc, y, attn_alpha, c_a, None, None, None,
                                                      False, False, True, dout_add=carry_in)
        d_alpha = _param_grad_alpha(rt, part_lam, p_alpha, c_a, red)
        dpr, _ = _swiglu_bwd(rt, dy_lo, "x.out", pr, M, C, C, None, 1.0)
        g_wout, g_bout = _wgrad(rt, dy_lo, g, (p_wout,), M, C, C, ctx.has_b)
        do = ops.gemm_nt(dpr, sh["x.proj.Wt"], M, C, 2 * C, out_dtype=td)
        g_wproj, g_bproj = _wgrad(rt, dpr, o, (p_wproj,), M, 2 * C, C, ctx.has_b, perm=1)
        dq = torch.empty((M, C), device=dev, dtype=td)
        dkv = torch.empty((M, 2 * C), device=dev, dtype=td)
        part_q, part_k = _attn_bwd(rt, ctx.attn, att_saved, do, o, lse, (dq, dkv), sqk, c_q, ctx.dims)
        d_sqk = _param_grad_scaled(rt, part_q, p_sqk, c_q, red, part_b=part_k)
        ops.gemm_nt(dq, sh["x.q.Wt"], M, C, C, out=dloc, accumulate=True)
        dglo = ops.gemm_nt(dkv, sh["x.kv.Wt"], M, C, 2 * C, out_dtype=torch.float32)
        g_wq, g_bq = _wgrad(rt, dq, loc_lo, (p_wq,), M, C, C, ctx.has_b)
        g_wkv, g_bkv = _wgrad(rt, dkv, glo_lo, (p_wk, p_wv), M, 2 * C, C, ctx.has_b)
        red.flush()
        gbk, gbv = (g_bkv[:C], g_bkv[C:]) if ctx.has_b else (None, None)
        return (dloc, dglo, None, None, None, None, d_alpha, d_sqk, g_wq, g_wkv[:C], g_wkv[C:], g_wproj, g_wout, g_bq, gbk, gbv,
                g_bproj, g_bout, None, None)


class _StdBlockFn(torch.autograd.Function):
    """One plain-ViT block (use_nvit=False, reference Block.forward model.py:92-169 with rmsnorm_att / rmsnorm_mlp
    built) and, with_skip, the norm_skip after it (model.py:84-87,450-452):
        a = rms_att(x);  h1 = a + attn(a) W_o^T;  bm = rms_mlp(h1);  h2 = bm + swiglu(bm W_fc^T) W_p^T;
        out = nrm(h2 * skip + x)   (with_skip; else out = h2).
    Attention is softmax(q k^T / sqrt(d)) v on the running-max kernels; the SwiGLU gate scale is 1 (no suv).
    gates (stochastic depth, with_skip only): (g_att, g_mlp) fp32 [B], h1 = a + g_att * attn(..), h2 = bm + g_mlp * mlp(..)
    per sample.  Backward: the gradient that goes on down the stream (d(h1) into a, d(h2) into bm) is that of the sum; the
    copy the branch's GEMMs read is gate * it - the gated row kernels write both, so in fp32 mode, where the two are one
    tensor without a gate, they are two."""

    @staticmethod
    def forward(ctx, x, rt, idx, with_skip, want_lo, impl, skip_param, w_att, w_mlp, wq, wk, wv, wo, wfc, wp, bq, bk_,
                bv, bo, bfc, bp, lean=False, gates=None):
        dims = _dims(rt, x.shape[0])
        B, T, C, H, d, M = dims
        dt = rt.dt
        lo = dt != F32
        sh = rt.sh
        pre = f"h{idx}."
        has_b = bq is not None
        a, a_lo, r_att = ops.res_rmsnorm_fwd(dt, x, None, w_att.detach(), RMS_EPS, want_lo=lo)
        if not lo:
            a_lo = a
        o, lse, att, att_saved = _attn_fwd(rt, impl, ((a_lo, pre + "qkv", 3),), None, 0.0, 1.0 / math.sqrt(d),
                                           dims, lean)
        y = ops.gemm_nt(o, sh[pre + "o.W"], M, C, C, out_dtype=rt.y_dtype(), bias=sh.get(pre + "o.b"))
        g_att, g_mlp = gates if gates is not None else (None, None)
        bm, bm_lo, r_mlp = ops.res_rmsnorm_fwd(dt, a, y, w_mlp.detach(), RMS_EPS, want_lo=lo, gate=g_att)
        if not lo:
            bm_lo = bm
        uv, xm = _swiglu_fwd(rt, bm_lo, pre + "fc", M, 4 * C, C, None, None, 1.0, lean)
        if with_skip:
            y2 = ops.gemm_nt(xm, sh[pre + "p.W"], M, C, 4 * C, out_dtype=rt.y_dtype(), bias=sh.get(pre + "p.b"))
            xn, xn_lo = ops.res_skip_fwd(dt, bm, y2, skip_param.detach(), x, want_lo=(lo and want_lo), gate=g_mlp)
        else:   # the block output itself: h2 = bm + y2 in the GEMM epilogue (row-add of bm)
            y2 = ops.gemm_nt(xm, sh[pre + "p.W"], M, C, 4 * C, out_dtype=torch.float32, bias=sh.get(pre + "p.b"),
                             rowadd=bm, rowadd_period=M)
            xn, xn_lo = y2, (ops.cast(y2, dt) if lo and want_lo else None)
        if xn_lo is None:
            xn_lo = xn.new_empty(0)   # fp32 mode: callers alias the stream itself (see _lo())
        if lean:
            return xn, xn_lo
        ctx.rt, ctx.idx, ctx.with_skip, ctx.has_b, ctx.attn = rt, idx, with_skip, has_b, att
        ctx.dims = dims
        ctx.gates = (g_att, g_mlp)    # (rows of the step's gate table: B floats each, no gradient)
        ctx.par = (skip_param, w_att, w_mlp, wq, wk, wv, wo, wfc, wp)   # gradient destinations
        ctx.save_for_backward(x, a, a_lo, r_att, o, lse, y, bm, bm_lo, r_mlp, uv, xm, y2, skip_param, w_att, w_mlp,
                              *att_saved)
        ctx.mark_non_differentiable(xn_lo)
        ctx.set_materialize_grads(False)
        return xn, xn_lo

    @staticmethod
    def backward(ctx, dxn, _unused):
        if dxn is None:
            return (None,) * 23
        g_att, g_mlp = ctx.gates
        (x, a, a_lo, r_att, o, lse, y, bm, bm_lo, r_mlp, uv, xm, y2, skip_param, w_att, w_mlp,
         *att_saved) = ctx.saved_tensors
        rt, idx = ctx.rt, ctx.idx
        B, T, C, H, d, M = ctx.dims
        p_skip, p_watt, p_wmlp, p_wq, p_wk, p_wv, p_wo, p_wfc, p_wp = ctx.par
        dt, td = rt.dt, ops.tdtype(rt.dt)
        lo = dt != F32
        sh = rt.sh
        pre = f"h{idx}."
        dxn = dxn.contiguous()
        red = ops.ReduceBatch()
        # ---- norm_skip: d(h2) and the direct part of d(x)
        if ctx.with_skip:
            # gated: dh2 = d(bm + g*y2) goes on into bm, its copy (made in fp32 mode too) is g * dh2 = d(y2)
            dh2, dh2_lo, dx, part_skip = ops.res_skip_bwd(dt, dxn, bm, y2, skip_param, x,
                                                          want_lo=lo or g_mlp is not None, gate=g_mlp)
            dskip = rt.grad_buf((p_skip,), p_skip.shape)
            red.add(part_skip, dskip, False)
        else:
            dh2, dh2_lo, dx, dskip = dxn, (ops.cast(dxn, dt) if lo else None), None, None
        dy2_lo = dh2_lo if dh2_lo is not None else dh2
        # ---- MLP branch
        duv, _ = _swiglu_bwd(rt, dy2_lo, pre + "p", uv, M, 4 * C, C, None, 1.0)
        g_wp, g_bp = _wgrad(rt, dy2_lo, xm, (p_wp,), M, C, 4 * C, ctx.has_b)
        dbm_add = ops.gemm_nt(duv, sh[pre + "fc.Wt"], M, C, 8 * C, out_dtype=td)   # added by the rms_mlp backward
        g_wfc, g_bfc = _wgrad(rt, duv, bm_lo, (p_wfc,), M, 8 * C, C, ctx.has_b, perm=1)
        # ---- rms_mlp: d(h1) = d(a + y)
        dh1, dh1_lo, part_mlp = ops.res_rmsnorm_bwd(dt, dh2, a, y, w_mlp, r_mlp, g_add=dbm_add,
                                                    want_lo=lo or g_att is not None, gate=g_att)
        del dbm_add
        g_wmlp = _param_grad_scaled(rt, part_mlp, p_wmlp, 1.0, red)
        dy_lo = dh1_lo if dh1_lo is not None else dh1
        # ---- attention branch
        do = ops.gemm_nt(dy_lo, sh[pre + "o.Wt"], M, C, C, out_dtype=td)
        g_wo, g_bo = _wgrad(rt, dy_lo, o, (p_wo,), M, C, C, ctx.has_b)
        dqkv = torch.empty((M, 3 * C), device=x.device, dtype=td)
        _attn_bwd(rt, ctx.attn, att_saved, do, o, lse, (dqkv,), None, 0.0, ctx.dims)
        da_add = ops.gemm_nt(dqkv, sh[pre + "qkv.Wt"], M, C, 3 * C, out_dtype=td)
        g_qkv, g_bqkv = _wgrad(rt, dqkv, a_lo, (p_wq, p_wk, p_wv), M, 3 * C, C, ctx.has_b)
        # ---- rms_att: d(x) += rms backward of d(a) = d(h1) + q/k/v data gradient
        dx, _, part_att = ops.res_rmsnorm_bwd(dt, dh1, x, None, w_att, r_att, g_add=da_add, dz=dx)
        g_watt = _param_grad_scaled(rt, part_att, p_watt, 1.0, red)
        red.flush()
        gq, gk, gv = g_qkv[:C], g_qkv[C:2 * C], g_qkv[2 * C:]
        if ctx.has_b:
            gbq, gbk, gbv = g_bqkv[:C], g_bqkv[C:2 * C], g_bqkv[2 * C:]
        else:
            gbq = gbk = gbv = None
        return (dx, None, None, None, None, None, dskip, g_watt, g_wmlp, gq, gk, gv, g_wo, g_wfc, g_wp, gbq, gbk, gbv,
                g_bo, g_bfc, g_bp, None, None)


class _StdCrossFn(torch.autograd.Function):
    """CrossAttentionBlock.forward, plain-ViT branch (reference model.py:219-275, use_nvit=False): RMSNorm of both
    inputs, attention with scale 1/sqrt(d), proj -> SwiGLU -> out_proj; the output is out_proj's result itself."""

    @staticmethod
    def forward(ctx, loc, glo, rt, impl, w_ln, w_gn, wq, wk, wv, wproj, wout, bq, bk_, bv, bproj, bout, lean=False):
        dims = _dims(rt, loc.shape[0])
        B, T, C, H, d, M = dims
        dt = rt.dt
        lo = dt != F32
        sh = rt.sh
        has_b = bq is not None
        ln, ln_lo, r_l = ops.res_rmsnorm_fwd(dt, loc, None, w_ln.detach(), RMS_EPS, want_lo=lo)
        gn, gn_lo, r_g = ops.res_rmsnorm_fwd(dt, glo, None, w_gn.detach(), RMS_EPS, want_lo=lo)
        if not lo:
            ln_lo, gn_lo = ln, gn
        o, lse, att, att_saved = _attn_fwd(rt, impl, ((ln_lo, "x.q", 1), (gn_lo, "x.kv", 2)), None, 0.0,
                                           1.0 / math.sqrt(d), dims, lean)
        pr, g = _swiglu_fwd(rt, o, "x.proj", M, C, C, None, None, 1.0, lean)
        out = ops.gemm_nt(g, sh["x.out.W"], M, C, C, out_dtype=torch.float32, bias=sh.get("x.out.b"))
        if lean:
            return out
        ctx.rt, ctx.has_b, ctx.attn = rt, has_b, att
        ctx.dims = dims
        ctx.par = (w_ln, w_gn, wq, wk, wv, wproj, wout)
        ctx.save_for_backward(loc, glo, ln_lo, gn_lo, r_l, r_g, o, lse, pr, g, w_ln, w_gn, *att_saved)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 17
        loc, glo, ln_lo, gn_lo, r_l, r_g, o, lse, pr, g, w_ln, w_gn, *att_saved = ctx.saved_tensors
        rt = ctx.rt
        B, T, C, H, d, M = ctx.dims
        p_wln, p_wgn, p_wq, p_wk, p_wv, p_wproj, p_wout = ctx.par
        dt, td = rt.dt, ops.tdtype(rt.dt)
        dev = loc.device
        sh = rt.sh
        dout = dout.contiguous()
        red = ops.ReduceBatch()
        dy_lo = ops.cast(dout, dt) if dt != F32 else dout
        dpr, _ = _swiglu_bwd(rt, dy_lo, "x.out", pr, M, C, C, None, 1.0)
        g_wout, g_bout = _wgrad(rt, dy_lo, g, (p_wout,), M, C, C, ctx.has_b)
        do = ops.gemm_nt(dpr, sh["x.proj.Wt"], M, C, 2 * C, out_dtype=td)
        g_wproj, g_bproj = _wgrad(rt, dpr, o, (p_wproj,), M, 2 * C, C, ctx.has_b, perm=1)
        dq = torch.empty((M, C), device=dev, dtype=td)
        dkv = torch.empty((M, 2 * C), device=dev, dtype=td)
        _attn_bwd(rt, ctx.attn, att_saved, do, o, lse, (dq, dkv), None, 0.0, ctx.dims)
        dln = ops.gemm_nt(dq, sh["x.q.Wt"], M, C, C, out_dtype=torch.float32)
        dgn = ops.gemm_nt(dkv, sh["x.kv.Wt"], M, C, 2 * C, out_dtype=torch.float32)
        g_wq, g_bq = _wgrad(rt, dq, ln_lo, (p_wq,), M, C, C, ctx.has_b)
        g_wkv, g_bkv = _wgrad(rt, dkv, gn_lo, (p_wk, p_wv), M, 2 * C, C, ctx.has_b)
        dloc, _, part_l = ops.res_rmsnorm_bwd(dt, dln, loc, None, w_ln, r_l)
        dglo, _, part_g = ops.res_rmsnorm_bwd(dt, dgn, glo, None, w_gn, r_g)
        g_wln = _param_grad_scaled(rt, part_l, p_wln, 1.0, red)
        g_wgn = _param_grad_scaled(rt, part_g, p_wgn, 1.0, red)
        red.flush()
        gbk, gbv = (g_bkv[:C], g_bkv[C:]) if ctx.has_b else (None, None)
        return (dloc, dglo, None, None, g_wln, g_wgn, g_wq, g_wkv[:C], g_wkv[C:], g_wproj, g_wout, g_bq, gbk, gbv,
                g_bproj, g_bout, None)


class _EmbedFn(torch.autograd.Function):
    """Dual patch embedding + position embeddings (reference model.py:286-304,407-415): one fused gather + MFMA kernel in
    the bf16 mode, im2col + exact-f32 GEMMs in the fp32 mode."""

    @staticmethod
    def forward(ctx, img, rt, wl, bl, posl, wg, bg, posg):
        cfg = rt.model.config
        C = cfg.n_embd
        Pl, Pg = cfg.local_patch_size, cfg.global_patch_size
        B = img.shape[0]
        T = rt.grid_tokens   # (posl, posg hold T rows: the parameters, or their resampled copies at another image size)
        M = B * T
        Kl, Kg = cfg.channels * Pl * Pl, cfg.channels * Pg * Pg
        # Precision policy of the bf16 mode: the two patch embeddings are computed to fp32 accuracy.  They are 0.55 % of
        # the step's FLOPs but their output IS the residual stream, so a bf16-operand rounding here (1.6e-3 relative)
        # reaches the logits undamped, while every later update is scaled by the LERP rate (~0.05): max |dlogit| vs
        # the fp32 oracle drops 1.2e-3 -> 1.5e-4 (micro), 1.4e-3 -> 5.1e-4 (mini), 2.6e-3 -> 9.4e-4 (tiny).
        # Done on the bf16 MFMA path by operand splitting, x = hi + lo, w = hi + lo (bf16 each), three products
        # hi*hi + lo*hi + hi*lo (missing lo*lo ~ 2^-16 relative) - in ONE kernel that gathers the patches from the
        # image into LDS (no im2col matrix in HBM), adds bias + position embedding in its epilogue, and leaves the
        # bf16 patch rows behind for the weight gradient (patch_embed.hip).
        if rt.dt == F32:
            A_l, A_g = ops.im2col(F32, img, Pl, Pg)
            loc = ops.gemm_nt(A_l, rt.sh["pe_l"], M, C, Kl, bias=bl, rowadd=posl.reshape(T, C), rowadd_period=T)
            glo = ops.gemm_nt(A_g, rt.sh["pe_g"], M, C, Kg, bias=bg, rowadd=posg.reshape(T, C), rowadd_period=T)
        else:
            # (the split weight images are part of the shadow set, built by nvit_shadow_weights)
            loc, glo, A_l, A_g, loc_lo, glo_lo = ops.patch_embed_fwd(img, rt.sh["pe_l"], bl, posl.reshape(T, C),
                                                                     rt.sh["pe_g"], bg, posg.reshape(T, C), Pl, Pg, C,
                                                                     twins=(C % 8 == 0 and cfg.use_nvit))
        ctx.rt = rt
        ctx.dims = (B, T, C, M, Kl, Kg)
        ctx.par = (wl, wg)
        ctx.shapes = (wl.shape, wg.shape, posl.shape)
        ctx.save_for_backward(A_l, A_g)
        if rt.dt == F32 or loc_lo is None:
            loc_lo, glo_lo = loc.new_empty(0), loc.new_empty(0)
        ctx.mark_non_differentiable(loc_lo, glo_lo)
        return loc, glo, loc_lo, glo_lo

    @staticmethod
    def backward(ctx, dloc, dglo, _lo1, _lo2):
        A_l, A_g = ctx.saved_tensors   # bf16 mode: [Mpad, Kp] patch rows written by the fused forward kernel
        rt = ctx.rt
        B, T, C, M, Kl, Kg = ctx.dims
        dev = A_l.device
        out = []
        for dy, A, K, pw in ((dloc, A_l, Kl, ctx.par[0]), (dglo, A_g, Kg, ctx.par[1])):
            dy = dy.contiguous()
            dy_lo = dy if rt.dt == F32 else ops.cast(dy, rt.dt)
            gw = ops.gemm_tn(dy_lo, A[:M, :K], rt.grad_buf((pw,), (C, K)), M, C, K)
            dpos = torch.empty((T, C), device=dev, dtype=torch.float32)
            ops.colsum(dy, M, C, dpos, False, period=T)
            db = torch.empty((C,), device=dev, dtype=torch.float32)
            ops.colsum_big(dpos, T, C, db, False)
            out.append((gw, db, dpos))
        (gwl, dbl, dposl), (gwg, dbg, dposg) = out
        wls, wgs, ps = ctx.shapes
        return None, None, gwl.reshape(wls), dbl, dposl.reshape(ps), gwg.reshape(wgs), dbg, dposg.reshape(ps)


class _PosResampleFn(torch.autograd.Function):
    """Position tables [1, g*g, C] or [g*g, C] (one or two) resampled to the grid g2 x g2, same rank: nvit_pos_resample_fwd,
    both tables in one launch; backward its exact adjoint nvit_pos_resample_bwd (resample.py)."""

    @staticmethod
    def forward(ctx, g, g2, *tables):
        flat = [t.detach().reshape(g * g, t.shape[-1]).contiguous().float() for t in tables]
        outs = ops.pos_resample_fwd(flat[0], flat[1] if len(flat) > 1 else None, g, g2)
        ctx.grids = (g, g2)
        ctx.shapes = [t.shape for t in tables]
        return tuple(o.reshape(t.shape[:-2] + (g2 * g2, t.shape[-1])) for o, t in zip(outs, tables))

    @staticmethod
    def backward(ctx, *douts):
        g, g2 = ctx.grids
        flat = [d.reshape(g2 * g2, d.shape[-1]).contiguous().float() for d in douts]
        grads = ops.pos_resample_bwd(flat[0], flat[1] if len(flat) > 1 else None, g, g2)
        return (None, None) + tuple(gr.reshape(shp) for gr, shp in zip(grads, ctx.shapes))


def resample_pos_embed(pos: Tensor, grid: int) -> Tensor:
    """A square position-embedding table pos, fp32 [1, g*g, C] or [g*g, C] on the HIP device, resampled to grid x grid
    tokens: timm's resample_abs_pos_embed without prefix tokens, i.e. F.interpolate(mode="bicubic", antialias=True,
    align_corners=False) of the [C, g, g] image, computed in fp32 by a HIP kernel.  Same rank as pos; differentiable (the
    backward is the exact adjoint); grid == g returns pos itself.  C a multiple of 4, at most MAX_EMBD; a grid ratio beyond
    the kernels' taps per row raises ValueError.  HIP device only."""
    if not isinstance(pos, Tensor) or pos.dim() not in (2, 3) or (pos.dim() == 3 and pos.shape[0] != 1):
        raise ValueError("resample_pos_embed: pos must be a [1, g*g, C] or [g*g, C] tensor")
    if pos.dtype != torch.float32:
        raise ValueError(f"resample_pos_embed: fp32 table expected, got {pos.dtype}")
    g = resample.grid_of(pos.shape[-2])
    resample.check_grids(g, grid)
    if pos.shape[-1] % 4 or pos.shape[-1] > MAX_EMBD:
        raise ValueError(f"resample_pos_embed: C must be a multiple of 4, at most {MAX_EMBD} (got {pos.shape[-1]})")
    if grid == g:
        return pos
    resample.host_tables(g, grid)   # (ValueError for a ratio over the tap cap, before any device work)
    if not pos.is_cuda:
        raise RuntimeError("nvit_amd.resample_pos_embed runs only on the HIP device (no CPU fallback)")
    return _PosResampleFn.apply(g, grid, pos)[0]


class _TokenDropFn(torch.autograd.Function):
    """Patch dropout between the embedding and the cross-attention block: the kept tokens of both embedding streams,
    loc, glo fp32 [B*T, C] -> [B*K, C] by keep int32 [B, K] (nvit_rows_gather, one launch), with the bf16 twins of the
    gathered rows when the embedding produced twins (want_lo).  Backward: nvit_rows_scatter hands _EmbedFn.backward
    full-size [B*T, C] gradients whose rows of dropped tokens are zeros (slot int32 [B, T] is keep's inverse)."""

    @staticmethod
    def forward(ctx, loc, glo, keep, slot, want_lo):
        B, T = slot.shape
        K = keep.shape[1]
        loc_k, glo_k, loc_lo, glo_lo = ops.rows_gather(loc, glo, keep, B, T, lo_dt=(BF16 if want_lo else None))
        ctx.dims = (B, K)
        ctx.save_for_backward(slot)
        if not want_lo:
            loc_lo, glo_lo = loc.new_empty(0), loc.new_empty(0)
        ctx.mark_non_differentiable(loc_lo, glo_lo)
        return loc_k, glo_k, loc_lo, glo_lo

    @staticmethod
    def backward(ctx, dloc, dglo, _lo1, _lo2):
        slot, = ctx.saved_tensors
        B, K = ctx.dims
        gloc, gglo = ops.rows_scatter(dloc.contiguous(), dglo.contiguous(), slot, B, K)
        return gloc, gglo, None, None, None


class _HeadFn(torch.autograd.Function):
    """mean-pool -> LayerNorm -> Linear -> * sz (reference model.py:455-456,466-468); sz None (plain ViT): no scale."""

    @staticmethod
    def forward(ctx, x, rt, ln_w, ln_b, wh, bh, sz):
        cfg = rt.model.config
        C, ncls = cfg.n_embd, cfg.num_classes
        T = rt.n_tokens   # (K behind a patch-dropout gather: the mean runs over the kept tokens)
        B = x.shape[0] // T
        c_sz = cfg.sz_init_value / cfg.sz_init_scaling
        pooled, ln, ln_lo, stats = ops.pool_ln_fwd(rt.dt, x, ln_w, ln_b, 1e-5, B, T, C)
        if rt.dt != F32:
            # the classifier is [B,C]x[C,ncls] (0.2 GFLOP at Base): exact-f32 MFMA on the fp32 master costs nothing and
            # removes the largest single bf16 rounding term from the logits (1.98e-3 -> 1.23e-3 on the micro config)
            raw = ops.gemm_nt(ln, wh.contiguous(), B, ncls, C, bias=bh)
        else:
            raw = ops.gemm_nt(ln_lo, rt.sh["head.W"], B, ncls, C, bias=bh)
        logits = ops.scale_cols(raw, sz, c_sz, B, ncls, torch.empty_like(raw)) if sz is not None else raw
        ctx.rt = rt
        ctx.dims = (B, T, C, ncls, c_sz)
        ctx.save_for_backward(pooled, ln_lo, stats, raw, ln_w, sz)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        pooled, ln_lo, stats, raw, ln_w, sz = ctx.saved_tensors
        rt = ctx.rt
        B, T, C, ncls, c_sz = ctx.dims
        dev = pooled.device
        dt, td = rt.dt, ops.tdtype(rt.dt)
        dlogits = dlogits.contiguous()
        Kp = rt.sh["head.Wt"].shape[1]
        if sz is not None:
            d_sz = torch.empty_like(sz)
            ops.colsum(dlogits, B, ncls, d_sz, False, b=raw, scale=c_sz)
            draw = ops.scale_cols(dlogits, sz, c_sz, B, ncls, torch.empty((B, ncls), device=dev, dtype=torch.float32))
        else:
            d_sz, draw, c_sz = None, dlogits, 1.0
        d_bh = torch.empty((ncls,), device=dev, dtype=torch.float32)
        ops.colsum_big(draw, B, ncls, d_bh, False)
        draw_lo = torch.zeros((B, Kp), device=dev, dtype=td)
        ops.scale_cols(dlogits, sz, c_sz, B, ncls, draw_lo)   # (sz None: a plain copy into the padded operand)
        g_pad = ops.gemm_tn(draw_lo, ln_lo, torch.empty((Kp, C), device=dev, dtype=torch.float32), B, Kp, C)
        dln = ops.gemm_nt(draw_lo, rt.sh["head.Wt"], B, C, Kp)
        d_lnw = torch.empty_like(ln_w)
        d_lnb = torch.empty_like(ln_w)
        dx = ops.pool_ln_bwd(dln, pooled, ln_w, stats, d_lnw, d_lnb, False, B, T, C)
        return dx, None, d_lnw, d_lnb, g_pad[:ncls], d_bh, d_sz


class _NormSkipFn(torch.autograd.Function):
    """Block.norm_skip as a standalone call (reference model.py:84-87)."""

    @staticmethod
    def forward(ctx, source, target, skip):
        source, target = source.contiguous().float(), target.contiguous().float()
        ctx.save_for_backward(source, target, skip)
        return ops.norm_skip_fwd(source, target, skip)

    @staticmethod
    def backward(ctx, dout):
        source, target, skip = ctx.saved_tensors
        return ops.norm_skip_bwd(dout.contiguous(), source, target, skip)


class _JustNormFn(torch.autograd.Function):
    """x / ||x||_2 over the last axis (reference model.py:43-44), rows of up to 2048 fp32 values."""

    @staticmethod
    def forward(ctx, x2):
        one = torch.ones(1, device=x2.device, dtype=torch.float32)
        ctx.save_for_backward(x2, one)
        return ops.norm_skip_fwd(x2, None, one)

    @staticmethod
    def backward(ctx, dout):
        x2, one = ctx.saved_tensors
        return ops.norm_skip_bwd(dout.contiguous(), x2, None, one)[0]


def justnorm(x: Tensor) -> Tensor:
    """Module-level `justnorm` of the reference (model.py:43-44): x / x.norm(p=2, dim=-1, keepdim=True), no eps.
    Inside ViT.forward the normalisations are fused into the LERP / q-k / GEMM-epilogue kernels; this entry point is
    for callers that use it on its own.  HIP device only (no CPU path); the result has x's dtype."""
    if not x.is_cuda:
        raise RuntimeError("nvit_amd.justnorm runs only on the HIP device (no CPU fallback)")
    D = x.shape[-1]
    if D % 4 != 0 or D > 2048:
        raise ValueError(f"justnorm: last dimension must be a multiple of 4 and <= 2048 (got {D})")
    out = _JustNormFn.apply(x.reshape(-1, D).contiguous().float())
    return out.reshape(x.shape).to(x.dtype)


class _ReconFn(torch.autograd.Function):
    """reconstruction head + loss: mean((tanh(x W_r^T + b_r) - local patches)^2) (reference model.py:459-464)."""

    @staticmethod
    def forward(ctx, x, x_lo, rt, img, wr, br):
        cfg = rt.model.config
        C, P = cfg.n_embd, cfg.local_patch_size
        Kl = cfg.channels * P * P
        M = x.shape[0]
        raw = ops.gemm_nt(x_lo, rt.sh["rec.W"], M, Kl, C, bias=br)
        loss = ops.recon_loss(raw, img, P)
        ctx.rt = rt
        ctx.dims = (M, C, Kl, P)
        ctx.save_for_backward(raw, img, x_lo)
        return loss

    @staticmethod
    def backward(ctx, g):
        raw, img, x_lo = ctx.saved_tensors
        rt = ctx.rt
        M, C, Kl, P = ctx.dims
        draw = ops.recon_bwd(rt.dt, raw, img, g.contiguous().reshape(1), P)
        dx = ops.gemm_nt(draw, rt.sh["rec.Wt"], M, C, Kl)
        g_w = ops.gemm_tn(draw, x_lo, torch.empty((Kl, C), device=raw.device, dtype=torch.float32), M, Kl, C)
        g_b = torch.empty((Kl,), device=raw.device, dtype=torch.float32)
        ops.colsum_big(draw, M, Kl, g_b, False)
        return dx, None, None, None, g_w, g_b


# --------------------------------------------------------------------------------------------
# Modules (parameter containers with the reference's names)
# --------------------------------------------------------------------------------------------
class Block(nn.Module):
    def __init__(self, config: ViTConfig) -> None:
        super().__init__()
        self.config = config
        C = config.n_embd
        self.key = nn.Linear(C, C, bias=config.bias)
        self.query = nn.Linear(C, C, bias=config.bias)
        self.value = nn.Linear(C, C, bias=config.bias)
        self.att_c_proj = nn.Linear(C, C, bias=config.bias)
        self.skip_param = nn.Parameter(torch.ones(1))
        self.c_fc = nn.Linear(C, 2 * 4 * C, bias=config.bias)
        self.silu = nn.SiLU()
        self.mlp_c_proj = nn.Linear(4 * C, C, bias=config.bias)
        # built in both modes: the reference builds them for use_nvit=True only, where they are dead, and its
        # use_nvit=False forward, which calls them, crashes; the nViT state_dict is unchanged
        self.rmsnorm_att = RMSNorm(C)
        self.rmsnorm_mlp = RMSNorm(C)
        if config.use_nvit:
            bs = config.base_scale
            self.attn_alpha_init_value = torch.scalar_tensor(0.05, dtype=torch.float32)
            self.attn_alpha_init_scaling = torch.scalar_tensor(bs, dtype=torch.float32)
            self.attn_alpha = nn.Parameter(bs * torch.ones(C, dtype=torch.float32))
            self.mlp_alpha_init_value = torch.scalar_tensor(0.05, dtype=torch.float32)
            self.mlp_alpha_init_scaling = torch.scalar_tensor(bs, dtype=torch.float32)
            self.mlp_alpha = nn.Parameter(bs * torch.ones(C, dtype=torch.float32))
            self.sqk_init_value = torch.scalar_tensor(1.0, dtype=torch.float32)
            self.sqk_init_scaling = torch.scalar_tensor(bs, dtype=torch.float32)
            self.sqk = nn.Parameter(bs * torch.ones(C, dtype=torch.float32))
            self.suv_init_value = torch.scalar_tensor(1.0, dtype=torch.float32)
            self.suv_init_scaling = torch.scalar_tensor(1.0, dtype=torch.float32)
            self.suv = nn.Parameter(torch.ones(2 * 4 * C, dtype=torch.float32))
        self._owner = None  # set by ViT: (weakref to model, layer index)

    def _args(self):
        b = lambda l: l.bias
        if self.config.use_nvit:
            lead = (self.skip_param, self.attn_alpha, self.mlp_alpha, self.sqk, self.suv)
        else:
            lead = (self.skip_param, self.rmsnorm_att.weight, self.rmsnorm_mlp.weight)
        return lead + (self.query.weight, self.key.weight, self.value.weight, self.att_c_proj.weight, self.c_fc.weight,
                       self.mlp_c_proj.weight, b(self.query), b(self.key), b(self.value), b(self.att_c_proj),
                       b(self.c_fc), b(self.mlp_c_proj))

    def _run(self, x: Tensor, x_lo: Tensor, with_skip: bool, chained: bool = False, want_lo: bool = True,
             gates=None):
        """-> (new stream, its MFMA-operand copy).  Plain-ViT mode: the copy is made only when `want_lo` (the blocks
        read their normalised inputs, not the stream; only the reconstruction head after the last block needs it).
        gates: this block's (attention, MLP) rows of the step's DropPath table, from ViT.forward's chain only
        (with_skip)."""
        model, idx = self._owner
        rt = model._rt
        if gates is not None and not with_skip:
            raise ValueError("Block._run: gates go with the block chain of ViT.forward (with_skip) only")
        if not self.config.use_nvit:
            xn, xn_lo = _StdBlockFn.apply(x, rt, idx, with_skip, want_lo, model._attn_impl(), *self._args(), _lean(),
                                          gates)
            return xn, (_lo(rt, xn, xn_lo) if want_lo else None)
        xn, xn_lo = _BlockFn.apply(x, x_lo, rt, idx, with_skip, model._attn_impl(), *self._args(), chained, _lean(),
                                   gates)
        return xn, _lo(rt, xn, xn_lo)

    def norm_skip(self, source: Tensor, target: Tensor) -> Tensor:
        """nrm(source * skip_param + target) (reference model.py:84-87)."""
        shp = source.shape
        Cc = shp[-1]
        out = _NormSkipFn.apply(source.reshape(-1, Cc), target.reshape(-1, Cc), self.skip_param)
        return out.reshape(shp)

    def justnorm(self, x: Tensor) -> Tensor:
        """Reference model.py:89-90."""
        return justnorm(x)

    def forward(self, h: Tensor) -> Tensor:
        """h [B,T,C] -> [B,T,C] (block output BEFORE norm_skip, like the reference)."""
        model, _ = self._owner
        B, T, C = h.shape
        x, x_lo = model._enter(h.reshape(B * T, C))
        out, _ = self._run(x, x_lo, False)
        return out.reshape(B, T, C)


class CrossAttentionBlock(nn.Module):
    def __init__(self, config: ViTConfig) -> None:
        super().__init__()
        self.config = config
        C = config.n_embd
        if not config.use_nvit:
            self.local_norm = RMSNorm(C)
            self.global_norm = RMSNorm(C)
        self.q_local = nn.Linear(C, C, bias=config.bias)
        self.k_global = nn.Linear(C, C, bias=config.bias)
        self.v_global = nn.Linear(C, C, bias=config.bias)
        self.proj = nn.Linear(C, 2 * C, bias=config.bias)
        self.silu = nn.SiLU()
        self.out_proj = nn.Linear(C, C, bias=config.bias)
        if config.use_nvit:
            bs = config.base_scale
            self.attn_alpha_init_value = torch.scalar_tensor(0.05, dtype=torch.float32)
            self.attn_alpha_init_scaling = torch.scalar_tensor(bs, dtype=torch.float32)
            self.attn_alpha = nn.Parameter(bs * torch.ones(C, dtype=torch.float32))
            self.sqk_init_value = torch.scalar_tensor(1.0, dtype=torch.float32)
            self.sqk_init_scaling = torch.scalar_tensor(bs, dtype=torch.float32)
            self.sqk = nn.Parameter(bs * torch.ones(C, dtype=torch.float32))
        self._owner = None

    def _args(self):
        b = lambda l: l.bias
        if not self.config.use_nvit:
            return (self.local_norm.weight, self.global_norm.weight, self.q_local.weight, self.k_global.weight,
                    self.v_global.weight, self.proj.weight, self.out_proj.weight, b(self.q_local), b(self.k_global),
                    b(self.v_global), b(self.proj), b(self.out_proj))
        return (self.attn_alpha, self.sqk, self.q_local.weight, self.k_global.weight, self.v_global.weight,
                self.proj.weight, self.out_proj.weight, b(self.q_local), b(self.k_global), b(self.v_global),
                b(self.proj), b(self.out_proj))

    def _run(self, loc: Tensor, glo: Tensor, loc_lo: Optional[Tensor] = None, glo_lo: Optional[Tensor] = None,
             chained: bool = False):
        model = self._owner
        if not self.config.use_nvit:   # (the plain branch reads its RMS-normalised inputs: no operand copies needed)
            return _StdCrossFn.apply(loc, glo, model._rt, model._attn_impl(), *self._args(), _lean()), None
        x, x_lo = _CrossFn.apply(loc, glo, loc_lo, glo_lo, model._rt, model._attn_impl(), *self._args(), chained,
                                 _lean())
        return x, _lo(model._rt, x, x_lo)

    def forward(self, local: Tensor, global_: Tensor) -> Tensor:
        model = self._owner
        B, T, C = local.shape
        model._prepare(local.device)
        x, _ = self._run(local.reshape(B * T, C).contiguous(), global_.reshape(B * T, C).contiguous())
        return x.reshape(B, T, C)


class ViT(nn.Module):
    def __init__(self, config: ViTConfig):
        super().__init__()
        if not config.use_nvit and config.use_kohonen:
            raise NotImplementedError("use_nvit=False with use_kohonen=True is not supported: the plain-ViT baseline runs "
                                      "without the Kohonen head only (no reference run profile uses that combination)")
        if config.n_embd % config.n_head != 0 or config.n_embd % 64 != 0:
            raise ValueError("n_embd must be a multiple of 64 and divisible by n_head")
        if config.n_embd > MAX_EMBD:
            raise ValueError(f"n_embd must be at most {MAX_EMBD}, the widest row the row kernels hold (got {config.n_embd})")
        if (config.n_embd // config.n_head) not in HEAD_DIMS + PADDED_HEAD_DIMS:
            raise ValueError(f"head dim must be one of {HEAD_DIMS} or, zero-padded to 128, one of {PADDED_HEAD_DIMS} "
                             f"(got {config.n_embd // config.n_head})")
        if config.flash_attn and (config.n_embd // config.n_head) in PADDED_HEAD_DIMS:
            raise ValueError(f"flash_attn=True (attention over the heads of each token) is built for head dims {HEAD_DIMS}; "
                             f"head dim {config.n_embd // config.n_head} runs with flash_attn=False only")
        if config.flash_attn and config.n_head > ATTN_HEADS_MAX_H:
            raise ValueError(f"flash_attn=True (attention over the heads of each token) is built for at most "
                             f"{ATTN_HEADS_MAX_H} heads (got n_head={config.n_head})")
        self.config = config
        self.step = 0
        self.total_steps = 0
        C = config.n_embd
        Pl, Pg = config.local_patch_size, config.global_patch_size
        self.local_patch_embed = nn.Conv2d(config.channels, C, kernel_size=Pl, stride=Pl)
        self.global_patch_embed = nn.Sequential(
            nn.ReflectionPad2d((Pg - Pl) // 2),
            nn.Conv2d(config.channels, C, kernel_size=Pg, stride=Pl),
        )
        self.n_tokens = (config.image_size // Pl) ** 2
        self.local_pos_embed = nn.Parameter(torch.zeros(1, self.n_tokens, C))
        self.global_pos_embed = nn.Parameter(torch.zeros(1, self.n_tokens, C))
        if config.use_kohonen:   # reference model.py:311-323
            k_alpha = config.kohonen_alpha if not config.kohonen_scheduler_enabled else config.kohonen_scheduler_min_lr
            self.local_kohonen = KohonenMap(C, config.kohonen_nodes // 2, k_alpha)
            self.global_kohonen = KohonenMap(C, config.kohonen_nodes // 2, k_alpha)
            self.map_balance = nn.Parameter(torch.tensor(config.map_balance_weight))
        self.cross_attention = CrossAttentionBlock(config)
        self.reconstruction_head = nn.Sequential(nn.Linear(C, Pl * Pl * config.channels), nn.Tanh())
        self.transformer = nn.ModuleDict({
            "drop": nn.Dropout(config.dropout),
            "h": nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
        })
        self.mlp_head = nn.Sequential(nn.LayerNorm(C), nn.Linear(C, config.num_classes))
        if config.use_nvit:
            self.sz = nn.Parameter(config.sz_init_scaling * torch.ones(config.num_classes, dtype=torch.float32))
        self._init_parameters()
        # runtime (not part of the state_dict)
        self.precision = os.environ.get("NVIT_PRECISION", "bf16")
        object.__setattr__(self, "_rt", _Runtime(self))
        object.__setattr__(self, "_node_sync", None)   # set by DataParallel: averages SOM nodes across ranks
        object.__setattr__(self, "_taps", None)        # tests: dict that receives the residual stream after each block
        object.__setattr__(self, "_grad_sink", None)   # set by DataParallel: gradients are produced inside its buckets
        object.__setattr__(self, "drop_path", None)    # attach_drop_path: stochastic depth of the block chain (training only)
        object.__setattr__(self, "patch_drop", None)   # attach_patch_drop: patch dropout behind the embedding (training only)
        object.__setattr__(self, "_dynamic_img_size", False)   # set_dynamic_img_size: forward takes other image sizes
        # set_input_size counts here: objects that hold the addresses of the parameters it replaced (GraphedTrainStep,
        # GraphedEval) compare it with the value they were built at and refuse the model
        object.__setattr__(self, "_size_epoch", 0)
        object.__setattr__(self.cross_attention, "_owner", self)
        for i, blk in enumerate(self.transformer.h):
            object.__setattr__(blk, "_owner", (self, i))

    # ---- init (reference model.py:354-367: Linear N(0,0.02), *c_proj N(0,0.02/sqrt(2L)), LN ones/zeros, sz const)
    def _init_parameters(self) -> None:
        L = self.config.n_layer
        for name, mod in self.named_modules():
            if isinstance(mod, nn.Linear):
                std = 0.02 / math.sqrt(2 * L) if name.endswith("c_proj") else 0.02
                nn.init.normal_(mod.weight, mean=0.0, std=std)
                if mod.bias is not None:
                    nn.init.zeros_(mod.bias)
            elif isinstance(mod, nn.LayerNorm):
                nn.init.ones_(mod.weight)
                nn.init.zeros_(mod.bias)
        if self.config.use_nvit:
            with torch.no_grad():
                self.sz.fill_(self.config.sz_init_value)

    def _stacked_grads(self):
        """Weights whose gradients leave ONE weight-gradient GEMM stacked along dim 0, in that GEMM's row order (the
        data-parallel wrapper lays them out adjacently so the GEMM writes the bucket directly)."""
        ca = self.cross_attention
        groups = [(ca.k_global.weight, ca.v_global.weight)]
        for blk in self.transformer.h:
            groups.append((blk.query.weight, blk.key.weight, blk.value.weight))
        return groups

    # ---- runtime helpers
    def set_precision(self, precision: str) -> "ViT":
        _dt_from_precision(precision)
        self.precision = precision
        return self

    def _check_image_size(self, S, what: str) -> int:
        """The token-grid side of an S x S image, or ValueError: S a multiple of the local patch, larger than the reflect
        pad of the global patch embedding (what the patch kernels accept)."""
        cfg = self.config
        Pl, Pg = cfg.local_patch_size, cfg.global_patch_size
        if isinstance(S, bool) or not isinstance(S, int) or S < 4 or S % Pl != 0:
            raise ValueError(f"{what}: the image side must be a positive multiple of local_patch_size = {Pl} (got {S!r})")
        if (Pg - Pl) // 2 >= S:
            raise ValueError(f"{what}: the image side {S} must exceed the reflect pad {(Pg - Pl) // 2} of the global patch "
                             "embedding")
        return S // Pl

    def set_input_size(self, image_size: int) -> "ViT":
        """Permanently change the model's image size (timm's set_input_size), to fine-tune at another resolution: both
        position-embedding tables become NEW nn.Parameters holding the tables resampled to the new token grid
        (resample_pos_embed: bicubic, antialiased, in fp32 on the device), and config.image_size (a copy of the config;
        the object handed to the constructor is left alone) and n_tokens follow.  Every other parameter is untouched.
        Because the two parameters are new objects, anything built on the old ones is stale: build a new optimizer and a
        new ModelEma (their state is not resampled), a new DataParallel wrapper (its buckets hold the old parameters), and
        a new GraphedTrainStep / GraphedEval (the old ones raise ValueError when called).  The current size is a no-op that changes no bit and replaces nothing.  The model must be
        on the HIP device unless the size is the current one.  A checkpoint saved afterwards carries the new size."""
        g2 = self._check_image_size(image_size, "set_input_size")
        if image_size == self.config.image_size:
            return self
        g = resample.grid_of(self.n_tokens)
        resample.host_tables(g, g2)   # (ValueError for a ratio over the tap cap, before any device work)
        posl, posg = self.local_pos_embed, self.global_pos_embed
        if not posl.is_cuda:
            raise RuntimeError("ViT.set_input_size resamples the position embeddings on the HIP device: move the model "
                               "there first (no CPU fallback)")
        C = self.config.n_embd
        with torch.no_grad():
            outl, outg = ops.pos_resample_fwd(posl.detach().reshape(g * g, C).contiguous().float(),
                                              posg.detach().reshape(g * g, C).contiguous().float(), g, g2)
        self.local_pos_embed = nn.Parameter(outl.reshape(1, g2 * g2, C), requires_grad=posl.requires_grad)
        self.global_pos_embed = nn.Parameter(outg.reshape(1, g2 * g2, C), requires_grad=posg.requires_grad)
        config = dataclasses.replace(self.config, image_size=image_size)
        for mod in self.modules():
            if getattr(mod, "config", None) is self.config and mod is not self:
                mod.config = config
        self.config = config
        self.n_tokens = g2 * g2
        object.__setattr__(self, "_size_epoch", self._size_epoch + 1)
        return self

    def set_dynamic_img_size(self, flag: bool = True) -> "ViT":
        """Off (the default): forward takes images of config.image_size only, anything else is a ValueError.  On (timm's
        dynamic_img_size=True): forward takes [B, ch, S, S] for every S that is a multiple of local_patch_size and larger
        than the global embedding's reflect pad; the two position tables are resampled to the (S / local_patch_size)^2
        grid inside the forward (resample_pos_embed), their gradients land on the native-size parameters, and everything
        behind the embedding runs on the forward's own token count - both model kinds, both attention forms, biases, the
        Kohonen head, the no_grad route, DropPath and PatchDropout (K from the forward's T).  S == config.image_size
        launches exactly what it launches with the flag off.  A method, not a config field: ViTConfig mirrors the
        reference's dataclass.  A resize beyond the kernels' taps per row (about 8x either way) is a ValueError."""
        object.__setattr__(self, "_dynamic_img_size", bool(flag))
        return self

    def _running_grid(self, img: Tensor) -> Optional[int]:
        """None for an image of the native size, else the token-grid side of this forward; ValueError, before any device
        work, for an image forward cannot take."""
        if img.dim() != 4:
            raise ValueError(f"ViT.forward: images [B, channels, S, S] expected, got shape {tuple(img.shape)}")
        S = img.shape[-1]
        if img.shape[-2] != S:
            raise ValueError(f"ViT.forward: square images only, got {img.shape[-2]} x {S}")
        if S == self.config.image_size:
            return None
        if not self._dynamic_img_size:
            raise ValueError(f"ViT.forward: image side {S}, the model's is {self.config.image_size}; "
                             "set_dynamic_img_size(True) resamples the position embeddings per forward, "
                             "set_input_size changes the model")
        g2 = self._check_image_size(S, "ViT.forward")
        resample.host_tables(resample.grid_of(self.n_tokens), g2)   # (ValueError for a ratio over the tap cap)
        return g2

    def attach_drop_path(self, drop_path) -> "ViT":
        """Stochastic depth for the block chain of forward(): `drop_path` is a `DropPath` (droppath.py) moved to the
        model's device, or None to detach.  While the model is in training mode and the rate is > 0, every forward calls
        `drop_path.draw(n_layer, B)` exactly once and hands rows 2*l and 2*l + 1 of the fp32 [2*n_layer, B] table it
        returns to block l (attention and MLP branch).  nViT: the gated LERP kernels multiply the step of every row of
        sample b by gate[b]; plain ViT: the gated residual kernels add gate[b] * branch output.  The backward is that of the
        gated forward.  The cross-attention block, the Kohonen head, the classifier head and stand-alone Block.forward are
        not gated.  eval(), no attachment or rate 0 launch exactly what they launch without the feature.  A scale_by_keep
        of None is resolved here: True for the plain ViT (timm's), False for nViT.
        Not part of the state_dict or the config: save `drop_path.state_dict()` (checkpoint.py takes drop_path=)."""
        if drop_path is None:
            object.__setattr__(self, "drop_path", None)
            return self
        from .droppath import DropPath
        if not isinstance(drop_path, DropPath):
            raise TypeError("attach_drop_path takes a DropPath or None")
        if drop_path.scale_by_keep is None:
            drop_path.scale_by_keep = not self.config.use_nvit
        object.__setattr__(self, "drop_path", drop_path)
        return self

    def _draw_gates(self, B: int):
        """The step's gate table, or None when stochastic depth is off (eval, nothing attached, rate 0)."""
        dp = self.drop_path
        if dp is None or not self.training or dp.rate <= 0.0:
            return None
        L = self.config.n_layer
        table = dp.draw(L, B)
        if (not isinstance(table, Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (2 * L, B)
                or not table.is_cuda or not table.is_contiguous()):
            raise ValueError(f"DropPath.draw must return a contiguous fp32 [{2 * L}, {B}] device tensor")
        return table

    def attach_patch_drop(self, patch_drop) -> "ViT":
        """Patch dropout for forward(): `patch_drop` is a `PatchDropout` (patchdrop.py) moved to the model's device, or
        None to detach.  While the model is in training mode with gradients enabled and the rate is > 0, every forward
        calls `patch_drop.draw(B, T)` exactly once, gathers the K kept tokens of both embedding streams directly behind the
        patch embedding (position embeddings included) and runs the cross-attention block, the block chain, stochastic
        depth and the mean-pool on K tokens per sample; the shape-dependent route choices decide by the K-token shapes.
        The backward scatters the gradients back to [B*T, C] with zero rows for the dropped tokens.  Such a forward does
        not evaluate the reconstruction head (see forward).  eval(), torch.no_grad(), nothing attached or rate 0 launch
        exactly what they launch without the feature.  Not with the Kohonen head (ValueError): the SOM and the
        reconstruction loss are defined per image patch.  A data-parallel rank passes first_index = rank * B.
        Not part of the state_dict or the config: save `patch_drop.state_dict()` (checkpoint.py takes patch_drop=)."""
        if patch_drop is None:
            object.__setattr__(self, "patch_drop", None)
            return self
        from .patchdrop import PatchDropout
        if not isinstance(patch_drop, PatchDropout):
            raise TypeError("attach_patch_drop takes a PatchDropout or None")
        if self.config.use_kohonen:
            raise ValueError("attach_patch_drop: not with use_kohonen=True (the SOM and the reconstruction loss are "
                             "defined per image patch)")
        object.__setattr__(self, "patch_drop", patch_drop)
        return self

    def _draw_tokens(self, B: int):
        """(keep, slot) of this forward, or None when patch dropout is off (eval, no_grad, nothing attached, rate 0)."""
        pd = self.patch_drop
        if pd is None or not self.training or pd.rate <= 0.0 or not torch.is_grad_enabled():
            return None
        T = self._rt.grid_tokens
        keep, slot = pd.draw(B, T)
        for t, n in ((keep, None), (slot, T)):
            if (not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B
                    or (n is not None and t.shape[1] != n) or not t.is_cuda or not t.is_contiguous()):
                raise ValueError(f"PatchDropout.draw must return contiguous int32 device tensors [{B}, K] and [{B}, {T}]")
        if not 1 <= keep.shape[1] <= T:
            raise ValueError(f"PatchDropout.draw: K = {keep.shape[1]} outside 1..{T}")
        return keep, slot

    def _attn_impl(self) -> int:
        """1: the MFMA flash kernels (bf16 mode, every supported head dim: 32, 64, 128, and the PADDED_HEAD_DIMS, which
        run them at 128); 0: the scalar-FMA kernels (fp32 mode).  The fused q/k-normalise paths (GEMM epilogue, attention
        backward) are head dim 64 only; the other head dims take the unfused route (fp32 projection, qknorm_fwd, attn_fwd
        bounded, attn_bwd, qknorm_bwd; the padded dims its zero-padding twins)."""
        d = self.config.n_embd // self.config.n_head
        return 1 if (self.precision == "bf16" and d in HEAD_DIMS + PADDED_HEAD_DIMS) else 0

    def _prepare(self, device) -> None:
        if device.type != "cuda":
            raise RuntimeError("nvit_amd.ViT runs only on an MI355X (HIP device): the hot path has no CPU fallback. "
                               "Use oracle/nvit_oracle.py for CPU reference numbers.")
        self._rt.refresh(device, _dt_from_precision(self.precision))

    def _enter(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        self._prepare(x.device)
        x = x.contiguous().float()
        return x, (x if self._rt.dt == F32 else ops.cast(x, self._rt.dt))

    # ---- reference API
    def configure_optimizers(self, weight_decay: float, learning_rate: float, betas: Tuple[float, float],
                             device_type: str, *, layer_decay: Optional[float] = None) -> torch.optim.AdamW:
        """Same parameter groups as reference model.py:369-385 (three with sz in nViT mode, two without).  On the HIP
        device the optimizer is FusedAdamW (torch.optim.AdamW subclass, same state_dict); the torch class is only
        returned for a CPU-resident model, which cannot run forward anyway (no CPU path).

        layer_decay (None: exactly the groups above): layer-wise lr decay, the groups of
        `schedule.layer_decay_groups` - the same split, further split by depth, each group with lr_scale = layer_decay **
        (n_layer + 2 - depth) and lr = learning_rate * lr_scale; an attached LRSchedule applies lr_scale at every step."""
        pd = {n: p for n, p in self.named_parameters() if p.requires_grad}
        if layer_decay is not None:
            from .schedule import layer_decay_groups
            groups = layer_decay_groups(self, weight_decay, learning_rate, layer_decay)
        elif self.config.use_nvit:
            groups = [
                {"params": [p for n, p in pd.items() if "sz" not in n and p.dim() >= 2], "weight_decay": weight_decay},
                {"params": [p for n, p in pd.items() if "sz" not in n and p.dim() < 2], "weight_decay": 0.0},
                {"params": [self.sz], "weight_decay": 0.0},
            ]
        else:
            groups = [
                {"params": [p for n, p in pd.items() if p.dim() >= 2], "weight_decay": weight_decay},
                {"params": [p for n, p in pd.items() if p.dim() < 2], "weight_decay": 0.0},
            ]
        if device_type == "cuda":
            from .optim import FusedAdamW  # a torch.optim.AdamW whose step runs as nvit_adamw_renorm
            return FusedAdamW(groups, lr=learning_rate, betas=betas)
        return torch.optim.AdamW(groups, lr=learning_rate, betas=betas)

    def estimate_mfu(self, fwdbwd_per_iter: int, dt: float) -> Tuple[float, float]:
        """Reference formula (model.py:387-401): 6N + 12LHQT per token against the A100 constant 312e12."""
        cfg = self.config
        N = self.num_params
        L, H, Q = cfg.n_layer, cfg.n_head, cfg.n_embd // cfg.n_head
        T = self.n_tokens
        flops = (6 * N + 12 * L * H * Q * T) * T * fwdbwd_per_iter / dt
        return flops / 312e12, flops

    @property
    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def get_kohonen_lr(self, step: int) -> float:
        cfg = self.config
        if not cfg.kohonen_scheduler_enabled:
            return cfg.kohonen_alpha
        w, dcy = cfg.kohonen_scheduler_warmup_steps, cfg.kohonen_scheduler_decay_steps
        lo, hi = cfg.kohonen_scheduler_min_lr, cfg.kohonen_alpha
        if step < w:
            return lo + (hi - lo) * (step / w)
        if step > dcy:
            return lo
        return lo + 0.5 * (1.0 + math.cos(math.pi * (step - w) / (dcy - w))) * (hi - lo)

    # ---- Kohonen helpers (reference model.py:477-561), same names and semantics
    def combine_representations(self, local_repr: Tensor, global_repr: Tensor) -> Tensor:
        """Element-wise product, then unit L2 norm over the channel axis (reference model.py:477-480; used by its
        debug visualisation only).  The product is one multiply; the normalisation is the justnorm row kernel."""
        return justnorm(local_repr * global_repr)

    def compute_consistency_loss(self, local_repr: Tensor, global_repr: Tensor) -> Tensor:
        Cc = local_repr.shape[-1]
        return CosConsistencyFn.apply(local_repr.reshape(-1, Cc), global_repr.reshape(-1, Cc))

    def get_neighbor_indices(self, indices: Tensor) -> Tensor:
        """8-neighbourhood indices on the periodic map (index arithmetic only; the loss kernel recomputes it)."""
        nodes_per_map = self.config.kohonen_nodes // 2
        ms = int(math.sqrt(nodes_per_map))
        if ms * ms != nodes_per_map:
            raise ValueError(f"Number of nodes per map ({nodes_per_map}) must be a perfect square. "
                             f"Got {self.config.kohonen_nodes} total nodes.")
        offs = torch.tensor([[-1, -1], [-1, 0], [-1, 1], [0, -1], [0, 1], [1, -1], [1, 0], [1, 1]],
                            device=indices.device)
        row = (indices // ms).unsqueeze(-1) + offs[:, 0]
        col = (indices % ms).unsqueeze(-1) + offs[:, 1]
        return (row % ms) * ms + (col % ms)

    def compute_map_smoothness(self, indices: Tensor, neighbor_indices: Optional[Tensor] = None,
                               is_local: bool = True) -> Tensor:
        km = self.local_kohonen if is_local else self.global_kohonen
        nodes_per_map = self.config.kohonen_nodes // 2
        ms = int(math.sqrt(nodes_per_map))
        if ms * ms != nodes_per_map or km.grid_size != nodes_per_map:
            raise ValueError(f"Number of nodes per map ({nodes_per_map}) must be a perfect square. "
                             f"Got {self.config.kohonen_nodes} total nodes.")
        return MapSmoothnessFn.apply(km.nodes, indices.reshape(-1).contiguous(), ms)

    def compute_smoothness_loss(self, local_indices: Tensor, global_indices: Tensor) -> Tensor:
        return (self.compute_map_smoothness(local_indices, None, True)
                + self.compute_map_smoothness(global_indices, None, False))

    def forward(self, img: Tensor) -> Tuple[Tensor, Dict[str, Tensor]]:
        """(logits, aux).  Under torch.no_grad / inference_mode the block functions take their forward-only route (see
        _lean()): the same logits and aux values bit for bit, without the stores and tensors only a backward reads.
        A training forward that drops patches (attach_patch_drop) does not evaluate the reconstruction head - its target
        is every image patch - and its aux has no "reconstruction" entry; without the Kohonen head, which patch dropout
        excludes, the loss never reads it (train.add_aux_losses)."""
        return self._forward(img, True)

    def _forward(self, img: Tensor, want_recon: bool) -> Tuple[Tensor, Dict[str, Tensor]]:
        """forward(); want_recon False (evaluate.predict) leaves the reconstruction head and aux["reconstruction"] out."""
        grid = self._running_grid(img)
        if self.training:
            self.step += 1
        self._prepare(img.device)
        rt = self._rt
        rt.tokens, rt.grid = None, grid
        try:
            return self._forward_body(img, want_recon)
        finally:
            # a dropping forward's K and another image size's grid are not left behind for stand-alone block calls
            rt.tokens, rt.grid = None, None

    def _forward_body(self, img: Tensor, want_recon: bool) -> Tuple[Tensor, Dict[str, Tensor]]:
        rt = self._rt
        if rt.carry is not None:
            # a chained backward stopped before the node that was to consume the pending q/k/v data gradient (autograd.grad
            # up to a block input, an exception inside backward): the gradients it did return were incomplete
            rt.carry = None
            raise RuntimeError("nvit_amd: the previous backward through ViT.forward stopped inside the block chain; in the "
                               "chained bf16 mode gradients at block inputs are incomplete there - use the fp32 mode to "
                               "differentiate up to an intermediate block input")
        cfg = self.config
        B = img.shape[0]
        T, C = rt.grid_tokens, cfg.n_embd
        img = img.contiguous().float()
        posl, posg = self.local_pos_embed, self.global_pos_embed
        if rt.grid is not None:   # another image size: the tables at this forward's grid, differentiable
            posl, posg = _PosResampleFn.apply(resample.grid_of(self.n_tokens), rt.grid, posl, posg)
        loc, glo, loc_lo, glo_lo = _EmbedFn.apply(img, rt, self.local_patch_embed.weight, self.local_patch_embed.bias,
                                                  posl, self.global_patch_embed[1].weight,
                                                  self.global_patch_embed[1].bias, posg)
        if loc_lo.numel() == 0:   # fp32 mode (or an embedding width the twin store does not cover): no bf16 copies
            loc_lo = glo_lo = None
        drawn = self._draw_tokens(B)
        if drawn is not None:
            keep, slot = drawn
            loc, glo, loc_k_lo, glo_k_lo = _TokenDropFn.apply(loc, glo, keep, slot, loc_lo is not None)
            if loc_lo is not None:
                loc_lo, glo_lo = loc_k_lo, glo_k_lo
            rt.tokens = keep.shape[1]   # everything behind the gather runs on K tokens per sample
            want_recon = False
        aux: Dict[str, Tensor] = {}
        if not cfg.use_nvit:
            return self._forward_std(img, loc, glo, aux, want_recon)
        if cfg.use_kohonen:
            # reference model.py:419-444
            lr = self.get_kohonen_lr(self.step)
            loc3, glo3 = loc.reshape(B, T, C), glo.reshape(B, T, C)
            local_repr, local_idx = self.local_kohonen(loc3)
            global_repr, global_idx = self.global_kohonen(glo3)
            if self.training:
                self.local_kohonen.update_nodes(loc3, local_idx, lr)
                self.global_kohonen.update_nodes(glo3, global_idx, lr)
                if self._node_sync is not None:   # data parallel: keep the SOM replicas identical
                    self._node_sync(self.local_kohonen.nodes.data, self.global_kohonen.nodes.data)
            lrep2, grep2 = local_repr.reshape(B * T, C), global_repr.reshape(B * T, C)
            local_new, _ = self.cross_attention._run(lrep2, loc, None, loc_lo)
            global_new, _ = self.cross_attention._run(grep2, glo, None, glo_lo)
            aux["kohonen_consistency"] = self.compute_consistency_loss(local_repr, global_repr)
            aux["kohonen_smoothness"] = self.compute_smoothness_loss(local_idx, global_idx)
            aux["local_quantization"] = HuberFn.apply(lrep2, loc)
            aux["global_quantization"] = HuberFn.apply(grep2, glo)
            x, x_lo = self.cross_attention._run(local_new, global_new, chained=True)
            if self._taps is not None:
                self._taps["lidx"], self._taps["gidx"] = local_idx.detach(), global_idx.detach()
        else:
            x, x_lo = self.cross_attention._run(loc, glo, loc_lo, glo_lo, chained=True)
        taps = self._taps
        if taps is not None:
            taps["loc"], taps["glo"], taps["x0"] = loc.detach(), glo.detach(), x.detach()
        table = self._draw_gates(B) if len(self.transformer.h) else None
        for i, blk in enumerate(self.transformer.h):
            x, x_lo = blk._run(x, x_lo, True, chained=True,
                               gates=None if table is None else (table[2 * i], table[2 * i + 1]))
            if taps is not None:
                taps[f"x{i + 1}"] = x.detach()
        logits = _HeadFn.apply(x, rt, self.mlp_head[0].weight, self.mlp_head[0].bias, self.mlp_head[1].weight,
                               self.mlp_head[1].bias, self.sz)
        if want_recon:
            aux["reconstruction"] = _ReconFn.apply(x, x_lo, rt, img, self.reconstruction_head[0].weight,
                                                   self.reconstruction_head[0].bias)
        return logits, aux

    def _forward_std(self, img: Tensor, loc: Tensor, glo: Tensor, aux: Dict[str, Tensor], want_recon: bool = True):
        """Plain-ViT remainder of forward (use_nvit=False, reference model.py:446-470 without the Kohonen head)."""
        rt = self._rt
        x, _ = self.cross_attention._run(loc, glo)
        taps = self._taps
        if taps is not None:
            taps["loc"], taps["glo"], taps["x0"] = loc.detach(), glo.detach(), x.detach()
        blocks = self.transformer.h
        x_lo = _lo(rt, x, ops.cast(x, rt.dt) if rt.dt != F32 else None) if len(blocks) == 0 else None
        table = self._draw_gates(x.shape[0] // rt.n_tokens) if len(blocks) else None
        for i, blk in enumerate(blocks):
            x, x_lo = blk._run(x, None, True, want_lo=(want_recon and i == len(blocks) - 1),
                               gates=None if table is None else (table[2 * i], table[2 * i + 1]))
            if taps is not None:
                taps[f"x{i + 1}"] = x.detach()
        logits = _HeadFn.apply(x, rt, self.mlp_head[0].weight, self.mlp_head[0].bias, self.mlp_head[1].weight,
                               self.mlp_head[1].bias, None)
        if want_recon:
            aux["reconstruction"] = _ReconFn.apply(x, x_lo, rt, img, self.reconstruction_head[0].weight,
                                                   self.reconstruction_head[0].bias)
        return logits, aux
