"""Oracles of the patch-dropout tests (a plain helper module: test_patchdrop_api.py uses it on the CPU,
test_gpu_patchdrop_ops.py and test_gpu_patchdrop.py against the HIP kernels).

* `words` / `draw`: the numpy twin of nvit_patchdrop_draw (patchdrop.hip), integer Philox and an integer sort, so the device
  tables must equal it bit for bit.
* `dropped_forward` / `dropped_loss_and_grads`: the nViT forward restated from the unchanged oracle's own pieces
  (oracle.nvit_oracle: embed, cross_block, block, layer_norm, linear) with a torch.gather of the kept tokens between embed
  and cross_block and the mean-pool over the K kept tokens, in fp64 by default.
* `dropped_vit_forward` / `dropped_vit_loss_and_grads`: the same for the plain ViT, vit_torch_ref.forward's body with the
  gather behind the position embeddings (its reconstruction head left out, as in the model).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from mix_ref import M32, philox_vec
from oracle import nvit_oracle as O

DOMAIN = 0x50445250   # plus the token's group t >> 2, xor-ed into the key's high word
MAX_TOKENS = 4096


# ------------------------------------------------------------------------------------------------ the draw
def num_keep(T: int, rate: float) -> int:
    """timm's PatchDropout: max(1, int(L * (1. - prob)))"""
    return max(1, int(T * (1.0 - rate)))


def words(seed: int, step: int, first_index: int, B: int, T: int) -> np.ndarray:
    """uint64 [B, T]: the 24-bit word u of every token, u = r >> 8, r = word t & 3 of the Philox call with counter
    (first_index + b, step) and key (seed low, seed high ^ (DOMAIN + (t >> 2)))."""
    g = np.array([first_index + b for b in range(B)], dtype=np.uint64)
    n = np.ones(B, dtype=np.uint64)
    u = np.zeros((B, (T + 3) // 4 * 4), dtype=np.uint64)
    for q in range((T + 3) // 4):
        k1 = ((seed >> 32) & 0xFFFFFFFF) ^ ((DOMAIN + q) & 0xFFFFFFFF)
        r = philox_vec(g & M32, g >> np.uint64(32), n * np.uint64(step & 0xFFFFFFFF), n * np.uint64(step >> 32),
                       seed & 0xFFFFFFFF, k1)
        for w in range(4):
            u[:, 4 * q + w] = r[w] >> np.uint64(8)
    return u[:, :T]


def draw(seed: int, step: int, first_index: int, B: int, T: int, K: int):
    """What nvit_patchdrop_draw writes: keep int32 [B, K] (ascending), slot int32 [B, T].  Kept: the K tokens with the
    smallest (u << 32) | t."""
    assert 1 <= K <= T <= MAX_TOKENS and B >= 1
    key = (words(seed, step, first_index, B, T) << np.uint64(32)) | np.arange(T, dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")     # (the keys are distinct: any sort gives this order)
    keep = np.sort(order[:, :K], axis=1).astype(np.int32)
    slot = np.full((B, T), -1, dtype=np.int32)
    np.put_along_axis(slot, keep.astype(np.int64), np.arange(K, dtype=np.int32)[None, :].repeat(B, 0), axis=1)
    return keep, slot


def slot_of(keep: torch.Tensor, T: int) -> torch.Tensor:
    """int32 [B, T] inverse of a keep table [B, K]"""
    B, K = keep.shape
    slot = torch.full((B, T), -1, dtype=torch.int32)
    slot.scatter_(1, keep.long(), torch.arange(K, dtype=torch.int32)[None, :].expand(B, K).contiguous())
    return slot


def take(x: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """[B, T, C] -> [B, K, C]: the kept tokens of every sample"""
    return torch.gather(x, 1, keep.long()[:, :, None].expand(-1, -1, x.shape[-1]))


# ------------------------------------------------------------------------------------------------ nViT
def dropped_forward(p, cfg, img, keep, lowp=None):
    """oracle.nvit_oracle.forward (no Kohonen head) on the kept tokens: logits [B, ncls]"""
    assert cfg.use_nvit and not cfg.use_kohonen
    loc, glo, _ = O.embed(p, cfg, img, lowp)
    loc, glo = take(loc, keep), take(glo, keep)
    x = O.cross_block(p, cfg, loc, glo, lowp)
    for i in range(cfg.n_layer):
        x = O.block(p, cfg, i, x, lowp)
    pooled = x.mean(dim=1)   # over the K kept tokens
    ln = O.layer_norm(pooled, p["mlp_head.0.weight"], p["mlp_head.0.bias"])
    logits = O.linear(ln, p["mlp_head.1.weight"], p["mlp_head.1.bias"], None)
    return logits * (p["sz"] * (cfg.sz_init_value / cfg.sz_init_scaling))


def dropped_loss_and_grads(state, cfg, X, y, keep, dtype=torch.float64, renormed=False):
    """-> params (with .grad), logits, loss: forward + cross-entropy backward in `dtype` of the formula weights `state`"""
    p = {n: t.detach().clone().to(dtype).requires_grad_(True) for n, t in state.items() if t.is_floating_point()}
    if renormed:
        O.renorm_(p, cfg)
    logits = dropped_forward(p, cfg, X.to(dtype), keep)
    loss = O.cross_entropy(logits, y)
    loss.backward()
    return p, logits.detach(), loss.detach()


# ------------------------------------------------------------------------------------------------ the plain ViT
def dropped_vit_forward(sd, cfg, X, keep):
    """vit_torch_ref.forward (use_nvit=False) with the kept tokens gathered behind the position embeddings"""
    C, H = cfg.n_embd, cfg.n_head
    d = C // H
    Pl, Pg = cfg.local_patch_size, cfg.global_patch_size

    def lin(x, n):
        return F.linear(x, sd[n + ".weight"], sd.get(n + ".bias"))

    def rms(x, w):
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w

    def attn(q, k, v):
        B, T, _ = q.shape
        heads = lambda t: t.reshape(B, T, H, d).transpose(1, 2)
        p = (heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(d)).softmax(-1)
        return (p @ heads(v)).transpose(1, 2).reshape(B, T, C)

    loc = F.conv2d(X, sd["local_patch_embed.weight"], sd["local_patch_embed.bias"], stride=Pl)
    pad = (Pg - Pl) // 2
    glo = F.conv2d(F.pad(X, (pad,) * 4, mode="reflect"), sd["global_patch_embed.1.weight"],
                   sd["global_patch_embed.1.bias"], stride=Pl)
    loc = take(loc.flatten(2).transpose(1, 2) + sd["local_pos_embed"], keep)
    glo = take(glo.flatten(2).transpose(1, 2) + sd["global_pos_embed"], keep)
    p = "cross_attention."
    ln, gn = rms(loc, sd[p + "local_norm.weight"]), rms(glo, sd[p + "global_norm.weight"])
    o = attn(lin(ln, p + "q_local"), lin(gn, p + "k_global"), lin(gn, p + "v_global"))
    u, v = lin(o, p + "proj").chunk(2, dim=-1)
    x = lin(u * F.silu(v), p + "out_proj")
    for i in range(cfg.n_layer):
        p = f"transformer.h.{i}."
        a = rms(x, sd[p + "rmsnorm_att.weight"])
        h1 = a + lin(attn(lin(a, p + "query"), lin(a, p + "key"), lin(a, p + "value")), p + "att_c_proj")
        bm = rms(h1, sd[p + "rmsnorm_mlp.weight"])
        u, v = lin(bm, p + "c_fc").chunk(2, dim=-1)
        h2 = bm + lin(u * F.silu(v), p + "mlp_c_proj")
        r = h2 * sd[p + "skip_param"] + x
        x = r / r.norm(p=2, dim=-1, keepdim=True)
    pooled = x.mean(dim=1)
    return F.linear(F.layer_norm(pooled, (C,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], 1e-5),
                    sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])


def dropped_vit_loss_and_grads(sd32, cfg, X, y, keep, dtype=torch.float64):
    """-> logits, loss, {name: grad} (vit_torch_ref.loss_and_grads without the reconstruction)"""
    sd = {n: t.detach().to(dtype).requires_grad_(True) for n, t in sd32.items() if t.is_floating_point()}
    logits = dropped_vit_forward(sd, cfg, X.to(dtype), keep)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {n: t.grad for n, t in sd.items() if t.grad is not None}
