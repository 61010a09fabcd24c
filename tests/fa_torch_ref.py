"""Head-axis attention (flash_attn=True) as a short torch restatement, for tests.

The reference calls flash_attn_func on [B, H, T, d] tensors, which flash-attn reads as [batch, seqlen, nheads, headdim]
(model.py:121-122, 252-253): for every token, the softmax runs over the H heads,
    out[b, t, i, :] = sum_j softmax_j(scale * <q~[b,t,i,:], k~[b,t,j,:]>) v[b,t,j,:].
nViT: the CPU oracle (oracle/nvit_oracle.py) with its `attend` swapped for this form (q~ = sqk * nrm(q), scale sqrt(d)).
Plain ViT: tests/vit_torch_ref.py's forward with the same swap (q~ = q, scale 1/sqrt(d)).
tests/test_flash_attn_config.py holds both to the numbers recorded from the reference itself (tests/golden/fa_*.npz), so
the GPU tests may use them where no recording exists.  Runs on the CPU in any dtype."""
import contextlib
import math
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import nvit_oracle as O


def heads_attention(q, k, v, scale):
    """q, k, v [..., H, d] (token-major: one token's heads on the second-to-last axis) -> softmax over the heads."""
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)
    return torch.matmul(p, v)


def attend(q, k, v, s_eff, H, lowp=None):
    """Drop-in for oracle.attend: q, k, v [B, T, C] -> [B, T, C]; q~ = s_eff * nrm(q_head) (fp32 / fp64 only)."""
    assert lowp is None
    B, T, C = q.shape
    d = C // H
    s = s_eff.reshape(H, d)
    sp = lambda t: t.reshape(B, T, H, d)
    return heads_attention(s * O.nrm(sp(q)), s * O.nrm(sp(k)), sp(v), math.sqrt(d)).reshape(B, T, C)


@contextlib.contextmanager
def nvit_flash():
    """Within the context the CPU oracle computes the flash_attn=True model."""
    with mock.patch.object(O, "attend", attend):
        yield


def _plain_attn(q, k, v, H):
    B, T, C = q.shape
    d = C // H
    sp = lambda t: t.reshape(B, T, H, d)
    return heads_attention(sp(q), sp(k), sp(v), 1.0 / math.sqrt(d)).reshape(B, T, C)


def vit_forward(sd, cfg, X):
    """Plain ViT with flash_attn=True: vit_torch_ref.forward (which defines its token attention inline) restated with
    the head-axis attention."""
    H, C = cfg.n_head, cfg.n_embd
    Pl, Pg = cfg.local_patch_size, cfg.global_patch_size

    def lin(x, n):
        return F.linear(x, sd[n + ".weight"], sd.get(n + ".bias"))

    def rms(x, w):
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w

    loc = F.conv2d(X, sd["local_patch_embed.weight"], sd["local_patch_embed.bias"], stride=Pl)
    pad = (Pg - Pl) // 2
    glo = F.conv2d(F.pad(X, (pad,) * 4, mode="reflect"), sd["global_patch_embed.1.weight"],
                   sd["global_patch_embed.1.bias"], stride=Pl)
    loc = loc.flatten(2).transpose(1, 2) + sd["local_pos_embed"]
    glo = glo.flatten(2).transpose(1, 2) + sd["global_pos_embed"]
    p = "cross_attention."
    ln, gn = rms(loc, sd[p + "local_norm.weight"]), rms(glo, sd[p + "global_norm.weight"])
    o = _plain_attn(lin(ln, p + "q_local"), lin(gn, p + "k_global"), lin(gn, p + "v_global"), H)
    u, v = lin(o, p + "proj").chunk(2, dim=-1)
    x = lin(u * F.silu(v), p + "out_proj")
    for i in range(cfg.n_layer):
        p = f"transformer.h.{i}."
        a = rms(x, sd[p + "rmsnorm_att.weight"])
        h1 = a + lin(_plain_attn(lin(a, p + "query"), lin(a, p + "key"), lin(a, p + "value"), H), p + "att_c_proj")
        bm = rms(h1, sd[p + "rmsnorm_mlp.weight"])
        u, v = lin(bm, p + "c_fc").chunk(2, dim=-1)
        h2 = bm + lin(u * F.silu(v), p + "mlp_c_proj")
        r = h2 * sd[p + "skip_param"] + x
        x = r / r.norm(p=2, dim=-1, keepdim=True)
    pooled = x.mean(dim=1)
    logits = F.linear(F.layer_norm(pooled, (C,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], 1e-5),
                      sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
    rec = torch.tanh(lin(x, "reconstruction_head.0"))
    target = X.unfold(2, Pl, Pl).unfold(3, Pl, Pl).permute(0, 2, 3, 1, 4, 5).reshape(rec.shape)
    return logits, F.mse_loss(rec, target)


def vit_loss_and_grads(sd32, cfg, X, y, dtype=torch.float64):
    """Plain ViT, flash_attn=True: forward + cross-entropy backward in `dtype`; -> logits, loss, recon, {name: grad}."""
    sd = {n: t.detach().to(dtype).requires_grad_(True) for n, t in sd32.items()}
    logits, recon = vit_forward(sd, cfg, X.to(dtype))
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {n: t.grad for n, t in sd.items() if t.grad is not None}
    return logits.detach(), loss.detach(), recon.detach(), grads
