"""Plain-ViT baseline (use_nvit=False) as a short torch restatement, for tests: reference model.py:92-169 (Block with the
RMSNorm modules built), :219-275 (CrossAttentionBlock), :404-470 (ViT.forward without the Kohonen head).
Runs on the CPU in any dtype (float64 for the oracle role).  tests/test_vit_baseline_config.py holds it to the numbers
recorded from the reference itself (tests/golden/vit_*.npz), so the GPU tests may use it where no recording exists
(other head dims, bias on / off)."""
import math

import torch
import torch.nn.functional as F


def forward(sd, cfg, X):
    """sd: state_dict-like mapping name -> tensor; X [B,ch,S,S].  -> (logits [B, classes], reconstruction loss)."""
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
    loc = loc.flatten(2).transpose(1, 2) + sd["local_pos_embed"]
    glo = glo.flatten(2).transpose(1, 2) + sd["global_pos_embed"]
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
    logits = F.linear(F.layer_norm(pooled, (C,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], 1e-5),
                      sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
    rec = torch.tanh(lin(x, "reconstruction_head.0"))
    target = X.unfold(2, Pl, Pl).unfold(3, Pl, Pl).permute(0, 2, 3, 1, 4, 5).reshape(rec.shape)
    return logits, F.mse_loss(rec, target)


def loss_and_grads(sd32, cfg, X, y, dtype=torch.float64):
    """Forward + cross-entropy backward in `dtype`; -> logits, loss, recon, {name: grad}."""
    sd = {n: t.detach().to(dtype).requires_grad_(True) for n, t in sd32.items()}
    logits, recon = forward(sd, cfg, X.to(dtype))
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {n: t.grad for n, t in sd.items() if t.grad is not None}
    return logits.detach(), loss.detach(), recon.detach(), grads
