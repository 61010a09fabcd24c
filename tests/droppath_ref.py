"""Oracles of the stochastic-depth tests (a plain helper module: test_droppath_api.py uses it on the CPU,
test_gpu_droppath_ops.py and test_gpu_droppath.py against the HIP kernels).

* `draw`: the numpy twin of nvit_droppath_draw (augment.hip), integer Philox and fp32 arithmetic, so the device table must
  equal it bit for bit.
* `gated_lerp_eval` / `gated_lerp_formula` / `gated_lerp_bounds`: rowops_check's LERP reference, step formula and fp64
  element bounds with the row's gate folded into the step sizes (lam_row = gate * |alpha c_a|: the one extra multiply);
  with every gate 1 they are rowops_check's own.
* `gated_res_rmsnorm_*` / `gated_res_skip_*`: the same for the plain-ViT residual kernels, the gate folded into y
  (z = a + gate * y, h + gate * y), with the gradient of y (`dy`: gate times the gradient of the sum) as an extra output.
* `gated_vit_loss_and_grads`: vit_torch_ref.py's plain-ViT forward with every residual add of the block chain gated.
* `gated_oracle`: runs oracle.nvit_oracle with `lerp` replaced by the gated form, the gate picked by the identity of the
  alpha tensor a block passes in (the cross-attention's alpha maps to no gate).
"""
from __future__ import annotations

import contextlib
from typing import Dict

import numpy as np
import torch

import rowops_check as rc
from mix_ref import M32, philox_vec
from oracle import nvit_oracle as O

DOMAIN = 0x44525054   # xor-ed, plus the table row, into the key's high word


# ------------------------------------------------------------------------------------------------ the draw
def rates(rate: float, n_layer: int) -> np.ndarray:
    """timm's linspace(0, rate, depth) in fp32; one layer never drops"""
    if n_layer == 1:
        return np.zeros(1, dtype=np.float32)
    return np.linspace(0.0, rate, n_layer).astype(np.float32)


def draw(seed: int, step: int, first_index: int, rate: float, n_layer: int, B: int, scale_by_keep: bool) -> np.ndarray:
    """What nvit_droppath_draw writes: float32 [2*n_layer, B]."""
    p = rates(rate, n_layer)
    g = np.array([first_index + b for b in range(B)], dtype=np.uint64)
    n = np.ones(B, dtype=np.uint64)
    table = np.zeros((2 * n_layer, B), dtype=np.float32)
    for row in range(2 * n_layer):
        k1 = ((seed >> 32) & 0xFFFFFFFF) ^ ((DOMAIN + row) & 0xFFFFFFFF)
        r0 = philox_vec(g & M32, g >> np.uint64(32), n * np.uint64(step & 0xFFFFFFFF), n * np.uint64(step >> 32),
                        seed & 0xFFFFFFFF, k1)[0]
        keep = np.float32(1.0) - p[row >> 1]
        kept = (r0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) < keep
        value = np.float32(1.0) / keep if scale_by_keep else np.float32(1.0)
        table[row] = np.where(kept, value, np.float32(0.0))
    return table


# ------------------------------------------------------------------------------------------------ gated LERP
def gate_rows(gate: torch.Tensor, T: int) -> torch.Tensor:
    """[B] gates -> [B*T, 1]: rows b*T .. b*T+T-1 belong to sample b"""
    return gate.repeat_interleave(T).reshape(-1, 1)


def gated_lerp_eval(d: Dict, gate: torch.Tensor, T: int, dtype=rc.F64) -> Dict[str, torch.Tensor]:
    """rc.lerp_eval with out = nrm(a + (gate * |alpha c_a|) (b - a)); gradients by autograd of that forward."""
    M, C = d["h"].shape
    g_ = gate_rows(gate, T).to(dtype)
    h, y, al = rc._leaf(d["h"], dtype), rc._leaf(d["y"], dtype), rc._leaf(d["alpha"].expand(M, C), dtype)
    a, b = O.nrm(h), O.nrm(y)
    out = O.nrm(a + (g_ * torch.abs(al * d["c_a"])) * (b - a))
    leaves = [h, y, al]
    if d["skip_x"] is not None:
        xs, sk = rc._leaf(d["skip_x"], dtype), rc._leaf(d["skip"].expand(M, 1), dtype)
        out = O.nrm(out * sk + xs)
        leaves += [xs, sk]
    res = {"out": out.detach()}
    if d.get("dout") is None:
        return res
    g = d["dout"].to(dtype)
    if d["dout_add"] is not None:
        g = g + d["dout_add"].to(dtype)
    gr = torch.autograd.grad(out, leaves, g)
    res.update(dh=gr[0] if d["old"] is None else gr[0] + d["old"].to(dtype), dy=gr[1], dalpha_rows=gr[2],
               dalpha=gr[2].sum(0))
    if d["skip_x"] is not None:
        res.update(dskip_x=gr[3], dskip_rows=gr[4], dskip=gr[4].sum().reshape(1))
    return res


def gated_lerp_formula(d: Dict, gate: torch.Tensor, T: int, dtype) -> Dict:
    """rc.lerp_formula with the row's step sizes lam_row = gate * lam and the row's d(lam) term carrying the gate."""
    h, y, alpha, xs, skip, g, add, old = (rc._as(d[k], dtype) for k in
                                          ("h", "y", "alpha", "skip_x", "skip", "dout", "dout_add", "old"))
    gt = rc._as(gate_rows(gate, T), dtype)   # exact fp32 inputs
    c_a = d["c_a"]
    lam = rc._abs(alpha * c_a) * gt          # the extra multiply
    a, rsx = rc._nrm(h)
    b, rsy = rc._nrm(y)
    o, rsr = rc._nrm(a + lam * (b - a))
    res = {"out": o}
    if xs is not None:
        t, rst = rc._nrm(o * skip + xs)
        res["out"] = t
    if g is None:
        return res
    if add is not None:
        g = g + add
    if xs is not None:
        dt_ = (g - t * rc._sum(t * g)) * rst
        res["dskip_x"] = dt_
        res["dskip_rows"] = rc._sum(dt_ * o)
        res["dskip"] = rc._flat(rc._sum(res["dskip_rows"], 0))
        g = dt_ * skip
    dr = (g - o * rc._sum(o * g)) * rsr
    res["dlam_rows"] = (dr * gt) * (b - a)
    sign = torch.sign(d["alpha"].double() * c_a)
    res["dalpha"] = rc._flat(rc._sum(res["dlam_rows"], 0) * c_a) * (rc.Ev(sign) if dtype == "ev" else sign.to(dtype))
    db = lam * dr
    dh = ((dr - db) - a * rc._sum(a * (dr - db))) * rsx
    res["dh"] = dh if old is None else dh + old
    res["dy"] = (db - b * rc._sum(b * db)) * rsy
    return res


def gated_lerp_bounds(d: Dict, gate: torch.Tensor, T: int):
    """(values, bounds) of the Ev run, as rc.lerp_bounds"""
    return rc._split(rc._pick(gated_lerp_formula(d, gate, T, "ev"), rc.LERP_OUT))


# ------------------------------------------------------------------------------------------------ gated residual kernels
def gated_res_rmsnorm_eval(d: Dict, gate: torch.Tensor, T: int, dtype=rc.F64) -> Dict[str, torch.Tensor]:
    """rc.res_rmsnorm_eval with z = a + gate * y.  dz = d(z) (+ old); dy = autograd's d(y) (+ gate * old: the kernel's
    low-precision output is gate * the dz it stores)."""
    M, C = d["h"].shape
    g_ = gate_rows(gate, T).to(dtype)
    a, y, w = rc._leaf(d["h"], dtype), rc._leaf(d["y"], dtype), rc._leaf(d["w"].expand(M, C), dtype)
    z = a + g_ * y
    rstd = torch.rsqrt((z * z).mean(dim=-1, keepdim=True) + d["eps"])
    out = z * rstd * w
    g = d["dout"].to(dtype)
    if d["dout_add"] is not None:
        g = g + d["dout_add"].to(dtype)
    gr = torch.autograd.grad(out, [a, y, w], g)
    old = 0 if d["old"] is None else d["old"].to(dtype)
    return {"out": out.detach(), "rstd": rstd.detach().reshape(M), "dz": gr[0] + old, "dy": gr[1] + g_ * old,
            "dw_rows": gr[2], "dw": gr[2].sum(0)}


def gated_res_rmsnorm_formula(d: Dict, gate: torch.Tensor, T: int, dtype) -> Dict:
    a, y, w, g, add, old = (rc._as(d[k], dtype) for k in ("h", "y", "w", "dout", "dout_add", "old"))
    gt = rc._as(gate_rows(gate, T), dtype)
    C = d["h"].shape[1]
    z = a + y * gt                             # the extra multiply
    rs = rc._rsqrt(rc._divc(rc._sum(z * z), C) + d["eps"])
    res = {"out": z * rs * w, "rstd": rc._flat(rs)}
    if add is not None:
        g = g + add
    zn = z * rs
    res["dw_rows"] = g * zn
    res["dw"] = rc._flat(rc._sum(res["dw_rows"], 0))
    gw = g * w
    dz = (gw - zn * rc._divc(rc._sum(gw * zn), C)) * rs
    res["dz"] = dz if old is None else dz + old
    res["dy"] = res["dz"] * gt                 # and one at the low-precision copy
    return res


GATED_RMS_OUT = rc.RMS_OUT + ("dy",)


def gated_res_rmsnorm_bounds(d: Dict, gate: torch.Tensor, T: int):
    return rc._split(rc._pick(gated_res_rmsnorm_formula(d, gate, T, "ev"), GATED_RMS_OUT))


def gated_res_skip_eval(d: Dict, gate: torch.Tensor, T: int, dtype=rc.F64) -> Dict[str, torch.Tensor]:
    """rc.res_skip_eval with out = nrm((h + gate * y) * skip + x); dh = d(h), dy = d(y)."""
    M, C = d["h"].shape
    g_ = gate_rows(gate, T).to(dtype)
    h, y, x = rc._leaf(d["h"], dtype), rc._leaf(d["y"], dtype), rc._leaf(d["x"], dtype)
    sk = rc._leaf(d["skip1"].expand(M, 1), dtype)
    out = O.nrm((h + g_ * y) * sk + x)
    gr = torch.autograd.grad(out, [h, y, x, sk], d["dout"].to(dtype))
    return {"out": out.detach(), "dh": gr[0], "dy": gr[1], "dx": gr[2], "dskip_rows": gr[3],
            "dskip": gr[3].sum().reshape(1)}


def gated_res_skip_formula(d: Dict, gate: torch.Tensor, T: int, dtype) -> Dict:
    h, y, x, skip, g = (rc._as(d[k], dtype) for k in ("h", "y", "x", "skip1", "dout"))
    gt = rc._as(gate_rows(gate, T), dtype)
    s = h + y * gt
    o, rs = rc._nrm(s * skip + x)
    dr = (g - o * rc._sum(o * g)) * rs
    res = {"out": o, "dx": dr, "dh": dr * skip, "dskip_rows": rc._sum(dr * s)}
    res["dy"] = res["dh"] * gt
    res["dskip"] = rc._flat(rc._sum(res["dskip_rows"], 0))
    return res


GATED_RES_SKIP_OUT = rc.RES_SKIP_OUT + ("dy",)


def gated_res_skip_bounds(d: Dict, gate: torch.Tensor, T: int):
    return rc._split(rc._pick(gated_res_skip_formula(d, gate, T, "ev"), GATED_RES_SKIP_OUT))


def within(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], bound: Dict[str, torch.Tensor]) -> Dict[str, bool]:
    """per output: does every element lie inside its bound (rc.check's comparison, without the assertion)"""
    res = {}
    for k in bound:
        out, r = got[k].detach().cpu(), ref[k].detach().to(rc.F64)
        b = bound[k].expand(r.shape)
        if out.dtype == torch.bfloat16:
            from kohonen_check import half_ulp_bf16
            b = b + half_ulp_bf16(r.abs() + b)
        res[k] = bool(((out.double().reshape(r.shape) - r).abs() <= b).all())
    return res


# ------------------------------------------------------------------------------------------------ the gated oracle
@contextlib.contextmanager
def gated_oracle(p: Dict[str, torch.Tensor], table: torch.Tensor):
    """Inside, oracle.nvit_oracle.lerp is the gated form: a call whose alpha IS p["transformer.h.{l}.attn_alpha"] takes
    row 2*l of `table` [2*n_layer, B], ...mlp_alpha row 2*l + 1, any other alpha (the cross-attention's) no gate."""
    by_alpha = {}
    for l in range(table.shape[0] // 2):
        by_alpha[id(p[f"transformer.h.{l}.attn_alpha"])] = table[2 * l]
        by_alpha[id(p[f"transformer.h.{l}.mlp_alpha"])] = table[2 * l + 1]
    plain = O.lerp

    def lerp(h, y, alpha, c_a):
        gate = by_alpha.get(id(alpha))
        if gate is None:
            return plain(h, y, alpha, c_a)
        B = gate.shape[0]
        g_ = gate.to(h.dtype).reshape(B, *([1] * (h.dim() - 1))) if h.shape[0] == B else \
            gate_rows(gate, h.shape[0] // B).to(h.dtype)
        a, b = O.nrm(h), O.nrm(y)
        return O.nrm(a + (g_ * torch.abs(alpha * c_a)) * (b - a))

    O.lerp = lerp
    try:
        yield
    finally:
        O.lerp = plain


# ------------------------------------------------------------------------------------------------ the gated plain ViT
def gated_vit_forward(sd, cfg, X, table):
    """vit_torch_ref.forward (the plain ViT, use_nvit=False) with h1 = a + g[2l] * attn(..) and h2 = bm + g[2l+1] * mlp(..)
    in block l, g = table [2*n_layer, B] broadcast over a sample's tokens; everything else as there."""
    import math
    import torch.nn.functional as F
    C, H = cfg.n_embd, cfg.n_head
    d = C // H
    Pl, Pg = cfg.local_patch_size, cfg.global_patch_size
    table = table.to(X.dtype)

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
        g_att, g_mlp = table[2 * i].reshape(-1, 1, 1), table[2 * i + 1].reshape(-1, 1, 1)
        a = rms(x, sd[p + "rmsnorm_att.weight"])
        h1 = a + g_att * lin(attn(lin(a, p + "query"), lin(a, p + "key"), lin(a, p + "value")), p + "att_c_proj")
        bm = rms(h1, sd[p + "rmsnorm_mlp.weight"])
        u, v = lin(bm, p + "c_fc").chunk(2, dim=-1)
        h2 = bm + g_mlp * lin(u * F.silu(v), p + "mlp_c_proj")
        r = h2 * sd[p + "skip_param"] + x
        x = r / r.norm(p=2, dim=-1, keepdim=True)
    pooled = x.mean(dim=1)
    logits = F.linear(F.layer_norm(pooled, (C,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], 1e-5),
                      sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
    return logits


def gated_vit_loss_and_grads(sd32, cfg, X, y, table, dtype=torch.float64):
    """Forward + cross-entropy backward in `dtype`; -> logits, loss, {name: grad} (vit_torch_ref.loss_and_grads)."""
    import torch.nn.functional as F
    sd = {n: t.detach().to(dtype).requires_grad_(True) for n, t in sd32.items()}
    logits = gated_vit_forward(sd, cfg, X.to(dtype), table)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {n: t.grad for n, t in sd.items() if t.grad is not None}
