"""Oracles of the input-end kernel tests: nvit_patch_embed_fwd (patch_embed.hip), nvit_im2col (misc.hip) and
nvit_shadow_weights (weights.hip).  A plain helper module; test_patch_check.py checks it on the CPU,
test_gpu_patch_bounds.py uses it against the HIP kernels.

Gather (`patches`), from its definition: token m = b T + ty G + tx (G = S / Pl, T = G G) takes, for patch element
k = (c P + ph) P + pw, the pixel img[b, c, R(ty Pl - pad + ph), R(tx Pl - pad + pw)], pad = (P - Pl) / 2, where R is the
reflection that does not repeat the edge pixel: R(i) = |i|, then 2 (S - 1) - i where that is >= S.

Patch embedding.  The kernel splits every pixel and weight into bf16 halves hi = bf16(x), lo = bf16(x - hi) (`split`; x
- hi is exact in fp32) and multiplies hi hi + lo hi + hi lo on the MFMA with fp32 accumulation, then adds bias and
pos[m % T].  Two references:

* ref_split = fp64 of ah.wh + al.wh + ah.wl + bias + pos[m % T]: what the kernel computes, with exact arithmetic.
  The kernel is held to it per element:
      bound = red(3 K, mag) + 2 u (mag + |bias| + |pos|),     mag = sum_k |ah wh| + |al wh| + |ah wl|
  red(n, mag) = LAMBDA sqrt(n) u mag for the fp32 sum of the 3 K products (exact in fp32: 8 x 8 significant bits), in
  whatever order the MFMA and the stage loop take them; the two epilogue adds round once each, at magnitudes of at most
  mag + |bias| and mag + |bias| + |pos|.  A bf16 twin adds half a bf16 ulp (`check`) and must equal bf16(out) bit for bit.
* ref_true = fp64 of the unsplit a.w + bias + pos.  With a = ah + al + ra, w = wh + wl + rw, |al| <= 2^-8 |a|,
  |ra| <= 2^-8 |al| <= 2^-16 |a| (the same for w):
      a w - (ah wh + al wh + ah wl) = al wl + ra w + (ah + al) rw,
  three terms of at most 2^-16 |a| |w|, the last times (1 + 2^-16) for |ah + al| <= |a| + |ra|.  So
      |ref_split - ref_true| <= SPLIT_REL sum_k |a| |w|,     SPLIT_REL = 3 * 2^-16 * (1 + 2^-16).
  This is the accuracy claim of the design ("~2^-16 relative"), asserted on the CPU only; it is no kernel property.

Data families: `identity` - every pixel a distinct integer below 2^16 per (b, c, y, x) (exactly hi + lo), weight row n
one-hot +-1 at patch element n % K, integer bias and position embedding: every output is one pixel plus two small
integers, exact in fp32 in any order, and must match bit for bit (`assert_exact`), which pins every gathered position of
both sides, the reflected border included.  `gauss` - randn image, weights randn K^-1/2, bias 0.1 randn, pos 0.02 randn,
held to the bound above.

`emulate` is the kernel in torch fp32 (stage by stage, three products per stage), with `mutant=` the wrong kernels the
CPU test must show outside the bounds or not bit-equal.

Weight shadows: every result is exact (a copy, a transpose, a row permutation, one rounding to bf16, the two halves of
the split).  `shadow_expected` builds, from the contract in include/nvit_hip.h, the whole flat destination buffer a table
of entries must leave behind - the stated extents written, every other element still the fill - and `shadow_walk`
restates the kernel's walk over the table (tile items, first_item search, grid stride) on the CPU.

No constant is fitted to a kernel's output.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from attn_check import SENTINEL
from gemm_check import EXACT_LIMIT, U32, _gen, int_data
from kohonen_check import red

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
TILE_M, TILE_N, K_STEP, XCDS = 256, 256, 32, 8
SPLIT_REL = 3 * 2.0 ** -16 * (1 + 2.0 ** -16)

# (B, ch, S, Pl, Pg, C)
GEOMETRIES = ([(1, 1, 4, 4, 4, 4), (3, 1, 8, 4, 8, 60), (1, 1, 8, 4, 16, 8), (2, 2, 8, 4, 12, 264)]
              + [(B, 1, 4, 4, 8, 8) for B in (255, 256, 257)]
              + [(2049, 1, 4, 4, 4, 8)]
              + [(257, 1, 4, 4, 4, C) for C in (252, 256, 260, 516)]
              + [(5, 3, 32, 4, 8, 192)])
REJECTED = [(1, 1, 4, 4, 12, 8, False), (1, 1, 6, 4, 8, 8, False), (1, 1, 12, 6, 12, 8, False), (1, 1, 8, 4, 8, 60, True)]
FAMILIES = ("identity", "gauss")


def geo_id(g) -> str:
    return "B{}_ch{}_S{}_Pl{}_Pg{}_C{}".format(*g)


def kp_of(K: int) -> int:
    return (K + K_STEP - 1) // K_STEP * K_STEP


# ------------------------------------------------------------------------------------------------ gather
def reflect(i: torch.Tensor, n: int, mode: str = "reflect") -> torch.Tensor:
    if mode == "symmetric":                                    # (mutant: the edge pixel repeated)
        i = torch.where(i < 0, -i - 1, i)
        return torch.where(i >= n, 2 * n - 1 - i, i)
    if mode == "none":                                         # (mutant: no reflection, clamped to stay in the image)
        return i.clamp(0, n - 1)
    i = i.abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def patches(img: torch.Tensor, P: int, Pl: int, mutant: Optional[str] = None, Kp: Optional[int] = None) -> torch.Tensor:
    """[B, ch, S, S] -> [B T, K] (or [B T, Kp] with zeros behind K), column order (c, ph, pw)."""
    B, ch, S, _ = img.shape
    G, pad, K = S // Pl, (P - Pl) // 2, ch * P * P
    t, k = torch.arange(G * G), torch.arange(K if Kp is None else Kp)
    ty, tx = t // G, t % G
    c, ph, pw = k // (P * P), (k // P) % P, k % P
    if mutant == "transposed":
        ph, pw = pw, ph
    y = reflect(ty[:, None] * Pl - pad + ph[None, :], S, "symmetric" if mutant == "symmetric" else
                "none" if mutant == "reflect_x_only" else "reflect")
    x = reflect(tx[:, None] * Pl - pad + pw[None, :], S, "symmetric" if mutant == "symmetric" else "reflect")
    if mutant == "k_tail":                                     # elements >= K read on into the next channel / image
        flat = img.reshape(-1)
        idx = (torch.arange(B)[:, None, None] * ch * S * S + ((c[None, :] * S + y) * S + x)[None]) % flat.numel()
        return flat[idx].reshape(B * G * G, -1)
    out = img[:, c.clamp(max=ch - 1)[None, :], y, x].reshape(B * G * G, -1)
    if Kp is not None:
        out = torch.where(k[None, :] < K, out, torch.zeros_like(out))
    return out


def split(x: torch.Tensor):
    """the bf16 halves the kernels form: hi = bf16(x), lo = bf16(x - hi)"""
    hi = x.float().bfloat16()
    return hi, (x.float() - hi.float()).bfloat16()


def split_image(w: torch.Tensor, fill: float = 0.0) -> torch.Tensor:
    """[rows, K] fp32 -> [rows, 2 Kp] bf16: per 32 columns one slice [hi32 | lo32]; the padding of the last slice
    keeps `fill` (nvit_shadow_weights does not write it)."""
    rows, K = w.shape
    Kp = kp_of(K)
    hi, lo = split(w)
    img = torch.full((rows, 2 * Kp), fill, dtype=BF16)
    k = torch.arange(K)
    img[:, (k // 32) * 64 + k % 32] = hi
    img[:, (k // 32) * 64 + 32 + k % 32] = lo
    return img


# ------------------------------------------------------------------------------------------------ cases
def case(geo, family: str, seed: int = 1, bias: bool = True) -> Dict:
    B, ch, S, Pl, Pg, C = geo
    T = (S // Pl) ** 2
    c = {"geo": geo, "family": family, "T": T, "M": B * T}
    if family == "identity":
        n = ch * S * S
        assert B * n < 2 ** 16, "identity: pixel ids must stay below 2^16"
        img = (torch.arange(B * n) + 1).float().reshape(B, ch, S, S)
        hi, lo = split(img)
        assert torch.equal(hi.float() + lo.float(), img), "identity: a pixel is not hi + lo"
        assert 2 ** 16 + 8 < EXACT_LIMIT
        c["img"] = img
        for side, P in (("l", Pl), ("g", Pg)):
            K = ch * P * P
            n_ = torch.arange(C)
            w = torch.zeros(C, K)
            w[n_, n_ % K] = torch.where(n_ % 3 == 2, -1.0, 1.0)
            c["w_" + side] = w
            c["b_" + side] = int_data((C,), 4, seed + (1 if side == "l" else 4)) if bias else None
            c["pos_" + side] = int_data((T, C), 4, seed + (2 if side == "l" else 3))
    else:
        g = _gen(seed)
        c["img"] = torch.randn(B, ch, S, S, generator=g)
        for side, P in (("l", Pl), ("g", Pg)):
            K = ch * P * P
            c["w_" + side] = torch.randn(C, K, generator=g) * K ** -0.5
            c["b_" + side] = 0.1 * torch.randn(C, generator=g) if bias else None
            c["pos_" + side] = 0.02 * torch.randn(T, C, generator=g)
    return c


def side_of(c: Dict, side: str):
    B, ch, S, Pl, Pg, C = c["geo"]
    P = Pl if side == "l" else Pg
    return P, ch * P * P, c["w_" + side], c["b_" + side], c["pos_" + side]


# ------------------------------------------------------------------------------------------------ references
def reference(c: Dict, side: str) -> Dict[str, torch.Tensor]:
    """ref_split, its bound, ref_true and the magnitude sum |a| |w| of one side, all [M, C] fp64; `rows` = bf16(patch)."""
    B, ch, S, Pl, Pg, C = c["geo"]
    P, K, w, b, pos = side_of(c, side)
    a = patches(c["img"], P, Pl)
    (ah, al), (wh, wl) = split(a), split(w)
    ah, al, wh, wl = (t.double() for t in (ah, al, wh, wl))
    add = pos.double()[torch.arange(c["M"]) % c["T"]] + (b.double() if b is not None else 0.0)
    ref_split = ah @ wh.t() + al @ wh.t() + ah @ wl.t() + add
    mag = ah.abs() @ wh.abs().t() + al.abs() @ wh.abs().t() + ah.abs() @ wl.abs().t()
    bound = red(3 * K, mag) + 2 * U32 * (mag + add.abs())
    return {"ref_split": ref_split, "bound": bound, "ref_true": a.double() @ w.double().t() + add,
            "mag_true": a.double().abs() @ w.double().abs().t(), "rows": a.bfloat16()}


# ------------------------------------------------------------------------------------------------ emulator
MUTANTS = ("drop_al_wh", "drop_ah_wl", "halves_swapped", "symmetric", "reflect_x_only", "transposed", "pos_by_m",
           "k_tail", "last_token_tile", "second_group_first_side", "last_column_tile")


def emulate(c: Dict, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """out_l / out_g [M, C] fp32 and the saved rows a_l / a_g [M, Kp] bf16 as the kernel forms them: per stage of 32
    patch elements acc += ah wh; acc += al wh; acc += ah wl in fp32, then + bias, + pos[m % T].  Elements a workgroup
    never writes keep SENTINEL."""
    B, ch, S, Pl, Pg, C = c["geo"]
    M, T = c["M"], c["T"]
    out = {}
    for side in ("l", "g"):
        P, K, w, b, pos = side_of(c, side)
        Kp = kp_of(K)
        gather_mutant = mutant if mutant in ("symmetric", "reflect_x_only", "transposed", "k_tail") else None
        a = patches(c["img"], P, Pl, gather_mutant, Kp)
        ah, al = split(a)
        wp = torch.zeros(C, Kp)
        wp[:, :K] = w
        wh, wl = split(wp)
        if mutant == "halves_swapped":
            wh, wl = wl, wh
        first = None
        if mutant == "second_group_first_side" and side == "l":     # token tiles >= 8 take side 0's (global) operands
            Pf, Kf, wf, bf, posf = side_of(c, "g")
            assert Kf == K
            wfp = torch.zeros(C, Kp)
            wfp[:, :K] = wf
            first = (split(wfp), bf, posf)
        acc = torch.zeros(M, C)
        late = torch.arange(M) >= XCDS * TILE_M
        for s0 in range(0, Kp, K_STEP):
            sl = slice(s0, s0 + K_STEP)
            for x, y, skip in ((ah, wh, None), (al, wh, "drop_al_wh"), (ah, wl, "drop_ah_wl")):
                if skip is not None and mutant == skip:
                    continue
                part = x[:, sl].float() @ y[:, sl].float().t()
                if first is not None:
                    (fh, fl) = first[0]
                    fy = fh if y is wh else fl
                    part = torch.where(late[:, None], x[:, sl].float() @ fy[:, sl].float().t(), part)
                acc = acc + part
        m = torch.arange(M)
        rows = m.clamp(max=T - 1) if mutant == "pos_by_m" else m % T
        if b is not None:
            bb = b[None, :].expand(M, C)
            if first is not None and first[1] is not None:
                bb = torch.where(late[:, None], first[1][None, :], bb)
            acc = acc + bb
        pp = pos[rows]
        if first is not None:
            pp = torch.where(late[:, None], first[2][rows], pp)
        acc = acc + pp
        if mutant == "last_token_tile":
            acc[(math.ceil(M / TILE_M) - 1) * TILE_M:] = SENTINEL
        if mutant == "last_column_tile":
            acc[:, (math.ceil(C / TILE_N) - 1) * TILE_N:] = SENTINEL
        out["out_" + side] = acc
        out["a_" + side] = ah
    return out


# ------------------------------------------------------------------------------------------------ weight shadows
SHADOW_CASES = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 40)]        # (rows, cols)
PERM1_F = [16, 48, 272]
PERM2_K = [16, 32, 48, 72, 768]
PERM2_ROWS = [4, 100]
SHADOW_TILE = 64
GRID_CAP = 4096


def perm1_rows(F: int) -> torch.Tensor:
    """source row of every shadow row of a [2F, K] matrix: shadow row 32q + w is source row 16q + w for w < 16 and
    F + 16q + (w - 16) for w >= 16"""
    assert F % 16 == 0
    s = torch.arange(2 * F)
    q, w = s // 32, s % 32
    return torch.where(w < 16, 16 * q + w, F + 16 * q + (w - 16))


def spec(src: torch.Tensor, perm: int = 0, dst: bool = True, dstT: bool = True, pad_c: int = 0, pad_r: int = 0,
         slack: int = 0) -> Dict:
    """One table entry: dst [rows, cols + pad_c] in rows of cols + pad_c + slack elements, dstT [cols, rows + pad_r] in
    rows of rows + pad_r + slack elements (perm 2: dst [rows, 2 Kp] only)."""
    rows, cols = src.shape
    if perm == 2:
        return {"src": src, "perm": 2, "dst": True, "dstT": False, "dst_cols": cols, "dst_ld": 2 * kp_of(cols) + slack,
                "dstT_cols": 0, "dstT_ld": 0}
    return {"src": src, "perm": perm, "dst": dst, "dstT": dstT, "dst_cols": cols + pad_c, "dst_ld": cols + pad_c + slack,
            "dstT_cols": rows + pad_r, "dstT_ld": rows + pad_r + slack}


def shadow_layout(specs: List[Dict], gap: int = 5):
    """Offsets (in elements) of every dst and dstT inside one flat destination buffer, `gap` untouched elements
    before, between and behind them; -> (offsets of dst, offsets of dstT, total)."""
    off, od, ot = gap, [], []
    for s in specs:
        rows, cols = s["src"].shape
        od.append(off if s["dst"] else None)
        if s["dst"]:
            off += rows * s["dst_ld"] + gap
        ot.append(off if s["dstT"] else None)
        if s["dstT"]:
            off += cols * s["dstT_ld"] + gap
    return od, ot, off


def shadow_expected(specs: List[Dict], td, fill: float = SENTINEL) -> torch.Tensor:
    """The flat destination after nvit_shadow_weights, from the header's contract."""
    od, ot, total = shadow_layout(specs)
    flat = torch.full((total,), fill, dtype=td)
    for s, o_d, o_t in zip(specs, od, ot):
        src = s["src"]
        rows, cols = src.shape
        if s["perm"] == 2:
            view = flat[o_d:o_d + rows * s["dst_ld"]].view(rows, s["dst_ld"])
            hi, lo = split(src)
            k = torch.arange(cols)
            view[:, (k // 32) * 64 + k % 32] = hi
            view[:, (k // 32) * 64 + 32 + k % 32] = lo
            continue
        val = (src[perm1_rows(rows // 2)] if s["perm"] == 1 else src).to(td)
        if s["dst"]:
            view = flat[o_d:o_d + rows * s["dst_ld"]].view(rows, s["dst_ld"])
            view[:, :s["dst_cols"]] = 0
            view[:, :cols] = val
        if s["dstT"]:
            view = flat[o_t:o_t + cols * s["dstT_ld"]].view(cols, s["dstT_ld"])
            view[:, :s["dstT_cols"]] = 0
            view[:, :rows] = val.t()
    return flat


def shadow_items(s: Dict):
    rows, cols = s["src"].shape
    tiles_c = math.ceil(max(cols, s["dst_cols"] if s["dst"] else 0) / SHADOW_TILE)
    tiles_r = math.ceil(max(rows, s["dstT_cols"] if s["dstT"] else 0) / SHADOW_TILE)
    return tiles_c, tiles_r


def shadow_walk(specs: List[Dict], td, fill: float = SENTINEL, grid: int = GRID_CAP, stride_loop: bool = True) -> torch.Tensor:
    """The kernel's walk restated: workgroup g takes the items g, g + grid, ...; an item finds its table row by the
    binary search over first_item and handles one 64 x 64 tile.  stride_loop=False is the kernel without its loop."""
    od, ot, total = shadow_layout(specs)
    flat = torch.full((total,), fill, dtype=td)
    first, tiles = [], []
    n_items = 0
    for s in specs:
        first.append(n_items)
        tiles.append(shadow_items(s))
        n_items += tiles[-1][0] * tiles[-1][1]
    for g in range(min(grid, n_items)):
        for item in (range(g, n_items, grid) if stride_loop else (g,)):
            lo, hi = 0, len(specs) - 1
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if first[mid] <= item:
                    lo = mid
                else:
                    hi = mid - 1
            s, src = specs[lo], specs[lo]["src"]
            rows, cols = src.shape
            local = item - first[lo]
            r0, c0 = (local // tiles[lo][0]) * 64, (local % tiles[lo][0]) * 64
            r, cc = torch.arange(r0, r0 + 64), torch.arange(c0, c0 + 64)
            rin, cin = r[r < rows], cc[cc < cols]
            if s["perm"] == 2:
                if rin.numel() and cin.numel():
                    view = flat[od[lo]:od[lo] + rows * s["dst_ld"]].view(rows, s["dst_ld"])
                    hi_, lo_ = split(src[rin][:, cin])
                    view[rin[:, None], ((cin // 32) * 64 + cin % 32)[None, :]] = hi_
                    view[rin[:, None], ((cin // 32) * 64 + 32 + cin % 32)[None, :]] = lo_
                continue
            tile = torch.zeros(64, 64)
            if rin.numel() and cin.numel():
                srows = perm1_rows(rows // 2)[rin] if s["perm"] == 1 else rin
                tile[:rin.numel(), :cin.numel()] = src[srows][:, cin]
            if s["dst"] and rin.numel():
                cw = cc[cc < s["dst_cols"]]
                if cw.numel():
                    view = flat[od[lo]:od[lo] + rows * s["dst_ld"]].view(rows, s["dst_ld"])
                    view[rin[:, None], cw[None, :]] = tile[:rin.numel(), :cw.numel()].to(td)
            if s["dstT"] and cin.numel():
                rw = r[r < s["dstT_cols"]]
                if rw.numel():
                    view = flat[ot[lo]:ot[lo] + cols * s["dstT_ld"]].view(cols, s["dstT_ld"])
                    view[cin[:, None], rw[None, :]] = tile[:rw.numel(), :cin.numel()].t().to(td)
    return flat


def big_table(seed: int = 7, n: int = 4200) -> List[Dict]:
    """More entries than the grid has workgroups: ragged single-tile matrices, perm 0 and 1 in turn (a perm-1 matrix
    has 32 or 64 rows), every 601st entry a multi-tile one; dst, dstT or both in turn."""
    g = _gen(seed)
    specs = []
    for i in range(n):
        perm = i % 2
        if i % 601 == 600:
            rows, cols = ((130, 70), (96, 130), (65, 63))[(i // 601) % 3] if perm == 0 else ((96, 70), (160, 65))[(i // 601) % 2]
        elif perm == 0:
            rows, cols = 1 + (i * 7) % 23, 1 + (i * 5) % 19
        else:
            rows, cols = 32 * (1 + (i // 2) % 2), 1 + (i * 3) % 11
        src = torch.randn(rows, cols, generator=g)
        which = i % 3
        specs.append(spec(src, perm, dst=which != 1, dstT=which != 0, pad_c=(i % 4 == 3) * 2, pad_r=(i % 5 == 4) * 3,
                          slack=i % 2))
    return specs
