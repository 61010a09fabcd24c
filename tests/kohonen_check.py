"""Oracles of the Kohonen-head, pooling and reconstruction kernel tests (a plain helper module;
test_kohonen_check.py checks it on the CPU, test_gpu_kohonen_ops.py uses it against the HIP kernels).

Every operation has an `*_eval(..., dtype)`: the operation in plain torch math, written from what it means, with the
gradients from autograd of that forward.  At dtype=float64 it is the reference; at float32 it is the "correct kernel in
fp32" that the CPU test holds against the bounds.  The `*_bounds` functions give a per-element, data-dependent error
bound for an fp32 kernel from the fp64 quantities:

* a reduction over n terms:  LAMBDA * sqrt(n) * U32 * (sum of |terms|)      (as gemm_check.gauss_bound)
* an element-wise result:    c * U32 * mag, c = fp32 roundings of the formula, + 4 per tanhf / expf / sqrtf / division,
  mag = sum of the absolute values of the terms before any cancellation
* an input that itself carries an error passes it on through the derivative of the formula (first order)
* a bf16 output adds half a bf16 ulp (`check` does that from the output's dtype)

Where a bound is 0 (an empty node, a distance between identical rows) the result must be exact.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from gemm_check import LAMBDA, U32, _gen, half_ulp_bf16

F64 = torch.float64
LIB = 4.0   # allowance, in fp32 roundings, for one tanhf / expf / sqrtf / division

# ------------------------------------------------------------------------------------------------ shapes
BMU_SHAPES = [(37, 9, 32), (257, 30, 100), (1001, 256, 192), (513, 256, 768), (300, 1024, 64)]       # (M, N, C)
BMU_MAX_CLOSE = 0.02
GATHER_SHAPES = [(M, C) for C in (4, 100, 768) for M in (1, 1001)]
ONEHOT_N = [4, 36, 256]
SCATTER_FALLBACK = [(1, 9, 32), (255, 9, 30), (256, 30, 32), (257, 30, 100), (1001, 25, 2048), (700, 9, 260)]
SCATTER_GEMM = [(1001, 36, 192), (5000, 256, 64)]
SOM_UPDATE_SHAPES = [(1, 1, 4, 1, 1), (5, 7, 260, 3, 4), (9, 4, 1028, 4, 4)]                          # (B, T, C, gm, gn)
COS_SHAPES = [(1, 4), (3, 260), (37, 768), (1001, 1028), (4100, 64)]
HUBER_SIZES = [4, 1028, 37 * 260, 1024 * 256 * 4 + 4 * 260]
# (map_size, C, M, pattern, duplicate rows): every map size, width and M of the issue; 70000 tokens only at C = 4 (the
# fp64 autograd reference holds M * 8 * C values several times over)
SMOOTH_CASES = [(1, 4, 1, "one", False), (1, 100, 255, "one", False), (2, 4, 257, "uniform", False),
                (2, 768, 255, "sparse", False), (2, 100, 257, "uniform", True), (3, 100, 257, "uniform", False),
                (3, 4, 70000, "uniform", False), (3, 768, 1, "one", False), (3, 100, 255, "sparse", True),
                (4, 100, 255, "sparse", False), (4, 4, 70000, "one", False), (4, 768, 257, "uniform", True),
                (16, 100, 257, "wave", False), (16, 4, 70000, "wave", False), (16, 768, 255, "uniform", False),
                (16, 4, 70000, "sparse", False)]
RECON_SHAPES = [(1, 1, 4, 4), (3, 3, 40, 8), (2, 3, 24, 4), (5, 1, 36, 12)]                            # (B, ch, S, P)
POOL_SHAPES = [(1, 1, 4), (5, 7, 260), (2, 784, 192), (3, 25, 1028), (1100, 3, 64), (2, 9, 2048)]     # (B, T, C)
COLSUM_CASES = [(1, 4, 1), (300, 52, 10), (1001, 260, 7)]                                              # (R, N, period | R)


# ------------------------------------------------------------------------------------------------ checks
def check(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, label: str, verbose: bool = True) -> float:
    """Assert |out - ref| <= bound element-wise (+ half a bf16 ulp for a bf16 output); returns and prints the largest
    err / bound.  Where the bound is 0 the output must equal the reference."""
    out = out.detach().cpu()
    ref = ref.detach().to(F64)
    bound = torch.as_tensor(bound, dtype=F64).expand(ref.shape)
    assert tuple(out.shape) == tuple(ref.shape), f"{label}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(out.float()).all(), f"{label}: non-finite output"
    if out.dtype == torch.bfloat16:
        bound = bound + half_ulp_bf16(ref.abs() + bound)
    err = (out.double() - ref).abs()
    zero = bound == 0
    assert not (err[zero] > 0).any(), f"{label}: nonzero error where the result must be exact"
    margin = (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0
    if verbose:
        print(f"   {label}: max err/bound {margin:.3f}")
    assert margin <= 1.0, f"{label}: max err/bound {margin:.3f} > 1"
    return margin


def check_all(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], bound: Dict[str, torch.Tensor], label: str,
              verbose: bool = True) -> float:
    assert set(bound) <= set(got) and set(bound) <= set(ref)
    return max(check(got[k], ref[k], bound[k], f"{label} {k}", verbose) for k in bound)


def red(n: float, mag: torch.Tensor) -> torch.Tensor:
    """Bound of an fp32 sum of n terms with sum of absolute values mag."""
    return LAMBDA * math.sqrt(max(n, 1)) * U32 * mag


# ------------------------------------------------------------------------------------------------ data
def index_patterns(M: int, N: int, seed: int) -> Dict[str, torch.Tensor]:
    """all tokens on one node / uniform spread / some nodes never hit."""
    g = _gen(seed)
    keep = torch.arange(0, N, 3) if N > 1 else torch.zeros(1, dtype=torch.long)
    return {"one": torch.full((M,), N // 2, dtype=torch.long),
            "uniform": torch.randint(0, N, (M,), generator=g),
            "sparse": keep[torch.randint(0, keep.numel(), (M,), generator=g)]}


def wave_distinct(M: int, N: int) -> torch.Tensor:
    """64 consecutive tokens (one wave) carry 64 distinct values (N >= 64); the phase moves every 256 tokens."""
    assert N >= 64
    i = torch.arange(M)
    return (i * 5 + i // 256 * 7) % N if N % 5 else (i + i // 256 * 7) % N


def make_index(pattern: str, M: int, N: int, seed: int) -> torch.Tensor:
    return wave_distinct(M, N) if pattern == "wave" else index_patterns(M, N, seed)[pattern]


# ------------------------------------------------------------------------------------------------ BMU
def bmu_ref(x: torch.Tensor, nodes: torch.Tensor) -> torch.Tensor:
    return torch.cdist(x.double(), nodes.double(), compute_mode="donot_use_mm_for_euclid_dist").argmin(dim=-1)


def bmu_check(idx: torch.Tensor, x: torch.Tensor, nodes: torch.Tensor, label: str, verbose: bool = True) -> float:
    """idx must be the fp64 argmin except on rows whose two best q = |n|^2 - 2 x.n lie closer than
    tol = 2 (C + 4) U32 (max |n|^2 + 2 max |x|.|n|); there the chosen node's q must be within tol of the minimum, and
    such rows are at most BMU_MAX_CLOSE of the case.  Returns the share of such rows."""
    idx = idx.detach().cpu()
    M, C = x.shape
    N = nodes.shape[0]
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (M,)
    assert ((idx >= 0) & (idx < N)).all(), f"{label}: index outside [0, {N})"
    x64, n64 = x.double(), nodes.double()
    nn = (n64 * n64).sum(-1)
    q = nn[None, :] - 2.0 * x64 @ n64.t()
    tol = 2.0 * (C + 4) * U32 * (nn.max() + 2.0 * (x64.abs() @ n64.abs().t()).max(dim=-1).values)
    ref = bmu_ref(x, nodes)
    if N > 1:
        two = q.topk(2, dim=-1, largest=False).values
        close = (two[:, 1] - two[:, 0]) < tol
    else:
        close = torch.zeros(M, dtype=torch.bool)
    wrong = idx != ref
    assert not (wrong & ~close).any(), \
        f"{label}: {(wrong & ~close).sum().item()} rows differ from the fp64 argmin with a clear gap"
    excess = q.gather(1, idx[:, None])[:, 0] - q.min(dim=-1).values
    assert (excess <= tol).all(), f"{label}: a chosen node is farther than the bound from the minimum"
    share = close.double().mean().item()
    if verbose:
        print(f"   {label}: {wrong.sum().item()} of {M} rows differ (all within the bound); close rows {share:.4f}")
    assert share <= BMU_MAX_CLOSE, f"{label}: {share:.4f} of the rows are closer than the bound"
    return share


def tie_case(N: int, C: int, seed: int):
    """nodes with duplicated rows at (5, 6) [neighbouring lanes], (10, 74) [one lane's strided loop, N > 74] and
    (3, N-1) [far lanes: the shuffle reduction]; x = the duplicated rows.  Returns (x, nodes, expected index)."""
    nodes = torch.randn(N, C, generator=_gen(seed))
    pairs = [(5, 6), (3, N - 1)] + ([(10, 74)] if N > 74 else [])
    for lo, hi in pairs:
        nodes[hi] = nodes[lo]
    want = torch.tensor([lo for lo, _ in pairs])
    return nodes[want].clone(), nodes, want


# ------------------------------------------------------------------------------------------------ scatter
def scatter_ref(dout: torch.Tensor, idx: torch.Tensor, N: int):
    """(ref, bound) of dnodes[n] = sum of the dout rows with idx == n; n of the bound = the node's hit count."""
    d = dout.double()
    ref = torch.zeros(N, d.shape[1], dtype=F64).index_add_(0, idx, d)
    mag = torch.zeros(N, d.shape[1], dtype=F64).index_add_(0, idx, d.abs())
    cnt = torch.bincount(idx, minlength=N).double()
    return ref, LAMBDA * cnt.sqrt()[:, None] * U32 * mag


def scatter_fp32(dout: torch.Tensor, idx: torch.Tensor, N: int) -> torch.Tensor:
    return torch.zeros(N, dout.shape[1]).index_add_(0, idx, dout.float())


# ------------------------------------------------------------------------------------------------ SOM update
def grid_d2(w: int, gm: int, gn: int, periodic: bool) -> torch.Tensor:
    """Squared grid distance of every node to node w; on the periodic map the smallest over the wrapped copies."""
    n = torch.arange(gm * gn)
    di, dj = (n // gn - w // gn).double(), (n % gn - w % gn).double()
    if not periodic:
        return di * di + dj * dj
    best = None
    for si in (-gm, 0, gm):
        for sj in (-gn, 0, gn):
            d = (di + si) ** 2 + (dj + sj) ** 2
            best = d if best is None else torch.minimum(best, d)
    return best


def som_update_eval(nodes, x, idx, la: float, sigma: float, gm: int, gn: int, periodic: bool, dtype=F64):
    """The sequential update: for sample i, node <- node + s_i (v_i - node), s_i = la exp(-d2(node, bmu_i) / 2 sigma^2),
    bmu_i = idx.flatten()[i], v_i = the sample's T*C values averaged in C groups of T consecutive ones.
    Returns (nodes after, bound).  Bound per step: the roundings of sub, mul, add; the strength's (1 conversion of la,
    1 mul, expf, and its argument's 7 = conversion of sigma, square, division, mul, passed on times the argument);
    the pooled value's T - 1 adds and one division; earlier error carried on by (1 - s)."""
    B, T, C = x.shape
    nd = nodes.to(dtype).clone()
    bound = torch.zeros_like(nd, dtype=F64)
    flat = idx.reshape(-1)
    for i in range(B):
        a = grid_d2(int(flat[i]), gm, gn, periodic) / (2.0 * sigma * sigma)
        s = (la * torch.exp(-a)).to(dtype)[:, None]
        xi = x[i].to(dtype).reshape(C, T)
        v = xi.mean(dim=1)[None, :]
        new = nd + s * (v - nd)
        if dtype == F64:
            e_v = U32 * (T - 1 + LIB) * xi.abs().mean(dim=1)[None, :]
            c_s = (2 + LIB + 7 * a)[:, None]
            bound = (1 - s).abs() * bound + s * e_v + U32 * (s * (v.abs() + nd.abs()) * (2 + c_s) + new.abs())
        nd = new
    return nd, bound


# ------------------------------------------------------------------------------------------------ consistency
def cos_data(M: int, C: int, seed: int):
    """two correlated views (cos about 0.9): a dropped or doubled row then shows in the loss."""
    a = torch.randn(M, C, generator=_gen(seed))
    return a, a + 0.5 * torch.randn(M, C, generator=_gen(seed + 1))


def cos_eval(a, b, g: float, dtype=F64) -> Dict[str, torch.Tensor]:
    a_, b_ = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    an = a_ / a_.norm(dim=-1, keepdim=True)
    bn = b_ / b_.norm(dim=-1, keepdim=True)
    loss = 1 - (an * bn).sum(dim=-1).mean()
    da, db = torch.autograd.grad(loss, (a_, b_), torch.tensor(g, dtype=dtype))
    return {"loss": loss.detach(), "da": da, "db": db}


def cos_bounds(a, b, g: float) -> Dict[str, torch.Tensor]:
    """cos_m = a.b / (|a| |b|): three sums over C, two sqrtf and two divisions, two muls.  loss = 1 - sum(cos) / M.
    da = gs (b^ - a^ cos) / |a|, gs = -g / M: per term 9 roundings (division of gs, 5 muls / subs) and twice the error of
    an inverse norm (half a sum's + sqrtf + division); the error of cos comes in through a^."""
    a, b = a.double(), b.double()
    M, C = a.shape
    na, nb = a.norm(dim=-1, keepdim=True), b.norm(dim=-1, keepdim=True)
    cs = (a * b).sum(-1, keepdim=True) / (na * nb)
    rc = LAMBDA * math.sqrt(C)
    e_cs = U32 * (rc * (a * b).abs().sum(-1, keepdim=True) / (na * nb) + cs.abs() * (rc + 2 * LIB + 2 * LIB + 2))
    loss = e_cs.mean() + red(M, cs.abs().mean()) + U32 * (LIB + 2) * (1 + cs.mean().abs())
    gs = abs(g) / M
    c_el = 9 + 2 * (rc / 2 + 2 * LIB)
    ah, bh = a / na, b / nb
    da = gs / na * (U32 * c_el * (bh.abs() + (ah * cs).abs()) + ah.abs() * e_cs)
    db = gs / nb * (U32 * c_el * (ah.abs() + (bh * cs).abs()) + bh.abs() * e_cs)
    return {"loss": loss, "da": da, "db": db}


# ------------------------------------------------------------------------------------------------ huber
def huber_data(n: int, seed: int):
    """|d| on both sides of 1, and elements with d = 1, d = -1 and d = 0 exactly."""
    g = _gen(seed)
    a = torch.randn(n, generator=g)
    b = a - 1.5 * torch.randn(n, generator=g)
    a[0], b[0] = 0.5, -0.5
    a[1], b[1] = 0.5, 1.5
    b[2] = a[2]
    if n > 8:
        a[n - 1], b[n - 1] = -0.25, 0.75
        b[n - 2] = a[n - 2]
    return a, b


def huber_eval(a, b, g: float, dtype=F64) -> Dict[str, torch.Tensor]:
    a_, b_ = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    loss = F.huber_loss(a_, b_, reduction="mean", delta=1.0)
    da, db = torch.autograd.grad(loss, (a_, b_), torch.tensor(g, dtype=dtype))
    return {"loss": loss.detach(), "da": da, "db": db}


def huber_bounds(a, b, g: float) -> Dict[str, torch.Tensor]:
    """term h(d), d = a - b: the subtraction's rounding passes through h' = clamp(d, -1, 1), then two roundings;
    the sum over n, then a division and a mul.  Gradient clamp(d) * g / n: the subtraction where |d| <= 1, and
    division + 2 muls."""
    a, b = a.double(), b.double()
    n = a.numel()
    d = a - b
    cl = d.clamp(-1, 1)
    h = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    e_term = U32 * ((a.abs() + b.abs()) * cl.abs() + 2 * h)
    loss = e_term.mean() + red(n, h.mean()) + U32 * (LIB + 1) * h.mean()
    gs = abs(g) / n
    dab = U32 * gs * ((a.abs() + b.abs()) * (d.abs() <= 1) + (LIB + 2) * cl.abs())
    return {"loss": loss, "da": dab, "db": dab}


# ------------------------------------------------------------------------------------------------ smoothness
def neighbour_table(ms: int) -> torch.Tensor:
    """[ms*ms, 8]: the 8 grid neighbours of every node on the wrapped ms x ms map, offsets in row-major order."""
    n = torch.arange(ms * ms)
    r, c = n // ms, n % ms
    offs = [(dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0)]
    return torch.stack([((r + dr) % ms) * ms + (c + dc) % ms for dr, dc in offs], dim=1)


def smooth_nodes(ms: int, C: int, seed: int, dup: bool) -> torch.Tensor:
    nodes = torch.randn(ms * ms, C, generator=_gen(seed))
    if dup:
        nodes[1] = nodes[0]        # (0,0) and (0,1): grid neighbours with identical rows
    return nodes


def smooth_eval(nodes, idx, ms: int, g: float, dtype=F64, table: Optional[torch.Tensor] = None,
                grouped: bool = False):
    """mean over tokens and their 8 wrapped neighbours of |nodes[idx] - nodes[nb]|; cnt = histogram of idx;
    D[n][k] = |nodes[n] - nodes[nb_k(n)]|."""
    tab = neighbour_table(ms) if table is None else table
    nd = nodes.to(dtype).requires_grad_(True)
    if grouped:     # equal terms grouped by the histogram (the fp32 restatement: no sum of M equal values)
        cnt = torch.bincount(idx, minlength=ms * ms).to(dtype)
        loss = (cnt[:, None] * torch.linalg.vector_norm(nd[:, None, :] - nd[tab], dim=-1)).sum() / (8 * idx.numel())
    else:
        loss = torch.linalg.vector_norm(nd[idx][:, None, :] - nd[tab[idx]], dim=-1).mean()
    (dn,) = torch.autograd.grad(loss, nd, torch.tensor(g, dtype=dtype))
    with torch.no_grad():
        D = torch.linalg.vector_norm(nd[:, None, :] - nd[tab], dim=-1)
    return {"loss": loss.detach(), "D": D, "dnodes": dn, "cnt": torch.bincount(idx, minlength=ms * ms)}


def smooth_bounds(nodes, idx, ms: int, g: float) -> Dict[str, torch.Tensor]:
    """D = sqrtf(sum_c d^2), d = a - b: each term's subtraction (mag |a| + |b|) and square, the sum over C, sqrtf.
    Tokens on the same node contribute equal terms, so the sums over tokens are the histogram times a term (an exact
    integer factor), not reductions: loss = sum_n cnt[n] sum_k D[n][k] / (8 M), a sum of 8 Nn positive terms with D's
    error, 2 muls and a division.  dnodes[n] = (g / 8M) sum_k (cnt[n] + cnt[nb_k]) (node_n - node_nb_k) / D[n][k], node
    n as centre and as neighbour: at most 16 terms, each with a division, a mul, the subtraction and D's relative
    error; the scale g / (8 M) with 3 muls and a division."""
    nodes = nodes.double()
    Nn, C = nodes.shape
    M = idx.numel()
    tab = neighbour_table(ms)
    diff = nodes[:, None, :] - nodes[tab]                       # [Nn, 8, C]
    mab = nodes.abs()[:, None, :] + nodes.abs()[tab]
    S2 = (diff * diff).sum(-1)
    D = S2.sqrt()
    pos = D > 0
    Ds = torch.where(pos, D, torch.ones_like(D))
    e_S = U32 * ((LAMBDA * math.sqrt(C) + 1) * S2 + 2 * (diff.abs() * mab).sum(-1))
    e_D = torch.where(pos, e_S / (2 * Ds) + U32 * LIB * D, torch.zeros_like(D))
    cnt = torch.bincount(idx, minlength=Nn).double()
    loss_v = (cnt[:, None] * D).sum() / (8 * M)
    loss = (cnt[:, None] * e_D).sum() / (8 * M) + red(8 * Nn, loss_v) + U32 * (LIB + 3) * loss_v
    pairs = torch.where(pos, cnt[:, None] + cnt[tab], torch.zeros_like(D))                        # [Nn, 8]
    w = (pairs / Ds)[:, :, None]
    rel_D = (e_D / Ds)[:, :, None]
    c_term = 2 + LIB + LAMBDA * math.sqrt(16) + 3 + LIB
    dn = abs(g) / (8 * M) * (w * (U32 * (mab + diff.abs() * c_term) + diff.abs() * rel_D)).sum(dim=1)
    return {"loss": loss, "D": e_D, "dnodes": dn}


# ------------------------------------------------------------------------------------------------ reconstruction
def recon_data(B: int, ch: int, S: int, P: int, seed: int):
    """raw [B*T, ch*P*P] with |raw| up to 12 (tanh saturates), img [B, ch, S, S]."""
    g = _gen(seed)
    T, K = (S // P) ** 2, ch * P * P
    raw = torch.randn(B * T, K, generator=g) * 1.5
    flat = raw.reshape(-1)
    flat[::7] = torch.empty(flat[::7].shape).uniform_(-12.0, 12.0, generator=g)
    flat[0], flat[-1] = 12.0, -12.0
    return raw, torch.randn(B, ch, S, S, generator=g)


def recon_eval(raw, img, P: int, g: float, dtype=F64, transpose_patch: bool = False) -> Dict[str, torch.Tensor]:
    B, ch, S, _ = img.shape
    r_ = raw.to(dtype).requires_grad_(True)
    im = img.to(dtype)
    if transpose_patch:                                        # (mutant of the CPU test: ph and pw swapped)
        im = im.transpose(-1, -2)
    tgt = F.unfold(im, kernel_size=P, stride=P).transpose(1, 2).reshape(r_.shape)     # [B*T, (c, ph, pw)]
    loss = F.mse_loss(torch.tanh(r_), tgt)
    (draw,) = torch.autograd.grad(loss, r_, torch.tensor(g, dtype=dtype))
    return {"loss": loss.detach(), "draw": draw}


def recon_bounds(raw, img, P: int, g: float) -> Dict[str, torch.Tensor]:
    """term (tanh(raw) - tgt)^2: tanhf and the subtraction pass through 2 |d|, then the square; the sum, 2 roundings of
    the scale.  draw = gs (r - tgt) (1 - r^2), gs = 2 g / n: mag |gs| (|r| + |tgt|) (1 + r^2) and c = 22: tanhf in the
    difference (4) and twice in the square (8), 2 subtractions, the square, 2 muls, gs (division + mul)."""
    raw, img = raw.double(), img.double()
    n = raw.numel()
    tgt = F.unfold(img, kernel_size=P, stride=P).transpose(1, 2).reshape(raw.shape)
    r = torch.tanh(raw)
    d = r - tgt
    e_term = U32 * (2 * d.abs() * ((LIB + 1) * r.abs() + tgt.abs()) + d * d)
    lv = (d * d).mean()
    loss = e_term.mean() + red(n, lv) + U32 * 2 * lv
    c = LIB + 2 * LIB + 2 + 1 + 2 + (LIB + 1)
    draw = c * U32 * (2 * abs(g) / n) * (r.abs() + tgt.abs()) * (1 + r * r)
    return {"loss": loss, "draw": draw}


# ------------------------------------------------------------------------------------------------ pool + LayerNorm
def pool_ln_eval(x, w, b, eps: float, g, old_dw=None, old_db=None, dtype=F64) -> Dict[str, torch.Tensor]:
    """x [B, T, C]; ln = LayerNorm(mean over tokens); gradients for upstream g [B, C] (+ the previous dw / db)."""
    x_, w_, b_ = (t.to(dtype).requires_grad_(True) for t in (x, w, b))
    pooled = x_.mean(dim=1)
    ln = F.layer_norm(pooled, (x.shape[-1],), w_, b_, eps)
    dx, dw, db = torch.autograd.grad(ln, (x_, w_, b_), g.to(dtype))
    if old_dw is not None:
        dw, db = dw + old_dw.to(dtype), db + old_db.to(dtype)
    return {"pooled": pooled.detach(), "ln": ln.detach(), "dx": dx, "dw": dw, "db": db}


def pool_ln_bounds(x, w, b, eps: float, g, old_dw=None, old_db=None) -> Dict[str, torch.Tensor]:
    """Forward: pooled = sum over T and a division; mean and variance = sums over C and a division each; rstd = add,
    sqrtf, division; the output 2 muls and an add; every error passed on to first order.  Backward
    dx = rstd (g w - m1 - xh m2) / T with m1, m2 means over C; dw, db sums over B (+ the old value)."""
    x, w, b, g = x.double(), w.double(), b.double(), g.double()
    B, T, C = x.shape
    rc = LAMBDA * math.sqrt(C)
    mean_c = lambda t: t.mean(dim=-1, keepdim=True)
    v = x.mean(dim=1)
    e_v = U32 * (LAMBDA * math.sqrt(T) + LIB) * x.abs().mean(dim=1)
    mu = mean_c(v)
    e_mu = U32 * (rc + LIB) * mean_c(v.abs()) + mean_c(e_v)
    cen = v - mu
    e_cen = e_v + e_mu + U32 * (v.abs() + mu.abs())
    var = mean_c(cen * cen)
    e_var = mean_c(2 * cen.abs() * e_cen) + U32 * (rc + 1 + LIB) * var
    rstd = (var + eps) ** -0.5
    r_rel = e_var / (2 * (var + eps)) + U32 * (1 + 2 * LIB)
    xh = cen * rstd
    e_xh = rstd * e_cen + xh.abs() * (r_rel + U32)
    ln = w.abs() * e_xh + U32 * (2 * (xh * w).abs() + b.abs())
    gg = g * w
    m1, m2 = mean_c(gg), mean_c(gg * xh)
    e_m1 = U32 * (rc + LIB + 1) * mean_c(gg.abs())
    e_m2 = mean_c(gg.abs() * e_xh) + U32 * (rc + LIB + 2) * mean_c((gg * xh).abs())
    inner = gg - m1 - xh * m2
    e_inner = (U32 * gg.abs() + e_m1 + e_xh * m2.abs() + xh.abs() * e_m2
               + 3 * U32 * (gg.abs() + m1.abs() + (xh * m2).abs()))
    dx = (rstd * e_inner + (rstd * inner).abs() * (r_rel + U32 * (3 + LIB))) / T
    odw = old_dw.double().abs() if old_dw is not None else 0.0
    odb = old_db.double().abs() if old_db is not None else 0.0
    db = red(B + 1, g.abs().sum(0) + odb)
    dw = (g.abs() * e_xh).sum(0) + U32 * (LAMBDA * math.sqrt(B + 1) + 3) * ((g * xh).abs().sum(0) + odw)
    return {"pooled": e_v, "ln": ln, "dx": dx[:, None, :].expand(B, T, C), "dw": dw, "db": db}


# ------------------------------------------------------------------------------------------------ colsum / scale_cols
def colsum_ref(a, b, R: int, N: int, period: int, scale: float, old=None):
    """(ref, bound) of out[rc, n] = scale * sum_{r = rc mod period} a[r, n] b[r, n] (+ old): the products' rounding,
    the sum, the scale, the add."""
    per = max(period, 1)
    p = a.double() * (b.double() if b is not None else 1.0)
    rows = torch.arange(R) % per
    ref = torch.zeros(per, N, dtype=F64).index_add_(0, rows, p) * scale
    mag = torch.zeros(per, N, dtype=F64).index_add_(0, rows, p.abs()) * abs(scale)
    if old is not None:
        ref, mag = ref + old.double().reshape(per, N), mag + old.double().abs().reshape(per, N)
    return ref, U32 * (LAMBDA * math.sqrt(math.ceil(R / per) + 1) + 2) * mag


def scale_cols_ref(a, s, c: float):
    """(ref, bound) of a[r, n] * s[n] * c: two muls."""
    ref = a.double() * (s.double() if s is not None else 1.0) * c
    return ref, 2 * U32 * ref.abs()
