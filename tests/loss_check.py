"""Oracles of the loss-end kernel tests: nvit_ce_loss, nvit_ce_loss_soft and nvit_eval_metrics (misc.hip).  A plain
helper module; test_loss_check.py checks it on the CPU, test_gpu_loss_bounds.py uses it against the HIP kernels.

The reference (`ce_eval` / `eval_metrics_eval` at dtype=float64) is written from the definitions of include/nvit_hip.h,
not from F.cross_entropy (which divides by the number of non-ignored rows and makes 0 * -inf a NaN):

    lse      = logsumexp(z)
    rowloss  = lse - (1 - eps) (lam z[y] + (1 - lam) z[y2]) - eps mean(z)       (hard loss: lam = 1, eps = 0)
    a label outside [0, N), tested on its 64-bit value, contributes no term; in the hard loss such a row has rowloss 0
    a term of weight 0 is skipped, not multiplied; eps = 0 skips the mean
    loss     = sum(rowloss) / B over ALL rows
    dlogits  = (softmax - t) / B,  t = (1 - eps) (lam e[y] + (1 - lam) e[y2]) + eps / N
    rank     = #{j : z_j beats z_y}; z_j beats z_y when it is larger, or equal at a lower index; a NaN is larger than
               every number and equal to another NaN (the order of torch.topk)
    metrics  = loss over the rows with a label in range / B, 100 #(rank < 1) / B, 100 #(rank < min(5, N)) / B, 1

The same functions at dtype=float32 are the "correct kernel in fp32" that the CPU test holds against the bounds, and
with `mutant=` the wrong kernels it must show outside them.

Bounds (`ce_bounds`, `eval_metrics_bounds`), per element, from the fp64 quantities, operation by operation.  u = U32
= 2^-24, LIB = 4 roundings for one expf / logf / division, red(n, mag) = LAMBDA sqrt(n) u mag for an fp32 sum of n terms
(gemm_check / kohonen_check), FTZ = 2^-126 where a true value is subnormal and the hardware may flush it.

* mx = max(z)                    exact (a selection)
* d  = z - mx                    one subtraction: u |d|
* p  = expf(d)                   p (u |d| + LIB u), + FTZ where 0 < p < 2^-126; 0 where p = 0 (d = -inf, or below the
                                 range of fp64, where fp32 gives 0 as well)
* s  = sum p                     red(N, s) + sum e_p         (every p >= 0, so the sum of magnitudes is s itself)
* lse = mx + logf(s)             LIB u |ln s| + e_s / s + u (|mx| + |ln s|)
* mean = sum z / N               red(N, sum |z|) / N + LIB u |mean|
* hard rowloss = lse - z[y]      e_lse + u (|lse| + |z_y|); 0 (exact) for a label out of range
* soft rowloss                   e_lse + eps e_mean + 7 u (|lse| + |w1 z_y| + |w2 z_y2| + |eps mean|): the longest chain
                                 of roundings a term passes through is (1 - lam), its product with z, the sum of the two
                                 products, (1 - eps), the product with it, and the two subtractions
* loss = sum rowloss / B         red(B, sum |rowloss|) / B + mean(e_rowloss) + LIB u |loss|
* dlogits = (p (1/s) - t) (1/B)  with sm = p / s:  [ e_p / s + sm (e_s / s + LIB u)      p and 1 / s
                                                    + c_t u t                            t: 0 roundings hard, 5 soft
                                                    + 2 u (sm + t)                       product and subtraction (or one fma)
                                                    + (LIB + 1) u |sm - t| ] / B         1 / B and the last product
                                 + FTZ / B where 0 < sm < 2 FTZ and + FTZ where 0 < |sm - t| / B < 2 FTZ: the relative
                                 rounding u |x| holds for normal results only, a product in (or within a factor 2 of,
                                 for the computed value is not the true one) the subnormal range may be flushed.
                                 Where p = 0 and t = 0 this is 0: the output must be exactly 0.
* eval loss                      the hard rowloss bounds; the sum over the rows (per wave, then the 16 waves in order:
                                 at most B terms) red(B, .), the division LIB u, and one add into the accumulator
                                 u (|acc before| + |batch loss|)
* the counts are exact integers and the stored percentages the fp32 value of 100 * count / B (`percent`)

No constant is fitted to a kernel's output.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from epilogue_check import FTZ
from gemm_check import U32, _gen
from kohonen_check import LIB, red

F64 = torch.float64
F32 = torch.float32
NEG_INF = float("-inf")

# ------------------------------------------------------------------------------------------------ shapes
CE_N = [1, 3, 63, 64, 65, 255, 256, 257, 1000, 1023, 4099]
CE_B = [1, 3, 257, 1000]
CE_SHAPES = [(3, N) for N in CE_N] + [(B, N) for N in (65, 257) for B in CE_B if B != 3]      # (B, N)
CE_COUNTING_ONLY = (257, 4099)
CE_FAMILIES = ("gauss", "shifted", "peaked", "counting", "masked")
SHIFTS = (1.0e4, -1.0e4, 88.0, -104.0)
EVAL_B = [1, 15, 16, 17, 33, 1000]
EVAL_N = [1, 2, 5, 6, 63, 64, 65, 1000, 4099]
EVAL_FAMILIES = ("levels", "shifted", "counting")


def out_of_range(N: int) -> List[int]:
    return [2 ** 32 + 1, -1, 2 ** 31, N, -100, N + 5]


# ------------------------------------------------------------------------------------------------ data
def logits(family: str, B: int, N: int, seed: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """fp32 logits [B, N] of a family and, for `peaked`, the column of each row's peak."""
    g = _gen(seed)
    z = 3.0 * torch.randn(B, N, generator=g)
    r = torch.arange(B)
    if family == "gauss":
        return z, None
    if family == "shifted":
        return z + torch.tensor(SHIFTS)[r % 4][:, None], None
    if family == "peaked":
        pk = torch.where(r % 2 == 0, torch.full((B,), N - 1), torch.randint(0, N, (B,), generator=g))
        lift = 60.0 + 60.0 * torch.rand(B, generator=g)
        z[r, pk] = z.max(dim=1).values + lift
        return z, pk
    if family == "counting":
        return ((r % 7 - 3).float() * 2.5)[:, None].expand(B, N).contiguous(), None
    if family == "masked":
        z[torch.rand(B, N, generator=g) < 0.1] = NEG_INF
        return z, None
    raise ValueError(family)


def labels(B: int, N: int, seed: int, mode: str = "in", k: int = 0, peak: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 labels.  "in": all in range (every other row on the peak when one is given).  "out": the rows r with
    r % 3 != 1 take out_of_range(N)[(r + k) % 6]."""
    y = torch.randint(0, N, (B,), generator=_gen(seed))
    r = torch.arange(B)
    if peak is not None:
        y = torch.where(r % 4 < 2, peak, y)
    if mode == "out":
        oor = torch.tensor(out_of_range(N), dtype=torch.int64)
        y = torch.where(r % 3 != 1, oor[(r + k) % 6], y)
    return y


def unmask_labels(z: torch.Tensor, *ys: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """The `masked` family never has -inf at a label: such entries get a finite value back."""
    B, N = z.shape
    z = z.clone()
    fresh = 3.0 * torch.randn(B, generator=_gen(seed + 99))
    for y in ys:
        ok = (y >= 0) & (y < N)
        rows = torch.arange(B)[ok]
        cols = y[ok]
        bad = z[rows, cols] == NEG_INF
        z[rows[bad], cols[bad]] = fresh[rows[bad]]
    return z


# (name, lam per row (None = cycle 0, 0.3, 1), eps, label mode of y, of y2, y2 == y)
SOFT_CONFIGS = [("lam.3_eps.1_in", 0.3, 0.1, "in", "in", False),
                ("lam0_eps0_yout", 0.0, 0.0, "out", "in", False),
                ("lam1_eps.1_y2out", 1.0, 0.1, "in", "out", False),
                ("lam.3_eps0_bothout", 0.3, 0.0, "out", "out", False),
                ("lammix_eps.1_same", None, 0.1, "in", "in", True),
                ("lammix_eps0_yout", None, 0.0, "out", "in", False)]
HARD_CONFIGS = [("in", "in", 0), ("out0", "out", 0), ("out1", "out", 1)]


def soft_case(family: str, B: int, N: int, cfg, seed: int) -> Optional[Dict]:
    name, lam, eps, my, my2, same = cfg
    if family == "masked" and eps != 0.0:
        return None
    z, pk = logits(family, B, N, seed)
    y = labels(B, N, seed + 1, my, 0, pk)
    y2 = y.clone() if same else labels(B, N, seed + 2, my2, 3, None)
    lam_t = torch.tensor([0.0, 0.3, 1.0])[torch.arange(B) % 3] if lam is None else torch.full((B,), lam)
    if family == "masked":
        z = unmask_labels(z, y, y2, seed=seed)
    return {"z": z, "y": y, "y2": y2, "lam": lam_t.float(), "eps": eps, "name": f"{family} {name}"}


def hard_case(family: str, B: int, N: int, cfg, seed: int) -> Optional[Dict]:
    name, mode, k = cfg
    z, pk = logits(family, B, N, seed)
    y = labels(B, N, seed + 1, mode, k, pk)
    if family == "masked":
        if mode != "in":
            return None                      # (a row without a valid label could be masked entirely)
        z = unmask_labels(z, y, seed=seed)
    return {"z": z, "y": y, "y2": None, "lam": None, "eps": 0.0, "name": f"{family} {name}"}


def families_of(B: int, N: int):
    return ("counting",) if (B, N) == CE_COUNTING_ONLY else CE_FAMILIES


# ------------------------------------------------------------------------------------------------ cross-entropy
def narrow32(y: torch.Tensor) -> torch.Tensor:
    """what (int)label keeps of an int64 label"""
    return ((y + 2 ** 31) % 2 ** 32) - 2 ** 31


def _label(y: torch.Tensor, N: int, mutant: Optional[str]):
    if mutant == "narrow32":
        y = narrow32(y)
    ok = (y >= 0) & (y < N)
    return ok, torch.where(ok, y, torch.zeros_like(y))


def _weighted(w: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return torch.where(w != 0, w * torch.where(w != 0, v, torch.zeros_like(v)), torch.zeros_like(v))


def ce_eval(c: Dict, dtype=F64, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """rowloss [B], loss [] and dlogits [B, N] of the hard (c["y2"] is None) or the soft loss."""
    z = c["z"].to(dtype)
    B, N = z.shape
    r = torch.arange(B)
    if mutant == "no_max":
        mx = torch.zeros(B, dtype=dtype)
    elif mutant == "max_first256":
        mx = z[:, :256].max(dim=1).values
    else:
        mx = z.max(dim=1).values
    p = torch.exp(z - mx[:, None])
    s = (p[:, :-1] if mutant == "drop_last_col" else p).sum(dim=1)
    lse = mx + torch.log(s)
    ok, yc = _label(c["y"], N, mutant)
    zy = torch.where(ok, z[r, yc], torch.zeros(B, dtype=dtype))
    oh = torch.zeros(B, N, dtype=dtype)
    oh[r[ok], yc[ok]] = 1.0
    if c["y2"] is None:
        rowloss = torch.where(ok, lse - zy, torch.zeros(B, dtype=dtype))
        t = oh
        valid = ok
    else:
        eps = torch.tensor(c["eps"], dtype=F32).to(dtype)
        lam = c["lam"].to(dtype)
        om = 1.0 - lam
        if mutant == "lam_swapped":
            lam, om = om, lam
        keep = 1.0 - eps
        ok2, yc2 = _label(c["y2"], N, mutant)
        zy2 = torch.where(ok2, z[r, yc2], torch.zeros(B, dtype=dtype))
        oh2 = torch.zeros(B, N, dtype=dtype)
        oh2[r[ok2], yc2[ok2]] = 1.0
        rowloss = lse - keep * (_weighted(lam, zy) + _weighted(om, zy2))
        t = (lam[:, None] * oh + om[:, None] * oh2) * keep
        if c["eps"] != 0.0:
            mean = z.sum(dim=1) / (N - 1 if mutant == "smooth_nm1" else N)
            rowloss = rowloss - eps * mean
            t = t + eps / N
        valid = torch.ones(B, dtype=torch.bool)
    summed = rowloss[:256] if mutant == "rowloss_first256" else rowloss
    den = valid.sum().to(dtype) if mutant == "div_valid" else B
    loss = summed.sum() / den
    inv = 1.0 / s
    dl = (p * inv[:, None] - t) * torch.tensor(1.0 / B, dtype=dtype)
    return {"rowloss": rowloss, "loss": loss, "dlogits": dl}


def _lse_parts(z: torch.Tensor):
    """fp64 pieces and error bounds of p, s and lse for the rows of z [B, N] (fp64)."""
    mx = z.max(dim=1).values
    d = z - mx[:, None]
    p = torch.exp(d)
    dabs = torch.where(p > 0, d.abs(), torch.zeros_like(d))
    e_p = p * U32 * (dabs + LIB) + FTZ * ((p > 0) & (p < FTZ))
    s = p.sum(dim=1)
    e_s = red(z.shape[1], s) + e_p.sum(dim=1)
    ln_s = torch.log(s)
    e_lse = LIB * U32 * ln_s.abs() + e_s / s + U32 * (mx.abs() + ln_s.abs())
    return mx, p, e_p, s, e_s, mx + ln_s, e_lse


def ce_bounds(c: Dict, ref: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    z = c["z"].double()
    B, N = z.shape
    r = torch.arange(B)
    mx, p, e_p, s, e_s, lse, e_lse = _lse_parts(z)
    ok, yc = _label(c["y"], N, None)
    zy = torch.where(ok, z[r, yc], torch.zeros(B, dtype=F64))
    oh = torch.zeros(B, N, dtype=F64)
    oh[r[ok], yc[ok]] = 1.0
    if c["y2"] is None:
        e_row = torch.where(ok, e_lse + U32 * (lse.abs() + zy.abs()), torch.zeros(B, dtype=F64))
        t, c_t = oh, 0.0
    else:
        eps = torch.tensor(c["eps"], dtype=F32).double()
        lam = c["lam"].double()
        keep = 1.0 - eps
        ok2, yc2 = _label(c["y2"], N, None)
        zy2 = torch.where(ok2, z[r, yc2], torch.zeros(B, dtype=F64))
        oh2 = torch.zeros(B, N, dtype=F64)
        oh2[r[ok2], yc2[ok2]] = 1.0
        mag = lse.abs() + (keep * _weighted(lam, zy)).abs() + (keep * _weighted(1.0 - lam, zy2)).abs()
        e_row = e_lse
        if c["eps"] != 0.0:
            mean = z.sum(dim=1) / N
            e_mean = red(N, z.abs().sum(dim=1)) / N + LIB * U32 * mean.abs()
            mag = mag + (eps * mean).abs()
            e_row = e_row + eps * e_mean
        e_row = e_row + 7 * U32 * mag
        t = (lam[:, None] * oh + (1.0 - lam)[:, None] * oh2) * keep + (eps / N if c["eps"] != 0.0 else 0.0)
        c_t = 5.0
    rl = ref["rowloss"].double()
    e_loss = red(B, rl.abs().sum()) / B + e_row.mean() + LIB * U32 * ref["loss"].double().abs()
    sm = p / s[:, None]
    e_dl = (e_p / s[:, None] + sm * (e_s / s + LIB * U32)[:, None] + c_t * U32 * t + 2 * U32 * (sm + t)
            + (LIB + 1) * U32 * (sm - t).abs()) / B
    q = (sm - t).abs() / B
    e_dl = e_dl + FTZ * ((sm > 0) & (sm < 2 * FTZ)) / B + FTZ * ((q > 0) & (q < 2 * FTZ))
    return {"rowloss": e_row, "loss": e_loss, "dlogits": e_dl}


# ------------------------------------------------------------------------------------------------ evaluation metrics
def eval_logits(family: str, B: int, N: int, seed: int) -> torch.Tensor:
    """levels: row b is a random permutation of the N distinct levels (j + u_b) 12 / N - 6; shifted: the same plus the
    per-row offsets of SHIFTS; counting: all logits of a row equal (every comparison a tie)."""
    g = _gen(seed)
    r = torch.arange(B)
    if family == "counting":
        return ((r % 7 - 3).float() * 2.5)[:, None].expand(B, N).contiguous()
    perm = torch.argsort(torch.rand(B, N, generator=g), dim=1).double()
    x = ((perm + torch.rand(B, 1, generator=g).double()) * (12.0 / N) - 6.0).float()
    if family == "shifted":
        x = x + torch.tensor(SHIFTS)[r % 4][:, None]
    return x


def eval_labels(z: torch.Tensor, seed: int, mode: str = "in", k: int = 0) -> torch.Tensor:
    """rows in turn: the largest logit, the third, the fifth, the sixth largest (a top-1 hit, two top-5-only hits, a
    miss, as far as N allows), a random class."""
    B, N = z.shape
    order = z.argsort(dim=1, descending=True, stable=True)
    r = torch.arange(B)
    place = torch.tensor([0, 2, 4, 5])[r % 5 % 4].clamp(max=N - 1)
    y = torch.where(r % 5 == 4, torch.randint(0, N, (B,), generator=_gen(seed)), order[r, place])
    if mode == "out":
        oor = torch.tensor(out_of_range(N), dtype=torch.int64)
        y = torch.where(r % 3 != 1, oor[(r + k) % 6], y)
    return y


def ranks(z: torch.Tensor, y: torch.Tensor, mutant: Optional[str] = None):
    """(label in range, rank of the label's logit) from the definition above."""
    B, N = z.shape
    ok, yc = _label(y, N, mutant)
    ly = z[torch.arange(B), yc][:, None]
    n = torch.arange(N)[None, :]
    first = (n > yc[:, None]) if mutant == "tie_high" else (n < yc[:, None])
    vn, ln = torch.isnan(z), torch.isnan(ly)
    beats = torch.where(ln, vn & first, vn | (z > ly) | ((z == ly) & first))
    return ok, beats.sum(dim=1)


def percent(count: int, B: int) -> torch.Tensor:
    """the stored fp32 value: 100.0f * (float)count / (float)B"""
    return torch.tensor(float(count), dtype=F32) * 100.0 / B


def eval_metrics_eval(z: torch.Tensor, y: torch.Tensor, dtype=F64, mutant: Optional[str] = None):
    """(batch loss [] of dtype, #top-1, #top-k) of one batch."""
    B, N = z.shape
    ok, rank = ranks(z, y, mutant)
    maxk = min(5, N)
    zz = z.to(dtype)
    mx = zz.max(dim=1).values
    lse = mx + torch.log(torch.exp(zz - mx[:, None]).sum(dim=1))
    _, yc = _label(y, N, mutant)
    row = torch.where(ok, lse - zz[torch.arange(B), yc], torch.zeros(B, dtype=dtype))
    c1 = int((ok & (rank < 1)).sum())
    ck = int((ok & ((rank <= maxk) if mutant == "rank_le_maxk" else (rank < maxk))).sum())
    return row.sum() / B, c1, ck


def eval_metrics_bounds(z: torch.Tensor, y: torch.Tensor, acc_before: float = 0.0) -> torch.Tensor:
    z = z.double()
    B, N = z.shape
    _, _, _, _, _, lse, e_lse = _lse_parts(z)
    ok, yc = _label(y, N, None)
    zy = z[torch.arange(B), yc]
    row = torch.where(ok, lse - zy, torch.zeros(B, dtype=F64))
    e_row = torch.where(ok, e_lse + U32 * (lse.abs() + zy.abs()), torch.zeros(B, dtype=F64))
    loss = row.sum() / B
    return red(B, row.abs().sum()) / B + e_row.mean() + LIB * U32 * loss.abs() + U32 * (abs(acc_before) + loss.abs())


def topk_counts(z: torch.Tensor, y: torch.Tensor) -> Tuple[int, int]:
    """(#top-1, #top-k) as the reference trainer counts them with torch.topk (labels in range)."""
    maxk = min(5, z.shape[1])
    pred = z.topk(maxk, 1, True, True).indices
    hit = pred.eq(y[:, None])
    return int(hit[:, 0].sum()), int(hit.sum())


def nan_rows(N: int, seed: int):
    """Rows with one NaN on, before and after the label (each with the label otherwise ranked first and ranked
    fourth), and rows with two NaNs: the label's own and one before / after it.  Returns (z, y, #NaN per row)."""
    assert N >= 8
    R, lab = 10, N // 2
    z = eval_logits("levels", R, N, seed)
    nan, before, after = float("nan"), lab - 3, lab + 2
    free = torch.tensor([c for c in range(N) if c not in (lab, before, after)])
    for i in range(R):           # the label's column gets the largest / fourth largest, the two NaN places the smallest
        vals = z[i].sort(descending=True).values
        pick = 0 if i % 2 == 0 else 3
        z[i, lab], z[i, before], z[i, after] = vals[pick], vals[N - 1], vals[N - 2]
        z[i, free] = vals[torch.tensor([j for j in range(N - 2) if j != pick])]
    y = torch.full((R,), lab, dtype=torch.int64)
    z[0, lab] = z[1, lab] = nan                                 # on the label
    z[2, before] = z[3, before] = nan
    z[4, after] = z[5, after] = nan
    z[6, lab] = z[6, before] = nan                              # two NaNs: the earlier one wins
    z[7, lab] = z[7, after] = nan
    return z, y, torch.isnan(z).sum(dim=1)                      # rows 8 and 9 stay free of NaN


# ------------------------------------------------------------------------------------------------ mutants
CE_MUTANTS = ("no_max", "max_first256", "drop_last_col", "rowloss_first256", "div_valid", "narrow32", "smooth_nm1",
              "lam_swapped")
EVAL_MUTANTS = ("tie_high", "rank_le_maxk", "narrow32")
