"""Mixup / CutMix on the device, and the soft targets (with label smoothing) that go with them.

The batch-level half of the DeiT / timm training recipe (mixup 0.8, cutmix 1.0, smoothing 0.1) as two HIP launches per
batch (nvit_mix_draw, nvit_mix_apply) plus a soft-target loss (nvit_ce_loss_soft), without host synchronisation, so that
it sits inside a captured train step.  Semantics (tests/mix_ref.py restates them in numpy): timm's `pair`
mode - row i of the batch is mixed with row B-1-i, one draw per pair - with timm's `rand_bbox` / `correct_lam` for the
CutMix box and timm's `mixup_target` for the target.

The draw is the counter-based generator of augment.py (Philox4x32-10; key = seed with a domain constant in its high
word, counter = (first_index + pair, step)); the step counter lives on the device and the draw kernel advances it, so a
replayed graph draws afresh.  lambda ~ Beta(alpha, alpha) comes from a quantile table of KNOTS + 1 values that the host
computes in fp64 (`beta_quantile_table`) and the kernel interpolates linearly: no transcendental runs on the device.
"""
from __future__ import annotations

import functools
import math
import struct
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import call
from .augment import MAX_SIDE, _f32_bits
from .ops import _chk_dev, _s
from .stages import DeviceStepCounter, StagedBatch, check_f32_batch, check_number, check_sides, check_unit

Tensor = torch.Tensor

KNOTS = _lib.const("MIX_KNOTS")   # the quantile table holds KNOTS + 1 values: Q[k] = F^-1(k / KNOTS)
ROW = _lib.const("MIX_ROW")       # ints per row of the table: mode, lambda bits, y0, y1, x0, x1, partner row, 0
MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2
ALPHA_MIN, ALPHA_MAX = 0.1, 4.0


# ---------------------------------------------------------------------------------------------- Beta quantiles (fp64)
def _betacf(a: float, b: float, x: float) -> float:
    """The continued fraction of the incomplete beta function (modified Lentz), for x < (a + 1) / (a + b + 2)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 2000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        de = d * c
        h *= de
        if abs(de - 1.0) <= 2.5e-16:
            return h
    raise ArithmeticError(f"incomplete beta: no convergence at a={a}, x={x}")


def _log_pdf_cdf(a: float, lnB: float, t: float):
    """(log pdf, cdf) of Beta(a, a) at x = exp(t) <= 1/2."""
    x = math.exp(t)
    lf = a * t + a * math.log1p(-x) - lnB            # log of x^a (1-x)^a / B(a,a)
    return lf - t - math.log1p(-x), math.exp(lf) / a * _betacf(a, a, x)


@functools.lru_cache(maxsize=None)
def beta_quantile_table(alpha: float) -> tuple:
    """Q[k] = the k/KNOTS quantile of Beta(alpha, alpha), k = 0..KNOTS, in fp64: Q[0] = 0, Q[KNOTS / 2] = 1/2, Q[KNOTS] = 1,
    Q[KNOTS - k] = 1 - Q[k].  The lower half is solved in t = log x (where the small quantiles of a small alpha live:
    7e-28 at alpha = 0.1) by Newton steps on log I_x = log p, kept inside a bisection bracket; I_x is the
    continued-fraction regularised incomplete beta.  Plain Python floats; accurate to a few ulp."""
    a = float(alpha)
    if not ALPHA_MIN <= a <= ALPHA_MAX:
        raise ValueError(f"alpha must be in [{ALPHA_MIN}, {ALPHA_MAX}] (got {alpha!r})")
    q = [0.0] * (KNOTS + 1)
    half = KNOTS // 2
    if a == 1.0:
        for k in range(half):
            q[k] = k / KNOTS
    else:
        lnB = 2.0 * math.lgamma(a) - math.lgamma(2.0 * a)
        t_top = math.log(0.5)
        t_prev, lp_prev = None, None
        for k in range(1, half):
            lp = math.log(k / KNOTS)
            lo = -745.0 if t_prev is None else t_prev
            hi = t_top
            # I_x ~ x^a / (a B) for small x: exact slope in log-log there
            t = (lp + math.log(a) + lnB) / a if t_prev is None else t_prev + (lp - lp_prev) / a
            t = min(max(t, lo), hi)
            for _ in range(200):
                lpdf, cdf = _log_pdf_cdf(a, lnB, t)
                if cdf <= 0.0:
                    lo, t = t, 0.5 * (t + hi)
                    continue
                err = math.log(cdf) - lp
                if err > 0.0:
                    hi = t
                else:
                    lo = t
                # d log I / dt = pdf * x / I
                step = err * cdf / math.exp(lpdf + t)
                tn = t - step
                if not lo < tn < hi:
                    tn = 0.5 * (lo + hi)
                if abs(tn - t) <= 4e-16 * max(1.0, abs(t)) or hi - lo <= 4e-16 * max(1.0, abs(t)):
                    t = tn
                    break
                t = tn
            else:
                raise ArithmeticError(f"beta quantile: no convergence at alpha={a}, k={k}")
            q[k] = math.exp(t)
            t_prev, lp_prev = t, lp
    q[half] = 0.5
    for k in range(half):
        q[KNOTS - k] = 1.0 - q[k]
    return tuple(q)


def _f32(v: float) -> float:
    return struct.unpack("<f", struct.pack("<f", v))[0]


# ---------------------------------------------------------------------------------------------- argument checks
def _check_alpha(what: str, a) -> float:
    if check_number(what, a) != 0 and not ALPHA_MIN <= a <= ALPHA_MAX:   # also refuses NaN
        raise ValueError(f"{what} must be 0 (off) or in [{ALPHA_MIN}, {ALPHA_MAX}] (got {a!r})")
    return float(a)


def _check_images(X) -> tuple:
    return check_f32_batch("Mixup", X, MAX_SIDE)


def _check_hw(H, W) -> None:
    check_sides("Mixup", H, W, MAX_SIDE)


def _check_labels(y, B: Optional[int] = None) -> int:
    if not isinstance(y, Tensor) or y.dtype != torch.int64:
        raise TypeError("Mixup takes int64 [B] labels")
    if y.dim() != 1 or y.shape[0] < 1 or (B is not None and y.shape[0] != B):
        raise ValueError(f"Mixup takes int64 [B] labels, one per image (got shape {tuple(y.shape)}"
                         + (f" for a batch of {B})" if B is not None else ")"))
    return y.shape[0]


class MixedTargets:
    """Soft targets of a batch: row b's target is (1 - smoothing) * (lam[b] * e[y[b]] + (1 - lam[b]) * e[y2[b]]) +
    smoothing / N.  y, y2 int64 [B], lam fp32 [B].  Goes where the int64 labels go in `train.total_loss` /
    `CrossEntropyFn`; `targets[i:j]` slices the rows (a micro-batch)."""

    def __init__(self, y: Tensor, y2: Tensor, lam: Tensor, smoothing: float = 0.0):
        for what, t, dt in (("y", y, torch.int64), ("y2", y2, torch.int64), ("lam", lam, torch.float32)):
            if not isinstance(t, Tensor) or t.dtype != dt:
                raise TypeError(f"MixedTargets: {what} must be a {str(dt).replace('torch.', '')} tensor")
        if y.dim() != 1 or y2.shape != y.shape or lam.shape != y.shape:
            raise ValueError("MixedTargets: y, y2 and lam must be [B]")
        self.y, self.y2, self.lam = y, y2, lam
        self.smoothing = check_unit("smoothing", smoothing, open_top=True)

    @property
    def shape(self):
        return self.y.shape

    @property
    def device(self):
        return self.y.device

    def __len__(self) -> int:
        return self.y.shape[0]

    def __getitem__(self, rows) -> "MixedTargets":
        if not isinstance(rows, slice):
            raise TypeError("MixedTargets supports row slices only")
        return MixedTargets(self.y[rows], self.y2[rows], self.lam[rows], self.smoothing)

    def to(self, device) -> "MixedTargets":
        return MixedTargets(self.y.to(device), self.y2.to(device), self.lam.to(device), self.smoothing)


class MixedBatch(StagedBatch):
    """A batch together with the Mixup that mixes it inside the step: what `Mixup.batch(X)` returns and `train_step` /
    `GraphedTrainStep` accept in place of X.  X: an fp32 [B,C,H,W] tensor, an `AutoAugment.batch(u8)`, or a
    `RandomErasing.batch(...)` (crop.py).  `.shape` is X's."""

    key, word, accepts, names = "mix", "Mixup", ("augment", "erase"), ("mix", "X")

    def __init__(self, mix: "Mixup", X):
        self.B = X.shape[0] if self.takes(X) else _check_images(X)[0]
        super().__init__(mix, X, X.shape)

    def check_labels(self, y) -> None:
        _check_labels(self.labels() if y is None else y, self.B)   # (y None: those of a loader batch inside, if there is one)

    def resolve(self, y=None):
        self.check_labels(y)   # before any launch of what X carries
        return super().resolve(y)

    def _run(self, x: Tensor, y, inplace: bool):
        return self.mix(x, y, inplace=inplace)

    def mixed(self, y: Tensor):
        """(X', MixedTargets): the launches of what X carries, then the draw and the apply."""
        return self.resolve(y)


class Mixup(DeviceStepCounter):
    """Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, seed=0,
    first_index=0).to(device)

    Per pair (rows p and B-1-p of the batch the call receives; the middle row of an odd batch stays as it is): with
    probability `prob` the pair is mixed, by CutMix with probability `switch_prob` and by Mixup otherwise (always the
    one whose alpha is > 0 when the other's is 0), at lambda ~ Beta(alpha, alpha).  alpha: 0 (off) or 0.1..4.
    first_index: the global index of this batch's first PAIR in the step; a data-parallel rank passes rank * ((B + 1) // 2)
    so that the ranks draw from disjoint counters.  Pairs are formed inside the batch a call receives, so - unlike
    AutoAugment - the result is not invariant to how a step's batch is split over ranks.

    `mix(X, y)` returns (X', MixedTargets); `draw` and `apply` are its two halves; `targets_for` writes a table by
    hand.  With both alphas 0 no image kernel runs and X' is X: label smoothing alone."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0, switch_prob: float = 0.5,
                 label_smoothing: float = 0.1, seed: int = 0, first_index: int = 0):
        self.mixup_alpha = _check_alpha("mixup_alpha", mixup_alpha)
        self.cutmix_alpha = _check_alpha("cutmix_alpha", cutmix_alpha)
        self.prob = check_unit("prob", prob)
        self.switch_prob = check_unit("switch_prob", switch_prob)
        self.label_smoothing = check_unit("label_smoothing", label_smoothing, open_top=True)
        super().__init__(seed, first_index)
        self._q_mix: Optional[Tensor] = None
        self._q_cut: Optional[Tensor] = None

    @property
    def mixes_images(self) -> bool:
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    # ------------------------------------------------------------------ device state
    def to(self, device) -> "Mixup":
        device = self._step_to(device)

        def table(alpha):
            if alpha == 0:
                return None
            return torch.tensor(beta_quantile_table(alpha), dtype=torch.float64).to(torch.float32).to(device)

        self._q_mix, self._q_cut = table(self.mixup_alpha), table(self.cutmix_alpha)
        return self

    # ------------------------------------------------------------------ the two launches
    def draw(self, y: Tensor, H: int, W: int):
        """(table int32 [B,8], MixedTargets) of the next step (nvit_mix_draw); advances the step counter."""
        B = _check_labels(y)
        _check_hw(H, W)
        self._need_device()
        _chk_dev(y)
        y = y.contiguous()
        table = torch.empty((B, ROW), device=y.device, dtype=torch.int32)
        lam = torch.empty(B, device=y.device, dtype=torch.float32)
        y2 = torch.empty_like(y)
        call("nvit_mix_draw", self.seed, self._step, self.first_index, self._q_mix, self._q_cut, self.prob, self.switch_prob,
             y, table, lam, y2, B, H, W, _s())
        return table, MixedTargets(y, y2, lam, self.label_smoothing)

    def apply(self, X: Tensor, table: Tensor, inplace: bool = False) -> Tensor:
        """The mixed fp32 [B,C,H,W] batch (nvit_mix_apply).  Out of place unless `inplace` (then X itself is returned,
        mixed): a caller's tensor is never modified behind their back."""
        B, C, H, W = _check_images(X)
        if not isinstance(table, Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (B, ROW):
            raise ValueError(f"Mixup.apply: the table must be int32 [{B},{ROW}]")
        _chk_dev(X, table)
        if inplace and not X.is_contiguous():
            raise ValueError("Mixup.apply: in place needs a contiguous batch")
        X, table = X.contiguous(), table.contiguous()
        out = X if inplace else torch.empty_like(X)
        call("nvit_mix_apply", X, table, out, B, C, H, W, _s())
        return out

    def __call__(self, X: Tensor, y: Tensor, inplace: bool = False):
        B, C, H, W = _check_images(X)
        _check_labels(y, B)
        _chk_dev(X, y)
        table, targets = self.draw(y, H, W)
        if not self.mixes_images:
            return X, targets   # every row is mode 0: label smoothing alone, no image kernel
        return self.apply(X, table, inplace=inplace), targets

    def batch(self, X) -> MixedBatch:
        """The X of `train_step(model, optimizer, mix.batch(X), y)` and of `GraphedTrainStep`: draw and apply run inside
        the step (and inside its captured graph), once per batch.  X: fp32 [B,C,H,W] or an `AutoAugment.batch(u8)`."""
        return MixedBatch(self, X)

    # ------------------------------------------------------------------ tables by hand
    def targets_for(self, y: Sequence, pairs: Sequence, H: int, W: int):
        """(table int32 [B,8], MixedTargets) written by hand, as the draw would write them: y the B labels, pairs[p] what
        happens to rows p and B-1-p: None (not mixed), ("mixup", lam), or ("cutmix", (y0, y1, x0, x1)) whose lambda is
        1 - area / (H*W) as the draw kernel computes it.  len(pairs) == B // 2; the middle row of an odd B is not mixed.
        The targets carry this object's label_smoothing."""
        _check_hw(H, W)
        y = [int(v) for v in (y.tolist() if isinstance(y, Tensor) else y)]
        B = len(y)
        pairs = list(pairs)
        if B < 1 or len(pairs) != B // 2:
            raise ValueError(f"targets_for: {B} labels need {B // 2} pairs (got {len(pairs)})")
        rows = [[MODE_NONE, _f32_bits(1.0), 0, 0, 0, 0, b, 0] for b in range(B)]
        lam = [1.0] * B
        y2 = list(y)
        for p, spec in enumerate(pairs):
            i, j = p, B - 1 - p
            box = (0, 0, 0, 0)
            if spec is None:
                mode, l = MODE_NONE, 1.0
            else:
                kind, arg = spec
                if kind == "mixup":
                    if not 0.0 <= float(arg) <= 1.0:
                        raise ValueError(f"targets_for: lambda {arg!r} outside [0,1]")
                    mode, l = MODE_MIXUP, _f32(float(arg))
                elif kind == "cutmix":
                    box = tuple(int(v) for v in arg)
                    if len(box) != 4 or not (0 <= box[0] <= box[1] <= H and 0 <= box[2] <= box[3] <= W):
                        raise ValueError(f"targets_for: box {arg!r} must be 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W")
                    mode = MODE_CUTMIX
                    l = _f32(1.0 - float((box[1] - box[0]) * (box[3] - box[2])) / float(H * W))
                else:
                    raise ValueError(f"targets_for: a pair is None, ('mixup', lam) or ('cutmix', box) (got {spec!r})")
            for b, partner in ((i, j), (j, i)):
                rows[b] = [mode, _f32_bits(l), *box, partner, 0]
                lam[b] = l
                y2[b] = y[partner]
        table = torch.tensor(rows, dtype=torch.int32)
        targets = MixedTargets(torch.tensor(y, dtype=torch.int64), torch.tensor(y2, dtype=torch.int64),
                               torch.tensor(lam, dtype=torch.float32), self.label_smoothing)
        if self.device is not None:
            table, targets = table.to(self.device), targets.to(self.device)
        return table, targets
