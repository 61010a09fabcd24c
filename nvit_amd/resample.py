"""Resampling a square position-embedding table to another token grid (timm's resample_abs_pos_embed): the host side.

The target is F.interpolate(p.reshape(1,g,g,C).permute(0,3,1,2), size=(g2,g2), mode="bicubic", align_corners=False,
antialias=True).  That operator is separable, out = (W (x) W) p with one [g2, g] matrix W per axis, and W is sparse: row o
holds the cubic (a = -0.5) filter sampled around the centre (o + 0.5) * g / g2, 4 taps wide when enlarging and
4 * g / g2 wide when shrinking, clipped to the table's edges and normalised to sum 1.  `tap_rows` computes W in fp64,
`transposed_rows` its transpose (the backward reads it: dP = (W^T (x) W^T) dOut, a gather like the forward, so every
element is written once and in a fixed order), `tap_tables` packs both for the kernels and caches them per device.

Packed layout, int32 [rows, 2 + MAX_TAPS]: row r = (first source index, tap count, the weights as fp32 bit patterns,
zeros behind the last tap).  MAX_TAPS is NVIT_POS_RESAMPLE_MAX_TAPS of the C header.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib

MAX_TAPS = _lib.const("POS_RESAMPLE_MAX_TAPS")
ROW = 2 + MAX_TAPS
Rows = Tuple[List[int], List[List[float]]]   # (first source index per row, the row's weights)


def _cubic(x: float) -> float:
    """Keys' cubic convolution kernel with a = -0.5 (the antialiasing filter of torch and Pillow)."""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def check_grids(g: int, g2: int) -> None:
    for name, v in (("g", g), ("g2", g2)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"pos_resample: grid side {name} must be an int >= 1 (got {v!r})")


def tap_rows(g: int, g2: int) -> Rows:
    """W [g2, g] of one axis in fp64, row o as (first[o], weights[o]); align_corners=False, antialias=True."""
    check_grids(g, g2)
    scale = g / g2
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    first, weights = [], []
    for o in range(g2):
        center = scale * (o + 0.5)
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), g) - lo
        w = [_cubic((j + lo - center + 0.5) * inv) for j in range(n)]
        total = 0.0
        for v in w:
            total += v
        first.append(lo)
        weights.append([v / total for v in w] if total != 0.0 else w)
    return first, weights


def transposed_rows(rows: Rows, g: int) -> Rows:
    """W^T [g, g2] of `rows` = W [g2, g]: row i lists W[o, i] over the outputs o that read source i (an interval, since
    first and end of W's rows ascend; an o inside it that does not read i contributes an exact 0)."""
    first, weights = rows
    tfirst, tweights = [], []
    for i in range(g):
        hit = [o for o in range(len(first)) if first[o] <= i < first[o] + len(weights[o])]
        if not hit:
            tfirst.append(0)
            tweights.append([])
            continue
        tfirst.append(hit[0])
        tweights.append([weights[o][i - first[o]] if first[o] <= i < first[o] + len(weights[o]) else 0.0
                         for o in range(hit[0], hit[-1] + 1)])
    return tfirst, tweights


def dense(rows: Rows, n_src: int) -> np.ndarray:
    """The fp64 matrix [rows, n_src] that `rows` stands for."""
    first, weights = rows
    W = np.zeros((len(first), n_src), dtype=np.float64)
    for o, (lo, w) in enumerate(zip(first, weights)):
        W[o, lo:lo + len(w)] = w
    return W


def max_taps(rows: Rows) -> int:
    return max((len(w) for w in rows[1]), default=0)


def pack(rows: Rows) -> np.ndarray:
    """int32 [rows, ROW] as the kernels read it; the weights rounded to fp32 here, once."""
    first, weights = rows
    t = np.zeros((len(first), ROW), dtype=np.int32)
    for o, (lo, w) in enumerate(zip(first, weights)):
        t[o, 0], t[o, 1] = lo, len(w)
        t[o, 2:2 + len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32).view(np.int32)
    return t


_HOST: Dict[Tuple[int, int], Tuple[Rows, Rows]] = {}
_DEVICE: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor]] = {}


def host_tables(g: int, g2: int) -> Tuple[Rows, Rows]:
    """(W, W^T) of g -> g2 in fp64, cached.  ValueError when a row of either needs more than MAX_TAPS taps: the forward's
    rows grow with g / g2 (shrinking), the transposed ones with g2 / g (enlarging)."""
    key = (g, g2)
    if key not in _HOST:
        fwd = tap_rows(g, g2)
        bwd = transposed_rows(fwd, g)
        need = max(max_taps(fwd), max_taps(bwd))
        if need > MAX_TAPS:
            raise ValueError(f"pos_resample: grid {g} -> {g2} needs {need} taps per row, the kernels hold {MAX_TAPS} "
                             f"(a ratio of about {MAX_TAPS // 4} either way)")
        _HOST[key] = (fwd, bwd)
    return _HOST[key]


def tap_tables(g: int, g2: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(forward table int32 [g2, ROW], transposed table int32 [g, ROW]) on `device`, sent once per (g, g2, device).  A
    first call copies from the host, so it cannot run under graph capture: the warm-up steps of a captured step make it."""
    key = (g, g2, str(device))
    if key not in _DEVICE:
        fwd, bwd = host_tables(g, g2)
        _DEVICE[key] = (torch.from_numpy(pack(fwd)).to(device), torch.from_numpy(pack(bwd)).to(device))
    return _DEVICE[key]


def grid_of(n_tokens: int) -> int:
    g = math.isqrt(n_tokens)
    if n_tokens < 1 or g * g != n_tokens:
        raise ValueError(f"pos_resample: {n_tokens} tokens are no square grid")
    return g
