"""Reference arithmetic of the weight EMA (nvit_ema_tick / nvit_ema_update, nvit_amd/ema.py) in numpy.

The device computes the decay of update t (t counted from 0) in fp64 and stores omd = (float)(1 - d); the update is
e <- fma(omd, p - e, e) in fp32.  Here: the decay formula, one update and the whole recurrence in float64 (the
reference the GPU tests compare with) and in float32 (the same order of operations, for orientation), both with `omd`
given, and the per-update error bound."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32


def decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """d of the update that follows t applied ones: timm's warm-up min(decay, (1 + t) / (10 + t)), or decay."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def omd_at(t: int, decay: float, warmup: bool = True) -> np.float32:
    """What nvit_ema_tick stores: every fp64 operation is correctly rounded on both sides, and so is the conversion."""
    return np.float32(1.0 - decay_at(t, decay, warmup))


def update64(e, p, omd) -> np.ndarray:
    """One update in float64 from the given (fp32 or fp64) e, p and the fp32 omd."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + np.float64(np.float32(omd)) * (p - e)


def update32(e, p, omd) -> np.ndarray:
    """One update in float32 in the kernel's order: the difference rounded to fp32, then a fused multiply-add (the
    product of two fp32 is exact in fp64; the sum is rounded to fp64 and then to fp32, which differs from the single
    rounding of a hardware fma only in rare double-rounding ties)."""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = (p - e).astype(np.float64)
    return (np.float64(np.float32(omd)) * d + e.astype(np.float64)).astype(np.float32)


def recurrence(e0, weights, omds, dtype=np.float64) -> np.ndarray:
    """e after len(weights) updates: weights[k] is p at update k, omds[k] the fp32 factor the device used for it."""
    step = update64 if dtype == np.float64 else update32
    e = np.asarray(e0, dtype=dtype)
    for p, omd in zip(weights, omds):
        e = step(e, p, omd)
    return e


def update_bound(e, p) -> np.ndarray:
    """|e_gpu - e_fp64| <= 2^-23 (|e| + |p|) after one update from identical fp32 e, p and omd <= 1: the difference is
    rounded once (<= U |p - e| <= U (|e| + |p|), then scaled by omd <= 1) and the fused multiply-add once (<= U |result|,
    the result lying between e and p, so <= U max(|e|, |p|) <= U (|e| + |p|)).  When one of e, p is zero the difference
    is exact and U max(|e|, |p|) alone remains; e == p gives a zero difference and e back bit for bit."""
    return 2.0 * U * (np.abs(np.asarray(e, dtype=np.float64)) + np.abs(np.asarray(p, dtype=np.float64)))
