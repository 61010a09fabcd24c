"""Oracles of the row-kernel tests (a plain helper module; test_rowops_check.py checks it on the CPU,
test_gpu_rowops.py uses it against the HIP kernels of rowops.hip).

Every operation has an `*_eval(inputs, dtype)`: the operation in plain torch math, written from what it means (with
oracle.nvit_oracle's lerp / nrm / heads), the gradients from autograd of that forward.  At dtype=float64 it is the
reference; at float32 it is the "correct kernel in fp32" that the CPU test holds against the bounds.  Inputs stored in
bf16 are exact inputs: the reference reads the bf16 values.

Every operation also has a `*_formula`: the steps a one-pass kernel takes (unit vectors, the projected-out gradient
(g - o <o, g>) / |r|, per-row terms of the parameter gradients), written once over an algebra that runs on plain
tensors (float64: the second reference of qknorm_bwd; float32: a second restatement) and on `Ev`, an fp64 value that
carries a first-order bound of the error of an fp32 evaluation.  `*_bounds` runs the formula on Ev and returns the
per-element bounds; its values must agree with the autograd reference (the CPU test asserts it), so a bound can not
belong to another function than the reference.  The rules of Ev are those stated at the top of kohonen_check.py, applied
operation by operation:

* a sum of n terms:      the terms' own errors + LAMBDA * sqrt(n) * U32 * sum |terms|                    (`red`)
* add / sub / mul:       the operands' errors passed on to first order + one rounding U32 * |result|
* sqrtf, division, expf: LIB roundings each (1 / sqrtf = 2 LIB)
* a Python float handed to a kernel (c_a, eps, ...) is rounded to fp32 once: U32 * |c| unless it is exact
* a bf16 output adds half a bf16 ulp (`check` does that from the output's dtype)

The kernels may contract a mul and an add into an fma (one rounding less) and sum in any order; both stay inside.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from gemm_check import U32, assert_exact, bits_equal, gauss_data, int_data   # noqa: F401  (assert_exact: for the tests)
from kohonen_check import F64, LIB, check, check_all, red                      # noqa: F401  (check, check_all likewise)
from oracle import nvit_oracle as O

F32T = torch.float32
BF16T = torch.bfloat16

# ------------------------------------------------------------------------------------------------ shapes
WIDTHS = [4, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 2044, 2048]   # one per edge of NV = 1, 2, 3, 4, 8
WIDTHS_SHORT = [4, 260, 768, 1028, 2048]
ROWS = [1, 3, 37]                       # default nblk: M = 1, 3 leave waves of the workgroup without a row
MULTI = (37, 3)                         # (M, nblk): 12 waves, 3 or 4 rows per wave, ragged end
MULTI_WIDTHS = [260, 1028]
ONE_BLOCK = (9, 1)                      # (M, nblk): 4 waves, 2 or 3 rows per wave
STRIDE_M, STRIDE_C = 8197, 64           # forward grids cap at 2048 workgroups of 4 rows: 8192 rows per sweep
QK_HEADS = [(1, 16), (3, 16), (2, 32), (5, 64), (12, 64), (5, 128), (16, 128)]   # (5, 64): a partly filled second pass
QK_BT = (2, 19)
QK_MULTI = (5, 128)
QK_STRIDE = (1, 8197, 2, 32)            # (B, T, H, d)
SWIGLU_F = [16, 48, 1024, 1040, 3072]
SWIGLU_M = [1, 77]
SWIGLU_TALL = (4099, 16)                # (M, F): 3 rows per workgroup, the last workgroup has one
CSR_NBLK = [1, 31, 32, 33, 127, 128, 129, 257, 4096]
CSR_N = [1, 31, 32, 33, 260]
CSR_N_KIND2 = [32, 96]
SENTINEL = -77.0


# ------------------------------------------------------------------------------------------------ the error algebra
class Ev:
    """fp64 value v with e >= the (first-order) error of an fp32 evaluation of the same expression."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64) if not isinstance(v, torch.Tensor) else v.detach().to(F64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def lift(x) -> "Ev":
        if isinstance(x, Ev):
            return x
        if isinstance(x, torch.Tensor):
            return Ev(x)
        x = float(x)
        exact = float(torch.tensor(x, dtype=F32T)) == x
        return Ev(torch.tensor(x, dtype=F64), torch.tensor(0.0 if exact else U32 * abs(x), dtype=F64))

    def __add__(self, o):
        o = Ev.lift(o)
        v = self.v + o.v
        return Ev(v, self.e + o.e + U32 * v.abs())

    __radd__ = __add__

    def __sub__(self, o):
        o = Ev.lift(o)
        v = self.v - o.v
        return Ev(v, self.e + o.e + U32 * v.abs())

    def __rsub__(self, o):
        return Ev.lift(o) - self

    def __mul__(self, o):
        o = Ev.lift(o)
        v = self.v * o.v
        return Ev(v, self.v.abs() * o.e + o.v.abs() * self.e + U32 * v.abs())

    __rmul__ = __mul__

    def __neg__(self):
        return Ev(-self.v, self.e)

    def map(self, fn) -> "Ev":
        """a reshape / permutation / slice of both parts"""
        return Ev(fn(self.v), fn(self.e))


def _sum(x, dim: int = -1):
    if isinstance(x, Ev):
        n = x.v.shape[dim]
        return Ev(x.v.sum(dim, keepdim=True), x.e.sum(dim, keepdim=True) + red(n, x.v.abs().sum(dim, keepdim=True)))
    return x.sum(dim, keepdim=True)


def _rsqrt(x):
    if isinstance(x, Ev):
        v = x.v ** -0.5
        return Ev(v, v * (0.5 * x.e / x.v + 2 * LIB * U32))
    return 1.0 / torch.sqrt(x)


def _recip(x):
    if isinstance(x, Ev):
        v = 1.0 / x.v
        return Ev(v, v.abs() * (x.e / x.v.abs() + LIB * U32))
    return 1.0 / x


def _divc(x, c: int):
    """division by an integer count"""
    if isinstance(x, Ev):
        return Ev(x.v / c, x.e / c + LIB * U32 * x.v.abs() / c)
    return x / c


def _exp(x):
    if isinstance(x, Ev):
        v = torch.exp(x.v)
        return Ev(v, v * (x.e + LIB * U32))
    return torch.exp(x)


def _abs(x):
    return Ev(x.v.abs(), x.e) if isinstance(x, Ev) else x.abs()


def _view(x, fn):
    return x.map(fn) if isinstance(x, Ev) else fn(x)


def _cat(xs, dim: int = -1):
    if isinstance(xs[0], Ev):
        return Ev(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim))
    return torch.cat(xs, dim)


def _as(x, dtype):
    """an input in the algebra of `dtype` ("ev", or a torch dtype)"""
    if x is None or isinstance(x, (float, int, Ev)):
        return x
    return Ev(x) if dtype == "ev" else x.detach().to(dtype)


def _split(res: Dict[str, Ev]):
    return {k: r.v for k, r in res.items()}, {k: r.e for k, r in res.items()}


def _nrm(x):
    rs = _rsqrt(_sum(x * x))
    return x * rs, rs


def _leaf(t, dtype):
    return t.detach().to(dtype).requires_grad_(True)


def _flat(x):
    return _view(x, lambda t: t.reshape(-1))


# ------------------------------------------------------------------------------------------------ data
def signed(v: torch.Tensor) -> torch.Tensor:
    """every third entry negated (fabsf and the kind-1 sign see both signs; none at zero)"""
    v = v.clone()
    v[::3] = -v[::3]
    assert (v != 0).all()
    return v


def row_case(M: int, C: int, seed: int, *, y_bf16: bool = False, skip: bool = False, add: bool = False,
             accum: bool = False, g_add_dtype=None) -> Dict:
    """Inputs of the [M, C] row kernels.  The first column of the skip / residual target is moved away from zero, so
    no row norm comes near it (the kernels have no epsilon there)."""
    y = gauss_data((M, C), seed + 1) * 0.3
    xs = gauss_data((M, C), seed + 3)
    xs[:, 0] += 3.0
    d = {"h": gauss_data((M, C), seed), "y": y.bfloat16() if y_bf16 else y,
         "alpha": signed(gauss_data((C,), seed + 2) * 0.01 + 1 / 32), "c_a": 0.05 * 32,
         "skip_x": xs if skip else None, "skip": torch.tensor([0.9]) if skip else None,
         "x": xs, "skip1": torch.tensor([0.9]),
         "w": gauss_data((C,), seed + 6) * 0.2 + 1.0, "eps": 1e-6,
         "dout": gauss_data((M, C), seed + 4),
         "dout_add": (gauss_data((M, C), seed + 5) * 0.5).bfloat16() if add else None,
         "old": gauss_data((M, C), seed + 7) if accum else None}
    if add and g_add_dtype is not None:
        d["dout_add"] = (gauss_data((M, C), seed + 5) * 0.5).to(g_add_dtype)
    for t in (d["h"], y, xs):
        assert t.norm(dim=-1).min() > 0.05
    return d


def qk_case(B: int, T: int, H: int, d: int, seed: int, in_dtype=F32T) -> Dict:
    M, C = B * T, H * d
    mk = lambda s: gauss_data((M, C), s).to(in_dtype)
    return {"q": mk(seed), "k": mk(seed + 1), "v": mk(seed + 2),
            "sqk": signed(gauss_data((C,), seed + 3) * 0.003 + 1 / 32), "c_q": 32.0, "B": B, "T": T, "H": H, "d": d,
            "gq": gauss_data((B, H, T, d), seed + 4), "gk": gauss_data((B, H, T, d), seed + 5),
            "gv": gauss_data((B, H, T, d), seed + 6)}


def interleave(x: torch.Tensor, F: int) -> torch.Tensor:
    """natural [.., 2F] (u | v) -> the layout of the GEMM shadow: blocks of 16 u, 16 v"""
    u, v = x[..., :F], x[..., F:]
    sh = x.shape[:-1]
    return torch.stack([u.reshape(*sh, F // 16, 16), v.reshape(*sh, F // 16, 16)], dim=-2).reshape(*sh, 2 * F)


def deinterleave(x: torch.Tensor, F: int) -> torch.Tensor:
    sh = x.shape[:-1]
    b = x.reshape(*sh, F // 16, 2, 16)
    return torch.cat([b[..., 0, :].reshape(*sh, F), b[..., 1, :].reshape(*sh, F)], dim=-1)


def swiglu_case(M: int, F: int, seed: int, use_suv: bool, dtype=F32T) -> Dict:
    """uv, dx in natural (u | v) order; the kernel takes interleave(uv) and returns interleave(duv)."""
    return {"uv": (gauss_data((M, 2 * F), seed) * 1.5).to(dtype),
            "suv": gauss_data((2 * F,), seed + 1) * 0.1 + 1.0 if use_suv else None,
            "gscale": 3.0 if use_suv else 1.0, "dx": gauss_data((M, F), seed + 2).to(dtype)}


# ------------------------------------------------------------------------------------------------ LERP (+ norm_skip)
def lerp_eval(d: Dict, dtype=F64) -> Dict[str, torch.Tensor]:
    """out = nrm(a + |alpha c_a| (b - a)), a = nrm(h), b = nrm(y); with skip: nrm(out * skip + skip_x).  Gradients for
    the upstream dout (+ dout_add), dh (+ old).  alpha and skip are given one copy per row, so their gradient rows are
    the per-row terms of the column sums (`dalpha_rows`, `dskip_rows`)."""
    M, C = d["h"].shape
    h, y, al = _leaf(d["h"], dtype), _leaf(d["y"], dtype), _leaf(d["alpha"].expand(M, C), dtype)
    out = O.lerp(h, y, al, d["c_a"])
    leaves = [h, y, al]
    if d["skip_x"] is not None:
        xs, sk = _leaf(d["skip_x"], dtype), _leaf(d["skip"].expand(M, 1), dtype)
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


def lerp_formula(d: Dict, dtype) -> Dict:
    """`dlam_rows`: the per-row terms of d|alpha c_a| (the column partials); dalpha = sum * c_a * sign(alpha c_a)."""
    h, y, alpha, xs, skip, g, add, old = (_as(d[k], dtype) for k in
                                          ("h", "y", "alpha", "skip_x", "skip", "dout", "dout_add", "old"))
    c_a = d["c_a"]
    lam = _abs(alpha * c_a)
    a, rsx = _nrm(h)
    b, rsy = _nrm(y)
    o, rsr = _nrm(a + lam * (b - a))
    res = {"out": o}
    if xs is not None:
        t, rst = _nrm(o * skip + xs)
        res["out"] = t
    if g is None:
        return res
    if add is not None:
        g = g + add
    if xs is not None:
        dt_ = (g - t * _sum(t * g)) * rst
        res["dskip_x"] = dt_
        res["dskip_rows"] = _sum(dt_ * o)
        res["dskip"] = _flat(_sum(res["dskip_rows"], 0))
        g = dt_ * skip
    dr = (g - o * _sum(o * g)) * rsr
    res["dlam_rows"] = dr * (b - a)
    sign = torch.sign(d["alpha"].double() * c_a)
    res["dalpha"] = _flat(_sum(res["dlam_rows"], 0) * c_a) * (Ev(sign) if dtype == "ev" else sign.to(dtype))
    db = lam * dr
    dh = ((dr - db) - a * _sum(a * (dr - db))) * rsx
    res["dh"] = dh if old is None else dh + old
    res["dy"] = (db - b * _sum(b * db)) * rsy
    return res


LERP_OUT = ("out", "dh", "dy", "dskip_x", "dalpha", "dskip")


def _pick(res: Dict, keys) -> Dict:
    return {k: res[k] for k in keys if k in res}


def lerp_bounds(d: Dict):
    """(values, bounds) of the Ev run; the values are the reference restated (the CPU test compares them)."""
    return _split(_pick(lerp_formula(d, "ev"), LERP_OUT))


# ------------------------------------------------------------------------------------------------ stand-alone norm_skip
def norm_skip_eval(d: Dict, dtype=F64, tgt: bool = True) -> Dict[str, torch.Tensor]:
    """out = nrm(src * skip + tgt) (tgt None: nrm(src * skip)); src = d["h"], tgt = d["x"], skip = d["skip1"]."""
    M, C = d["h"].shape
    src, sk = _leaf(d["h"], dtype), _leaf(d["skip1"].expand(M, 1), dtype)
    leaves = [src, sk]
    t = src * sk
    if tgt:
        x = _leaf(d["x"], dtype)
        t = t + x
        leaves.append(x)
    out = O.nrm(t)
    gr = torch.autograd.grad(out, leaves, d["dout"].to(dtype))
    res = {"out": out.detach(), "dsrc": gr[0], "dskip_rows": gr[1], "dskip": gr[1].sum().reshape(1)}
    if tgt:
        res["dtgt"] = gr[2]
    return res


def norm_skip_formula(d: Dict, dtype, tgt: bool = True) -> Dict:
    src, x, skip, g = (_as(d[k], dtype) for k in ("h", "x", "skip1", "dout"))
    o, rs = _nrm(src * skip + x if tgt else src * skip)
    dt_ = (g - o * _sum(o * g)) * rs
    res = {"out": o, "dsrc": dt_ * skip, "dskip_rows": _sum(dt_ * src)}
    res["dskip"] = _flat(_sum(res["dskip_rows"], 0))
    if tgt:
        res["dtgt"] = dt_
    return res


NORM_SKIP_OUT = ("out", "dsrc", "dtgt", "dskip")


def norm_skip_bounds(d: Dict, tgt: bool = True):
    return _split(_pick(norm_skip_formula(d, "ev", tgt), NORM_SKIP_OUT))


# ------------------------------------------------------------------------------------------------ (residual +) RMSNorm
def res_rmsnorm_eval(d: Dict, dtype=F64, with_y: bool = True) -> Dict[str, torch.Tensor]:
    """out = z * rsqrt(mean(z^2) + eps) * w, z = a + y (with_y False: z = a: plain RMSNorm); a = d["h"].  Gradients
    for the upstream dout (+ dout_add), dz (+ old); w has one copy per row (`dw_rows`)."""
    M, C = d["h"].shape
    a, w = _leaf(d["h"], dtype), _leaf(d["w"].expand(M, C), dtype)
    z = a + d["y"].to(dtype) if with_y else a
    rstd = torch.rsqrt((z * z).mean(dim=-1, keepdim=True) + d["eps"])
    out = z * rstd * w
    g = d["dout"].to(dtype)
    if d["dout_add"] is not None:
        g = g + d["dout_add"].to(dtype)
    gr = torch.autograd.grad(out, [a, w], g)
    return {"out": out.detach(), "rstd": rstd.detach().reshape(M),
            "dz": gr[0] if d["old"] is None else gr[0] + d["old"].to(dtype), "dw_rows": gr[1], "dw": gr[1].sum(0)}


def res_rmsnorm_formula(d: Dict, dtype, with_y: bool = True) -> Dict:
    a, y, w, g, add, old = (_as(d[k], dtype) for k in ("h", "y", "w", "dout", "dout_add", "old"))
    C = d["h"].shape[1]
    z = a + y if with_y else a
    rs = _rsqrt(_divc(_sum(z * z), C) + d["eps"])
    res = {"out": z * rs * w, "rstd": _flat(rs)}
    if add is not None:
        g = g + add
    zn = z * rs
    res["dw_rows"] = g * zn
    res["dw"] = _flat(_sum(res["dw_rows"], 0))
    gw = g * w
    dz = (gw - zn * _divc(_sum(gw * zn), C)) * rs
    res["dz"] = dz if old is None else dz + old
    return res


RMS_OUT = ("out", "rstd", "dz", "dw")


def res_rmsnorm_bounds(d: Dict, with_y: bool = True):
    return _split(_pick(res_rmsnorm_formula(d, "ev", with_y), RMS_OUT))


# ------------------------------------------------------------------------------------------------ residual + norm_skip
def res_skip_eval(d: Dict, dtype=F64) -> Dict[str, torch.Tensor]:
    """out = nrm((h + y) * skip + x); dh = d(h + y)."""
    M, C = d["h"].shape
    s, x = _leaf(d["h"].to(dtype) + d["y"].to(dtype), dtype), _leaf(d["x"], dtype)
    sk = _leaf(d["skip1"].expand(M, 1), dtype)
    out = O.nrm(s * sk + x)
    gr = torch.autograd.grad(out, [s, x, sk], d["dout"].to(dtype))
    return {"out": out.detach(), "dh": gr[0], "dx": gr[1], "dskip_rows": gr[2], "dskip": gr[2].sum().reshape(1)}


def res_skip_formula(d: Dict, dtype) -> Dict:
    h, y, x, skip, g = (_as(d[k], dtype) for k in ("h", "y", "x", "skip1", "dout"))
    s = h + y
    o, rs = _nrm(s * skip + x)
    dr = (g - o * _sum(o * g)) * rs
    res = {"out": o, "dx": dr, "dh": dr * skip, "dskip_rows": _sum(dr * s)}
    res["dskip"] = _flat(_sum(res["dskip_rows"], 0))
    return res


RES_SKIP_OUT = ("out", "dh", "dx", "dskip")


def res_skip_bounds(d: Dict):
    return _split(_pick(res_skip_formula(d, "ev"), RES_SKIP_OUT))


# ------------------------------------------------------------------------------------------------ q/k normalise
def to_heads(x, B: int, T: int, H: int, d: int):
    """[M, C] -> [B, H, T, d]"""
    return _view(x, lambda t: O.heads(t.reshape(B, T, H * d), H))


def from_heads(x, B: int, T: int, H: int, d: int):
    """[B, H, T, d] -> [M, C]"""
    return _view(x, lambda t: t.permute(0, 2, 1, 3).reshape(B * T, H * d))


def qknorm_eval(c: Dict, dtype=F64, group: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """qh = s * nrm(heads(q)), kh likewise, s = sqk * c_q per head column; rq, rk [M, H] = 1 / |head|; vh = heads(v).
    Gradients of sum(qh gq + kh gk + vh gv); sqk has one copy per row (`dsqk_rows`).
    group: the width of the normalised groups when it is not the head dim (the mutants of the CPU test)."""
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    M, C = B * T, H * d
    q, k, v, sq = _leaf(c["q"], dtype), _leaf(c["k"], dtype), _leaf(c["v"], dtype), _leaf(c["sqk"].expand(M, C), dtype)
    gw = group or d
    s = O.heads((sq * c["c_q"]).reshape(B, T, C), H)
    Cp = -(-C // gw) * gw       # (a group wider than what is left of the row sees zeros there, as masked lanes do)

    def unit(x):
        xp = torch.nn.functional.pad(x, (0, Cp - C)).reshape(B, T, Cp // gw, gw)
        return O.heads(O.nrm(xp).reshape(B, T, Cp)[..., :C], H)

    qh, kh, vh = s * unit(q), s * unit(k), O.heads(v.reshape(B, T, C), H)
    inv = lambda x: 1.0 / torch.sqrt((x.reshape(M, H, d) ** 2).sum(-1))
    gq, gk, gv = (c[n].to(dtype) for n in ("gq", "gk", "gv"))
    gr = torch.autograd.grad((qh * gq + kh * gk + vh * gv).sum(), [q, k, v, sq])
    return {"qh": qh.detach(), "kh": kh.detach(), "vh": vh.detach(), "rq": inv(q).detach(), "rk": inv(k).detach(),
            "dq": gr[0], "dk": gr[1], "dv": gr[2], "dsqk_rows": gr[3], "dsqk": gr[3].sum(0)}


def qknorm_fwd_formula(c: Dict, dtype) -> Dict:
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    M, C = B * T, H * d
    s = _as(c["sqk"], dtype) * c["c_q"]

    def one(x):
        xh = _view(_as(x, dtype), lambda t: t.reshape(M, H, d))
        r = _rsqrt(_sum(xh * xh))
        return to_heads(_view(xh * r, lambda t: t.reshape(M, C)) * s, B, T, H, d), _view(r, lambda t: t.reshape(M, H))

    qh, rq = one(c["q"])
    kh, rk = one(c["k"])
    return {"qh": qh, "kh": kh, "rq": rq, "rk": rk}


def qknorm_bwd_formula(c: Dict, fwd: Dict, dtype) -> Dict:
    """The backward from the tensors a kernel is handed (`fwd`: qh, kh [B, H, T, d], rq, rk [M, H]): the unit vector is
    qh / s, ds = gq . unit, dq = (s gq - unit <s gq, unit>) * rq per head; dsqk = (column sums of ds) * c_q."""
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    M, C = B * T, H * d
    s = _as(c["sqk"], dtype) * c["c_q"]
    sinv = _recip(s)
    res, ds = {}, None
    for n in ("q", "k"):
        g = from_heads(_as(c["g" + n], dtype), B, T, H, d)
        u = from_heads(_as(fwd[n + "h"], dtype), B, T, H, d) * sinv
        r = _view(_as(fwd["r" + n], dtype), lambda t: t.reshape(M, H, 1))
        ds = g * u if ds is None else ds + g * u
        sg = g * s
        hv = lambda x: _view(x, lambda t: t.reshape(M, H, d))
        dot = _sum(hv(sg * u))
        res["d" + n] = _view((hv(sg) - hv(u) * dot) * r, lambda t: t.reshape(M, C))
    res["dsqk_rows"] = ds
    res["dsqk"] = _flat(_sum(ds, 0)) * c["c_q"]
    return res


def qknorm_bounds(c: Dict, fwd_given: Optional[Dict] = None):
    """(values, bounds).  fwd_given None: forward and backward chained, the forward's error passed on into the backward
    (against autograd of the fp64 forward).  Otherwise the backward alone from those tensors taken as exact."""
    if fwd_given is None:
        fwd = qknorm_fwd_formula(c, "ev")
        res = dict(fwd)
        res.update(_pick(qknorm_bwd_formula(c, fwd, "ev"), ("dq", "dk", "dsqk")))
    else:
        res = _pick(qknorm_bwd_formula(c, fwd_given, "ev"), ("dq", "dk", "dsqk"))
    return _split(res)


# ------------------------------------------------------------------------------------------------ SwiGLU
def swiglu_eval(c: Dict, dtype=F64, dv_mutant: bool = False) -> Dict[str, torch.Tensor]:
    """x = u * silu(v), (u | v) = uv * suv * gscale (natural column order); gradients for upstream dx; suv has one copy
    per row (`dsuv_rows`).  dv_mutant: the gradient of silu without its v (1 - sigmoid) term (CPU test)."""
    M, F2 = c["uv"].shape
    F = F2 // 2
    uv = _leaf(c["uv"], dtype)
    leaves = [uv]
    z = uv
    if c["suv"] is not None:
        su = _leaf(c["suv"].expand(M, F2), dtype)
        z = uv * (su * c["gscale"])
        leaves.append(su)
    u, v = z[:, :F], z[:, F:]
    sg = torch.sigmoid(v)
    act = v * (sg.detach() if dv_mutant else sg)
    x = u * act
    gr = torch.autograd.grad(x, leaves, c["dx"].to(dtype))
    res = {"x": x.detach(), "duv": gr[0]}
    if c["suv"] is not None:
        res.update(dsuv_rows=gr[1], dsuv=gr[1].sum(0))
    return res


def swiglu_formula(c: Dict, dtype) -> Dict:
    uv, suv, g = (_as(c[k], dtype) for k in ("uv", "suv", "dx"))
    F = c["uv"].shape[1] // 2
    cols = lambda x, lo: _view(x, lambda t: t[..., lo:lo + F])
    ur, vr = cols(uv, 0), cols(uv, F)
    if suv is not None:
        gu, gv = cols(suv, 0) * c["gscale"], cols(suv, F) * c["gscale"]
        u, v = ur * gu, vr * gv
    else:
        u, v = ur, vr
    sg = _recip(1.0 + _exp(-v))
    res = {"x": u * (v * sg)}
    du = g * v * sg
    dv = g * u * sg * (1.0 + v * (1.0 - sg))
    if suv is not None:
        res["dsuv_rows"] = _cat([du * ur, dv * vr])
        res["dsuv"] = _flat(_sum(res["dsuv_rows"], 0)) * c["gscale"]
        du, dv = du * gu, dv * gv
    res["duv"] = _cat([du, dv])
    return res


def swiglu_bounds(c: Dict):
    return _split(_pick(swiglu_formula(c, "ev"), ("x", "duv", "dsuv")))


# ------------------------------------------------------------------------------------------------ column partials
def wave_visits(M: int, nblk: int) -> List[List[int]]:
    """the rows each of the 4 * nblk waves walks: wave g starts at row g and strides by the wave count"""
    S = 4 * nblk
    return [list(range(g, M, S)) for g in range(S)]


def wave_partials(rows: torch.Tensor, nblk: int, per_block: bool = False, visits: Optional[List[List[int]]] = None,
                  keep_last: bool = False) -> torch.Tensor:
    """The partial array a backward row kernel leaves, summed the way it sums (in `rows`' dtype): every wave adds its
    rows' terms in order ([4 * nblk, C]; a wave without a row leaves zeros); per_block: the four waves of a workgroup
    are then added in order ([nblk, C]).  visits / keep_last: the mutants of the CPU test."""
    M = rows.shape[0]
    visits = wave_visits(M, nblk) if visits is None else visits
    part = torch.zeros((4 * nblk,) + tuple(rows.shape[1:]), dtype=rows.dtype)
    for g, ms in enumerate(visits):
        for m in ms:
            part[g] = rows[m] if keep_last else part[g] + rows[m]
    if per_block:
        p4 = part.reshape(nblk, 4, *rows.shape[1:])
        part = ((p4[:, 0] + p4[:, 1]) + p4[:, 2]) + p4[:, 3]
    return part


def kind2_dst(N: int) -> torch.Tensor:
    """destination of column n for kind 2: the interleaved (16 u | 16 v) columns back to natural (u | v) order"""
    n = torch.arange(N)
    q, w = n // 32, n % 32
    return torch.where(w < 16, q * 16 + w, N // 2 + q * 16 + (w - 16))


def csr_eval(part, kind: int = 0, ref=None, scale: float = 1.0, old=None, part_b=None, dtype=F64,
             mutant: Optional[str] = None) -> torch.Tensor:
    """out[dst(n)] = (old +) f * sum_b part[b, n] (+ f * sum_b part_b[b, n]); f = scale (kinds 0, 2) or
    scale * sign(ref * scale) (kind 1); dst = kind2_dst for kind 2.  mutant: "sign", "dst", "accumulate", "part_b"."""
    p2 = lambda t: t.reshape(t.shape[0], -1).to(dtype)
    s = p2(part).sum(0)
    N = s.numel()
    f = torch.full((N,), scale, dtype=dtype)
    if kind == 1 and mutant != "sign":
        f = f * torch.sign(ref.to(dtype) * scale)

    def place(t):
        if kind != 2 or mutant == "dst":
            return t
        res = torch.empty_like(t)
        res[kind2_dst(N)] = t
        return res

    out = place(s * f)
    if old is not None and mutant != "accumulate":
        out = old.to(dtype).reshape(-1) + out
    if part_b is not None and mutant != "part_b":
        out = out + place(p2(part_b).sum(0) * f)
    return out


def csr_bound(part, kind: int = 0, scale: float = 1.0, old=None, part_b=None) -> torch.Tensor:
    """each array: the sum over its rows (red) and the scale (its fp32 rounding and the mul); then one add each for the
    old value and the second array."""
    p2 = lambda t: t.reshape(t.shape[0], -1).double()
    a = p2(part)
    N = a.shape[1]
    sa = abs(scale)
    b = sa * (red(a.shape[0], a.abs().sum(0)) + 2 * U32 * a.sum(0).abs())
    tot = (a.sum(0) * sa).abs()
    if part_b is not None:
        pb = p2(part_b)
        b = b + sa * (red(pb.shape[0], pb.abs().sum(0)) + 2 * U32 * pb.sum(0).abs())
        tot = tot + (pb.sum(0) * sa).abs()
    if old is not None:
        o = old.double().reshape(-1).abs()
        tot = tot + (o[kind2_dst(N)] if kind == 2 else o)
    b = b + 2 * U32 * tot
    if kind == 2:
        res = torch.empty_like(b)
        res[kind2_dst(N)] = b
        b = res
    return b


def csr_int_case(nblk: int, N: int, seed: int, kind: int, accumulate: bool, nblk_b: int = 0) -> Dict:
    """small integers and a power-of-two scale: every fp32 sum is exact in any order (|sum| <= 4097 * 4 * 2 + 8)"""
    assert (nblk + nblk_b) * 4 * 2 + 8 < 2 ** 24
    return {"part": int_data((nblk, N), 4, seed), "kind": kind, "scale": -2.0 if kind == 0 else 2.0,
            "ref": signed(int_data((N,), 3, seed + 1) * 2 + 1) if kind == 1 else None,
            "old": int_data((N,), 8, seed + 2) if accumulate else None,
            "part_b": int_data((nblk_b, N), 4, seed + 3) if nblk_b else None}


def csr_gauss_case(nblk: int, N: int, seed: int, kind: int, accumulate: bool, nblk_b: int = 0) -> Dict:
    return {"part": gauss_data((nblk, N), seed), "kind": kind, "scale": 1.6,
            "ref": signed(gauss_data((N,), seed + 1) + 3.0) if kind == 1 else None,
            "old": gauss_data((N,), seed + 2) if accumulate else None,
            "part_b": gauss_data((nblk_b, N), seed + 3) if nblk_b else None}


def csr_ref(c: Dict, dtype=F64, mutant: Optional[str] = None) -> torch.Tensor:
    return csr_eval(c["part"], c["kind"], c["ref"], c["scale"], c["old"], c["part_b"], dtype, mutant)


def csr_case_bound(c: Dict) -> torch.Tensor:
    return csr_bound(c["part"], c["kind"], c["scale"], c["old"], c["part_b"])


# ------------------------------------------------------------------------------------------------ checks
U64 = 2.0 ** -53        # unit roundoff of fp64


def close_values(vals: Dict[str, torch.Tensor], bound: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor],
                 label: str) -> None:
    """The Ev run's values are the autograd reference restated.  Both are fp64 evaluations of the same function, and
    the bound of an fp32 evaluation scales with the unit roundoff: each lies within bound * U64 / U32 of the truth."""
    for k, v in vals.items():
        r = ref[k].double().reshape(v.shape)
        tol = 2 * bound[k] * (U64 / U32)
        assert ((v - r).abs() <= tol).all(), f"{label} {k}: formula and reference differ beyond the fp64 bound"


def rounded_copy(lo: torch.Tensor, full: torch.Tensor, label: str) -> None:
    """a low-precision twin must be the fp32 output rounded once to nearest even, bit for bit"""
    assert bits_equal(lo.detach().cpu(), full.detach().cpu().to(lo.dtype)), \
        f"{label}: the low-precision copy is not the fp32 output rounded to nearest even"
