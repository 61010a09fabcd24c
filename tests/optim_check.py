"""Oracles of the optimizer and renorm kernel tests (a plain helper module; test_optim_check.py checks it on the CPU,
test_gpu_optim_bounds.py uses it against the HIP kernels of optim.hip and the renorm kernel of weights.hip).

The fused step is  clip_grad_norm_ -> torch.optim.AdamW.step -> x / ||x||  over a table of parameters:

* `adamw_eval(table, p0, steps, hyper, dtype)`: that sequence in plain torch math (the clip factor max_norm / (norm + 1e-6),
  applied only below 1; decoupled decay; bias corrections from the step count in double; then the row / column
  normalisation of the entries that have one).  float64: the reference; float32: a correct kernel.
* `adamw_bounds(table, p0, steps, hyper, exact_sum)`: the formula once over `Ev` of rowops_check.py (an fp64 value with a first-order
  bound of the error of an fp32 evaluation, rules at the top of that file).  The state (p, m, v) is carried as Ev from
  step to step, so the errors of earlier steps enter to first order; host scalars (lr, weight decay, betas, eps, the
  bias corrections) count one fp32 rounding unless they are exact.  No constant here was tuned to an output.
* `walk(case, grid, npart, dtype, mutant)`: an fp32 restatement of the two launches in the kernels' own order (workgroup
  b takes chunk / item b, b + grid, ...), item by item, without LDS; it carries the named mutants.
* `renorm_eval` / `renorm_bounds`: the stand-alone x / ||x||.

Everything lives in ONE flat vector per quantity (p, g, m, v): entry i is the slice [off, off + numel), offsets are
multiples of 4 floats (the kernels' 16-byte accesses), the pad elements are zero and stay zero (their bound is 0).

Gradient families.  "gauss": N(0, 0.02) times a per-step magnitude, one element in 16 near eps (1e-8 .. 1e-6), one in 16
exactly zero; run without clipping.  "exact": integers in [-2, 2] times one power of two per step: every partial sum of
squares is an integer below 2^24 (times the squared scale), exact in any order, so the reported norm must be sqrtf of the
exact sum bit for bit and the clip factor carries the roundings of sqrtf, one add and one division only.  Clipping is
tested with this family alone: with Gaussian gradients the summation bound of the norm would flow into every update.
"""
from __future__ import annotations

import bisect
import math
import types
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from nvit_amd import _lib
from rowops_check import LIB, U32, Ev, check, check_all, red  # noqa: F401  (check_all: for the tests)

F64 = torch.float64
F32T = torch.float32

CHUNK = _lib.const("OPT_CHUNK")
ROWS_PER_ITEM = _lib.const("OPT_ROWS_PER_ITEM")
SLAB_COLS = _lib.const("OPT_SLAB_COLS")
SLAB_ROWS = _lib.const("OPT_SLAB_ROWS")
TALL_COLS = _lib.const("OPT_TALL_COLS")
TALL_ROWS = _lib.const("OPT_TALL_ROWS")
ROW_COLS = _lib.const("OPT_ROW_COLS")
WIDE_COLS = _lib.const("OPT_WIDE_COLS")
OPT_GRID = _lib.const("OPT_MAX_GRID")
NPART = 1024                                  # optim._NPART (test_optim_check asserts it)
R_ROWS = _lib.const("RENORM_ROWS_PER_ITEM")
R_COLS = _lib.const("RENORM_COLS_PER_ITEM")
R_TALL_ROWS = _lib.const("RENORM_TALL_ROWS")
R_TALL_COLS = _lib.const("RENORM_TALL_COLS_PER_ITEM")
R_MAX_ROWS = _lib.const("RENORM_MAX_ROWS_DIM0")
R_GRID = _lib.const("RENORM_MAX_GRID")
MAX_EMBD = _lib.const("MAX_EMBD")


# ------------------------------------------------------------------------------------------------ moved helper
def _fake_model(rows, cols):
    """The renorm map step_fused builds from ViT blocks, for hand-made matrices: blocks of 4 row-normalised + 2
    column-normalised slots, padded with repeats."""
    W = lambda p: types.SimpleNamespace(weight=p)
    blocks = []
    for i in range(max(len(rows), len(cols), 1)):
        r, c = rows[i % len(rows)], cols[i % len(cols)]
        blocks.append(types.SimpleNamespace(query=W(r), key=W(r), value=W(r), c_fc=W(r), att_c_proj=W(c),
                                            mlp_c_proj=W(c)))
    return types.SimpleNamespace(config=types.SimpleNamespace(use_nvit=True),
                                 transformer=types.SimpleNamespace(h=blocks))


# ------------------------------------------------------------------------------------------------ tables
class Entry:
    __slots__ = ("kind", "shape", "rows", "cols", "numel", "group", "off", "items", "chunks", "first_item",
                 "first_chunk")


class Table:
    """entries in table order (param group by param group, as FusedAdamW._table walks them) and their flat layout"""

    def __init__(self, specs):
        self.entries: List[Entry] = []
        off = item = chunk = 0
        assert [g for _, _, g in specs] == sorted(g for _, _, g in specs), "table order is group order"
        for kind, shape, group in specs:
            e = Entry()
            e.kind, e.shape, e.group = kind, tuple(shape), group
            e.numel = math.prod(shape)
            e.rows, e.cols = (shape if kind >= 0 else (1, e.numel))
            assert kind < 0 or len(shape) == 2
            e.chunks = -(-e.numel // CHUNK)
            if kind == 1:
                assert e.cols % 4 == 0 and e.cols <= WIDE_COLS
                e.items = -(-e.rows // ROWS_PER_ITEM)
            elif kind == 0:
                assert e.rows <= TALL_ROWS
                e.items = -(-e.cols // slab_cols(e.rows))
            else:
                e.items = e.chunks
            e.off, e.first_item, e.first_chunk = off, item, chunk
            off += -(-e.numel // 4) * 4
            item += e.items
            chunk += e.chunks
            self.entries.append(e)
        self.total, self.items, self.chunks = off, item, chunk
        self.n_elems = sum(e.numel for e in self.entries)
        self._fi = [e.first_item for e in self.entries]
        self._fc = [e.first_chunk for e in self.entries]
        self.grid = min(self.items, OPT_GRID)

    def of_item(self, item: int) -> Entry:
        return self.entries[bisect.bisect_right(self._fi, item) - 1]

    def of_chunk(self, chunk: int) -> Entry:
        return self.entries[bisect.bisect_right(self._fc, chunk) - 1]

    def view(self, flat, e: Entry):
        """entry e of a flat torch / numpy vector as [rows, cols]"""
        return flat[e.off:e.off + e.numel].reshape(e.rows, e.cols)

    def per_element(self, values):
        """values[group] spread over the flat vector (pads: group of the entry before them)"""
        out = torch.zeros(self.total, dtype=F64)
        for e in self.entries:
            out[e.off:e.off + -(-e.numel // 4) * 4] = values[e.group]
        return out

    def mask(self):
        m = torch.zeros(self.total, dtype=torch.bool)
        for e in self.entries:
            m[e.off:e.off + e.numel] = True
        return m


def slab_cols(rows: int) -> int:
    return SLAB_COLS if rows <= SLAB_ROWS else TALL_COLS


def item_class(e: Entry) -> str:
    if e.kind < 0:
        return "plain"
    if e.kind == 1:
        return "reg_row" if e.cols <= ROW_COLS else "wide_row"
    return "slab32" if e.rows <= SLAB_ROWS else "slab16"


def item_region(e: Entry, local: int):
    """what item `local` of entry e covers: (axis, lo, hi): axis None = flat elements, 0 = rows, 1 = columns"""
    if e.kind < 0:
        return None, local * CHUNK, min((local + 1) * CHUNK, e.numel)
    if e.kind == 1:
        return 0, local * ROWS_PER_ITEM, min((local + 1) * ROWS_PER_ITEM, e.rows)
    sc = slab_cols(e.rows)
    return 1, local * sc, min((local + 1) * sc, e.cols)


def coverage(t: Table):
    """(times each flat element is covered by the update items, by the norm chunks)"""
    items, chunks = np.zeros(t.total, np.int32), np.zeros(t.total, np.int32)
    for it in range(t.items):
        e = t.of_item(it)
        axis, lo, hi = item_region(e, it - e.first_item)
        assert hi > lo
        v = t.view(items, e)
        if axis is None:
            v[0, lo:hi] += 1
        elif axis == 0:
            v[lo:hi] += 1
        else:
            v[:, lo:hi] += 1
    for ch in range(t.chunks):
        e = t.of_chunk(ch)
        lo = (ch - e.first_chunk) * CHUNK
        assert lo < e.numel
        chunks[e.off + lo:e.off + min(lo + CHUNK, e.numel)] += 1
    return items, chunks


def handoffs(t: Table, grid: int):
    """{(class of item i, class of item i + grid)}: what some workgroup takes one after the other"""
    return {(item_class(t.of_item(i)), item_class(t.of_item(i + grid))) for i in range(t.items - grid)}


def _groups3(specs2):
    """(kind, shape) in table order -> thirds of the list as param groups 0, 1, 2"""
    n = len(specs2)
    return [(k, s, min(2, 3 * i // n)) for i, (k, s) in enumerate(specs2)]


def _edges_specs():
    rows = [(1, 4), (16, 4), (17, 252), (2, 256), (17, 260), (33, 1536), (5, 1540), (18, 2048)]
    cols = [(1, 1), (1, 33), (7, 32), (127, 31), (129, 35), (1152, 37), (1153, 16), (1153, 17), (2048, 33)]
    plain = [(1,), (3,), (4,), (8192,), (8193,), (8195,), (16396,), (2, 3, 5, 7)]
    # dealt round robin, so that every kind lands in each of the three groups
    mixed = []
    for i in range(max(len(rows), len(cols), len(plain))):
        mixed += [(1, rows[i])] if i < len(rows) else []
        mixed += [(0, cols[i])] if i < len(cols) else []
        mixed += [(-1, plain[i])] if i < len(plain) else []
    return _groups3(mixed)


def _plain_run(n: int, start: int = 0):
    return [(-1, (1 + (start + i) % 9,)) for i in range(n)]


def _sweep_specs():
    """Two full sweeps of the update grid and a ragged third.  Sweep 0 opens with one item pair of each class that a
    hand-off starts from, sweep 1 opens with the classes they hand over to; the rest is small entries."""
    G = OPT_GRID
    s0 = [(1, (2 * ROWS_PER_ITEM, ROW_COLS + 4)),          # items 0, 1: wide rows            -> slab32
          (0, (SLAB_ROWS + 1, 2 * TALL_COLS)),             # items 2, 3: 16-column tall slab  -> slab32
          (0, (7, 2 * SLAB_COLS)),                         # items 4, 5: slab32               -> wide row
          (1, (2 * ROWS_PER_ITEM, 4)),                     # items 6, 7: register rows        -> slab32
          ] + _plain_run(G - 8)                            # items 8 ..: plain                -> wide row, then the rest
    s1 = [(0, (5, 4 * SLAB_COLS)),                         # items G .. G+3
          (1, (2 * ROWS_PER_ITEM, WIDE_COLS)),             # items G+4, G+5
          (0, (1, 2 * SLAB_COLS)),                         # items G+6, G+7
          (1, (2 * ROWS_PER_ITEM, ROW_COLS + 8)),          # items G+8, G+9
          (1, (ROWS_PER_ITEM * 700, 4)), (0, (1, SLAB_COLS * 700))] + _plain_run(60, 3)
    used = 10 + 700 + 700 + 60
    s1 += [(1, (ROWS_PER_ITEM * (G - used), 4))]
    s2 = [(0, (2, SLAB_COLS * 300 - 5))] + _plain_run(100, 5) + [(1, (ROWS_PER_ITEM * 200 + 5, 8))]
    return _groups3(s0 + s1 + s2)


EDGES = Table(_edges_specs())
SWEEP = Table(_sweep_specs())

for _t in (EDGES, SWEEP):
    assert 4 * _t.n_elems < 2 ** 24, "exact-sum data: the sum of squares of integers in [-2, 2] stays below 2^24"
    for _k in (-1, 0, 1):
        assert len({e.group for e in _t.entries if e.kind == _k}) >= 2, "every kind in at least two param groups"
assert EDGES.items <= OPT_GRID and EDGES.chunks <= NPART, "EDGES is a single sweep"
assert SWEEP.items > 2 * OPT_GRID and SWEEP.items % OPT_GRID != 0 and SWEEP.items < 3 * OPT_GRID
assert SWEEP.chunks > 2 * NPART and len(SWEEP.entries) > 2000
assert SWEEP.n_elems < 1 << 20
HANDOFFS = {("wide_row", "slab32"), ("slab16", "slab32"), ("slab32", "wide_row"), ("reg_row", "slab32"),
            ("plain", "wide_row")}
assert HANDOFFS <= handoffs(SWEEP, SWEEP.grid)


# ------------------------------------------------------------------------------------------------ hyperparameters, data
HYPER = {"betas": (0.9, 0.95), "eps": 1e-8,
         "groups": [{"lr": 1e-2, "weight_decay": 0.1}, {"lr": 3e-3, "weight_decay": 0.0},
                    {"lr": 2e-2, "weight_decay": 0.05}],
         "lr_change": (2, 1, 5e-3)}      # before step index 2, group 1 gets this lr (through param_groups)
GAUSS_MAGS = (1.0, 2.0 ** -7, 8.0)
EXACT_STEPS = ((2.0 ** -6, 1.0), (2.0 ** -12, 1.0), (2.0 ** -20, 1e-4))    # (scale of the integers, max_norm)
NSTEPS = 3


def group_hyper(hyper, si: int):
    """[(lr, weight_decay)] per group at step index si"""
    out = [(g["lr"], g["weight_decay"]) for g in hyper["groups"]]
    at, gi, lr = hyper["lr_change"]
    if si >= at:
        out[gi] = (lr, out[gi][1])
    return out


class Case:
    """table, p0 (flat fp32), steps = [(flat fp32 gradient, max_norm)], hyper"""

    def __init__(self, name: str, table: Table, family: str, seed: int):
        self.name, self.table, self.family, self.hyper = name, table, family, HYPER
        gen = torch.Generator().manual_seed(seed)
        mask = table.mask()
        n = table.total
        self.p0 = torch.where(mask, torch.randn(n, generator=gen) * 0.05, torch.zeros(n))
        self.steps = []
        for si in range(NSTEPS):
            if family == "gauss":
                g = torch.randn(n, generator=gen) * (0.02 * GAUSS_MAGS[si])
                pick = torch.randint(0, 16, (n,), generator=gen)
                tiny = torch.pow(10.0, -8.0 + 2.0 * torch.rand(n, generator=gen, dtype=F64)).float()
                g = torch.where(pick == 0, torch.sign(g) * tiny, g)
                g = torch.where(pick == 1, torch.zeros(n), g)
                max_norm = 0.0
            else:
                scale, max_norm = EXACT_STEPS[si]
                g = torch.randint(-2, 3, (n,), generator=gen).float() * scale
            self.steps.append((torch.where(mask, g, torch.zeros(n)), max_norm))
        if family == "exact":
            c = [mn / (exact_norm(g) + 1e-6) for g, mn in self.steps]
            assert c[0] < 0.5 and c[1] > 2.0 and c[2] < 0.5, "a clipped step, an unclipped one, a clipped tiny one"
            assert 1e-6 / exact_norm(self.steps[2][0]) > 1e-4, "the 1e-6 of the denominator is visible"


def exact_sumsq(g: torch.Tensor) -> float:
    s = float((g.double() ** 2).sum())
    assert float(np.float32(s)) == s, "the sum of squares is not exact in fp32"
    return s


def exact_norm(g: torch.Tensor) -> float:
    """sqrtf of the exact sum: what the kernel must report, bit for bit"""
    return float(np.sqrt(np.float32(exact_sumsq(g))))


_CASES: Dict[str, Case] = {}
CASE_DEFS = {"edges_gauss": (EDGES, "gauss", 11), "edges_exact": (EDGES, "exact", 12), "sweep": (SWEEP, "exact", 13)}


def case(name: str) -> Case:
    if name not in _CASES:
        _CASES[name] = Case(name, *CASE_DEFS[name])
    return _CASES[name]


# ------------------------------------------------------------------------------------------------ reference
def adamw_eval(table: Table, p0: torch.Tensor, steps, hyper, dtype=F64) -> List[Dict]:
    """[{p, m, v (flat, dtype), norm}] after every step"""
    b1, b2 = hyper["betas"]
    eps = hyper["eps"]
    p = p0.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for si, (g32, max_norm) in enumerate(steps):
        t = si + 1
        g = g32.to(dtype)
        norm = None
        if max_norm > 0:
            norm = (g * g).sum().sqrt()
            c = max_norm / (norm + 1e-6)
            if c < 1:
                g = g * c
        gh = group_hyper(hyper, si)
        lr = table.per_element([h[0] for h in gh]).to(dtype)
        wd = table.per_element([h[1] for h in gh]).to(dtype)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p * (1 - lr * wd)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        denom = v.sqrt() / math.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
        for e in table.entries:
            if e.kind >= 0:
                x = table.view(p, e)
                x.copy_(x / x.norm(dim=e.kind, keepdim=True))
        out.append({"p": p.clone(), "m": m.clone(), "v": v.clone(), "norm": norm})
    return out


def renorm_eval(w: torch.Tensor, dim: int, dtype=F64) -> torch.Tensor:
    x = w.to(dtype)
    return x / x.norm(dim=dim, keepdim=True)


# ------------------------------------------------------------------------------------------------ bounds
def _sqrt(x: Ev) -> Ev:
    """sqrtf: |sqrt(x + d) - sqrt(x)| = |d| / (sqrt(x + d) + sqrt(x)) (first order d / (2 sqrt x), and finite at
    x = 0, where the error is 0 as well), + LIB roundings"""
    v = torch.sqrt(x.v)
    den = v + torch.sqrt((x.v - x.e).clamp_min(0.0))
    carried = torch.where(x.e > 0, x.e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(v))
    carried = torch.where((x.e > 0) & (den == 0), torch.sqrt(x.e), carried)
    return Ev(v, carried + LIB * U32 * v)


def _div(a: Ev, b: Ev) -> Ev:
    v = a.v / b.v
    return Ev(v, a.e / b.v.abs() + v.abs() * b.e / b.v.abs() + LIB * U32 * v.abs())


def _sumall(x: Ev, n: int) -> Ev:
    return Ev(x.v.sum(), x.e.sum() + red(n, x.v.abs().sum()))


def _per_element(table: Table, vals) -> Ev:
    lifted = [Ev.lift(float(x)) for x in vals]
    return Ev(table.per_element([float(l.v) for l in lifted]), table.per_element([float(l.e) for l in lifted]))


def _normalise(x: Ev, dim: int) -> Ev:
    sq = x * x
    n = x.v.shape[dim]
    ss = Ev(sq.v.sum(dim, keepdim=True), sq.e.sum(dim, keepdim=True) + red(n, sq.v.sum(dim, keepdim=True)))
    return _div(x, _sqrt(ss))


def adamw_formula(table: Table, p0: torch.Tensor, steps, hyper, exact_sum: bool) -> List[Dict[str, Ev]]:
    """The kernels' formula over Ev.  exact_sum: the sum of the squared gradients is exact (asserted), so the norm
    carries sqrtf alone; otherwise the products and the sum of n terms count."""
    b1, b2 = hyper["betas"]
    P, M, V = Ev(p0), Ev(torch.zeros_like(p0)), Ev(torch.zeros_like(p0))
    out = []
    for si, (g32, max_norm) in enumerate(steps):
        t = si + 1
        G = Ev(g32)
        norm = None
        if max_norm > 0:
            ss = Ev(torch.tensor(exact_sumsq(g32), dtype=F64)) if exact_sum else _sumall(G * G, table.n_elems)
            norm = _sqrt(ss)
            c = _div(Ev.lift(float(max_norm)), norm + 1e-6)
            assert abs(float(c.v) - 1.0) > 1e3 * float(c.e), "the clip factor is too close to 1 to say which side"
            if float(c.v) < 1.0:
                G = G * c
        gh = group_hyper(hyper, si)
        lr, wd = _per_element(table, [h[0] for h in gh]), _per_element(table, [h[1] for h in gh])
        ibc1 = Ev.lift(1.0 / (1.0 - b1 ** t))
        isb2 = Ev.lift(1.0 / math.sqrt(1.0 - b2 ** t))
        B1, B2 = Ev.lift(b1), Ev.lift(b2)
        P = P * (1.0 - lr * wd)
        M = B1 * M + (1.0 - B1) * G
        V = B2 * V + (1.0 - B2) * G * G
        denom = _sqrt(V) * isb2 + hyper["eps"]
        P = P - (lr * ibc1) * _div(M, denom)
        pv, pe = P.v.clone(), P.e.clone()
        for e in table.entries:
            if e.kind >= 0:
                o = _normalise(Ev(table.view(pv, e), table.view(pe, e)), e.kind)
                table.view(pv, e).copy_(o.v)
                table.view(pe, e).copy_(o.e)
        P = Ev(pv, pe)
        out.append({"p": P, "m": M, "v": V, "norm": norm})
    return out


def adamw_bounds(table: Table, p0, steps, hyper, exact_sum: bool):
    """(values, bounds): per step {p, m, v: flat fp64, norm: 0-d or None}"""
    res = adamw_formula(table, p0, steps, hyper, exact_sum)
    pick = lambda f: [{k: (None if r[k] is None else f(r[k])) for k in r} for r in res]
    return pick(lambda x: x.v), pick(lambda x: x.e)


def renorm_bounds(w: torch.Tensor, dim: int):
    o = _normalise(Ev(w), dim)
    return o.v, o.e


def unit_norm_bound(ref: torch.Tensor, bound: torch.Tensor, dim: int) -> torch.Tensor:
    """| ||out|| - 1 | to first order: sum_i |ref_i| * bound_i (ref has unit norm), + the roundings of measuring it in
    fp64 (negligible, not counted)"""
    return (ref.abs() * bound).sum(dim)


_ORACLE: Dict[str, Tuple] = {}


def oracle(name: str):
    """(case, fp64 reference, bounds, bounds' values) computed once per case"""
    if name not in _ORACLE:
        c = case(name)
        ref = adamw_eval(c.table, c.p0, c.steps, c.hyper, F64)
        vals, bnd = adamw_bounds(c.table, c.p0, c.steps, c.hyper, c.family == "exact")
        _ORACLE[name] = (c, ref, bnd, vals)
    return _ORACLE[name]


# ------------------------------------------------------------------------------------------------ comparison
KEYS = ("p", "m", "v")


def ratio(out, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """largest err / bound; inf where the bound is 0 and the result differs, or the result is not finite"""
    out = torch.as_tensor(out).detach().cpu().double()
    if not torch.isfinite(out).all():
        return math.inf
    err = (out - ref).abs()
    zero = bound == 0
    if (err[zero] > 0).any():
        return math.inf
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


def margins(got: List[Dict], ref: List[Dict], bnd: List[Dict]) -> Dict[str, float]:
    """largest err / bound per output over all steps (norm: against its bound, where one is reported)"""
    res = {k: max(ratio(g[k], r[k], b[k]) for g, r, b in zip(got, ref, bnd)) for k in KEYS}
    res["norm"] = max([ratio(torch.as_tensor(g["norm"]).reshape(()), r["norm"], b["norm"])
                       for g, r, b in zip(got, ref, bnd) if r["norm"] is not None] or [0.0])
    return res


def check_steps(got: List[Dict], ref: List[Dict], bnd: List[Dict], label: str) -> Dict[str, float]:
    """every element of p, m, v after every step inside its bound (rowops_check.check: finite, exact where the bound
    is 0); prints and returns the largest err / bound per output"""
    worst = {k: 0.0 for k in KEYS + ("norm",)}
    for si, (g, r, b) in enumerate(zip(got, ref, bnd)):
        for k in KEYS:
            worst[k] = max(worst[k], check(torch.as_tensor(g[k]), r[k], b[k], f"{label} step {si} {k}", verbose=False))
        if r["norm"] is not None:
            worst["norm"] = max(worst["norm"], check(torch.as_tensor(g["norm"]).reshape(()).float(), r["norm"], b["norm"],
                                                     f"{label} step {si} norm", verbose=False))
    print(f"   {label}: max err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def norms_exact(got: List[Dict], steps) -> bool:
    """the reported norm of every step is sqrtf of the exact sum of squares, bit for bit"""
    return all(np.float32(float(g["norm"])).tobytes() == np.float32(exact_norm(g32)).tobytes()
               for g, (g32, _) in zip(got, steps))


# ------------------------------------------------------------------------------------------------ restatement, mutants
MUTANTS = ("eps_inside_bias_correction", "eps_under_root", "coupled_decay", "lr_other_group", "wd_other_group",
           "clip_m_only", "clip_uncapped", "clip_no_1e6", "bias_correction_prev_step", "norm_before_update",
           "clamped_lanes_counted", "neighbour_column", "sweep_last_dropped", "partial_chunk_dropped", "item_twice")

# which cases kill which mutant: the whole matrix (test_optim_check asserts that the named cases kill and the others do
# not).  The clip mutants and the dropped chunk need clipping (the Gaussian family runs without), the dropped last sweep
# needs a second sweep.
_ALL, _CLIPPED = ("edges_gauss", "edges_exact", "sweep"), ("edges_exact", "sweep")
KILLS = {"eps_inside_bias_correction": _ALL, "eps_under_root": _ALL, "coupled_decay": _ALL, "lr_other_group": _ALL,
         "wd_other_group": _ALL, "clip_m_only": _CLIPPED, "clip_uncapped": _CLIPPED, "clip_no_1e6": _CLIPPED,
         "bias_correction_prev_step": _ALL, "norm_before_update": _ALL, "clamped_lanes_counted": _ALL,
         "neighbour_column": _ALL, "sweep_last_dropped": ("sweep",), "partial_chunk_dropped": _CLIPPED,
         "item_twice": _ALL}


def walk(c: Case, grid: Optional[int] = None, npart: int = NPART, dtype=np.float32, mutant: Optional[str] = None):
    """Both launches in the kernels' order, in `dtype` arithmetic: workgroup b of the norm kernel adds the chunks b,
    b + npart, ... into partial[b]; every workgroup of the update sums the partials to the clip factor, then workgroup b
    takes the items b, b + grid, ...  Mutants:
      eps_inside_bias_correction  (sqrt(v) + eps) / sqrt(bc2)          eps_under_root   sqrt(v + eps) / sqrt(bc2)
      coupled_decay      g += wd * p instead of p *= 1 - lr * wd       lr_ / wd_other_group   the next group's value
      clip_m_only        v from the unclipped gradient                 clip_uncapped    the factor also when it is >= 1
      clip_no_1e6        max_norm / norm                               bias_correction_prev_step   t - 1 (from step 2 on)
      norm_before_update the row / column norm of the weights as read  clamped_lanes_counted   the lanes of the register
      row path past the row's end (which load its first 4 columns) counted into its norm
      neighbour_column   column j of a slab divided by the norm of column j ^ 1
      sweep_last_dropped the items of the last sweep are left out when there is more than one sweep
      partial_chunk_dropped  the last chunk of an entry of more than one chunk is left out of the norm when it is partial
      item_twice         the first item of the second sweep (the last item of a single sweep) is processed twice"""
    assert mutant is None or mutant in MUTANTS
    t = c.table
    f = dtype
    grid = t.grid if grid is None else grid
    b1, b2, eps = f(c.hyper["betas"][0]), f(c.hyper["betas"][1]), f(c.hyper["eps"])
    one = f(1)
    p = c.p0.numpy().astype(f)
    m, v = np.zeros_like(p), np.zeros_like(p)
    ngroups = len(c.hyper["groups"])
    out = []
    for si, (g32, max_norm) in enumerate(c.steps):
        g = g32.numpy().astype(f)
        # ---- launch 1 and the head of launch 2
        clip, nrm = one, None
        if max_norm > 0:
            partial = np.zeros(npart, f)
            for b in range(min(npart, t.chunks)):
                for ch in range(b, t.chunks, npart):
                    e = t.of_chunk(ch)
                    lo = (ch - e.first_chunk) * CHUNK
                    hi = min(lo + CHUNK, e.numel)
                    if mutant == "partial_chunk_dropped" and e.chunks > 1 and hi == e.numel and hi - lo < CHUNK:
                        continue
                    x = g[e.off + lo:e.off + hi]
                    partial[b] += (x * x).sum(dtype=f)
            nrm = np.sqrt(partial.sum(dtype=f))
            cf = f(max_norm) / (nrm if mutant == "clip_no_1e6" else nrm + f(1e-6))
            clip = cf if (cf < one or mutant == "clip_uncapped") else one
        tb = si + 1
        if mutant == "bias_correction_prev_step" and tb > 1:
            tb -= 1
        ibc1 = f(1.0 / (1.0 - float(c.hyper["betas"][0]) ** tb))
        isb2 = f(1.0 / math.sqrt(1.0 - float(c.hyper["betas"][1]) ** tb))
        gh = group_hyper(c.hyper, si)

        def adam(pp, gg, mm, vv, lr, wd):
            gc = gg * clip
            gv = gg if mutant == "clip_m_only" else gc
            if mutant == "coupled_decay":
                gc = gc + wd * pp
                gv = gc
                pn = pp
            else:
                pn = pp * (one - lr * wd)
            mn = b1 * mm + (one - b1) * gc
            vn = b2 * vv + (one - b2) * gv * gv
            if mutant == "eps_inside_bias_correction":
                denom = (np.sqrt(vn) + eps) * isb2
            elif mutant == "eps_under_root":
                denom = np.sqrt(vn + eps) * isb2
            else:
                denom = np.sqrt(vn) * isb2 + eps
            return pn - (lr * ibc1) * (mn / denom), mn, vn

        def do_item(item: int):
            e = t.of_item(item)
            axis, lo, hi = item_region(e, item - e.first_item)
            lr = f(gh[(e.group + 1) % ngroups if mutant == "lr_other_group" else e.group][0])
            wd = f(gh[(e.group + 1) % ngroups if mutant == "wd_other_group" else e.group][1])
            P, G, M, V = (t.view(a, e) for a in (p, g, m, v))
            if axis is None:
                sl = (0, slice(lo, hi))
            elif axis == 0:
                sl = (slice(lo, hi), slice(None))
            else:
                sl = (slice(None), slice(lo, hi))
            old = P[sl]
            pn, mn, vn = adam(old, G[sl], M[sl], V[sl], lr, wd)
            M[sl], V[sl] = mn, vn
            if axis is not None:
                src = old if mutant == "norm_before_update" else pn
                ss = (src * src).sum(axis=1 - axis, dtype=f)
                if mutant == "clamped_lanes_counted" and axis == 0 and e.cols <= ROW_COLS:
                    extra = ((e.cols + 255) >> 8) * 64 - e.cols // 4
                    ss = ss + f(extra) * (src[:, :4] * src[:, :4]).sum(axis=1, dtype=f)
                nr = np.sqrt(ss)
                if mutant == "neighbour_column" and axis == 1:
                    j = np.arange(nr.shape[0]) ^ 1
                    nr = nr[np.where(j < nr.shape[0], j, j ^ 1)]
                pn = pn / (nr[:, None] if axis == 0 else nr[None, :])
            P[sl] = pn

        sweeps = -(-t.items // grid)
        for b in range(min(grid, t.items)):
            for item in range(b, t.items, grid):
                if mutant == "sweep_last_dropped" and sweeps > 1 and item >= (sweeps - 1) * grid:
                    continue
                do_item(item)
                if mutant == "item_twice" and item == min(grid, t.items - 1):
                    do_item(item)
        out.append({"p": torch.from_numpy(p.copy()), "m": torch.from_numpy(m.copy()), "v": torch.from_numpy(v.copy()),
                    "norm": None if nrm is None else float(nrm)})
    return out


def killed(name: str, mutant: str) -> bool:
    """the mutant exceeds 2 x a bound somewhere, or (exact-sum data) reports a norm that is not bit-exact"""
    c, ref, bnd, _ = oracle(name)
    got = walk(c, mutant=mutant)
    if c.family == "exact" and not norms_exact(got, c.steps):
        return True
    return max(margins(got, ref, bnd).values()) > 2.0


# ------------------------------------------------------------------------------------------------ stand-alone renorm
def renorm_items(rows: int, cols: int, dim: int) -> int:
    if dim == 1:
        return -(-rows // R_ROWS)
    assert rows <= R_MAX_ROWS
    return -(-cols // (R_COLS if rows <= R_TALL_ROWS else R_TALL_COLS))


def renorm_path(rows: int, cols: int, dim: int) -> str:
    if dim == 1:
        return "row_reg" if cols % 4 == 0 and cols <= MAX_EMBD else "row_scalar"
    return "panel64" if rows <= R_TALL_ROWS else "panel32"


def _renorm_sweep():
    """((rows, cols), dim) in table order: more than two sweeps of the renorm grid, the paths interleaved"""
    return [((R_ROWS * 100 + 3, 33), 1), ((1, R_COLS * 1500), 0), ((R_TALL_ROWS, 2 * R_COLS + 5), 0),
            ((R_ROWS * 1400, 4), 1), ((R_TALL_ROWS + 1, 2 * R_TALL_COLS + 3), 0), ((R_ROWS * 50 + 1, 50), 1),
            ((2, R_COLS * 900), 0), ((3, MAX_EMBD + 4), 1), ((7, R_COLS * 200), 0), ((R_ROWS * 12, 260), 1)]


RENORM_SWEEP = _renorm_sweep()
RENORM_EDGES = [(e.shape, e.kind) for e in EDGES.entries if e.kind >= 0]
RENORM_SWEEP_ITEMS = sum(renorm_items(r, c, d) for (r, c), d in RENORM_SWEEP)
assert RENORM_SWEEP_ITEMS > 2 * R_GRID
assert {renorm_path(r, c, d) for (r, c), d in RENORM_SWEEP} == {"row_reg", "row_scalar", "panel64", "panel32"}
assert {(r, c) for (r, c), d in RENORM_SWEEP if d == 1 and c in (33, 50)} and \
    {r for (r, c), d in RENORM_SWEEP if d == 0} >= {R_TALL_ROWS, R_TALL_ROWS + 1}


def renorm_data(mats, seed: int) -> List[torch.Tensor]:
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=gen) for shape, _ in mats]


_RENORM: Dict[str, Tuple] = {}


def renorm_oracle(name: str):
    """(mats, inputs, fp64 references, bounds) of "sweep" / "edges", computed once"""
    if name not in _RENORM:
        mats = RENORM_SWEEP if name == "sweep" else RENORM_EDGES
        ws = renorm_data(mats, 21 if name == "sweep" else 22)
        both = [renorm_bounds(w, d) for w, (_, d) in zip(ws, mats)]
        _RENORM[name] = (mats, ws, [renorm_eval(w, d) for w, (_, d) in zip(ws, mats)], [b for _, b in both],
                         [v for v, _ in both])
    return _RENORM[name]
